"""CPU SPECIFICATION (test infrastructure, NOT product code) of bundle adjustment under a robust loss ("The
loss"): Huber and soft L1 as iteratively reweighted Gauss-Newton on top of tests/util_bundle.py and tests/util_bundle_intr.py,
which this file builds on and does not change.  numpy only.

The rule, for a usable observation with the unweighted residual r = (ru, rv), s = ru ru + rv rv and the scale c in px, float64 in
single operations in the kernel's order, sqrt the only library call:
  trivial   rho = s, w = 1
  huber     s <= c c: rho = s, w = 1; otherwise q = sqrt(s), rho = (2 c) q - c c, w = c / q
  soft_l1   q = sqrt(1 + s / (c c)), rho = 2 s / (1 + q), w = 1 / q
sw = sqrt(w); the observation's J_c (its held columns zeroed), J_p, r and, with a border, J_theta are multiplied by sw before
anything is formed from them; everything downstream is util_bundle's and util_bundle_intr's arithmetic on the scaled values;
cost_j = 0.5 sum rho in track order.  This is the build's own published rule: parity with Ceres' loss functions is unpinned.
"""
import numpy as np

import util_bundle as ub
import util_bundle_intr as ui

TRIVIAL, HUBER, SOFT_L1 = 0, 1, 2                                    # VC_BA_LOSS_*
LOSSES = {"trivial": TRIVIAL, "huber": HUBER, "soft_l1": SOFT_L1}
# worst relative difference max|host - spec| / max|spec| of every array of the plain and of the bordered system between this
# specification and the kernels' routines compiled for the host (tools/bundle_host.cpp with the loss extension of its
# problem file) over the windowed problem, the corrupted one, the 300 random problems and the nine edge problems, Huber and soft
# L1 at 1 px and at 0.25 px, where most observations are on the outer branch (measured by tests/test_bundle_loss_spec.py, which
# prints each figure: B 1.27e-12 on a random problem and h 1.18e-12 on the windowed one under soft L1 at 0.25 px, where the two
# sums that are kept apart cancel, as without a loss; vinv 3.1e-13, dx 1.1e-13, C 8.5e-14, S 5.8e-14, the terms 2.7e-14, g 1.8e-14,
# the points 7.2e-15, the ordered sums 5.7e-15, g_p 4.1e-16, T 2.2e-16; obs_w, the costs and obs_xn are equal to the bit: what
# depends on the loss alone is written in the kernel's order).  Four times the worst is the project's margin for instruction
# selection.
HOST_SPEC_REL = 1.3e-12
TOL_REL = 4 * HOST_SPEC_REL


def loss_terms(kind, c, s):
    """s = |r|^2 of the unweighted residual -> rho(s), w = rho'(s) in the kernel's order of operations."""
    s, c = np.float64(s), np.float64(c)
    with np.errstate(all="ignore"):
        if kind == HUBER:
            if s <= c * c:
                return s, np.float64(1.0)
            q = np.sqrt(s)
            return (2.0 * c) * q - c * c, c / q
        if kind == SOFT_L1:
            q = np.sqrt(1.0 + s / (c * c))
            return 2.0 * s / (1.0 + q), 1.0 / q
    assert kind == TRIVIAL, kind
    return s, np.float64(1.0)


def linearize(cams, points, offsets, obs_cam, obs_xy, const_mask, lam, loss=TRIVIAL, loss_scale=1.0):
    """ub.linearize under the loss -> its dict, r, Jc, Jp and W scaled, and sw (total,): sqrt(w) of a usable observation, 0 of
    any other."""
    cams, points = np.asarray(cams, np.float64).reshape(-1, 16), np.asarray(points, np.float64).reshape(-1, 3)
    obs_xy = np.asarray(obs_xy, np.float64).reshape(-1, 2)
    n, total, n_cams = len(points), len(obs_xy), len(cams)
    ok, r, sw = np.zeros(total, bool), np.zeros((total, 2)), np.zeros(total)
    Jc, Jp, W = np.zeros((total, 2, 6)), np.zeros((total, 2, 3)), np.zeros((total, 6, 3))
    vinv, gp, cost, count = np.zeros((n, 3, 3)), np.zeros((n, 3)), np.zeros(n), np.zeros(n, np.int32)
    constant = np.ones(n, bool)
    valid = ub._valid_points(offsets, total)
    for j in range(n):
        if not valid[j]:
            continue
        V, c = np.zeros((3, 3)), 0.0
        for o in range(offsets[j], offsets[j + 1]):
            slot = int(obs_cam[o])
            if not 0 <= slot < n_cams:
                continue
            ok[o], r[o], Jc[o], Jp[o] = ub.observe(cams[slot], points[j], obs_xy[o], const_mask[slot])
            if not ok[o]:
                continue
            with np.errstate(all="ignore"):
                rho, w = loss_terms(loss, loss_scale, r[o, 0] * r[o, 0] + r[o, 1] * r[o, 1])
                sw[o] = np.sqrt(w)
                r[o], Jc[o], Jp[o] = sw[o] * r[o], sw[o] * Jc[o], sw[o] * Jp[o]
                W[o] = Jc[o].T @ Jp[o]
                V = V + Jp[o].T @ Jp[o]
                gp[j] = gp[j] + Jp[o].T @ r[o]
                c = c + rho
            count[j] += 1
        cost[j] = 0.5 * c
        with np.errstate(all="ignore"):
            V[np.diag_indices(3)] += lam * np.diag(V)
        inv, det = ub.adjugate_inverse(V)
        if count[j] >= 2 and np.isfinite(det) and det > 0:
            vinv[j], constant[j] = inv, False
    with np.errstate(all="ignore"):
        total_cost = float(np.cumsum(np.concatenate([[0.0], cost]))[-1])
    return dict(ok=ok, r=r, Jc=Jc, Jp=Jp, W=W, vinv=vinv, gp=gp, cost=cost, count=count, constant=constant, sw=sw, total_cost=total_cost)


def linearize_intrinsics(lin, cams, points, offsets, obs_cam, cam_group, n_groups, intr_mask):
    """ui.linearize_intrinsics on `lin` of `linearize`: J_theta (its constant columns too) is multiplied by sw; xn stays the
    unscaled (x, y)."""
    cams, points = np.asarray(cams, np.float64).reshape(-1, 16), np.asarray(points, np.float64).reshape(-1, 3)
    n, total, G = len(points), len(lin["ok"]), n_groups
    xn, Jt = np.zeros((total, 2)), np.zeros((total, 2, 4))
    T, q, hq = np.zeros((n, G, 4, 3)), np.zeros((n, G, 4, 4)), np.zeros((n, G, 4))
    valid = ub._valid_points(offsets, total)
    for j in range(n):
        if not valid[j]:
            continue
        for o in range(offsets[j], offsets[j + 1]):
            if not lin["ok"][o]:
                continue
            slot = int(obs_cam[o])
            xn[o] = ui.normalised(cams[slot], points[j])
            g = ui.group_of(cam_group, slot, G)
            if g < 0:
                continue
            Jt[o] = lin["sw"][o] * ui.jtheta(xn[o, 0], xn[o, 1], intr_mask[g])
            T[j, g] = T[j, g] + Jt[o].T @ lin["Jp"][o]
            q[j, g] = q[j, g] + Jt[o].T @ Jt[o]
            hq[j, g] = hq[j, g] + Jt[o].T @ lin["r"][o]
    TV = np.einsum("ngik,nkl->ngil", T, lin["vinv"])
    return dict(xn=xn, Jt=Jt, T=T, q=q, hq=hq, P=np.einsum("ngil,nhkl->nghik", TV, T), p=np.einsum("ngil,nl->ngi", TV, lin["gp"]))


def bundle_adjust(cams, points, offsets, obs_cam, obs_xy, const_mask, loss=TRIVIAL, loss_scale=1.0, max_iterations=ub.BA_MAX_ITERATIONS,
                  cam_group=None, intr_mask=None):
    """ub.bundle_adjust (with cam_group and intr_mask: ui.bundle_adjust) with the loss: the same loop, accept iff the candidate's
    total robust cost is finite and lower.  The report gains loss and loss_scale."""
    cams, points = np.array(cams, np.float64).reshape(-1, 16), np.array(points, np.float64).reshape(-1, 3)
    n_cams, G = len(cams), 0 if intr_mask is None else len(intr_mask)
    index = ub.camera_index(obs_cam, offsets, n_cams)
    before = ui.group_intrinsics(cams, cam_group, G) if G else None

    def lin_at(c, p, lam):
        return linearize(c, p, offsets, obs_cam, obs_xy, const_mask, lam, loss, loss_scale)

    lam = ub.BA_LAMBDA0
    lin = lin_at(cams, points, lam)
    cost = initial = lin["total_cost"]
    iterations, decisions = 1, []
    while iterations < max_iterations and len(points) and n_cams:
        S, g = ub.reduce_cameras(lin, n_cams, offsets, obs_cam, const_mask, *index, lam)
        if G:
            li = linearize_intrinsics(lin, cams, points, offsets, obs_cam, cam_group, G, intr_mask)
            B, C, h, free = ui.reduce_border(lin, li, n_cams, cam_group, G, intr_mask, offsets, obs_cam, *index, lam)
            dc, dtheta = ui.solve_bordered(S, g, B, C, h, const_mask, free)
        else:
            dc = ub.solve_cameras(S, g, const_mask)
        lower = max(lam / 10, ub.BA_LAMBDA_MIN)
        iterations += 1
        accepted = False
        if dc is not None:
            if G:
                cand_cams, cand_points, _, valid = ui.step_intrinsics(lin, li, cams, points, offsets, obs_cam, cam_group, G, intr_mask, dc, dtheta)
            else:
                cand_cams, cand_points, _ = ub.step(lin, cams, points, offsets, obs_cam, dc)
                valid = np.ones(1, bool)
            cand = lin_at(cand_cams, cand_points, lower)
            accepted = bool(valid.all() and np.isfinite(cand["total_cost"]) and cand["total_cost"] < cost)
        decisions.append(accepted)
        if accepted:
            decrease = (cost - cand["total_cost"]) / cost
            cams, points, lin, cost, lam = cand_cams, cand_points, cand, cand["total_cost"], lower
            if decrease < ub.BA_REL_DECREASE:
                break
        else:
            lam = lam * 10
            if lam > ub.BA_LAMBDA_MAX or iterations >= max_iterations:
                break
            lin = lin_at(cams, points, lam)
            iterations += 1
    report = dict(iterations=iterations, accepted_steps=int(sum(decisions)), initial_cost=initial, final_cost=cost, final_lambda=lam,
                  decisions=decisions, loss={v: k for k, v in LOSSES.items()}[loss], loss_scale=float(loss_scale))
    if G:
        report["intrinsics"] = dict(before=before, after=ui.group_intrinsics(cams, cam_group, G))
    return cams, points, report


def corrupt(obs_xy, fraction=0.05):
    """Observations displaced by 8-40 px in a random direction, from RandomState(16000) -> obs_xy, bad (the sorted indices)."""
    rs = np.random.RandomState(16000)
    total = len(obs_xy)
    bad = np.sort(rs.choice(total, int(round(fraction * total)), replace=False))
    angle = rs.uniform(0, 2 * np.pi, len(bad))
    magnitude = rs.uniform(8, 40, len(bad))
    out = np.array(obs_xy, np.float64)
    out[bad] += np.stack([magnitude * np.cos(angle), magnitude * np.sin(angle)], axis=1)
    return out, bad


def corrupted_windowed_problem(fraction=0.05):
    """The grown model of the windowed 12-view scene with `fraction` of its observations corrupted -> problem (cams, points,
    offsets, obs_cam, obs_xy, const_mask), bad."""
    from test_bundle_spec import adjusted

    _, _, _, problem, adj = adjusted()
    cams, points, offsets, obs_cam, obs_xy = problem[1:]
    obs_xy, bad = corrupt(obs_xy, fraction)
    return (cams, points, offsets, obs_cam, obs_xy, adj["held"][2]), bad
