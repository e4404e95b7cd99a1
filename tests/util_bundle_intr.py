"""CPU SPECIFICATION (test infrastructure, NOT product code) of bundle adjustment with refined intrinsics (DESIGN.md §4.2k,
"The border"): the intrinsics theta_g = (fx, fy, cx, cy) of every group of cameras as a border [[S, B], [B', C]] of the reduced
camera system of tests/util_bundle.py, which this file builds on and does not change.  numpy only.

The per-observation arithmetic is written in the kernel's order of single float64 operations; the accumulations are written
independently of csrc/bundle.hip (whole blocks through numpy's matrix products, the ordered sums through cumsum), in the
order the rule gives.  This is the build's own published rule: parity with COLMAP's bundle adjuster and with Ceres is unpinned.
"""
import numpy as np

import util_bundle as ub

MAX_GROUPS = 8                       # VC_BA_MAX_GROUPS
HOLD_FX, HOLD_FY, HOLD_CX, HOLD_CY, TIED = 1, 2, 4, 8, 16
HOLD_PRINCIPAL = HOLD_CX | HOLD_CY
HOLD_ALL = 15
# worst relative difference max|host - spec| / max|spec| of T, the terms, the ordered sums, B, C, h and dX between this
# specification and the kernels' routines compiled for the host (tools/bundle_intr_host.cpp, -O2 -ffp-contract=off) over the
# windowed problem, the 300 random problems with 1-3 groups and random held and tied bits, and the edge cases (measured by
# tests/test_bundle_intr_spec.py, which prints each figure: B 6.7e-13 and h 6.1e-13 on random problems, where the two sums
# that are kept apart cancel; C 5.4e-14, dX 3.1e-14, the terms 1.4e-14, the ordered sums 6.7e-15, T 1.9e-16, obs_xn 0).  Four
# times the worst is the project's margin for instruction selection.
HOST_SPEC_REL = 6.7e-13
TOL_REL = 4 * HOST_SPEC_REL


def theta_held(mask):
    """intr_mask of one group -> bool (4,): the parameter does not move (held, or parameter 1 of a tied group)."""
    m = int(mask)
    return np.array([bool((m >> i) & 1) or (bool(m & TIED) and i == 1) for i in range(4)])


def group_of(cam_group, slot, n_groups):
    g = int(cam_group[slot])
    return g if 0 <= g < n_groups else -1


def normalised(row, X):
    """x = Xc_x / Xc_z, y = Xc_y / Xc_z in the kernel's order of operations."""
    R, t = row[:9], row[9:12]
    Xc = np.array([R[3 * i] * X[0] + R[3 * i + 1] * X[1] + R[3 * i + 2] * X[2] for i in range(3)]) + t
    return Xc[0] / Xc[2], Xc[1] / Xc[2]


def jtheta(x, y, mask):
    """J_theta (2, 4) of a usable observation at the normalised point (x, y) under the group's mask."""
    J = np.array([[x, 0.0, 1.0, 0.0], [0.0, y, 0.0, 1.0]])
    if int(mask) & TIED:
        J[:, 0], J[:, 1] = (x, y), 0.0
    J[:, theta_held(mask)] = 0.0
    return J


def apply_theta(row, dtheta, mask):
    """(fx, fy, cx, cy) += dtheta; tied: dtheta_0 goes to fx and fy."""
    out = np.array(row, np.float64)
    out[12] = row[12] + dtheta[0]
    out[13] = row[13] + (dtheta[0] if int(mask) & TIED else dtheta[1])
    out[14], out[15] = row[14] + dtheta[2], row[15] + dtheta[3]
    return out


def residual_theta(row, X, uv, dtheta, mask):
    """The residual with the intrinsics moved by dtheta (for the derivative test)."""
    return ub.residual_at(apply_theta(row, dtheta, mask), X, uv, np.zeros(3), np.zeros(3))


def linearize_intrinsics(lin, cams, points, offsets, obs_cam, cam_group, n_groups, intr_mask):
    """`lin` of ub.linearize -> dict(xn (total, 2), Jt (total, 2, 4), T (n, G, 4, 3), q (n, G, 4, 4), hq (n, G, 4), P (n, G, G,
    4, 4) = T_g V^-1 T_g'', p (n, G, 4) = T_g V^-1 g_p)."""
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
            xn[o] = normalised(cams[slot], points[j])
            g = group_of(cam_group, slot, G)
            if g < 0:
                continue
            Jt[o] = jtheta(xn[o, 0], xn[o, 1], intr_mask[g])
            T[j, g] = T[j, g] + Jt[o].T @ lin["Jp"][o]
            q[j, g] = q[j, g] + Jt[o].T @ Jt[o]
            hq[j, g] = hq[j, g] + Jt[o].T @ lin["r"][o]
    TV = np.einsum("ngik,nkl->ngil", T, lin["vinv"])
    return dict(xn=xn, Jt=Jt, T=T, q=q, hq=hq, P=np.einsum("ngil,nhkl->nghik", TV, T), p=np.einsum("ngil,nl->ngi", TV, lin["gp"]))


def _ordered(a):
    """The sum over the first axis, one after another in ascending order (np.sum adds in pairs)."""
    return np.cumsum(np.concatenate([np.zeros((1,) + a.shape[1:]), a]), axis=0)[-1]


def reduce_border(lin, li, n_cams, cam_group, n_groups, intr_mask, offsets, obs_cam, cam_offsets, cam_obs, obs_point, lam):
    """-> B (6 n_cams, 4 G), C (4 G, 4 G), h (4 G,), free bool (4 G,): the border of one linearisation."""
    G, total = n_groups, len(lin["ok"])
    Q, SP, shq, sp = _ordered(li["q"]), _ordered(li["P"]), _ordered(li["hq"]), _ordered(li["p"])
    free = np.array([[not held and Q[g, i, i] != 0 for i, held in enumerate(theta_held(intr_mask[g]))] for g in range(G)]).reshape(-1)
    C = np.zeros((G, 4, G, 4))
    for g in range(G):
        Qd = Q[g].copy()
        Qd[np.diag_indices(4)] += lam * np.diag(Q[g])
        for h_ in range(G):
            C[g, :, h_, :] = (Qd if g == h_ else 0.0) - SP[g, h_]
    C = C.reshape(4 * G, 4 * G)
    C[~free, :], C[:, ~free] = 0.0, 0.0
    C[~free, ~free] = 1.0
    h = np.where(free, (shq - sp).reshape(-1), 0.0)
    valid = ub._valid_points(offsets, total)
    B = np.zeros((n_cams, 6, G, 4))
    for a in range(n_cams):
        first, second = np.zeros((G, 6, 4)), np.zeros((G, 6, 4))
        ga = group_of(cam_group, a, G)
        lo, hi = int(cam_offsets[a]), int(cam_offsets[a + 1])
        if 0 <= lo <= hi <= total:
            for o in (int(v) for v in cam_obs[lo:hi]):
                if not (0 <= o < total and lin["ok"][o] and obs_cam[o] == a):
                    continue
                j = int(obs_point[o])
                if not (0 <= j < len(valid) and valid[j] and offsets[j] <= o < offsets[j + 1]):
                    continue
                Y = lin["W"][o] @ lin["vinv"][j]
                if ga >= 0:
                    first[ga] += lin["Jc"][o].T @ li["Jt"][o]
                second += np.einsum("rk,gik->gri", Y, li["T"][j])
        B[a] = (first - second).transpose(1, 0, 2)
    return B.reshape(6 * n_cams, 4 * G), C, h, free


def solve_bordered(S, g, B, C, h, const_mask, free):
    """[[S, B], [B', C]] (dc, dtheta) = -(g, h) by Cholesky -> dc, dtheta (4 G,), or (None, None) where the system is not
    positive definite; a parameter that does not move has a step of exactly 0.  The factorisation is carried out by blocks, S
    first as ub.solve_cameras factors it, then the Schur complement of the border, D = C - B' S^-1 B: the bordered matrix is
    positive definite exactly where both are, and with every intrinsic held (B = 0) the camera step is ub.solve_cameras' bit
    for bit, which one library call on the larger matrix does not promise.  (The product factors the assembled matrix at once.)"""
    try:
        L = np.linalg.cholesky(S)

        def s_solve(b):
            return np.linalg.solve(L.T, np.linalg.solve(L, b))

        D = C - B.T @ s_solve(B)
        LD = np.linalg.cholesky(D)
    except np.linalg.LinAlgError:
        return None, None
    dtheta = np.linalg.solve(LD.T, np.linalg.solve(LD, -h - B.T @ s_solve(-g)))
    dtheta = np.where(free, dtheta, 0.0)
    dc = s_solve(-g - B @ dtheta)
    if not (np.isfinite(dc).all() and np.isfinite(dtheta).all()):
        return None, None
    held = np.array([[(int(m) >> i) & 1 for i in range(6)] for m in const_mask], bool).reshape(-1)
    return np.where(held, 0.0, dc), dtheta


def step_intrinsics(lin, li, cams, points, offsets, obs_cam, cam_group, n_groups, intr_mask, dc, dtheta):
    """The back-substitution and the update -> candidate cams, candidate points, dX, valid bool (n_cams,): the slot's group holds
    its intrinsics or its new fx and fy are finite and positive."""
    cams, points = np.asarray(cams, np.float64).reshape(-1, 16), np.asarray(points, np.float64).reshape(-1, 3)
    dc6, dtheta = np.asarray(dc, np.float64).reshape(-1, 6), np.asarray(dtheta, np.float64).reshape(-1, 4)
    dX = np.zeros_like(points)
    pts_valid = ub._valid_points(offsets, len(lin["ok"]))
    for j in range(len(points)):
        if not pts_valid[j]:
            continue
        s = lin["gp"][j].copy()
        for o in range(offsets[j], offsets[j + 1]):
            if lin["ok"][o]:
                s = s + lin["W"][o].T @ dc6[obs_cam[o]]
        for g in range(n_groups):
            s = s + li["T"][j, g].T @ dtheta[g]
        dX[j] = -(lin["vinv"][j] @ s)
    out, _, _ = ub.step(lin, cams, points[:0], offsets[:1], obs_cam, dc6)        # the pose update is util_bundle's
    valid = np.ones(len(cams), bool)
    with np.errstate(all="ignore"):
        for a in range(len(cams)):
            g = group_of(cam_group, a, n_groups)
            if g >= 0:
                out[a] = apply_theta(out[a], dtheta[g], intr_mask[g])
                valid[a] = bool(np.isfinite(out[a, 12:14]).all() and (out[a, 12:14] > 0).all())
    return out, points + dX, dX, valid


def group_intrinsics(cams, cam_group, n_groups):
    """-> float64 (G, 4): (fx, fy, cx, cy) of the first slot of each group, NaN for a group without a slot."""
    out = np.full((n_groups, 4), np.nan)
    for a in range(len(cams) - 1, -1, -1):
        g = group_of(cam_group, a, n_groups)
        if g >= 0:
            out[g] = cams[a, 12:16]
    return out


def bundle_adjust(cams, points, offsets, obs_cam, obs_xy, const_mask, cam_group, intr_mask, max_iterations=ub.BA_MAX_ITERATIONS):
    """The loop of ub.bundle_adjust over (c, theta, X); a candidate one of whose focal lengths is not finite or not positive
    is rejected.  The report gains `intrinsics`: dict(before (G, 4), after (G, 4))."""
    cams, points = np.array(cams, np.float64).reshape(-1, 16), np.array(points, np.float64).reshape(-1, 3)
    n_cams, G = len(cams), len(intr_mask)
    index = ub.camera_index(obs_cam, offsets, n_cams)
    before = group_intrinsics(cams, cam_group, G)
    lam = ub.BA_LAMBDA0
    lin = ub.linearize(cams, points, offsets, obs_cam, obs_xy, const_mask, lam)
    cost = initial = lin["total_cost"]
    iterations, decisions = 1, []
    while iterations < max_iterations and len(points) and n_cams:
        S, g = ub.reduce_cameras(lin, n_cams, offsets, obs_cam, const_mask, *index, lam)
        li = linearize_intrinsics(lin, cams, points, offsets, obs_cam, cam_group, G, intr_mask)
        B, C, h, free = reduce_border(lin, li, n_cams, cam_group, G, intr_mask, offsets, obs_cam, *index, lam)
        dc, dtheta = solve_bordered(S, g, B, C, h, const_mask, free)
        lower = max(lam / 10, ub.BA_LAMBDA_MIN)
        iterations += 1
        accepted = False
        if dc is not None:
            cand_cams, cand_points, _, valid = step_intrinsics(lin, li, cams, points, offsets, obs_cam, cam_group, G, intr_mask, dc, dtheta)
            cand = ub.linearize(cand_cams, cand_points, offsets, obs_cam, obs_xy, const_mask, lower)
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
            lin = ub.linearize(cams, points, offsets, obs_cam, obs_xy, const_mask, lam)
            iterations += 1
    return cams, points, dict(iterations=iterations, accepted_steps=int(sum(decisions)), initial_cost=initial, final_cost=cost,
                              final_lambda=lam, decisions=decisions,
                              intrinsics=dict(before=before, after=group_intrinsics(cams, cam_group, G)))


def random_groups(i, n_cams):
    """The groups of random problem i from RandomState(25000 + i): 1-3 groups, every slot in one of them, any of the 32 masks of
    held and tied bits per group -> cam_group int32, intr_mask uint8."""
    rs = np.random.RandomState(25000 + i)
    G = int(rs.randint(1, 4))
    return rs.randint(0, G, n_cams).astype(np.int32), rs.randint(0, 32, G).astype(np.uint8)
