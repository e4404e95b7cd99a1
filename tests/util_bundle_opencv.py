"""CPU SPECIFICATION (test infrastructure, NOT product code) of bundle adjustment with radial and tangential distortion (DESIGN.md
§4.2k, "The tangential terms"): COLMAP's OPENCV camera, theta_g = (fx, fy, cx, cy, k1, k2, p1, p2) of every group of cameras as the
border of tests/util_bundle_intr.py with eight unknowns per group, under the losses of tests/util_bundle_loss.py.  It builds on
tests/util_bundle.py, tests/util_bundle_intr.py, tests/util_bundle_loss.py and tests/util_bundle_radial.py by import and changes
none of them.  numpy only.

The rule, for camera row c = (R, t, fx, fy, cx, cy), its (k1, k2, p1, p2) and the point X, float64 in single operations in the
written order (left to right, the usual precedence), as include/vitcolmap_hip.h states it:
  Y = R X, Xc = Y + t, iu = 1 / Xc_z, xu = Xc_x / Xc_z, xv = Xc_y / Xc_z
  nu_k = iu (R_0k - xu R_2k), nv_k = iu (R_1k - xv R_2k)
  rho = xu xu + xv xv, s = 1 + k1 rho + k2 rho rho, e = 2 (k1 + 2 k2 rho)
  xd = xu s + 2 p1 xu xv + p2 (rho + 2 xu xu), yd = xv s + p1 (rho + 2 xv xv) + 2 p2 xu xv
  d00 = s + xu xu e + 2 p1 xv + 6 p2 xu, d01 = xu xv e + 2 p1 xu + 2 p2 xv, d11 = s + xv xv e + 6 p1 xv + 2 p2 xu
  r = (fx xd + cx - u, fy yd + cy - v)
  J_p = (fx (d00 nu + d01 nv); fy (d01 nu + d11 nv)), J_c likewise from the pinhole rows at fx = fy = 1
  J_theta, columns (fx, fy, cx, cy, k1, k2, p1, p2):
    row u (xd, 0, 1, 0, fx xu rho, (fx xu rho) rho, fx 2 xu xv, fx (rho + 2 xu xu))
    row v (0, yd, 0, 1, fy xv rho, (fy xv rho) rho, fy (rho + 2 xv xv), fy 2 xu xv)
  tied: column 0 = (xd, yd), column 1 = 0; a held column is 0; bit 7 of the mask holds p1 and p2 together
The forward model and D are tests/util_undistort.py's distort_normalised and jacobian (the radial term first, the tangential terms
added after it), so undistortion and adjustment agree on one model.  The accumulations are util_bundle's and util_bundle_intr's,
written independently of csrc/bundle.hip.  This is the build's own published rule: parity with COLMAP and Ceres is unpinned.
"""
import numpy as np

import util_bundle as ub
import util_bundle_intr as ui
import util_bundle_loss as ul
import util_bundle_radial as ur
import util_mapper as um
import util_undistort as uu

MAX_GROUPS = 4                       # VC_BA_MAX_GROUPS_OPENCV
HOLD_TANGENTIAL = 128                # bit 7 of a group's intr_mask: p1 and p2 held, both; bits 0-6 are util_bundle_radial's
HOLD_DIST = ur.HOLD_DIST | HOLD_TANGENTIAL
N = 8                                # unknowns per group
JT = 10                              # numbers per observation from which the border rebuilds J_theta
# worst relative difference max|host - spec| / max|spec| of every array of the plain and of the bordered system between this
# specification and the kernels' routines compiled for the host (tools/bundle_host.cpp with the OPENCV section of its problem
# file) over the distorted windowed problem, 100 random problems with 1-3 groups, random masks (bit 7 among them), |k1| <= 0.2,
# |k2| <= 0.05, |p| <= 2e-3, and the nine edge problems, without a loss and under Huber at 1 px (measured by
# tests/test_bundle_opencv_spec.py, which prints each figure: h 6.37e-12 on random problem 68 under Huber and C 1.90e-12 on random
# problem 56 under Huber, where the two sums that are kept apart cancel, as without the tangential terms; B 1.4e-13, dx 4.0e-14,
# vinv 2.8e-14, g 1.6e-14, the terms 7.8e-15, S 6.9e-15, the ordered sums 2.9e-15, the points 1.5e-15, g_p 3.3e-16, T 2.9e-16;
# obs_jt, obs_w, out_dist and the costs are equal to the bit).  The tolerance of the loss and the radial tests, ul.TOL_REL =
# 5.2e-12, does not hold the h of random problem 68: its masks and distortion come from another random stream than the radial
# section's (eight unknowns per group, 256 masks), and there sum hq - sum T V^-1 g_p leaves 1e-3 of either sum, so the rounding of
# the sums (1e-15) is 6e-12 of what is left.  The arithmetic is the radial section's.  The tolerance is therefore 4x the measured
# worst, rounded up, the project's margin.
HOST_SPEC_REL = 6.37e-12
TOL_REL = 2.6e-11


def theta_held(mask):
    """intr_mask of one group -> bool (8,): the parameter does not move."""
    m = int(mask)
    return np.concatenate([ur.theta_held(m), [bool(m & HOLD_TANGENTIAL)] * 2])


def distortion(xu, xv, dist):
    """-> rho, (xd, yd), (d00, d01, d11) in the kernel's order of operations."""
    k1, k2, p1, p2 = (np.float64(v) for v in dist)
    rho = xu * xu + xv * xv
    s = 1.0 + k1 * rho + k2 * rho * rho
    e = 2.0 * (k1 + 2.0 * k2 * rho)
    xd = xu * s + 2.0 * p1 * xu * xv + p2 * (rho + 2.0 * xu * xu)
    yd = xv * s + p1 * (rho + 2.0 * xv * xv) + 2.0 * p2 * xu * xv
    d00 = s + xu * xu * e + 2.0 * p1 * xv + 6.0 * p2 * xu
    d01 = xu * xv * e + 2.0 * p1 * xu + 2.0 * p2 * xv
    d11 = s + xv * xv * e + 6.0 * p1 * xv + 2.0 * p2 * xu
    return rho, (xd, yd), (d00, d01, d11)


def project(row, dist, X):
    """The pixel of X in the camera (row, dist), through util_undistort's forward model (for the derivative tests and the scenes)."""
    Xc = row[:9].reshape(3, 3) @ X + row[9:12]
    xd, yd = uu.distort_normalised(Xc[0] / Xc[2], Xc[1] / Xc[2], np.concatenate([row[12:16], dist]))
    return np.array([row[12] * xd + row[14], row[13] * yd + row[15]])


def observe(row, dist, X, uv, mask=0):
    """One observation -> usable, r (2,), J_c (2, 6), J_p (2, 3), jt (10,) in the kernel's order."""
    R, t, fx, fy, cx, cy = row[:9], row[9:12], row[12], row[13], row[14], row[15]
    dist = np.asarray(dist, np.float64)
    with np.errstate(all="ignore"):
        Y = np.array([R[3 * i] * X[0] + R[3 * i + 1] * X[1] + R[3 * i + 2] * X[2] for i in range(3)])
        Xc = Y + t
        z = Xc[2]
        usable = bool(np.isfinite(row).all() and np.isfinite(uv).all() and np.isfinite(dist).all() and z > 0)
        if not usable:
            return False, np.zeros(2), np.zeros((2, 6)), np.zeros((2, 3)), np.zeros(JT)
        iu, xu, xv = 1.0 / z, Xc[0] / z, Xc[1] / z
        nu = np.array([iu * (R[k] - xu * R[6 + k]) for k in range(3)])
        nv = np.array([iu * (R[3 + k] - xv * R[6 + k]) for k in range(3)])
        rho, (xd, yd), (d00, d01, d11) = distortion(xu, xv, dist)
        pu, pv = fx * xu * rho, fy * xv * rho
        jt = np.array([xd, yd, pu, pv, pu * rho, pv * rho, fx * 2.0 * xu * xv, fy * (rho + 2.0 * xv * xv), fx * (rho + 2.0 * xu * xu),
                       fy * 2.0 * xu * xv])
        r = np.array([fx * xd + cx - uv[0], fy * yd + cy - uv[1]])
        Jp = np.array([[fx * (d00 * nu[k] + d01 * nv[k]) for k in range(3)], [fy * (d01 * nu[k] + d11 * nv[k]) for k in range(3)]])
        au, av = iu * xu, iu * xv
        mu = [-(au * Y[1]), iu * Y[2] + au * Y[0], -(iu * Y[1]), iu, 0.0, -au]
        mv = [-(iu * Y[2] + av * Y[1]), av * Y[0], iu * Y[0], 0.0, iu, -av]
        Jc = np.array([[fx * (d00 * mu[i] + d01 * mv[i]) for i in range(6)], [fy * (d01 * mu[i] + d11 * mv[i]) for i in range(6)]])
        for i in range(6):
            if (int(mask) >> i) & 1:
                Jc[:, i] = 0.0
    return usable, r, Jc, Jp, jt


def jtheta(jt, mask):
    """J_theta (2, 8) of a usable observation from its ten numbers under the group's mask."""
    J = np.array([[jt[0], 0.0, 1.0, 0.0, jt[2], jt[4], jt[6], jt[8]], [0.0, jt[1], 0.0, 1.0, jt[3], jt[5], jt[7], jt[9]]])
    if int(mask) & ui.TIED:
        J[:, 0], J[:, 1] = (jt[0], jt[1]), 0.0
    J[:, theta_held(mask)] = 0.0
    return J


def apply_theta(row, dist, dtheta, mask):
    """(fx, fy, cx, cy) and (k1, k2, p1, p2) += dtheta; tied: dtheta_0 goes to fx and fy."""
    return ui.apply_theta(row, dtheta[:4], mask), np.array([dist[i] + dtheta[4 + i] for i in range(4)])


def linearize(cams, dist, points, offsets, obs_cam, obs_xy, const_mask, lam, loss=ul.TRIVIAL, loss_scale=1.0):
    """ur.linearize under the four distortion numbers -> its dict, with jt (total, 10), unscaled."""
    cams, points = np.asarray(cams, np.float64).reshape(-1, 16), np.asarray(points, np.float64).reshape(-1, 3)
    dist, obs_xy = np.asarray(dist, np.float64).reshape(-1, 4), np.asarray(obs_xy, np.float64).reshape(-1, 2)
    n, total, n_cams = len(points), len(obs_xy), len(cams)
    ok, r, sw, jt = np.zeros(total, bool), np.zeros((total, 2)), np.zeros(total), np.zeros((total, JT))
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
            ok[o], r[o], Jc[o], Jp[o], jt[o] = observe(cams[slot], dist[slot], points[j], obs_xy[o], const_mask[slot])
            if not ok[o]:
                continue
            with np.errstate(all="ignore"):
                rho, w = ul.loss_terms(loss, loss_scale, r[o, 0] * r[o, 0] + r[o, 1] * r[o, 1])
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
    return dict(ok=ok, r=r, Jc=Jc, Jp=Jp, W=W, vinv=vinv, gp=gp, cost=cost, count=count, constant=constant, sw=sw, jt=jt,
                total_cost=total_cost)


def linearize_intrinsics(lin, offsets, obs_cam, cam_group, n_groups, intr_mask):
    """`lin` of `linearize` -> dict(Jt (total, 2, 8), T (n, G, 8, 3), q (n, G, 8, 8), hq (n, G, 8), P (n, G, G, 8, 8), p (n, G, 8));
    J_theta (its constant columns too) is multiplied by sw."""
    n, total, G = len(lin["gp"]), len(lin["ok"]), n_groups
    Jt = np.zeros((total, 2, N))
    T, q, hq = np.zeros((n, G, N, 3)), np.zeros((n, G, N, N)), np.zeros((n, G, N))
    valid = ub._valid_points(offsets, total)
    for j in range(n):
        if not valid[j]:
            continue
        for o in range(offsets[j], offsets[j + 1]):
            if not lin["ok"][o]:
                continue
            g = ui.group_of(cam_group, int(obs_cam[o]), G)
            if g < 0:
                continue
            Jt[o] = lin["sw"][o] * jtheta(lin["jt"][o], intr_mask[g])
            T[j, g] = T[j, g] + Jt[o].T @ lin["Jp"][o]
            q[j, g] = q[j, g] + Jt[o].T @ Jt[o]
            hq[j, g] = hq[j, g] + Jt[o].T @ lin["r"][o]
    TV = np.einsum("ngik,nkl->ngil", T, lin["vinv"])
    return dict(Jt=Jt, T=T, q=q, hq=hq, P=np.einsum("ngil,nhkl->nghik", TV, T), p=np.einsum("ngil,nl->ngi", TV, lin["gp"]))


def reduce_border(lin, li, n_cams, cam_group, n_groups, intr_mask, offsets, obs_cam, cam_offsets, cam_obs, obs_point, lam):
    """ui.reduce_border with eight unknowns per group -> B (6 n_cams, 8 G), C (8 G, 8 G), h (8 G,), free bool (8 G,)."""
    G, total = n_groups, len(lin["ok"])
    Q, SP, shq, sp = ui._ordered(li["q"]), ui._ordered(li["P"]), ui._ordered(li["hq"]), ui._ordered(li["p"])
    free = np.array([[not held and Q[g, i, i] != 0 for i, held in enumerate(theta_held(intr_mask[g]))] for g in range(G)]).reshape(-1)
    C = np.zeros((G, N, G, N))
    for g in range(G):
        Qd = Q[g].copy()
        Qd[np.diag_indices(N)] += lam * np.diag(Q[g])
        for h_ in range(G):
            C[g, :, h_, :] = (Qd if g == h_ else 0.0) - SP[g, h_]
    C = C.reshape(N * G, N * G)
    C[~free, :], C[:, ~free] = 0.0, 0.0
    C[~free, ~free] = 1.0
    h = np.where(free, (shq - sp).reshape(-1), 0.0)
    valid = ub._valid_points(offsets, total)
    B = np.zeros((n_cams, 6, G, N))
    for a in range(n_cams):
        first, second = np.zeros((G, 6, N)), np.zeros((G, 6, N))
        ga = ui.group_of(cam_group, a, G)
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
    return B.reshape(6 * n_cams, N * G), C, h, free


def step(lin, li, cams, dist, points, offsets, obs_cam, cam_group, n_groups, intr_mask, dc, dtheta):
    """-> candidate cams, dist, points, dX, valid bool (n_cams,): the slot's group holds its intrinsics, or its new fx and fy are
    finite and positive and its four new distortion numbers finite."""
    cams, points = np.asarray(cams, np.float64).reshape(-1, 16), np.asarray(points, np.float64).reshape(-1, 3)
    dist = np.asarray(dist, np.float64).reshape(-1, 4)
    dc6, dtheta = np.asarray(dc, np.float64).reshape(-1, 6), np.asarray(dtheta, np.float64).reshape(-1, N)
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
    out, _, _ = ub.step(lin, cams, points[:0], offsets[:1], obs_cam, dc6)
    out_dist = dist.copy()
    valid = np.ones(len(cams), bool)
    with np.errstate(all="ignore"):
        for a in range(len(cams)):
            g = ui.group_of(cam_group, a, n_groups)
            if g >= 0:
                out[a], out_dist[a] = apply_theta(out[a], dist[a], dtheta[g], intr_mask[g])
                valid[a] = bool(np.isfinite(out[a, 12:14]).all() and (out[a, 12:14] > 0).all() and np.isfinite(out_dist[a]).all())
    return out, out_dist, points + dX, dX, valid


def group_intrinsics(cams, dist, cam_group, n_groups):
    """-> float64 (G, 8): (fx, fy, cx, cy, k1, k2, p1, p2) of the first slot of each group, NaN for a group without a slot."""
    out = np.full((n_groups, N), np.nan)
    for a in range(len(cams) - 1, -1, -1):
        g = ui.group_of(cam_group, a, n_groups)
        if g >= 0:
            out[g] = np.concatenate([cams[a, 12:16], dist[a]])
    return out


def one_pass(problem, dist, groups, lam=ub.BA_LAMBDA0, loss=ul.TRIVIAL, loss_scale=1.0):
    """One linearisation, both reductions, the bordered solve and the step."""
    cams, points, offsets, obs_cam, obs_xy, mask = problem
    cam_group, intr_mask = groups
    G, index = len(intr_mask), ub.camera_index(obs_cam, offsets, len(cams))
    lin = linearize(cams, dist, points, offsets, obs_cam, obs_xy, mask, lam, loss, loss_scale)
    S, g = ub.reduce_cameras(lin, len(cams), offsets, obs_cam, mask, *index, lam)
    li = linearize_intrinsics(lin, offsets, obs_cam, cam_group, G, intr_mask)
    B, C, h, free = reduce_border(lin, li, len(cams), cam_group, G, intr_mask, offsets, obs_cam, *index, lam)
    dc, dtheta = ui.solve_bordered(S, g, B, C, h, mask, free)
    if dc is None:
        dc, dtheta = np.zeros(6 * len(cams)), np.zeros(N * G)
    out_cams, out_dist, out_points, dX, valid = step(lin, li, cams, dist, points, offsets, obs_cam, cam_group, G, intr_mask, dc, dtheta)
    return dict(lin=lin, li=li, S=S, g=g, B=B, C=C, h=h, free=free, dc=dc, dtheta=dtheta, cams=out_cams, dist=out_dist, points=out_points,
                dx=dX, valid=valid)


def bundle_adjust(cams, dist, points, offsets, obs_cam, obs_xy, const_mask, cam_group, intr_mask, loss=ul.TRIVIAL, loss_scale=1.0,
                  max_iterations=ub.BA_MAX_ITERATIONS):
    """The loop of ur.bundle_adjust over (c, theta, X) with theta = (fx, fy, cx, cy, k1, k2, p1, p2) -> cams, dist, points, report;
    `intrinsics` = dict(before (G, 8), after (G, 8))."""
    cams, points = np.array(cams, np.float64).reshape(-1, 16), np.array(points, np.float64).reshape(-1, 3)
    dist = np.array(dist, np.float64).reshape(-1, 4)
    n_cams, G = len(cams), len(intr_mask)
    index = ub.camera_index(obs_cam, offsets, n_cams)
    before = group_intrinsics(cams, dist, cam_group, G)

    def lin_at(c, k, p, lam):
        return linearize(c, k, p, offsets, obs_cam, obs_xy, const_mask, lam, loss, loss_scale)

    lam = ub.BA_LAMBDA0
    lin = lin_at(cams, dist, points, lam)
    cost = initial = lin["total_cost"]
    iterations, decisions = 1, []
    while iterations < max_iterations and len(points) and n_cams:
        S, g = ub.reduce_cameras(lin, n_cams, offsets, obs_cam, const_mask, *index, lam)
        li = linearize_intrinsics(lin, offsets, obs_cam, cam_group, G, intr_mask)
        B, C, h, free = reduce_border(lin, li, n_cams, cam_group, G, intr_mask, offsets, obs_cam, *index, lam)
        dc, dtheta = ui.solve_bordered(S, g, B, C, h, const_mask, free)
        lower = max(lam / 10, ub.BA_LAMBDA_MIN)
        iterations += 1
        accepted = False
        if dc is not None:
            cand_cams, cand_dist, cand_points, _, valid = step(lin, li, cams, dist, points, offsets, obs_cam, cam_group, G, intr_mask, dc, dtheta)
            cand = lin_at(cand_cams, cand_dist, cand_points, lower)
            accepted = bool(valid.all() and np.isfinite(cand["total_cost"]) and cand["total_cost"] < cost)
        decisions.append(accepted)
        if accepted:
            decrease = (cost - cand["total_cost"]) / cost
            cams, dist, points, lin, cost, lam = cand_cams, cand_dist, cand_points, cand, cand["total_cost"], lower
            if decrease < ub.BA_REL_DECREASE:
                break
        else:
            lam = lam * 10
            if lam > ub.BA_LAMBDA_MAX or iterations >= max_iterations:
                break
            lin = lin_at(cams, dist, points, lam)
            iterations += 1
    report = dict(iterations=iterations, accepted_steps=int(sum(decisions)), initial_cost=initial, final_cost=cost, final_lambda=lam,
                  decisions=decisions, loss={v: k for k, v in ul.LOSSES.items()}[loss], loss_scale=float(loss_scale),
                  intrinsics=dict(before=before, after=group_intrinsics(cams, dist, cam_group, G)))
    return cams, dist, points, report


# ---- the host program's OPENCV section --------------------------------------------------------------------------------------------------
def write_problem_file(path, problem, dist, lam, dc, groups, dtheta, loss=ul.TRIVIAL, loss_scale=1.0, index=None):
    """The input of tools/bundle_host.cpp with the loss and the OPENCV section (marker 2) appended; dist (n_cams, 4), dtheta (G, 8)."""
    from test_bundle_spec import write_problem_file as write_plain

    write_plain(path, problem, lam, dc, index, groups, np.zeros(4 * len(groups[1])))
    with open(path, "ab") as f:
        f.write(np.array([loss], np.int32).tobytes() + np.array([loss_scale], np.float64).tobytes() + np.array([2], np.int32).tobytes())
        f.write(np.ascontiguousarray(dist, np.float64).tobytes() + np.ascontiguousarray(dtheta, np.float64).tobytes())


def term_rows(G):
    """Rows of the per-point terms: (N N + 2 N) G + N N G^2; 1344 at G = 4."""
    return 80 * G + 64 * G * G


def result_shapes(n_cams, n_points, total, G):
    """The float64 arrays of the border's section of an OPENCV result."""
    rows = term_rows(G)
    return [("jt", (total, JT)), ("T", (n_points, G, 3 * N)), ("terms", (rows, n_points)), ("sums", (rows,)), ("B", (6 * n_cams, N * G)),
            ("C", (N * G, N * G)), ("h", (N * G,)), ("cams", (n_cams, 16)), ("points", (n_points, 3)), ("dx", (n_points, 3)),
            ("dist", (n_cams, 4))]


def read_result_file(path, n_cams, n_points, total, G):
    raw = open(path, "rb").read()
    at = 0

    def take(dtype, shape):
        nonlocal at
        a = np.frombuffer(raw, dtype, int(np.prod(shape)), at).reshape(shape)
        at += a.nbytes
        return a

    shapes = [("vinv", (n_points, 6)), ("gp", (n_points, 3)), ("cost", (n_points,)), ("total_cost", (1,)), ("S", (6 * n_cams, 6 * n_cams)),
              ("g", (6 * n_cams,)), ("cams", (n_cams, 16)), ("points", (n_points, 3)), ("dx", (n_points, 3)), ("obs_lin", (total, 32))]
    plain = {name: take(np.float64, shape) for name, shape in shapes}
    plain["count"], plain["obs_ok"] = take(np.int32, (n_points,)), take(np.uint8, (total,))
    out = dict({name: take(np.float64, shape) for name, shape in result_shapes(n_cams, n_points, total, G)}, plain=plain)
    out["free"], out["valid"] = take(np.uint8, (N * G,)), take(np.uint8, (n_cams,))
    out["obs_w"] = take(np.float64, (total,))
    assert at == len(raw)
    return out


def run_host(program, tmp_path, problem, dist, lam, dc, groups, dtheta, loss=ul.TRIVIAL, loss_scale=1.0, index=None, name="opencv"):
    import subprocess

    write_problem_file(tmp_path / f"{name}.bin", problem, dist, lam, dc, groups, dtheta, loss, loss_scale, index)
    done = subprocess.run([program, str(tmp_path / f"{name}.bin"), str(tmp_path / f"{name}_result.bin")], stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, text=True)
    assert done.returncode == 0, done.stderr
    return read_result_file(tmp_path / f"{name}_result.bin", len(problem[0]), len(problem[1]), len(problem[3]), len(groups[1])), done.stderr


def random_groups(i, n_cams):
    """The groups and the distortion of random problem i from RandomState(37000 + i): 1-3 groups, every slot in one of them, any
    of the 256 masks per group (bit 7 among them), |k1| <= 0.2, |k2| <= 0.05, |p1|, |p2| <= 2e-3 per group
    -> (cam_group int32, intr_mask uint8), dist (n_cams, 4)."""
    rs = np.random.RandomState(37000 + i)
    G = int(rs.randint(1, 4))
    cam_group = rs.randint(0, G, n_cams).astype(np.int32)
    k = np.stack([rs.uniform(-0.2, 0.2, G), rs.uniform(-0.05, 0.05, G), rs.uniform(-2e-3, 2e-3, G), rs.uniform(-2e-3, 2e-3, G)], axis=1)
    return (cam_group, rs.randint(0, 256, G).astype(np.uint8)), k[cam_group]


# ---- the distorted scene ---------------------------------------------------------------------------------------------------------------
DIST_TRUE = uu.PARAMETER_SETS[3]     # (-0.2, 0.05, 1e-3, -2e-3)


def distorted_windowed_scene(dist=DIST_TRUE):
    """um.windowed_scene() with every true keypoint moved by util_undistort.distort under (fx, fy, cx, cy, *dist); the random
    keypoints are left alone."""
    scene = um.windowed_scene()
    K = scene["K"]
    cam = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2], *dist], np.float64)
    kps = [np.where(seen[:, None], uu.distort(kp.astype(np.float64), cam), kp.astype(np.float64)).astype(np.float32)
           for kp, seen in zip(scene["keypoints"], scene["visible"])]
    return dict(scene, keypoints=kps, dist=tuple(float(v) for v in dist))
