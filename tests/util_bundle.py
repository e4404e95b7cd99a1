"""CPU SPECIFICATION (test infrastructure, NOT product code) of bundle adjustment: the linearisation of
every observation, the per-point Schur complement, the reduced camera system, the back-substitution, the trig-free pose
update, the Levenberg-Marquardt loop, the gauge, the rescale and the filter that turn a grown model into an adjusted one.
numpy only; the grown model and the scenes are tests/util_mapper.py's and tests/util_absolute_pose.py's.

The per-observation arithmetic is written in the kernel's order of single float64 operations; the accumulations are written
independently of csrc/bundle.hip (whole 3x3 and 6x6 blocks through numpy's matrix products and its unbuffered scatter-add
instead of one entry per lane), in the order the rule gives.  This is the build's own published rule: parity with COLMAP's
bundle adjuster and with Ceres is unpinned.
"""
import numpy as np

import util_absolute_pose as ua
import util_mapper as um

BA_LAMBDA0 = 1e-4
BA_LAMBDA_MIN, BA_LAMBDA_MAX = 1e-12, 1e12
BA_MAX_ITERATIONS = 25               # linearisations
BA_REL_DECREASE = 1e-8               # an accepted step that lowers the cost by less (relative) ends the loop
MAX_ERROR = um.MAX_ERROR             # px, the filter after the adjustment  [recalled: COLMAP filter_max_reproj_error 4 px]
HELD_ALL = 63                        # bits 0-2: the rotation w, bits 3-5: the translation t
# worst relative difference max|host - spec| / max|spec| of V^-1, g_p, S, g and dX between this specification and the kernel's
# routines compiled for the host (tools/bundle_host.cpp, -O2 -ffp-contract=off) over the windowed problem, the 300 random
# problems and the edge cases of `edge_problems`, the usable counts and the constant points equal (measured by
# tests/test_bundle_spec.py, which prints each figure: V^-1 3.4e-14, dX 2.0e-14, g 1.6e-14, S 4.0e-15, g_p 2.9e-16, all on
# random problems, where a point seen by two close cameras has a V of condition 1e2 and more; dX is compared under the
# specification's own dc, so that the comparison does not go through a solve of either S).  Four times that is the project's
# margin for instruction selection.
HOST_SPEC_REL = 3.4e-14
TOL_REL = 4 * HOST_SPEC_REL


# ---- the problem's indices ------------------------------------------------------------------------------------------------------
def camera_index(obs_cam, offsets, n_cams):
    """-> cam_offsets (n_cams + 1,), cam_obs (total,): the observations of each camera in ascending order (those whose slot is
    outside [0, n_cams) belong to none and are left out, the tail of cam_obs is then unused), obs_point (total,): the point
    of each observation."""
    obs_cam, offsets = np.asarray(obs_cam, np.int64), np.asarray(offsets, np.int64)
    total = len(obs_cam)
    inside = (obs_cam >= 0) & (obs_cam < n_cams)
    order = np.argsort(np.where(inside, obs_cam, n_cams), kind="stable")[:int(inside.sum())]
    cam_obs = np.full(total, -1, np.int32)
    cam_obs[:len(order)] = order
    cam_offsets = np.concatenate([[0], np.cumsum(np.bincount(obs_cam[inside], minlength=n_cams))]).astype(np.int32)
    obs_point = np.full(total, -1, np.int32)
    for j in range(len(offsets) - 1):
        if 0 <= offsets[j] <= offsets[j + 1] <= total:
            obs_point[offsets[j]:offsets[j + 1]] = j
    return cam_offsets, cam_obs, obs_point


def _valid_points(offsets, total):
    lo, hi = np.asarray(offsets[:-1], np.int64), np.asarray(offsets[1:], np.int64)
    return (lo >= 0) & (hi >= lo) & (hi <= total)


# ---- one linearisation --------------------------------------------------------------------------------------------------------------
def observe(row, X, uv, mask=0):
    """One observation: camera row (16,), point (3,), pixel (2,), the camera's held bits -> usable, r (2,), J_c (2, 6), J_p
    (2, 3) in the kernel's order of operations."""
    R, t, fx, fy, cx, cy = row[:9], row[9:12], row[12], row[13], row[14], row[15]
    with np.errstate(all="ignore"):
        Y = np.array([R[3 * i] * X[0] + R[3 * i + 1] * X[1] + R[3 * i + 2] * X[2] for i in range(3)])
        Xc = Y + t
        z = Xc[2]
        usable = bool(np.isfinite(row).all() and np.isfinite(uv).all() and z > 0)
        if not usable:
            return False, np.zeros(2), np.zeros((2, 6)), np.zeros((2, 3))
        r = np.array([fx * Xc[0] / z + cx - uv[0], fy * Xc[1] / z + cy - uv[1]])
        fu, fv, xu, xv = fx / z, fy / z, Xc[0] / z, Xc[1] / z
        au, av = fu * xu, fv * xv
        Jp = np.array([[fu * (R[k] - xu * R[6 + k]) for k in range(3)], [fv * (R[3 + k] - xv * R[6 + k]) for k in range(3)]])
        Jc = np.array([[-(au * Y[1]), fu * Y[2] + au * Y[0], -(fu * Y[1]), fu, 0.0, -au],
                       [-(fv * Y[2] + av * Y[1]), av * Y[0], fv * Y[0], 0.0, fv, -av]])
        for i in range(6):
            if (int(mask) >> i) & 1:
                Jc[:, i] = 0.0
    return usable, r, Jc, Jp


def residual_at(row, X, uv, w, dt):
    """The residual of the pose perturbed on the left by the exact rotation Rot(w) and by dt (for the derivative test)."""
    R = ua.rodrigues(np.asarray(w, np.float64)) @ row[:9].reshape(3, 3)
    Xc = R @ X + row[9:12] + dt
    return np.array([row[12] * Xc[0] / Xc[2] + row[14] - uv[0], row[13] * Xc[1] / Xc[2] + row[15] - uv[1]])


def adjugate_inverse(V):
    """The symmetric 3x3 V -> (its inverse by the adjugate, the determinant), as the triangulation refit does it."""
    A00, A01, A02, A11, A12, A22 = V[0, 0], V[0, 1], V[0, 2], V[1, 1], V[1, 2], V[2, 2]
    c00, c01, c02 = A11 * A22 - A12 * A12, A02 * A12 - A01 * A22, A01 * A12 - A02 * A11
    c11, c12, c22 = A00 * A22 - A02 * A02, A01 * A02 - A00 * A12, A00 * A11 - A01 * A01
    det = A00 * c00 + A01 * c01 + A02 * c02
    with np.errstate(all="ignore"):
        inv = 1.0 / det
        return np.array([[c00 * inv, c01 * inv, c02 * inv], [c01 * inv, c11 * inv, c12 * inv], [c02 * inv, c12 * inv, c22 * inv]]), det


def linearize(cams, points, offsets, obs_cam, obs_xy, const_mask, lam):
    """-> dict(ok bool (total,), r (total, 2), Jc (total, 2, 6), Jp (total, 2, 3), W (total, 6, 3), vinv (n, 3, 3) damped, gp
    (n, 3), cost (n,), count (n,), constant bool (n,), total_cost)."""
    cams, points = np.asarray(cams, np.float64).reshape(-1, 16), np.asarray(points, np.float64).reshape(-1, 3)
    obs_xy = np.asarray(obs_xy, np.float64).reshape(-1, 2)
    n, total, n_cams = len(points), len(obs_xy), len(cams)
    ok, r = np.zeros(total, bool), np.zeros((total, 2))
    Jc, Jp, W = np.zeros((total, 2, 6)), np.zeros((total, 2, 3)), np.zeros((total, 6, 3))
    vinv, gp, cost, count = np.zeros((n, 3, 3)), np.zeros((n, 3)), np.zeros(n), np.zeros(n, np.int32)
    constant = np.ones(n, bool)
    valid = _valid_points(offsets, total)
    for j in range(n):
        if not valid[j]:
            continue
        V, c = np.zeros((3, 3)), 0.0
        for o in range(offsets[j], offsets[j + 1]):
            slot = int(obs_cam[o])
            if not 0 <= slot < n_cams:
                continue
            ok[o], r[o], Jc[o], Jp[o] = observe(cams[slot], points[j], obs_xy[o], const_mask[slot])
            if not ok[o]:
                continue
            W[o] = Jc[o].T @ Jp[o]
            V = V + Jp[o].T @ Jp[o]
            gp[j] = gp[j] + Jp[o].T @ r[o]
            c = c + (r[o, 0] * r[o, 0] + r[o, 1] * r[o, 1])
            count[j] += 1
        cost[j] = 0.5 * c
        V[np.diag_indices(3)] += lam * np.diag(V)
        inv, det = adjugate_inverse(V)
        if count[j] >= 2 and np.isfinite(det) and det > 0:
            vinv[j], constant[j] = inv, False
    return dict(ok=ok, r=r, Jc=Jc, Jp=Jp, W=W, vinv=vinv, gp=gp, cost=cost, count=count, constant=constant,
                total_cost=float(np.cumsum(np.concatenate([[0.0], cost]))[-1]))


def reduce_cameras(lin, n_cams, offsets, obs_cam, const_mask, cam_offsets, cam_obs, obs_point, lam):
    """-> S (6 n_cams, 6 n_cams), g (6 n_cams,): the reduced camera system of one linearisation."""
    total = len(lin["ok"])
    S = np.zeros((n_cams, 6, n_cams, 6))
    g = np.zeros((n_cams, 6))
    valid = _valid_points(offsets, total)
    for a in range(n_cams):
        U, gr, gy, acc = np.zeros((6, 6)), np.zeros(6), np.zeros(6), np.zeros((n_cams, 6, 6))
        lo, hi = int(cam_offsets[a]), int(cam_offsets[a + 1])
        if 0 <= lo <= hi <= total:
            for o in (int(v) for v in cam_obs[lo:hi]):
                if not (0 <= o < total and lin["ok"][o] and obs_cam[o] == a):
                    continue
                j = int(obs_point[o])
                if not (0 <= j < len(valid) and valid[j] and offsets[j] <= o < offsets[j + 1]):
                    continue
                Y = lin["W"][o] @ lin["vinv"][j]
                U += lin["Jc"][o].T @ lin["Jc"][o]
                gr += lin["Jc"][o].T @ lin["r"][o]
                gy += Y @ lin["gp"][j]
                track = np.arange(offsets[j], offsets[j + 1])
                track = track[lin["ok"][track]]
                np.add.at(acc, obs_cam[track], np.einsum("rk,tck->trc", Y, lin["W"][track]))       # unbuffered: in track order
        d = np.diag(U).copy()
        U[np.diag_indices(6)] = np.where(np.array([(int(const_mask[a]) >> i) & 1 for i in range(6)], bool) | (d == 0), 1.0, d + lam * d)
        S[a] = -acc.transpose(1, 0, 2)
        S[a, :, a, :] = U - acc[a]
        g[a] = gr - gy
    return S.reshape(6 * n_cams, 6 * n_cams), g.reshape(-1)


def solve_cameras(S, g, const_mask):
    """S dc = -g by Cholesky -> dc, or None where S is not positive definite; a held parameter's step is exactly 0."""
    try:
        L = np.linalg.cholesky(S)
    except np.linalg.LinAlgError:
        return None
    dc = np.linalg.solve(L.T, np.linalg.solve(L, -g))
    held = np.array([[(int(m) >> i) & 1 for i in range(6)] for m in const_mask], bool).reshape(-1)
    return np.where(held, 0.0, dc) if np.isfinite(dc).all() else None


def quat_rotation(w):
    """The trig-free rotation of the update: q = (1, w / 2) / |(1, w / 2)| -> R(q)."""
    h = 0.5 * np.asarray(w, np.float64)
    n = np.sqrt(1.0 + h[0] * h[0] + h[1] * h[1] + h[2] * h[2])
    qw, x, y, z = 1.0 / n, h[0] / n, h[1] / n, h[2] / n
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * qw), 2 * (x * z + y * qw)],
                     [2 * (x * y + z * qw), 1 - 2 * (x * x + z * z), 2 * (y * z - x * qw)],
                     [2 * (x * z - y * qw), 2 * (y * z + x * qw), 1 - 2 * (x * x + y * y)]])


def step(lin, cams, points, offsets, obs_cam, dc):
    """The back-substitution and the update -> candidate cams, candidate points, dX."""
    cams, points = np.asarray(cams, np.float64).reshape(-1, 16), np.asarray(points, np.float64).reshape(-1, 3)
    dc = np.asarray(dc, np.float64).reshape(-1, 6)
    dX = np.zeros_like(points)
    valid = _valid_points(offsets, len(lin["ok"]))
    for j in range(len(points)):
        if not valid[j]:
            continue
        s = lin["gp"][j].copy()
        for o in range(offsets[j], offsets[j + 1]):
            if lin["ok"][o]:
                s = s + lin["W"][o].T @ dc[obs_cam[o]]
        dX[j] = -(lin["vinv"][j] @ s)
    out = cams.copy()
    with np.errstate(all="ignore"):
        for a in range(len(cams)):
            out[a, :9] = (quat_rotation(dc[a, :3]) @ cams[a, :9].reshape(3, 3)).reshape(9)
            out[a, 9:12] = cams[a, 9:12] + dc[a, 3:]
    return out, points + dX, dX


def bundle_adjust(cams, points, offsets, obs_cam, obs_xy, const_mask, max_iterations=BA_MAX_ITERATIONS):
    """The Levenberg-Marquardt loop -> cams, points, report dict(iterations, accepted_steps, initial_cost, final_cost,
    final_lambda, decisions [bool per attempted step]).  `iterations` counts linearisations: the first, one per attempted step
    (the candidate's) and one per rejected step (the old parameters again under the new damping)."""
    cams, points = np.array(cams, np.float64).reshape(-1, 16), np.array(points, np.float64).reshape(-1, 3)
    n_cams = len(cams)
    cam_offsets, cam_obs, obs_point = camera_index(obs_cam, offsets, n_cams)
    lam = BA_LAMBDA0
    lin = linearize(cams, points, offsets, obs_cam, obs_xy, const_mask, lam)
    cost = initial = lin["total_cost"]
    iterations, decisions = 1, []
    while iterations < max_iterations and len(points) and n_cams:
        S, g = reduce_cameras(lin, n_cams, offsets, obs_cam, const_mask, cam_offsets, cam_obs, obs_point, lam)
        dc = solve_cameras(S, g, const_mask)
        lower = max(lam / 10, BA_LAMBDA_MIN)
        iterations += 1
        accepted = False
        if dc is not None:
            cand_cams, cand_points, _ = step(lin, cams, points, offsets, obs_cam, dc)
            cand = linearize(cand_cams, cand_points, offsets, obs_cam, obs_xy, const_mask, lower)
            accepted = bool(np.isfinite(cand["total_cost"]) and cand["total_cost"] < cost)
        decisions.append(accepted)
        if accepted:
            decrease = (cost - cand["total_cost"]) / cost
            cams, points, lin, cost, lam = cand_cams, cand_points, cand, cand["total_cost"], lower
            if decrease < BA_REL_DECREASE:
                break
        else:
            lam = lam * 10
            if lam > BA_LAMBDA_MAX or iterations >= max_iterations:
                break
            lin = linearize(cams, points, offsets, obs_cam, obs_xy, const_mask, lam)
            iterations += 1
    return cams, points, dict(iterations=iterations, accepted_steps=int(sum(decisions)), initial_cost=initial, final_cost=cost,
                              final_lambda=lam, decisions=decisions)


# ---- a grown model -> an adjusted one --------------------------------------------------------------------------------------------------
def gauge_mask(cams, slot_a, slot_b):
    """The first image of the initial pair held entirely; of the second the translation coordinate of largest magnitude
    (the lowest index on ties)  [recalled: COLMAP holds one coordinate of the second image]."""
    mask = np.zeros(len(cams), np.uint8)
    mask[slot_a] = HELD_ALL
    mask[slot_b] = 1 << (3 + int(np.argmax(np.abs(cams[slot_b, 9:12]))))
    return mask


def model_problem(images, grown):
    """The grown model of um.grow_model as the arrays of one adjustment -> ids, cams, points, offsets, obs_cam, obs_xy."""
    ids = sorted(grown["poses"])
    slot = {i: s for s, i in enumerate(ids)}
    cams = np.stack([um.camera_row(*grown["poses"][i], images[i]["K"]) for i in ids])
    offsets = np.concatenate([[0], np.cumsum([len(t) for t in grown["tracks"]])]).astype(np.int32)
    obs_cam = np.array([slot[i] for t in grown["tracks"] for i, _ in t], np.int32)
    obs_xy = np.array([images[i]["keypoints"][kp, :2] for t in grown["tracks"] for i, kp in t], np.float64).reshape(-1, 2)
    return ids, cams, np.asarray(grown["xyz"], np.float64).reshape(-1, 3), offsets, obs_cam, obs_xy


def rescale(cams, points, slot_a, slot_b):
    """Every t and X scaled so that the pair's baseline is 1."""
    centre = [-(cams[s, :9].reshape(3, 3).T @ cams[s, 9:12]) for s in (slot_a, slot_b)]
    scale = 1.0 / np.linalg.norm(centre[1] - centre[0])
    cams = cams.copy()
    cams[:, 9:12] = cams[:, 9:12] * scale
    return cams, points * scale


def filter_tracks(cams, points, offsets, obs_cam, obs_xy, max_error=MAX_ERROR, tan2=um.MIN_TRI_ANGLE_TAN2):
    """-> keep_obs bool (total,): the observations within max_error px under the final poses; keep_point bool (n,): the points
    left with two or more of them, some pair of which passes the parallax test of §4.2j; error (n,): the mean pixel error of
    a kept point's kept observations."""
    total, n = len(obs_cam), len(points)
    keep_obs, keep_point, error = np.zeros(total, bool), np.zeros(n, bool), np.full(n, np.nan)
    for j in range(n):
        sl = slice(offsets[j], offsets[j + 1])
        rows = cams[obs_cam[sl]]
        Xc = np.einsum("nij,j->ni", rows[:, :9].reshape(-1, 3, 3), points[j]) + rows[:, 9:12]
        with np.errstate(all="ignore"):
            p = np.stack([rows[:, 12] * Xc[:, 0] / Xc[:, 2] + rows[:, 14], rows[:, 13] * Xc[:, 1] / Xc[:, 2] + rows[:, 15]], axis=1)
            err = np.where(Xc[:, 2] > 0, np.linalg.norm(p - obs_xy[sl], axis=1), np.inf)
        keep = err <= max_error
        keep_obs[sl] = keep
        if keep.sum() < 2:
            continue
        centres = -np.einsum("nji,nj->ni", rows[keep, :9].reshape(-1, 3, 3), rows[keep, 9:12])
        gq = points[j] - centres
        dots = gq @ gq.T
        cross2 = (np.cross(gq[:, None, :], gq[None, :, :]) ** 2).sum(axis=2)
        if np.any(np.triu(np.ones_like(dots, bool), 1) & ((dots <= 0) | (cross2 >= tan2 * dots * dots))):
            keep_point[j], error[j] = True, float(err[keep].mean())
    keep_obs &= np.repeat(keep_point, np.diff(offsets))
    return keep_obs, keep_point, error


def adjust_model(images, grown, adjust=bundle_adjust):
    """um.grow_model's dict -> the adjusted model: dict(initial_pair, poses, point_ids (1-based ids of the grown model's
    points that are kept), xyz, tracks, error, report, held (cams before, cams after the loop and before the rescale, mask))."""
    ids, cams, points, offsets, obs_cam, obs_xy = model_problem(images, grown)
    slot = {i: s for s, i in enumerate(ids)}
    a, b = (slot[i] for i in grown["initial_pair"])
    mask = gauge_mask(cams, a, b)
    new_cams, new_points, report = adjust(cams, points, offsets, obs_cam, obs_xy, mask)
    scaled_cams, scaled_points = rescale(new_cams, new_points, a, b)
    keep_obs, keep_point, error = filter_tracks(scaled_cams, scaled_points, offsets, obs_cam, obs_xy)
    tracks = [[node for node, k in zip(t, keep_obs[offsets[j]:offsets[j + 1]]) if k] for j, t in enumerate(grown["tracks"])]
    kept = np.nonzero(keep_point)[0]
    return dict(initial_pair=grown["initial_pair"], poses={i: (scaled_cams[s, :9].reshape(3, 3), scaled_cams[s, 9:12]) for i, s in slot.items()},
                point_ids=[int(j) + 1 for j in kept], xyz=scaled_points[kept], tracks=[tracks[j] for j in kept], error=error[kept],
                report=report, held=(cams, new_cams, mask))


# ---- test problems ------------------------------------------------------------------------------------------------------------------------
def random_problem(i, noise=0.5):
    """Problem i of the 300 small ones, from RandomState(15000 + i): 2-12 of the arc cameras, 1-40 points of arc_scene's box,
    each seen by 2 or more of the cameras (all of them when there are two), `noise` px on every pixel, the cameras and the
    points moved off the truth (1e-2 rad, 2e-2, 3e-2 units), the first camera held and one translation coordinate of the
    second -> cams, points, offsets, obs_cam, obs_xy, const_mask."""
    rs = np.random.RandomState(15000 + i)
    poses = um.arc_cameras()
    n_cams, n_points = int(rs.randint(2, 13)), int(rs.randint(1, 41))
    views = np.sort(rs.choice(12, n_cams, replace=False))
    X = np.stack([rs.uniform(-2, 2, n_points), rs.uniform(-1.5, 1.5, n_points), rs.uniform(-1.5, 1.5, n_points)], axis=1)
    obs_cam, obs_xy, lengths = [], [], []
    for j in range(n_points):
        seen = np.sort(rs.choice(n_cams, int(rs.randint(2, n_cams + 1)), replace=False))
        for s in seen:
            R, t = poses[views[s]]
            p = ua.ue.SCENE_K @ (R @ X[j] + t)
            obs_cam.append(s), obs_xy.append(p[:2] / p[2] + rs.normal(0, noise, 2))
        lengths.append(len(seen))
    cams = []
    for s, v in enumerate(views):
        R, t = poses[v]
        if s:
            R, t = ua.rodrigues(rs.normal(0, 1e-2, 3)) @ R, t + rs.normal(0, 2e-2, 3)
        cams.append(um.camera_row(R, t, ua.ue.SCENE_K))
    cams = np.stack(cams)
    return (cams, X + rs.normal(0, 3e-2, X.shape), np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32),
            np.array(obs_cam, np.int32), np.array(obs_xy, np.float64), gauge_mask(cams, 0, 1))


def edge_problems():
    """Problem 7 of `random_problem` grown to the cases a kernel can get wrong, one problem each -> {name: problem}: a slot
    outside the table in the first slot of a track and one in the last, a NaN camera row, a NaN pixel, a point behind a
    camera, points of 0 and of 1 observations, a camera without observations, a track that names one camera twice, a partly
    held camera."""
    base = random_problem(7)
    out = {}

    def variant(name):
        out[name] = [a.copy() for a in base]
        return out[name]

    p = variant("slot_first")
    p[3][p[2][3]] = -1
    p = variant("slot_last")
    p[3][p[2][4] - 1] = len(p[0])
    p = variant("nan_camera")
    p[0][2, 10] = np.nan
    p = variant("nan_pixel")
    p[4][p[2][5], 1] = np.nan
    p = variant("behind")
    flip = np.diag([-1.0, 1.0, -1.0])
    p[0][1, :9], p[0][1, 9:12] = (flip @ p[0][1, :9].reshape(3, 3)).reshape(9), flip @ p[0][1, 9:12]
    p = variant("short_tracks")                                     # a point of no observation first, one of a single observation last
    total = len(p[3])
    p[1] = np.concatenate([[[0.1, 0.2, 0.3]], p[1], [[0.3, 0.2, 0.1]]])
    p[2] = np.concatenate([[0], p[2], [total + 1]]).astype(np.int32)
    p[3] = np.concatenate([p[3], [1]]).astype(np.int32)
    p[4] = np.concatenate([p[4], [[320.0, 240.0]]])
    p = variant("empty_camera")
    p[0] = np.concatenate([p[0], p[0][-1:]])
    p[5] = np.concatenate([p[5], [0]]).astype(np.uint8)
    p = variant("camera_twice")
    lo = p[2][2]
    p[3][lo + 1] = p[3][lo]
    p[4][lo + 1] = p[4][lo] + 0.25
    p = variant("partly_held")
    p[5][2] = 0b001010
    return out
