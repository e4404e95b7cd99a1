"""CPU SPECIFICATION (test infrastructure, NOT product code) of the matrix-free solver of bundle adjustment ("The solver" in
DESIGN.md §4.2k), on top of tests/util_bundle.py: the camera blocks U_a, D_a = S_aa, D_a^-1, g_a and the fixed parameters, the
product q = S p without S, preconditioned conjugate gradients on S dc = -g with the block-Jacobi preconditioner, and the
Levenberg-Marquardt loop of util_bundle.bundle_adjust with that solve in the place of the Cholesky factorisation.  numpy only.

Everything but the solve is util_bundle's, unchanged.  The accumulations are written independently of csrc/bundle.hip (whole
blocks and numpy's unbuffered scatter-add instead of one entry per lane) in the order the rule gives; the 6x6 factorisation is
written out, entry by entry, in the rule's order.
"""
from functools import lru_cache

import numpy as np

import util_absolute_pose as ua
import util_bundle as ub
import util_mapper as um

PCG_REL_TOL = 1e-6                   # |r| <= PCG_REL_TOL |r_0| ends a solve
PCG_MAX_ITERATIONS = 500             # [recalled: Ceres' default max_linear_solver_iterations]
# worst relative difference max|host - spec| / max|spec| of U, D, g, s and q between this specification and the kernels' routines
# compiled for the host (tools/bundle_pcg_host.cpp, -O2 -ffp-contract=off) over the windowed problem, the 300 random problems and
# the edge cases, the fixed flags equal (measured by tests/test_bundle_pcg_spec.py, which prints each figure: s 3.3e-14, g 1.6e-14,
# q 1.1e-14, D 4.0e-15, U 4.2e-16, all on random problems; s and g carry V^-1, whose own figure is util_bundle's 3.4e-14).  D^-1
# is measured apart, 4.6e-12 on random 275: it is the inverse of a block whose condition passes 1e4 there, of a D that already
# differs in its last digits.  Four times either is the project's margin for instruction selection.
HOST_SPEC_REL = 3.3e-14
HOST_SPEC_MINV_REL = 4.7e-12
TOL_REL, TOL_MINV_REL = 4 * HOST_SPEC_REL, 4 * HOST_SPEC_MINV_REL
# the specification against the dense system of util_bundle on the same problems, measured: worst |M^-1 D - I| 1.21e-10 (an entry
# of the product for the worst-conditioned block), worst max|schur_product(p) - S p| / max|S p| 1.45e-14 over three p per problem
# (the two associate the sum differently); the bounds are 4x
MINV_IDENTITY = 1.21e-10
PRODUCT_DENSE_REL = 1.45e-14
# the pcg loop against the dense loop on the windowed problem, measured: the same decisions, final cost 4.07e-15 relative apart
# (each solve ends at |r| <= 1e-6 |r_0|, and at the minimum the cost does not move with the step to first order); 4x
# the host build against this specification on `lists_problem`, whose cameras have lists of up to 520 observations where the
# problems above have up to some 400: measured s 1.87e-14, g 1.43e-14, q 8.0e-16, D 4.8e-16, U 7.6e-17, and D^-1 3.27e-13; 4x
HOST_SPEC_LISTS_REL = 1.87e-14
HOST_SPEC_LISTS_MINV_REL = 3.27e-13
LOOP_DENSE_REL = 4.07e-15
WINDOWED_PCG_ITERATIONS = [47, 47, 48, 47, 48]          # products per solve on the windowed problem (72 unknowns, 65 of them free)
ARC_MAX_ITERATIONS = 6               # linearisations of the arc's loop in the tests: four solves, which take the numpy loop 7 s


def _valid_points(offsets, total):
    lo, hi = np.asarray(offsets[:-1], np.int64), np.asarray(offsets[1:], np.int64)
    return (lo >= 0) & (hi >= lo) & (hi <= total)


def camera_lists(lin, n_cams, offsets, obs_cam, cam_offsets, cam_obs, obs_point):
    """Per camera the usable observations of its list, in list order, as the rule passes over the rest -> [int64 array]."""
    total = len(lin["ok"])
    valid = _valid_points(offsets, total)
    out = []
    for a in range(n_cams):
        lo, hi = int(cam_offsets[a]), int(cam_offsets[a + 1])
        keep = []
        if 0 <= lo <= hi <= total:
            for o in (int(v) for v in cam_obs[lo:hi]):
                if not (0 <= o < total and lin["ok"][o] and obs_cam[o] == a):
                    continue
                j = int(obs_point[o])
                if 0 <= j < len(valid) and valid[j] and offsets[j] <= o < offsets[j + 1]:
                    keep.append(o)
        out.append(np.array(keep, np.int64))
    return out


def cholesky_inverse(D):
    """The symmetric 6x6 D -> D^-1 column by column: D = L L' by rows, L y = e_k, L' x = y, every sum subtracted from its first
    term left to right; the identity where a pivot is not finite and positive."""
    L = np.zeros((6, 6))
    with np.errstate(all="ignore"):
        for j in range(6):
            s = D[j, j]
            for m in range(j):
                s = s - L[j, m] * L[j, m]
            if not (np.isfinite(s) and s > 0):
                return np.eye(6)
            L[j, j] = np.sqrt(s)
            for i in range(j + 1, 6):
                t = D[i, j]
                for m in range(j):
                    t = t - L[i, m] * L[j, m]
                L[i, j] = t / L[j, j]
        inv = np.zeros((6, 6))
        for k in range(6):
            y, x = np.zeros(6), np.zeros(6)
            for i in range(6):
                s = 1.0 if i == k else 0.0
                for m in range(i):
                    s = s - L[i, m] * y[m]
                y[i] = s / L[i, i]
            for i in range(5, -1, -1):
                s = y[i]
                for m in range(i + 1, 6):
                    s = s - L[m, i] * x[m]
                x[i] = s / L[i, i]
            inv[:, k] = x
    return inv


def camera_blocks(lin, n_cams, offsets, obs_cam, const_mask, cam_offsets, cam_obs, obs_point, lam):
    """-> dict(U (n_cams, 6, 6) damped, D (n_cams, 6, 6), Minv (n_cams, 6, 6), g (6 n_cams,), fixed bool (6 n_cams,); what the
    product walks: lists, use, owner)."""
    U, D, Minv = np.zeros((n_cams, 6, 6)), np.zeros((n_cams, 6, 6)), np.zeros((n_cams, 6, 6))
    g, fixed = np.zeros((n_cams, 6)), np.zeros((n_cams, 6), bool)
    lists = camera_lists(lin, n_cams, offsets, obs_cam, cam_offsets, cam_obs, obs_point)
    for a in range(n_cams):
        Ua, gr, gy, acc = np.zeros((6, 6)), np.zeros(6), np.zeros(6), np.zeros((6, 6))
        for o in lists[a]:
            j = int(obs_point[o])
            Y = lin["W"][o] @ lin["vinv"][j]
            Ua += lin["Jc"][o].T @ lin["Jc"][o]
            gr += lin["Jc"][o].T @ lin["r"][o]
            gy += Y @ lin["gp"][j]
            track = np.arange(offsets[j], offsets[j + 1])
            track = track[lin["ok"][track]]
            terms = np.einsum("rk,tck->trc", Y, lin["W"][track])
            for t in np.nonzero(obs_cam[track] == a)[0]:                 # track order; the observation itself and a camera twice included
                acc += terms[t]
        d = np.diag(Ua).copy()
        fixed[a] = np.array([(int(const_mask[a]) >> i) & 1 for i in range(6)], bool) | (d == 0)
        Ua[np.diag_indices(6)] = np.where(fixed[a], 1.0, d + lam * d)
        U[a], D[a] = Ua, Ua - acc
        g[a] = np.where(fixed[a], 0.0, gr - gy)
        Minv[a] = cholesky_inverse(D[a])
    # the usable observations of every point whose offsets delimit a track, point after point in track order, and their points
    valid = _valid_points(offsets, len(lin["ok"]))
    use = np.array([o for j in np.nonzero(valid)[0] for o in range(offsets[j], offsets[j + 1])
                    if lin["ok"][o] and 0 <= obs_cam[o] < n_cams], np.int64)
    owner = np.full(len(lin["ok"]), -1, np.int64)
    for j in np.nonzero(valid)[0]:
        owner[offsets[j]:offsets[j + 1]] = j
    return dict(U=U, D=D, Minv=Minv, g=g.reshape(-1), fixed=fixed.reshape(-1), lists=lists, use=use, owner=owner)


def schur_product(lin, blocks, offsets, obs_cam, obs_point, p):
    """q = S p without S -> s (n_points, 3), q (6 n_cams,).  The points pass adds W_o' p_cam(o) over each track in track order and
    multiplies by V^-1; the cameras pass adds W_o s_point(o) over each camera's list in list order and takes it from U_a p_a."""
    n_cams, n_points = len(blocks["U"]), len(lin["vinv"])
    fixed = blocks["fixed"]
    with np.errstate(all="ignore"):
        e = np.where(fixed, 0.0, np.asarray(p, np.float64)).reshape(n_cams, 6)
        use, owner = blocks["use"], blocks["owner"]
        W, pe = lin["W"][use], e[obs_cam[use]]
        c = W[:, 0, :] * pe[:, 0:1]
        for i in range(1, 6):
            c = c + W[:, i, :] * pe[:, i:i + 1]
        t = np.zeros((n_points, 3))
        np.add.at(t, owner[use], c)                                      # unbuffered: in track order
        V = lin["vinv"]
        s = np.stack([V[:, k, 0] * t[:, 0] + V[:, k, 1] * t[:, 1] + V[:, k, 2] * t[:, 2] for k in range(3)], axis=1)
        order = np.concatenate(blocks["lists"]) if n_cams else np.zeros(0, np.int64)
        cam_of = np.repeat(np.arange(n_cams), [len(v) for v in blocks["lists"]])
        Wo, so = lin["W"][order], s[obs_point[order]]
        ws = Wo[:, :, 0] * so[:, 0:1] + Wo[:, :, 1] * so[:, 1:2] + Wo[:, :, 2] * so[:, 2:3]
        acc = np.zeros((n_cams, 6))
        np.add.at(acc, cam_of, ws)                                       # unbuffered: in list order
        U = blocks["U"]
        up = U[:, :, 0] * e[:, 0:1]
        for k in range(1, 6):
            up = up + U[:, :, k] * e[:, k:k + 1]
        q = np.where(fixed, np.asarray(p, np.float64), (up - acc).reshape(-1))
    return s, q


def apply_preconditioner(blocks, r):
    return np.einsum("aik,ak->ai", blocks["Minv"], r.reshape(-1, 6)).reshape(-1)


def pcg_solve(lin, blocks, offsets, obs_cam, obs_point, tol=PCG_REL_TOL, max_iterations=PCG_MAX_ITERATIONS, product=None):
    """S x = -g by preconditioned conjugate gradients -> (x or None where the solve ended on a p'q that is not finite and
    positive or on a non-finite x, the number of products)."""
    product = product or (lambda p: schur_product(lin, blocks, offsets, obs_cam, obs_point, p)[1])
    fixed = blocks["fixed"]
    with np.errstate(all="ignore"):
        x = np.zeros(len(fixed))
        r = np.where(fixed, 0.0, -blocks["g"])
        r0 = np.sqrt(r @ r)
        if r0 == 0:
            return x, 0
        if not np.isfinite(r0):
            return None, 0
        z = apply_preconditioner(blocks, r)
        p, rz = z.copy(), r @ z
        for k in range(1, max_iterations + 1):
            q = product(p)
            pq = p @ q
            if not (np.isfinite(pq) and pq > 0):
                return None, k
            alpha = rz / pq
            x = x + alpha * p
            r = r - alpha * q
            if not np.isfinite(x).all():
                return None, k
            if np.sqrt(r @ r) <= tol * r0 or k == max_iterations:
                return np.where(fixed, 0.0, x), k
            z = apply_preconditioner(blocks, r)
            rz_new = r @ z
            p, rz = z + (rz_new / rz) * p, rz_new
    return np.where(fixed, 0.0, x), max_iterations


def bundle_adjust(cams, points, offsets, obs_cam, obs_xy, const_mask, max_iterations=ub.BA_MAX_ITERATIONS, tol=PCG_REL_TOL,
                  pcg_max_iterations=PCG_MAX_ITERATIONS, linearize=ub.linearize):
    """util_bundle.bundle_adjust with pcg_solve in the place of reduce_cameras + solve_cameras; the report gains solver and
    pcg_iterations (one count per solve).  `linearize`: the linearisation (tests/util_bundle_loss.py's under a loss)."""
    cams, points = np.array(cams, np.float64).reshape(-1, 16), np.array(points, np.float64).reshape(-1, 3)
    n_cams = len(cams)
    index = ub.camera_index(obs_cam, offsets, n_cams)
    lam = ub.BA_LAMBDA0
    lin = linearize(cams, points, offsets, obs_cam, obs_xy, const_mask, lam)
    cost = initial = lin["total_cost"]
    iterations, decisions, counts = 1, [], []
    while iterations < max_iterations and len(points) and n_cams:
        blocks = camera_blocks(lin, n_cams, offsets, obs_cam, const_mask, *index, lam)
        dc, k = pcg_solve(lin, blocks, offsets, obs_cam, index[2], tol, pcg_max_iterations)
        counts.append(k)
        lower = max(lam / 10, ub.BA_LAMBDA_MIN)
        iterations += 1
        accepted = False
        if dc is not None:
            cand_cams, cand_points, _ = ub.step(lin, cams, points, offsets, obs_cam, dc)
            cand = linearize(cand_cams, cand_points, offsets, obs_cam, obs_xy, const_mask, lower)
            accepted = bool(np.isfinite(cand["total_cost"]) and cand["total_cost"] < cost)
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
            lin = linearize(cams, points, offsets, obs_cam, obs_xy, const_mask, lam)
            iterations += 1
    return cams, points, dict(iterations=iterations, accepted_steps=int(sum(decisions)), initial_cost=initial, final_cost=cost,
                              final_lambda=lam, decisions=decisions, solver="pcg", pcg_iterations=counts)


@lru_cache(maxsize=None)
def arc_spec():
    """The loop above on `arc_problem`, ARC_MAX_ITERATIONS linearisations at most (computed once; the CPU and the GPU tests share it)
    -> cams, points, report."""
    return bundle_adjust(*arc_problem(), max_iterations=ARC_MAX_ITERATIONS)


# ---- test problems ------------------------------------------------------------------------------------------------------------------------
ARC_K = np.array([[600.0, 0, 320.0], [0, 600.0, 240.0], [0, 0, 1]])
ARC_CAMS, ARC_POINTS = 520, 1000     # 2600 points take the numpy loop a minute; 1000 still give every camera its points


def arc_problem(n_cams=ARC_CAMS, n_points=ARC_POINTS, seed=1, noise=0.5):
    """The arc of tools/bench_bundle.py restated: n_cams cameras 0.5 degrees apart on a circle of radius 8 looking at the origin,
    n_points points of the box each seen by 3-8 cameras four apart around a centre that walks along the whole arc (so that every camera
    sees points; tools/bench_bundle.py draws the starts and leaves the last cameras empty), `noise` px on every pixel, the translations 5e-3 and the points 1e-2 off the truth, camera 0 held and one
    translation coordinate of camera 1 -> cams, points, offsets, obs_cam, obs_xy, const_mask."""
    rs = np.random.RandomState(seed)
    rows = []
    for a in np.radians(0.5 * (np.arange(n_cams) - n_cams / 2)):
        c = np.array([8.0 * np.sin(a), 0.2 * np.cos(5 * a), -8.0 * np.cos(a)])
        z = -c / np.linalg.norm(c)
        x = np.cross([0.0, 1.0, 0.0], z)
        x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z])
        rows.append(np.concatenate([R.reshape(9), -R @ c, [ARC_K[0, 0], ARC_K[1, 1], ARC_K[0, 2], ARC_K[1, 2]]]))
    cams = np.stack(rows)
    lengths = rs.randint(3, 9, n_points)
    offsets = np.concatenate([[0], np.cumsum(lengths)])
    point_of = np.repeat(np.arange(n_points), lengths)
    # a point's cameras: every fourth camera around a centre that walks along the whole arc, shifted inside by fours where the arc ends
    centre = (np.arange(n_points) * n_cams) // n_points
    first = centre - 4 * (lengths // 2)
    first = first + 4 * ((np.maximum(-first, 0) + 3) // 4)
    first = first - 4 * ((np.maximum(first + 4 * (lengths - 1) - (n_cams - 1), 0) + 3) // 4)
    obs_cam = (first[point_of] + 4 * (np.arange(offsets[-1]) - offsets[:-1][point_of])).astype(np.int32)
    X = np.stack([rs.uniform(-2, 2, n_points), rs.uniform(-1.5, 1.5, n_points), rs.uniform(-1.5, 1.5, n_points)], axis=1)
    Xc = np.einsum("nij,nj->ni", cams[obs_cam, :9].reshape(-1, 3, 3), X[point_of]) + cams[obs_cam, 9:12]
    obs_xy = np.stack([ARC_K[0, 0] * Xc[:, 0] / Xc[:, 2] + ARC_K[0, 2], ARC_K[1, 1] * Xc[:, 1] / Xc[:, 2] + ARC_K[1, 2]], axis=1)
    obs_xy = obs_xy + rs.normal(0, noise, (len(obs_cam), 2))
    moved = cams.copy()
    moved[1:, 9:12] += rs.normal(0, 5e-3, (n_cams - 1, 3))
    mask = np.zeros(n_cams, np.uint8)
    mask[0], mask[1] = ub.HELD_ALL, 1 << (3 + int(np.argmax(np.abs(cams[1, 9:12]))))
    return moved, X + rs.normal(0, 1e-2, X.shape), offsets.astype(np.int32), obs_cam, obs_xy, mask


LISTS = (1, 63, 64, 65, 130, 255, 256, 257, 520, 520)    # observations per camera: both camera passes' batches (64, 256) crossed and part-filled


@lru_cache(maxsize=None)
def lists_problem():
    """Ten cameras whose lists have LISTS observations: camera a sees the first LISTS[a] of 520 points, 0.5 px noise, the points
    0.03 off the truth, the last camera held.  The points past 257 are seen by the last two cameras only."""
    rs = np.random.RandomState(19000)
    n = len(LISTS)
    cams = np.stack([um.camera_row(*ua.look_at(np.array([8.0 * np.sin(a), 0.2 * np.cos(5 * a), -8.0 * np.cos(a)]), np.zeros(3)), ua.ue.SCENE_K)
                     for a in np.radians(4.0 * np.arange(n) - 20.0)])
    n_points = max(LISTS)
    X = np.stack([rs.uniform(-2, 2, n_points), rs.uniform(-1.5, 1.5, n_points), rs.uniform(-1.5, 1.5, n_points)], axis=1)
    seen = [np.array([a for a in range(n) if LISTS[a] > j], np.int32) for j in range(n_points)]
    obs_cam = np.concatenate(seen)
    offsets = np.concatenate([[0], np.cumsum([len(v) for v in seen])]).astype(np.int32)
    Xc = np.einsum("nij,nj->ni", cams[obs_cam, :9].reshape(-1, 3, 3), np.repeat(X, np.diff(offsets), axis=0)) + cams[obs_cam, 9:12]
    obs_xy = ua.ue.SCENE_K[0, 0] * Xc[:, :2] / Xc[:, 2:] + ua.ue.SCENE_K[:2, 2] + rs.normal(0, 0.5, (len(obs_cam), 2))
    mask = np.zeros(n, np.uint8)
    mask[n - 1] = ub.HELD_ALL
    return cams, X + rs.normal(0, 0.03, X.shape), offsets, obs_cam, obs_xy, mask
