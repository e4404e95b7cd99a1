"""CPU SPECIFICATION (test infrastructure, NOT product code) of image registration: the minimal P3P
absolute-pose solver, the float32 scoring of pose hypotheses against 2D-3D correspondences, the RANSAC rule with its refit
and acceptance test (`estimate_absolute_pose`) and the seed model (`seed_model`).  numpy only; the sampler is
oracle/two_view_oracle.py's, the triangulation tests/util_pose.py's.

The solver's route differs from the kernel's (csrc/absolute_pose.hip), so agreement between the two is a test of both.  Both
start from the three law-of-cosines equations in the depths s1, s2, s3 along the unit rays and substitute s2 = u s1,
s3 = v s1, which leaves two conics in (u, v).
  kernel  subtracts the conics (linear in v), substitutes v(u) and finds the real roots of a quartic in u by bracketing and
          bisection; (R, t) from two orthonormal frames on the triangles
  here    the Sylvester resultant of the two conics with respect to u, a quartic in v; roots by `numpy.roots` (companion
          matrix eigenvalues); u from the conics' common root; a Gauss-Newton polish of (s1, s2, s3) on the three distance
          equations; (R, t) by Procrustes with an SVD
This is the build's own published rule: parity with COLMAP's absolute-pose estimator is unpinned.
"""
import numpy as np

from oracle import two_view_oracle as tv
import util_essential as ue
import util_pose as up

SALT_P = 0x96969696
NUM_HYP_P = 128
MAX_SOLUTIONS = 4
ABS_POSE_MAX_ERROR = 12.0            # px  [recalled: COLMAP IncrementalMapperOptions default]
ABS_POSE_MIN_NUM_INLIERS = 30        #     [recalled: COLMAP IncrementalMapperOptions default]
ABS_POSE_MIN_INLIER_RATIO = 0.25     #     [recalled: COLMAP IncrementalMapperOptions default]
INIT_MIN_TRI_ANGLE = np.radians(16.0)    # [recalled: COLMAP IncrementalMapperOptions default]
INIT_MIN_NUM_INLIERS = 100           #     [recalled: COLMAP IncrementalMapperOptions default]
FILTER_MIN_TRI_ANGLE = np.radians(1.5)   # [recalled: COLMAP IncrementalMapperOptions default]
REFIT_STEPS = 10
PARALLEL_TOL = 1e-20                 # squared sine below which two rays / two triangle sides count as parallel
POLISH_STEPS = 3
# worst distance (Frobenius on R + 2-norm on t) of the nearest solution to the true pose over the 300 minimal problems:
# 7.9e-9 without the polish, 2.9e-12 with it (measured; tests/test_absolute_pose_spec.py asserts the bound)
SPEC_TRUTH_DISTANCE = 2.9e-12
# worst matched distance between this specification and the kernel's solver functions compiled for the host
# (tools/p3p_host.cpp, -O2 -ffp-contract=off) over the same 300 problems, no problem unmatched (measured: 6.98e-12)
HOST_SPEC_DISTANCE = 7.0e-12
# what the GPU test allows between a kernel solution and its match: 4x the larger of the two, for the differences in libm
# and instruction selection between host and device (the algebra is the same)
TOL_POSE = 4 * max(HOST_SPEC_DISTANCE, SPEC_TRUTH_DISTANCE)


# ---- the minimal solver ---------------------------------------------------------------------------------------------------------
def _degenerate(f, X):
    """Unit rays f (3, 3), world points X (3, 3): non-finite input, two coincident points or rays, collinear points."""
    if not (np.all(np.isfinite(f)) and np.all(np.isfinite(X))):
        return True
    for i, j in ((0, 1), (0, 2), (1, 2)):
        c = np.cross(f[i], f[j])
        if not c @ c > PARALLEL_TOL:
            return True
        d = X[i] - X[j]
        if not d @ d > 0:
            return True
    e1, e2 = X[1] - X[0], X[2] - X[0]
    n = np.cross(e1, e2)
    return not n @ n > PARALLEL_TOL * (e1 @ e1) * (e2 @ e2)


def _polish_depths(s, c12, c13, c23, d12, d13, d23, steps=POLISH_STEPS):
    """Newton on the three distance equations from the depths s (3,); a step is kept only if it lowers the residual."""
    def res(s):
        return np.array([s[0] * s[0] + s[1] * s[1] - 2 * s[0] * s[1] * c12 - d12,
                         s[0] * s[0] + s[2] * s[2] - 2 * s[0] * s[2] * c13 - d13,
                         s[1] * s[1] + s[2] * s[2] - 2 * s[1] * s[2] * c23 - d23])

    r = res(s)
    for _ in range(steps):
        J = np.array([[2 * s[0] - 2 * s[1] * c12, 2 * s[1] - 2 * s[0] * c12, 0.0],
                      [2 * s[0] - 2 * s[2] * c13, 0.0, 2 * s[2] - 2 * s[0] * c13],
                      [0.0, 2 * s[1] - 2 * s[2] * c23, 2 * s[2] - 2 * s[1] * c23]])
        try:
            s2 = s - np.linalg.solve(J, r)
        except np.linalg.LinAlgError:
            break
        r2 = res(s2)
        if not r2 @ r2 < r @ r:
            break
        s, r = s2, r2
    return s


def _procrustes(Xw, Xc):
    """(R, t) with Xc_i = R Xw_i + t in the least-squares sense, R in SO(3)."""
    mw, mc = Xw.mean(axis=0), Xc.mean(axis=0)
    U, _, Vt = np.linalg.svd((Xc - mc).T @ (Xw - mw))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt)) or 1.0])
    R = U @ D @ Vt
    return R, mc - R @ mw


def p3p(x, X, polish=True):
    """x (3, 2) normalised image points, X (3, 3) world points -> list of (R, t) with X_cam = R X + t, at most 4, ascending in
    the root variable v = s3 / s1."""
    x, X = np.asarray(x, np.float64).reshape(3, 2), np.asarray(X, np.float64).reshape(3, 3)
    with np.errstate(all="ignore"):
        f = np.concatenate([x, np.ones((3, 1))], axis=1)
        f = f / np.linalg.norm(f, axis=1, keepdims=True)
        if _degenerate(f, X):
            return []
        c12, c13, c23 = f[0] @ f[1], f[0] @ f[2], f[1] @ f[2]
        d12, d13, d23 = ((X[0] - X[1]) ** 2).sum(), ((X[0] - X[2]) ** 2).sum(), ((X[1] - X[2]) ** 2).sum()
        A, B = d13 / d12, d23 / d12
        # two quadratics in u whose coefficients are polynomials in v (numpy.poly1d, highest power first)
        #   A (1 + u^2 - 2 u c12) = 1 + v^2 - 2 v c13        B (1 + u^2 - 2 u c12) = u^2 + v^2 - 2 u v c23
        P = np.poly1d
        a2, a1, a0 = P([A]), P([-2 * A * c12]), P([-1.0, 2 * c13, A - 1.0])
        b2, b1, b0 = P([B - 1.0]), P([2 * c23, -2 * B * c12]), P([-1.0, 0.0, B])
        m20, m21, m10 = a2 * b0 - a0 * b2, a2 * b1 - a1 * b2, a1 * b0 - a0 * b1
        resultant = m20 * m20 - m21 * m10
        coeffs = np.zeros(5)
        coeffs[5 - len(resultant.coeffs):] = resultant.coeffs
        if not np.all(np.isfinite(coeffs)) or not np.any(coeffs):
            return []
        roots = np.roots(coeffs)
    out = []
    for v in sorted(r.real for r in roots if abs(r.imag) <= 1e-9 * max(1.0, abs(r))):
        with np.errstate(all="ignore"):
            if not v > 0:
                continue
            u = -m20(v) / m21(v)                                    # the common root of the two quadratics
            if not (np.isfinite(u) and u > 0):
                continue
            s1 = np.sqrt(d12 / (1 + u * u - 2 * u * c12))
            s = np.array([s1, u * s1, v * s1])
            if polish:
                s = _polish_depths(s, c12, c13, c23, d12, d13, d23)
            if not (np.all(np.isfinite(s)) and np.all(s > 0)):
                continue
            R, t = _procrustes(X, f * s[:, None])
        if np.all(np.isfinite(R)) and np.all(np.isfinite(t)) and abs(np.linalg.det(R) - 1) < 1e-9:
            if not any(pose_distance(R, t, R2, t2) < 1e-9 for R2, t2 in out):      # a double root reported twice
                out.append((R, t))
    return out[:MAX_SOLUTIONS]


def pose_distance(R1, t1, R2, t2):
    """Frobenius norm on R plus the 2-norm on t."""
    return float(np.linalg.norm(np.asarray(R1) - np.asarray(R2)) + np.linalg.norm(np.asarray(t1) - np.asarray(t2)))


def minimal_problem(i):
    """Three exact float64 2D-3D correspondences under the pose (SCENE_R, SCENE_T), from RandomState(9000 + i): camera-frame
    points uniform in [-1.5, 1.5] x [-1, 1] x [2, 6] -> x (3, 2) normalised image points, X (3, 3) world points."""
    rs = np.random.RandomState(9000 + i)
    Xc = np.stack([rs.uniform(-1.5, 1.5, 3), rs.uniform(-1, 1, 3), rs.uniform(2, 6, 3)], axis=1)
    X = (Xc - ue.SCENE_T) @ ue.SCENE_R                               # R' (Xc - t)
    return Xc[:, :2] / Xc[:, 2:], X


def exact_problem(n, seed=77):
    """n exact correspondences under (SCENE_R, SCENE_T) -> x (n, 2) normalised, X (n, 3)."""
    rs = np.random.RandomState(seed)
    Xc = np.stack([rs.uniform(-1.5, 1.5, n), rs.uniform(-1, 1, n), rs.uniform(2, 6, n)], axis=1)
    return Xc[:, :2] / Xc[:, 2:], (Xc - ue.SCENE_T) @ ue.SCENE_R


# ---- scoring: float32, no division, this order of single operations ------------------------------------------------------------
def projection_matrix(K, R, t):
    """P = K [R | t] for a K without skew, float64 in a fixed order (row 0: fx r0 + cx r2, row 1: fy r1 + cy r2, row 2: r2),
    rounded to float32 (12,)."""
    Rt = np.concatenate([np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3, 1)], axis=1)
    with np.errstate(all="ignore"):
        P = np.stack([K[0, 0] * Rt[0] + K[0, 2] * Rt[2], K[1, 1] * Rt[1] + K[1, 2] * Rt[2], Rt[2]])
        return P.reshape(12).astype(np.float32)


def inliers(P34, obs, xyz, max_error=ABS_POSE_MAX_ERROR):
    """P34 float32 (12,) row-major pixel projection, obs (n, 2) px, xyz (n, 3) -> bool (n,): p = P (X, 1); inlier iff p_w > 0
    and |p_xy - obs p_w|^2 <= e^2 p_w^2."""
    m = np.asarray(P34, np.float32).reshape(12)
    obs, xyz = np.asarray(obs, np.float32).reshape(-1, 2), np.asarray(xyz, np.float32).reshape(-1, 3)
    x, y, z, ox, oy = xyz[:, 0], xyz[:, 1], xyz[:, 2], obs[:, 0], obs[:, 1]
    e = np.float32(max_error)
    t2 = e * e
    with np.errstate(all="ignore"):
        p0 = m[0] * x + m[1] * y + m[2] * z + m[3]
        p1 = m[4] * x + m[5] * y + m[6] * z + m[7]
        pw = m[8] * x + m[9] * y + m[10] * z + m[11]
        dx = p0 - ox * pw
        dy = p1 - oy * pw
        return (pw > 0) & (dx * dx + dy * dy <= t2 * (pw * pw))        # NaN compares false


def score(P34, obs, xyz, max_error=ABS_POSE_MAX_ERROR):
    return int(inliers(P34, obs, xyz, max_error).sum())


# ---- the rule for one problem -----------------------------------------------------------------------------------------------------
def rodrigues(w):
    th = np.linalg.norm(w)
    W = ue.skew(w)
    if th < 1e-12:
        return np.eye(3) + W
    return np.eye(3) + np.sin(th) / th * W + (1 - np.cos(th)) / (th * th) * (W @ W)


def _reprojection(K, R, t, obs, xyz):
    Xc = xyz @ R.T + t
    with np.errstate(all="ignore"):
        r = np.stack([K[0, 0] * Xc[:, 0] / Xc[:, 2] + K[0, 2] - obs[:, 0], K[1, 1] * Xc[:, 1] / Xc[:, 2] + K[1, 2] - obs[:, 1]], axis=1)
    return Xc, r


def refit_pose(K, R, t, obs, xyz, steps=REFIT_STEPS):
    """At most `steps` Gauss-Newton steps on (rotation vector, t), R <- exp(w) R, minimising the pixel reprojection error over
    the given correspondences; a step is kept only if it lowers the cost."""
    obs, xyz = np.asarray(obs, np.float64), np.asarray(xyz, np.float64)
    Xc, r = _reprojection(K, R, t, obs, xyz)
    cost = (r * r).sum()
    for _ in range(steps):
        with np.errstate(all="ignore"):
            iz = 1.0 / Xc[:, 2]
            du = np.stack([K[0, 0] * iz, np.zeros_like(iz), -K[0, 0] * Xc[:, 0] * iz * iz], axis=1)      # d u / d Xc
            dv = np.stack([np.zeros_like(iz), K[1, 1] * iz, -K[1, 1] * Xc[:, 1] * iz * iz], axis=1)
            Y = xyz @ R.T                                                                               # d Xc / d w = -[R X]x
            J = np.concatenate([np.stack([np.cross(Y, du), du], axis=1).reshape(-1, 6)[:, None, :],
                                np.stack([np.cross(Y, dv), dv], axis=1).reshape(-1, 6)[:, None, :]], axis=1).reshape(-1, 6)
        if not np.all(np.isfinite(J)):
            break
        try:
            step = np.linalg.solve(J.T @ J, -J.T @ r.reshape(-1))
        except np.linalg.LinAlgError:
            break
        R2, t2 = rodrigues(step[:3]) @ R, t + step[3:]
        Xc2, r2 = _reprojection(K, R2, t2, obs, xyz)
        cost2 = (r2 * r2).sum()
        if not cost2 < cost:
            break
        R, t, Xc, r, cost = R2, t2, Xc2, r2, cost2
    return R, t


def normalise_obs(obs, K):
    Ki = np.linalg.inv(K)
    p = np.asarray(obs, np.float64)
    return p * [Ki[0, 0], Ki[1, 1]] + [Ki[0, 2], Ki[1, 2]]


def estimate_absolute_pose(obs, xyz, K, seed, n_hyp=NUM_HYP_P, max_error=ABS_POSE_MAX_ERROR, perturb=None):
    """obs (n, 2) px, xyz (n, 3), K (3, 3) -> dict(success, R, t, qvec, tvec, num_inliers, inlier_mask).
    `perturb(R, t) -> (R, t)` (tests only) moves every solver solution before it is scored."""
    obs32, xyz32 = np.asarray(obs, np.float32).reshape(-1, 2), np.asarray(xyz, np.float32).reshape(-1, 3)
    n = len(obs32)
    fail = dict(success=False, R=np.eye(3), t=np.zeros(3), qvec=np.array([1.0, 0, 0, 0]), tvec=np.zeros(3), num_inliers=0,
                inlier_mask=np.zeros(n, bool))
    if n < 3:
        return fail
    xn, X = normalise_obs(obs32, K), xyz32.astype(np.float64)
    idx = tv.sample_indices(int(seed) & 0xFFFFFFFF, n_hyp, 3, n, SALT_P)
    best_n, best = 0, None
    for k in range(n_hyp):
        if idx[k, 0] < 0:
            continue
        for R, t in p3p(xn[idx[k]], X[idx[k]]):
            if perturb is not None:
                R, t = perturb(R, t)
            c = score(projection_matrix(K, R, t), obs32, xyz32, max_error)
            if c > best_n:                                          # most inliers, lowest (sample, solution) on ties
                best_n, best = c, (R, t)
    if best is None:
        return fail
    R, t = best
    mask = inliers(projection_matrix(K, R, t), obs32, xyz32, max_error)
    Rr, tr = refit_pose(K, R, t, obs32[mask].astype(np.float64), X[mask])
    if np.all(np.isfinite(Rr)) and np.all(np.isfinite(tr)):
        rmask = inliers(projection_matrix(K, Rr, tr), obs32, xyz32, max_error)
        if rmask.sum() >= mask.sum():
            R, t, mask = Rr, tr, rmask
    num = int(mask.sum())
    ok = num >= ABS_POSE_MIN_NUM_INLIERS and num / n >= ABS_POSE_MIN_INLIER_RATIO
    return dict(success=bool(ok), R=R, t=t, qvec=ue.rot_to_quat(R), tvec=np.asarray(t, np.float64).copy(), num_inliers=num,
                inlier_mask=mask)


def registration_problem(seed, n, outlier_frac, noise=0.5, R=None, t=None):
    """n correspondences under (SCENE_R, SCENE_T), or the pose (R, t) given, and SCENE_K with pixel noise; an outlier observes
    a uniform random pixel -> obs float32 (n, 2), xyz float32 (n, 3), the inlier flags.  Under a pose that is given, a point
    not at least 0.5 in front of the camera is drawn again."""
    rs = np.random.RandomState(seed)
    X = np.stack([rs.uniform(-3, 3, n), rs.uniform(-2, 2, n), rs.uniform(4, 9, n)], axis=1)
    given = R is not None or t is not None
    R, t = ue.SCENE_R if R is None else np.asarray(R, np.float64), ue.SCENE_T if t is None else np.asarray(t, np.float64)
    while given:                                                     # the default scene draws exactly what it always drew
        behind = (X @ R.T + t)[:, 2] < 0.5
        if not behind.any():
            break
        k = int(behind.sum())
        X[behind] = np.stack([rs.uniform(-3, 3, k), rs.uniform(-2, 2, k), rs.uniform(4, 9, k)], axis=1)
    Xc = X @ R.T + t
    p = (ue.SCENE_K @ Xc.T).T
    obs = p[:, :2] / p[:, 2:] + rs.normal(0, noise, (n, 2))
    is_in = rs.uniform(size=n) >= outlier_frac
    wrong = np.stack([rs.uniform(0, 640, n), rs.uniform(0, 480, n)], axis=1)
    obs = np.where(is_in[:, None], obs, wrong)
    return obs.astype(np.float32), X.astype(np.float32), is_in


def pose_error(R, t, R_true=ue.SCENE_R, t_true=ue.SCENE_T):
    """-> (rotation error in degrees, distance between the camera centres)."""
    c = np.clip((np.trace(R.T @ R_true) - 1) / 2, -1, 1)
    return float(np.degrees(np.arccos(c))), float(np.linalg.norm(-R.T @ t + R_true.T @ t_true))


# ---- the seed model on plain arrays --------------------------------------------------------------------------------------------
def _directed(pairs, i, j):
    """The geometry of (i -> j) from a table keyed (lower id, higher id): match columns (i, j), X_j = R X_i + t."""
    g = pairs.get((min(i, j), max(i, j)))
    if g is None:
        return None
    m, q, t = np.asarray(g["inlier_matches"], np.int64).reshape(-1, 2), np.asarray(g["qvec"], np.float64), np.asarray(g["tvec"], np.float64)
    R = quat_to_rot(q)
    if i > j:
        m, R, t = m[:, ::-1], R.T, -R.T @ t
    return dict(config=g["config"], matches=m, R=R, t=t)


def quat_to_rot(q):
    w, x, y, z = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def point_angles(X, centre):
    """Angle at each point X (n, 3) between the rays to the origin and to `centre`."""
    e = X - centre
    k = np.cross(X, e)
    return np.arctan2(np.linalg.norm(k, axis=1), (X * e).sum(axis=1))


def pixel_errors(K, R, t, xyz, obs):
    Xc = xyz @ R.T + t
    with np.errstate(all="ignore"):
        p = np.stack([K[0, 0] * Xc[:, 0] / Xc[:, 2] + K[0, 2], K[1, 1] * Xc[:, 1] / Xc[:, 2] + K[1, 2]], axis=1)
        err = np.linalg.norm(p - obs, axis=1)
    return np.where(Xc[:, 2] > 0, err, np.inf)


def seed_model(images, pairs, estimate=estimate_absolute_pose):
    """images: {image_id: dict(K (3, 3) or None where the camera has no usable prior, keypoints (n, 2))};
    pairs: {(i, j), i < j: dict(config, qvec, tvec, inlier_matches (m, 2))}, X_j = R X_i + t
    -> dict(initial_pair (a, b), poses {image_id: (R, t)}, xyz (n, 3), tracks [list of (image_id, keypoint index)]).
    Raises ValueError when no pair can start the model."""
    cands = []
    for (i, j), g in sorted(pairs.items()):
        if g["config"] != tv.CONFIG_CALIBRATED or not np.any(g["tvec"]) or len(g["inlier_matches"]) < INIT_MIN_NUM_INLIERS:
            continue
        if images[i]["K"] is None or images[j]["K"] is None:
            continue
        cands.append((i, j))
    if not cands:
        raise ValueError("seed model: no CALIBRATED pair with a translation, two focal-length priors and at least "
                         f"{INIT_MIN_NUM_INLIERS} inliers")
    best = None
    for i, j in cands:
        d = _directed(pairs, i, j)
        kp1, kp2 = images[i]["keypoints"], images[j]["keypoints"]
        pts = np.concatenate([kp1[d["matches"][:, 0], :2], kp2[d["matches"][:, 1], :2]], axis=1).astype(np.float32)
        xn = up.normalise(pts, images[i]["K"], images[j]["K"])
        cand = np.full((4, 12), np.nan)
        cand[0, :9], cand[0, 9:] = d["R"].reshape(9), d["t"]
        counts, _, tri, X = up.choose(xn, cand)
        if tri >= INIT_MIN_TRI_ANGLE and (best is None or counts[0] > best[0]):       # lowest pair id on ties
            best = (int(counts[0]), (i, j), d, X, pts)
    if best is None:
        raise ValueError(f"seed model: no candidate pair reaches a triangulation angle of {np.degrees(INIT_MIN_TRI_ANGLE):.0f} degrees")
    _, (a, b), d, X, pts = best
    Ka, Kb = images[a]["K"], images[b]["K"]
    centre_b = -d["R"].T @ d["t"]
    front = np.isfinite(X).all(axis=1)
    Xs = np.where(front[:, None], X, 1.0)
    keep = front & (point_angles(Xs, centre_b) >= FILTER_MIN_TRI_ANGLE)
    keep &= pixel_errors(Ka, np.eye(3), np.zeros(3), Xs, pts[:, :2].astype(np.float64)) <= tv.MAX_ERROR
    keep &= pixel_errors(Kb, d["R"], d["t"], Xs, pts[:, 2:].astype(np.float64)) <= tv.MAX_ERROR
    xyz = X[keep]
    tracks = [[(a, int(m[0])), (b, int(m[1]))] for m in d["matches"][keep]]
    point_of = {a: {int(m[0]): k for k, m in enumerate(d["matches"][keep])}, b: {int(m[1]): k for k, m in enumerate(d["matches"][keep])}}
    poses = {a: (np.eye(3), np.zeros(3)), b: (d["R"], d["t"])}
    for c in sorted(images):
        if c in (a, b) or images[c]["K"] is None:
            continue
        used, kp_idx, pt_idx = set(), [], []
        for other in (a, b):
            g = _directed(pairs, c, other)
            if g is None:
                continue
            for kc, ko in g["matches"]:
                k = point_of[other].get(int(ko))
                if k is not None and int(kc) not in used:
                    used.add(int(kc)), kp_idx.append(int(kc)), pt_idx.append(k)
        if len(kp_idx) < ABS_POSE_MIN_NUM_INLIERS:
            continue
        obs = images[c]["keypoints"][kp_idx, :2]
        r = estimate(obs, xyz[pt_idx], images[c]["K"], c)
        if not r["success"]:
            continue
        poses[c] = (quat_to_rot(r["qvec"]), np.asarray(r["tvec"], np.float64))
        for kc, k, ok in zip(kp_idx, pt_idx, r["inlier_mask"]):
            if ok:
                tracks[k].append((c, kc))
    return dict(initial_pair=(a, b), poses=poses, xyz=xyz, tracks=tracks)


# ---- a synthetic multi-view scene -------------------------------------------------------------------------------------------------
def look_at(centre, target):
    z = target - centre
    z = z / np.linalg.norm(z)
    x = np.cross([0.0, 1.0, 0.0], z)
    x = x / np.linalg.norm(x)
    R = np.stack([x, np.cross(z, x), z])                             # rows: the camera axes in the world
    return R, -R @ centre


def arc_scene(seed=5, n_views=5, n_points=200, noise=0.3, unmatched=0.2, duplicate=False, step_deg=18.0):
    """n_views PINHOLE 640x480 cameras (SCENE_K) on an arc around n_points non-planar points -> dict(K, poses [(R, t)] world ->
    camera, X (n_points, 3), keypoints [float32 (n_points, 2)], visible [bool (n_points,)]): keypoint i of every view observes
    point i; where `visible` is False the keypoint is a uniform random pixel (an unmatched keypoint).  `duplicate`: every view
    is view 0 (no baseline anywhere); `step_deg`: the angle of the arc between neighbouring views."""
    rs = np.random.RandomState(seed)
    X = np.stack([rs.uniform(-2, 2, n_points), rs.uniform(-1.5, 1.5, n_points), rs.uniform(-1.5, 1.5, n_points)], axis=1)
    poses, kps, vis = [], [], []
    for v in range(n_views):
        ang = 0.0 if duplicate else np.radians(step_deg * (v - 2))
        centre = np.array([8.0 * np.sin(ang), 0.3 * (0 if duplicate else v), -8.0 * np.cos(ang)])
        R, t = look_at(centre, np.zeros(3))
        p = (ue.SCENE_K @ (X @ R.T + t).T).T
        kp = p[:, :2] / p[:, 2:] + rs.normal(0, noise, (n_points, 2))
        seen = rs.uniform(size=n_points) >= unmatched
        kp = np.where(seen[:, None], kp, np.stack([rs.uniform(0, 640, n_points), rs.uniform(0, 480, n_points)], axis=1))
        poses.append((R, t)), kps.append(kp.astype(np.float32)), vis.append(seen)
    return dict(K=ue.SCENE_K.copy(), poses=poses, X=X, keypoints=kps, visible=vis)


def align_errors(model_poses, scene, a, b):
    """Model poses {image_id (1-based view + 1): (R, t)} in the frame of view a with |baseline(a, b)| = 1 against the scene's
    truth -> (worst rotation error in degrees, worst camera-centre error in units of the true baseline)."""
    Ra, ta = scene["poses"][a - 1]
    Rb, tb = scene["poses"][b - 1]
    ca, cb = -Ra.T @ ta, -Rb.T @ tb
    base = np.linalg.norm(cb - ca)
    rot, pos = 0.0, 0.0
    for i, (R, t) in model_poses.items():
        Rt, tt = scene["poses"][i - 1]
        R_true = Rt @ Ra.T                                            # view a's camera frame -> view i's
        c_true = Ra @ (-Rt.T @ tt - ca) / base
        c = -R.T @ t
        rot = max(rot, float(np.degrees(np.arccos(np.clip((np.trace(R.T @ R_true) - 1) / 2, -1, 1)))))
        pos = max(pos, float(np.linalg.norm(c - c_true)))
    return rot, pos
