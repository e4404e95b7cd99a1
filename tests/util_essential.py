"""CPU SPECIFICATION (test infrastructure, NOT product code) of the calibrated branch of geometric verification
(DESIGN.md §4.2f): the five-point essential-matrix solver in the Stewénius formulation (null space by SVD, the ten cubic
constraints as a 10x20 matrix, the action matrix of x, `numpy.linalg.eig`, real eigenvalues kept, each solution polished by
Gauss-Newton on the ten cubics so that it satisfies them to round-off), the decision rule for one
pair (`verify_pair_calibrated`) and the pose choice.  numpy only; the sampler, the float32 scoring and the scenes are
oracle/two_view_oracle.py's.  The HIP kernel (csrc/essential.hip) takes another route to the same solution set (Nistér's
degree-10 polynomial), so agreement between the two is a test of both.
"""
import numpy as np

from oracle import two_view_oracle as tv

SALT_E = 0x5A5A5A5A
NUM_HYP_E = 128
MAX_SOLUTIONS = 10
MIN_E_F_INLIER_RATIO = 0.95
USABLE_MODELS = {"SIMPLE_PINHOLE": 0, "PINHOLE": 0, "SIMPLE_RADIAL": 1, "RADIAL": 2, "OPENCV": 4}   # name -> distortion params

# ---- polynomial bookkeeping: monomials of x, y, z as exponent triples -------------------------------------------------------
_LIN = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]
_QUAD = sorted({tuple(np.add(a, b)) for a in _LIN for b in _LIN}, reverse=True)
# the ten cubic monomials first, then the basis of the quotient ring: x^2 xy xz y^2 yz z^2 x y z 1
_CUB = [(3, 0, 0), (2, 1, 0), (2, 0, 1), (1, 2, 0), (1, 1, 1), (1, 0, 2), (0, 3, 0), (0, 2, 1), (0, 1, 2), (0, 0, 3),
        (2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0), (0, 1, 1), (0, 0, 2), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]
_T2 = np.zeros((16, 10))
for _i, _a in enumerate(_LIN):
    for _j, _b in enumerate(_LIN):
        _T2[_i * 4 + _j, _QUAD.index(tuple(np.add(_a, _b)))] = 1.0
_T3 = np.zeros((40, 20))
for _q, _a in enumerate(_QUAD):
    for _k, _b in enumerate(_LIN):
        _T3[_q * 4 + _k, _CUB.index(tuple(np.add(_a, _b)))] = 1.0


def _ll(a, b):
    """linear x linear -> quadratic (coefficient vectors over _LIN, _QUAD)."""
    return np.outer(a, b).reshape(16) @ _T2


def _ql(q, a):
    """quadratic x linear -> cubic (over _CUB)."""
    return np.outer(q, a).reshape(40) @ _T3


def null_space(x1, x2):
    """x1, x2 (5, 2) float64 normalised points, or (5, 3) homogeneous ones -> (4, 3, 3): an orthonormal basis of
    {E : x2' E x1 = 0 for the five}."""
    h1, h2 = (x if x.shape[1] == 3 else np.concatenate([x, np.ones((5, 1))], axis=1) for x in (x1, x2))
    a = (h2[:, :, None] * h1[:, None, :]).reshape(5, 9)
    return np.linalg.svd(a)[2][5:].reshape(4, 3, 3)


def _frame(seed):
    """A fixed rotation far from every axis, for `five_point`'s image frames."""
    q = np.linalg.qr(np.random.RandomState(seed).normal(size=(3, 3)))[0]
    return q * np.sign(np.linalg.det(q))


_FRAME1, _FRAME2 = _frame(0x5E1), _frame(0x5E2)


def constraint_matrix(basis):
    """(4, 3, 3) -> (10, 20): det E = 0 and 2 E E' E - tr(E E') E = 0 for E = x B0 + y B1 + z B2 + B3, columns over _CUB."""
    E = np.transpose(basis, (1, 2, 0))                                  # E[i, j] is a linear form over _LIN
    EEt = np.array([[sum(_ll(E[i, k], E[j, k]) for k in range(3)) for j in range(3)] for i in range(3)])
    lam = EEt.copy()
    tr = EEt[0, 0] + EEt[1, 1] + EEt[2, 2]
    for i in range(3):
        lam[i, i] -= 0.5 * tr
    rows = [sum(_ql(lam[i, k], E[k, j]) for k in range(3)) for i in range(3) for j in range(3)]
    det = (_ql(_ll(E[1, 1], E[2, 2]) - _ll(E[1, 2], E[2, 1]), E[0, 0]) + _ql(_ll(E[1, 2], E[2, 0]) - _ll(E[1, 0], E[2, 2]), E[0, 1])
           + _ql(_ll(E[1, 0], E[2, 1]) - _ll(E[1, 1], E[2, 0]), E[0, 2]))
    return np.array(rows + [det])


_EXP = np.array(_CUB)                                                  # (20, 3) exponents of the cubic columns


def _monomials(xyz):
    """-> the 20 monomials at (x, y, z) and their (20, 3) Jacobian."""
    p = np.prod(xyz[None, :] ** _EXP, axis=1)
    J = np.zeros((20, 3))
    for v in range(3):
        e = _EXP.copy()
        e[:, v] = np.maximum(e[:, v] - 1, 0)
        J[:, v] = _EXP[:, v] * np.prod(xyz[None, :] ** e, axis=1)
    return p, J


def _polish(m, xyz, steps=3):
    """Gauss-Newton on the ten cubics m (10, 20) from an eigenvector's (x, y, z); a step is kept only if it lowers the residual."""
    mono, J = _monomials(xyz)
    r = m @ mono
    for _ in range(steps):
        try:
            step = np.linalg.lstsq(m @ J, -r, rcond=None)[0]
        except np.linalg.LinAlgError:
            break
        mono2, J2 = _monomials(xyz + step)
        r2 = m @ mono2
        if not np.linalg.norm(r2) < np.linalg.norm(r):
            break
        xyz, r, J = xyz + step, r2, J2
    return xyz


def five_point(x1, x2):
    """x1, x2 (5, 2) float64 normalised image points -> (n, 3, 3), n <= 10: every real essential matrix through the five
    correspondences, unit Frobenius norm (no solution for a degenerate sample).

    The action matrix is built on a fixed monomial basis and needs the ten cubics to be solvable for the ten cubic monomials;
    a motion aligned with the image axes (R = I with t along x: E has two non-zero entries) makes that system singular for
    every choice of points.  So the problem is solved in image frames turned by two fixed generic rotations, h1 -> Q1 h1 and
    h2 -> Q2 h2 on homogeneous points, under which E -> Q2 E Q1' and no axis is special, and the solutions are turned back."""
    x1, x2 = np.asarray(x1, np.float64), np.asarray(x2, np.float64)
    if not (np.all(np.isfinite(x1)) and np.all(np.isfinite(x2))):
        return np.zeros((0, 3, 3))
    try:
        with np.errstate(all="ignore"):
            h1 = np.concatenate([x1, np.ones((5, 1))], axis=1) @ _FRAME1.T
            h2 = np.concatenate([x2, np.ones((5, 1))], axis=1) @ _FRAME2.T
            if np.linalg.matrix_rank((h2[:, :, None] * h1[:, None, :]).reshape(5, 9)) < 5:
                return np.zeros((0, 3, 3))                              # dependent equations: more than four dimensions of E
            basis = null_space(h1, h2)
            m = constraint_matrix(basis)
        if not np.all(np.isfinite(m)):
            return np.zeros((0, 3, 3))
        if np.linalg.cond(m[:, :10]) > 1e14:
            return np.zeros((0, 3, 3))
        b = np.linalg.solve(m[:, :10], m[:, 10:])
    except np.linalg.LinAlgError:
        return np.zeros((0, 3, 3))
    act = np.zeros((10, 10))                                           # x * [x^2 xy xz y^2 yz z^2 x y z 1] in that basis
    act[:6] = -b[:6]
    act[6, 0] = act[7, 1] = act[8, 2] = act[9, 6] = 1.0
    try:
        w, v = np.linalg.eig(act)
    except np.linalg.LinAlgError:
        return np.zeros((0, 3, 3))
    out = []
    for k in np.argsort(w.real):
        if w[k].imag != 0 or abs(v[9, k]) == 0:
            continue
        vec = v[:, k].real
        xyz = _polish(m, vec[6:9] / vec[9])
        E = _FRAME2.T @ (xyz[0] * basis[0] + xyz[1] * basis[1] + xyz[2] * basis[2] + basis[3]) @ _FRAME1
        n = np.linalg.norm(E)
        if np.isfinite(n) and n > 0:
            out.append(E / n)
    return np.array(out).reshape(-1, 3, 3)


def matrix_distance(a, b):
    """Frobenius distance between unit-norm matrices, up to sign."""
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    return min(np.linalg.norm(a - b), np.linalg.norm(a + b))


# ---- the 300 exact minimal problems ----------------------------------------------------------------------------------------
SCENE_K = np.array([[600.0, 0, 320.0], [0, 600.0, 240.0], [0, 0, 1]])
_A = 0.12
SCENE_R = np.array([[np.cos(_A), 0, np.sin(_A)], [0, 1, 0], [-np.sin(_A), 0, np.cos(_A)]])
SCENE_T = np.array([-0.8, 0.05, 0.1])


def skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0.0]])


def true_essential():
    E = skew(SCENE_T) @ SCENE_R
    return E / np.linalg.norm(E)


def minimal_problem(i):
    """Five exact float64 correspondences of synthetic_two_view's cameras, from RandomState(500 + i) -> x1, x2 (5, 2)."""
    rs = np.random.RandomState(500 + i)
    X = np.stack([rs.uniform(-3, 3, 5), rs.uniform(-2, 2, 5), rs.uniform(4, 9, 5)], axis=1)
    X2 = X @ SCENE_R.T + SCENE_T
    return X[:, :2] / X[:, 2:], X2[:, :2] / X2[:, 2:]


# ---- cameras ------------------------------------------------------------------------------------------------------------------
def camera_prior(camera):
    """camera: an object with model, params, has_prior_focal_length -> (K (3, 3) float64, usable prior?).  Usable: the flag is
    set and the model is SIMPLE_PINHOLE / PINHOLE, or SIMPLE_RADIAL / RADIAL / OPENCV with every distortion parameter zero."""
    model = camera.model if isinstance(camera.model, str) else getattr(camera.model, "name", str(camera.model))
    p = [float(v) for v in camera.params]
    if model not in USABLE_MODELS:
        return np.eye(3), False
    if model in ("PINHOLE", "OPENCV"):
        fx, fy, cx, cy, dist = p[0], p[1], p[2], p[3], p[4:]
    else:
        fx, fy, cx, cy, dist = p[0], p[0], p[1], p[2], p[3:]
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    ok = bool(camera.has_prior_focal_length) and all(d == 0 for d in dist) and fx > 0 and fy > 0
    return K, ok


def f_from_e(E, K1, K2):
    """F_px = K2^-T E K1^-1 at unit Frobenius norm, float32 (9,)."""
    F = np.linalg.inv(K2).T @ np.asarray(E, np.float64).reshape(3, 3) @ np.linalg.inv(K1)
    n = np.linalg.norm(F)
    return (F / n if n > 0 else F).reshape(9).astype(np.float32)


def project_to_essential(M):
    """Closest matrix with singular values (1, 1, 0), scaled to unit Frobenius norm."""
    U, _, Vt = np.linalg.svd(np.asarray(M, np.float64).reshape(3, 3))
    return U @ np.diag([1.0, 1.0, 0.0]) @ Vt / np.sqrt(2.0)


def eight_point(xn):
    """xn (n, 4) float64 normalised correspondences -> the unit 3x3 minimising sum (x2' M x1)^2 (eigenvector of A'A)."""
    x1, y1, x2, y2 = xn.T
    a = np.stack([x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, np.ones_like(x1)], axis=1)
    return np.linalg.eigh(a.T @ a)[1][:, 0].reshape(3, 3)


def rot_to_quat(R):
    """Rotation matrix -> unit quaternion (w, x, y, z), w >= 0."""
    t = np.trace(R)
    if t > 0:
        s = np.sqrt(t + 1.0) * 2
        q = np.array([0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s])
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k]) * 2
        q = np.zeros(4)
        q[0] = (R[k, j] - R[j, k]) / s
        q[1 + i] = 0.25 * s
        q[1 + j] = (R[j, i] + R[i, j]) / s
        q[1 + k] = (R[k, i] + R[i, k]) / s
    q /= np.linalg.norm(q)
    return -q if q[0] < 0 else q


def choose_pose(E, xn):
    """Of E's four decompositions (R, t) with X2 = R X1 + t, the one with most of xn (n, 4) in front of both cameras (first on
    ties, order (Ra, u), (Ra, -u), (Rb, u), (Rb, -u)) -> qvec (w, x, y, z), unit tvec, R."""
    U, _, Vt = np.linalg.svd(np.asarray(E, np.float64).reshape(3, 3))
    if np.linalg.det(U) < 0:
        U = -U
    if np.linalg.det(Vt) < 0:
        Vt = -Vt
    W = np.array([[0, -1.0, 0], [1.0, 0, 0], [0, 0, 1.0]])
    u = U[:, 2]
    x1 = np.concatenate([xn[:, :2], np.ones((len(xn), 1))], axis=1)
    x2 = np.concatenate([xn[:, 2:], np.ones((len(xn), 1))], axis=1)
    best = None
    for R in (U @ W @ Vt, U @ W.T @ Vt):
        for t in (u, -u):
            # depths d1, d2 with d2 x2 = d1 R x1 + t, least squares per point
            a = x1 @ R.T
            aa, ab, bb = (a * a).sum(1), (a * x2).sum(1), (x2 * x2).sum(1)
            at, bt = a @ t, x2 @ t
            det = aa * bb - ab * ab
            with np.errstate(all="ignore"):
                d1 = (-bb * at + ab * bt) / det
                d2 = (-ab * at + aa * bt) / det
            n = int(((d1 > 0) & (d2 > 0)).sum())
            if best is None or n > best[0]:
                best = (n, R, t)
    _, R, t = best
    return rot_to_quat(R), t / np.linalg.norm(t), R


# ---- the rule for one pair -------------------------------------------------------------------------------------------------
def estimate_e(pts, seed, K1, K2, n_hyp=NUM_HYP_E, perturb=None):
    """pts (M, 4) float32 pixel matches -> (E unit (3, 3) or None, F_px float32 (9,), mask bool (M,)).
    `perturb(E) -> E` (tests only) moves every solver solution before it is scored."""
    M = len(pts)
    K1i, K2i = np.linalg.inv(K1), np.linalg.inv(K2)
    p64 = pts.astype(np.float64)
    xn = np.concatenate([p64[:, :2] * [K1i[0, 0], K1i[1, 1]] + [K1i[0, 2], K1i[1, 2]],
                         p64[:, 2:] * [K2i[0, 0], K2i[1, 1]] + [K2i[0, 2], K2i[1, 2]]], axis=1)
    idx = tv.sample_indices(seed, n_hyp, 5, M, SALT_E)
    best_n, best = 0, None
    for k in range(n_hyp):
        if idx[k, 0] < 0:
            continue
        for E in five_point(xn[idx[k], :2], xn[idx[k], 2:]):
            if perturb is not None:
                E = perturb(E)
            f9 = f_from_e(E, K1, K2)
            n = int(tv.inliers_f32("F", f9, pts).sum())
            if n > best_n:                                      # most inliers, lowest (k, solution) on ties
                best_n, best = n, (E, f9)
    if best is None:
        return None, np.full(9, np.nan, np.float32), np.zeros(M, bool)
    E, f9 = best
    mask = tv.inliers_f32("F", f9, pts)
    if mask.sum() >= 8:
        Er = project_to_essential(eight_point(xn[mask]))
        fr = f_from_e(Er, K1, K2)
        rmask = tv.inliers_f32("F", fr, pts)
        if rmask.sum() >= mask.sum():
            E, f9, mask = Er, fr, rmask
    return E / np.linalg.norm(E), f9, mask


def verify_pair_calibrated(kp1, kp2, matches, pair_id, cam1, cam2, num_e=NUM_HYP_E, perturb=None):
    """verify_pair with the calibrated branch: cam1, cam2 are Camera rows.  A pair without two usable priors, or whose E
    does not reach max(15, 0.25 M) and 0.95 n_f inliers, gets verify_pair's result unchanged."""
    res = tv.verify_pair(kp1, kp2, matches, pair_id)
    (K1, ok1), (K2, ok2) = camera_prior(cam1), camera_prior(cam2)
    matches = np.asarray(matches, np.uint32).reshape(-1, 2)
    if not (ok1 and ok2) or len(matches) < tv.MIN_NUM_INLIERS:
        return res
    pts = np.concatenate([kp1[matches[:, 0], :2], kp2[matches[:, 1], :2]], axis=1).astype(np.float32)
    seed = int(pair_id) & 0xFFFFFFFF
    E, f9, emask = estimate_e(pts, seed, K1, K2, num_e, perturb)
    n_e = int(emask.sum())
    res["n_e"] = n_e
    if E is None or n_e < max(tv.MIN_NUM_INLIERS, tv.MIN_INLIER_RATIO * len(matches)) or n_e < MIN_E_F_INLIER_RATIO * res["n_f"]:
        return res
    h9, hmask = tv.estimate_model("H", pts, seed, tv.NUM_HYP_H)
    if h9 is not None:
        H = np.asarray(h9, np.float64).reshape(3, 3)
        res["H"] = H / H[2, 2] if H[2, 2] != 0 else H
    res["E"] = E
    res["F"] = tv.stored_f(f9)
    mask, res["model"], res["model9"] = emask, "F", f9
    res["config"] = tv.CONFIG_CALIBRATED
    if res["n_h"] / n_e > tv.MAX_H_INLIER_RATIO:
        res["config"] = tv.CONFIG_PLANAR_OR_PANORAMIC
        if res["n_h"] > n_e:
            mask, res["model"], res["model9"] = hmask, "H", h9
    K1i, K2i = np.linalg.inv(K1), np.linalg.inv(K2)
    p64 = pts[emask].astype(np.float64)
    xn = np.concatenate([p64[:, :2] * [K1i[0, 0], K1i[1, 1]] + [K1i[0, 2], K1i[1, 2]],
                         p64[:, 2:] * [K2i[0, 0], K2i[1, 1]] + [K2i[0, 2], K2i[1, 2]]], axis=1)
    res["qvec"], res["tvec"], _ = choose_pose(E, xn)
    res["inlier_matches"] = matches[mask]
    return res


def pose_errors(qvec, tvec, R_true=SCENE_R, t_true=SCENE_T):
    """-> (rotation error, translation-direction error) in degrees."""
    w, x, y, z = qvec
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    c = np.clip((np.trace(R.T @ R_true) - 1) / 2, -1, 1)
    ct = np.clip(tvec @ t_true / (np.linalg.norm(tvec) * np.linalg.norm(t_true)), -1, 1)
    return float(np.degrees(np.arccos(c))), float(np.degrees(np.arccos(ct)))
