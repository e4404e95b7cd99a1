"""CPU SPECIFICATION (test infrastructure, NOT product code) of two-view relative pose: the pose candidates
of a pair from its essential matrix or its homography, the triangulation of every inlier under every candidate in a fixed
order of float64 operations, and the rule that turns the counts and angles into pose, triangulation angle and the
PLANAR / PANORAMIC split.  numpy only, built from oracle/two_view_oracle.py and tests/util_essential.py.  The HIP kernel
(csrc/pose.hip) does the triangulation, the choice and the median; matching/pose.py the candidates and the rule.
This is the build's own published rule: parity with COLMAP is unpinned.
"""
import numpy as np

from oracle import two_view_oracle as tv
import util_essential as ue

H_ROTATION_EPS = 1e-10      # sigma_1^2 - sigma_3^2 of Hn (middle singular value 1) below this: Hn is a rotation, t = 0


# ---- candidates: (4, 12) float64, R row-major then t; NaN in the first element marks an unused slot ---------------------------
def _pack(cands):
    out = np.full((4, 12), np.nan)
    for k, (R, t) in enumerate(cands):
        out[k, :9], out[k, 9:] = np.asarray(R).reshape(9), t
    return out


def e_candidates(E):
    """The four decompositions of an essential matrix in choose_pose's order (Ra, u), (Ra, -u), (Rb, u), (Rb, -u), |u| = 1."""
    U, _, Vt = np.linalg.svd(np.asarray(E, np.float64).reshape(3, 3))
    if np.linalg.det(U) < 0:
        U = -U
    if np.linalg.det(Vt) < 0:
        Vt = -Vt
    W = np.array([[0, -1.0, 0], [1.0, 0, 0], [0, 0, 1.0]])
    u = U[:, 2] / np.linalg.norm(U[:, 2])
    return _pack([(R, t) for R in (U @ W @ Vt, U @ W.T @ Vt) for t in (u, -u)])


def normalise_homography(Hn):
    """Scale so that the middle singular value is 1 and the determinant positive."""
    Hn = np.asarray(Hn, np.float64).reshape(3, 3)
    Hn = Hn / np.linalg.svd(Hn, compute_uv=False)[1]
    return -Hn if np.linalg.det(Hn) < 0 else Hn


def fix_eigenvector_signs(V):
    """Columns v1, v2, v3 of an eigenvector matrix of Hn'Hn (eigenvalues descending) -> the stated convention: the component
    of largest magnitude (the first on ties) of v1 and of v3 is positive, v2 = v3 x v1; the result is in SO(3)."""
    def pos(v):
        return -v if v[int(np.argmax(np.abs(v)))] < 0 else v

    v1, v3 = pos(V[:, 0]), pos(V[:, 2])
    return np.stack([v1, np.cross(v3, v1), v3], axis=1)


def nearest_rotation(M):
    U, _, Vt = np.linalg.svd(M)
    R = U @ Vt
    return U @ np.diag([1.0, 1.0, -1.0]) @ Vt if np.linalg.det(R) < 0 else R


def h_decompositions(Hn, flip=(1.0, 1.0, 1.0)):
    """Hn (normalised coordinates, any scale) -> list of (R, t, n) with Hn ~ R + t n' (Ma, Soatto, Kosecka, Sastry, An
    Invitation to 3-D Vision, Theorem 5.19), in the order (R1, t1, n1), (R1, -t1, -n1), (R2, t2, n2), (R2, -t2, -n2); t is NOT
    yet scaled.  A rotation (sigma_1^2 - sigma_3^2 < H_ROTATION_EPS): the single (R nearest to Hn, 0, 0).
    `flip` (tests only) multiplies the eigenvectors before the sign convention is applied."""
    Hn = normalise_homography(Hn)
    w, V = np.linalg.eigh(Hn.T @ Hn)
    w, V = w[::-1], V[:, ::-1] * np.asarray(flip)[None, :]              # descending: sigma_1^2 >= sigma_2^2 = 1 >= sigma_3^2
    if w[0] - w[2] < H_ROTATION_EPS:
        return [(nearest_rotation(Hn), np.zeros(3), np.zeros(3))]
    V = fix_eigenvector_signs(V)
    v1, v2, v3 = V[:, 0], V[:, 1], V[:, 2]
    a, b = np.sqrt(max(1.0 - w[2], 0.0)), np.sqrt(max(w[0] - 1.0, 0.0))
    den = np.sqrt(w[0] - w[2])
    out = []
    for u in ((a * v1 + b * v3) / den, (a * v1 - b * v3) / den):
        Um = np.stack([v2, u, np.cross(v2, u)], axis=1)
        hv, hu = Hn @ v2, Hn @ u
        Wm = np.stack([hv, hu, np.cross(hv, hu)], axis=1)
        R = Wm @ Um.T
        n = np.cross(v2, u)
        t = (Hn - R) @ n
        out += [(R, t, n), (R, -t, -n)]
    return out


def h_candidates(Hn, flip=(1.0, 1.0, 1.0)):
    cands = []
    for R, t, _ in h_decompositions(Hn, flip):
        nt = np.linalg.norm(t)
        cands.append((R, t / nt if nt > 0 else np.zeros(3)))
    return _pack(cands)


# ---- triangulation of every point under one candidate: float64, this order of single operations, no fused multiply-add ---------
def triangulate(xn, cand12):
    """xn (n, 4), one candidate (12,) -> in-front mask (n,), midpoints in camera 1 (n, 3), triangulation angles (n,)."""
    r00, r01, r02, r10, r11, r12, r20, r21, r22, t0, t1, t2 = (float(v) for v in cand12)
    x, y, u, v = (np.ascontiguousarray(xn[:, i], np.float64) for i in range(4))
    with np.errstate(all="ignore"):
        a0 = r00 * x + r01 * y + r02
        a1 = r10 * x + r11 * y + r12
        a2 = r20 * x + r21 * y + r22
        aa = a0 * a0 + a1 * a1 + a2 * a2
        ab = a0 * u + a1 * v + a2
        bb = u * u + v * v + 1.0
        at = a0 * t0 + a1 * t1 + a2 * t2
        bt = u * t0 + v * t1 + t2
        det = aa * bb - ab * ab
        d1 = (-bb * at + ab * bt) / det
        d2 = (-ab * at + aa * bt) / det
        front = np.isfinite(d1) & np.isfinite(d2) & (d1 > 0) & (d2 > 0)
        w0, w1, w2 = d2 * u - t0, d2 * v - t1, d2 - t2
        X0 = 0.5 * (d1 * x + (r00 * w0 + r10 * w1 + r20 * w2))
        X1 = 0.5 * (d1 * y + (r01 * w0 + r11 * w1 + r21 * w2))
        X2 = 0.5 * (d1 + (r02 * w0 + r12 * w1 + r22 * w2))
        c0 = -(r00 * t0 + r10 * t1 + r20 * t2)                         # c2 = -R' t, the second camera's centre
        c1 = -(r01 * t0 + r11 * t1 + r21 * t2)
        c2 = -(r02 * t0 + r12 * t1 + r22 * t2)
        e0, e1, e2 = X0 - c0, X1 - c1, X2 - c2
        k0, k1, k2 = X1 * e2 - X2 * e1, X2 * e0 - X0 * e2, X0 * e1 - X1 * e0
        angle = np.arctan2(np.sqrt(k0 * k0 + k1 * k1 + k2 * k2), X0 * e0 + X1 * e1 + X2 * e2)
    return front, np.stack([X0, X1, X2], axis=1), angle


def median_angle(angles):
    s = np.sort(np.asarray(angles, np.float64))
    if len(s) == 0:
        return 0.0
    return float(s[len(s) // 2]) if len(s) % 2 else float(0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2]))


def choose(xn, cand):
    """What the kernel computes for one pair: xn (n, 4), cand (4, 12) -> front counts int32 (4,), best slot, tri_angle,
    midpoints (n, 3) under the best candidate (NaN where the point is not in front)."""
    xn = np.asarray(xn, np.float64).reshape(-1, 4)
    counts = np.zeros(4, np.int32)
    for k in range(4):
        if np.isnan(cand[k, 0]) or not cand[k, 9:].any():               # unused slot, or t = 0
            continue
        counts[k] = int(triangulate(xn, cand[k])[0].sum())
    best = int(np.argmax(counts))                                         # the lowest slot wins ties
    pts = np.full((len(xn), 3), np.nan)
    if counts[best] == 0:
        return counts, best, 0.0, pts
    front, X, angle = triangulate(xn, cand[best])
    pts[front] = X[front]
    return counts, best, median_angle(angle[front]), pts


# ---- the rule for one pair ------------------------------------------------------------------------------------------------------
def normalise(pts, K1, K2):
    K1i, K2i = np.linalg.inv(K1), np.linalg.inv(K2)
    p64 = np.asarray(pts, np.float64)
    return np.concatenate([p64[:, :2] * [K1i[0, 0], K1i[1, 1]] + [K1i[0, 2], K1i[1, 2]],
                           p64[:, 2:] * [K2i[0, 0], K2i[1, 1]] + [K2i[0, 2], K2i[1, 2]]], axis=1)


def angle_floor(K1, K2, max_error=tv.MAX_ERROR):
    """The angle the verifier's pixel tolerance subtends at the shorter focal length."""
    return float(np.arctan(max_error / min((K1[0, 0] + K1[1, 1]) / 2, (K2[0, 0] + K2[1, 1]) / 2)))


def pair_candidates(res, K1, K2, perturb=None):
    """The candidates of a verified pair.  PLANAR_OR_PANORAMIC (H explains the matches): from the stored H, K2^-1 H K1,
    whichever mask gave the inliers — an E or F fitted to coplanar points or to a rotation is not determined by them, and its
    decomposition is arbitrary.  CALIBRATED / UNCALIBRATED: from E where the best model is E, else from
    K2' F K1 (F = `model9`) projected onto the essential manifold.  `perturb(M) -> M` (tests only) moves the decomposed matrix."""
    same = perturb or (lambda M: M)
    if res["config"] == tv.CONFIG_PLANAR_OR_PANORAMIC:
        return h_candidates(same(np.linalg.inv(K2) @ np.asarray(res["H"], np.float64).reshape(3, 3) @ K1))
    if "E" in res:
        return e_candidates(same(np.asarray(res["E"], np.float64)))
    F = np.asarray(res["model9"], np.float64).reshape(3, 3)
    return e_candidates(same(ue.project_to_essential(K2.T @ F @ K1)))


def apply_pose_rule(res, kp1, kp2, K1, K2, perturb=None):
    """res: a verify result that carries `model` / `model9` (not DEGENERATE) -> the same dict with the relative pose."""
    m = np.asarray(res["inlier_matches"], np.int64).reshape(-1, 2)
    pts = np.concatenate([kp1[m[:, 0], :2], kp2[m[:, 1], :2]], axis=1).astype(np.float32)
    xn = normalise(pts, K1, K2)
    cand = pair_candidates(res, K1, K2, perturb)
    counts, best, tri, _ = choose(xn, cand)
    R, t = cand[best, :9].reshape(3, 3), cand[best, 9:]
    res["qvec"], res["tvec"] = ue.rot_to_quat(R), t.copy()
    res["tri_angle"], res["n_front"] = tri, int(counts[best])
    if res["config"] == tv.CONFIG_PLANAR_OR_PANORAMIC:
        panoramic = counts[best] == 0 or tri < angle_floor(K1, K2)
        res["config"] = tv.CONFIG_PANORAMIC if panoramic else tv.CONFIG_PLANAR
    if res["config"] == tv.CONFIG_PANORAMIC:
        res["tvec"] = np.zeros(3)
    return res


def with_model(res, kp1, kp2, matches, pair_id):
    """oracle verify_pair's result plus the model whose mask produced the inliers (what matching/two_view.py adds)."""
    if res["config"] != tv.CONFIG_DEGENERATE and "model" not in res:
        m = np.asarray(matches, np.uint32).reshape(-1, 2)
        pts = np.concatenate([kp1[m[:, 0], :2], kp2[m[:, 1], :2]], axis=1).astype(np.float32)
        use_h = res["config"] == tv.CONFIG_PLANAR_OR_PANORAMIC and res["n_h"] > res["n_f"]
        res["model"] = "H" if use_h else "F"
        res["model9"], mask = tv.estimate_model(res["model"], pts, int(pair_id) & 0xFFFFFFFF, tv.NUM_HYP_H if use_h else tv.NUM_HYP_F)
        assert np.array_equal(m[mask], res["inlier_matches"])
    return res


def verify_pair_pose(kp1, kp2, matches, pair_id, cam1, cam2, perturb=None):
    """verify_pair_calibrated, then the relative pose of every non-DEGENERATE pair whose two cameras have a usable prior."""
    res = ue.verify_pair_calibrated(kp1, kp2, matches, pair_id, cam1, cam2)
    (K1, ok1), (K2, ok2) = ue.camera_prior(cam1), ue.camera_prior(cam2)
    if not (ok1 and ok2) or res["config"] == tv.CONFIG_DEGENERATE:
        return res
    return apply_pose_rule(with_model(res, kp1, kp2, matches, pair_id), kp1, kp2, K1, K2, perturb)


# ---- scenes -----------------------------------------------------------------------------------------------------------------------
def pure_rotation_two_view(seed, n_points=300, outlier_frac=0.3, noise=0.5):
    """synthetic_two_view's camera, point cloud, noise and wrong matches with t = 0: a panorama."""
    rs = np.random.RandomState(seed)
    X = np.stack([rs.uniform(-3, 3, n_points), rs.uniform(-2, 2, n_points), rs.uniform(4, 9, n_points)], axis=1)
    p1 = (ue.SCENE_K @ X.T).T
    p2 = (ue.SCENE_K @ (ue.SCENE_R @ X.T)).T
    kp1 = (p1[:, :2] / p1[:, 2:]) + rs.normal(0, noise, (n_points, 2))
    kp2 = (p2[:, :2] / p2[:, 2:]) + rs.normal(0, noise, (n_points, 2))
    is_in = rs.uniform(size=n_points) >= outlier_frac
    perm = rs.permutation(n_points)
    j = np.where(is_in, np.arange(n_points), perm)
    is_in &= j == np.arange(n_points)
    matches = np.stack([np.arange(n_points), j], axis=1).astype(np.uint32)
    return kp1.astype(np.float32), kp2.astype(np.float32), matches, is_in
