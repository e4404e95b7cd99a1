"""CPU SPECIFICATION (test infrastructure, NOT product code) of the focal-length estimate from the verified pairs (DESIGN.md
§4.2o): the self-calibration cost of one pair under one candidate (`focal_pair_cost`, the rule of csrc/focal.hip), the call of
vc_focal_cost on numpy arrays (`focal_cost`), the grid search on plain arrays (`estimate_ratio`, the rule of
vit_colmap_amd/matching/focal.py) and the scene that the feature is tested on (`skew_scene`).  numpy only.

The cost is Mendonça and Cipolla's: for a camera that is the same in both images K' F K is an essential matrix, whose two
non-zero singular values are equal; (s1 - s2) / (s1 + s2) of it, weighted by the pair's inlier count and summed over the
UNCALIBRATED pairs of a camera, is minimised over one scale r on the stored focal length(s).  Every operation of
`focal_pair_cost` and of the sums is a single float64 one in the kernel's order, so the host build of the kernel's routine
returns this file's bytes.  This is the build's own published rule: parity with COLMAP's handling of an unknown focal length
is unpinned.
"""
import numpy as np

import util_mapper as um

FOCAL_CHUNK = 256                  # pairs per partial sum (kFocalChunk of csrc/focal.hip)
FOCAL_MIN_PAIRS = 3
GRID_STEPS = 64                    # 65 candidates per level
GRID_LEVELS = 4
GRID_LO, GRID_SPAN = 0.25, 16.0    # level 0: r_k = 0.25 * 16^(k / 64), 0.25 .. 4

# ---- measured constants (tests/test_focal_spec.py asserts every one; all are the SPECIFICATION's, measured on the CPU) ---------------
# worst |focal_pair_cost - (s1 - s2) / (s1 + s2) of numpy.linalg.svd| over the 300 matrices of `random_pair` x the 65 level-0
# candidates: measured 1.41e-8, at the true focal, where s1 = s2.  The closed form takes the square root of a discriminant
# that is the difference of two numbers of order 1, so it resolves a cost only to sqrt(eps) = 1.5e-8; the bound is 2x the
# measurement, rounded up.  Away from the true focal the two agree to 1e-15.
DEFINITION_ABS = 3.0e-8
# the relative error of r* on the exact F of `skew_scene`.  The bound is the issue's; measured 5.9e-8, 5.5e-10, 6.0e-8 and 2.3e-8
# at the true ratios 1/1.3, 1, 1.3 and 2.5.  With two grid levels, as first proposed, it is 1.0e-4 at every ratio but 1: the
# cost has a kink at its minimum (see estimate_ratio), which is why GRID_LEVELS is 4
SPEC_EXACT_REL = 1e-6
# the relative error of r* with F refitted by `eight_point` from the scene's matches under 1 px of noise, true ratio 1/1.3:
# measured 1.17e-2 (r* 0.760224 for 0.769231), rounded up.  The device path may be 2x that: the two differ only in rounding
SPEC_NOISY_REL = 1.2e-2
# host build against this file: every byte of out_cost and out_weight is equal over all the sizes of HOST_SIZES (measured: 0
# values differ), so no tolerance: gcc's, clang's and numpy's sqrt are all the correctly rounded one
HOST_SPEC_REL = 0.0


# ---- one pair -----------------------------------------------------------------------------------------------------------------------
def pair_matrix(F, cx, cy):
    """F (9,) row-major, the principal point -> A = T' F T at unit Frobenius norm (9,) and whether the pair counts (a norm that
    is finite and not 0).  T = [[1, 0, cx], [0, 1, cy], [0, 0, 1]]."""
    f = [np.float64(v) for v in np.asarray(F, np.float64).reshape(9)]
    cx, cy = np.float64(cx), np.float64(cy)
    with np.errstate(all="ignore"):
        g = [f[0], f[1], f[0] * cx + f[1] * cy + f[2],
             f[3], f[4], f[3] * cx + f[4] * cy + f[5],
             f[6], f[7], f[6] * cx + f[7] * cy + f[8]]
        a = g[:6] + [cx * g[0] + cy * g[3] + g[6], cx * g[1] + cy * g[4] + g[7], cx * g[2] + cy * g[5] + g[8]]
        n2 = np.float64(0.0)
        for v in a:
            n2 = n2 + v * v
        norm = np.sqrt(n2)
        ok = bool(np.isfinite(norm) and norm > 0)
        return np.array([v / norm for v in a]), ok


def focal_pair_cost(A, d0, d1):
    """A (..., 9) unit-norm, d = (d0, d1, 1) the candidate's focal lengths (arrays broadcast) -> (s1 - s2) / (s1 + s2) of
    E = diag(d) A diag(d), by the closed form on the characteristic polynomial of E'E (rank 2: its roots are those of
    x^2 - c2 x + c1)."""
    A = np.asarray(A, np.float64)
    d = (np.asarray(d0, np.float64), np.asarray(d1, np.float64), np.float64(1.0))
    with np.errstate(all="ignore"):
        E = [[(d[i] * A[..., 3 * i + j]) * d[j] for j in range(3)] for i in range(3)]
        c2 = 0.0
        for i in range(3):
            for j in range(3):
                c2 = c2 + E[i][j] * E[i][j]
        m2 = 0.0
        for i in range(3):
            for j in range(3):
                m = E[0][i] * E[0][j] + E[1][i] * E[1][j] + E[2][i] * E[2][j]
                m2 = m2 + m * m
        c1 = (c2 * c2 - m2) * 0.5
        disc = c2 * c2 - 4.0 * c1
        disc = np.where(disc > 0, disc, 0.0)
        l1 = (c2 + np.sqrt(disc)) * 0.5
        l2 = c1 / l1
        l2 = np.where(l2 > 0, l2, 0.0)
        s1, s2 = np.sqrt(l1), np.sqrt(l2)
        return (s1 - s2) / (s1 + s2)


def svd_cost(A, d0, d1):
    """The definition: the singular values of diag(d) A diag(d) from numpy.linalg.svd."""
    D = np.diag([d0, d1, 1.0])
    s = np.linalg.svd(D @ np.asarray(A, np.float64).reshape(3, 3) @ D, compute_uv=False)
    return (s[0] - s[1]) / (s[0] + s[1])


# ---- the call -----------------------------------------------------------------------------------------------------------------------
def focal_cost(F, pair_cam, w, cams, ratios):
    """vc_focal_cost on numpy arrays: F (n_pairs, 9), pair_cam int32 (n_pairs,), w (n_pairs,), cams (n_cams, 4) = (fx0, fy0, cx,
    cy), ratios (n_cand,) -> out_cost (n_cams, n_cand), out_weight (n_cams,).  A pair counts where its slot is inside the table,
    its weight is finite and positive and its A has a norm; a ratio that is not finite and positive gives a NaN column."""
    F, cams = np.asarray(F, np.float64).reshape(-1, 9), np.asarray(cams, np.float64).reshape(-1, 4)
    pair_cam, w, ratios = np.asarray(pair_cam, np.int64), np.asarray(w, np.float64), np.asarray(ratios, np.float64)
    n_pairs, n_cams, n_cand = len(F), len(cams), len(ratios)
    total, weight = np.zeros((n_cams, n_cand)), np.zeros(n_cams)
    good = np.isfinite(ratios) & (ratios > 0)
    r = np.where(good, ratios, 1.0)
    with np.errstate(all="ignore"):
        for lo in range(0, n_pairs, FOCAL_CHUNK):
            part, part_w = np.zeros((n_cams, n_cand)), np.zeros(n_cams)
            for p in range(lo, min(lo + FOCAL_CHUNK, n_pairs)):
                c = int(pair_cam[p])
                if not (0 <= c < n_cams and np.isfinite(w[p]) and w[p] > 0):
                    continue
                A, ok = pair_matrix(F[p], cams[c, 2], cams[c, 3])
                if not ok:
                    continue
                part[c] = part[c] + w[p] * focal_pair_cost(A, r * cams[c, 0], r * cams[c, 1])
                part_w[c] = part_w[c] + w[p]
            total, weight = total + part, weight + part_w
        cost = total / weight[:, None]
    cost[:, ~good] = np.nan
    return np.where(np.isnan(cost), np.nan, cost), weight                 # every NaN is numpy's one NaN


# ---- the grid search ------------------------------------------------------------------------------------------------------------------
def level0():
    return GRID_LO * np.power(GRID_SPAN, np.arange(GRID_STEPS + 1) / GRID_STEPS)


def level1(lo, hi):
    return lo * np.power(hi / lo, np.arange(GRID_STEPS + 1) / GRID_STEPS)


def estimate_ratio(F, w, cam, cost_fn=focal_cost):
    """The pairs of one camera (F (n, 9), w (n,)), cam = (fx0, fy0, cx, cy) -> dict(ratio, pairs, weight, cost_min, cost_median,
    reason): the rule of vit_colmap_amd/matching/focal.py, written on its own.  Level 0 is the grid of `level0`; each further
    level is 65 log-spaced values between the neighbours of the minimum of the level before; r* is the vertex of the parabola
    through the last level's minimum and its two neighbours in log r.  (s1 - s2) / (s1 + s2) is |s1 - s2| of two singular values
    that cross at the true focal: a V, not a bowl, and the parabola through three points of a V misses its tip by up to a sixth
    of the spacing.  Hence GRID_LEVELS = 4: the last spacing is 1.3e-6 in log r."""
    F, w = np.asarray(F, np.float64).reshape(-1, 9), np.asarray(w, np.float64).reshape(-1)
    slots, cams = np.zeros(len(F), np.int32), np.asarray(cam, np.float64).reshape(1, 4)
    r0 = level0()
    J0, W = cost_fn(F, slots, w, cams, r0)
    counted = sum(1 for f, x in zip(F, w) if x > 0 and np.isfinite(x) and pair_matrix(f, cam[2], cam[3])[1])
    out = dict(ratio=None, pairs=counted, weight=float(W[0]) if len(W) else 0.0, cost_min=None, cost_median=None, reason=None)
    if not out["weight"] > 0:
        return dict(out, reason="no weight: no UNCALIBRATED pair of this camera has inliers and a finite F")
    if counted < FOCAL_MIN_PAIRS:
        return dict(out, reason=f"{counted} pairs, fewer than {FOCAL_MIN_PAIRS}")
    k = int(np.argmin(J0[0]))
    out["cost_median"] = float(np.median(J0[0]))
    if k == 0 or k == GRID_STEPS:
        return dict(out, cost_min=float(J0[0][k]), reason="the minimum is on the edge of the grid")
    r1, m = r0, k
    for _ in range(1, GRID_LEVELS):
        r1 = level1(r1[max(m - 1, 0)], r1[min(m + 1, GRID_STEPS)])
        J1 = cost_fn(F, slots, w, cams, r1)[0][0]
        m = int(np.argmin(J1))
    x = np.log(r1)
    best = x[m]
    if 0 < m < GRID_STEPS:
        h = 0.5 * (x[m + 1] - x[m - 1])
        den = J1[m - 1] - 2.0 * J1[m] + J1[m + 1]
        if den > 0:
            best = x[m] + 0.5 * h * (J1[m - 1] - J1[m + 1]) / den
    return dict(out, ratio=float(np.exp(best)), cost_min=float(J1[m]))


# ---- problems -------------------------------------------------------------------------------------------------------------------------
def rotation(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    S = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * S + (1 - np.cos(angle)) * S @ S


def fundamental(K, pose_i, pose_j):
    """x_j' F x_i = 0 in pixels for two world -> camera poses under one K, at unit Frobenius norm."""
    (Ri, ti), (Rj, tj) = pose_i, pose_j
    R, t = Rj @ Ri.T, tj - Rj @ Ri.T @ ti
    E = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]) @ R
    Ki = np.linalg.inv(K)
    F = Ki.T @ E @ Ki
    return F / np.linalg.norm(F)


def random_pair(i):
    """Problem i of the 300 of the definition test, from RandomState(15000 + i): a random K (f 300-1500, aspect 0.9-1.1, the
    principal point near the centre of 640x480), a random rotation of up to 40 degrees and a random baseline -> F (9,), K."""
    rs = np.random.RandomState(15000 + i)
    f = rs.uniform(300, 1500)
    K = np.array([[f, 0, 320 + rs.uniform(-40, 40)], [0, f * rs.uniform(0.9, 1.1), 240 + rs.uniform(-40, 40)], [0, 0, 1.0]])
    R = rotation(rs.normal(size=3), np.radians(rs.uniform(2, 40)))
    return fundamental(K, (np.eye(3), np.zeros(3)), (R, rs.normal(size=3))).reshape(9), K


JITTER_DEG = 8.0          # the largest rotation of a view of `skew_scene` about its own centre


def skew_scene(seed=5, jitter_seed=77, noise=0.3):
    """um.windowed_scene with every view turned about its own centre by a rotation of 2 to JITTER_DEG degrees about a random
    axis (RandomState(jitter_seed); a random axis has a component along the optical axis, so the jitter includes roll).  The
    arc cameras all fixate the origin: their optical axes meet, which is the configuration in which F says nothing about an
    unknown focal length (tests/test_focal_spec.py shows it on um.windowed_scene).  Turned, the axes are skew.  With this
    jitter the specification returns r on the exact F of the scene to better than 1e-6 (the figures are at SPEC_EXACT_REL).  Keypoints are
    re-projected under the turned poses with `noise` px; an unseen keypoint stays the uniform random pixel it was."""
    scene = um.windowed_scene(seed=seed)
    rs = np.random.RandomState(jitter_seed)
    poses, kps = [], []
    for (R, t), kp, seen in zip(scene["poses"], scene["keypoints"], scene["visible"]):
        J = rotation(rs.normal(size=3), np.radians(rs.uniform(2.0, JITTER_DEG)))
        R2, t2 = J @ R, J @ t
        p = (scene["K"] @ (scene["X"] @ R2.T + t2).T).T
        xy = p[:, :2] / p[:, 2:] + rs.normal(0, noise, (len(p), 2))
        poses.append((R2, t2))
        kps.append(np.where(seen[:, None], xy, kp).astype(np.float32))
    return dict(scene, poses=poses, keypoints=kps)


def scene_pairs(scene):
    """[(i, j)] 0-based, i < j, of the views that share at least 15 points."""
    n = len(scene["poses"])
    return [(i, j) for i in range(n) for j in range(i + 1, n) if int((scene["visible"][i] & scene["visible"][j]).sum()) >= 15]


def exact_rows(scene, pairs=None):
    """The exact F of every pair and its number of common points -> F (n, 9), w (n,)."""
    pairs = scene_pairs(scene) if pairs is None else pairs
    F = np.stack([fundamental(scene["K"], scene["poses"][i], scene["poses"][j]).reshape(9) for i, j in pairs])
    return F, np.array([float((scene["visible"][i] & scene["visible"][j]).sum()) for i, j in pairs])


def eight_point(x1, x2):
    """The specification's own refit: Hartley-normalised eight-point least squares over all the matches x1, x2 (n, 2), the
    closest rank-2 matrix, unit Frobenius norm -> F (9,)."""
    def normalise(x):
        mu = x.mean(axis=0)
        s = np.sqrt(2.0) / np.linalg.norm(x - mu, axis=1).mean()
        T = np.array([[s, 0, -s * mu[0]], [0, s, -s * mu[1]], [0, 0, 1.0]])
        return (x - mu) * s, T

    (a, T1), (b, T2) = normalise(np.asarray(x1, np.float64)), normalise(np.asarray(x2, np.float64))
    rows = np.stack([b[:, 0] * a[:, 0], b[:, 0] * a[:, 1], b[:, 0], b[:, 1] * a[:, 0], b[:, 1] * a[:, 1], b[:, 1], a[:, 0], a[:, 1],
                     np.ones(len(a))], axis=1)
    U, s, Vt = np.linalg.svd(np.linalg.svd(rows)[2][-1].reshape(3, 3))
    F = T2.T @ (U @ np.diag([s[0], s[1], 0.0]) @ Vt) @ T1
    return (F / np.linalg.norm(F)).reshape(9)


def noisy_rows(scene, noise=1.0, seed=91, pairs=None):
    """F refitted by `eight_point` from the common points of every pair, re-projected exactly and given `noise` px -> F, w."""
    pairs = scene_pairs(scene) if pairs is None else pairs
    rs = np.random.RandomState(seed)
    F, w = [], []
    for i, j in pairs:
        both = scene["visible"][i] & scene["visible"][j]
        xs = []
        for v in (i, j):
            R, t = scene["poses"][v]
            p = (scene["K"] @ (scene["X"][both] @ R.T + t).T).T
            xs.append(p[:, :2] / p[:, 2:] + rs.normal(0, noise, (int(both.sum()), 2)))
        F.append(eight_point(*xs)), w.append(float(both.sum()))
    return np.stack(F), np.array(w)


def camera_of(scene, factor):
    """(fx0, fy0, cx, cy) of a database whose stored focal is `factor` times the scene's."""
    K = scene["K"]
    return np.array([K[0, 0] * factor, K[1, 1] * factor, K[0, 2], K[1, 2]])


def off_scene(scene, factor=1.3):
    """The scene as a database would carry it with the focal `factor` times the true one."""
    K = scene["K"].copy()
    K[0, 0], K[1, 1] = K[0, 0] * factor, K[1, 1] * factor
    return dict(scene, K=K)


# ---- calls of vc_focal_cost with everything that can go wrong in them ---------------------------------------------------------------
HOST_SIZES = [(n, k) for n in (0, 1, 255, 256, 257, 1000) for k in (1, 64, 65)]
CALL_CAMS = np.array([[780.0, 780.0, 320.0, 240.0], [500.0, 520.0, 300.0, 250.0]])


def call_case(n_pairs, n_cand, edges=True):
    """One call: random rank-2 F (`random_pair`'s construction), two cameras interleaved, weights 15-400, the first n_cand
    candidates of a 65-point grid.  With `edges` and room for them: pairs with slot -1, n_cams, -5 and 2^31 - 1, a NaN F, a
    zero F, w = 0, NaN and -3, an F of 1e200 (A's norm overflows), and the candidates NaN, -1, inf and 0 in columns 1-4.
    -> F, pair_cam, w, cams, ratios."""
    rs = np.random.RandomState(16000 + 100 * n_pairs + n_cand)
    F = np.zeros((n_pairs, 9))
    for p in range(n_pairs):
        f = rs.uniform(300, 1500)
        K = np.array([[f, 0, 320 + rs.uniform(-40, 40)], [0, f * rs.uniform(0.9, 1.1), 240 + rs.uniform(-40, 40)], [0, 0, 1.0]])
        F[p] = fundamental(K, (np.eye(3), np.zeros(3)), (rotation(rs.normal(size=3), np.radians(rs.uniform(2, 40))), rs.normal(size=3))).reshape(9)
    pair_cam = (np.arange(n_pairs) % 2).astype(np.int32)
    w = rs.randint(15, 401, n_pairs).astype(np.float64)
    ratios = level0()[:n_cand].copy() if n_cand <= GRID_STEPS + 1 else np.linspace(0.3, 3.0, n_cand)
    if edges and n_pairs >= 255:
        pair_cam[[3, 40, 77, 254]] = [-1, len(CALL_CAMS), -5, 2 ** 31 - 1]
        F[5, 4], F[8], F[90] = np.nan, 0.0, 1e200
        w[[10, 11, 12]] = [0.0, np.nan, -3.0]
    if edges and n_cand >= 64:
        ratios[1:5] = [np.nan, -1.0, np.inf, 0.0]
    return F, pair_cam, w, CALL_CAMS.copy(), ratios


def write_pairs_file(path, F, pair_cam, w, cams, ratios):
    """The input of tools/focal_cost_host.cpp."""
    with open(path, "wb") as f:
        f.write(np.array([len(pair_cam), len(cams), len(ratios)], np.int32).tobytes())
        f.write(np.ascontiguousarray(pair_cam, np.int32).tobytes())
        for a in (F, w, cams, ratios):
            f.write(np.ascontiguousarray(a, np.float64).tobytes())


def run_host(program, tmp_path, F, pair_cam, w, cams, ratios, name="pairs"):
    """-> (out_cost (n_cams, n_cand), out_weight (n_cams,)), the program's stderr."""
    import subprocess

    write_pairs_file(tmp_path / f"{name}.bin", F, pair_cam, w, cams, ratios)
    done = subprocess.run([program, str(tmp_path / f"{name}.bin"), str(tmp_path / f"{name}_out.bin")], stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, text=True)
    assert done.returncode == 0, done.stderr
    raw = np.fromfile(tmp_path / f"{name}_out.bin", np.float64)
    n_cams, n_cand = len(cams), len(ratios)
    assert len(raw) == n_cams * n_cand + n_cams
    return (raw[:n_cams * n_cand].reshape(n_cams, n_cand), raw[n_cams * n_cand:]), done.stderr


# ---- databases ----------------------------------------------------------------------------------------------------------------------
def write_rows_db(path, scene, factor, F, w, pairs=None, model="PINHOLE", matches=False):
    """The scene as a database whose one camera (no focal-length prior) stores `factor` times the true focal: images, keypoints
    and one UNCALIBRATED row per pair of `pairs` (default `scene_pairs`) with the given F and the pair's common points as
    inlier matches (w is their number).  `matches`: also the `matches` rows, the common points plus a tenth as many wrong ones."""
    from oracle import two_view_oracle as tv
    from vit_colmap_amd.database import ColmapDatabase
    from vit_colmap_amd.database.colmap_db import Camera

    pairs = scene_pairs(scene) if pairs is None else pairs
    fx, fy, cx, cy = camera_of(scene, factor)
    params = {"PINHOLE": [fx, fy, cx, cy], "SIMPLE_PINHOLE": [fx, cx, cy], "SIMPLE_RADIAL": [fx, cx, cy, 0.0], "OPENCV": [fx, fy, cx, cy, 0, 0, 0, 0]}[model]
    db = ColmapDatabase(str(path))
    cam = db.db.write_camera(Camera(model=model, width=640, height=480, params=params, has_prior_focal_length=False))
    for k, kp in enumerate(scene["keypoints"]):
        db.add_keypoints(db.add_image(f"view{k}.png", cam), kp)
    rs = np.random.RandomState(23)
    for (i, j), f, n in zip(pairs, F, w):
        both = np.nonzero(scene["visible"][i] & scene["visible"][j])[0]
        assert len(both) == int(n)
        m = np.stack([both, both], axis=1).astype(np.uint32)
        if f is not None:
            db.db.write_two_view_geometry(i + 1, j + 1, m, tv.CONFIG_UNCALIBRATED, F=np.asarray(f).reshape(3, 3), commit=False)
        if matches:
            free = [np.nonzero(~scene["visible"][v])[0] for v in (i, j)]
            wrong = np.stack([rs.choice(free[0], len(both) // 10, replace=False), rs.choice(free[1], len(both) // 10, replace=False)], axis=1)
            db.db.write_matches(i + 1, j + 1, np.concatenate([m, wrong.astype(np.uint32)]), commit=False)
    db.db.commit()
    db.db.close()
    return cam
