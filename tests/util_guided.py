"""Guided matching: the numpy specification the HIP kernel is compared with, and the "twin" scenes the tests use.

The rule is built from the two oracles only: the int32 similarity matrix and the top-2 / angle / ratio /
cross-check rule of oracle/matcher_oracle.py, applied to a matrix in which every candidate (i, j) that is not an inlier of
the pair's model under oracle/two_view_oracle.py inliers_f32 holds 0 — the matcher's "never matches, never a runner-up"
value."""
import numpy as np

from oracle import matcher_oracle as mo
from oracle import two_view_oracle as tv


def admissible(kp1, kp2, kind, m9, max_error):
    """bool (n1, n2): inliers_f32 of every candidate pair of keypoints (first two columns) under the model."""
    n1, n2 = len(kp1), len(kp2)
    if n1 == 0 or n2 == 0:
        return np.zeros((n1, n2), bool)
    k1 = np.asarray(kp1, np.float32)[:, :2]
    k2 = np.asarray(kp2, np.float32)[:, :2]
    pts = np.concatenate([np.repeat(k1, n2, axis=0), np.tile(k2, (n1, 1))], axis=1)
    return tv.inliers_f32(kind, m9, pts, max_error).reshape(n1, n2)


def guided_match_pair(d1, d2, kp1, kp2, kind, m9, max_error=tv.MAX_ERROR, max_ratio=0.8, max_distance=0.7,
                      cross_check=True):
    """uint8 (n1, D), (n2, D), keypoints (n, >= 2), kind "F" | "H", model float32 (9,) -> uint32 (M, 2) ordered by i."""
    if len(d1) == 0 or len(d2) == 0:
        return np.zeros((0, 2), np.uint32)
    S = np.where(admissible(kp1, kp2, kind, m9, max_error), mo.similarity(d1, d2), 0).astype(np.int32)
    m12 = mo.one_way(S, max_ratio, max_distance)
    i = np.nonzero(m12 >= 0)[0]
    if cross_check:
        m21 = mo.one_way(np.ascontiguousarray(S.T), max_ratio, max_distance)
        i = i[m21[m12[i]] == i]
    return np.stack([i, m12[i]], axis=1).astype(np.uint32)


def twin_descriptors(rs, n, n_unique, D, views):
    """`views` uint8 (n, D) descriptor sets of the same n points: rows n_unique, n_unique + 2, ... share their base with the
    next row (look-alikes), every view adds its own noise."""
    base = np.abs(rs.standard_normal((n, D))).astype(np.float32)
    twin = np.arange(n_unique, n - 1, 2)
    base[twin + 1] = base[twin]
    out = []
    for _ in range(views):
        d = np.abs(base + 0.05 * rs.standard_normal(base.shape).astype(np.float32))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        out.append(np.clip(d * 512, 0, 255).astype(np.uint8))
    return out


def twin_scene(seed, n, n_unique, planar=False, D=128):
    """-> kp1, kp2 float32 (n, 2) (point i of view 1 is point i of view 2, no outliers), d1, d2 uint8 (n, D), and the
    bool (n,) mask of the rows that have a look-alike."""
    kp1, kp2, _, _ = tv.synthetic_two_view(seed, n, 0.0, planar)
    d1, d2 = twin_descriptors(np.random.RandomState(seed), n, n_unique, D, 2)
    is_twin = np.arange(n) >= n_unique
    if (n - n_unique) % 2:
        is_twin[-1] = False          # an odd row out has no partner
    return kp1, kp2, d1, d2, is_twin


def plain_inliers(kp1, kp2, d1, d2, kind_wanted="F", seed=1234):
    """Unguided matches, the oracle's model of `kind_wanted` on them and its inliers: (matches, model9, inlier matches)."""
    m = mo.match_pair(d1, d2)
    pts = np.concatenate([kp1[m[:, 0], :2], kp2[m[:, 1], :2]], axis=1).astype(np.float32)
    m9, mask = tv.estimate_model(kind_wanted, pts, seed, tv.NUM_HYP_F if kind_wanted == "F" else tv.NUM_HYP_H)
    return m, m9, m[mask]
