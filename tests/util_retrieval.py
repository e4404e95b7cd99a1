"""Retrieval matching: the rule as numpy (the specification of vit_colmap_amd/matching/retrieval.py and of
csrc/retrieval.hip) and the "trajectory" test input.

The rule, for images 0..n-1 in ascending id order, uint8 descriptor blocks [n][n_max][D] and counts[n]:
  1. pool       sums[i, :] = sum over r < counts[i] of desc[i, r, :], int32                     (device, exact)
  2. global     valid = counts > 0; m = sums / counts; c = mean of m over the valid images; g = m - c;
                g /= |g| where the norm is > 0, else 0; q = clip(rint(g S), -127, 127) int8, S = 127 sqrt(D) / 4;
                rows of invalid images 0; columns zero padded                                    (host, float64)
  3. neighbours score[i, j] = q[i] . q[j] in int32; for each valid i the k best valid j != i by (score descending,
                index ascending); -1 behind the last candidate; invalid rows all -1              (device, exact)
  4. pairs      the set of (min(i, j), max(i, j)) over all neighbours, ascending by (a, b)
"""
import numpy as np

from util_data import quantize

INT32_MIN = np.iinfo(np.int32).min


def pool_sums(block, counts):
    block, counts = np.asarray(block), np.asarray(counts)
    out = np.zeros((block.shape[0], block.shape[2]), np.int32)
    for i in range(block.shape[0]):
        out[i] = block[i, : counts[i]].astype(np.int32).sum(axis=0, dtype=np.int32)
    return out


def global_descriptors(sums, counts, pad=32):
    sums = np.asarray(sums).astype(np.float64)
    counts = np.asarray(counts).astype(np.int64)
    n, D = sums.shape
    valid = counts > 0
    q = np.zeros((n, (max(D, 1) + pad - 1) // pad * pad), np.int8)
    if valid.any():
        m = sums[valid] / counts[valid][:, None]
        c = m.mean(axis=0)
        g = m - c
        norm = np.sqrt((g * g).sum(axis=1))
        unit = np.zeros_like(g)
        nz = norm > 0
        unit[nz] = g[nz] / norm[nz][:, None]
        S = 127.0 * np.sqrt(float(D)) / 4.0
        q[valid, :D] = np.clip(np.rint(unit * S), -127, 127).astype(np.int8)
    return q, valid.astype(np.int32)


def neighbours(q, valid, k, row_chunk=1024):
    """-> (idx int32 (n, k), score int32 (n, k)); INT32_MIN where idx is -1.  The products run in float64, where they
    are exact (|score| < 2^24)."""
    q = np.asarray(q, np.int8)
    valid = np.asarray(valid).astype(bool)
    n = len(q)
    idx = np.full((n, k), -1, np.int32)
    score = np.full((n, k), INT32_MIN, np.int32)
    qf = q.astype(np.float64)
    cols = np.nonzero(valid)[0]
    for r0 in range(0, n, row_chunk):
        rows = np.arange(r0, min(r0 + row_chunk, n))
        s = (qf[rows] @ qf[cols].T).astype(np.int64)                 # (rows, valid columns), columns ascending
        order = np.argsort(-s, axis=1, kind="stable")                # score descending, then index ascending
        for t, i in enumerate(rows):
            if not valid[i]:
                continue
            o = order[t]
            o = o[cols[o] != i][:k]
            idx[i, : len(o)] = cols[o]
            score[i, : len(o)] = s[t, o]
    return idx, score


def pairs_of(neigh):
    neigh = np.asarray(neigh)
    found = set()
    for i in range(len(neigh)):
        for j in neigh[i]:
            if j >= 0 and j != i:
                found.add((min(i, int(j)), max(i, int(j))))
    return np.array(sorted(found), np.int32).reshape(-1, 2)


def neighbour_fn(block, counts, k):
    """The whole selection in numpy: stands in for the device path in the CPU tests (match_retrieval's `neighbour_fn`)."""
    block, counts = np.asarray(block), np.asarray(counts)
    q, valid = global_descriptors(pool_sums(block, counts), counts)
    return neighbours(q, valid, k)[0]


def trajectory(seed=7, n=24, w=256, stride=64, D=128):
    """A camera moving along a scene: image i sees a shuffled subset of rows [i stride, i stride + w) of one pool of
    stride (n - 1) + w normal rows, drops up to w / 8 of them and adds noise of 0.2 x the mean absolute pool value;
    rows quantised with util_data.quantize.  -> uint8 [n][w][D], counts int32 [n].  Images |i - j| < w / stride apart
    share rows."""
    rs = np.random.RandomState(seed)
    pool = rs.standard_normal((stride * (n - 1) + w, D))
    sigma = 0.2 * np.abs(pool).mean()
    block = np.zeros((n, w, D), np.uint8)
    counts = np.zeros(n, np.int32)
    for i in range(n):
        rows = i * stride + rs.permutation(w)
        keep = w - rs.randint(0, w // 8 + 1)
        x = pool[rows[:keep]] + sigma * rs.standard_normal((keep, D))
        block[i, :keep] = quantize(x)
        counts[i] = keep
    return block, counts


def make_feature_db(path, block, counts, seed=0, focal_prior=False):
    """A COLMAP database with one PINHOLE camera, image k = `im{k:03d}.png` with counts[k] keypoints and descriptors."""
    from vit_colmap_amd.database import ColmapDatabase

    db = ColmapDatabase(str(path))
    cam = db.add_pinhole_camera(640, 480, 640, 640, 320, 240)
    for k in range(len(counts)):
        i = db.add_image(f"im{k:03d}.png", cam)
        if counts[k]:
            kp = np.random.RandomState(seed + k).rand(int(counts[k]), 2).astype(np.float32) * np.float32([640, 480])
            db.add_keypoints(i, kp)
            db.add_descriptors(i, block[k, : counts[k]])
    db.db.close()
