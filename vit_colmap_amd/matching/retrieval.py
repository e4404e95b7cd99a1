"""Retrieval matching over a COLMAP database: every image is matched only to its k nearest images.

The exhaustive matcher visits all n (n - 1) / 2 pairs; most of them share no scene content.  This module chooses the
pairs first — the part COLMAP's vocabulary-tree matcher and hloc's "pairs from retrieval" play there; the rule is the
build's own, published in tests/util_retrieval.py, and parity with either is not claimed:

  1. pool     sums[i] = sum of image i's uint8 descriptor rows, int32                      (device, vc_pool_descriptors_u8)
  2. global   mean-pooled, centred on the mean over the images, unit norm, quantised to int8   (host, numpy float64, n x D)
  3. search   score[i, j] = q[i] . q[j] in int32; the k best j != i by (score desc, index asc)  (device, vc_retrieval_topk_i8)
  4. pairs    the set of (min, max) over all neighbours, ascending: a sub-sequence of the exhaustive list

Steps 1 and 3 are integer, so the neighbour lists equal the numpy rule bit for bit and are the same on every rank.
`match_retrieval` then runs the body of `match_exhaustive` (matching/exhaustive.py: match_database) on that list: only
the selected pairs are matched and verified and only they get `matches` and `two_view_geometries` rows, as COLMAP's
non-exhaustive matchers do.
"""
import logging
import time

import numpy as np
import torch

from .. import _lib
from .exhaustive import match_database

logger = logging.getLogger(__name__)

Q_PAD = 32   # the search kernel takes rows of a multiple of 32 bytes (one MFMA k-step), zero padded


def _to_device(x, dtype, device):
    t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x, dtype))
    return t.to(device).contiguous()


def pool_descriptors(block, counts, device="cuda") -> np.ndarray:
    """uint8 blocks [n][n_max][D] + counts int32 [n] (host or device) -> int32 (n, D): the sum of each image's first
    counts[i] rows, on the device.  Blocks with more rows than one kernel block holds (VC_MAX_KEYPOINTS; match_exhaustive
    takes them too, hip_match_blocks) are pooled in row sub-blocks of that many rows, each a contiguous copy with its
    counts moved down and cut to the sub-block: integer sums add, so the result is the same."""
    if not torch.cuda.is_available():
        raise _lib.HipLibraryError("descriptor pooling is HIP-only (no CPU fallback): no GPU visible")
    d_desc, d_counts = _to_device(block, np.uint8, device), _to_device(counts, np.int32, device)
    assert d_desc.dtype == torch.uint8 and d_desc.dim() == 3 and d_counts.dtype == torch.int32
    n, n_max, D = d_desc.shape
    d_counts = d_counts.reshape(-1)
    assert d_counts.numel() == n
    if D > _lib.VC_MAX_DESC_DIM:
        raise _lib.HipLibraryError(f"descriptors of {D} bytes exceed the kernels' limit ({_lib.VC_MAX_DESC_DIM})")
    sums = torch.zeros((n, D), dtype=torch.int32, device=d_desc.device)
    if n == 0 or n_max == 0 or D == 0:
        return sums.cpu().numpy()
    lib = _lib.load()
    step = _lib.VC_MAX_KEYPOINTS
    part = sums if n_max <= step else torch.empty_like(sums)             # (the kernel zeroes what it writes)
    for r0 in range(0, n_max, step):
        rows = min(step, n_max - r0)
        sub = d_desc if n_max <= step else d_desc[:, r0:r0 + rows].contiguous()
        sub_counts = d_counts if r0 == 0 else (d_counts - r0).clamp_(min=0)      # the kernel cuts counts above `rows`
        _lib.check(lib.vc_pool_descriptors_u8(_lib.ptr(sub), _lib.ptr(sub_counts), n, rows, D, _lib.ptr(part),
                                              _lib.stream_ptr()), "vc_pool_descriptors_u8")
        if part is not sums:
            sums += part
    return sums.cpu().numpy()


def global_descriptors(sums, counts):
    """int32 sums (n, D) + counts (n,) -> (q int8 (n, D rounded up to a multiple of 32, zero padded), valid int32 (n,)).
    The host step of the rule, numpy float64: mean row of every image with descriptors, centred on the mean of those
    rows over the images, scaled to unit norm (0 where the norm is 0), times S = 127 sqrt(D) / 4, rounded half to even
    and clipped to +-127.  Rows of images without descriptors are 0."""
    sums = np.asarray(sums, np.float64)
    counts = np.asarray(counts, np.int64).reshape(-1)
    n, D = sums.shape
    valid = counts > 0
    q = np.zeros((n, -(-max(D, 1) // Q_PAD) * Q_PAD), np.int8)
    if valid.any():
        m = sums[valid] / counts[valid, None].astype(np.float64)
        g = m - m.mean(axis=0)
        norm = np.sqrt((g * g).sum(axis=1))
        g = np.divide(g, norm[:, None], out=np.zeros_like(g), where=norm[:, None] > 0)
        scale = 127.0 * np.sqrt(float(D)) / 4.0
        q[valid, :D] = np.clip(np.rint(g * scale), -127, 127).astype(np.int8)
    return q, valid.astype(np.int32)


def nearest_images(q, valid, k, device="cuda", return_scores=False):
    """int8 q (n, d_pad) + valid int32 (n,) -> int32 (n, k): every valid image's k best valid other images by (score
    descending, index ascending), -1 behind the last candidate and in the rows of invalid images; on the device.
    return_scores: also the int32 scores (INT32_MIN where the index is -1)."""
    if not torch.cuda.is_available():
        raise _lib.HipLibraryError("the image search is HIP-only (no CPU fallback): no GPU visible")
    k = int(k)
    if not 1 <= k <= _lib.VC_MAX_NEIGHBOURS:
        raise ValueError(f"k = {k} is outside 1 .. VC_MAX_NEIGHBOURS = {_lib.VC_MAX_NEIGHBOURS}")
    d_q, d_valid = _to_device(q, np.int8, device), _to_device(valid, np.int32, device)
    assert d_q.dtype == torch.int8 and d_q.dim() == 2 and d_valid.dtype == torch.int32
    n, d_pad = d_q.shape
    assert d_valid.numel() == n
    idx = torch.empty((n, k), dtype=torch.int32, device=d_q.device)
    score = torch.empty((n, k), dtype=torch.int32, device=d_q.device)
    if n:
        lib = _lib.load()
        nbytes = lib.vc_retrieval_workspace_bytes(n, d_pad, k)
        if nbytes == 0:
            raise _lib.HipLibraryError(f"unsupported search shape n={n} d_pad={d_pad} k={k}")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=d_q.device)
        _lib.check(lib.vc_retrieval_topk_i8(_lib.ptr(d_q), _lib.ptr(d_valid), n, d_pad, k, _lib.ptr(idx), _lib.ptr(score),
                                            _lib.ptr(ws), nbytes, _lib.stream_ptr()), "vc_retrieval_topk_i8")
    return (idx.cpu().numpy(), score.cpu().numpy()) if return_scores else idx.cpu().numpy()


def retrieval_pairs(neighbours) -> np.ndarray:
    """int (n, k) neighbour lists (-1 = none) -> int32 (P, 2): the set of (min(i, j), max(i, j)), ascending by (a, b) —
    a sub-sequence of hip_matcher.exhaustive_pairs(n)."""
    nb = np.asarray(neighbours, np.int64)
    nb = nb.reshape(len(nb), -1)
    i, j = np.nonzero(nb >= 0)
    j = nb[i, j]
    keep = i != j
    a, b = np.minimum(i, j)[keep], np.maximum(i, j)[keep]
    codes = np.unique(a * len(nb) + b)
    return np.stack([codes // max(len(nb), 1), codes % max(len(nb), 1)], axis=1).astype(np.int32).reshape(-1, 2)


def hip_neighbours(block, counts, k, device="cuda") -> np.ndarray:
    """The device path of the selection: pool, global descriptors, search -> int32 (n, k)."""
    sums = pool_descriptors(block, counts, device=device)
    q, valid = global_descriptors(sums, np.asarray(counts.cpu() if torch.is_tensor(counts) else counts))
    return nearest_images(q, valid, k, device=device)


def check_num_neighbors(num_neighbors) -> int:
    """num_neighbors < 1: ValueError; above VC_MAX_NEIGHBOURS: clamped, with one log line."""
    k = int(num_neighbors)
    if k < 1:
        raise ValueError(f"num_neighbors must be at least 1 (got {num_neighbors})")
    if k > _lib.VC_MAX_NEIGHBOURS:
        logger.warning("num_neighbors = %d is above VC_MAX_NEIGHBOURS: clamped to %d", k, _lib.VC_MAX_NEIGHBOURS)
        k = _lib.VC_MAX_NEIGHBOURS
    return k


def match_retrieval(database_path: str, matching_options=None, sift_options=None, num_neighbors: int = 20, device="cuda",
                    distributed=None, match_fn=None, verify: bool = True, verify_fn=None, guided_fn=None,
                    neighbour_fn=None, pair_chunk: int = 16384) -> dict:
    """`match_exhaustive` on the pairs (image, one of its `num_neighbors` nearest images) only: same database-in /
    database-out contract, same options, same `match_fn` / `verify_fn` / `guided_fn` stand-ins, same multi-rank
    behaviour (rank 0 also chooses the pairs and broadcasts the list; pair p of it goes to rank p % world).  Guided
    matching and relative pose run unchanged on the selected pairs.
    `neighbour_fn(block, counts, k) -> (n, k)` replaces the device path of the selection (hip_neighbours) in the CPU
    tests, as `match_fn` replaces the matcher.
    The stats dict of match_exhaustive, where `pairs` is the number of pairs matched, plus `num_neighbors`,
    `candidate_pairs` (= n (n - 1) / 2) and `retrieval_s` (the selection, rank 0's wall time)."""
    k = check_num_neighbors(num_neighbors)
    if neighbour_fn is None:
        if not torch.cuda.is_available():
            raise _lib.HipLibraryError("match_retrieval needs an MI355X: the image search is HIP-only (no CPU fallback)")

        def neighbour_fn(block, counts, kk):
            return hip_neighbours(block, counts, kk, device=device)

    def select_pairs(block, counts, stats):
        t0 = time.perf_counter()
        n = len(counts)
        nb = np.asarray(neighbour_fn(block, counts, min(k, max(n - 1, 1))), np.int64).reshape(n, -1)
        pairs = retrieval_pairs(nb)
        stats["retrieval_s"] = time.perf_counter() - t0
        logger.info("retrieval: %d of %d pairs selected (%d neighbours per image)", len(pairs), n * (n - 1) // 2, k)
        return pairs

    stats = match_database(database_path, matching_options, sift_options, device, pair_chunk, distributed, match_fn, verify,
                           verify_fn, guided_fn, select_pairs=select_pairs, what="match_retrieval")
    n = stats["images"]
    stats["num_neighbors"] = k
    stats["candidate_pairs"] = n * (n - 1) // 2
    stats.setdefault("retrieval_s", 0.0)                                      # (fewer than two images: nothing was selected)
    return stats
