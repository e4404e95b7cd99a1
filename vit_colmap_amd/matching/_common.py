"""What the estimators share (two_view.py, essential.py, pose.py and mapping/absolute_pose.py): the constants of the
verification rule, the published sampler, the front ends of the two-view scoring kernels (csrc/two_view.hip), the batch
layout of a chunk of pairs or problems and the tail of the RANSAC, which is the same for F, H, E and the absolute pose
whatever residual scores them.  matching/two_view.py re-exports the two-view part under these names."""
import numpy as np
import torch

from .. import _lib

CONFIG_UNDEFINED, CONFIG_DEGENERATE, CONFIG_CALIBRATED, CONFIG_UNCALIBRATED = 0, 1, 2, 3
CONFIG_PLANAR, CONFIG_PANORAMIC, CONFIG_PLANAR_OR_PANORAMIC = 4, 5, 6
MIN_NUM_INLIERS = 15
MAX_ERROR = 4.0
MAX_H_INLIER_RATIO = 0.8
MIN_INLIER_RATIO = 0.25
NUM_HYP_F, NUM_HYP_H = 512, 128
NUM_CANDIDATES = 32
SALT = {"F": 0x0F0F0F0F, "H": 0x3C3C3C3C, "E": 0x5A5A5A5A, "P": 0x96969696, "T": 0xC3C3C3C3}
MODEL_CODE = {"F": 0, "H": 1}
_M32 = 0xFFFFFFFF


def _lowbias32(x):
    """int64 tensor holding 32-bit values -> lowbias32 hash (Python-int constants keep the products below 2^63)."""
    x = x & _M32
    x = x ^ (x >> 16)
    x = (x * 0x7FEB352D) & _M32
    x = x ^ (x >> 15)
    x = (x * 0x846CA68B) & _M32
    return x ^ (x >> 16)


def _sample_indices(seeds, counts, n_hyp, S, salt):
    """seeds, counts int64 (P,) -> int64 (P, n_hyp, S): the first S distinct values of hash(seed, k, j) mod M, -1 if void."""
    dev = seeds.device
    P = seeds.shape[0]
    k = torch.arange(n_hyp, dtype=torch.int64, device=dev)[None, :, None]
    j = torch.arange(NUM_CANDIDATES, dtype=torch.int64, device=dev)[None, None, :]
    # 32-bit wrap-around arithmetic on int64: every product is reduced before it can reach 2^63
    x = ((seeds[:, None, None] & _M32) * 0x9E3779B1) & _M32
    x = (x + ((k * 0x85EBCA6B) & _M32) + ((j * 0xC2B2AE35) & _M32) + salt) & _M32
    cand = _lowbias32(x) % counts[:, None, None].clamp(min=1)
    chosen = torch.full((P, n_hyp, S), -1, dtype=torch.int64, device=dev)
    count = torch.zeros((P, n_hyp), dtype=torch.int64, device=dev)
    slot = torch.arange(S, dtype=torch.int64, device=dev)[None, None, :]
    for jj in range(NUM_CANDIDATES):
        c = cand[:, :, jj]
        take = ~(chosen == c[:, :, None]).any(dim=2) & (count < S)
        put = take[:, :, None] & (slot == count[:, :, None])
        chosen = torch.where(put, c[:, :, None], chosen)
        count = count + take.to(torch.int64)
    return torch.where((count < S)[:, :, None], torch.full_like(chosen, -1), chosen)


def _score(pts, offsets, hyp, model, max_error):
    lib = _lib.load()
    P, K, _ = hyp.shape
    counts = torch.zeros((P, K), dtype=torch.int32, device=pts.device)
    _lib.check(lib.vc_two_view_score(_lib.ptr(pts), _lib.ptr(offsets), P, _lib.ptr(hyp), K, MODEL_CODE[model], float(max_error),
                                     _lib.ptr(counts), _lib.stream_ptr()), "vc_two_view_score")
    return counts


def _mask(pts, offsets, models, model, max_error):
    lib = _lib.load()
    mask = torch.zeros((pts.shape[0],), dtype=torch.uint8, device=pts.device)
    _lib.check(lib.vc_two_view_inliers(_lib.ptr(pts), _lib.ptr(offsets), models.shape[0], _lib.ptr(models), MODEL_CODE[model],
                                       float(max_error), _lib.ptr(mask), _lib.stream_ptr()), "vc_two_view_inliers")
    return mask.bool()


def _solve_minimal(entry, needs, points, offsets, samples, max_solutions, width):
    """The front end of a minimal-solver kernel (csrc/minimal_solver.h).  points: the float64 arrays of the correspondences,
    in the entry point's order; offsets int32 (P + 1), samples int32 (P, n_hyp, S), all on one GPU
    -> solutions float64 (P, n_hyp, max_solutions, width) (NaN past the count), count int32 (P, n_hyp)."""
    if not (points[0].is_cuda and all(p.dtype == torch.float64 for p in points) and offsets.dtype == torch.int32
            and samples.dtype == torch.int32):
        raise ValueError(f"{needs} and int32 offsets / samples on the GPU")
    lib = _lib.load()
    P, n_hyp = int(samples.shape[0]), int(samples.shape[1])
    points, offsets, samples = [p.contiguous() for p in points], offsets.contiguous(), samples.contiguous()
    out = torch.empty((P, n_hyp, max_solutions, width), dtype=torch.float64, device=points[0].device)
    count = torch.zeros((P, n_hyp), dtype=torch.int32, device=points[0].device)
    _lib.check(getattr(lib, entry)(*map(_lib.ptr, points), _lib.ptr(offsets), P, _lib.ptr(samples), n_hyp, _lib.ptr(out),
                                   _lib.ptr(count), _lib.stream_ptr()), entry)
    return out, count


def _pair_batch(rows, seeds, device):
    """The device layout of a chunk of pairs.  rows: one (M_i, 4) array per pair, seeds: one integer per pair (or None)
    -> points (sum M_i, 4) in the arrays' dtype, offsets int32 (P + 1,), pair_of int64 (sum M_i,) the pair of every
    row, seeds int64 (P,) cut to 32 bits (None where none were given)."""
    pts = torch.from_numpy(np.concatenate(rows)).to(device).contiguous()
    offsets = torch.tensor(np.concatenate([[0], np.cumsum([len(r) for r in rows])]), dtype=torch.int32, device=device)
    pair_of = torch.repeat_interleave(torch.arange(len(rows), device=device), (offsets[1:] - offsets[:-1]).to(torch.int64))
    if seeds is not None:
        seeds = torch.tensor([int(s) & _M32 for s in seeds], dtype=torch.int64, device=device)
    return pts, offsets, pair_of, seeds


def _best_hypothesis(counts):
    """counts int64 (P, n) -> the index of the hypothesis with most inliers (P,), the lowest on ties."""
    n = counts.shape[1]
    key = counts * n + (n - 1 - torch.arange(n, device=counts.device))[None, :]
    return (n - 1) - (key.max(dim=1).values % n)


def _ransac_tail(hyp32, counts, score, mask, refit):
    """What every estimator does once its hypotheses hyp32 float32 (P, n, W) are scored (counts int64 (P, n)): take the
    best one (_best_hypothesis) and mask it; `refit(mask, nbest) -> (float32 (P, W), ok bool (P,))` fits one model to those
    inliers; the refit is taken iff it is `ok` and has no fewer inliers.  The residual is the caller's:
    `score(float32 (P, n, W)) -> counts (P, n)` and `mask(float32 (P, W)) -> bool (total,)`.  -> final model float32 (P, W)
    (NaN where it has no inlier), its inlier mask bool (total,), its count int64 (P,), kbest (P,), refit taken? bool (P,)."""
    kbest = _best_hypothesis(counts)
    rows = torch.arange(counts.shape[0], device=counts.device)
    best, nbest = hyp32[rows, kbest].contiguous(), counts[rows, kbest]
    refit32, ok = refit(mask(best), nbest)
    rcount = score(refit32[:, None, :].contiguous()).to(torch.int64)[:, 0]
    use = ok & (rcount >= nbest)
    final = torch.where(use[:, None], refit32, best).contiguous()
    fmask = mask(final)
    fcount = torch.where(use, rcount, nbest)
    final = torch.where((fcount > 0)[:, None], final, torch.full_like(final, float("nan")))
    return final, fmask, fcount, kbest, use
