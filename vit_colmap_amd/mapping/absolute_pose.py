"""Image registration: the absolute pose of an image from 2D-3D correspondences, a minimal P3P solver
inside RANSAC, every image of a batch in the same launches.  Specification: tests/util_absolute_pose.py.  This build's own
published rule; parity with COLMAP's absolute-pose estimator is unpinned.

Where the work runs
  HIP     the P3P solver, every sample of every problem in one launch (csrc/absolute_pose.hip, vc_p3p); the inlier counts
          of every hypothesis and the masks (vc_absolute_pose_score, vc_absolute_pose_inliers)
  torch   the sampler and the tail of the RANSAC (matching/_common.py), P = K [R | t], the Gauss-Newton refit over the best
          hypothesis' inliers (batched float64, a 6x6 solve per problem and step) — plumbing, as the refit SVDs of estimate_e are
  host    K^-1 per problem, the acceptance rule, the quaternion
"""
from functools import partial

import numpy as np
import torch

from .. import _lib
from ..matching._common import SALT, _best_hypothesis, _pair_batch, _ransac_tail, _sample_indices, _solve_minimal
from ..matching.essential import rot_to_quat

NUM_HYP_P = 128
MAX_SOLUTIONS = 4
ABS_POSE_MAX_ERROR = 12.0            # px  [recalled: COLMAP IncrementalMapperOptions default]
ABS_POSE_MIN_NUM_INLIERS = 30        #     [recalled: COLMAP IncrementalMapperOptions default]
ABS_POSE_MIN_INLIER_RATIO = 0.25     #     [recalled: COLMAP IncrementalMapperOptions default]
INIT_MIN_TRI_ANGLE = float(np.radians(16.0))     # [recalled: COLMAP IncrementalMapperOptions default]
INIT_MIN_NUM_INLIERS = 100           #     [recalled: COLMAP IncrementalMapperOptions default]
FILTER_MIN_TRI_ANGLE = float(np.radians(1.5))    # [recalled: COLMAP IncrementalMapperOptions default]
REFIT_STEPS = 10


def solve_p3p(rays_n, xyz, offsets, samples):
    """rays_n float64 (total, 2), xyz float64 (total, 3), offsets int32 (P + 1), samples int32 (P, n_hyp, 3), all on one GPU
    -> pose float64 (P, n_hyp, 4, 12) (R row-major then t; NaN past the count), count int32 (P, n_hyp)."""
    return _solve_minimal("vc_p3p", "solve_p3p needs float64 rays and points", [rays_n, xyz], offsets, samples, MAX_SOLUTIONS, 12)


def score_poses(obs, xyz4, offsets, hyp, max_error):
    """obs float32 (total, 2) px, xyz4 float32 (total, 4), hyp float32 (P, n, 12) -> inlier counts int32 (P, n)."""
    lib = _lib.load()
    P, n, _ = hyp.shape
    counts = torch.zeros((P, n), dtype=torch.int32, device=obs.device)
    _lib.check(lib.vc_absolute_pose_score(_lib.ptr(obs), _lib.ptr(xyz4), _lib.ptr(offsets), P, _lib.ptr(hyp), n, float(max_error),
                                          _lib.ptr(counts), _lib.stream_ptr()), "vc_absolute_pose_score")
    return counts


def pose_masks(obs, xyz4, offsets, models, max_error):
    """models float32 (P, 12) -> inlier mask bool (total,)."""
    lib = _lib.load()
    mask = torch.zeros((obs.shape[0],), dtype=torch.uint8, device=obs.device)
    _lib.check(lib.vc_absolute_pose_inliers(_lib.ptr(obs), _lib.ptr(xyz4), _lib.ptr(offsets), models.shape[0], _lib.ptr(models),
                                            float(max_error), _lib.ptr(mask), _lib.stream_ptr()), "vc_absolute_pose_inliers")
    return mask.bool()


def projection_matrices(K, R, t):
    """K (P, 3, 3) without skew, R (P, n, 3, 3), t (P, n, 3) float64 -> P = K [R | t] float32 (P, n, 12), in the
    specification's order: row 0 = fx r0 + cx r2, row 1 = fy r1 + cy r2, row 2 = r2."""
    Rt = torch.cat([R, t[..., None]], dim=-1)
    fx, fy, cx, cy = (K[:, i, j][:, None, None] for i, j in ((0, 0), (1, 1), (0, 2), (1, 2)))
    P34 = torch.stack([fx * Rt[:, :, 0] + cx * Rt[:, :, 2], fy * Rt[:, :, 1] + cy * Rt[:, :, 2], Rt[:, :, 2]], dim=2)
    return P34.reshape(P34.shape[0], P34.shape[1], 12).to(torch.float32).contiguous()


def _rodrigues(w):
    """Rotation vectors (P, 3) -> rotation matrices (P, 3, 3)."""
    th = torch.linalg.norm(w, dim=1)
    z = torch.zeros_like(th)
    W = torch.stack([z, -w[:, 2], w[:, 1], w[:, 2], z, -w[:, 0], -w[:, 1], w[:, 0], z], dim=1).reshape(-1, 3, 3)
    small = th < 1e-12
    ths = torch.where(small, torch.ones_like(th), th)
    a = torch.where(small, torch.ones_like(th), torch.sin(ths) / ths)
    b = torch.where(small, torch.zeros_like(th), (1 - torch.cos(ths)) / (ths * ths))
    return torch.eye(3, dtype=w.dtype, device=w.device)[None] + a[:, None, None] * W + b[:, None, None] * (W @ W)


def _reprojection(K, R, t, obs, xyz, prob_of):
    Xc = (R[prob_of] @ xyz[:, :, None])[:, :, 0] + t[prob_of]
    r = torch.stack([K[prob_of, 0, 0] * Xc[:, 0] / Xc[:, 2] + K[prob_of, 0, 2] - obs[:, 0],
                     K[prob_of, 1, 1] * Xc[:, 1] / Xc[:, 2] + K[prob_of, 1, 2] - obs[:, 1]], dim=1)
    return Xc, r


def refit_poses(K, R, t, obs, xyz, prob_of, weight, steps=REFIT_STEPS):
    """At most `steps` Gauss-Newton steps on (rotation vector, t), R <- exp(w) R, per problem, minimising the pixel
    reprojection error over the correspondences with weight 1; a problem keeps a step only if it lowers its cost and stops at
    the first step it does not keep.  All float64 on the device."""
    P = K.shape[0]

    def cost_of(r):
        c = torch.where(weight > 0, (r * r).sum(dim=1), torch.zeros_like(weight))
        return torch.zeros((P,), dtype=r.dtype, device=r.device).index_add_(0, prob_of, c)

    Xc, r = _reprojection(K, R, t, obs, xyz, prob_of)
    cost = cost_of(r)
    active = torch.ones((P,), dtype=torch.bool, device=K.device)
    for _ in range(steps):
        iz = 1.0 / Xc[:, 2]
        fx, fy = K[prob_of, 0, 0], K[prob_of, 1, 1]
        zero = torch.zeros_like(iz)
        du = torch.stack([fx * iz, zero, -fx * Xc[:, 0] * iz * iz], dim=1)                  # d u / d Xc
        dv = torch.stack([zero, fy * iz, -fy * Xc[:, 1] * iz * iz], dim=1)
        Y = (R[prob_of] @ xyz[:, :, None])[:, :, 0]                                        # d Xc / d w = -[R X]x
        Ju = torch.cat([torch.linalg.cross(Y, du), du], dim=1)
        Jv = torch.cat([torch.linalg.cross(Y, dv), dv], dim=1)
        keep = (weight > 0)[:, None]
        Ju, Jv = torch.where(keep, Ju, torch.zeros_like(Ju)), torch.where(keep, Jv, torch.zeros_like(Jv))
        rw = torch.where(keep, r, torch.zeros_like(r))
        JtJ = torch.zeros((P, 6, 6), dtype=K.dtype, device=K.device).index_add_(
            0, prob_of, Ju[:, :, None] * Ju[:, None, :] + Jv[:, :, None] * Jv[:, None, :])
        Jtr = torch.zeros((P, 6), dtype=K.dtype, device=K.device).index_add_(0, prob_of, Ju * rw[:, :1] + Jv * rw[:, 1:])
        step = torch.linalg.solve_ex(JtJ, -Jtr[:, :, None]).result[:, :, 0]                # singular: not finite, not kept
        step = torch.where(torch.isfinite(step).all(dim=1, keepdim=True), step, torch.full_like(step, float("nan")))
        R2, t2 = _rodrigues(step[:, :3]) @ R, t + step[:, 3:]
        Xc2, r2 = _reprojection(K, R2, t2, obs, xyz, prob_of)
        cost2 = cost_of(r2)
        take = active & (cost2 < cost)                                                      # false for NaN
        active = take
        R, t = torch.where(take[:, None, None], R2, R), torch.where(take[:, None], t2, t)
        cost = torch.where(take, cost2, cost)
        Xc, r = torch.where(take[prob_of][:, None], Xc2, Xc), torch.where(take[prob_of][:, None], r2, r)
    return R, t


def _failure(n):
    return dict(success=False, qvec=np.array([1.0, 0.0, 0.0, 0.0]), tvec=np.zeros(3), num_inliers=0, inlier_mask=np.zeros(n, bool))


def estimate_absolute_poses(problems, device, max_error=ABS_POSE_MAX_ERROR, n_hyp=NUM_HYP_P):
    """All problems in one batch.  problems: list of dict(obs (n, 2) px, xyz (n, 3), K (3, 3), seed)
    -> per problem dict(success, qvec (w, x, y, z), tvec, num_inliers, inlier_mask bool (n,)), X_cam = R X + t."""
    n_prob = len(problems)
    sizes = [len(np.asarray(p["obs"]).reshape(-1, 2)) for p in problems]
    if n_prob == 0 or sum(sizes) == 0:
        return [_failure(n) for n in sizes]
    obs32 = np.concatenate([np.asarray(p["obs"], np.float32).reshape(-1, 2) for p in problems])
    xyz32 = np.concatenate([np.asarray(p["xyz"], np.float32).reshape(-1, 3) for p in problems])
    Kn = np.stack([np.asarray(p["K"], np.float64).reshape(3, 3) for p in problems])
    Ki = np.linalg.inv(Kn)
    which = np.repeat(np.arange(n_prob), sizes)
    rays = obs32.astype(np.float64) * np.stack([Ki[which, 0, 0], Ki[which, 1, 1]], axis=1) + np.stack([Ki[which, 0, 2], Ki[which, 1, 2]], axis=1)

    xyz4_rows = np.split(np.concatenate([xyz32, np.ones((len(xyz32), 1), np.float32)], axis=1), np.cumsum(sizes)[:-1])
    xyz4, offsets, prob_of, seeds = _pair_batch(xyz4_rows, [p["seed"] for p in problems], device)
    obs, xyz64 = torch.from_numpy(obs32).to(device).contiguous(), xyz4[:, :3].to(torch.float64).contiguous()
    rays = torch.from_numpy(rays).to(device).contiguous()
    K = torch.from_numpy(Kn).to(device)

    idx = _sample_indices(seeds, (offsets[1:] - offsets[:-1]).to(torch.int64), n_hyp, 3, SALT["P"]).to(torch.int32).contiguous()
    pose, _ = solve_p3p(rays, xyz64, offsets, idx)
    pose = pose.reshape(n_prob, n_hyp * MAX_SOLUTIONS, 12)                                   # ranked by (sample, solution)
    hyp32 = projection_matrices(K, pose[:, :, :9].reshape(n_prob, -1, 3, 3), pose[:, :, 9:])
    score = partial(score_poses, obs, xyz4, offsets, max_error=max_error)
    counts = score(hyp32).to(torch.int64)
    rows = torch.arange(n_prob, device=counts.device)
    refit64 = None

    def refit(mask, nbest):                                                                  # Gauss-Newton from the best hypothesis
        nonlocal refit64
        best = torch.nan_to_num(pose[rows, _best_hypothesis(counts)])                        # NaN only where nbest is 0
        Rr, tr = refit_poses(K, best[:, :9].reshape(n_prob, 3, 3), best[:, 9:], obs.to(torch.float64), xyz64, prob_of,
                             mask.to(torch.float64))
        refit64 = torch.cat([Rr.reshape(n_prob, 9), tr], dim=1)
        return projection_matrices(K, Rr[:, None], tr[:, None])[:, 0], torch.isfinite(refit64).all(dim=1) & (nbest > 0)

    _, fmask, fcount, kbest, use = _ransac_tail(hyp32, counts, score, partial(pose_masks, obs, xyz4, offsets, max_error=max_error), refit)
    final = torch.where(use[:, None], refit64, pose[rows, kbest]).cpu().numpy()              # R row-major, then t
    fmask, fcount = fmask.cpu().numpy(), fcount.cpu().numpy()

    out, lo = [], 0
    for p, size in enumerate(sizes):
        num = int(fcount[p])
        if num == 0:
            out.append(_failure(size))
        else:
            ok_p = num >= ABS_POSE_MIN_NUM_INLIERS and num / size >= ABS_POSE_MIN_INLIER_RATIO
            out.append(dict(success=bool(ok_p), qvec=rot_to_quat(final[p, :9].reshape(3, 3)), tvec=final[p, 9:].copy(), num_inliers=num,
                            inlier_mask=fmask[lo:lo + size].copy()))
        lo += size
    return out
