#!/usr/bin/env python3
"""Image registration (developer tool, bench.py is the judged entry).  Times vc_p3p (hypotheses per second)
and vc_absolute_pose_score (point tests per second) on 64 problems x 128 samples x 1000 correspondences with 30 % outliers
and 0.5 px noise (device events, warm-up launches excluded, the median over --iters launches), then the whole
estimate_absolute_poses batch on a host clock that ends in a synchronise.  The scored hypotheses are the solver's own, so
the scoring kernel sees the NaN slots it sees in use.  Prints one JSON line.  Needs a GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vit_colmap_amd.mapping import absolute_pose as ap  # noqa: E402
from vit_colmap_amd.matching._common import SALT, _sample_indices  # noqa: E402

K = np.array([[600.0, 0, 320.0], [0, 600.0, 240.0], [0, 0, 1]])


def problem(seed, n, outlier_frac=0.3, noise=0.5):
    """n correspondences of one camera looking at a box of points: obs float32 (n, 2) px, xyz float32 (n, 3)."""
    rs = np.random.RandomState(seed)
    a = 0.1 + 0.01 * (seed % 16)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    t = np.array([-0.8, 0.05, 0.1])
    X = np.stack([rs.uniform(-3, 3, n), rs.uniform(-2, 2, n), rs.uniform(4, 9, n)], axis=1)
    p = (K @ (X @ R.T + t).T).T
    obs = p[:, :2] / p[:, 2:] + rs.normal(0, noise, (n, 2))
    wrong = np.stack([rs.uniform(0, 640, n), rs.uniform(0, 480, n)], axis=1)
    obs = np.where((rs.uniform(size=n) >= outlier_frac)[:, None], obs, wrong)
    return dict(obs=obs.astype(np.float32), xyz=X.astype(np.float32), K=K, seed=seed)


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return dict(median=float(np.median(ms)), min=float(np.min(ms)), max=float(np.max(ms)))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--problems", type=int, default=64)
    p.add_argument("--samples", type=int, default=128)
    p.add_argument("--points", type=int, default=1000)
    p.add_argument("--iters", type=int, default=50)
    p.add_argument("--batch-iters", dest="batch_iters", type=int, default=5)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_register needs a GPU: nothing is measured without one")
    problems = [problem(1 + q, a.points) for q in range(a.problems)]
    P, n = a.problems, a.points
    obs32 = np.concatenate([q["obs"] for q in problems])
    xyz32 = np.concatenate([q["xyz"] for q in problems])
    Ki = np.linalg.inv(K)
    rays = torch.from_numpy(obs32.astype(np.float64) * [Ki[0, 0], Ki[1, 1]] + [Ki[0, 2], Ki[1, 2]]).cuda().contiguous()
    xyz64 = torch.from_numpy(xyz32.astype(np.float64)).cuda().contiguous()
    obs = torch.from_numpy(obs32).cuda().contiguous()
    xyz4 = torch.from_numpy(np.concatenate([xyz32, np.ones((len(xyz32), 1), np.float32)], axis=1)).cuda().contiguous()
    offsets = torch.arange(P + 1, dtype=torch.int32, device="cuda") * n
    seeds = torch.arange(1, P + 1, dtype=torch.int64, device="cuda")
    counts_n = torch.full((P,), n, dtype=torch.int64, device="cuda")
    idx = _sample_indices(seeds, counts_n, a.samples, 3, SALT["P"]).to(torch.int32).contiguous()

    solver_ms = timed(lambda: ap.solve_p3p(rays, xyz64, offsets, idx), a.iters)
    pose, count = ap.solve_p3p(rays, xyz64, offsets, idx)
    pose = pose.reshape(P, a.samples * ap.MAX_SOLUTIONS, 12)
    Kd = torch.from_numpy(np.tile(K, (P, 1, 1))).cuda()
    hyp32 = ap.projection_matrices(Kd, pose[:, :, :9].reshape(P, -1, 3, 3), pose[:, :, 9:])
    score_ms = timed(lambda: ap.score_poses(obs, xyz4, offsets, hyp32, ap.ABS_POSE_MAX_ERROR), a.iters)

    def batch():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = ap.estimate_absolute_poses(problems, "cuda", n_hyp=a.samples)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res

    batch()
    runs = [batch() for _ in range(a.batch_iters)]
    res = runs[-1][1]
    n_hyp_scored = P * a.samples * ap.MAX_SOLUTIONS
    out = dict(problems=P, samples=a.samples, points=n, iters=a.iters,
               solver_ms=solver_ms, samples_per_s=P * a.samples / (solver_ms["median"] * 1e-3),
               solutions=int(count.sum().item()), solutions_per_s=float(count.sum().item()) / (solver_ms["median"] * 1e-3),
               score_ms=score_ms, scored_hypotheses=n_hyp_scored, point_tests_per_s=n_hyp_scored * n / (score_ms["median"] * 1e-3),
               batch_s=float(np.median([r[0] for r in runs])), registered=int(sum(r["success"] for r in res)),
               mean_inliers=float(np.mean([r["num_inliers"] for r in res])))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
