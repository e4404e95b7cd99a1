#!/usr/bin/env python3
"""The calibrated branch of verification (developer tool, bench.py is the judged entry).  Times
vc_essential_5pt on 1024 pairs x 128 hypotheses (device events, warm-up launches excluded) and verify_pairs on the same
scenes with and without focal-length priors, the two alternating inside every repetition.  Prints one JSON line:
hypotheses/s of the solver, and the ratio of calibrated to uncalibrated verification time.  Needs a GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.two_view_oracle import synthetic_two_view  # noqa: E402
from vit_colmap_amd.matching import essential, two_view  # noqa: E402

K = np.array([[600.0, 0, 320.0], [0, 600.0, 240.0], [0, 0, 1]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1024)
    ap.add_argument("--hypotheses", type=int, default=essential.NUM_HYP_E)
    ap.add_argument("--points", type=int, default=300)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--verify-iters", dest="verify_iters", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_essential needs a GPU: nothing is measured without one")
    P = a.pairs
    kps, pair_images, pids, lists = {}, [], [], []
    for q in range(P):                                   # 16 distinct scenes (every fourth planar), each under many pair ids
        kp1, kp2, m, _ = synthetic_two_view(1 + q % 16, a.points, 0.3 if q % 2 else 0.5, planar=q % 4 == 3)
        kps[2 * q], kps[2 * q + 1] = kp1, kp2
        pair_images.append((2 * q, 2 * q + 1))
        pids.append((2 * q + 1) * 2147483647 + 2 * q + 2)
        lists.append(m)
    cameras = (np.tile(K, (2 * P, 1, 1)), np.ones(2 * P, np.uint8))

    # ---- the solver alone -------------------------------------------------------------------------------------------------
    pts = np.concatenate([np.concatenate([kps[a_][m[:, 0]], kps[b_][m[:, 1]]], axis=1) for (a_, b_), m in zip(pair_images, lists)])
    offsets = torch.tensor(np.arange(P + 1) * a.points, dtype=torch.int32, device="cuda")
    pair_of = torch.repeat_interleave(torch.arange(P, device="cuda"), a.points)
    Ki = torch.from_numpy(np.tile(np.linalg.inv(K), (P, 1, 1))).cuda()
    xn = essential.normalise_points(torch.from_numpy(pts).cuda().to(torch.float64), pair_of, Ki, Ki)
    seeds = torch.tensor([p & 0xFFFFFFFF for p in pids], dtype=torch.int64, device="cuda")
    counts = torch.full((P,), a.points, dtype=torch.int64, device="cuda")
    samples = two_view._sample_indices(seeds, counts, a.hypotheses, 5, two_view.SALT["E"]).to(torch.int32).contiguous()
    for _ in range(3):
        E, n = essential.solve_five_point(xn, offsets, samples)
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        E, n = essential.solve_five_point(xn, offsets, samples)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    med = float(np.median(ms))
    out = dict(pairs=P, hypotheses=a.hypotheses, points=a.points, iters=a.iters,
               solver_ms=dict(median=med, min=float(np.min(ms)), max=float(np.max(ms))),
               hypotheses_per_s=P * a.hypotheses / (med * 1e-3), solutions_per_hypothesis=float(n.float().mean().item()))

    # ---- verify_pairs with and without the priors ----------------------------------------------------------------------------
    def run(cams):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = two_view.verify_pairs(kps, pair_images, pids, lists, cameras=cams)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res

    run(None), run(cameras)                              # warm-up of every shape
    t_plain, t_cal = [], []
    for _ in range(a.verify_iters):
        t_plain.append(run(None)[0])
        dt, res = run(cameras)
        t_cal.append(dt)
    out["verify_uncalibrated_s"] = float(np.median(t_plain))
    out["verify_calibrated_s"] = float(np.median(t_cal))
    out["calibrated_over_uncalibrated"] = out["verify_calibrated_s"] / out["verify_uncalibrated_s"]
    out["configs"] = {str(c): int(sum(r["config"] == c for r in res)) for c in sorted({r["config"] for r in res})}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
