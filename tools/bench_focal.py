#!/usr/bin/env python3
"""Focal length from the verified pairs (developer tool, bench.py is the judged entry).  Times one launch of
vc_focal_cost at the pair count of c5 (--images 500: 124 750 pairs, every one UNCALIBRATED under one camera) on generated
rank-2 F (a random rotation of 2-40 degrees and a random baseline under K = (600, 600, 320, 240), stored 1.3 times off) with
the 65 candidates of level 0: device events, 3 warm-up launches, the median over --iters launches.  An estimate is four such
launches.  Measurement only: nothing here is gated.  Prints one JSON line.  Needs a GPU."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vit_colmap_amd.matching.focal import estimate_camera, focal_cost, level0  # noqa: E402


def generated_f(n, rs):
    """n rank-2 fundamental matrices at unit norm, float64 (n, 9), vectorised."""
    axis = rs.normal(size=(n, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    ang = np.radians(rs.uniform(2, 40, n))
    S = np.zeros((n, 3, 3))
    S[:, 0, 1], S[:, 0, 2], S[:, 1, 0], S[:, 1, 2], S[:, 2, 0], S[:, 2, 1] = -axis[:, 2], axis[:, 1], axis[:, 2], -axis[:, 0], -axis[:, 1], axis[:, 0]
    R = np.eye(3) + np.sin(ang)[:, None, None] * S + (1 - np.cos(ang))[:, None, None] * (S @ S)
    t = rs.normal(size=(n, 3))
    T = np.zeros((n, 3, 3))
    T[:, 0, 1], T[:, 0, 2], T[:, 1, 0], T[:, 1, 2], T[:, 2, 0], T[:, 2, 1] = -t[:, 2], t[:, 1], t[:, 2], -t[:, 0], -t[:, 1], t[:, 0]
    Ki = np.linalg.inv(np.array([[600.0, 0, 320], [0, 600.0, 240], [0, 0, 1]]))
    F = Ki.T @ (T @ R) @ Ki
    return (F / np.linalg.norm(F.reshape(n, 9), axis=1)[:, None, None]).reshape(n, 9)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--images", type=int, default=500)
    p.add_argument("--iters", type=int, default=50)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_focal needs a GPU: nothing is measured without one")
    rs = np.random.RandomState(1)
    n = a.images * (a.images - 1) // 2
    F, w = generated_f(n, rs), rs.randint(15, 401, n).astype(np.float64)
    cam = np.array([780.0, 780.0, 320.0, 240.0])
    d = [torch.from_numpy(x).cuda() for x in (F, np.zeros(n, np.int32), w, cam[None], level0())]
    for _ in range(3):
        cost, weight = focal_cost(*d)
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        focal_cost(*d)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    med = float(np.median(ms))
    e = estimate_camera(F, w, cam)
    print(json.dumps(dict(images=a.images, pairs=n, candidates=65, iters=a.iters, ms=dict(median=med, min=float(np.min(ms)), max=float(np.max(ms))),
                          pair_candidates_per_s=65 * n / (med * 1e-3), gb_per_s=88 * n / (med * 1e-3) / 1e9,
                          estimate=dict(ratio=e["ratio"], true_ratio=1 / 1.3, cost_min=e["cost_min"], cost_median=e["cost_median"]))))


if __name__ == "__main__":
    main()
