#!/usr/bin/env python3
"""Two-view relative pose (developer tool, bench.py is the judged entry).  Times vc_two_view_pose on the
inliers of 1024 pairs x 300 matches (16 distinct scenes; device events, warm-up launches excluded) and verify_pairs with
priors on every camera, `relative_pose` off against on, the two alternating inside every repetition: the option-off run is
the behaviour before the option existed and is the baseline.  Prints one JSON line.  Needs a GPU."""
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
from vit_colmap_amd.matching import pose, two_view  # noqa: E402

K = np.array([[600.0, 0, 320.0], [0, 600.0, 240.0], [0, 0, 1]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1024)
    ap.add_argument("--points", type=int, default=300)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--verify-iters", dest="verify_iters", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pose needs a GPU: nothing is measured without one")
    P = a.pairs
    kps, pair_images, pids, lists = {}, [], [], []
    for q in range(P):                                   # 16 distinct scenes (every fourth planar), each under many pair ids
        kp1, kp2, m, _ = synthetic_two_view(1 + q % 16, a.points, 0.3 if q % 2 else 0.5, planar=q % 4 == 3)
        kps[2 * q], kps[2 * q + 1] = kp1, kp2
        pair_images.append((2 * q, 2 * q + 1))
        pids.append((2 * q + 1) * 2147483647 + 2 * q + 2)
        lists.append(m)
    cameras = (np.tile(K, (2 * P, 1, 1)), np.ones(2 * P, np.uint8))

    def run(on):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = two_view.verify_pairs(kps, pair_images, pids, lists, cameras=cameras, relative_pose=on)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res

    run(False), run(True)                                # warm-up of every shape
    t_off, t_on = [], []
    for _ in range(a.verify_iters):
        t_off.append(run(False)[0])
        dt, res = run(True)
        t_on.append(dt)

    # ---- the kernel alone, on the inliers and candidates of that run ----------------------------------------------------------
    Ki = np.linalg.inv(K)
    posed = [(q, r) for q, r in enumerate(res) if "tri_angle" in r]
    xn, offs = [], [0]
    d_cand = torch.full((len(posed), 4, 12), float("nan"), dtype=torch.float64, device="cuda")
    for n, (q, r) in enumerate(posed):
        (i, j), inl = pair_images[q], r["inlier_matches"].astype(np.int64)
        p = np.concatenate([kps[i][inl[:, 0]], kps[j][inl[:, 1]]], axis=1).astype(np.float64)
        xn.append(p * [Ki[0, 0], Ki[1, 1], Ki[0, 0], Ki[1, 1]] + [Ki[0, 2], Ki[1, 2], Ki[0, 2], Ki[1, 2]])
        offs.append(offs[-1] + len(inl))
        if r["config"] in (two_view.CONFIG_PLANAR, two_view.CONFIG_PANORAMIC):
            d_cand[n] = pose.h_candidates(torch.from_numpy(Ki @ r["H"] @ K)[None].cuda())[0]
        else:
            E = r["E"] if "E" in r else K.T @ np.asarray(r["model9"], np.float64).reshape(3, 3) @ K
            d_cand[n] = pose.e_candidates(pose.project_to_essential(torch.from_numpy(E)[None].cuda()))[0]
    d_xn = torch.from_numpy(np.concatenate(xn)).cuda()
    d_off = torch.tensor(offs, dtype=torch.int32, device="cuda")
    for _ in range(3):
        pose.two_view_pose(d_xn, d_off, d_cand)
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        pose.two_view_pose(d_xn, d_off, d_cand)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    med = float(np.median(ms))
    out = dict(pairs=P, points=a.points, iters=a.iters, posed_pairs=len(posed), inliers=int(offs[-1]),
               kernel_ms=dict(median=med, min=float(np.min(ms)), max=float(np.max(ms))),
               triangulations_per_s=4 * offs[-1] / (med * 1e-3),
               verify_option_off_s=float(np.median(t_off)), verify_option_on_s=float(np.median(t_on)))
    out["on_over_off"] = out["verify_option_on_s"] / out["verify_option_off_s"]
    out["configs"] = {str(c): int(sum(r["config"] == c for r in res)) for c in sorted({r["config"] for r in res})}
    out["median_tri_angle_deg"] = float(np.degrees(np.median([r["tri_angle"] for _, r in posed]))) if posed else 0.0
    print(json.dumps(out))


if __name__ == "__main__":
    main()
