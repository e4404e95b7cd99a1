#!/usr/bin/env python3
"""Developer tool: the device detectors of the hybrid extractor against the work they sit in front of.

  python tools/bench_detect.py            one JSON line per measurement, on 16 frames of 640x480 (checkerboard + noise):
      detect/<sift|fast|gftt>   the detector alone, with bytes-over-time against HBM bandwidth for FAST and GFTT
      vitb+describe_at          the ViT-B/14 forward and `describe_at` of the same batch (2048 points per image)
      e2e                       the per-image path with precomputed keypoints (`keypoint_fn`, detection free: the only
                                hybrid path before the device detectors) against the batched `_run_batch` with FAST
  python tools/bench_detect.py --kernels  the same, then a `rocprofv3 --kernel-trace --stats` run of the detectors in a
                                          child process, summarised per kernel
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
H, W, N = 480, 640, 16
HBM_BYTES_PER_S = 8.0e12          # MI355X peak HBM3E bandwidth


def frames_np(n=N, seed=0, amp=40):
    """Checkerboard shifted per frame + uniform noise (the synthetic frames of the GPU tests)."""
    import numpy as np

    out = []
    for k in range(n):
        rs = np.random.RandomState(seed + k)
        yy, xx = np.mgrid[0:H, 0:W]
        img = ((((xx + 7 * k) // 40 + (yy + 5 * k) // 40) % 2 == 0) * 255).astype(np.int16)[..., None].repeat(3, 2)
        img = img + rs.randint(-amp, amp + 1, img.shape).astype(np.int16)
        out.append(np.clip(img, 0, 255).astype(np.uint8))
    return out


def timed(fn, iters, warmup):
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def detectors(x):
    from vit_colmap_amd.features import hip_detect, sift_extractor

    return {"sift": lambda: sift_extractor.detect_device(x, 2048), "fast": lambda: hip_detect.fast(x, 2048),
            "gftt": lambda: hip_detect.gftt(x, 2048)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--detect-only", action="store_true", help="(used by --kernels) skip the ViT measurements")
    args = ap.parse_args()
    import numpy as np
    import torch

    assert torch.cuda.is_available(), "bench_detect needs a GPU"
    from vit_colmap_amd.features import hip_select
    from vit_colmap_amd.features.hybrid_extractor import HybridViTExtractor

    imgs = frames_np()
    x = torch.from_numpy(np.stack(imgs)).cuda()
    px = N * H * W
    # bytes each detector has to move at least (FAST: the BGR frames once) and what its kernels do move
    moved = {"fast": dict(least=3 * px, actual=(3 + 1 + 1) * px), "gftt": dict(least=3 * px, actual=(3 + 4 + 4 + 4) * px)}
    for name, fn in detectors(x).items():
        dt = timed(fn, args.iters, args.warmup)
        row = dict(what=f"detect/{name}", images=N, ms=round(dt * 1e3, 3), us_per_image=round(dt * 1e6 / N, 1))
        if name in moved:
            row.update(least_bytes=moved[name]["least"], moved_bytes=moved[name]["actual"],
                       moved_GBps=round(moved[name]["actual"] / dt / 1e9, 1),
                       hbm_floor_us=round(moved[name]["least"] / HBM_BYTES_PER_S * 1e6, 2),
                       share_of_hbm_peak=round(moved[name]["least"] / HBM_BYTES_PER_S / dt, 4))
        print(json.dumps(row), flush=True)
    if args.detect_only:
        return
    rs = np.random.RandomState(1)
    pts = [np.stack([rs.uniform(0, W, 2048), rs.uniform(0, H, 2048)], 1).astype(np.float32) for _ in range(N)]
    proj = rs.randn(768, 256).astype(np.float32) / np.sqrt(768)
    ex = HybridViTExtractor(num_keypoints=2048, descriptor_dim=256, detector_type="fast", projection=proj)
    kp = torch.from_numpy(np.stack(pts)).cuda()
    cnt = torch.full((N,), 2048, dtype=torch.int32, device="cuda")
    with torch.inference_mode():
        dt_vit = timed(lambda: ex._describe_device(x, kp, cnt), args.iters, args.warmup)
    print(json.dumps(dict(what="vitb+describe_at", images=N, ms=round(dt_vit * 1e3, 3))), flush=True)
    by_id = {id(im): p for im, p in zip(imgs, pts)}
    old = HybridViTExtractor(num_keypoints=2048, descriptor_dim=256, keypoint_fn=lambda im: by_id[id(im)], projection=proj)
    dt_old = timed(lambda: [old._run_inference(im) for im in imgs], max(args.iters // 4, 3), 1)
    dt_new = timed(lambda: ex._run_batch(imgs), max(args.iters // 4, 3), 1)
    print(json.dumps(dict(what="e2e", images=N, per_image_keypoint_fn_ms=round(dt_old * 1e3, 2),
                          batched_fast_ms=round(dt_new * 1e3, 2), ratio_old_over_new=round(dt_old / dt_new, 3))), flush=True)
    if args.kernels:
        out = tempfile.mkdtemp(prefix="bench_detect_")
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable,
               os.path.abspath(__file__), "--detect-only", "--iters", str(args.iters), "--warmup", "1"]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL)
        f = sorted(glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True))[0]
        rows = [r for r in csv.DictReader(open(f))]
        print(f"{'kernel':44s} {'calls':>7s} {'total ms':>10s} {'avg us':>10s}")
        for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"]))[:24]:
            print(f"{r['Name'][:44]:44s} {int(r['Calls']):7d} {float(r['TotalDurationNs']) / 1e6:10.3f} "
                  f"{float(r['AverageNs']) / 1e3:10.2f}")


if __name__ == "__main__":
    main()
