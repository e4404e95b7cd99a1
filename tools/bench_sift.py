#!/usr/bin/env python3
"""Developer tool: throughput of the HIP SIFT extractor (features/sift_extractor.extract_device, COLMAP default options)
at 640x480 and 1600x1200, device-resident uint8 frames, and its per-stage split.

  python tools/bench_sift.py                      images/s at both sizes (one JSON line per size)
  python tools/bench_sift.py --stages             the same, then a `rocprofv3 --kernel-trace --stats` run of it in a child
                                                  process, summarised per kernel (stage)
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
SIZES = {"640x480": (480, 640, 16), "1600x1200": (1200, 1600, 4)}   # h, w, images per call


def frames(h, w, n, seed=0):
    import numpy as np
    import torch

    rs = np.random.RandomState(seed)
    small = rs.randint(0, 256, (n, h // 8 + 1, w // 8 + 1, 3)).astype(np.float32)
    t = torch.from_numpy(small).permute(0, 3, 1, 2)
    t = torch.nn.functional.interpolate(t, size=(h, w), mode="bicubic", align_corners=False)   # smooth texture
    return t.clamp(0, 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous().cuda()


def measure(name, iters, warmup):
    import torch

    from vit_colmap_amd.features import sift_extractor as se

    h, w, n = SIZES[name]
    x = frames(h, w, n)
    for _ in range(warmup):
        res = se.extract_device(x)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        res = se.extract_device(x)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / iters
    return dict(size=name, images_per_call=n, ms_per_call=round(dt * 1e3, 3), images_per_s=round(n / dt, 1),
                mean_keypoints=round(float(res["count"].float().mean()), 1))


def stages(iters):
    out = tempfile.mkdtemp(prefix="bench_sift_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--",
           sys.executable, os.path.abspath(__file__), "--iters", str(iters), "--warmup", "1"]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL)
    f = sorted(glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True))[0]
    rows = [r for r in csv.DictReader(open(f))]
    tot = sum(float(r["TotalDurationNs"]) for r in rows)
    print(f"{'kernel':40s} {'calls':>7s} {'total ms':>10s} {'avg us':>10s} {'%':>6s}")
    for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
        name = r["Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        if "_GLOBAL__N_1" in name:                     # mangled: _ZN12_GLOBAL__N_1<len><name>E...
            rest = name.split("_GLOBAL__N_1", 1)[1]
            digits = len(rest) - len(rest.lstrip("0123456789"))
            name = rest[digits:digits + int(rest[:digits])]
        print(f"{name[:40]:40s} {int(r['Calls']):7d} {float(r['TotalDurationNs']) / 1e6:10.3f} "
              f"{float(r['AverageNs']) / 1e3:10.2f} {float(r['TotalDurationNs']) / tot * 100:6.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--stages", action="store_true")
    a = ap.parse_args()
    for name in SIZES:
        print(json.dumps(measure(name, a.iters, a.warmup)), flush=True)
    if a.stages:
        stages(max(2, a.iters // 4))


if __name__ == "__main__":
    main()
