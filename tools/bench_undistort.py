#!/usr/bin/env python3
"""Keypoint undistortion (developer tool, bench.py is the judged entry).  Times vc_undistort_points on
--images x --keypoints uniform random pixels of a 640 x 480 image under one camera per image (|k1| <= 0.2, |k2| <= 0.05,
|p| <= 2e-3): the front end (its one-flag slot check and wait included) by device events, 3 warm-up launches, the median over
--iters launches, next to the numpy specification on the same call.  The kernel is bandwidth-trivial (28 bytes per keypoint, once
per image): the figure is here to say so, not to be tuned.  Prints one JSON line.  Needs a GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from vit_colmap_amd.matching.undistort import undistort_points  # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--images", type=int, default=50)
    p.add_argument("--keypoints", type=int, default=2048)
    p.add_argument("--iters", type=int, default=50)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_undistort needs a GPU: nothing is measured without one")
    import util_undistort as uu  # noqa: E402

    rs = np.random.RandomState(1)
    n = a.images * a.keypoints
    xy = np.stack([rs.uniform(0, uu.WIDTH, n), rs.uniform(0, uu.HEIGHT, n)], axis=1).astype(np.float32)
    cam = np.repeat(np.arange(a.images, dtype=np.int32), a.keypoints)
    cams = np.stack([uu.random_camera(i) for i in range(a.images)])
    d = [torch.from_numpy(x).cuda() for x in (xy, cam, cams)]
    for _ in range(3):
        out, valid = undistort_points(*d)
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        undistort_points(*d)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    t0 = time.perf_counter()
    want, want_valid = uu.undistort(xy, cam, cams)
    dt = time.perf_counter() - t0
    med = float(np.median(ms))
    print(json.dumps(dict(images=a.images, keypoints=n, iters=a.iters, ms=dict(median=med, min=float(np.min(ms)), max=float(np.max(ms))),
                          keypoints_per_s=n / (med * 1e-3), gb_per_s=28 * n / (med * 1e-3) / 1e9, valid=int(valid.sum().item()),
                          spec=dict(seconds=dt, keypoints_per_s=n / dt,
                                    bits_equal=bool(np.array_equal(want_valid, valid.cpu().numpy())
                                                    and np.array_equal(want, out.cpu().numpy(), equal_nan=True))))))


if __name__ == "__main__":
    main()
