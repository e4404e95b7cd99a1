#!/usr/bin/env python3
"""Track splitting (developer tool, bench.py is the judged entry).  Times one launch of vc_split_tracks on two
calls: the largest one the growth makes on the 12-view windowed scene with 10 % of its consecutive matches swapped (the
specification's growth on the host supplies it: 85 of the scene's 112 inconsistent components, max_points 4), and --comps generated merged
components (tests/util_split.py, 15 % random pixels, all nodes free), next to vc_triangulate_tracks on the same arrays read
as tracks: the same node count, one point per component instead of up to four.  Device events, 3 warm-up launches, the
median over --iters launches; the labels and points are restored before every launch, outside the timed region.  Prints
one JSON line.  Needs a GPU."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from vit_colmap_amd import _lib  # noqa: E402
from vit_colmap_amd.mapping.triangulate import MAX_ERROR, MIN_TRI_ANGLE_TAN2, SPLIT_MAX_POINTS  # noqa: E402


def growth_call():
    """The arguments of the largest vc_split_tracks call of the swapped scene's growth."""
    import util_mapper as um
    import util_split as us
    from test_absolute_pose_spec import scene_images, truth_pairs

    calls = []

    def capture(obs, cam, offsets, cams, seeds, max_points, label, pts):
        calls.append((obs, cam, offsets, cams, seeds, label.copy(), pts.copy()))
        return us.split_tracks(obs, cam, offsets, cams, seeds, max_points, label, pts)

    scene = um.windowed_scene()
    us.grow_model(scene_images(scene), us.swapped_pairs(truth_pairs(scene), 0.1), split=capture)
    return max(calls, key=lambda c: len(c[4]))


def generated_call(n):
    import util_split as us

    return us.as_one_call([us.merged_component(i, outliers=0.15) for i in range(n)], SPLIT_MAX_POINTS)


def time_call(lib, call, iters):
    obs, cam, offsets, cams, seeds, label, pts = call
    C, total = len(offsets) - 1, len(cam)
    d = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in
         (np.asarray(obs, np.float64), np.asarray(cam, np.int32), np.asarray(offsets, np.int32), np.asarray(cams, np.float64),
          np.asarray(seeds, np.int64).astype(np.uint32).view(np.int32))]
    label0, pts0 = torch.from_numpy(np.asarray(label, np.int32)).cuda(), torch.from_numpy(np.asarray(pts, np.float64)).cuda()
    work = [label0.clone(), pts0.clone(), torch.empty((C, SPLIT_MAX_POINTS), dtype=torch.int32, device="cuda"),
            torch.empty((C, SPLIT_MAX_POINTS), dtype=torch.uint8, device="cuda"),
            torch.empty((C, SPLIT_MAX_POINTS), dtype=torch.float64, device="cuda")]
    tri = [torch.empty((C, 3), dtype=torch.float64, device="cuda"), torch.empty((total,), dtype=torch.uint8, device="cuda"),
           torch.empty((C,), dtype=torch.int32, device="cuda"), torch.empty((C,), dtype=torch.float64, device="cuda")]

    def split():
        _lib.check(lib.vc_split_tracks(*[_lib.ptr(t) for t in d[:3]], C, _lib.ptr(d[3]), int(d[3].shape[0]), _lib.ptr(d[4]), SPLIT_MAX_POINTS,
                                       MAX_ERROR, MIN_TRI_ANGLE_TAN2, *[_lib.ptr(t) for t in work], _lib.stream_ptr()), "vc_split_tracks")

    def triangulate():
        _lib.check(lib.vc_triangulate_tracks(*[_lib.ptr(t) for t in d[:3]], C, _lib.ptr(d[3]), int(d[3].shape[0]), _lib.ptr(d[4]), MAX_ERROR,
                                             MIN_TRI_ANGLE_TAN2, *[_lib.ptr(t) for t in tri], _lib.stream_ptr()), "vc_triangulate_tracks")

    res = dict(components=C, nodes=total)
    for name, fn in (("vc_split_tracks", split), ("vc_triangulate_tracks", triangulate)):
        ms = []
        for it in range(3 + iters):
            work[0].copy_(label0), work[1].copy_(pts0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if it >= 3:
                ms.append(e0.elapsed_time(e1))
        res[name] = dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)))
    res["points_created"] = int(work[3].sum().item())
    res["points_triangulated"] = int((tri[2] > 0).sum().item())
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--comps", type=int, default=4096)
    p.add_argument("--iters", type=int, default=50)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_split needs a GPU: nothing is measured without one")
    lib = _lib.load()
    print(json.dumps(dict(iters=a.iters, growth=time_call(lib, growth_call(), a.iters), generated=time_call(lib, generated_call(a.comps), a.iters))))


if __name__ == "__main__":
    main()
