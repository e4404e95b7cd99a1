#!/usr/bin/env python3
"""Track triangulation (developer tool, bench.py is the judged entry).  Times vc_triangulate_tracks on
200 000 synthetic tracks: lengths drawn from the histogram of the grown 12-view windowed scene (2: 152, 3: 316, 4: 434,
5: 259 of 1161 tracks) plus a tail of 1 % tracks of 12-60 observations (--tail), 72 cameras on an arc, 0.5 px noise, 10 %
gross outliers.  The front end is timed with and without its sort by length, and the kernel alone on the sorted and on the
shuffled call (device events, 3 warm-up launches, the median over --iters launches); the numpy specification runs 2 000 of
those tracks on the host.  An observation test is one inlier test of the hypothesis stage: a track of n observations with
h hypotheses counts h n of them (an upper bound: a void hypothesis tests nothing).  Prints one JSON line.  Needs a GPU."""
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
from vit_colmap_amd import _lib  # noqa: E402
from vit_colmap_amd.mapping.triangulate import MAX_ERROR, MIN_TRI_ANGLE_TAN2, triangulate_tracks  # noqa: E402

K = np.array([[600.0, 0, 320.0], [0, 600.0, 240.0], [0, 0, 1]])
HISTOGRAM = {2: 152, 3: 316, 4: 434, 5: 259}


def cameras(n=72):
    rows = []
    for a in np.radians(1.2 * np.arange(n) - 40.0):
        c = np.array([8.0 * np.sin(a), 0.2 * np.cos(5 * a), -8.0 * np.cos(a)])
        z = -c / np.linalg.norm(c)
        x = np.cross([0.0, 1.0, 0.0], z)
        x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z])
        rows.append(np.concatenate([R.reshape(9), -R @ c, [K[0, 0], K[1, 1], K[0, 2], K[1, 2]]]))
    return np.stack(rows)


def tracks(n_tracks, seed=1, tail=0.01, noise=0.5, outliers=0.1):
    rs = np.random.RandomState(seed)
    cams = cameras()
    sizes, weights = np.array(list(HISTOGRAM)), np.array(list(HISTOGRAM.values()), np.float64)
    lengths = rs.choice(sizes, n_tracks, p=weights / weights.sum())
    long = rs.uniform(size=n_tracks) < tail
    lengths = np.where(long, rs.randint(12, 61, n_tracks), lengths)
    offsets = np.concatenate([[0], np.cumsum(lengths)])
    total = int(offsets[-1])
    track_of = np.repeat(np.arange(n_tracks), lengths)
    X = np.stack([rs.uniform(-2, 2, n_tracks), rs.uniform(-1.5, 1.5, n_tracks), rs.uniform(-1.5, 1.5, n_tracks)], axis=1)[track_of]
    # distinct views per track: a random start and the following views of the ring
    slots = ((rs.randint(72, size=n_tracks)[track_of] + (np.arange(total) - offsets[:-1][track_of])) % 72).astype(np.int32)
    R, t = cams[slots, :9].reshape(-1, 3, 3), cams[slots, 9:12]
    Xc = np.einsum("nij,nj->ni", R, X) + t
    obs = np.stack([K[0, 0] * Xc[:, 0] / Xc[:, 2] + K[0, 2], K[1, 1] * Xc[:, 1] / Xc[:, 2] + K[1, 2]], axis=1) + rs.normal(0, noise, (total, 2))
    wrong = rs.uniform(size=total) < outliers
    obs = np.where(wrong[:, None], np.stack([rs.uniform(0, 640, total), rs.uniform(0, 480, total)], axis=1), obs)
    seeds = rs.randint(0, 1 << 31, n_tracks).astype(np.int32)
    return obs, slots, offsets.astype(np.int32), cams, seeds


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
    p.add_argument("--tracks", type=int, default=200000)
    p.add_argument("--iters", type=int, default=50)
    p.add_argument("--spec-tracks", dest="spec_tracks", type=int, default=2000)
    p.add_argument("--tail", type=float, default=0.01, help="fraction of tracks of 12-60 observations (0: the histogram alone)")
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_triangulate needs a GPU: nothing is measured without one")
    obs, slots, offsets, cams, seeds = tracks(a.tracks, tail=a.tail)
    lengths = np.diff(offsets).astype(np.int64)
    hyps = np.where(lengths * (lengths - 1) // 2 <= 64, lengths * (lengths - 1) // 2, 64)
    tests = int((hyps * lengths).sum())
    d = [torch.from_numpy(x).cuda() for x in (obs, slots, offsets, cams, seeds)]
    lib = _lib.load()

    def kernel_only(args):
        T, total = len(args[4]), len(args[1])
        out = (torch.empty((T, 3), dtype=torch.float64, device="cuda"), torch.empty((total,), dtype=torch.uint8, device="cuda"),
               torch.empty((T,), dtype=torch.int32, device="cuda"), torch.empty((T,), dtype=torch.float64, device="cuda"))

        def fn():
            _lib.check(lib.vc_triangulate_tracks(*[_lib.ptr(t) for t in args[:3]], T, _lib.ptr(args[3]), int(args[3].shape[0]),
                                                 _lib.ptr(args[4]), MAX_ERROR, MIN_TRI_ANGLE_TAN2, *[_lib.ptr(t) for t in out],
                                                 _lib.stream_ptr()), "vc_triangulate_tracks")
        return fn

    # the sorted call, built once the way the front end builds it
    order = np.argsort(-lengths, kind="stable")
    new_off = np.concatenate([[0], np.cumsum(lengths[order])])
    src = np.repeat(offsets[:-1][order] - new_off[:-1], lengths[order]) + np.arange(len(slots))
    s = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (obs[src], slots[src], new_off.astype(np.int32), cams, seeds[order])]

    res = dict(tracks=a.tracks, tail=a.tail, observations=int(offsets[-1]), observation_tests=tests, iters=a.iters,
               mean_length=float(lengths.mean()), longest=int(lengths.max()))
    for name, fn in (("kernel_sorted", kernel_only(s)), ("kernel_unsorted", kernel_only(d)),
                     ("front_end_sorted", lambda: triangulate_tracks(*d, sort_by_length=True)), ("front_end_unsorted", lambda: triangulate_tracks(*d))):
        ms = timed(fn, a.iters)
        res[name] = dict(ms=ms, tracks_per_s=a.tracks / (ms["median"] * 1e-3), observation_tests_per_s=tests / (ms["median"] * 1e-3))
    xyz, mask, count, error = triangulate_tracks(*d)
    res["accepted"] = int((count > 0).sum().item())

    import util_mapper as um  # noqa: E402

    n = min(a.spec_tracks, a.tracks)
    hi = int(offsets[n])
    t0 = time.perf_counter()
    spec = um.triangulate_tracks(obs[:hi], slots[:hi], offsets[:n + 1], cams, seeds[:n])
    dt = time.perf_counter() - t0
    res["spec"] = dict(tracks=n, seconds=dt, tracks_per_s=n / dt, observation_tests_per_s=int((hyps[:n] * lengths[:n]).sum()) / dt,
                       counts_equal=bool(np.array_equal(spec[2], count[:n].cpu().numpy())))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
