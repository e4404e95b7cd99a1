#!/usr/bin/env python3
"""Retrieval matching (developer tool, bench.py is the judged entry).  Times
  * vc_pool_descriptors_u8 on c5's descriptor block (500 x 2048 x 256, every row counted) and reports GB/s against the
    one read of the block,
  * vc_retrieval_topk_i8 (search + merge) at (n, D, k) = (500, 256, 20) and (16384, 256, 20), random int8 rows,
  * match_retrieval against match_exhaustive, database to database, on the trajectory input of tests/util_retrieval.py
    scaled to 200 images (w = 256, stride = 64, D = 128, max_distance 1.25 so that the rows do match), the two
    alternating inside every repetition.
Kernel times are device events around one call, warm-up launches excluded.  Prints one JSON line.  Needs a GPU."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import util_retrieval as ur  # noqa: E402
from vit_colmap_amd import _lib  # noqa: E402
from vit_colmap_amd.matching import match_exhaustive, match_retrieval  # noqa: E402
from vit_colmap_amd.utils.config import MatchingConfig  # noqa: E402


def timed(fn, iters, warmup=3):
    for _ in range(warmup):
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


def bench_pool(lib, n, n_max, D, iters):
    desc = torch.randint(0, 256, (n, n_max, D), dtype=torch.uint8, device="cuda")
    counts = torch.full((n,), n_max, dtype=torch.int32, device="cuda")
    sums = torch.empty((n, D), dtype=torch.int32, device="cuda")

    def call():
        _lib.check(lib.vc_pool_descriptors_u8(_lib.ptr(desc), _lib.ptr(counts), n, n_max, D, _lib.ptr(sums), _lib.stream_ptr()),
                   "vc_pool_descriptors_u8")

    ms = timed(call, iters)
    assert torch.equal(sums, desc.to(torch.int32).sum(dim=1, dtype=torch.int32))
    nbytes = n * n_max * D
    return dict(shape=[n, n_max, D], bytes=nbytes, ms=ms, gb_per_s=nbytes / (ms["median"] * 1e-3) / 1e9)


def bench_topk(lib, n, D, k, iters):
    q = torch.randint(-127, 128, (n, D), dtype=torch.int8, device="cuda")
    valid = torch.ones(n, dtype=torch.int32, device="cuda")
    idx = torch.empty((n, k), dtype=torch.int32, device="cuda")
    score = torch.empty((n, k), dtype=torch.int32, device="cuda")
    nbytes = lib.vc_retrieval_workspace_bytes(n, D, k)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")

    def call():
        _lib.check(lib.vc_retrieval_topk_i8(_lib.ptr(q), _lib.ptr(valid), n, D, k, _lib.ptr(idx), _lib.ptr(score), _lib.ptr(ws),
                                            nbytes, _lib.stream_ptr()), "vc_retrieval_topk_i8")

    ms = timed(call, iters)
    return dict(n=n, D=D, k=k, workspace_bytes=int(nbytes), ms=ms, tera_ops_per_s=2.0 * n * n * D / (ms["median"] * 1e-3) / 1e12)


def bench_e2e(n_images, k, reps):
    opts = MatchingConfig(max_distance=1.25).to_matching_options()
    block, counts = ur.trajectory(seed=7, n=n_images, w=256, stride=64, D=128)
    small = ur.trajectory(seed=7, n=24, w=256, stride=64, D=128)
    out = dict(images=n_images, num_neighbors=k, retrieval=[], exhaustive=[])
    with tempfile.TemporaryDirectory() as tmp:
        for name in ("warm_r.db", "warm_e.db"):                           # first-use costs of every kernel, outside the timing
            ur.make_feature_db(os.path.join(tmp, name), *small)
        match_retrieval(database_path=os.path.join(tmp, "warm_r.db"), matching_options=opts, num_neighbors=4)
        match_exhaustive(database_path=os.path.join(tmp, "warm_e.db"), matching_options=opts)
        for r in range(reps):
            for kind in ("retrieval", "exhaustive"):
                path = os.path.join(tmp, f"{kind}_{r}.db")
                ur.make_feature_db(path, block, counts)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                s = match_retrieval(database_path=path, matching_options=opts, num_neighbors=k) if kind == "retrieval" else \
                    match_exhaustive(database_path=path, matching_options=opts)
                torch.cuda.synchronize()
                s["wall_s"] = time.perf_counter() - t0
                out[kind].append({key: s[key] for key in ("wall_s", "pairs", "matches", "verified_pairs", "gpu_s", "db_s") +
                                  (("retrieval_s", "candidate_pairs") if kind == "retrieval" else ())})
    t_r, t_e = (float(np.median([s["wall_s"] for s in out[kind]])) for kind in ("retrieval", "exhaustive"))
    near = sum(1 for i in range(n_images) for j in range(i + 1, n_images) if j - i <= 3)   # pairs that share pool rows
    out.update(retrieval_s=t_r, exhaustive_s=t_e, exhaustive_over_retrieval=t_e / t_r, pairs_sharing_rows=near,
               verified_kept=out["retrieval"][0]["verified_pairs"] / max(out["exhaustive"][0]["verified_pairs"], 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--large-iters", dest="large_iters", type=int, default=5)
    ap.add_argument("--e2e-images", dest="e2e_images", type=int, default=200)
    ap.add_argument("--e2e-reps", dest="e2e_reps", type=int, default=2)
    ap.add_argument("--num-neighbors", dest="num_neighbors", type=int, default=20)
    ap.add_argument("--skip-e2e", dest="skip_e2e", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_retrieval needs a GPU: nothing is measured without one")
    lib = _lib.load()
    out = dict(pool=bench_pool(lib, 500, 2048, 256, a.iters),
               topk=[bench_topk(lib, 500, 256, 20, a.iters), bench_topk(lib, 16384, 256, 20, a.large_iters)])
    if not a.skip_e2e:
        out["e2e"] = bench_e2e(a.e2e_images, a.num_neighbors, a.e2e_reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
