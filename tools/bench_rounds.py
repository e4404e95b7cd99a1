#!/usr/bin/env python3
"""Adjustment per growth round (developer tool, bench.py is the judged entry; measurement only, no
threshold).  On the 24-view windowed scene (2400 points, 1 px noise, the rows an ideal verifier would write) it times
build_mapped_model against build_sparse_model followed by build_adjusted_model, wall clock with a device synchronisation
on either side, the median over --iters runs after one warm-up run, and splits the mapped model's time into its A-steps (the
bundle adjustments of the rounds), its E-steps (the vc_refine_tracks launches with their uploads and downloads), the tail
(build_adjusted_model on the mapped rounds) and the rest, which is the growth itself.  Prints one JSON line.  Needs a GPU."""
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
import util_absolute_pose as ua  # noqa: E402
import util_mapper as um  # noqa: E402
from test_absolute_pose_spec import truth_pairs, write_scene_db  # noqa: E402
from vit_colmap_amd.mapping import rounds  # noqa: E402
from vit_colmap_amd.mapping.bundle import build_adjusted_model, bundle_adjust  # noqa: E402
from vit_colmap_amd.mapping.grow import build_sparse_model  # noqa: E402


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def drift(model, scene):
    poses = {i: (ua.quat_to_rot(im["qvec"]), im["tvec"]) for i, im in model.images.items()}
    rot, pos = ua.align_errors(poses, scene, *model.initial_pair)
    return dict(rotation_deg=rot, centre_baselines=pos)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--views", type=int, default=24)
    p.add_argument("--points", type=int, default=2400)
    p.add_argument("--noise", type=float, default=1.0)
    p.add_argument("--iters", type=int, default=3)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rounds needs a GPU: nothing is measured without one")
    scene = um.windowed_scene(n_views=a.views, n_points=a.points, noise=a.noise)
    with tempfile.TemporaryDirectory() as tmp:
        db = os.path.join(tmp, "scene.db")
        write_scene_db(db, scene, pairs=truth_pairs(scene))
        spent = dict(a_step=0.0, e_step=0.0, tail=0.0)

        def timed_bundle(*args, **kw):
            out, ms = wall(lambda: bundle_adjust(*args, **kw))
            spent["a_step"] += ms
            return out

        def timed_refine(*args):
            out, ms = wall(lambda: rounds._gpu_refine(*args))
            spent["e_step"] += ms
            return out

        def once():
            grown, t_grow = wall(lambda: build_sparse_model(db))
            adjusted, t_adjust = wall(lambda: build_adjusted_model(db, grown=grown))
            return adjusted, dict(grow_ms=t_grow, adjust_ms=t_adjust, total_ms=t_grow + t_adjust)

        def per_round():
            for k in spent:
                spent[k] = 0.0
            (model, reports), t_rounds = wall(lambda: rounds.build_mapped_rounds(db, bundle_fn=timed_bundle, refine_fn=timed_refine))
            mapped, t_tail = wall(lambda: build_adjusted_model(db, grown=model))
            mapped.round_adjustments = reports
            total = t_rounds + t_tail
            return mapped, dict(total_ms=total, a_step_ms=spent["a_step"], e_step_ms=spent["e_step"], tail_ms=t_tail,
                                growth_ms=t_rounds - spent["a_step"] - spent["e_step"], a_step_share=spent["a_step"] / total,
                                e_step_share=spent["e_step"] / total)

        res = dict(views=a.views, points=a.points, noise=a.noise, iters=a.iters)
        for name, fn in (("adjusted_once", once), ("adjusted_per_round", per_round)):
            fn()                                                     # warm-up: library load, allocator, first launches
            runs = [fn() for _ in range(a.iters)]
            model = runs[-1][0]
            res[name] = {k: float(np.median([r[1][k] for r in runs])) for k in runs[0][1]}
            res[name].update(registered_images=len(model.images), points=len(model.points3D), drift=drift(model, scene),
                             linearisations=model.bundle_adjustment["iterations"])
            if model.round_adjustments is not None:
                res[name].update(rounds=len(model.round_adjustments), round_linearisations=[r["iterations"] for r in model.round_adjustments],
                                 added_observations=sum(r["added_observations"] for r in model.round_adjustments),
                                 dropped_observations=sum(r["dropped_observations"] for r in model.round_adjustments),
                                 dropped_points=sum(r["dropped_points"] for r in model.round_adjustments))
        res["per_round_over_once"] = res["adjusted_per_round"]["total_ms"] / res["adjusted_once"]["total_ms"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
