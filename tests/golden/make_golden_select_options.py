#!/usr/bin/env python3
"""Golden vectors for the selection stages OFF the reference's defaults (bin size 16, NMS radius 1.5).

Run in the build container only (needs the reference checkout, like make_golden.py):

    python tests/golden/make_golden_select_options.py

Runs the reference's own `ViTExtractor._spatial_binning_selection` and `_apply_nms` (loaded the way
make_golden.py loads them) on seeded, tie-free score maps and writes `select_options.npz`: per case the
parameters and the two coordinate lists (the scores are the map's values at those coordinates, so they are
not stored).  The score map of a case is `score_map(seed, H, W)` below; tests/test_select_rule.py restates
that line.

The radii include the float32 roots of d^2 = 5, 10, 20, 26, 37, 40, 41, 58, 61: there `sqrt(d^2) < r`
(the reference's rule, float32) and `d^2 < r^2` disagree, and every cell of the grid is a candidate, so
pairs at exactly that distance are present in each of those cases.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import assert_distinct, bare_extractor, load_reference  # noqa: E402


def root32(d2):
    return float(np.sqrt(np.float32(d2)))


# (seed, H, W, bin_size, target, nms_radius)
CASES = [
    (101, 12, 17, 5, 40, 2.5),        # 2 x 3 bins, ragged margins, 6 per bin
    (102, 9, 9, 3, 81, 1.0),          # every cell a candidate, radius 1: nothing at distance < 1
    (103, 20, 31, 8, 64, 3.0),        # 2 x 3 bins of 64 cells, 10 per bin
    (104, 6, 40, 2, 100, 4.75),       # 60 bins, one per bin, then no cut
    (105, 11, 13, 4, 5, 2.0),         # target below the number of bins: one per bin, global cut to 5
    (106, 11, 13, 4, 30, 0.0),        # radius 0: NMS keeps everything
    (107, 10, 10, 5, 100, 8.0),       # the largest radius
    (108, 7, 5, 32, 35, 0.5),         # bin larger than the grid
] + [(110 + d2, 10, 11, 16, 110, root32(d2)) for d2 in (5, 10, 20, 26, 37, 40, 41, 58, 61)]


def score_map(seed, H, W):
    return np.random.RandomState(seed).rand(H, W).astype(np.float32)


def main():
    torch.set_num_threads(1)
    ex = bare_extractor(load_reference(), 0, 0, "harris")
    out = {"params": np.array(CASES, dtype=np.float64)}
    for i, (seed, H, W, bin_size, target, radius) in enumerate(CASES):
        score = score_map(seed, H, W)
        assert_distinct(score.reshape(-1), f"case {i}: score map")
        with torch.no_grad():
            coords, scores = ex._spatial_binning_selection(torch.from_numpy(score), target, bin_size=bin_size)
            kept, kept_scores = ex._apply_nms(coords, scores, nms_radius=radius)
        coords, kept = coords.numpy(), kept.numpy()
        assert np.array_equal(scores.numpy(), score[coords[:, 0], coords[:, 1]])
        assert np.array_equal(kept_scores.numpy(), score[kept[:, 0], kept[:, 1]])
        out[f"bin_{i}"] = coords.astype(np.uint8)
        out[f"nms_{i}"] = kept.astype(np.uint8)
        print(f"case {i}: {H}x{W} bin {bin_size} target {target} radius {radius!r}: binned {len(coords)} kept {len(kept)}")
    path = os.path.join(HERE, "select_options.npz")
    np.savez_compressed(path, **out)
    print(f"-> {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
