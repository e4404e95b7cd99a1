"""CPU checks of the selection oracle off the reference's defaults: the NMS distance rule at every
attainable distance, and binning / top-k / NMS against vectors the reference's own functions produced
at other bin sizes and radii (tests/golden/make_golden_select_options.py -> select_options.npz)."""
import os

import numpy as np

from oracle import select_oracle as so
from util_select import ATTAINABLE_D2, radii_near_root, reference_suppresses

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def test_nms_rule_is_the_references_at_every_distance_and_radius():
    """`apply_nms` on two points at squared distance d2 keeps one or two exactly as the reference's comparison
    `sqrt(d2) < r` in float32 (vit_extractor.py:534-537) says: every d2 = a^2 + b^2 <= 128 (a, b <= 8), every float32
    radius within 3 ulp of its root, and the radii of the option sweep."""
    scores = np.array([0.75, 0.25], np.float32)
    n_differs_from_square_rule = 0
    for d2, (a, b) in sorted(ATTAINABLE_D2.items()):
        coords = np.array([[3, 2], [3 + a, 2 + b]], np.int64)
        for r in radii_near_root(d2) + [0.0, 0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 4.75, 8.0]:
            kept, kept_s = so.apply_nms(coords, scores, r)
            want = 1 if reference_suppresses(d2, r) else 2
            assert len(kept) == want, (d2, r)
            assert np.array_equal(kept[0], coords[0]) and kept_s[0] == scores[0]
            n_differs_from_square_rule += (np.float32(d2) < np.float32(r) * np.float32(r)) != reference_suppresses(d2, r)
    # the corner is real: the float32 product rule is a different function on this domain
    assert n_differs_from_square_rule > 0
    assert not reference_suppresses(37, float(np.sqrt(np.float32(37)))) and np.float32(37) < np.sqrt(np.float32(37)) ** 2
    assert not reference_suppresses(61, float(np.sqrt(np.float32(61)))) and np.float32(61) < np.sqrt(np.float32(61)) ** 2


def test_oracle_equals_reference_off_the_defaults():
    g = np.load(os.path.join(GOLD, "select_options.npz"))
    params = g["params"]
    assert len(params) >= 12
    corner_d2 = set()
    for i, (seed, H, W, bin_size, target, radius) in enumerate(params):
        seed, H, W, bin_size, target = int(seed), int(H), int(W), int(bin_size), int(target)
        score = np.random.RandomState(seed).rand(H, W).astype(np.float32)
        want_bin = g[f"bin_{i}"].astype(np.int64)
        want_nms = g[f"nms_{i}"].astype(np.int64)
        coords, scores = so.spatial_binning_selection(score, target, bin_size)
        assert np.array_equal(coords, want_bin), i
        assert np.array_equal(scores, score[want_bin[:, 0], want_bin[:, 1]]), i
        kept, kept_s = so.apply_nms(coords, scores, float(radius))
        assert np.array_equal(kept, want_nms), (i, radius)
        assert np.array_equal(kept_s, score[want_nms[:, 0], want_nms[:, 1]]), i
        for d2 in ATTAINABLE_D2:
            if float(np.sqrt(np.float32(d2))) == radius:
                corner_d2.add(d2)
    assert corner_d2 >= {5, 10, 20, 26, 37, 40, 41, 58, 61}        # the radii where d2 < r^2 is the wrong rule
    assert len({int(p[3]) for p in params}) >= 6 and 16 in {int(p[3]) for p in params}   # bin sizes off (and on) the default
