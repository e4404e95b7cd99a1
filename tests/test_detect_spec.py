"""The numpy specification of the device detectors (tests/util_detect.py) against the definitions it restates, its tie
rules, and the configuration / CLI plumbing of the hybrid extractor.  No GPU."""
import argparse

import numpy as np
import pytest

import util_detect as ud
from test_host_logic import checkerboard


def _patch(circle_values, centre, size=9):
    """A size x size grey patch, `centre` everywhere, with the 16 circle pixels of the middle set to circle_values."""
    g = np.full((size, size), centre, np.uint8)
    c = size // 2
    for (dx, dy), v in zip(ud.CIRCLE, circle_values):
        g[c + dy, c + dx] = v
    return g, c


# ---- FAST ------------------------------------------------------------------------------------------------------------
def test_fast_score_equals_its_definition_by_brute_force():
    rs = np.random.RandomState(3)
    nonzero = 0
    for trial in range(40):
        # small value ranges make long arcs (and therefore non-zero scores) frequent
        lo, hi = [(0, 256), (100, 140), (0, 4), (120, 125)][trial % 4]
        g = rs.randint(lo, hi, (9, 11)).astype(np.uint8)
        if trial % 3 == 0:
            g[3:6, 4:7] = rs.randint(0, 256)            # a blob against the ground
        s = ud.fast_score(g)
        for y in range(3, 6):
            for x in range(3, 8):
                assert s[y, x] == ud.fast_score_bruteforce(g, y, x), (trial, y, x)
                nonzero += s[y, x] > 0
        assert not s[:3].any() and not s[-3:].any() and not s[:, :3].any() and not s[:, -3:].any()
    assert nonzero >= 30, nonzero          # the comparison was not of zeros with zeros


def test_fast_threshold_and_arc_length():
    t = 10
    for arc, delta, corner in [(9, t + 1, True), (9, t, False), (8, t + 1, False), (8, 100, False), (16, t + 1, True)]:
        vals = [100 + delta if k < arc else 100 for k in range(16)]
        g, c = _patch(vals, 100)
        xy, total, sc = ud.fast_detect(g, threshold=t)
        found = any((x, y) == (c, c) for x, y in xy.astype(int))
        assert found == corner, (arc, delta)
        if corner:
            assert ud.fast_score(g)[c, c] == delta
    # dark arcs count as bright ones do, and the arc may wrap around the end of the circle
    vals = [100] * 16
    for k in (12, 13, 14, 15, 0, 1, 2, 3, 4):
        vals[k] = 100 - (t + 1)
    g, c = _patch(vals, 100)
    assert ud.fast_score(g)[c, c] == t + 1


def test_fast_ignores_corners_closer_than_3_to_the_edge():
    g = np.full((20, 20), 50, np.uint8)
    g[2, 2] = 255                       # an isolated bright pixel is a corner (all 16 circle pixels darker) ...
    g[10, 10] = 255
    xy, total, _ = ud.fast_detect(g)
    assert total == 1 and xy.tolist() == [[10.0, 10.0]]     # ... but not 2 pixels from the edge
    g[3, 16] = 255                      # exactly 3 from the top edge and from the right edge (x = w - 4): found
    xy, total, _ = ud.fast_detect(g)
    assert xy.tolist() == [[16.0, 3.0], [10.0, 10.0]]


def test_fast_limit_cuts_a_run_of_equal_scores_by_raster_position():
    g = ud.grey_u8(ud.noisy_checkerboard(3, 320, 240))
    xy_all, total, sc_all = ud.fast_detect(g, max_keypoints=1 << 30)
    assert total == len(xy_all) > 600
    n = 500
    xy, total2, sc = ud.fast_detect(g, max_keypoints=n)
    assert total2 == total and len(xy) == n
    cut = sc.min()
    tied_all, tied_kept = int((sc_all == cut).sum()), int((sc == cut).sum())
    assert 0 < tied_kept < tied_all, "the limit must cut through a run of equal scores for this test to mean anything"
    # every larger score is kept; of the tied ones exactly the first in raster order; the output is in raster order
    assert np.array_equal(xy[sc > cut], xy_all[sc_all > cut])
    assert np.array_equal(xy[sc == cut], xy_all[sc_all == cut][:tied_kept])
    key = xy[:, 1] * g.shape[1] + xy[:, 0]
    assert np.all(np.diff(key) > 0)


# ---- GFTT ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("image", ["noise", "rectangles", "checkerboard"])
def test_gftt_greedy_forms_agree_and_keep_the_minimum_distance(image):
    img = {"noise": lambda: ud.noisy_checkerboard(1, 320, 240), "rectangles": lambda: ud.rectangles(320, 240),
           "checkerboard": lambda: checkerboard(320, 240)}[image]()
    ys, xs, v = ud.gftt_candidates(ud.grey_u8(img))
    assert len(ys) > 50 and np.all(np.diff(v) <= 0)
    for max_corners in (40, 1 << 30):
        plain = ud.greedy_plain(ys, xs, 7, max_corners)
        assert ud.greedy_grid(ys, xs, 7, max_corners) == plain
        assert ud.greedy_rounds(ys, xs, 7, max_corners) == plain        # the parallel form of the kernel
    acc = np.array(plain)                                               # of the unlimited pass
    p = np.stack([ys[acc], xs[acc]], 1).astype(np.int64)
    d2 = ((p[:, None] - p[None]) ** 2).sum(-1)
    assert d2[~np.eye(len(p), dtype=bool)].min() >= 49
    accepted = np.zeros(len(ys), bool)
    accepted[acc] = True
    for i in np.nonzero(~accepted)[0]:      # every rejected candidate has a higher-ranked accepted one in range
        higher = acc[acc < i]
        assert (((ys[higher] - ys[i]) ** 2 + (xs[higher] - xs[i]) ** 2) < 49).any()


def test_gftt_tie_rule_on_a_pure_checkerboard():
    g = ud.grey_u8(checkerboard())
    ys, xs, v = ud.gftt_candidates(g)
    values, counts = np.unique(v, return_counts=True)
    assert len(ys) == 5940 and int(counts[counts > 1].sum()) >= 5939 - 1        # all but at most one value are shared
    idx = ys * g.shape[1] + xs
    same = v[1:] == v[:-1]
    assert same.sum() > 5000 and np.all(idx[1:][same] < idx[:-1][same])        # among equals the LATER position ranks first
    xy, n_cand = ud.gftt_detect(g)
    assert n_cand == 5940 and len(xy) == 330


def test_gftt_uniform_image_has_no_corners():
    xy, n = ud.gftt_detect(np.full((32, 40), 77, np.uint8))
    assert n == 0 and xy.shape == (0, 2)


def test_grey_is_opencvs_fixed_point():
    bgr = np.array([[[255, 255, 255], [0, 0, 0], [255, 0, 0], [0, 255, 0], [0, 0, 255], [10, 200, 31]]], np.uint8)
    want = [255, 0, (1868 * 255 + 8192) >> 14, (9617 * 255 + 8192) >> 14, (4899 * 255 + 8192) >> 14,
            (1868 * 10 + 9617 * 200 + 4899 * 31 + 8192) >> 14]
    assert ud.grey_u8(bgr)[0].tolist() == want


# ---- configuration / CLI ---------------------------------------------------------------------------------------------
def test_config_and_cli_carry_the_hybrid_extractor_and_its_detector(monkeypatch):
    from vit_colmap_amd.pipeline import run_pipeline
    from vit_colmap_amd.utils.config import Config, ExtractorConfig

    assert ExtractorConfig().detector_type == "sift"
    cfg = Config.from_args(argparse.Namespace(extractor="hybrid", detector="gftt"))
    assert cfg.extractor.extractor_type == "hybrid" and cfg.extractor.detector_type == "gftt"
    assert Config.from_args(argparse.Namespace(extractor="hybrid")).extractor.detector_type == "sift"   # no --detector flag

    seen = {}

    class FakePipeline:
        def __init__(self, config):
            seen["config"] = config

        def run(self, *a):
            seen["run"] = a

    monkeypatch.setattr(run_pipeline, "Pipeline", FakePipeline)
    monkeypatch.setattr("sys.argv", ["prog", "--images", "i", "--output", "o", "--db", "d.db", "--extractor", "hybrid",
                                     "--detector", "fast"])
    run_pipeline.main()
    assert seen["config"].extractor.extractor_type == "hybrid" and seen["config"].extractor.detector_type == "fast"
    monkeypatch.setattr("sys.argv", ["prog", "--images", "i", "--output", "o", "--db", "d.db", "--detector", "orb"])
    with pytest.raises(SystemExit):
        run_pipeline.main()


def test_pipeline_builds_the_hybrid_extractor_with_the_device_backend(monkeypatch):
    from vit_colmap_amd.features import hybrid_extractor
    from vit_colmap_amd.pipeline.run_pipeline import Pipeline
    from vit_colmap_amd.utils.config import Config

    made = {}

    class Fake:
        def __init__(self, **kw):
            made.update(kw)

    monkeypatch.setattr(hybrid_extractor, "HybridViTExtractor", Fake)
    cfg = Config()
    cfg.extractor.extractor_type, cfg.extractor.detector_type, cfg.extractor.vit_weights_path = "hybrid", "fast", "w.pth"
    assert isinstance(Pipeline(cfg)._make_extractor(), Fake)
    assert made == {"weights_path": "w.pth", "detector_type": "fast", "detector_backend": "hip"}


def test_orb_without_opencv_names_the_detectors_that_work(monkeypatch):
    from vit_colmap_amd import _lib
    from vit_colmap_amd.features import hybrid_extractor as he

    class NoViT:
        def __init__(self, **kw):
            self.device, self.descriptor_projection = "cpu", None

    monkeypatch.setattr(he, "ViTExtractor", NoViT)
    monkeypatch.setattr(he, "_cv2_importable", lambda: False)
    for backend in ("auto", "hip"):
        with pytest.raises(_lib.HipLibraryError) as e:
            he.HybridViTExtractor(detector_type="orb", detector_backend=backend)
        assert all(name in str(e.value) for name in ("sift", "fast", "gftt"))
    for det in ("sift", "fast", "gftt"):
        ex = he.HybridViTExtractor(detector_type=det)          # the default constructor works without OpenCV
        assert ex.detector_backend == "hip" and ex.batch_size > 1
    ex = he.HybridViTExtractor(detector_type="orb", keypoint_fn=lambda img: np.zeros((0, 2), np.float32))
    assert ex.detector_backend == "keypoint_fn" and ex.batch_size == 1
    with pytest.raises(ValueError):
        he.HybridViTExtractor(detector_backend="opencl")
    with pytest.raises(ValueError):
        he.HybridViTExtractor(detector_type="harris")
