"""extract_device across the SiftOptions that validate() accepts, not only COLMAP's defaults: octave resolutions 1 .. 8,
both first octaves, L2 normalisation, upright, 1 .. 4 orientations, the detect relaunch, empty results, the edge
threshold, the octave count, truncation by max_num_features, degenerate image sizes and launch groups.  Each run is
checked stage by stage (bit-exact) and row by row (within tolerance) against tests/util_sift.py."""
import numpy as np
import pytest

import util_sift as us
from test_sift_gpu import colour, compare_rows, dev, textured
from vit_colmap_amd.features import sift_extractor as se
from vit_colmap_amd.features.sift_extractor import SiftExtractor, SiftOptions

pytestmark = pytest.mark.gpu


def egg_crate(h, w, period=7, seed=0):
    """cos x cos y of the given period (pixels) plus a little noise: an extremum every half period in x and y, dense
    enough that octave -1 holds more keypoints than extract_device's first detect cap."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[:h, :w].astype(np.float64)
    g = 127.5 + 100 * np.cos(2 * np.pi * xx / period) * np.cos(2 * np.pi * yy / period) + rs.uniform(-3, 3, (h, w))
    return np.repeat(np.clip(np.round(g), 0, 255).astype(np.uint8)[..., None], 3, 2)


def check_stages(img, opts):
    """Grey image, Gaussian levels, DoG, unrefined extrema and accepted keypoints of every octave, bit-exact (the checks
    of test_sift_gpu.test_kernels_match_oracle for any options) -> the oracle's keypoint count per octave."""
    S = opts.octave_resolution
    batch = dev([img])
    g = us.grey(img, opts.max_image_size)
    o_pyr = us.pyramid(g, S, opts.first_octave, opts.num_octaves)
    counts = []
    for (o, oc), (oo, lv, dog) in zip(se.pyramid_octaves(batch, opts), o_pyr):
        assert o == oo
        assert np.array_equal(oc.levels[:, 0].cpu().numpy(), lv), f"Gaussian levels differ (octave {o})"
        assert np.array_equal(oc.dog[:, 0].cpu().numpy(), dog), f"DoG differs (octave {o})"
        kp, _, n = se._detect(oc, S, opts, cap=4096, refine=False)
        raw = kp[0, : int(n[0])].cpu().numpy()
        exp = us._extrema(dog, S, us.prefilter_of(opts.peak_threshold))
        assert np.array_equal(raw[:, 4:7].astype(np.int64), exp), f"unrefined extrema differ (octave {o})"
        kp, _, n = se._detect(oc, S, opts, cap=4096)
        ref = kp[0, : int(n[0])].cpu().numpy()
        exp = us.detect(dog, S, opts.peak_threshold, opts.edge_threshold)
        assert np.array_equal(ref[:, 4:7], exp[:, 4:7]), f"accepted keypoints differ (octave {o})"
        assert np.abs(ref[:, :3] - exp[:, :3]).max(initial=0) <= 1e-5
        counts.append(len(exp))
    assert len(counts) == len(o_pyr)
    return counts


def check_rows(g_rows, g_desc, o_rows, o_desc):
    """DESIGN.md §4.7's tolerances; an empty oracle result must be an empty GPU result."""
    m = len(g_rows)
    if len(o_rows) == 0:
        assert m == 0
        return
    share, diffs = compare_rows(o_rows, o_desc, g_rows, g_desc)
    assert share >= 0.995, share
    assert (diffs == 0).mean() >= 0.99, (diffs == 0).mean()
    assert np.abs(diffs).max() <= 1
    assert abs(m - len(o_rows)) <= 0.005 * len(o_rows) + 1


def gpu_rows(res, b):
    m = int(res["count"][b])
    K = res["keypoints"].shape[1]
    kps, desc = res["keypoints"][b].cpu().numpy(), res["descriptors"][b].cpu().numpy()
    assert not kps[m:].any() and not desc[m:].any(), "rows past count are not zero"
    assert m <= K
    return kps[:m], desc[:m]


def check_extract(img, opts, min_rows=1):
    counts = check_stages(img, opts)
    o_rows, o_desc = us.extract(img, opts)
    assert len(o_rows) >= min_rows
    g_rows, g_desc = gpu_rows(se.extract_device(dev([img]), opts), 0)
    check_rows(g_rows, g_desc, o_rows, o_desc)
    return counts, o_rows, g_rows


@pytest.mark.parametrize("S", [1, 2, 4, 8])
@pytest.mark.parametrize("first_octave", [-1, 0])
def test_octave_resolution(S, first_octave):
    check_extract(colour(50 + S, 120, 160), SiftOptions(octave_resolution=S, first_octave=first_octave), min_rows=20)


@pytest.mark.parametrize("kw", [dict(normalization="L2"), dict(upright=True), dict(max_num_orientations=1),
                                dict(max_num_orientations=3), dict(max_num_orientations=4), dict(edge_threshold=1.5),
                                dict(edge_threshold=50.0), dict(num_octaves=1), dict(num_octaves=12),
                                dict(upright=True, normalization="L2", octave_resolution=2)],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_options(kw):
    img = colour(61, 128, 176)
    opts = SiftOptions(**kw)
    counts, o_rows, g_rows = check_extract(img, opts, min_rows=50)
    theta = np.arctan2(g_rows[:, 4], g_rows[:, 2])
    if opts.upright:
        assert np.all(theta == 0)
    if kw.get("num_octaves") == 12:
        assert len(counts) == len(us.pyramid(us.grey(img), 3, -1, 12)) < 12      # MIN_OCTAVE_SIZE ends the pyramid
    if kw.get("num_octaves") == 1:
        assert len(counts) == 1


def test_max_orientations_change_the_rows():
    """More orientations per keypoint give more rows, and max_num_orientations = 1 keeps the first peak only."""
    img = colour(61, 128, 176)
    n = {k: len(us.extract(img, SiftOptions(max_num_orientations=k))[0]) for k in (1, 2, 4)}
    assert n[1] < n[2] < n[4]
    for k in (1, 4):
        res = se.extract_device(dev([img]), SiftOptions(max_num_orientations=k))
        assert abs(int(res["count"][0]) - n[k]) <= 0.005 * n[k] + 1


def test_peak_threshold_zero_relaunches_detect():
    img = egg_crate(120, 160)
    opts = SiftOptions(peak_threshold=0.0)
    counts, o_rows, _ = check_extract(img, opts, min_rows=1000)
    first_cap = [max(1024, h * w // 64) for _, h, w in se.octave_sizes(160, 120, opts)]
    assert any(c > cap for c, cap in zip(counts, first_cap)), (counts, first_cap)   # _detect's second launch ran


def test_threshold_above_every_response_gives_no_rows():
    img = colour(62, 120, 160)
    opts = SiftOptions(peak_threshold=10.0)
    assert sum(check_stages(img, opts)) == 0
    res = se.extract_device(dev([img, img[::-1].copy()]), opts)
    assert res["count"].tolist() == [0, 0]
    assert not res["keypoints"].any() and not res["descriptors"].any()


def test_max_num_features_truncates_inside_an_octave():
    img = colour(63, 120, 160)
    full, _ = us.extract(img, SiftOptions(max_num_features=100000))
    K = len(full) - 7                          # the finest octave loses its last 7 rows, the coarser ones stay whole
    opts = SiftOptions(max_num_features=K)
    o_rows, o_desc = us.extract(img, opts)
    assert len(o_rows) == K
    res = se.extract_device(dev([img]), opts)
    assert int(res["count"][0]) == K
    check_rows(*gpu_rows(res, 0), o_rows, o_desc)


@pytest.mark.parametrize("h,w", [(3, 2), (5, 7), (4, 1000), (1000, 4)])
def test_degenerate_sizes(h, w):
    img = colour(64, h, w) if min(h, w) > 2 else np.random.RandomState(1).randint(0, 256, (h, w, 3)).astype(np.uint8)
    opts = SiftOptions()
    n_oct = len(se.octave_sizes(w, h, opts))
    assert n_oct == {(3, 2): 0, (5, 7): 1}.get((h, w), n_oct)
    check_stages(img, opts)
    o_rows, o_desc = us.extract(img, opts)
    res = se.extract_device(dev([img, np.ascontiguousarray(img[::-1, ::-1])]), opts)
    check_rows(*gpu_rows(res, 0), o_rows, o_desc)
    check_rows(*gpu_rows(res, 1), *us.extract(np.ascontiguousarray(img[::-1, ::-1]), opts))


def test_batch_of_flat_tiny_and_full_textures():
    h, w = 120, 160
    flat = np.full((h, w, 3), 90, np.uint8)
    tiny = flat.copy()
    tiny[50:70, 60:84] = textured(65, 20, 24)
    imgs = [flat, tiny, colour(66, h, w), colour(67, h, w)]
    opts = SiftOptions()
    res = se.extract_device(dev(imgs), opts)
    assert int(res["count"][0]) == 0
    for b, img in enumerate(imgs):
        check_rows(*gpu_rows(res, b), *us.extract(img, opts))
    assert int(res["count"][1]) > 0


def test_launch_groups_equal_single_calls(monkeypatch):
    imgs = [colour(70 + i, 96, 128) for i in range(8)]
    ex = SiftExtractor(device="cuda", batch_size=16)
    per_image = (2 * 3 + 6) * 4 * 4 * 96 * 128
    monkeypatch.setattr(se, "LEVEL_BYTES_BUDGET", 3 * per_image + per_image // 2)
    assert ex._group_size(96, 128) == 3
    groups = ex._run_batch(imgs)
    for img, (k, d) in zip(imgs, groups):
        s = se.extract_device(dev([img]))
        n = int(s["count"][0])
        assert n == len(k) > 0
        assert np.array_equal(s["keypoints"][0, :n].cpu().numpy(), k)
        assert np.array_equal(s["descriptors"][0, :n].cpu().numpy(), d)
