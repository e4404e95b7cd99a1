"""CPU tests of the SIFT extractor's specification (tests/util_sift.py), its host-side rules and C-ABI argument checks,
and the pipeline's "sift" dispatch.  No kernels are launched."""
import ctypes
import math

import numpy as np
import pytest

import util_sift as us
from vit_colmap_amd.features.sift_extractor import SiftExtractor, SiftOptions, select_rows
from vit_colmap_amd.utils import Config


def blob_image(n, t, amp=200.0, bg=30.0):
    yy, xx = np.mgrid[:n, :n]
    c = n // 2
    g = bg + amp * np.exp(-((xx - c) ** 2 + (yy - c) ** 2) / (2.0 * t * t))
    return np.repeat(np.round(g).astype(np.uint8)[..., None], 3, 2), c


def textured(seed, h, w, sigma=2.0):
    """Seeded smooth random texture (uint8 BGR), the same image in every channel."""
    rs = np.random.RandomState(seed)
    g = us.blur(rs.rand(h, w).astype(np.float32), us.gaussian_taps(sigma))
    g = (g - g.min()) / (g.max() - g.min())
    return np.repeat(np.round(255 * g).astype(np.uint8)[..., None], 3, 2)


@pytest.mark.parametrize("t", [2, 4, 8])
def test_gaussian_blob_gives_one_keypoint_at_its_centre(t):
    img, c = blob_image(24 * t + 48, t)
    rows, desc = us.extract(img, SiftOptions())
    pos = np.unique(rows[:, :2], axis=0)
    assert len(pos) == 1, rows
    assert np.abs(pos[0] - (c + 0.5)).max() <= 0.05
    sigma = np.hypot(rows[:, 2], rows[:, 4])
    # the DoG between levels s and s+1 peaks at the lower level's sigma times 2^(-1/2S) (S = 3) for a blob of std t
    assert np.all(np.abs(sigma - t * 2 ** (-1 / 6)) <= 0.1 * t), sigma
    assert desc.shape == (len(rows), 128) and desc.dtype == np.uint8


@pytest.mark.parametrize("S", [1, 2, 4, 8])
def test_gaussian_blob_scale_for_every_octave_resolution(S):
    sigma = {}
    for t in (4, 8):
        img, c = blob_image(24 * t + 48, t)
        rows, _ = us.extract(img, SiftOptions(octave_resolution=S))
        pos = np.unique(rows[:, :2], axis=0)
        assert len(pos) == 1, rows
        assert np.abs(pos[0] - (c + 0.5)).max() <= 0.05
        s = np.hypot(rows[:, 2], rows[:, 4])
        assert np.ptp(s) <= 1e-5 * s[0]
        sigma[t] = float(s[0])
        # the DoG between levels sigma and sigma 2^(1/S) peaks at sigma 2^(-1/2S) = t: within 3 % (1.1 % .. 2.4 % seen
        # at S = 1, less for larger S); a sigma0 that ignores S is off by 2^(1/S - 1/3): 59 % at S = 1, 6 % at S = 4,
        # 13 % at S = 8
        assert abs(sigma[t] / (t * 2 ** (-1 / (2 * S))) - 1) <= 0.03, (t, sigma[t])
    # doubling the blob doubles sigma: the image's own 0.5 px blur and sampling shift the ratio by about 0.3 % at
    # t = 4 -> 8, so 1 % of 2 is a tight bound that still holds for every S
    assert abs(sigma[8] / sigma[4] - 2) <= 0.02, sigma


def test_flat_and_tiny_images_give_no_keypoints():
    for img in (np.full((120, 160, 3), 128, np.uint8), np.random.RandomState(1).randint(0, 256, (3, 2, 3), np.uint8)):
        rows, desc = us.extract(img, SiftOptions())
        assert rows.shape == (0, 6) and desc.shape == (0, 128)


def test_rot90_equivariance():
    img = textured(3, 161, 161)            # 161 = 5 * 32 + 1: every octave's grid is mirror-symmetric in its interior
    opts = SiftOptions()
    r0, d0 = us.extract(img, opts)
    r1, d1 = us.extract(np.ascontiguousarray(np.rot90(img)), opts)
    assert len(r0) > 50
    # np.rot90: new[i, j] = old[j, w - 1 - i]; in pixel-centre coordinates (x, y) -> (y, w - x)
    exp_xy = np.stack([r0[:, 1], 161.0 - r0[:, 0]], 1)
    th0 = np.arctan2(r0[:, 4], r0[:, 2])
    th1 = np.arctan2(r1[:, 4], r1[:, 2])
    hits = 0
    for i in range(len(r0)):
        d = np.hypot(*(r1[:, :2] - exp_xy[i]).T)
        cand = np.nonzero(d < 0.05)[0]
        if len(cand) == 0:
            continue
        dth = np.abs((th1[cand] - th0[i] + np.pi / 2 + np.pi) % (2 * np.pi) - np.pi)
        k = cand[np.argmin(dth)]
        if dth.min() > 0.05:
            continue
        l1 = np.abs(d1[k].astype(np.int32) - d0[i].astype(np.int32)).sum()
        if l1 <= 0.05 * d0[i].astype(np.int32).sum():
            hits += 1
    assert hits >= 0.9 * len(r0), (hits, len(r0))


def test_max_num_features_keeps_coarsest_octaves_and_truncates_in_order():
    assert select_rows([50, 30, 20, 10], 35) == [0, 5, 20, 10]
    assert select_rows([50, 30, 20, 10], 1000) == [50, 30, 20, 10]
    assert select_rows([5, 0, 7], 3) == [0, 0, 3]
    for counts, k in (([50, 30, 20, 10], 35), ([3, 9, 1], 4)):
        assert us.select_rows(counts, k) == select_rows(counts, k)
    img = textured(5, 160, 200)
    full_r, full_d, st = us.extract(img, SiftOptions(max_num_features=100000), return_stages=True)
    per = []
    for s in st:
        n = 0
        for kp in s["kps"]:
            mod, ang = us.gradient(s["levels"][int(kp[4])])
            n += min(len(us.orientations(mod, ang, kp)), 2)
        per.append(n)
    assert sum(per) == len(full_r) and len(per) >= 3 and per[-1] > 0
    k = per[-1] + per[-2] + 5            # the two coarsest octaves whole, the first 5 rows of the one before
    assert per[-3] >= 5
    r, d = us.extract(img, SiftOptions(max_num_features=k))
    lo, hi = sum(per[:-3]), sum(per[:-2])
    assert len(r) == k
    assert np.array_equal(r, np.concatenate([full_r[lo:lo + 5], full_r[hi:]]))
    assert np.array_equal(d, np.concatenate([full_d[lo:lo + 5], full_d[hi:]]))


def test_quantiser_rounds_half_up_and_clamps():
    v = np.array([0.0, 0.5 / 512, 1.49 / 512, 1.5 / 512, 254.5 / 512, 0.6, 1.0], np.float32)
    assert us.quantize(v).tolist() == [0, 1, 1, 2, 255, 255, 255]


def test_l1_root_rows_have_unit_norm_before_quantisation():
    img = textured(7, 120, 160)
    g = us.grey(img)
    (o, levels, dog), = us.pyramid(g, 3, -1, 1)
    kps = us.detect(dog, 3, 0.02 / 3, 10)
    assert len(kps) > 10
    for kp in kps[:20]:
        mod, ang = us.gradient(levels[int(kp[4])])
        for a in us.orientations(mod, ang, kp)[:2]:
            for norm in ("L1_ROOT", "L2"):
                v = us.descriptor(mod, ang, kp, a, norm)
                assert abs(float(np.sqrt((v.astype(np.float64) ** 2).sum())) - 1.0) < 1e-3
                assert v.min() >= 0


def test_affine_keypoint_layout():
    rows, _ = us.extract(textured(9, 100, 140), SiftOptions())
    assert rows.ndim == 2 and rows.shape[1] == 6 and len(rows) > 0
    a11, a12, a21, a22 = rows[:, 2], rows[:, 3], rows[:, 4], rows[:, 5]
    assert np.allclose(a11, a22) and np.allclose(a12, -a21)
    s = np.hypot(a11, a21)
    assert np.all(s > 0.5) and np.allclose(a11 * a22 - a12 * a21, s * s, rtol=1e-5)
    r = us.affine_rows(np.float32([3.0]), np.float32([4.0]), np.float32([2.0]), np.float32([math.pi / 2]))
    assert np.allclose(r, [[3.5, 4.5, 0.0, -2.0, 2.0, 0.0]], atol=1e-6)


def test_options_refuse_what_is_not_built():
    for bad in (dict(estimate_affine_shape=True), dict(domain_size_pooling=True), dict(darkness_adaptivity=True),
                dict(normalization="L1"), dict(first_octave=1), dict(max_num_orientations=5)):
        with pytest.raises(ValueError):
            SiftOptions(**bad).validate()
    o = SiftOptions()
    assert (o.max_image_size, o.max_num_features, o.first_octave, o.num_octaves, o.octave_resolution) == (3200, 8192, -1, 4, 3)
    assert (o.peak_threshold, o.edge_threshold, o.max_num_orientations, o.upright, o.normalization) == \
        (0.02 / 3, 10.0, 2, False, "L1_ROOT")


def test_pipeline_dispatch_sift(tmp_path):
    from vit_colmap_amd._lib import HipLibraryError
    from vit_colmap_amd.pipeline import Pipeline

    c = Config()
    c.extractor.extractor_type = "sift"
    assert isinstance(Pipeline(c)._make_extractor(), SiftExtractor)
    (tmp_path / "images").mkdir()
    from vit_colmap_amd.utils import image_io

    image_io.imwrite(tmp_path / "images" / "a.png", textured(1, 64, 64))
    with pytest.raises(HipLibraryError):
        SiftExtractor(device="cpu").extract(tmp_path / "images", tmp_path / "d.db", "SIMPLE_PINHOLE")
    with pytest.raises(HipLibraryError):
        SiftExtractor(device="cpu")._run_batch([textured(1, 64, 64)])
    c.extractor.extractor_type = "colmap_sift"
    with pytest.raises(NotImplementedError):
        Pipeline(c).run(tmp_path, tmp_path / "o", tmp_path / "d2.db")


def test_sift_abi_rejects_bad_arguments_without_gpu():
    from vit_colmap_amd import _lib

    lib = _lib.load()
    fake = ctypes.c_void_p(256)
    taps = np.ones(2 * 65 + 1, np.float32)
    tp = taps.ctypes.data_as(_lib._f32p)
    assert lib.vc_sift_grey(None, 1, 4, 4, 4, 4, 1, None, None) == -1
    assert lib.vc_sift_grey(fake, 1, 4, 4, 8, 4, 0, fake, None) == -1           # no upscaling resize
    assert lib.vc_sift_blur(fake, fake, fake, 1, 4, 4, tp, 2, None) == -1       # tmp aliases src
    assert lib.vc_sift_blur(fake, ctypes.c_void_p(512), fake, 1, 4, 4, tp, 65, None) == -2
    assert lib.vc_sift_downsample(fake, 1, 1, 4, fake, None) == -1
    assert lib.vc_sift_dog(fake, 1, 1, 4, 4, fake, None) == -1
    assert lib.vc_sift_detect(None, 1, 8, 8, 5, 0.01, 10.0, 1, fake, 16, fake, fake, None) == -1
    assert lib.vc_sift_detect(fake, 1, 8, 8, 5, 0.01, 0.0, 1, fake, 16, fake, fake, None) == -1
    assert lib.vc_sift_orient(fake, 6, 1, 8, 8, fake, fake, 16, 5, 0, fake, fake, None) == -1
    assert lib.vc_sift_describe(fake, 6, 1, 8, 8, fake, fake, 16, fake, fake, 2, 1, 1.0, 1.0, 1.0, fake, 31, fake, fake,
                                fake, None) == -4
    assert lib.vc_sift_describe(fake, 6, 1, 8, 8, fake, fake, 16, fake, fake, 2, 7, 1.0, 1.0, 1.0, fake, 32, fake, fake,
                                fake, None) == -1
