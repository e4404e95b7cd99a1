"""The seven vc_sift_* entry points one at a time on hand-built inputs, against tests/util_sift.py: blur radii up to
VC_SIFT_MAX_RADIUS, odd and degenerate shapes, every octave resolution the options allow, the detect cap path,
crafted orientation histograms and the descriptor's row offsets, normalisations and scales.

Every entry point runs with B >= 2 (different content per image) and with B = 1 into a larger backing buffer whose
tail holds a sentinel that must survive the call."""
import math
import types

import numpy as np
import pytest
import torch

import util_sift as us
from vit_colmap_amd import _lib
from vit_colmap_amd.features import sift_extractor as se
from vit_colmap_amd.features.sift_extractor import SiftOptions

pytestmark = pytest.mark.gpu

F = np.float32
TAIL = 4099                          # sentinel elements behind the B = 1 outputs
SENTINEL_F32 = -12345.678
SENTINEL_I32 = -0x5A5A5A5
SENTINEL_U8 = 0xA5
PEAK = 0.02 / 3                      # COLMAP's default peak_threshold


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def backed(n, dtype, sentinel):
    """(view of the first n elements, the whole backing buffer) of a 1-D device buffer pre-filled with a sentinel."""
    buf = torch.full((n + TAIL,), sentinel, dtype=dtype, device="cuda")
    return buf[:n], buf


def assert_tail(buf, n, sentinel, what):
    tail = buf[n:].cpu().numpy()
    assert np.array_equal(tail, np.full_like(tail, sentinel)), f"{what}: the sentinel behind the output was overwritten"


def call(name, *args):
    """One C-ABI call.  numpy arrays are copied to the GPU and tensors passed by pointer; the call holds both until the
    kernels have finished (a pointer to a temporary would let the allocator hand its memory to the next copy)."""
    held = [cuda(a) if isinstance(a, np.ndarray) else a for a in args]
    _lib.check(getattr(_lib.load(), name)(*[P(a) if isinstance(a, torch.Tensor) else a for a in held]), name)
    torch.cuda.synchronize()


P, S_ = _lib.ptr, _lib.stream_ptr


# ---- vc_sift_blur ---------------------------------------------------------------------------------------------------
def blur64(img, taps):
    """float64 correlation of the same taps, edge replicate, rows then columns: the spec of the float32 oracle."""
    r = (len(taps) - 1) // 2
    h, w = img.shape
    t = taps.astype(np.float64)
    pad = np.pad(img.astype(np.float64), ((0, 0), (r, r)), mode="edge")
    acc = sum(t[k] * pad[:, k:k + w] for k in range(2 * r + 1))
    pad = np.pad(acc, ((r, r), (0, 0)), mode="edge")
    return sum(t[k] * pad[k:k + h, :] for k in range(2 * r + 1))


def run_blur(imgs, taps):
    B, (h, w) = len(imgs), imgs[0].shape
    src = cuda(np.stack(imgs))
    tmp = torch.empty((B, h, w), dtype=torch.float32, device="cuda")
    dst = torch.empty_like(tmp)
    call("vc_sift_blur", P(src), P(tmp), P(dst), B, h, w, taps.ctypes.data_as(_lib._f32p), (len(taps) - 1) // 2, S_())
    return dst.cpu().numpy()


@pytest.mark.parametrize("r", [1, 2, 13, 14, 45, 63, 64])
@pytest.mark.parametrize("h,w", [(1, 1), (1, 300), (300, 1), (3, 5), (63, 64), (65, 257), (130, 513)])
def test_blur_any_radius_and_shape(r, h, w):
    rs = np.random.RandomState(1000 * r + h + w)
    taps = rs.uniform(0.1, 1.0, 2 * r + 1).astype(F)            # asymmetric: a reversed tap order fails
    taps = (taps / taps.sum(dtype=np.float64)).astype(F)
    imgs = [rs.rand(h, w).astype(F) for _ in range(3)]
    out = run_blur(imgs, taps)
    for b, img in enumerate(imgs):
        exp = us.blur(img, taps)
        assert np.array_equal(out[b], exp), f"image {b} differs from util_sift.blur"
        # float32 sums of <= 129 positive terms of at most 1: both passes within (2 (2r + 1) + 2) 2^-24 of float64
        assert np.abs(exp - blur64(img, taps)).max() <= (4 * r + 4) * 2.0 ** -24
    assert not np.array_equal(us.blur(imgs[0], taps[::-1].copy()), out[0]) or h * w == 1
    # B = 1 into backed buffers: nothing is written behind h x w
    src = cuda(imgs[1])
    tmp, tbuf = backed(h * w, torch.float32, SENTINEL_F32)
    dst, dbuf = backed(h * w, torch.float32, SENTINEL_F32)
    call("vc_sift_blur", P(src), P(tmp), P(dst), 1, h, w, taps.ctypes.data_as(_lib._f32p), r, S_())
    assert np.array_equal(dst.cpu().numpy().reshape(h, w), out[1])
    assert_tail(tbuf, h * w, SENTINEL_F32, "blur tmp")
    assert_tail(dbuf, h * w, SENTINEL_F32, "blur dst")


# ---- vc_sift_grey, vc_sift_downsample, vc_sift_dog ---------------------------------------------------------------------
@pytest.mark.parametrize("h,w,oh,ow", [(7, 9, 7, 9), (1, 1, 1, 1), (5, 9, 1, 9), (5, 9, 5, 1), (5, 9, 1, 1),
                                       (37, 53, 20, 29), (37, 53, 37, 29), (64, 48, 63, 47), (2, 300, 1, 150)])
@pytest.mark.parametrize("upsample", [0, 1])
def test_grey_resize_and_upsample(h, w, oh, ow, upsample):
    rs = np.random.RandomState(h * w + oh + ow)
    imgs = [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(2)]
    f = 2 if upsample else 1
    out = torch.empty((2, f * oh, f * ow), dtype=torch.float32, device="cuda")
    src = cuda(np.stack(imgs))
    call("vc_sift_grey", P(src), 2, h, w, oh, ow, upsample, P(out), S_())
    exps = []
    for b, img in enumerate(imgs):
        g = us.grey(img, size=(ow, oh))
        exps.append(us.upsample(g) if upsample else g)
        assert np.array_equal(out[b].cpu().numpy(), exps[-1]), f"image {b} differs"
    o1, buf = backed(f * f * oh * ow, torch.float32, SENTINEL_F32)
    call("vc_sift_grey", imgs[1], 1, h, w, oh, ow, upsample, P(o1), S_())
    assert np.array_equal(o1.cpu().numpy().reshape(f * oh, f * ow), exps[1])
    assert_tail(buf, f * f * oh * ow, SENTINEL_F32, "grey")


@pytest.mark.parametrize("h,w", [(2, 2), (3, 2), (7, 9), (9, 7), (65, 257), (131, 515)])
def test_downsample_odd_sizes(h, w):
    rs = np.random.RandomState(h + 7 * w)
    imgs = rs.rand(3, h, w).astype(F)
    out = torch.empty((3, h // 2, w // 2), dtype=torch.float32, device="cuda")
    call("vc_sift_downsample", imgs, 3, h, w, P(out), S_())
    exp = imgs[:, 0::2, 0::2][:, : h // 2, : w // 2]
    assert np.array_equal(out.cpu().numpy(), exp)
    n = (h // 2) * (w // 2)
    o1, buf = backed(n, torch.float32, SENTINEL_F32)
    call("vc_sift_downsample", imgs[2], 1, h, w, P(o1), S_())
    assert np.array_equal(o1.cpu().numpy().reshape(h // 2, w // 2), exp[2])
    assert_tail(buf, n, SENTINEL_F32, "downsample")


@pytest.mark.parametrize("L,B,h,w", [(n, 2, 13, 17) for n in range(4, 12)] + [(5, 2, 1024, 2100)])
def test_dog_levels_and_grid_stride(L, B, h, w):
    rs = np.random.RandomState(L)
    levels = rs.rand(L, B, h, w).astype(F)
    exp = levels[1:] - levels[:-1]
    if h * w > 1 << 20:
        assert exp.size > 65536 * 256             # more elements than one pass of the grid: the stride loop runs
    out = torch.empty((L - 1, B, h, w), dtype=torch.float32, device="cuda")
    lv = cuda(levels)
    call("vc_sift_dog", P(lv), L, B, h, w, P(out), S_())
    assert np.array_equal(out.cpu().numpy(), exp)
    n = (L - 1) * h * w
    o1, buf = backed(n, torch.float32, SENTINEL_F32)
    call("vc_sift_dog", levels[:, 1], L, 1, h, w, P(o1), S_())
    assert np.array_equal(o1.cpu().numpy().reshape(L - 1, h, w), exp[:, 1])
    assert_tail(buf, n, SENTINEL_F32, "dog")


# ---- vc_sift_detect ------------------------------------------------------------------------------------------------
def texture_grey(seed, h, w, sigma=2.0):
    rs = np.random.RandomState(seed)
    g = us.blur(rs.rand(h, w).astype(F), us.gaussian_taps(sigma))
    return ((g - g.min()) / (g.max() - g.min())).astype(F)


def texture_dogs(S, seeds=(1, 2), h=64, w=80):
    """First octave (o = -1) of the oracle pyramid of textures -> (levels (S+3, B, 2h, 2w), dog (S+2, B, 2h, 2w))."""
    pyr = [us.pyramid(texture_grey(s, h, w), S, -1, 1)[0] for s in seeds]
    return np.stack([p[1] for p in pyr], 1), np.stack([p[2] for p in pyr], 1)


def run_detect(dog, S, peak, edge, refine, cap):
    L, B, h, w = dog.shape
    d = cuda(dog)
    rows = torch.empty((B, S, h), dtype=torch.int32, device="cuda")
    kp = torch.full((B, cap, 8), SENTINEL_F32, dtype=torch.float32, device="cuda")
    count = torch.empty((B,), dtype=torch.int32, device="cuda")
    call("vc_sift_detect", P(d), B, h, w, L, float(peak), float(edge), refine, P(rows), cap, P(kp), P(count), S_())
    return kp.cpu().numpy(), count.cpu().numpy()


def assert_records_equal(got, exp, what):
    """Detection records: x, y, s, j, y0, x0 bit-exact; sigma = sigma0 exp2(s / S) within 2 ulp (exp2f against numpy)."""
    assert got.shape == exp.shape, f"{what}: {len(got)} records, the oracle has {len(exp)}"
    cols = [0, 1, 2, 4, 5, 6, 7]
    assert np.array_equal(got[:, cols], exp[:, cols]), f"{what}: records differ"
    assert np.all(np.abs(got[:, 3] - exp[:, 3]) <= 2.5e-7 * exp[:, 3]), f"{what}: sigma differs"


THRESHOLDS = [(PEAK, 10.0), (0.0, 10.0), (1e6, 10.0), (PEAK, 1.5), (PEAK, 50.0), (0.0, 1.5)]


@pytest.mark.parametrize("S", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("refine", [0, 1])
@pytest.mark.parametrize("peak,edge", THRESHOLDS)
def test_detect_textures_every_octave_resolution(S, refine, peak, edge):
    _, dog = texture_dogs(S)
    B = dog.shape[1]
    exps = [us.detect(dog[:, b], S, peak, edge, refine=bool(refine)) for b in range(B)]
    n_max = max(len(e) for e in exps)
    if peak < 1e6:
        assert n_max > 0
    kp, count = run_detect(dog, S, peak, edge, refine, max(n_max, 1))
    for b, exp in enumerate(exps):
        assert count[b] == len(exp)
        assert_records_equal(kp[b, : count[b]], exp, f"image {b}")
    if S >= 4 and refine and peak < 1e6:       # the acceptance sn <= S + 1 binds above sn = 4 only when S >= 4
        assert max(e[:, 2].max(initial=-2) for e in exps) > 4


def plant(h=24, w=40, L=5):
    """A DoG stack (S = L - 2) of zeros with planted structures on level j = 2 (one image) -> (dog, notes)."""
    d = np.zeros((L, h, w), F)
    # strict extrema on rows / columns 1 and h - 2 / w - 2, maxima and minima, with one lopsided neighbour each
    for k, (y, x) in enumerate([(1, 1), (1, w - 2), (h - 2, 1), (h - 2, w - 2), (1, 20), (h - 2, 9), (12, 1), (9, w - 2)]):
        sgn = 1 if k % 2 == 0 else -1
        d[2, y, x] = sgn * F(0.05 + 0.01 * k)
        d[2, y, x + (1 if x < w // 2 else -1)] = sgn * F(0.02)
        d[1, y, x] = sgn * F(0.01)
    # plateaus: equal neighbours in x, in y and across scale are not strict extrema
    d[2, 5, 8] = d[2, 5, 9] = F(0.07)
    d[2, 8, 14] = d[2, 9, 14] = F(-0.07)
    d[2, 15, 14] = d[3, 15, 14] = F(0.07)
    # a spike of 1e-12: its Hessian is below VLFeat's 1e-10 pivot limit, the step is zero
    d[2, 4, 28] = F(1e-12)
    # a narrow ridge along (2, 1) in (x, y) whose peak lies 1.4 px from the sampled maximum: inside, Newton moves the
    # point; against the right border (x = w - 2) the move is refused and the offset leaves the octave.  The blocks
    # border on zeros, which makes a few more extrema at their edges
    for (y0, x0) in [(16, 24), (15, w - 2)]:
        for y in range(max(y0 - 2, 0), min(y0 + 3, h)):
            for x in range(max(x0 - 2, 0), min(x0 + 3, w)):
                for j in (1, 2, 3):
                    u, v = (x - x0) - 1.3, (y - y0) - 0.55      # position relative to the peak
                    along = (2 * u + v) / math.sqrt(5)
                    across = (-u + 2 * v) / math.sqrt(5)
                    d[j, y, x] = F(0.2 - 0.01 * along ** 2 - 0.3 * across ** 2 - 0.1 * (j - 2) ** 2)
    return d


def test_detect_planted_borders_plateaus_singular_and_newton_paths():
    d0 = plant()
    d1 = -plant()[:, ::-1].copy()                         # the second image: mirrored, extrema swapped
    dog = np.stack([d0, d1], 1)
    S = 3
    h, w = d0.shape[1:]
    raw = us._extrema(d0, S, us.prefilter_of(0.0))
    pos = {(int(j), int(y), int(x)) for j, y, x in raw}
    for y, x in [(1, 1), (1, w - 2), (h - 2, 1), (h - 2, w - 2), (12, 1), (9, w - 2)]:
        assert (2, y, x) in pos                           # border extrema are found by the spec
    for y, x in [(5, 8), (5, 9), (8, 14), (9, 14)]:
        assert (2, y, x) not in pos                       # plateaus are not
    assert (2, 15, 14) not in pos and (3, 15, 14) not in pos
    acc = us.detect(d0, S, 0.0, 10.0)
    tiny = acc[(acc[:, 5] == 4) & (acc[:, 6] == 28)]
    assert len(tiny) == 1 and tiny[0, 0] == 28 and tiny[0, 1] == 4 and tiny[0, 2] == 1   # singular: offsets zero
    # the ridges fail the edge test at 10; with the edge test out of the way (1e4) the inner one moves one pixel and is
    # kept, the one against the border cannot move and its offset leaves the octave
    assert not ((acc[:, 5] == 16) & (acc[:, 6] == 24)).any()
    acc = us.detect(d0, S, 0.0, 1e4)
    inner = acc[(acc[:, 5] == 16) & (acc[:, 6] == 24)]
    assert len(inner) == 1 and inner[0, 0] > 25 and inner[0, 1] < 17
    assert (2, 15, w - 2) in pos and not ((acc[:, 5] == 15) & (acc[:, 6] == w - 2)).any()
    for peak, edge in [(0.0, 10.0), (PEAK, 10.0), (0.0, 1.5), (0.0, 1e4)]:
        for refine in (0, 1):
            exps = [us.detect(dog[:, b], S, peak, edge, refine=bool(refine)) for b in range(2)]
            kp, count = run_detect(dog, S, peak, edge, refine, 64)
            for b in range(2):
                assert count[b] == len(exps[b]) > 0
                assert_records_equal(kp[b, : count[b]], exps[b], f"image {b}, peak {peak}, refine {refine}")


@pytest.mark.parametrize("value", [0.0, 0.25])
def test_detect_flat_stack_finds_nothing(value):
    dog = np.full((5, 2, 16, 20), value, F)
    kp, count = run_detect(dog, 3, 0.0, 10.0, 1, 8)
    assert count.tolist() == [0, 0]
    assert np.all(kp == F(SENTINEL_F32))


@pytest.mark.parametrize("S", [2, 3])
def test_detect_cap_writes_the_first_rows_and_counts_all(S):
    _, dog = texture_dogs(S, seeds=(5, 6))
    L, B, h, w = dog.shape
    exps = [us.detect(dog[:, b], S, PEAK, 10.0) for b in range(B)]
    N = min(len(e) for e in exps)
    assert N >= 9
    for cap in (1, N // 3):
        kp, count = run_detect(dog, S, PEAK, 10.0, 1, cap)
        for b, exp in enumerate(exps):
            assert count[b] == len(exp)                      # the full total, though only cap rows fit
            assert_records_equal(kp[b], exp[:cap], f"image {b}, cap {cap}")
        # B = 1: the rows behind cap are not touched
        d = cuda(dog[:, 1])
        rows = torch.empty((1, S, h), dtype=torch.int32, device="cuda")
        out, buf = backed(cap * 8, torch.float32, SENTINEL_F32)
        cnt = torch.empty((1,), dtype=torch.int32, device="cuda")
        call("vc_sift_detect", P(d), 1, h, w, L, PEAK, 10.0, 1, P(rows), cap, P(out), P(cnt), S_())
        assert int(cnt[0]) == len(exps[1])
        assert_records_equal(out.cpu().numpy().reshape(cap, 8), exps[1][:cap], f"B = 1, cap {cap}")
        assert_tail(buf, cap * 8, SENTINEL_F32, "detect keypoints")
    # the driver relaunches with a larger cap until every keypoint fits
    oc = types.SimpleNamespace(dog=cuda(dog))
    kp, count, n = se._detect(oc, S, SiftOptions(octave_resolution=S), cap=1)
    assert n.tolist() == [len(e) for e in exps] and kp.shape[1] >= max(n.tolist())
    for b, exp in enumerate(exps):
        assert_records_equal(kp[b, : len(exp)].cpu().numpy(), exp, f"_detect, image {b}")


# ---- vc_sift_orient ------------------------------------------------------------------------------------------------
def polygon_roof(h, w, cx, cy, k, phase):
    """-max_i <(x, y) - c, n_i> over k unit normals at phase + 2 pi i / k (k = 1: a plane, k = 2: a V): continuous,
    piecewise linear, one gradient direction per facet and facets of equal angular size -> k histogram peaks."""
    yy, xx = np.mgrid[:h, :w].astype(np.float64)
    th = phase + 2 * np.pi * np.arange(k) / k
    proj = (xx[..., None] - cx) * np.cos(th) + (yy[..., None] - cy) * np.sin(th)
    return (-0.01 * proj.max(-1)).astype(F)


def orient_oracle(level, rec, max_ori, upright):
    if upright:
        return [F(0)]
    mod, ang = us.gradient(level)
    return us.orientations(mod, ang, rec)[:max_ori]


def run_orient(levels, kp, count, cap, max_ori, upright):
    L, B, h, w = levels.shape
    angles = torch.full((B, cap, 4), SENTINEL_F32, dtype=torch.float32, device="cuda")
    n_angles = torch.full((B, cap), SENTINEL_I32, dtype=torch.int32, device="cuda")
    call("vc_sift_orient", levels, L, B, h, w, kp, count, cap, max_ori, upright, P(angles),
         P(n_angles), S_())
    return angles.cpu().numpy(), n_angles.cpu().numpy()


def record(x, y, sigma, j):
    return np.array([x, y, 0, sigma, j, round(y), round(x), 0], F)


def crafted_orient_case():
    """Levels (6, 2, 48, 64) and records whose full peak counts cover 0 .. 6, plus border and oversized windows."""
    h, w, L = 48, 64, 6
    rs = np.random.RandomState(3)
    levels = np.stack([texture_grey(40 + l, h, w) for l in range(2 * L)]).reshape(L, 2, h, w)
    recs = [[], []]
    levels[1, 0] = 0.5                                            # a flat level: no peak at all
    recs[0].append(record(20.3, 30.6, 2.5, 1))
    for k in range(1, 7):                                         # one polygon roof per level and image
        b, j = k % 2, 1 + k // 2
        cx, cy = 31.7 + 0.1 * k, 23.4 - 0.1 * k
        levels[j, b] = polygon_roof(h, w, cx, cy, k, 0.05 + 0.3 * k)
        recs[b].append(record(cx, cy, 3.0, j))
    for b in range(2):                                            # the border, and windows wider than the image
        for x, y, s in [(0, 20, 2.0), (w - 1, 17, 2.5), (30, 0, 1.7), (11, h - 1, 3.3), (0, 0, 4.0), (w - 1, h - 1, 2.2),
                        (31.5, 24.2, 20.0), (5.4, 40.1, 35.0)]:
            recs[b].append(record(x, y, s, 4))
        for _ in range(20):
            recs[b].append(record(rs.uniform(0, w - 1), rs.uniform(0, h - 1), rs.uniform(1.0, 6.0), 4 + rs.randint(2)))
    return levels, recs


def test_orient_crafted_peak_counts_cover_zero_to_five_and_more():
    levels, recs = crafted_orient_case()
    seen = set()
    for b in range(2):
        for rec in recs[b][:4]:
            mod, ang = us.gradient(levels[int(rec[4]), b])
            seen.add(min(len(us.orientations(mod, ang, rec, max_peaks=36)), 5))
    assert seen == {0, 1, 2, 3, 4, 5}, seen


@pytest.mark.parametrize("max_ori", [1, 2, 3, 4])
@pytest.mark.parametrize("upright", [0, 1])
def test_orient_crafted_and_border_records(max_ori, upright):
    levels, recs = crafted_orient_case()
    cap = max(len(r) for r in recs) + 3
    kp = np.zeros((2, cap, 8), F)
    for b in range(2):
        kp[b, : len(recs[b])] = recs[b]
    count = np.array([len(r) for r in recs], np.int32)
    angles, n_angles = run_orient(levels, kp, count, cap, max_ori, upright)
    for b in range(2):
        for k, rec in enumerate(recs[b]):
            exp = orient_oracle(levels[int(rec[4]), b], rec, max_ori, upright)
            assert n_angles[b, k] == len(exp), (b, k, rec)
            got = angles[b, k, : len(exp)]
            assert np.all(np.abs(got - np.array(exp, F)) <= 1e-3), (b, k, got, exp)
        assert np.all(n_angles[b, len(recs[b]):] == SENTINEL_I32)       # records past count are not processed


@pytest.mark.parametrize("max_ori", [1, 2, 3, 4])
def test_orient_detected_records_on_textures(max_ori):
    S = 3
    levels, dog = texture_dogs(S, seeds=(8, 9), h=96, w=128)
    exps = [us.detect(dog[:, b], S, PEAK, 10.0) for b in range(2)]
    cap = max(len(e) for e in exps)
    kp = np.zeros((2, cap, 8), F)
    for b, e in enumerate(exps):
        kp[b, : len(e)] = e
    count = np.array([len(e) for e in exps], np.int32)
    angles, n_angles = run_orient(levels, kp, count, cap, max_ori, 0)
    same = total = 0
    for b, e in enumerate(exps):
        grads = {j: us.gradient(levels[j, b]) for j in range(1, S + 1)}
        for k, rec in enumerate(e):
            exp = us.orientations(*grads[int(rec[4])], rec)[:max_ori]
            total += 1
            if n_angles[b, k] == len(exp):
                same += 1
                assert np.all(np.abs(angles[b, k, : len(exp)] - np.array(exp, F)) <= 1e-3), (b, k)
    assert total > 100 and same >= 0.995 * total, (same, total)


def test_orient_count_above_cap_processes_cap_records():
    levels, recs = crafted_orient_case()
    L, _, h, w = levels.shape
    cap = 12
    kp = np.zeros((cap, 8), F)
    kp[:] = recs[1][:cap]
    k_buf = cuda(np.concatenate([kp, np.tile(kp[:1], (TAIL, 1))]))    # valid records behind cap too
    for upright in (0, 1):
        angles, abuf = backed(cap * 4, torch.float32, SENTINEL_F32)
        n_angles, nbuf = backed(cap, torch.int32, SENTINEL_I32)
        count = torch.tensor([cap + 40], dtype=torch.int32, device="cuda")
        call("vc_sift_orient", levels[:, 1], L, 1, h, w, P(k_buf), P(count), cap, 4, upright, P(angles),
             P(n_angles), S_())
        assert_tail(abuf, cap * 4, SENTINEL_F32, "orient angles")
        assert_tail(nbuf, cap, SENTINEL_I32, "orient n_angles")
        got = n_angles.cpu().numpy()
        for k in range(cap):
            assert got[k] == len(orient_oracle(levels[int(kp[k, 4]), 1], kp[k], 4, upright))


# ---- vc_sift_describe ----------------------------------------------------------------------------------------------
def describe_case(seed):
    """Levels (6, 2, 72, 96), records from detection plus border records, random angles and n_angles in 0 .. 4."""
    S = 3
    levels, dog = texture_dogs(S, seeds=(seed, seed + 1), h=36, w=48)
    L, B, h, w = levels.shape
    rs = np.random.RandomState(seed)
    recs = []
    for b in range(B):
        r = list(us.detect(dog[:, b], S, PEAK, 10.0)[:40])
        for x, y in [(0, 30), (w - 1, 11), (40, 0), (7, h - 1), (0, 0), (w - 1, h - 1), (1, 1), (w - 2, h - 2)]:
            r.append(record(x, y, rs.uniform(1.5, 4.0), 1 + rs.randint(S)))
        recs.append(np.array(r, F))
    cap = max(len(r) for r in recs) + 5
    kp = np.zeros((B, cap, 8), F)
    angles = rs.uniform(0, 2 * np.pi, (B, cap, 4)).astype(F)
    n_angles = np.zeros((B, cap), np.int32)
    for b in range(B):
        kp[b, : len(recs[b])] = recs[b]
        n_angles[b] = rs.randint(0, 5, cap)
        n_angles[b, :5] = [0, 1, 2, 3, 4]
    count = np.array([len(r) for r in recs], np.int32)
    return levels, kp, count, cap, angles, n_angles


def describe_oracle(levels, kp, count, angles, n_angles, norm, oct_scale, sx, sy):
    """-> per image (rows (N, 6), desc (N, 128)) in keypoint order, as extract_grey builds them."""
    out = []
    for b in range(kp.shape[0]):
        grads = {}
        r, d = [], []
        for k in range(count[b]):
            rec = kp[b, k]
            j = int(rec[4])
            if j not in grads:
                grads[j] = us.gradient(levels[j, b])
            for o in range(n_angles[b, k]):
                a = angles[b, k, o]
                d.append(us.quantize(us.descriptor(*grads[j], rec, a, norm)))
                r.append((rec[0], rec[1], rec[3], a))
        r = np.array(r, F).reshape(-1, 4)
        k = F(oct_scale)
        aff = us.affine_rows(r[:, 0] * k, r[:, 1] * k, r[:, 2] * k, r[:, 3])
        aff[:, [0, 2, 3]] *= F(sx)
        aff[:, [1, 4, 5]] *= F(sy)
        out.append((aff, np.array(d, np.uint8).reshape(-1, 128)))
    return out


def assert_rows_match(g_rows, g_desc, o_rows, o_desc, what):
    assert np.array_equal(g_rows[:, :2], o_rows[:, :2]), f"{what}: x, y differ"     # the same float32 operations
    s = np.hypot(o_rows[:, 2], o_rows[:, 4])[:, None]
    assert np.all(np.abs(g_rows[:, 2:] - o_rows[:, 2:]) <= 1e-5 * s), f"{what}: affine columns differ"
    diff = g_desc.astype(np.int32) - o_desc.astype(np.int32)
    assert np.abs(diff).max(initial=0) <= 1, f"{what}: a descriptor byte differs by more than 1"
    assert (diff == 0).mean() >= 0.99, f"{what}: {(diff == 0).mean():.4f} of descriptor bytes equal"


@pytest.mark.parametrize("norm", ["L1_ROOT", "L2"])
@pytest.mark.parametrize("oct_scale,sx,sy", [(1.0, 1.0, 1.0), (0.5, 1.25, 0.8), (8.0, 0.75, 1.5)])
def test_describe_rows_offsets_and_scales(norm, oct_scale, sx, sy):
    levels, kp, count, cap, angles, n_angles = describe_case(13)
    L, B, h, w = levels.shape
    row_cap = cap * 4
    rows = torch.full((B, row_cap, 6), SENTINEL_F32, dtype=torch.float32, device="cuda")
    desc = torch.full((B, row_cap, 128), SENTINEL_U8, dtype=torch.uint8, device="cuda")
    rcount = torch.empty((B,), dtype=torch.int32, device="cuda")
    offs = torch.empty((B, cap), dtype=torch.int32, device="cuda")
    call("vc_sift_describe", levels, L, B, h, w, kp, count, cap, angles,
         n_angles, 4, se.NORMALIZATIONS[norm], oct_scale, sx, sy, P(offs), row_cap, P(rows), P(desc), P(rcount),
         S_())
    rows, desc, rcount = rows.cpu().numpy(), desc.cpu().numpy(), rcount.cpu().numpy()
    exp = describe_oracle(levels, kp, count, angles, n_angles, norm, oct_scale, sx, sy)
    for b, (o_rows, o_desc) in enumerate(exp):
        n = int(rcount[b])
        assert n == len(o_rows) == n_angles[b, : count[b]].sum()
        assert_rows_match(rows[b, :n], desc[b, :n], o_rows, o_desc, f"image {b}")
        assert np.all(rows[b, n:] == F(SENTINEL_F32)) and np.all(desc[b, n:] == SENTINEL_U8)
    # B = 1 into backed buffers with row_cap = cap * 4 exactly: nothing behind row_cap
    r1, rbuf = backed(row_cap * 6, torch.float32, SENTINEL_F32)
    d1, dbuf = backed(row_cap * 128, torch.uint8, SENTINEL_U8)
    c1 = torch.empty((1,), dtype=torch.int32, device="cuda")
    call("vc_sift_describe", levels[:, 1], L, 1, h, w, kp[1], count[1:], cap,
         angles[1], n_angles[1], 4, se.NORMALIZATIONS[norm], oct_scale, sx, sy, P(offs), row_cap,
         P(r1), P(d1), P(c1), S_())
    n = int(c1[0])
    assert n == int(rcount[1])
    assert np.array_equal(r1.cpu().numpy().reshape(row_cap, 6)[:n], rows[1, :n])
    assert np.array_equal(d1.cpu().numpy().reshape(row_cap, 128)[:n], desc[1, :n])
    assert_tail(rbuf, row_cap * 6, SENTINEL_F32, "describe rows")
    assert_tail(dbuf, row_cap * 128, SENTINEL_U8, "describe descriptors")


def test_describe_count_above_cap_and_normalisations_differ():
    levels, kp, count, cap, angles, n_angles = describe_case(17)
    L, B, h, w = levels.shape
    n_angles[:, :] = np.minimum(n_angles, 2)
    k_cap = int(count.min()) - 3                           # count > cap: only the first cap records make rows
    kp_c = np.ascontiguousarray(kp[:, :k_cap])
    out = {}
    for norm in ("L1_ROOT", "L2"):
        rows = torch.full((B, k_cap * 2, 6), SENTINEL_F32, dtype=torch.float32, device="cuda")
        desc = torch.full((B, k_cap * 2, 128), SENTINEL_U8, dtype=torch.uint8, device="cuda")
        rcount = torch.empty((B,), dtype=torch.int32, device="cuda")
        offs = torch.empty((B, k_cap), dtype=torch.int32, device="cuda")
        call("vc_sift_describe", levels, L, B, h, w, kp_c, count, k_cap,
             angles[:, :k_cap], n_angles[:, :k_cap], 2,
             se.NORMALIZATIONS[norm], 2.0, 1.0, 1.0, P(offs), k_cap * 2, P(rows), P(desc), P(rcount), S_())
        exp = describe_oracle(levels, kp_c, np.full(B, k_cap), angles[:, :k_cap], n_angles[:, :k_cap], norm, 2.0, 1, 1)
        rows, desc, rcount = rows.cpu().numpy(), desc.cpu().numpy(), rcount.cpu().numpy()
        for b, (o_rows, o_desc) in enumerate(exp):
            assert rcount[b] == len(o_rows)
            assert_rows_match(rows[b, : rcount[b]], desc[b, : rcount[b]], o_rows, o_desc, f"{norm}, image {b}")
        out[norm] = desc[0, : rcount[0]]
    assert not np.array_equal(out["L1_ROOT"], out["L2"])
