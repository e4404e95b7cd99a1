"""csrc/detect.hip against its numpy specification (tests/util_detect.py): FAST and GFTT must equal it exactly — points,
their order and the counts — across sizes, batch sizes and limits, and refuse what they do not cover."""
import functools

import numpy as np
import pytest

import util_detect as ud
from test_host_logic import checkerboard

pytestmark = pytest.mark.gpu

SIZES = [(640, 480), (333, 217)]
LIMITS = [8, 128, 2048]


@functools.lru_cache(maxsize=None)
def slot_image(w, h, slot):
    """The image of batch slot `slot`: every slot differs.  0: noise amplitude 40 (the e2e helper's); 1: rotated
    rectangles, +-3 noise; 2: uniform (nothing to find; GFTT's max <= 0 branch); 3: amplitude 20; then alternating."""
    if slot == 1:
        return ud.rectangles(w, h)
    if slot == 2:
        return np.full((h, w, 3), 93, np.uint8)
    return ud.noisy_checkerboard(slot, w, h, amp=20 if slot % 2 else 40)


@functools.lru_cache(maxsize=None)
def fast_spec(w, h, slot, limit):
    xy, total, _ = ud.fast_detect(ud.grey_u8(slot_image(w, h, slot)), 10, limit)
    return xy, total


@functools.lru_cache(maxsize=None)
def gftt_spec(w, h, slot, limit):
    return ud.gftt_detect(ud.grey_u8(slot_image(w, h, slot)), limit)


def _batch(w, h, B):
    import torch

    return torch.from_numpy(np.stack([slot_image(w, h, s) for s in range(B)])).cuda()


def _check(got_xy, got_count, got_aux, specs, limit):
    xy, count, aux = (t.cpu().numpy() for t in (got_xy, got_count, got_aux))
    assert xy.shape == (len(specs), limit, 2) and xy.dtype == np.float32
    for b, (want, want_aux) in enumerate(specs):
        assert aux[b] == want_aux, (b, aux[b], want_aux)
        assert count[b] == len(want), (b, count[b], len(want))
        assert np.array_equal(xy[b, :count[b]], want), b          # the points AND their order
        assert not xy[b, count[b]:].any()


@pytest.mark.parametrize("limit", LIMITS)
@pytest.mark.parametrize("B", [1, 3, 16])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_fast_equals_the_specification(size, B, limit):
    from vit_colmap_amd.features import hip_detect

    w, h = size
    specs = [fast_spec(w, h, s, limit) for s in range(B)]
    if size == (640, 480) and B >= 4:
        # a condition on the inputs, not a measurement: both sides of every limit are exercised
        totals = [t for _, t in specs]
        assert totals[2] == 0 and 8 < totals[1] < 128 < totals[3] < 2048 < totals[0], totals
    _check(*hip_detect.fast(_batch(w, h, B), limit, threshold=10), specs, limit)


@pytest.mark.parametrize("limit", LIMITS)
@pytest.mark.parametrize("B", [1, 3, 16])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_gftt_equals_the_specification(size, B, limit):
    from vit_colmap_amd.features import hip_detect

    w, h = size
    specs = [gftt_spec(w, h, s, limit) for s in range(B)]
    if size == (640, 480) and B >= 4:
        free = [len(gftt_spec(w, h, s, 2048)[0]) for s in range(B)]
        assert free[2] == 0 and specs[2][1] == 0 and all(128 < n < 2048 for n in free[:2] + free[3:]), free
    _check(*hip_detect.gftt(_batch(w, h, B), limit), specs, limit)


def test_fast_limit_cuts_through_tied_scores_on_the_device():
    """Over 2 000 of the 2 048 kept points of the amplitude-40 image share their score with another kept point."""
    _, _, sc = ud.fast_detect(ud.grey_u8(slot_image(640, 480, 0)), 10, 2048)
    values, counts = np.unique(sc, return_counts=True)
    assert counts[counts > 1].sum() > 2000
    _, _, sc_all = ud.fast_detect(ud.grey_u8(slot_image(640, 480, 0)), 10, 1 << 30)
    assert (sc_all == sc.min()).sum() > (sc == sc.min()).sum() > 0      # the cut falls inside a run of equal scores


def test_real_corners_not_only_noise():
    from vit_colmap_amd.features import hip_detect

    fxy, ftotal = fast_spec(640, 480, 1, 2048)
    gxy, gcand = gftt_spec(640, 480, 1, 2048)
    assert 10 <= ftotal <= 60 and 60 <= len(gxy) <= 400, (ftotal, len(gxy))
    batch = _batch(640, 480, 2)[1:]
    _check(*hip_detect.fast(batch, 2048), [(fxy, ftotal)], 2048)
    _check(*hip_detect.gftt(batch, 2048), [(gxy, gcand)], 2048)


def test_gftt_ties_and_candidate_overflow():
    """A pure checkerboard: 5 940 candidates, nearly all with a value shared by another one, so the order among equal
    lambda decides; and a candidate list that starts too small is grown, never cut short."""
    import torch

    from vit_colmap_amd.features import hip_detect

    img = checkerboard()
    want, n_cand = ud.gftt_detect(ud.grey_u8(img), 2048)
    assert n_cand == 5940 and len(want) == 330
    batch = torch.from_numpy(np.stack([img, slot_image(640, 480, 0)])).cuda()
    specs = [(want, n_cand), gftt_spec(640, 480, 0, 2048)]
    _check(*hip_detect.gftt(batch, 2048, cand_cap=8192), specs, 2048)
    _check(*hip_detect.gftt(batch, 2048, cand_cap=100), specs, 2048)          # 100 -> 5 940: one repeat
    # at the ABI: the count reports the overflow, the image that overflowed gets no points, the other one is complete
    lib, _lib = hip_detect._lib.load(), hip_detect._lib
    cap = 1024
    nbytes = lib.vc_detect_gftt_workspace_bytes(2, 480, 640, cap)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    xy = torch.empty((2, 2048, 2), dtype=torch.float32, device="cuda")
    cnt, cand = (torch.empty(2, dtype=torch.int32, device="cuda") for _ in range(2))
    st = lib.vc_detect_gftt(_lib.ptr(batch), 2, 480, 640, 0.01, 7, 7, 2048, cap, _lib.ptr(ws), nbytes, _lib.ptr(xy), _lib.ptr(cnt),
                            _lib.ptr(cand), _lib.stream_ptr())
    assert st == 0 and cand.tolist() == [5940, specs[1][1]] and cnt.tolist() == [0, len(specs[1][0])]
    assert np.array_equal(xy[1, :cnt[1]].cpu().numpy(), specs[1][0])


@pytest.mark.parametrize("block_size", [3, 5])
def test_gftt_other_windows(block_size):
    from vit_colmap_amd.features import hip_detect

    batch = _batch(333, 217, 2)
    specs = [ud.gftt_detect(ud.grey_u8(slot_image(333, 217, s)), 300, 0.05, 4, block_size) for s in range(2)]
    _check(*hip_detect.gftt(batch, 300, quality_level=0.05, min_distance=4, block_size=block_size), specs, 300)


def test_smallest_size():
    import torch

    from vit_colmap_amd.features import hip_detect

    rs = np.random.RandomState(11)
    imgs = rs.randint(0, 256, (5, 8, 8, 3)).astype(np.uint8)
    imgs[1] = 10
    imgs[1, 3:5, 3:5] = 250                                   # a blob in the 2x2 pixels where FAST can fire at all
    imgs[2] = 40
    imgs[2, 4, 4] = 255
    batch = torch.from_numpy(imgs).cuda()
    fspecs = [ud.fast_detect(ud.grey_u8(i), 10, 8)[:2] for i in imgs]
    gspecs = [ud.gftt_detect(ud.grey_u8(i), 8) for i in imgs]
    assert sum(t for _, t in fspecs) > 0 and sum(len(x) for x, _ in gspecs) > 0
    _check(*hip_detect.fast(batch, 8), fspecs, 8)
    _check(*hip_detect.gftt(batch, 8), gspecs, 8)


def test_refusals_at_the_abi_and_in_the_wrappers(monkeypatch):
    import torch

    from vit_colmap_amd import _lib
    from vit_colmap_amd.features import hip_detect

    lib = _lib.load()
    img = torch.zeros((1, 16, 16, 3), dtype=torch.uint8, device="cuda")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    xy = torch.empty((1, 8, 2), dtype=torch.float32, device="cuda")
    a, b = (torch.empty(1, dtype=torch.int32, device="cuda") for _ in range(2))
    P, S = _lib.ptr, _lib.stream_ptr

    def fast(images=img, n=1, h=16, w=16, thr=10, k=8, wsp=ws, nbytes=ws.numel(), out=xy):
        return lib.vc_detect_fast(P(images), n, h, w, thr, k, P(wsp), nbytes, P(out), P(a), P(b), S())

    def gftt(images=img, n=1, h=16, w=16, q=0.01, md=7, bs=7, k=8, cap=64, wsp=ws, nbytes=ws.numel(), out=xy):
        return lib.vc_detect_gftt(P(images), n, h, w, q, md, bs, k, cap, P(wsp), nbytes, P(out), P(a), P(b), S())

    assert fast() == 0 and gftt() == 0
    for f in (fast, gftt):
        assert f(images=None) == -1 and f(wsp=None) == -1 and f(out=None) == -1
        assert f(n=-1) == -1 and f(h=-3) == -1 and f(w=0) == -1 and f(k=0) == -1
        assert f(h=7, w=640) == -2 and f(h=640, w=7) == -2            # VC_ERR_UNSUPPORTED: under 8 pixels
        assert f(nbytes=16) == -4                                      # VC_ERR_WORKSPACE
    assert fast(thr=-1) == -1 and fast(thr=255) == -1
    assert gftt(q=0.0) == -1 and gftt(md=0) == -1 and gftt(cap=0) == -1
    assert gftt(bs=9) == -2 and gftt(bs=4) == -2 and gftt(cap=16385) == -2
    assert lib.vc_detect_fast_workspace_bytes(1, 7, 640) == 0 and lib.vc_detect_gftt_workspace_bytes(1, 480, 640, 16385) == 0
    torch.cuda.synchronize()

    with pytest.raises(_lib.HipLibraryError):
        hip_detect.fast(img.cpu(), 8)
    with pytest.raises(_lib.HipLibraryError):
        hip_detect.gftt(img.cpu(), 8)

    class NoLaunch:
        def __getattr__(self, name):
            raise AssertionError(f"{name} called for an image the kernels do not cover")

    monkeypatch.setattr(_lib, "load", lambda: NoLaunch())
    small = torch.zeros((2, 7, 640, 3), dtype=torch.uint8, device="cuda")
    for fn in (hip_detect.fast, hip_detect.gftt):
        pts, count, aux = fn(small, 8)
        assert pts.shape == (2, 8, 2) and count.tolist() == [0, 0] and aux.tolist() == [0, 0]
