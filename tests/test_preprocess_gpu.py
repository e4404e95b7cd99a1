"""vc_preprocess_u8 (csrc/preprocess.hip) against oracle/preprocess_oracle.py at many sizes, through the C ABI.

For every (h, w) -> (out_h, out_w): the resized uint8 frame equals `resize_linear_u8` bit for bit; float32 NCHW is within
rtol 1e-6 / atol 1e-6 of the oracle's normalisation; float32 patches equal `patchify` of the device's own NCHW exactly;
bf16 outputs equal the round-to-nearest-even cast of the float32 ones exactly; and the padded-patch kernel (bf16,
VC_LAYOUT_PATCHES_PAD, no debug frame, aligned output) equals the bf16 patches with zeros in elements 588..639 of a
buffer pre-filled with a sentinel.  The entry's fall-back (misaligned output or a requested debug frame -> the generic
kernel writes the padded layout) gives the same bits.
"""
import numpy as np
import pytest
import torch

from oracle import preprocess_oracle as po
from util_select import patch_windows_fit

gpu = pytest.mark.gpu          # per test: the check of the size list below needs no GPU

NCHW, PATCHES, PATCHES_PAD = 0, 1, 2
F32_CODE, BF16_CODE = 0, 1
K, KPAD = 588, 640

# (h, w, out_h, out_w, images per call, how the patches' source windows sit against the padded kernel's LDS staging)
SIZES = [
    # the product's rule: floor to multiples of 14
    (14, 14, 14, 14, 2, "fit"),            # no resize, one patch
    (27, 27, 14, 14, 2, "global"),         # one patch over 27 source rows: taller than the 24-row window
    (15, 41, 14, 28, 3, "fit"),
    (28, 14, 28, 14, 2, "fit"),
    # 5 images of 63933 resp. 64581 bytes (1 mod 4): the images start at byte offsets 0, 1, 2, 3, 0 mod 4 and the batch's
    # byte count is not a multiple of 4, so the window of its last patch ends in the byte-tail branch
    (101, 211, 98, 210, 5, "fit"),
    (103, 209, 98, 196, 5, "fit"),
    (480, 640, 476, 630, 2, "fit"),
    (1080, 1920, 1078, 1918, 1, "fit"),
    (1200, 1600, 1190, 1596, 1, "fit"),
    # arbitrary targets, which only the ABI offers
    (480, 640, 14, 14, 2, "global"),
    (480, 640, 56, 84, 2, "global"),
    (480, 640, 140, 98, 2, "global"),
    (480, 640, 966, 1274, 1, "fit"),       # up-scaling: source coordinates below 0 clamp
    (24, 30, 14, 14, 5, "fit"),            # a window of exactly 24 rows x 96 bytes: the largest that is staged
    (25, 31, 14, 14, 5, "global"),         # one row and one pixel more
    (47, 153, 28, 70, 3, "mixed"),         # patch columns alternate between 30 and 31 source pixels: both branches in one launch
]
IDS = [f"{h}x{w}-{oh}x{ow}" for h, w, oh, ow, _, _ in SIZES]


def _images(seed, B, h, w):
    rs = np.random.RandomState(seed)
    img = rs.randint(0, 256, (B, h, w, 3)).astype(np.int32)
    ramp = (np.arange(w)[None, :, None] * 255 // max(w - 1, 1) + np.arange(h)[:, None, None] * 3) % 256
    img[B // 2] = (img[B // 2] // 4 + ramp) % 256                   # one structured frame among the noise
    return img.astype(np.uint8)


def _call(d, oh, ow, dtype_code, layout, out, dbg=None):
    from vit_colmap_amd import _lib

    B, h, w, _ = d.shape
    st = _lib.load().vc_preprocess_u8(_lib.ptr(d), B, h, w, oh, ow, dtype_code, layout, _lib.ptr(out), _lib.ptr(dbg), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert st == 0, st
    return out


def _empty(shape, dtype, fill):
    return torch.full(shape, fill, dtype=dtype, device="cuda")


def test_size_list_reaches_both_window_branches():
    """`use_win` restated with the oracle's own coefficients: the list holds sizes whose patches are all staged in LDS,
    sizes whose patches all read their taps from global memory, and one with both kinds in the same launch."""
    seen = set()
    for h, w, oh, ow, _, kind in SIZES:
        fit = patch_windows_fit(h, w, oh, ow)
        assert fit.shape == (oh // 14, ow // 14)
        got = "fit" if fit.all() else "global" if not fit.any() else "mixed"
        assert got == kind, (h, w, oh, ow, got)
        seen.add(got)
    assert seen == {"fit", "global", "mixed"}
    assert (101 * 211 * 3) % 4 == 1 and (103 * 209 * 3) % 4 == 1 and (5 * 101 * 211 * 3) % 4 != 0
    y0, y1, _, _ = po._coefs(14, 24)
    x0, x1, _, _ = po._coefs(14, 30)
    assert y1[-1] - y0[0] + 1 == 24 and 3 * (x1[-1] - x0[0] + 1) + 6 == 96        # the boundary case is the boundary


@gpu
@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_preprocess_against_oracle(size):
    h, w, oh, ow, B, _ = size
    imgs = _images(h * 10000 + w + oh, B, h, w)
    d = torch.from_numpy(imgs).cuda()
    assert d.data_ptr() % 4 == 0
    P = (oh // 14) * (ow // 14)

    resized = _empty((B, oh, ow, 3), torch.uint8, 0)
    nchw = _call(d, oh, ow, F32_CODE, NCHW, _empty((B, 3, oh, ow), torch.float32, -7.0), resized).cpu().numpy()
    resized = resized.cpu().numpy()
    for b in range(B):
        ref = po.resize_linear_u8(imgs[b], oh, ow)
        assert np.array_equal(resized[b], ref), (size, b)                                         # uint8 resize: bit-exact
        rgb = ref[:, :, ::-1].astype(np.float32) / np.float32(255.0)                              # preprocess_oracle.preprocess
        x = ((rgb - po.MEAN) / po.STD).astype(np.float32).transpose(2, 0, 1)
        np.testing.assert_allclose(nchw[b], x, rtol=1e-6, atol=1e-6)
    if (oh, ow) == ((h // 14) * 14, (w // 14) * 14):                                              # the product's rule: the oracle's entry
        x0, r0 = po.preprocess(imgs[0])
        assert np.array_equal(r0, resized[0])
        np.testing.assert_allclose(nchw[0], x0, rtol=1e-6, atol=1e-6)

    patches = _call(d, oh, ow, F32_CODE, PATCHES, _empty((B, P, K), torch.float32, -7.0))
    for b in range(B):
        assert np.array_equal(patches[b].cpu().numpy(), po.patchify(nchw[b])), (size, b)
    nchw16 = _call(d, oh, ow, BF16_CODE, NCHW, _empty((B, 3, oh, ow), torch.bfloat16, -7.0))
    assert torch.equal(nchw16, torch.from_numpy(nchw).cuda().to(torch.bfloat16))                  # RN-even cast
    p16 = _call(d, oh, ow, BF16_CODE, PATCHES, _empty((B, P, K), torch.bfloat16, -7.0))
    assert torch.equal(p16, patches.to(torch.bfloat16))

    pad = _empty((B, P, KPAD), torch.bfloat16, 7.0)
    assert pad.data_ptr() % 16 == 0
    _call(d, oh, ow, BF16_CODE, PATCHES_PAD, pad)                                                 # the wave-per-patch kernel
    assert torch.equal(pad[..., :K], p16), size
    assert not bool(pad[..., K:].any()), size

    # fall-back of the entry: the generic kernel writes the padded layout
    flat = _empty((B * P * KPAD + 8,), torch.bfloat16, 7.0)
    off = flat[1:1 + B * P * KPAD].view(B, P, KPAD)
    assert off.data_ptr() % 16 == 2
    _call(d, oh, ow, BF16_CODE, PATCHES_PAD, off)
    assert torch.equal(off, pad), size
    assert float(flat[0]) == 7.0 and bool((flat[1 + B * P * KPAD:] == 7.0).all())                 # nothing outside the view
    dbg = _empty((B, oh, ow, 3), torch.uint8, 0)
    with_dbg = _call(d, oh, ow, BF16_CODE, PATCHES_PAD, _empty((B, P, KPAD), torch.bfloat16, 7.0), dbg)
    assert torch.equal(with_dbg, pad) and np.array_equal(dbg.cpu().numpy(), resized), size
    pad32 = _call(d, oh, ow, F32_CODE, PATCHES_PAD, _empty((B, P, KPAD), torch.float32, 7.0))
    assert torch.equal(pad32[..., :K], patches) and not bool(pad32[..., K:].any()), size


@gpu
def test_preprocess_front_end_floors_to_patch_multiples():
    """hip_preprocess.preprocess (what the extractors call) picks floor(h / 14) * 14 and the padded layout's shape."""
    from vit_colmap_amd.features import hip_preprocess as hp

    imgs = _images(5, 5, 101, 211)
    d = torch.from_numpy(imgs).cuda()
    out, resized = hp.preprocess(d, torch.bfloat16, "patches_pad", want_resized=True)
    assert tuple(out.shape) == (5, 7 * 15, KPAD) and tuple(resized.shape) == (5, 98, 210, 3)
    fast = hp.preprocess(d, torch.bfloat16, "patches_pad")
    assert torch.equal(fast, out)
    for b in range(5):
        assert np.array_equal(resized[b].cpu().numpy(), po.resize_linear_u8(imgs[b], 98, 210))
