"""Unit order of the attention kernel (csrc/attention.hip).

A launch slot is mapped to its work unit — 128 or 256 query rows of one (image, head) — by vc::xcd_tile, which must be a
bijection at every unit count.  `vc_attention_bf16` is called through `_lib` with the output pre-filled with NaN, so a unit
that the map skips shows as NaN rows (and one computed twice leaves another skipped).

Reference: util_vit.attention_reference (float32 softmax on the same bf16 data); tolerance: that of
test_vit_gpu.test_attention_prescaled_q_lazy_max (maximum absolute error < 3e-2, relative L2 < 1e-2)."""
import math

import pytest
import torch

from util_vit import attention_reference

pytestmark = pytest.mark.gpu

MAX_ABS, REL_L2 = 3e-2, 1e-2

# (B, N, H): QT = 2 from 512 tokens on, units = B * H * ceil(N / (128 QT))
SHAPES = [
    (1, 64, 1),      # QT 1,  1 unit
    (1, 520, 2),     # QT 2,  6 units: fewer than XCDs, ragged last unit and key block
    (3, 600, 3),     # QT 2, 27 units: not a multiple of 8
    (9, 130, 1),     # QT 1, 18 units: not a multiple of 8
    (2, 300, 5),     # QT 1, 30 units, ragged last key block
    (1, 1531, 6),    # QT 2, 36 units: one image at the bench's token count
]


def make_qkv(B, N, H, spread, q_prescaled):
    """The construction of test_attention_prescaled_q_lazy_max: late keys larger, so that the row maximum keeps moving;
    with q_prescaled the q part carries (1/8) log2 e.  -> (B, N, 3 * H * 64) bf16."""
    g = torch.Generator(device="cuda").manual_seed(B * 100 + N + H)
    qkv = torch.randn(B, N, 3, H, 64, device="cuda", generator=g)
    qkv[:, :, 0] *= spread * (0.125 * math.log2(math.e) if q_prescaled else 1.0)
    qkv[:, :, 1] *= torch.linspace(0.5, 1.5, N, device="cuda")[None, :, None, None]
    return qkv.to(torch.bfloat16).reshape(B, N, 3 * H * 64).contiguous()


def run_into_nan(qkv, H, q_prescaled):
    from vit_colmap_amd import _lib

    B, N, _ = qkv.shape
    out = torch.full((B, N, H * 64), float("nan"), dtype=torch.bfloat16, device=qkv.device)
    lib = _lib.load()
    _lib.check(lib.vc_attention_bf16(_lib.ptr(qkv), B, N, H, 64, int(q_prescaled), _lib.ptr(out), _lib.stream_ptr()),
               "vc_attention_bf16")
    torch.cuda.synchronize()
    return out.float()


def check(out, ref, what):
    bad_rows = (~torch.isfinite(out)).any(dim=2).nonzero().tolist()
    assert not bad_rows, f"{what}: {len(bad_rows)} rows not written, first (image, token) {bad_rows[:4]}"
    err = (out - ref).abs()
    rel = float((out - ref).norm() / ref.norm())
    print(f"{what}: max abs {float(err.max()):.3e}, rel L2 {rel:.3e}")
    assert float(err.max()) < MAX_ABS and rel < REL_L2, (what, float(err.max()), rel)


@pytest.mark.parametrize("q_prescaled", [1, 0])
@pytest.mark.parametrize("B,N,H", SHAPES)
def test_every_unit_is_computed_once(B, N, H, q_prescaled):
    qkv = make_qkv(B, N, H, 1.0, q_prescaled)
    out = run_into_nan(qkv, H, q_prescaled)
    ref = attention_reference(qkv, H, math.log(2.0) if q_prescaled else 0.125)
    check(out, ref, f"units B{B} N{N} H{H} prescaled {q_prescaled}")


def test_units_that_take_the_exact_pass():
    """Spread 6 (test_attention_range_gpu.test_whole_input_in_range's construction): later scores exceed the first block's
    maximum by more than the fast pass's reach, so units also take the exact pass, which re-centres rows: the accumulators'
    start value must be the moved maximum from the next key block on, in every unit."""
    B, N, H = 1, 520, 2
    qkv = make_qkv(B, N, H, 6.0, 1)
    out = run_into_nan(qkv, H, 1)
    check(out, attention_reference(qkv, H, math.log(2.0)), f"moving maximum B{B} N{N} H{H}")
