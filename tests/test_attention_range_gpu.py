"""Range behaviour of the q_prescaled attention kernel (csrc/attention.hip).

With pre-scaled q a score is a base-2 exponent.  The kernel's fast pass keeps the row maximum of the first key block as its
reference to the end and never tests a later block; a unit in which a row sum then passes 64 N (some later score stood more
than 2^6 above the reference) or an output is not finite is recomputed by the exact online-softmax pass.  These cases put scores at chosen levels — whole rows (any level must cancel),
and later keys against the first block's (inside the reach, at its edge, far outside) — and compare every row with a float64
softmax on the same bf16 data.

Score levels are exact: dimension 0 of every key is 1.0 and dimension 0 of query row r is a bf16-exact offset c_r, so the
row's scores are c_r + (a random part of standard deviation ~1 from the other 63 dimensions).  A constant per row leaves the
true softmax unchanged, so the reference of such a case is computed with the offsets set to 0.

Tolerance: that of test_vit_gpu.test_attention_prescaled_q_lazy_max (maximum absolute error < 3e-2, relative L2 < 1e-2), over
every row of every case."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

# (B, N, H): QT = 1 with two key blocks and a ragged last one; QT = 2 with nine key blocks, a ragged last one and a partly
# filled last 256-query unit; a head count other than the bench's
SHAPES = [(1, 100, 2), (1, 520, 2), (1, 520, 12)]

LADDER = [0.0] + [s * c for c in (32, 64, 96, 112, 124, 128, 136, 160, 256, 1024) for s in (1.0, -1.0)]
# a smaller set: float32 could hold 2^level itself, which a kernel that did not subtract a row's maximum would depend on
LADDER_INSIDE = [0.0, 32.0, -32.0, 64.0, -64.0, 96.0, -96.0, 112.0, -100.0]

MAX_ABS, REL_L2 = 3e-2, 1e-2


def reference64(q, k, v):
    """softmax(q k^T) v in base 2 and float64 (a score is a base-2 exponent), (B, N, H, 64) each -> (B, N, H * 64)."""
    B, N, H, _ = q.shape
    s = torch.einsum("bqhd,bkhd->bhqk", q.double(), k.double()) * math.log(2.0)
    out = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, dim=-1), v.double())
    return out.reshape(B, N, H * 64)


def base_parts(B, N, H, seed):
    """q, k, v (B, N, H, 64) float32: q . k over dimensions 1..63 has standard deviation ~1; dimension 0 of k is 1, of q 0."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    sd = 63.0 ** -0.25
    q = torch.randn(B, N, H, 64, device="cuda", generator=g) * sd
    k = torch.randn(B, N, H, 64, device="cuda", generator=g) * sd
    v = torch.randn(B, N, H, 64, device="cuda", generator=g)
    q[..., 0] = 0.0
    k[..., 0] = 1.0
    return q, k, v


def run_kernel(q, k, v):
    from vit_colmap_amd.vit.hip_ops import attention

    B, N, H, _ = q.shape
    qkv = torch.stack((q, k, v), dim=2).to(torch.bfloat16)           # (B, N, 3, H, 64), as util_vit.attention_reference reads it
    out = attention(qkv.reshape(B, N, 3 * H * 64).contiguous(), H, q_prescaled=True).float()
    q16, k16, v16 = (t.float() for t in qkv.unbind(dim=2))
    return out, q16, k16, v16


def check_all_rows(out, ref, what):
    ref = ref.float()
    assert bool(torch.isfinite(out).all()), f"{what}: {int((~torch.isfinite(out)).sum())} non-finite outputs"
    err = (out - ref).abs()
    rel = float((out - ref).norm() / ref.norm())
    row = int(err.amax(dim=(0, 2)).argmax())
    print(f"{what}: max abs {float(err.max()):.3e} (row {row}), rel L2 {rel:.3e}")
    assert float(err.max()) < MAX_ABS and rel < REL_L2, (what, float(err.max()), row, rel)


def offsets_for(N, ladder):
    return torch.tensor([ladder[r % len(ladder)] for r in range(N)], device="cuda")


@pytest.mark.parametrize("B,N,H", SHAPES)
@pytest.mark.parametrize("ladder", [LADDER, LADDER_INSIDE], ids=["ladder", "inside"])
def test_offset_ladder(B, N, H, ladder):
    """Rows cycle through the offsets (21 and 9 of them: every one occurs in every workgroup).  LADDER reaches far beyond
    float32 on both sides; a row's level must cancel against its own maximum whatever it is."""
    q, k, v = base_parts(B, N, H, 1000 + N + H)
    c = offsets_for(N, ladder)
    assert torch.equal(c.to(torch.bfloat16).float(), c)             # bf16-exact levels
    q[..., 0] = c[None, :, None]
    out, q16, k16, v16 = run_kernel(q, k, v)
    q16[..., 0] = 0.0                                                # the same softmax, computed where float64 exp has no trouble either
    check_all_rows(out, reference64(q16, k16, v16), f"ladder B{B} N{N} H{H}")


@pytest.mark.parametrize("B,N,H", SHAPES)
def test_later_keys_above_the_first_block(B, N, H):
    """Dimension 1 of the keys is 0 in the first key block and 1 after it, dimension 1 of query row r cycles through LADDER:
    the row's later scores stand that far above (or below) the maximum the fast pass keeps, so that every workgroup holds
    rows the fast pass may keep (0 and below, where the later keys vanish) and rows that force the exact pass."""
    q, k, v = base_parts(B, N, H, 4000 + N + H)
    k[..., 1] = (torch.arange(N, device="cuda") >= 64).float()[None, :, None]
    q[..., 1] = offsets_for(N, LADDER)[None, :, None]
    out, q16, k16, v16 = run_kernel(q, k, v)
    check_all_rows(out, reference64(q16, k16, v16), f"later keys B{B} N{N} H{H}")


@pytest.mark.parametrize("B,N,H", SHAPES)
def test_late_overflow(B, N, H):
    """Every score is ordinary until the last key block, where one key meets a few query rows (of one workgroup) at 2^256:
    those rows must return that key's v row, the others must not notice."""
    q, k, v = base_parts(B, N, H, 2000 + N + H)
    key = N - 3                                                      # in the last, ragged key block
    rows = [N - 9, N - 37, N - 70]                                   # all in one unit (N = 520: the second of three)
    k[..., 1] = 0.0
    k[:, key, :, 1] = 1.0
    q[:, rows, :, 1] = 256.0
    out, q16, k16, v16 = run_kernel(q, k, v)
    check_all_rows(out, reference64(q16, k16, v16), f"late overflow B{B} N{N} H{H}")
    hit = out.reshape(B, N, H, 64)[:, rows]
    assert float((hit - v16[:, key][:, None]).abs().max()) < MAX_ABS


@pytest.mark.parametrize("B,N,H", SHAPES)
def test_wide_spread_inside_a_row(B, N, H):
    """Keys alternate between +96 and -96 for every query: a row's probabilities span 2^192, more than float32 holds below
    one; what underflows is negligible, and no unit needs the exact pass."""
    q, k, v = base_parts(B, N, H, 3000 + N + H)
    k[..., 1] = (1.0 - 2.0 * (torch.arange(N, device="cuda") % 2))[None, :, None]
    q[..., 1] = 96.0
    out, q16, k16, v16 = run_kernel(q, k, v)
    check_all_rows(out, reference64(q16, k16, v16), f"wide spread B{B} N{N} H{H}")


@pytest.mark.parametrize("B,N,H", SHAPES[:2])
def test_whole_input_in_range(B, N, H):
    """The spread = 6.0 construction of test_vit_gpu.test_attention_prescaled_q_lazy_max: ordinary scores only."""
    from vit_colmap_amd.vit.hip_ops import attention

    g = torch.Generator(device="cuda").manual_seed(B * 100 + N + H)
    qkv = torch.randn(B, N, 3, H, 64, device="cuda", generator=g)
    qkv[:, :, 0] *= 6.0 * 0.125 * math.log2(math.e)
    qkv[:, :, 1] *= torch.linspace(0.5, 1.5, N, device="cuda")[None, :, None, None]
    qkv = qkv.to(torch.bfloat16)
    out = attention(qkv.reshape(B, N, 3 * H * 64).contiguous(), H, q_prescaled=True).float()
    q16, k16, v16 = (t.float() for t in qkv.unbind(dim=2))
    check_all_rows(out, reference64(q16, k16, v16), f"in range B{B} N{N} H{H}")
