"""GPU tests of the SwiGLU epilogue of vc_linear_bf16 and of DINOv2 ViT-g/14 on the hand-written kernels: the epilogue
against the float32 evaluation of the same bf16 data on both tile forms, saturating gates, the entry's argument checks, and the
giant (with and without register tokens) through `ViTExtractor`: prepared, no TunableOp, no library GEMM or SDPA reached,
tokens inside the bounds tests/test_vit_variants_gpu.py set for the library path, stream shards bit-identical."""
import numpy as np
import pytest
import torch

from test_e2e_gpu import synthetic_image
from util_vit import assert_token_errors, format_errors, token_errors

pytestmark = pytest.mark.gpu

SEED = 3
GIANT_BOUNDS = (3.8e-2, 4.4e-2)      # tests/test_vit_variants_gpu.py, dinov2_vitg14: twice the library path's measured error

# both tile forms (128 x 128 below 128 large tiles, the persistent 256 x 256 above) with ragged last tiles
ROWS = [1, 37, 1023, 1024, 1531, 2 * 1531, 16 * 1531 + 5]
SHAPES = [(64, 256), (1536, 8192), (768, 512)]


def _swiglu_case(rows, K, N, seed):
    """bf16 x, w12-style weight and bias: asymmetric, row-scaled (a swapped half, fragment or tile cannot pass), the value
    half at another scale and offset than the gate half."""
    H = N // 2
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(rows, K, device="cuda", generator=g).to(torch.bfloat16)
    w = torch.randn(N, K, device="cuda", generator=g) / K ** 0.5 * torch.linspace(0.5, 2.0, N, device="cuda")[:, None]
    w[H:] *= 0.6
    b = torch.randn(N, device="cuda", generator=g)
    b[H:] = 0.5 * b[H:] + 0.3
    return x, w.to(torch.bfloat16), b.to(torch.bfloat16)


def _reference(x, w, b):
    """-> (silu(a) * b, a, b) in float32 from the bf16 data."""
    H = w.shape[0] // 2
    pre = x.float() @ w.float().t() + b.float()
    a, v = pre[:, :H], pre[:, H:]
    return torch.nn.functional.silu(a) * v, a, v


def _assert_swiglu_close(out, x, w, b):
    """One rounding of the float32 product to bf16 (2^-8 |ref|) plus 2e-3 of accumulation-order slack on each pre-activation,
    pushed through silu(a) * b (|silu'| <= 1.1): every element is judged."""
    ref, a, v = _reference(x, w, b)
    assert out.shape == ref.shape and out.dtype == torch.bfloat16
    assert bool(torch.isfinite(out).all())
    err = (out.float() - ref).abs()
    tol = ref.abs() * 2 ** -8 + 2e-3 * (1.1 * v.abs() + torch.nn.functional.silu(a).abs()) + 1e-6
    ratio = float((err / tol).max())
    print(f"\n[swiglu rows {x.shape[0]} k {x.shape[1]} n {w.shape[0]}] max |err| {float(err.max()):.3e}, max err / tol {ratio:.3f}")
    assert bool((err <= tol).all()), (float(err.max()), ratio, int((err > tol).sum()))


@pytest.mark.parametrize("K,N", SHAPES)
@pytest.mark.parametrize("rows", ROWS)
def test_swiglu_epilogue_matches_float32_reference(rows, K, N):
    from vit_colmap_amd.vit.hip_ops import EPI_SWIGLU, linear

    x, w, b = _swiglu_case(rows, K, N, rows + K + N)
    out = linear(x, w, b, EPI_SWIGLU)
    assert tuple(out.shape) == (rows, N // 2)
    _assert_swiglu_close(out, x, w, b)


def test_swiglu_epilogue_single_k_step_on_the_large_tile():
    """k_in = 64 is one K tile: the 256 x 256 form's ring is filled by its prologue alone (157 row tiles, the last ragged)."""
    from vit_colmap_amd.vit.hip_ops import EPI_SWIGLU, linear

    x, w, b = _swiglu_case(40000, 64, 256, 11)
    _assert_swiglu_close(linear(x, w, b, EPI_SWIGLU), x, w, b)


@pytest.mark.parametrize("rows", [300, 16500])      # the 128 x 128 and the 256 x 256 form
def test_swiglu_large_gate_magnitudes(rows):
    """Gate pre-activations around -100, -20, 0, 20, 100 (through the gate bias, column j -> level j % 5): exp(-a) overflows
    float32 below about -88; the result must be 0 there, a * b far above zero, finite everywhere."""
    from vit_colmap_amd.vit.hip_ops import EPI_SWIGLU, linear

    K, N = 64, 512
    H = N // 2
    x, w, b = _swiglu_case(rows, K, N, 5)
    levels = torch.tensor([-100.0, -20.0, 0.0, 20.0, 100.0], device="cuda")
    col_level = levels[torch.arange(H, device="cuda") % 5]
    wf = w.float()
    wf[:H] *= 0.05                                   # gate = level + O(0.1)
    w = wf.to(torch.bfloat16)
    bf = b.float()
    bf[:H] = col_level
    b = bf.to(torch.bfloat16)
    out = linear(x, w, b, EPI_SWIGLU)
    assert bool(torch.isfinite(out).all()) and not bool(torch.isnan(out).any())
    ref, a, v = _reference(x, w, b)
    assert float((a - col_level).abs().max()) < 1.5
    o = out.float()
    assert bool((o[:, col_level == -100.0] == 0).all())                         # silu saturates to (-)0
    hi = col_level == 100.0
    av = (a * v)[:, hi]                                                         # ... and to a: silu(a) * b == a * b there
    assert bool(((o[:, hi] - av).abs() <= av.abs() * 2 ** -8 + 2e-3 * (1.1 * v[:, hi].abs() + a[:, hi].abs()) + 1e-6).all())
    _assert_swiglu_close(out, x, w, b)


def test_swiglu_argument_checks():
    from vit_colmap_amd import _lib
    from vit_colmap_amd.vit.hip_ops import EPI_BIAS, EPI_SWIGLU, linear

    z = lambda *s: torch.zeros(*s, device="cuda", dtype=torch.bfloat16)
    assert tuple(linear(z(4, 64), z(256, 64), z(256), EPI_SWIGLU).shape) == (4, 128)
    with pytest.raises(_lib.HipLibraryError):
        linear(z(4, 64), z(256, 64), z(256), EPI_SWIGLU, residual=z(4, 128))      # no residual with the gate
    with pytest.raises(_lib.HipLibraryError):
        linear(z(4, 64), z(384, 64), z(384), EPI_SWIGLU)                           # n_out % 256
    assert tuple(linear(z(4, 64), z(384, 64), z(384), EPI_BIAS).shape) == (4, 384)
    with pytest.raises(_lib.HipLibraryError):
        linear(z(4, 96), z(256, 96), z(256), EPI_SWIGLU)                           # k_in % 64
    with pytest.raises(_lib.HipLibraryError):
        linear(z(4, 64), z(256, 64), z(256), 3)                                    # the internal patch-embedding code
    with pytest.raises(_lib.HipLibraryError):
        linear(z(4, 64), z(256, 64), z(256), 3, residual=z(4, 256))
    torch.cuda.synchronize()


# ---- the model -----------------------------------------------------------------------------------------------------------

def _frames(ks=(0, 5)):
    return np.stack([synthetic_image(k) for k in ks])


def _giant(name):
    from vit_colmap_amd.features.vit_extractor import ViTExtractor

    return ViTExtractor(model_name=name, precision="bf16", seed=SEED, num_keypoints=256, descriptor_dim=128)


@pytest.fixture(scope="module")
def giant():
    """One bf16 `dinov2_vitg14` extractor (2.3 GB of operands) shared by the tests that only run it."""
    ex = _giant("dinov2_vitg14")
    yield ex
    del ex
    torch.cuda.empty_cache()


def _forbid_library_paths(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a library GEMM / SDPA was reached on the hand-written path")

    monkeypatch.setattr(torch.nn.functional, "linear", refuse)
    monkeypatch.setattr(torch.nn.functional, "scaled_dot_product_attention", refuse)


def _check_giant(ex, name, monkeypatch):
    from vit_colmap_amd.vit import DINOV2_ARCHS

    arch = DINOV2_ARCHS[name]
    assert arch.ffn == "swiglu"
    hip = ex.model._hip
    assert bool(hip) and len(hip) == arch.depth and all(h["kind"] == "gemm" and "w12" in h and "w3" in h for h in hip)
    assert tuple(hip[0]["w12"][0].shape) == (8192, 1536) and tuple(hip[0]["w3"][0].shape) == (1536, 4096)
    assert ex.tune_gemm is False                                   # (default constructor argument: tune_gemm=True)
    assert ex.model.accepts_padded_patches is (arch.registers == 0)
    d = torch.from_numpy(_frames()).cuda()
    with monkeypatch.context() as mp:
        _forbid_library_paths(mp)
        tokens, hp, wp = ex._tokens(d)
        torch.cuda.synchronize()
    assert (hp, wp) == (34, 45) and tuple(tokens.shape) == (2, hp * wp, arch.dim) and tokens.dtype == torch.bfloat16
    got = tokens.float()
    del tokens
    return got, d


def _compare_with_float32(name, got, d, capsys):
    from vit_colmap_amd.features.vit_extractor import ViTExtractor

    assert not torch.backends.cuda.matmul.allow_tf32
    ref_ex = ViTExtractor(model_name=name, precision="fp32", seed=SEED, num_keypoints=256, descriptor_dim=128)
    assert ref_ex.dtype == torch.float32 and not getattr(ref_ex.model, "_hip", None)
    ref = ref_ex._tokens(d)[0].float()
    del ref_ex
    e = token_errors(got, ref)
    with capsys.disabled():
        print(f"\n[{name} bf16 tokens on the hand-written kernels vs float32 module path] {format_errors(e)}")
    assert_token_errors(e, *GIANT_BOUNDS)
    del got, ref
    torch.cuda.empty_cache()


def test_giant_runs_on_the_hand_written_kernels(giant, monkeypatch, capsys):
    got, d = _check_giant(giant, "dinov2_vitg14", monkeypatch)
    _compare_with_float32("dinov2_vitg14", got, d, capsys)


def test_giant_stream_shards_are_bit_identical(giant):
    """16 frames through `_tokens` whole and as two shards on two streams: the GEMM path is row-local."""
    d = torch.from_numpy(_frames(range(16))).cuda()
    was = giant.model.batch_shards
    try:
        giant.model.batch_shards = 1
        whole = giant._tokens(d)[0].clone()
        giant.model.batch_shards = 2
        assert giant.model._shard_plan(torch.empty(16, 1, 1, device="cuda")) is not None
        sharded = giant._tokens(d)[0]
        torch.cuda.synchronize()
    finally:
        giant.model.batch_shards = was
    assert bool(torch.isfinite(whole.float()).all())
    assert torch.equal(whole, sharded)
    del whole, sharded
    torch.cuda.empty_cache()


def test_giant_through_the_extractor(giant):
    kp, desc = giant._run_inference(synthetic_image(1))
    assert kp.dtype == np.float32 and kp.ndim == 2 and kp.shape[1] == 2 and 0 < len(kp) <= 256
    assert desc.dtype == np.uint8 and desc.shape == (len(kp), 128)
    assert np.isfinite(kp).all()
    assert int((desc.astype(np.int32).sum(axis=1) > 0).sum()) == len(kp)


def test_giant_with_registers_runs_on_the_hand_written_kernels(monkeypatch, capsys):
    torch.cuda.empty_cache()
    ex = _giant("dinov2_vitg14_reg")
    got, d = _check_giant(ex, "dinov2_vitg14_reg", monkeypatch)
    del ex
    torch.cuda.empty_cache()
    _compare_with_float32("dinov2_vitg14_reg", got, d, capsys)
