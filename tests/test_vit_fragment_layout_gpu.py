"""The ViT-S block kernels with x and the attention output in fragment order (VC_ACT_FRAGMENT) against the
same kernels on row-major tensors: same operands, same arithmetic, same 32-row groups, so every comparison is torch.equal."""
import pytest
import torch

pytestmark = pytest.mark.gpu

K = 384
NAN = float("nan")


def fm_pack(x, fill=NAN):
    """[M][384] bf16 -> fragment order, the padding rows filled with `fill`: element (m, k) is [m >> 5][k >> 4]
    [((k >> 3) & 1) * 32 + (m & 31)][k & 7]."""
    M = x.shape[0]
    Mp = (M + 31) // 32 * 32
    xp = torch.full((Mp, K), fill, dtype=x.dtype, device=x.device)
    xp[:M] = x
    return xp.view(Mp // 32, 32, 24, 2, 8).permute(0, 2, 3, 1, 4).contiguous().view(Mp // 32, 24, 64, 8)


def fm_unpack(t, M):
    nb = t.shape[0]
    return t.view(nb, 24, 2, 32, 8).permute(0, 3, 1, 2, 4).reshape(nb * 32, K)[:M].contiguous()


def test_pack_helpers_follow_the_byte_formula():
    x = torch.arange(70 * K, device="cuda").remainder(251).to(torch.bfloat16).view(70, K)
    flat = fm_pack(x, 0.0).view(-1)
    for m, k in [(0, 0), (1, 7), (31, 8), (32, 15), (33, 16), (69, 383), (40, 200)]:
        byte = ((m >> 5) * 24 + (k >> 4)) * 1024 + (((k >> 3) & 1) * 32 + (m & 31)) * 16 + (k & 7) * 2
        assert flat[byte // 2] == x[m, k]
    assert torch.equal(fm_unpack(fm_pack(x), 70), x)


def _rand(g, *shape, scale=1.0, shift=0.0):
    return (torch.randn(*shape, device="cuda", generator=g) * scale + shift).to(torch.bfloat16)


@pytest.mark.parametrize("M", [1, 32, 33, 255, 257, 300])
def test_xs_qkv_from_fragment_order(M):
    """LayerNorm + bias, n_out 1152: x in fragment order, row-major out."""
    from vit_colmap_amd.vit.hip_ops import FRAGMENT, XsLinear

    g = torch.Generator(device="cuda").manual_seed(M)
    x = _rand(g, M, K, scale=1.5, shift=0.3)
    N = 1152
    lin = XsLinear(torch.randn(N, K, device="cuda", generator=g) / K ** 0.5, torch.randn(N, device="cuda", generator=g),
                   1 + 0.2 * torch.randn(K, device="cuda", generator=g), 0.1 * torch.randn(K, device="cuda", generator=g), 1e-6)
    ref = lin(x)
    out = torch.full((M, N), NAN, dtype=torch.bfloat16, device="cuda")
    lin(fm_pack(x), rows=M, x_layout=FRAGMENT, out=out)
    assert torch.equal(out, ref)


@pytest.mark.parametrize("M", [1, 32, 33, 255, 257, 300])
def test_xs_proj_in_fragment_order(M):
    """Residual epilogue, n_out 384: in place on a residual in fragment order, and out of place from a row-major residual
    into an output pre-filled with NaN."""
    from vit_colmap_amd.vit.hip_ops import EPI_RESIDUAL, FRAGMENT, ROW_MAJOR, XsLinear

    g = torch.Generator(device="cuda").manual_seed(1000 + M)
    a, res = _rand(g, M, K), _rand(g, M, K, scale=2.0)
    lin = XsLinear(torch.randn(K, K, device="cuda", generator=g) / K ** 0.5, torch.randn(K, device="cuda", generator=g))
    ref = lin(a, EPI_RESIDUAL, residual=res)
    assert not torch.isnan(ref).any()

    xf = fm_pack(res)
    lin(fm_pack(a), EPI_RESIDUAL, residual=xf, out=xf, rows=M, x_layout=FRAGMENT, residual_layout=FRAGMENT, out_layout=FRAGMENT)
    assert torch.equal(fm_unpack(xf, M), ref)

    out = fm_pack(torch.full((M, K), NAN, dtype=torch.bfloat16, device="cuda"))
    lin(fm_pack(a), EPI_RESIDUAL, residual=res, out=out, rows=M, x_layout=FRAGMENT, residual_layout=ROW_MAJOR, out_layout=FRAGMENT)
    assert torch.equal(fm_unpack(out, M), ref)


@pytest.mark.parametrize("M", [1, 129, 300])
def test_fused_mlp_in_fragment_order(M):
    """Fragment order in place and fragment order -> row-major rows, against the row-major kernel.  Two hidden features
    have a bias beyond the GELU table's range (|pre-activation| >= 8), so their chunks take the float path and the others
    the table."""
    from vit_colmap_amd.vit.hip_ops import FRAGMENT, FusedMlp

    Hd = 1536
    g = torch.Generator(device="cuda").manual_seed(2000 + M)
    x = _rand(g, M, K, scale=1.5, shift=0.3)
    w1 = torch.randn(Hd, K, device="cuda", generator=g) / K ** 0.5
    b1 = 0.5 * torch.randn(Hd, device="cuda", generator=g)
    b1[5], b1[700] = 40.0, -40.0
    w2 = torch.randn(K, Hd, device="cuda", generator=g) / Hd ** 0.5
    b2 = torch.randn(K, device="cuda", generator=g)
    mlp = FusedMlp(w1, b1, 1 + 0.2 * torch.randn(K, device="cuda", generator=g), 0.1 * torch.randn(K, device="cuda", generator=g),
                   w2, b2, 1e-6)
    ref = mlp(x.clone())
    assert not torch.isnan(ref).any()

    xf = fm_pack(x)
    assert mlp(xf, rows=M, x_layout=FRAGMENT) is xf
    assert torch.equal(fm_unpack(xf, M), ref)

    xf, out = fm_pack(x), torch.full((M, K), NAN, dtype=torch.bfloat16, device="cuda")
    assert mlp(xf, rows=M, x_layout=FRAGMENT, out=out) is out
    assert torch.equal(out, ref)
    assert torch.equal(fm_unpack(xf, M), x)


@pytest.mark.parametrize("B,N", [(2, 65), (3, 257), (2, 577)])
def test_attention_output_in_fragment_order(B, N):
    """6 heads; N is no multiple of 32, so a wave's queries straddle the 32-row blocks of the flat row index.  (2, 577)
    runs two query tiles per wave."""
    from vit_colmap_amd.vit.hip_ops import FRAGMENT, Q_PRESCALE, attention

    g = torch.Generator(device="cuda").manual_seed(B * N)
    qkv = torch.randn(B, N, 3, 6, 64, device="cuda", generator=g)
    for prescaled in (True, False):
        t = qkv.clone()
        if prescaled:
            t[:, :, 0] *= Q_PRESCALE
        t = t.to(torch.bfloat16).view(B, N, 3 * K)
        ref = attention(t, 6, q_prescaled=prescaled)
        assert not torch.isnan(ref).any()
        out = attention(t, 6, q_prescaled=prescaled, out_layout=FRAGMENT)
        assert torch.equal(fm_unpack(out, B * N), ref.view(B * N, K))


@pytest.fixture(scope="module")
def vits():
    from vit_colmap_amd.vit import build_dinov2

    return build_dinov2("dinov2_vits14").init_random(seed=3).eval().fold_layerscale().to("cuda", torch.bfloat16)


@pytest.mark.parametrize("B,side", [(3, 224), (17, 224), (2, 322)])
def test_forward_equals_the_row_major_loop(vits, B, side):
    """3 images: one stream; 17: two shards, each with its own tensors; 322 x 322: 530 tokens, two query tiles per wave."""
    hp = side // 14
    g = torch.Generator(device="cuda").manual_seed(B + side)
    patches = torch.randn(B, hp * hp, 588, device="cuda", generator=g).to(torch.bfloat16)
    try:
        with torch.inference_mode():
            vits.fragment_layout = False
            ref = vits.forward_patch_tokens(patches, hp, hp)
            vits.fragment_layout = True
            out = vits.forward_patch_tokens(patches, hp, hp)
        torch.cuda.synchronize()
    finally:
        vits.fragment_layout = True
    assert not torch.isnan(ref).any()
    assert torch.equal(out, ref)
