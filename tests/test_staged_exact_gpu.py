"""The staged GEMMs (gemm.hip gemm_kernel and gemm256_kernel behind vc_linear_bf16, vc_patch_embed_bf16 and vc_conv_taps_bf16)
and add + LayerNorm (vit_ops.hip) on exact operands: bf16 inputs for which bf16 x bf16 products, float32 accumulation and one
bf16 rounding have ONE possible result (util_vit_exact.py; proved on the CPU by test_staged_exact_spec.py).  Outputs are
pre-filled with NaN, every element is judged, and the comparison is bit equality — or, behind the GELU, SwiGLU and LayerNorm
arithmetic, a bound derived per element.  Every test that is meant for one tile form of vc_linear_bf16 asserts the form
through hip_ops.linear_tile_rows and derives its row count from the device's CU count.  A dropped or doubled K tile, a tile
written to the wrong rows, a tap taken from the wrong pixel change bits here; under the tolerances of test_vit_gpu.py they
do not."""
import pytest
import torch

import util_vit_exact as U

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
RAGGED = 219                  # the last row tile of the 256-row shapes holds 256 - 219 = 37 rows


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.bfloat16, device=DEV)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _ceil_div(a, b):
    return -(-a // b)


def _head(case, rows):
    """The case cut to its first `rows` rows (operands and expectation)."""
    cut = dict(case, name=f"{case['name']} first {rows} rows")
    for key in ("x", "residual", "expect_bits", "ref", "bound", "h"):
        if case.get(key) is not None:
            cut[key] = case[key][:rows].contiguous()
    return cut


def _judge(out, case):
    """The case's comparison; for a case judged by a bound, its largest err / bound is printed first."""
    if "ref" in case:
        print(f"{case['name']}: max err / bound = {U.bound_ratio(out, case):.3f}")
    U.compare(out, case)


def _check_linear(case, tile):
    """vc_linear_bf16 into a NaN-filled output, and for EPI_RESIDUAL also in place on the residual; the tile form asserted."""
    from vit_colmap_amd.vit.hip_ops import linear, linear_tile_rows

    rows, n = case["x"].shape[0], case["w"].shape[0]
    assert linear_tile_rows(rows, n) == tile, (rows, n, _cus())
    out = _nan(rows, n // 2 if case["epi"] == U.EPI_SWIGLU else n)
    linear(case["x"], case["w"], case["b"], case["epi"], case["residual"], out=out)
    _judge(out, case)
    if case["epi"] == U.EPI_RESIDUAL:
        r2 = case["residual"].clone()
        linear(case["x"], case["w"], case["b"], case["epi"], r2, out=r2)
        _judge(r2, dict(case, name=case["name"] + " in place"))


FORMS = [("dense", U.EPI_BIAS), ("dense", U.EPI_RESIDUAL), ("sparse", U.EPI_BIAS), ("sparse", U.EPI_RESIDUAL), ("sparse", U.EPI_GELU)]


# ---- a. vc_linear_bf16 on the 128 x 128 tile ------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 127, 129, 1025])
@pytest.mark.parametrize("K,N,n_swiglu", [(64, 128, 256), (128, 384, 768), (192, 384, 768), (3072, 768, 256)])
def test_linear_128_tile(rows, K, N, n_swiglu):
    """One, two, three and 48 K tiles, one row to nine row tiles with a ragged last one, every epilogue, both operand kinds.
    n_swiglu is the width of the SwiGLU product (the output is half as wide)."""
    for kind, epi in FORMS:
        _check_linear(U.linear_case(rows, K, N, kind, epi, seed=rows + K + N + epi, device=DEV), 128)
    _check_linear(U.linear_case(rows, K, n_swiglu, "sparse", U.EPI_SWIGLU, seed=rows + K + n_swiglu, device=DEV), 128)


# ---- b. vc_linear_bf16 on the 256 x 256 tile ------------------------------------------------------------------------------
def _threshold_rows(tiles_n):
    """The fewest row tiles with which tiles * 2 >= CUs, the last of them 37 rows."""
    return 256 * _ceil_div(_ceil_div(_cus(), 2), tiles_n) - RAGGED


def _walk_rows(tiles_n):
    """Somewhat more than two tiles per workgroup: workgroups take two or three, the tile seam is crossed once and twice."""
    return 256 * _ceil_div(2 * _cus() + 11, tiles_n) - RAGGED


def _check_both_sides(case):
    """The case on the 256 x 256 tile, and with one row tile fewer — below the threshold — on the 128 x 128 tile: same bits."""
    _check_linear(case, 256)
    _check_linear(_head(case, case["x"].shape[0] - 256), 128)


@pytest.mark.parametrize("K", [64, 128, 192, 448, 3072])
def test_linear_256_tile_at_the_threshold(K):
    """N = 768 with the fewest row tiles that take the large tile: 1, 2, 3, 7 and 48 K tiles through the two-buffer ring (two:
    the nk > 1 prologue wait and the t + 2 < nk tail; three and seven: odd counts)."""
    rows = _threshold_rows(3)
    for kind, epi in FORMS:
        _check_both_sides(U.linear_case(rows, K, 768, kind, epi, seed=K + epi, device=DEV))


def test_linear_256_tile_k4096():
    """ViT-L's fc2 / ViT-g's w3 depth: 64 K tiles at N = 1024."""
    rows = _threshold_rows(4)
    for kind, epi in FORMS:
        _check_both_sides(U.linear_case(rows, 4096, 1024, kind, epi, seed=4096 + epi, device=DEV))


@pytest.mark.parametrize("K", [64, 192])
def test_linear_256_tile_walk(K):
    """Persistent workgroups walk two or three tiles: the next tile's copies land in the buffer the epilogue just transposed
    through."""
    rows = _walk_rows(3)
    assert 2 * _cus() < _ceil_div(rows, 256) * 3 < 3 * _cus()
    for kind, epi in FORMS:
        _check_linear(U.linear_case(rows, K, 768, kind, epi, seed=K + epi + 100, device=DEV), 256)


@pytest.mark.parametrize("n_out", [512, 1536])
@pytest.mark.parametrize("K", [64, 192])
def test_linear_256_tile_swiglu(n_out, K):
    """SwiGLU on the large tile (a tile makes 128 output columns): at the threshold, on both sides of it, and walking."""
    _check_both_sides(U.linear_case(_threshold_rows(n_out // 256), K, n_out, "sparse", U.EPI_SWIGLU, seed=n_out + K, device=DEV))
    _check_linear(U.linear_case(_walk_rows(n_out // 256), K, n_out, "sparse", U.EPI_SWIGLU, seed=n_out + K + 1, device=DEV), 256)


# ---- c. vc_patch_embed_bf16 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,n_out,k_in", [(5, 100, 384, 640), (130, 1, 128, 64), (2, 257, 256, 128)])
def test_patch_embed_bits(B, T, n_out, k_in):
    """Row m = (b, t) goes to row m + b + 1 of out with pos_embed[1 + t]: images straddle row tiles, T = 1 makes b = m.  The
    class-token rows keep their NaN and the row behind `out` is untouched."""
    from vit_colmap_amd.vit.hip_ops import patch_embed

    c = U.patch_case(B, T, n_out, k_in, seed=B + T + n_out, device=DEV)
    buf = _nan(B * (T + 1) + 1, n_out)
    out = buf[:-1].view(B, T + 1, n_out)
    patch_embed(c["x"], c["w"], c["b"], c["pos"], out)
    U.compare(out[:, 1:], c)
    assert bool(torch.isnan(out[:, 0]).all()) and bool(torch.isnan(buf[-1]).all())


# ---- d. vc_conv_taps_bf16 -------------------------------------------------------------------------------------------------
def _run_conv(case, out=None, out_parity=-1):
    from vit_colmap_amd.vit.hip_ops import conv_taps

    B, H, W, kh, kw, dy0, dx0 = case["geometry"]
    xr = case["x_rows"].clone()
    assert bool(xr[-1].any())                                             # junk in the spare row: the call must zero it
    if out is None:
        out = _nan(B * H * W, case["w"].shape[0])
    conv_taps(xr, case["w"], case["b"], B, H, W, kh, kw, dy0, dx0, case["epi"], out=out, out_parity=out_parity)
    assert not bool(xr[-1].any()) and torch.equal(xr[:-1], case["x_rows"][:-1])
    return out


@pytest.mark.parametrize("kind,epi", [("dense", U.EPI_BIAS), ("sparse", U.EPI_BIAS), ("sparse", U.EPI_GELU)])
def test_conv_3x3_bits(kind, epi):
    """3 x 3 pad 1 on (3, 9, 31, 128) -> 512: two K tiles per tap, four ragged row tiles that straddle images."""
    c = U.conv_case(3, 9, 31, 128, 512, 3, 3, -1, -1, kind, epi, seed=31 + epi, device=DEV)
    _judge(_run_conv(c), c)


def test_conv_sixteen_taps_bits():
    """4 x 4 taps at (-1, -2): every bit of the kernel's 16-bit tap mask."""
    for kind in ("dense", "sparse"):
        c = U.conv_case(2, 6, 5, 64, 256, 4, 4, -1, -2, kind, U.EPI_BIAS, seed=16, device=DEV)
        U.compare(_run_conv(c), c)


@pytest.mark.parametrize("dy0,dx0", [(-8, 0), (8, 0), (0, -8), (0, 8)])
def test_conv_farthest_tap_bits(dy0, dx0):
    """One tap 8 pixels away, the largest offset the entry accepts: rows nearer than 8 to that edge are the bias alone."""
    B, H, W, N = 1, 12, 11, 256
    c = U.conv_case(B, H, W, 64, N, 1, 1, dy0, dx0, "dense", U.EPI_BIAS, seed=8 + dy0 + 3 * dx0, device=DEV)
    out = _run_conv(c)
    U.compare(out, c)
    grid = out.reshape(B, H, W, N)
    edge = {(-8, 0): grid[:, :8], (8, 0): grid[:, H - 8:], (0, -8): grid[:, :, :8], (0, 8): grid[:, :, W - 8:]}[(dy0, dx0)]
    assert torch.equal(edge, c["b"].expand_as(edge))


def test_conv_walk_bits():
    """2 x 2 taps, C = 64, N = 512, more tiles than CUs: persistent workgroups cross the tile seam."""
    H, W = 9, 31
    B = 256 * (_cus() // 2) // (H * W) + 1
    assert _ceil_div(B * H * W, 256) * 2 > _cus()
    for kind in ("dense", "sparse"):
        c = U.conv_case(B, H, W, 64, 512, 2, 2, -1, 0, kind, U.EPI_BIAS, seed=22, device=DEV)
        U.compare(_run_conv(c), c)


def test_conv_parity_classes_bits():
    """The four parity classes of a stride-2 transposed convolution (model/hip_heads.py deconv_class_matrices) with exact
    weights into a NaN-filled [B][2H][2W][N] and a sentinel row: bits of torch's float64 conv_transpose2d (CPU) on the same
    operands, which the four class cases must reproduce exactly too."""
    from vit_colmap_amd.model.hip_heads import deconv_class_matrices

    B, H, W, C, N = 2, 5, 7, 64, 256
    g = U.gen(44)
    img = U.dyadic(-8, 8, 0.25, (B, H, W, C), g)
    wt = U.pm_values((C, N, 4, 4), g)                                     # ConvTranspose2d layout
    b = U.dyadic(-8, 8, 0.25, (N,), g)
    ref = torch.nn.functional.conv_transpose2d(img.permute(0, 3, 1, 2), wt, b, stride=2, padding=1).permute(0, 2, 3, 1)
    buf = _nan(B * 4 * H * W + 1, N)
    expect = torch.zeros(B, 2 * H, 2 * W, N, dtype=torch.int32, device=DEV)
    for m, i, j, dy0, dx0 in deconv_class_matrices(wt):
        c = U.conv_case(B, H, W, C, N, 2, 2, dy0, dx0, "dense", U.EPI_BIAS, seed=i + j, device=DEV, img=img, weight=m, bias=b)
        expect[:, i::2, j::2] = c["expect_bits"].reshape(B, H, W, N)
        _run_conv(c, out=buf, out_parity=2 * i + j)
    assert torch.equal(expect.cpu(), U.f64_to_bits(U.bf16_rne(ref)))
    U.compare(buf[:-1], dict(name="conv parity classes", expect_bits=expect))
    assert bool(torch.isnan(buf[-1]).all())


# ---- e. the comparisons are not vacuous: the kernels fed ONE doubled weight must fail them --------------------------------
def _doubled_weight(case, col):
    k = int(torch.nonzero(case["w"][col])[0])
    w = case["w"].clone()
    w[col, k] *= 2
    return dict(case, w=w)


@pytest.mark.parametrize("tile", [128, 256])
def test_linear_with_one_doubled_weight_is_caught(tile):
    from vit_colmap_amd.vit.hip_ops import linear, linear_tile_rows

    rows = 129 if tile == 128 else _threshold_rows(3)
    c = U.linear_case(rows, 192, 768, "sparse", U.EPI_BIAS, seed=9, device=DEV)
    assert linear_tile_rows(rows, 768) == tile
    col = 500
    wrong = _doubled_weight(c, col)
    out = _nan(rows, 768)
    linear(c["x"], wrong["w"], c["b"], U.EPI_BIAS, out=out)
    bad = U.bits_of(out) != c["expect_bits"]
    assert bool(bad[:, col].all()) and int(bad.sum()) == rows            # exactly that column, on every row (x has no zero)
    with pytest.raises(AssertionError):
        U.compare(out, c)


def test_conv_with_one_doubled_weight_is_caught():
    c = U.conv_case(3, 9, 31, 128, 512, 3, 3, -1, -1, "sparse", U.EPI_BIAS, seed=31, device=DEV)
    out = _run_conv(_doubled_weight(c, 300))
    bad = U.bits_of(out) != c["expect_bits"]
    assert bool(bad.any()) and not bool(bad[:, :300].any()) and not bool(bad[:, 301:].any())
    with pytest.raises(AssertionError):
        U.compare(out, c)


# ---- f. add + LayerNorm ---------------------------------------------------------------------------------------------------
def _add_layernorm(x, residual, gamma, beta, eps, want_sum=True):
    """vc_add_layernorm_bf16 into NaN-filled outputs -> (sum or None, y)."""
    from vit_colmap_amd import _lib

    rows, C = x.shape
    y = _nan(rows, C)
    s = _nan(rows, C) if residual is not None and want_sum else None
    _lib.check(_lib.load().vc_add_layernorm_bf16(_lib.ptr(x), _lib.ptr(residual), _lib.ptr(gamma), _lib.ptr(beta), eps, rows, C,
                                                 _lib.ptr(s), _lib.ptr(y), _lib.stream_ptr()), "vc_add_layernorm_bf16")
    return s, y


@pytest.mark.parametrize("C", U.LN_WIDTHS)
@pytest.mark.parametrize("rows", U.LN_ROWS)
def test_add_layernorm_exact(rows, C):
    """C = 8 (one live lane), 72, 384, 520 (65 chunks: ragged), 1536, 2048 (all four chunks of every lane); level-set rows plus a
    constant row, a row at 96 + 0.5 k and a row of +-2^-7, under eps = 1e-6 and 1e-5.  sum_out by bits; every element of y
    within 0.5 ulp_bf16(ref) + LN_T 2^-24 (|gamma| (1 + max |v| / sigma) + |beta|) of float64 LayerNorm of the rounded sum.
    (Measured on an MI355X: beside a rounding tie err / bound comes to 1.000 as it must, the kernel's float32 share
    (err - 0.5 ulp) / t stays at 0.14 or below.)"""
    tiny = {}
    for eps in U.LN_EPS:
        c = U.ln_case(rows, C, eps, seed=rows + C)
        x, r, gamma, beta = (c[k].to(DEV) for k in ("x", "residual", "gamma", "beta"))
        s, y = _add_layernorm(x, r, gamma, beta, eps)
        U.compare_bits(s, dict(name=c["name"] + " sum", expect_bits=c["sum_bits"]))
        err = (y.to(F64) - c["ref"].to(DEV)).abs()
        excess = float(((err - 0.5 * U.ulp_bf16(c["ref"]).to(DEV)) / c["t"].to(DEV)).max())
        print(f"{c['name']}: max err / bound = {U.bound_ratio(y, c):.3f}, float32 share (err - 0.5 ulp) / t = {excess:.3f}")
        U.compare_bound(y, c)
        assert torch.equal(y[c["const_row"]], beta)                      # a constant row: y == beta exactly
        s2, y2 = _add_layernorm(x, r, gamma, beta, eps, want_sum=False)
        assert s2 is None and torch.equal(U.bits_of(y2), U.bits_of(y))
        # the level-set rows alone (one row: one live wave of the workgroup's four)
        _, y3 = _add_layernorm(x[:rows].contiguous(), r[:rows].contiguous(), gamma, beta, eps, want_sum=False)
        assert torch.equal(U.bits_of(y3), U.bits_of(y[:rows]))
        tiny[eps] = y[c["tiny_row"]]
    assert not torch.equal(U.bits_of(tiny[1e-6]), U.bits_of(tiny[1e-5]))  # variance 2^-14: eps decides


@pytest.mark.parametrize("B,N,C", [(1, 2, 8), (3, 5, 2048), (2, 130, 520)])
def test_layernorm_drop_first_is_the_slice_of_add_layernorm(B, N, C):
    from vit_colmap_amd.vit.hip_ops import layernorm_drop_first

    g = U.gen(B + N + C)
    x = U.to_bf16(U.ln_rows(B * N, g, width=C)[0].to(F64)).to(DEV)
    gamma, beta = (U.to_bf16(U.choice(v, (C,), g)).to(DEV) for v in ((0.5, 1.0, 2.0), (-0.5, 0.0, 0.5)))
    for eps in U.LN_EPS:
        _, y = _add_layernorm(x, None, gamma, beta, eps)
        buf = _nan(B * (N - 1) + 1, C)
        layernorm_drop_first(x.reshape(B, N, C), gamma, beta, eps, out=buf[:-1].view(B, N - 1, C))
        assert torch.equal(U.bits_of(buf[:-1]).reshape(B, N - 1, C), U.bits_of(y).reshape(B, N, C)[:, 1:])
        assert not bool(torch.isnan(buf[:-1]).any()) and bool(torch.isnan(buf[-1]).all())
