"""CPU proofs behind tests/test_staged_exact_gpu.py: the exact-operand cases of util_vit_exact.py for the staged GEMMs
(vc_linear_bf16 on both tile forms, vc_patch_embed_bf16, vc_conv_taps_bf16) and for add + LayerNorm have the properties the
GPU comparisons rely on, a float32 restatement of each kernel's contract — the products added in a random order — passes the
comparator, and every single-defect mutant of it fails: a product dropped or doubled, a K tile of 64 taken twice in place of
its neighbour, two output rows exchanged, SwiGLU's gate and value exchanged in one column, pos_embed[t] in place of
pos_embed[1 + t], a convolution tap read from the neighbouring pixel.  The bounds of the cases that are not judged by bits
(SwiGLU, the float GELU, LayerNorm) are measured against the emulation here: it must stay under 0.75 of each."""
import pytest
import torch

import util_vit_exact as U

F64 = torch.float64
ROWS, KK = 37, 192            # three K tiles: a tile has a neighbour on either side


def _case(kind, epi, n_out=256, seed=3):
    return U.linear_case(ROWS, KK, n_out, kind, epi, seed=seed)


def _nonzero_product(c, row=5, col=7):
    """(row, col, k) of a non-zero product of output (row, col)."""
    k = int(torch.nonzero((c["x"][row].to(F64) * c["w"][col].to(F64)) != 0)[0])
    return row, col, k


# ---- operands -------------------------------------------------------------------------------------------------------------
def test_dense_operands_sum_exactly_in_float32():
    c = _case("dense", U.EPI_RESIDUAL)
    x, w, b, r = (c[k].to(F64) for k in ("x", "w", "b", "residual"))
    assert float(x.abs().max()) <= 2 and bool((x * 4 == torch.round(x * 4)).all())
    assert set(w.abs().unique().tolist()) == {0.25, 0.5, 1.0}
    assert bool((b * 4 == torch.round(b * 4)).all()) and bool((r * 8 == torch.round(r * 8)).all()) and float(r.abs().max()) <= 4
    prod = x[:, None, :] * w[None, :, :] * 16
    assert bool((prod == torch.round(prod)).all())
    assert U.sum_fits_float32(x.abs() @ w.abs().t() + b.abs() + r.abs(), 2.0 ** -4)
    # at K = 4096: sum |product| <= 2 * 4096 = 2^17 units of 2^-4, far below 2^24
    assert 2 * 4096 * 16 + 2 * 16 + 4 * 16 < 2 ** 20


@pytest.mark.parametrize("k,n_out", [(64, 128), (192, 384), (3072, 768), (4096, 1024)])
def test_sparse_operands_make_every_product_visible(k, n_out):
    c = U.linear_case(9, k, n_out, "sparse", U.EPI_BIAS, seed=k + n_out)
    x, w, b, h = c["x"].to(F64), c["w"].to(F64), c["b"].to(F64), c["h"]
    assert set(x.abs().unique().tolist()) <= {0.25, 0.5, 1.0} and bool(((w != 0).sum(dim=1) == U.SPARSE_NNZ).all())
    assert bool(((b * 32) % 2 == 1).all()) and float(b.abs().max()) <= 1
    U.assert_sparse_range(h)
    assert float(h.abs().min()) >= 2.0 ** -5 and float(h.abs().max()) < 8
    # every K tile of 64 holds a non-zero of some row of every 256-column tile, and the columns reach over the whole of K
    for n0 in range(0, n_out, 256):
        assert bool((w[n0:n0 + 256] != 0).any(dim=0).reshape(k // 64, 64).any(dim=1).all())
    # a dropped or doubled non-zero product moves h by an even multiple of 2^-5 that is not 0: to another bf16 number
    r, col, kk = _nonzero_product(c, 3, 11)
    for f in (-1.0, 1.0):
        moved = h[r, col] + f * x[r, kk] * w[col, kk]
        assert U.is_bf16_exact(moved) and float(moved) != float(h[r, col])


# ---- linear: the contract passes in any order, the single defects fail ----------------------------------------------------
LINEAR_FORMS = [("dense", U.EPI_BIAS), ("dense", U.EPI_RESIDUAL), ("sparse", U.EPI_BIAS), ("sparse", U.EPI_RESIDUAL),
                ("sparse", U.EPI_GELU), ("sparse", U.EPI_SWIGLU)]


@pytest.mark.parametrize("kind,epi", LINEAR_FORMS)
def test_linear_comparator_accepts_the_contract_in_any_order(kind, epi):
    c = _case(kind, epi)
    for order in range(3):
        U.compare(U.emulate_linear(c, order_seed=order), c)


@pytest.mark.parametrize("kind,epi", LINEAR_FORMS)
def test_linear_comparator_rejects_single_defects(kind, epi):
    c = _case(kind, epi)
    if kind == "sparse":
        r, col, k = _nonzero_product(c)
    else:
        # dense sums reach a few tens, where a product of 1/16 is below the bf16 ulp: take a product of at least two ulps
        term = c["x"].to(F64)[:, None, :] * c["w"].to(F64)[None, :, :]
        out = c["h"] + c["residual"].to(F64) if epi == U.EPI_RESIDUAL else c["h"]
        vis = term.abs() >= 2 * U.ulp_bf16(out.abs() + 2.0)[:, :, None]
        r, col, k = (int(v) for v in torch.nonzero(vis)[0])
    mutants = [("drop", r, col, k), ("double", r, col, k), ("ktile", 0), ("ktile", 1), ("rows", 3, 4), ("rows", 0, ROWS - 1)]
    if epi == U.EPI_SWIGLU:
        mutants += [("swiglu_swap", 9), ("swiglu_swap", 127)]
    for m in mutants:
        with pytest.raises(AssertionError):
            U.compare(U.emulate_linear(c, mutate=m), c)
    nan = U.emulate_linear(c).clone()
    nan[ROWS - 1, 1] = float("nan")
    with pytest.raises(AssertionError):
        U.compare(nan, c)


def test_todays_conv_bound_accepts_a_dropped_product():
    """The data distribution and the bound of test_vit_gpu.py::test_conv_taps_matches_float32_convolution (3 x 3 taps of 128
    channels): the 'kernel' is the float32 product with ONE product of median size missing from ONE output.  ref 2^-7 + 2e-2
    accepts it; on sparse exact operands the same defect changes the bits (test_conv_comparator)."""
    g = torch.Generator().manual_seed(1)
    rows, K, N = 64, 9 * 128, 256
    x = (torch.randn(rows, K, generator=g) * 1.2 + 0.2).to(torch.bfloat16).float()
    w = (torch.randn(N, K, generator=g) / K ** 0.5 * torch.linspace(0.5, 2.0, N)[:, None]).to(torch.bfloat16).float()
    ref = x @ w.t() + torch.randn(N, generator=g).to(torch.bfloat16).float()
    acc = ref.clone()
    r, col = 17, 200
    k = int((x[r] * w[col]).abs().argsort()[K // 2])
    dropped = float(x[r, k] * w[col, k])
    assert abs(dropped) > 5e-3
    acc[r, col] -= dropped
    out = acc.to(torch.bfloat16).float()
    assert bool(((out - ref).abs() <= ref.abs() * 2 ** -7 + 2e-2).all())


# ---- the bounds of the epilogues that are not judged by bits --------------------------------------------------------------
def test_swiglu_emulation_stays_inside_its_bound():
    """The float32 emulation (torch exp2 and reciprocal, three summation orders, two widths) against ulp_bf16(ref) + 2^-20 (1 +
    |a|) |ref|: the largest err / bound is recorded in linear_case's docstring.  Under 0.75: the float32 term stays as derived."""
    worst = 0.0
    for n_out, seed in ((256, 1), (768, 2)):
        c = U.linear_case(129, KK, n_out, "sparse", U.EPI_SWIGLU, seed=seed)
        for order in range(3):
            worst = max(worst, U.bound_ratio(U.emulate_linear(c, order_seed=order), c))
        # beside the ulp term the float32 term is small: the bound stays a one-ulp bound
        assert float((c["bound"] / U.ulp_bf16(c["ref"])).max()) < 1.01
    print(f"SwiGLU float32 emulation: max err / bound = {worst:.3f}")
    assert worst <= 0.75, worst


def test_gelu_emulation_stays_inside_its_bound():
    """The float path's bound is the project's own (xs_case(gelu_float=True)): its first term, 2^-8 |ref|, is between half a
    bf16 ulp and a whole one, so the rounding alone reaches err / bound close to 1 just above a power of two (0.84 here)."""
    c = _case("sparse", U.EPI_GELU)
    worst = max(U.bound_ratio(U.emulate_linear(c, order_seed=o), c) for o in range(3))
    print(f"GELU float path, float32 emulation: max err / bound = {worst:.3f}")
    assert worst <= 1.0, worst


# ---- patch embedding ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,n_out,k_in", [(5, 10, 128, 128), (7, 1, 128, 64)])
def test_patch_comparator(B, T, n_out, k_in):
    c = U.patch_case(B, T, n_out, k_in, seed=B + T)
    pos = c["pos"].to(F64)
    assert bool((pos * 8 == torch.round(pos * 8)).all()) and float(pos.abs().max()) <= 4
    for order in range(3):
        U.compare(U.emulate_patch(c, order_seed=order), c)
    assert not torch.equal(c["pos"][1:], c["pos"][:-1])
    with pytest.raises(AssertionError):
        U.compare(U.emulate_patch(c, mutate=("pos",)), c)
    with pytest.raises(AssertionError):
        U.compare(_rows_swapped(U.emulate_patch(c), 0, B * T - 1), c)
    if k_in > 64:
        with pytest.raises(AssertionError):
            U.compare(U.emulate_patch(c, mutate=("ktile", 0)), c)


def _rows_swapped(out, r1, r2):
    flat = out.clone().reshape(-1, out.shape[-1])
    flat[[r1, r2]] = flat[[r2, r1]]
    return flat.reshape(out.shape)


# ---- convolution ----------------------------------------------------------------------------------------------------------
CONV_GEOMETRIES = [(2, 5, 7, 64, 256, 3, 3, -1, -1), (1, 6, 5, 64, 256, 4, 4, -1, -2), (1, 12, 11, 64, 256, 1, 1, -8, 0),
                   (1, 12, 11, 64, 256, 1, 1, 0, 8), (2, 4, 3, 128, 256, 2, 2, 0, 0)]


@pytest.mark.parametrize("geo", CONV_GEOMETRIES)
@pytest.mark.parametrize("kind,epi", [("dense", U.EPI_BIAS), ("sparse", U.EPI_BIAS), ("sparse", U.EPI_GELU)])
def test_conv_comparator(geo, kind, epi):
    B, H, W, C, N, kh, kw, dy0, dx0 = geo
    c = U.conv_case(*geo, kind, epi, seed=sum(geo) + epi)
    assert c["x_rows"].shape == (B * H * W + 1, C) and bool(c["x_rows"][-1].any()), "the spare row holds junk"
    for order in range(2):
        U.compare(U.emulate_conv(c, order_seed=order), c)
    # torch's own float64 convolution agrees with the gather (every sum is exact in float64, so: equality)
    img = c["x_rows"][:-1].to(F64).reshape(B, H, W, C).permute(0, 3, 1, 2)
    pad = (max(-dx0, 0), max(kw - 1 + dx0, 0), max(-dy0, 0), max(kh - 1 + dy0, 0))
    full = torch.nn.functional.conv2d(torch.nn.functional.pad(img, pad), c["w"].to(F64).reshape(N, kh, kw, C).permute(0, 3, 1, 2), c["b"].to(F64))
    oy, ox = max(dy0, 0), max(dx0, 0)                                    # a window that starts inside the image: crop
    assert torch.equal(full[:, :, oy:oy + H, ox:ox + W].permute(0, 2, 3, 1).reshape(B * H * W, N), c["h"])
    if kh == 1 and abs(dy0) + abs(dx0) == 8:
        # rows nearer than 8 to that edge are the bias alone
        hh = c["h"].reshape(B, H, W, N)
        edge = hh[:, :8] if dy0 == -8 else hh[:, :, W - 8:]
        assert torch.equal(edge, c["b"].to(F64).expand_as(edge))
    for t in {0, kh * kw - 1}:
        with pytest.raises(AssertionError):
            U.compare(U.emulate_conv(c, mutate=("tap", t)), c)
    with pytest.raises(AssertionError):
        U.compare(U.emulate_conv(c, mutate=("rows", 0, B * H * W - 1)), c)
    if kind == "sparse":
        cols = U.conv_gather(c["x_rows"][:-1].to(F64).reshape(B, H, W, C), kh, kw, dy0, dx0)
        r, k = (int(v) for v in torch.nonzero((cols * c["w"][3].to(F64)) != 0)[-1])
        for kind_m in ("drop", "double"):
            if epi == U.EPI_BIAS:
                with pytest.raises(AssertionError):
                    U.compare(U.emulate_conv(c, mutate=(kind_m, r, 3, k)), c)


# ---- add + LayerNorm ------------------------------------------------------------------------------------------------------
def test_ln_rows_take_a_width():
    for C in U.LN_WIDTHS:
        x, si, sc = U.ln_rows(20, U.gen(C), width=C)
        assert x.shape == (20, C) and U.is_bf16_exact(x)
        for row, s, a in zip(x, si, sc):
            lv = U.LEVEL_SETS[int(s)]
            assert sorted(row.tolist()) == sorted(v * float(a) for v in lv for _ in range(C // len(lv)))
    assert U.ln_rows(3, U.gen(1))[0].shape == (3, U.K)


def test_layernorm_emulation_stays_inside_its_bound():
    """The float32 emulation of add_layernorm_kernel's sequence over every width, row count and eps of the GPU test: y within
    0.5 ulp + the float32 term t with constant LN_T.  The rounding to bf16 alone costs half an ulp beside a tie, so err / bound
    of the rounded values comes arbitrarily close to 1 whatever t is; what t has to cover is the float32 error BEFORE that
    rounding, and that must stay under 0.75 t.  The largest ratio is recorded beside LN_T."""
    worst, where = 0.0, None
    for C in U.LN_WIDTHS:
        for rows in U.LN_ROWS:
            for eps in U.LN_EPS:
                c = U.ln_case(rows, C, eps, seed=rows + C)
                y = U.emulate_layernorm(c)
                U.compare_bound(y, c)
                assert torch.equal(y[c["const_row"]].to(F64), c["beta"].to(F64))
                ratio = float(((U.emulate_layernorm(c, rounded=False).to(F64) - c["ref"]).abs() / c["t"]).max())
                if ratio > worst:
                    worst, where = ratio, c["name"]
    print(f"LayerNorm float32 emulation with LN_T = {U.LN_T}: max |y32 - ref| / t = {worst:.3f} at {where}")
    assert worst <= 0.75, (worst, where)


@pytest.mark.parametrize("C", [8, 520, 2048])
def test_layernorm_case_properties_and_sharpness(C):
    c5, c6 = (U.ln_case(5, C, eps, seed=5 + C) for eps in (1e-5, 1e-6))
    assert torch.equal(c5["x"], c6["x"]) and c5["x"].shape == (8, C)
    x, r = c6["x"].to(F64), c6["residual"].to(F64)
    assert bool((r * 8 == torch.round(r * 8)).all())
    assert set(c6["gamma"].to(F64).unique().tolist()) <= {0.5, 1.0, 2.0} and set(c6["beta"].to(F64).unique().tolist()) <= {-0.5, 0.0, 0.5}
    assert bool(((x + r)[c6["const_row"]] == 3.0).all())
    off = x[c6["offset_row"]]
    assert float(off.min()) >= 94.5 and float(off.max()) <= 97.5 and bool((off * 2 == torch.round(off * 2)).all())
    assert bool((x[c6["tiny_row"]].abs() == 2.0 ** -7).all())
    # the +-2^-7 row gives different bits under the two eps, in the reference and in the emulation
    t = c6["tiny_row"]
    assert not torch.equal(U.bf16_rne(c5["ref"][t]), U.bf16_rne(c6["ref"][t]))
    y5, y6 = U.emulate_layernorm(c5), U.emulate_layernorm(c6)
    assert not torch.equal(y5[t], y6[t])
    with pytest.raises(AssertionError):
        U.compare_bound(U.emulate_layernorm(c6, mutate=("eps", 1e-5)), c6)
    with pytest.raises(AssertionError):
        U.compare_bound(y5, c6)
    # the last chunk left out of the statistics (the ragged chunk count at C = 520: chunk 64 is lane 0's second)
    with pytest.raises(AssertionError):
        U.compare_bound(U.emulate_layernorm(c6, mutate=("skip_chunk", C // 8 - 1)), c6)
    nan = y6.clone()
    nan[0, C - 1] = float("nan")
    with pytest.raises(AssertionError):
        U.compare_bound(nan, c6)
