"""CPU proofs behind tests/test_vit_exact_gpu.py: the exact-operand constructions of util_vit_exact.py have the properties the
GPU comparisons rely on, and the comparators are sharp — they accept a float32 restatement of each kernel's contract and
reject every single-defect mutation of it, three of which the tolerances of tests/test_vit_gpu.py accept.

Constructions (all bf16-exact):
  LayerNorm rows   K = 384 values from one level set with equal counts, times a scale, permuted.  The normalised values sit
                   >= 0.11 bf16 ulp from a rounding tie, so the kernel's float32 statistics and float64 round to the same bf16.
  weights          W in multiples of 1/4, gamma in {1/2, 1, 2}, beta in {-1/2, 0, 1/2}: W gamma and W beta are exact, every
                   product is a multiple of 2^-12 and sum |product| < 2^12, so every partial sum in every order is a float32
                   number and the float32 accumulator holds the float64 result.
  attention        q[i] = 8 onehot(dim of the group i asks for); k[j, e] = 0 where j belongs to the group on dimension e, else
                   -128: q.k is 0 inside the group and -1024 outside, a weight of 2^-1024 (q_prescaled) or e^-128, both 0
                   in float32.  v[j, d] = 2^((j // 64) % 4) at d = j % 64: an output row is a code of the keys counted.
"""
import pytest
import torch

import util_vit_exact as U

F64 = torch.float64


# ---- LayerNorm rows -------------------------------------------------------------------------------------------------------
XHAT_VALUES = {1.0, -1.0, 229 / 512, -229 / 512, 43 / 32, -43 / 32, -119 / 128, -143 / 256, -95 / 512, 107 / 64}


def _rows_of(levels, scale):
    return (torch.tensor(levels, dtype=F64).repeat(U.K // len(levels)) * scale)[None, :]


@pytest.mark.parametrize("levels", U.LEVEL_SETS)
@pytest.mark.parametrize("scale", U.SCALES)
def test_layernorm_rows_round_one_way(levels, scale):
    x = _rows_of(levels, scale)
    assert U.is_bf16_exact(x)
    assert not bool((x == x.mean()).any()), "a level equals the row mean: its x-hat is a float32 residue, not 0"
    y64 = U.xhat_f64(x)
    y32 = U.xhat_f32_kernel_sequence(x).to(F64)
    m64, m32 = float(U.tie_margin(y64).min()), float(U.tie_margin(y32).min())
    print(f"levels {levels} scale {scale}: tie margin {m64:.3f} (float64) {m32:.3f} (float32 sequence) bf16 ulp")
    assert m64 >= 0.05 and m32 >= 0.05
    b64, b32 = U.bf16_rne(y64), U.bf16_rne(y32)
    assert torch.equal(b64, b32)
    assert set(b64.reshape(-1).tolist()) <= XHAT_VALUES
    # ... and a few float32 ulps of difference in the statistics (another summation order, a 1-ulp rsqrt) change nothing
    for rel in (-4 * 2.0 ** -23, 4 * 2.0 ** -23):
        assert torch.equal(U.bf16_rne(y32 * (1 + rel)), b64)


def test_level_set_with_a_level_at_the_mean_is_refused():
    x = _rows_of((-2, 0, 1, 5), 1.0)
    assert bool((x == x.mean()).any())


def test_rows_of_one_launch_mix_every_set_and_scale():
    x, si, sc = U.ln_rows(45, U.gen(1))
    assert len({(int(a), float(b)) for a, b in zip(si, sc)}) == len(U.LEVEL_SETS) * len(U.SCALES)
    assert U.is_bf16_exact(x)
    for row, s, a in zip(x, si, sc):
        want = sorted(v * float(a) for v in U.LEVEL_SETS[int(s)] for _ in range(U.K // len(U.LEVEL_SETS[int(s)])))
        assert sorted(row.tolist()) == want
    assert set(U.xhat_bf16(x).reshape(-1).tolist()) == XHAT_VALUES
    big, _, _ = U.ln_rows(5000, U.gen(2))
    assert big.shape == (5000, U.K) and torch.unique(big, dim=0).shape[0] >= 2048 - 8


# ---- weights: exact folding, order independence ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["dense", "sparse"])
@pytest.mark.parametrize("ln", [False, True])
@pytest.mark.parametrize("epi", [U.EPI_BIAS, U.EPI_RESIDUAL])
def test_xs_sums_are_exact_in_float32_in_any_order(kind, ln, epi):
    c = U.xs_case(45, 96, kind, ln, epi, seed=7)
    w, gam, bet = c["w"].to(F64), c["gamma"], c["beta"]
    assert bool((w * 4 == torch.round(w * 4)).all())
    if ln:
        assert U.is_bf16_exact(w * gam.to(F64))
        # W beta: multiples of 1/8 below 2^8, and the folded bias the prepare step computes in float32 is the exact one
        assert torch.equal((c["b"] + (c["w"] * bet).sum(dim=1)).to(F64), c["b_folded"])
        assert torch.equal(c["b"].to(F64) + w @ bet.to(F64), c["b_folded"])
    # products are multiples of 2^-12 (x-hat: 2^-9, W gamma: 2^-3) or of 2^-5 (raw rows: 2^-2); sum |product| + |bias|
    # + |residual| stays below 2^24 units: every partial sum, in any order, is a float32 number
    unit = 2.0 ** -12 if ln or kind == "sparse" else 2.0 ** -5
    prod_unit = (c["xin"][:, None, :] * c["wg"][None, :, :]) / unit
    assert bool((prod_unit == torch.round(prod_unit)).all()) and bool((c["b_folded"] / unit == torch.round(c["b_folded"] / unit)).all())
    total = c["xin"].abs() @ c["wg"].abs().t() + c["b_folded"].abs() + (0 if c["residual"] is None else c["residual"].to(F64).abs())
    assert U.sum_fits_float32(total, unit)
    for order in range(3):
        U.compare(U.emulate_xs(c, order_seed=order), c)
    if kind == "dense":
        assert torch.unique(c["wg"], dim=0).shape[0] == 96
    else:
        assert bool(((c["wg"] != 0).sum(dim=1) == 8).all()) and bool((c["wg"].abs() <= 0.5).all())
        odd = c["b_folded"] * 2.0 ** 12
        assert bool((odd % 2 == 1).all()) and bool((c["b_folded"].abs() <= 1).all())


def test_sparse_pre_activations_stay_inside_the_gelu_table():
    tab = U.host_gelu_table()
    c = U.xs_case(300, 1536, "sparse", True, U.EPI_GELU, seed=3, table=tab)
    h = c["h"]
    assert float(h.abs().min()) >= 2.0 ** -12 and float(h.abs().max()) < 8.0
    for order in range(3):
        U.compare(U.emulate_xs(c, table=tab, order_seed=order), c)


# ---- x-stationary GEMM: sharpness -----------------------------------------------------------------------------------------
def _visible_term(c):
    """A product of the case that is at least two bf16 ulps of its output: dropping or doubling it must change the bits."""
    term = c["xin"][:, None, :] * c["wg"][None, :, :]
    out = c["h"] if c["residual"] is None else c["h"] + c["residual"].to(F64)
    vis = term.abs() >= 2 * torch.maximum(U.ulp_bf16(out), U.ulp_bf16(out.abs() + term.abs().amax(dim=2)))[:, :, None]
    assert bool(vis.any())
    return tuple(int(v) for v in torch.nonzero(vis)[0])


@pytest.mark.parametrize("kind,ln,epi", [("dense", True, U.EPI_BIAS), ("dense", False, U.EPI_RESIDUAL), ("sparse", True, U.EPI_RESIDUAL),
                                         ("sparse", True, U.EPI_GELU)])
def test_xs_comparator_rejects_a_dropped_and_a_doubled_term(kind, ln, epi):
    tab = U.host_gelu_table()
    c = U.xs_case(45, 96, kind, ln, epi, seed=11, table=tab)
    U.compare(U.emulate_xs(c, table=tab), c)
    if epi == U.EPI_GELU:
        # the table is constant over stretches of h (|gelu'| < 1 below 0): take a term that moves the looked-up value
        term = c["xin"][:, None, :] * c["wg"][None, :, :]
        moved = U.table_gelu(U.bf16_rne(c["h"][:, :, None] - term), tab) != U.table_gelu(U.bf16_rne(c["h"]), tab)[:, :, None]
        moved &= U.table_gelu(U.bf16_rne(c["h"][:, :, None] + term), tab) != U.table_gelu(U.bf16_rne(c["h"]), tab)[:, :, None]
        r, col, k = (int(v) for v in torch.nonzero(moved & (term != 0))[0])
    else:
        r, col, k = _visible_term(c)
    for kind_m in ("drop", "double"):
        with pytest.raises(AssertionError):
            U.compare(U.emulate_xs(c, table=tab, mutate=(kind_m, r, col, k)), c)
    nan = U.emulate_xs(c, table=tab).clone()
    nan[3, 5] = float("nan")
    with pytest.raises(AssertionError):
        U.compare(nan, c)


def test_todays_xs_bound_accepts_a_dropped_term():
    """The distribution of the data (drawn here on the CPU) and the three assertions of
    test_xs_linear_matches_float32_reference at (300, 384), LayerNorm on; the 'kernel'
    is the bf16-operand contract with ONE product missing from ONE output.  It passes: that bound cannot see the defect."""
    g = torch.Generator().manual_seed(300 + 384 + 7)
    rows, n = 300, 384
    x = (torch.randn(rows, U.K, generator=g) * 1.5 + 0.3).to(torch.bfloat16)
    w = torch.randn(n, U.K, generator=g) / U.K ** 0.5 * torch.linspace(0.5, 2.0, n)[:, None]
    b = torch.randn(n, generator=g)
    gam = 1 + 0.2 * torch.randn(U.K, generator=g)
    bet = 0.1 * torch.randn(U.K, generator=g)
    ref = torch.nn.functional.layer_norm(x.float(), (U.K,), gam, bet, 1e-6) @ w.t() + b
    xh = U.xhat_f32_kernel_sequence(x).to(torch.bfloat16).float()
    wg = (w * gam).to(torch.bfloat16).float()
    acc = xh @ wg.t() + (b + w @ bet)
    # the product of median size of output (17, 200): a few hundredths, like most of its 384 terms
    r, col = 17, 200
    k = int((xh[r] * wg[col]).abs().argsort()[U.K // 2])
    dropped = float(xh[r, k] * wg[col, k])
    assert 0.01 < abs(dropped) < 6e-2
    acc[r, col] -= dropped
    out = acc.to(torch.bfloat16).float()
    err = (out - ref).abs()
    tol = ref.abs() * 2 ** -7 + 6e-2
    assert bool((err <= tol).all())
    assert float((err > ref.abs() * 2 ** -7 + 3e-2).float().mean()) < 1e-5
    assert float((out - ref).norm() / ref.norm()) < 6e-3


# ---- fused MLP ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mlp_cases():
    tab = U.host_gelu_table()
    return {fb: U.mlp_case(70, 192, seed=5, table=tab, float_blocks=fb) for fb in (False, True)}


def test_mlp_construction(mlp_cases):
    for fb, c in mlp_cases.items():
        p = c["p"]
        assert bool(((p["w2"] != 0).sum(dim=1) == U.W2_NNZ).all())
        assert bool(((p["w2"] != 0).sum(dim=0) >= 1).all()), "a hidden unit feeds no output"
        assert set(p["w2"].abs().unique().tolist()) == {0.0, 0.25, 0.5, 1.0}
        assert U.is_bf16_exact(p["b2"]) and U.is_bf16_exact(p["w1g"]) and U.is_bf16_exact(c["x"].to(F64))
        assert torch.equal((p["b1"].float() + (p["w1"].float() * p["beta"].float()).sum(dim=1)).to(F64), p["b1_folded"])
        frac = float(c["fblock"].float().mean())
        if fb:
            # chunk 0: a unit at +16; chunk 3: a unit at h == 0; both on every row block
            assert bool(c["fblock"][:, 0].all()) and bool(c["fblock"][:, 3].all()) and int(c["fblock"].sum()) == 2 * c["fblock"].shape[0]
            assert 0.25 <= frac <= 0.75
        else:
            assert frac == 0.0
    # beside the ulp term the derived bound stays below 1e-3 (0.12 today); the float-path widening is one ulp of g per unit
    c = mlp_cases[False]
    assert float((c["bound"] - 2.0 ** -8 * c["ref"].abs()).max()) < 1e-3
    cf = mlp_cases[True]
    widening = cf["bound"] - 2.0 ** -8 * cf["ref"].abs()
    fmask = cf["fblock"][:, None, :, None].expand(-1, 32, -1, 32).reshape(-1, 192)[:70]
    assert float((widening - (U.ulp_bf16(cf["g"]) * fmask) @ cf["p"]["w2"].abs().t()).max()) < 1e-3


@pytest.mark.parametrize("fb", [False, True])
def test_mlp_comparator_accepts_the_contract_in_any_order(mlp_cases, fb):
    for order in range(3):
        U.compare(U.emulate_mlp(mlp_cases[fb], order_seed=order), mlp_cases[fb])


def _sharpest(c, delta_per_unit):
    """(row, unit, output) where a change of the activation by delta_per_unit[row, unit] moves the output furthest beyond
    its bound; asserts that it is at least three bounds (the mutant's own bf16 rounding moves it by at most one)."""
    w2 = c["p"]["w2"]
    ratio = delta_per_unit[:, None, :] * w2.abs()[None, :, :] / c["bound"][:, :, None]      # [rows][out][hidden]
    flat = int(ratio.argmax())
    r, rest = divmod(flat, ratio.shape[1] * ratio.shape[2])
    o, u = divmod(rest, ratio.shape[2])
    assert float(ratio[r, o, u]) >= 3.0, float(ratio[r, o, u])
    return r, u, o


def test_mlp_comparator_rejects_single_defects(mlp_cases):
    c, cf = mlp_cases[False], mlp_cases[True]
    w2 = c["p"]["w2"]
    # two W2 k indices exchanged: one that output 0 uses and one that it does not
    k1, k2 = int(torch.nonzero(w2[0] != 0)[0]), int(torch.nonzero(w2[0] == 0)[0])
    with pytest.raises(AssertionError):
        U.compare(U.emulate_mlp(c, mutate=("swap_w2", k1, k2)), c)
    # one table entry one bf16 ulp up
    r, u, _ = _sharpest(c, U.ulp_bf16(c["g"]))
    hb = U.bf16_rne(U.xhat_bf16(c["x"].to(F64)) @ c["p"]["w1g"].t() + c["p"]["b1_folded"])
    k, sign, ok = U.table_index(U.f64_to_bits(hb[r, u]))
    assert bool(ok)
    with pytest.raises(AssertionError):
        U.compare(U.emulate_mlp(c, mutate=("table", int(k), int(sign))), c)
    # one hidden activation wrong by 1.0
    r, u, _ = _sharpest(c, torch.ones_like(c["g"]))
    with pytest.raises(AssertionError):
        U.compare(U.emulate_mlp(c, mutate=("act", r, u, 1.0)), c)
    # a float-path block answered from the table (the clamped index reads the last entry, gelu(7.97), for 16 and for 0)
    with pytest.raises(AssertionError):
        U.compare(U.emulate_mlp(cf, mutate=("float_from_table",)), cf)
    nan = U.emulate_mlp(c).clone()
    nan[69, 383] = float("nan")
    with pytest.raises(AssertionError):
        U.compare(nan, c)


def test_todays_mlp_bound_accepts_an_activation_off_by_one():
    """The distribution of the data (drawn here on the CPU) and the two assertions of tests/test_vit_gpu.py _check_fused_mlp
    (127 rows, hidden 1536); the 'kernel' is the
    bf16 contract with ONE hidden activation wrong by 1.0.  Every output of that row moves by |w2| ~ 0.03: accepted."""
    rows, Hd, K = 127, 1536, U.K
    g = torch.Generator().manual_seed(rows)
    x = (torch.randn(rows, K, generator=g) * 1.5 + 0.3).to(torch.bfloat16)
    w1 = torch.randn(Hd, K, generator=g) / K ** 0.5 * torch.linspace(0.5, 2.0, Hd)[:, None]
    b1 = 0.5 * torch.randn(Hd, generator=g)
    w2 = torch.randn(K, Hd, generator=g) / Hd ** 0.5 * torch.linspace(0.5, 1.5, K)[:, None]
    b2 = torch.randn(K, generator=g)
    gam = 1 + 0.2 * torch.randn(K, generator=g)
    bet = 0.1 * torch.randn(K, generator=g)
    xin = x.float()
    h = torch.nn.functional.layer_norm(xin, (K,), gam, bet, 1e-6) @ w1.t() + b1
    hg = torch.nn.functional.gelu(h.to(torch.bfloat16).float()).to(torch.bfloat16).float()
    ref = xin + hg @ w2.t() + b2
    xh = U.xhat_f32_kernel_sequence(x).to(torch.bfloat16).float()
    hk = xh @ (w1 * gam).to(torch.bfloat16).float().t() + (b1 + w1 @ bet)
    gk = torch.nn.functional.gelu(hk.to(torch.bfloat16).float()).to(torch.bfloat16).float()
    gk[60, 700] += 1.0
    out = (gk @ w2.to(torch.bfloat16).float().t() + b2 + xin).to(torch.bfloat16).float()
    err = (out - ref).abs()
    assert float(w2[:, 700].abs().max()) > 0.03
    assert float((out - ref).norm() / ref.norm()) < 8e-3
    assert bool((err <= ref.abs() * 2 ** -6 + 0.12).all())


# ---- attention ------------------------------------------------------------------------------------------------------------
ATT_SHAPES = [(1, 100, 2), (1, 520, 2), (2, 300, 5)]


@pytest.fixture(scope="module")
def att_cases():
    return {s: U.attention_case(*s, seed=sum(s)) for s in ATT_SHAPES}


@pytest.mark.parametrize("shape", ATT_SHAPES + [(1, 1531, 1)])
@pytest.mark.parametrize("fast", [False, True])
def test_attention_closed_form(shape, fast, att_cases):
    c = (None if fast else att_cases.get(shape)) or U.attention_case(*shape, seed=sum(shape), fast_pass=fast)
    N = shape[1]
    sizes = [len(s) for s in c["groups"]]
    assert set(sizes) <= {32, 64} and len(sizes) == (5 if N >= 128 and not fast else 4)
    assert c["groups"][1][-1] == N - 1 and N - 1 in c["groups"][3]
    # which pass stores the result under q_prescaled: the default cases hold groups with no key in block 0 from N = 128 on
    # (every unit goes to the exact pass), the fast_pass cases none — and still reach the ragged last key block
    assert U.leaves_fast_pass(c["groups"]) == (N >= 128 and not fast)
    assert all(min(s) < 64 for s in c["groups"]) == (fast or N < 128)
    assert len(set(c["groups"][1]) & set(range(N - 63, N))) == 63
    assert U.is_bf16_exact(c["exact"]) and U.is_bf16_exact(c["qkv"].to(F64))
    for pre in (True, False):
        assert float((U.attention_softmax_f64(c, pre) - c["exact"]).abs().max()) <= 1e-12
    # every unit of 128 queries asks for every group
    for u0 in range(0, N, 128):
        if u0 + len(sizes) <= N:
            assert set(c["ask"][0, 0, u0:u0 + 128].tolist()) == set(range(len(sizes)))


@pytest.mark.parametrize("fast", [False, True])
def test_attention_odd_group_is_judged_at_one_ulp(fast):
    c = U.attention_case(1, 300, 2, seed=9, odd_group=True, fast_pass=fast)
    assert [len(s) for s in c["groups"]] == [48, 64, 64, 32] + [32] * (not fast)
    assert float((U.attention_softmax_f64(c, True) - c["ref"]).abs().max()) <= 1e-12
    rows48 = c["ask"][0, 0] == 0
    assert bool((c["bound"][0, rows48, :64].amax(dim=1) > 0).all()) and float(c["bound"][0, ~rows48, :64].max()) == 0.0
    for pre in (True, False):
        U.compare(U.emulate_attention(c, pre), c)
    row = int(torch.nonzero(rows48)[0])
    with pytest.raises(AssertionError):
        U.compare(U.emulate_attention(c, True, mutate=("drop", 0, 0, row, 30)), c)
    with pytest.raises(AssertionError):
        U.compare(U.emulate_attention(c, True, mutate=("extra", 0, 0, row, 299)), c)


@pytest.mark.parametrize("shape", ATT_SHAPES)
@pytest.mark.parametrize("pre", [True, False])
@pytest.mark.parametrize("fast", [False, True])
def test_attention_comparator_is_sharp(shape, pre, fast, att_cases):
    c = U.attention_case(*shape, seed=sum(shape), fast_pass=True) if fast else att_cases[shape]
    U.compare(U.emulate_attention(c, pre), c)
    B, N, H = shape
    b, h = B - 1, H - 1
    for grp in range(len(c["groups"])):
        row = int(torch.nonzero(c["ask"][b, h] == grp)[-1])
        keys = c["groups"][grp]
        outside = next(j for j in range(N - 1, -1, -1) if j not in keys)
        for mutate in (("drop", b, h, row, keys[0]), ("drop", b, h, row, keys[-1]), ("double", b, h, row, keys[len(keys) // 2]),
                       ("extra", b, h, row, outside)):
            with pytest.raises(AssertionError):
                U.compare(U.emulate_attention(c, pre, mutate=mutate), c)


def test_todays_attention_bounds_accept_an_extra_key_with_zero_v(att_cases):
    """N = 520: a key from outside the group counted in one row's sum (zero V: nothing else sees it) scales that row by 64/65,
    every value of it by a bf16 ulp or two — far under max-abs 3e-2 and rel-L2 1e-2, the bounds of
    test_attention_prescaled_q_lazy_max.  The new comparison rejects it (test_attention_comparator_is_sharp)."""
    c = att_cases[(1, 520, 2)]
    ref = U.attention_softmax_f64(c, True)
    row = 519
    assert int(c["ask"][0, 1, row]) == 0 and 300 not in c["groups"][0]
    out = U.emulate_attention(c, True, mutate=("extra", 0, 1, row, 300)).to(F64)
    err = (out - ref).abs()
    assert float(err.max()) > 0 and int((err.reshape(520, 128) > 1e-12).any(dim=1).sum()) == 1
    assert float(err.max()) < 3e-2 and float((out - ref).norm() / ref.norm()) < 1e-2
    with pytest.raises(AssertionError):
        U.compare(out, c)
