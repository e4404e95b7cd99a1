"""Exact-operand cases for the ViT kernels (x-stationary GEMM, fused MLP, attention; the staged GEMMs behind vc_linear_bf16,
vc_patch_embed_bf16 and vc_conv_taps_bf16; add + LayerNorm) and their comparators.

The kernels' documented arithmetic is bf16 operands, float32 accumulation, bf16 results.  The operands built here are
chosen so that this arithmetic has ONE possible result: every product and every partial sum is exactly representable in
float32 in whatever order it is taken, LayerNorm outputs sit far from a bf16 rounding tie, softmax weights are exactly 1 or
0.  A comparison is then bit equality, or a bound derived per element (fused MLP: its second product sums rounded GELU
values).  Everything is torch float64 on the device of the inputs; the random draws are made on the CPU from a seed, so a
case is the same wherever it is built.

Comparators take (got, case) and raise AssertionError on a mismatch; `got` is a bf16 tensor (or its bit patterns).
The float32 emulations (emulate_*) restate a kernel's contract step by step on the CPU in float32 and take single-defect
mutations; tests/test_vit_exact_spec.py and tests/test_staged_exact_spec.py prove with them that the comparators accept the
contract and reject the defects.
"""
import math

import numpy as np
import torch

K = 384                       # width of the residual stream (the K of every kernel here)
EPS = 1e-6
LEVEL_SETS = ((-1, 1), (-3, -1, 1, 3), (0, 2, 4, 6), (-1, 1, 3, 5), (0, 1, 2, 7))
SCALES = (0.25, 1.0, 8.0)
EPI_BIAS, EPI_GELU, EPI_RESIDUAL = 0, 1, 2

GT_LO = (127 - 14) << 7       # gemm.hip kGtLo: bf16 bits of 2^-14, the table's first magnitude
GT_N = 17 * 128               # gemm.hip kGtN: magnitudes covered, [2^-14, 8)
F64 = torch.float64


# ---- bf16 on float64 values ---------------------------------------------------------------------------------------------
def ulp_bf16(x: torch.Tensor) -> torch.Tensor:
    """Spacing of bf16 at |x| (float64): 2^(e - 7), e = floor(log2 |x|) clamped to the smallest normal exponent."""
    # (on the float64 bit pattern: integer operations only, the same on every device)
    e = ((x.to(F64).abs().clamp_min(2.0 ** -126).contiguous().view(torch.int64) >> 52) & 0x7FF) - 1023
    return ((e - 7 + 1023) << 52).view(F64)


def bf16_rne(x: torch.Tensor) -> torch.Tensor:
    """float64 -> the nearest bf16 value (ties to even), as float64: one rounding, never through float32."""
    x = x.to(F64)
    u = ulp_bf16(x)
    return torch.round(x / u) * u                                       # torch.round: half to even; the scalings are exact


def tie_margin(x: torch.Tensor) -> torch.Tensor:
    """Distance of x (float64) from the nearest bf16 rounding tie, in bf16 ulps (0.5 = x is a bf16 value)."""
    q = x.to(F64) / ulp_bf16(x)
    return ((q - torch.floor(q)) - 0.5).abs()


def is_bf16_exact(x: torch.Tensor) -> bool:
    return bool((bf16_rne(x) == x.to(F64)).all())


def to_bf16(x: torch.Tensor) -> torch.Tensor:
    """bf16-exact float64 values -> a bf16 tensor (asserted exact)."""
    y = x.to(torch.float32).to(torch.bfloat16)
    assert bool((y.to(F64) == x.to(F64)).all()), "value is not a bf16 number"
    return y


def bits_of(t: torch.Tensor) -> torch.Tensor:
    """bf16 tensor (or integer bit patterns) -> int32 bit patterns 0..65535."""
    if t.dtype == torch.bfloat16:
        return t.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
    return t.to(torch.int32) & 0xFFFF


def bits_to_f64(bits: torch.Tensor) -> torch.Tensor:
    return (bits.to(torch.int32) << 16).view(torch.float32).to(F64)


def f64_to_bits(x: torch.Tensor) -> torch.Tensor:
    return bits_of(to_bf16(x))


def gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def choice(values, shape, g: torch.Generator) -> torch.Tensor:
    v = torch.tensor(values, dtype=F64)
    return v[torch.randint(0, len(values), shape, generator=g)]


# ---- LayerNorm rows -----------------------------------------------------------------------------------------------------
def ln_rows(rows: int, g: torch.Generator, level_sets=LEVEL_SETS, scales=SCALES, pool: int = 2048, width: int = K):
    """[rows][width] float32 (bf16-exact values): each row = one level set (equal counts), one scale, one random permutation.
    More than `pool` rows are drawn (with a random, non-periodic index) from a pool of that many distinct rows.
    width: 384, the K of the GEMM cases, or any multiple of 4 (the level sets hold 2 or 4 levels).
    -> (x, set index, scale)."""
    K = width
    n = min(rows, pool)
    si = torch.randint(0, len(level_sets), (n,), generator=g)
    sc = torch.tensor(scales, dtype=F64)[torch.randint(0, len(scales), (n,), generator=g)]
    if n >= len(level_sets) * len(scales):                             # every (set, scale) pair is present
        pairs = torch.arange(len(level_sets) * len(scales))
        si[: len(pairs)] = pairs // len(scales)
        sc[: len(pairs)] = torch.tensor(scales, dtype=F64)[pairs % len(scales)]
    base = torch.empty(n, K, dtype=F64)
    for s, lv in enumerate(level_sets):
        assert K % len(lv) == 0
        base[si == s] = torch.tensor(lv, dtype=F64).repeat(K // len(lv))
    perm = torch.rand(n, K, generator=g).argsort(dim=1)
    x = (torch.gather(base, 1, perm) * sc[:, None]).float()             # (exact; half the bytes for the long cases)
    if rows > n:
        pick = torch.randint(0, n, (rows,), generator=g)
        pick[:n] = torch.arange(n)
        x, si, sc = x[pick], si[pick], sc[pick]
    return x, si, sc


def xhat_f64(x: torch.Tensor, eps: float = EPS) -> torch.Tensor:
    x = x.to(F64)
    d = x - x.mean(dim=1, keepdim=True)
    return d / torch.sqrt((d * d).mean(dim=1, keepdim=True) + eps)


def xhat_f32_kernel_sequence(x: torch.Tensor, eps: float = EPS) -> torch.Tensor:
    """gemm.hip x_rows_finish<LN> in float32: mean = sum * fl(1/384); q = sum (x - mean)^2; rstd = rsqrt(q * fl(1/384) + eps);
    (x - mean) * rstd.  (The kernel's rsqrt is the hardware approximation, good to 1 ulp; the sums run in its lane order —
    differences of a few float32 ulps, 2^-16 of a bf16 ulp.)  -> float32, not yet rounded to bf16."""
    x = x.to(torch.float32)
    inv_k = torch.tensor(1.0 / K, dtype=torch.float32)
    mean = x.sum(dim=1, keepdim=True) * inv_k
    d = x - mean
    q = (d * d).sum(dim=1, keepdim=True)
    rstd = torch.rsqrt(q * inv_k + torch.tensor(eps, dtype=torch.float32))
    return d * rstd


def xhat_bf16(x: torch.Tensor, eps: float = EPS) -> torch.Tensor:
    """The normalised rows as the kernels use them: rounded to bf16 (float64 values)."""
    return bf16_rne(xhat_f64(x, eps))


# ---- weights ------------------------------------------------------------------------------------------------------------
def ln_params(ln: bool, g: torch.Generator):
    if not ln:
        return None, None
    return choice((0.5, 1.0, 2.0), (K,), g), choice((-0.5, 0.0, 0.5), (K,), g)


def dense_weight(n_out: int, g: torch.Generator) -> torch.Tensor:
    """[n_out][384], every entry in {+-1/4, +-1/2, +-1}; magnitudes follow a row pattern (row n leans on magnitude
    n % 3) so that rows differ in scale as well as in signs.  No two rows are equal (asserted)."""
    mags = torch.tensor((0.25, 0.5, 1.0), dtype=F64)
    lean = (torch.arange(n_out) % 3)[:, None]
    pick = torch.where(torch.rand(n_out, K, generator=g) < 0.5, lean.expand(n_out, K), torch.randint(0, 3, (n_out, K), generator=g))
    w = mags[pick] * (torch.randint(0, 2, (n_out, K), generator=g) * 2 - 1).to(F64)
    assert torch.unique(w @ torch.rand(K, dtype=F64, generator=g)).numel() == n_out, "two equal weight rows"
    return w


def sparse_weight(n_out: int, gamma, g: torch.Generator, nnz: int = 8) -> torch.Tensor:
    """[n_out][384] with `nnz` non-zeros per row, W in multiples of 1/4 and |W gamma| in {1/4, 1/2}: with x-hat in multiples
    of 2^-9 every product is a multiple of 2^-11, so an odd multiple of 2^-12 as the bias keeps the sum off zero."""
    gam = torch.ones(K, dtype=F64) if gamma is None else gamma
    cols = torch.rand(n_out, K, generator=g).argsort(dim=1)[:, :nnz]
    wg_mag = torch.where(torch.rand(n_out, nnz, generator=g) < 0.5, 0.25, 0.5).to(F64)
    wg_mag = torch.where(gam[cols] == 2.0, 0.5, wg_mag)                  # W = 1/8 would not be a multiple of 1/4
    val = wg_mag / gam[cols] * (torch.randint(0, 2, (n_out, nnz), generator=g) * 2 - 1).to(F64)
    w = torch.zeros(n_out, K, dtype=F64)
    w.scatter_(1, cols, val)
    assert bool((w * 4 == torch.round(w * 4)).all()) and bool(((w != 0).sum(dim=1) == nnz).all())
    assert set((w * gam).abs().unique().tolist()) <= {0.0, 0.25, 0.5}
    return w


def odd_bias(n: int, g: torch.Generator) -> torch.Tensor:
    """Odd multiples of 2^-12 with |b| <= 1."""
    return (2 * torch.randint(-2048, 2048, (n,), generator=g) + 1).to(F64) * 2.0 ** -12


def fold(w, b_folded, gamma, beta):
    """(W gamma, the bias b to pass so that the prepare step's b + W beta is `b_folded`)."""
    wg = w if gamma is None else w * gamma
    b = b_folded if beta is None else b_folded - w @ beta
    return wg, b


def sum_fits_float32(terms_abs_sum: torch.Tensor, unit: float) -> bool:
    """Every partial sum of terms that are multiples of `unit`, in any order, is a float32 number: sum |term| < 2^24 unit."""
    return bool((terms_abs_sum < 2.0 ** 24 * unit).all())


# ---- the GELU table (host restatement of gemm.hip gelu_table_kernel; the GPU tests read the device's) -----------------
def host_gelu_table() -> torch.Tensor:
    """[GT_N][2] int32 bf16 bit patterns: entry [k][sign] = bf16(gelu(x)), x = the bf16 with bits sign << 15 | GT_LO + k,
    gelu in float32 with erff."""
    k = torch.arange(GT_N, dtype=torch.int32)[:, None]
    sign = torch.arange(2, dtype=torch.int32)[None, :]
    x = (((sign << 15) | (GT_LO + k)) << 16).view(torch.float32)
    return bits_of(torch.nn.functional.gelu(x).to(torch.bfloat16))


def device_table_bits(table_u8: torch.Tensor) -> torch.Tensor:
    """hip_ops.gelu_table's byte tensor -> [GT_N][2] int32 bit patterns (same device)."""
    return (table_u8.view(torch.int16).to(torch.int32) & 0xFFFF).reshape(GT_N, 2)


def table_index(h_bits: torch.Tensor):
    """bf16 bit patterns -> (k, sign, in_range): gemm.hip gelu_table_slice, k = (bits & 0x7fff) - kGtLo."""
    k = (h_bits & 0x7FFF) - GT_LO
    return k, h_bits >> 15, (k >= 0) & (k < GT_N)


def table_gelu(h_b: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
    """g = table[bf16 h] as float64; h_b: bf16-exact float64 values, all inside the table's range (asserted)."""
    k, sign, ok = table_index(f64_to_bits(h_b))
    assert bool(ok.all()), "pre-activation outside the table's range"
    return bits_to_f64(table.to(h_b.device)[k.long(), sign.long()])


def gelu_f64(x: torch.Tensor) -> torch.Tensor:
    return 0.5 * x * (1.0 + torch.erf(x * (0.5 ** 0.5)))


def gelu_float_path(x: torch.Tensor) -> torch.Tensor:
    """gemm.hip:66-99 (gelu_erf / gelu_erf2), the kernels' float path, in float64 with the kernel's float32 constants:
    erf by Abramowitz-Stegun 7.1.26, gelu = max(x, 0) - 0.5 |x| poly(t) t exp(-x^2 / 2).  Its |error| <= 1.5e-7 in erf is
    many bf16 ulps of gelu(x) for x < -4, so a float-path block is compared with THIS, not with the erf of the table."""
    f = lambda c: float(np.float32(c))
    x = x.to(F64)
    ax = x.abs()
    t = 1.0 / (1.0 + ax * f(np.float32(0.3275911) * np.float32(0.70710678118654752)))
    p = t * f(1.061405429) + f(-1.453152027)
    p = p * t + f(1.421413741)
    p = p * t + f(-0.284496736)
    p = p * t + f(0.254829592)
    zl = x * f(0.84932180028801907)
    q = p * t * torch.exp2(-(zl * zl))
    return x.clamp_min(0.0) - 0.5 * ax * q


# ---- comparators --------------------------------------------------------------------------------------------------------
def _first(bad: torch.Tensor):
    return tuple(int(v) for v in torch.nonzero(bad)[0])


def compare_bits(got: torch.Tensor, case: dict):
    """Every element's bit pattern equals case['expect_bits'] (NaN never does)."""
    gb, want = bits_of(got).reshape(-1), case["expect_bits"].reshape(-1).to(got.device)
    assert gb.numel() == want.numel(), (gb.numel(), want.numel())
    bad = gb != want
    if bool(bad.any()):
        i = _first(bad)[0]
        raise AssertionError(f"{case.get('name', 'case')}: {int(bad.sum())} of {bad.numel()} elements differ; first at flat index {i}: "
                             f"got {float(bits_to_f64(gb[i])):.9g} (0x{int(gb[i]):04x}), expected {float(bits_to_f64(want[i])):.9g} (0x{int(want[i]):04x})")


def compare_bound(got: torch.Tensor, case: dict):
    """|got - case['ref']| <= case['bound'] element by element (float64; a NaN fails)."""
    val = bits_to_f64(bits_of(got)).reshape(case["ref"].shape)
    ref, bound = case["ref"].to(val.device), case["bound"].to(val.device)
    bad = ~((val - ref).abs() <= bound)
    if bool(bad.any()):
        i = _first(bad)
        raise AssertionError(f"{case.get('name', 'case')}: {int(bad.sum())} of {bad.numel()} elements out of bound; first at {i}: "
                             f"got {float(val[i]):.9g}, reference {float(ref[i]):.9g}, bound {float(bound[i]):.3g}")


def compare(got: torch.Tensor, case: dict):
    """The comparison a case asks for: bit equality where it carries expect_bits, its per-element bound otherwise."""
    (compare_bits if "expect_bits" in case else compare_bound)(got, case)


# ---- x-stationary GEMM --------------------------------------------------------------------------------------------------
def xs_case(rows: int, n_out: int, kind: str, ln: bool, epi: int, seed: int, device="cpu", table=None, gelu_float=False) -> dict:
    """vc_linear_xs_bf16 on exact operands.  kind 'dense' / 'sparse'; epi EPI_BIAS / EPI_RESIDUAL: out bits = bf16(h64 (+ r));
    EPI_GELU with `table` ([GT_N][2] bit patterns): out bits = table[bf16(h64)]; EPI_GELU with gelu_float: the float
    path's bound of test_xs_gelu_table_is_the_bf16_gelu_for_every_input, |err| <= 2^-8 |ref| + 2e-7 (1 + |h|)."""
    g = gen(seed)
    x, _, _ = ln_rows(rows, g)
    gamma, beta = ln_params(ln, g)
    if kind == "dense":
        w = dense_weight(n_out, g)
        b_folded = torch.randint(-8, 9, (n_out,), generator=g).to(F64) * 0.25
    else:
        w = sparse_weight(n_out, gamma, g)
        b_folded = odd_bias(n_out, g)
    wg, b = fold(w, b_folded, gamma, beta)
    res = torch.randint(-32, 33, (rows, n_out), generator=g).to(F64) * 0.125 if epi == EPI_RESIDUAL else None
    x, wg, b_folded = x.to(device).to(F64), wg.to(device), b_folded.to(device)
    xin = xhat_bf16(x) if ln else x
    h = xin @ wg.t() + b_folded                                          # exact: every partial sum is a float64 number
    case = dict(name=f"xs {kind} rows={rows} n={n_out} ln={ln} epi={epi}", x=to_bf16(x), w=w.float(), b=b.float(),
                gamma=None if gamma is None else gamma.float(), beta=None if beta is None else beta.float(), epi=epi,
                residual=None if res is None else to_bf16(res.to(device)), xin=xin, wg=wg, b_folded=b_folded, h=h)
    assert is_bf16_exact(wg) and bool((b.float().to(F64) == b).all())
    if epi == EPI_GELU:
        assert kind == "sparse" and ln
        assert bool((h.abs() >= 2.0 ** -12).all()) and bool((h.abs() < 8.0).all())
        if gelu_float:
            case["ref"] = gelu_f64(h)
            case["bound"] = 2.0 ** -8 * case["ref"].abs() + 2e-7 * (1 + h.abs())
        else:
            case["expect_bits"] = f64_to_bits(table_gelu(bf16_rne(h), table))
    else:
        case["expect_bits"] = f64_to_bits(bf16_rne(h if res is None else h + res.to(device)))
    return case


def emulate_xs(case: dict, table=None, order_seed: int = 0, mutate=None) -> torch.Tensor:
    """The kernel's contract in float32 on the CPU: x-hat by the kernel's sequence rounded to bf16, bias as the initial
    value, the 384 products added one by one in a random order (order_seed), epilogue, one rounding to bf16.
    mutate = (kind, row, col, k): 'drop' / 'double' the product x-hat[row, k] W'[col, k] of output (row, col).  -> bf16."""
    f32 = torch.float32
    x = case["x"].cpu()
    xin = xhat_f32_kernel_sequence(x).to(torch.bfloat16).to(f32) if case["gamma"] is not None else x.to(f32)
    wg = case["wg"].cpu().to(torch.bfloat16).to(f32)
    acc = case["b_folded"].cpu().to(f32)[None, :].repeat(x.shape[0], 1)
    for k in torch.randperm(K, generator=gen(1000 + order_seed)).tolist():
        acc += xin[:, k, None] * wg[None, :, k]
    if mutate is not None:
        kind, r, c, k = mutate
        acc[r, c] += {"drop": -1.0, "double": 1.0}[kind] * xin[r, k] * wg[c, k]
    if case["epi"] == EPI_RESIDUAL:
        acc = acc + case["residual"].cpu().to(f32)
    if case["epi"] == EPI_GELU:
        k, sign, ok = table_index(bits_of(acc.to(torch.bfloat16)))
        assert bool(ok.all())
        return table[k.long(), sign.long()].to(torch.int16).view(torch.bfloat16)
    return acc.to(torch.bfloat16)


# ---- fused MLP ----------------------------------------------------------------------------------------------------------
W2_NNZ = 32


def mlp_weights(n_hidden: int, g: torch.Generator, float_blocks: bool):
    """W1 / b1 sparse as for the x-stationary kernel, W2 [384][n_hidden] with 32 non-zeros per output row in
    {+-1/4, +-1/2, +-1} (four of them placed so that every hidden unit feeds an output), b2 in multiples of 1/8.
    float_blocks: in every third 32-chunk of the hidden layer one unit leaves the GELU table's range — chunks 0, 6, ..:
    folded bias +-16 (alternating); chunks 3, 9, ..: a zero W1 row with folded bias 0, the value that makes h == 0 on
    every row — so that (32 rows x that chunk) blocks take the kernel's float path.  -> dict of float64 tensors."""
    gamma, beta = ln_params(True, g)
    w1 = sparse_weight(n_hidden, gamma, g)
    b1_folded = odd_bias(n_hidden, g)
    special = []
    if float_blocks:
        for c in range(0, n_hidden // 32, 3):
            u = 32 * c + int(torch.randint(0, 32, (1,), generator=g))
            if (c // 3) % 2 == 0:
                b1_folded[u] = 16.0 if (c // 6) % 2 == 0 else -16.0
            else:
                w1[u] = 0.0
                b1_folded[u] = 0.0
            special.append(u)
    w1g, b1 = fold(w1, b1_folded, gamma, beta)
    forced = (4 * torch.arange(K)[:, None] + torch.arange(4)[None, :]) % n_hidden
    order = torch.rand(K, n_hidden, generator=g)
    order.scatter_(1, forced, -1.0)                                      # the forced columns sort first
    cols = order.argsort(dim=1)[:, :W2_NNZ]
    val = choice((0.25, 0.5, 1.0), (K, W2_NNZ), g) * (torch.randint(0, 2, (K, W2_NNZ), generator=g) * 2 - 1).to(F64)
    w2 = torch.zeros(K, n_hidden, dtype=F64)
    w2.scatter_(1, cols, val)
    b2 = torch.randint(-16, 17, (K,), generator=g).to(F64) * 0.125
    return dict(gamma=gamma, beta=beta, w1=w1, b1=b1, w1g=w1g, b1_folded=b1_folded, w2=w2, b2=b2, special=special)


def mlp_reference(x, p: dict, table):
    """The kernel's contract step by step (float64, on x's device): x-hat rounded to bf16; exact h; per (32 rows x 32 hidden)
    block g = table[bf16(h)], or — a block that holds a value outside the table's range, gemm.hip gelu_table_slice
    slice 15 — g = bf16(gelu_float_path(bf16(h))); float64 sum W2 g + b2 + x.
    -> (ref, bound, float-path mask [row blocks][chunks], g)."""
    dev = x.device
    rows, n_hidden = x.shape[0], p["w1"].shape[0]
    h = xhat_bf16(x) @ p["w1g"].to(dev).t() + p["b1_folded"].to(dev)      # exact
    hb = bf16_rne(h)
    k, sign, ok = table_index(f64_to_bits(hb))
    tab = table.to(dev)
    g = bits_to_f64(tab[k.clamp(0, GT_N - 1).long(), sign.long()])
    n_rb = (rows + 31) // 32
    pad = n_rb * 32 - rows
    bad = torch.nn.functional.pad(~ok, (0, 0, 0, pad)).reshape(n_rb, 32, n_hidden // 32, 32)
    fblock = bad.any(dim=3).any(dim=1)                                    # [row blocks][chunks]
    fmask = fblock[:, None, :, None].expand(n_rb, 32, n_hidden // 32, 32).reshape(n_rb * 32, n_hidden)[:rows]
    g = torch.where(fmask, bf16_rne(gelu_float_path(hb)), g)
    w2 = p["w2"].to(dev)
    ref = g @ w2.t() + p["b2"].to(dev) + x
    mag = g.abs() @ w2.abs().t() + p["b2"].to(dev).abs() + x.abs()
    # one bf16 ulp of the result + the float32 summation bound over nnz + 2 terms; a float-path unit may come out one bf16
    # ulp of g beside the float64 evaluation of the same formula
    bound = 2.0 ** -8 * ref.abs() + 2 * (W2_NNZ + 2) * 2.0 ** -24 * mag + (ulp_bf16(g) * fmask) @ w2.abs().t()
    return ref, bound, fblock, g


def mlp_case(rows: int, n_hidden: int, seed: int, device="cpu", table=None, float_blocks=False) -> dict:
    g = gen(seed)
    x, _, _ = ln_rows(rows, g)
    p = mlp_weights(n_hidden, g, float_blocks)
    x = x.to(device).to(F64)
    ref, bound, fblock, act = mlp_reference(x, p, table)
    return dict(name=f"mlp rows={rows} hidden={n_hidden} float_blocks={float_blocks}", x=to_bf16(x), p=p, ref=ref, bound=bound,
                fblock=fblock, g=act, table=table)


def emulate_mlp(case: dict, order_seed: int = 0, mutate=None) -> torch.Tensor:
    """The fused MLP's contract in float32 on the CPU, fc2's products added one by one in a random order, then + b2, + x,
    one rounding.  mutate: ('swap_w2', k1, k2) W2's k indices k1 and k2 exchanged; ('table', k, sign) that table entry one
    bf16 ulp up; ('float_from_table',) the float-path blocks answered from the (clamped) table; ('act', row, unit, delta)
    one hidden activation off by delta.  -> bf16."""
    f32 = torch.float32
    p, x, table = case["p"], case["x"].cpu(), case["table"].cpu().clone()
    rows, n_hidden = x.shape[0], p["w1"].shape[0]
    mutate = mutate or ("none",)
    if mutate[0] == "table":
        table[mutate[1], mutate[2]] += 1
    xin = xhat_f32_kernel_sequence(x).to(torch.bfloat16).to(f32)
    w1g = p["w1g"].to(torch.bfloat16).to(f32)
    h = p["b1_folded"].to(f32)[None, :].repeat(rows, 1)
    for k in torch.randperm(K, generator=gen(2000 + order_seed)).tolist():
        h += xin[:, k, None] * w1g[None, :, k]
    hb = h.to(torch.bfloat16)
    k, sign, ok = table_index(bits_of(hb))
    g = table[k.clamp(0, GT_N - 1).long(), sign.long()].to(torch.int16).view(torch.bfloat16).to(f32)
    if mutate[0] != "float_from_table":
        fmask = case["fblock"].cpu()[:, None, :, None].expand(-1, 32, -1, 32).reshape(-1, n_hidden)[:rows]
        gf = gelu_float_path(hb.to(F64)).to(f32).to(torch.bfloat16).to(f32)
        g = torch.where(fmask, gf, g)
    if mutate[0] == "act":
        g[mutate[1], mutate[2]] += mutate[3]
    w2 = p["w2"].to(torch.bfloat16).to(f32).clone()
    if mutate[0] == "swap_w2":
        w2[:, [mutate[1], mutate[2]]] = w2[:, [mutate[2], mutate[1]]]
    acc = torch.zeros(rows, K, dtype=f32)
    for u in torch.randperm(n_hidden, generator=gen(3000 + order_seed)).tolist():
        acc += g[:, u, None] * w2[None, :, u]
    return ((acc + p["b2"].to(f32)) + x.to(f32)).to(torch.bfloat16)


# ---- attention ----------------------------------------------------------------------------------------------------------
HD = 64


def attention_groups(n: int, odd_group: bool = False, fast_pass: bool = False):
    """Key sets, each of 32 or 64 keys (1 / l exact): the first 64 keys; the last 64 (into the ragged last key block); 64
    keys straddling the block boundary at key 64; 32 keys spread evenly with key n - 1 among them; for n >= 128, 32 keys
    spread evenly behind key block 0.
    Which pass of attention_kernel<QT, LAZY = true> (q_prescaled) a case's result comes from (attention.hip:338-361): a row
    whose group has no key in block 0 starts from m0 = -1024, its group's keys then weigh exp2(+1024) = inf, the row fails
    the range test, and ONE such row sends its whole unit to the EXACT pass.  For n >= 128 the last 64 keys and the set
    behind block 0 are such groups, and every unit holds their rows: every unit is recomputed by the exact pass.
    fast_pass: every group reaches into key block 0 — the 'last' group is key 7 and the last 63 keys, the set behind block 0
    is left out — so every row passes the range test and what is stored is the FAST pass's result.
    odd_group: the first set becomes keys 20 .. 67, 48 keys (1 / 48 is not dyadic)."""
    assert n >= 96
    last = [7] + list(range(n - 63, n)) if fast_pass else list(range(n - 64, n))
    groups = [list(range(20, 68)) if odd_group else list(range(64)), last, list(range(32, 96)),
              sorted(n - 1 - i * ((n - 1) // 31) for i in range(32))]
    if n >= 128 and not fast_pass:
        groups.append([64 + (i * (n - 64)) // 32 for i in range(32)])
    for s in groups:
        assert len(set(s)) == len(s) and 0 <= min(s) and max(s) < n
    assert not (fast_pass and leaves_fast_pass(groups))
    return groups


def leaves_fast_pass(groups) -> bool:
    """Under q_prescaled: does some group have no key in key block 0 (then every unit that holds one of its rows — here every
    unit — is recomputed by the exact pass)?"""
    return any(min(s) >= 64 for s in groups)


def attention_case(B: int, N: int, H: int, seed: int = 0, device="cpu", odd_group: bool = False, fast_pass: bool = False) -> dict:
    """qkv [B][N][3 H 64] bf16 with one-hot queries, membership keys and position-coded values (module docstring of the
    spec test); the same tensors serve q_prescaled 1 and 0.  Group s of (b, h) lives on head dimension dim[b, h, s]; query
    i asks for group (i + b + h) % n_groups.  expect: the closed form  sum_{j in S} v[j] / |S|."""
    g = gen(seed)
    groups = attention_groups(N, odd_group, fast_pass)
    ng = len(groups)
    member = torch.zeros(ng, N, dtype=torch.bool)
    for s, keys in enumerate(groups):
        member[s, keys] = True
    j = torch.arange(N)
    v = torch.zeros(N, HD, dtype=F64)
    v[j, j % 64] = torch.pow(2.0, ((j // 64) % 4).to(F64))
    qkv = torch.zeros(B, N, 3, H, HD, dtype=F64)
    expect = torch.zeros(B, N, H, HD, dtype=F64)
    ask = torch.zeros(B, H, N, dtype=torch.int64)
    dims = torch.zeros(B, H, ng, dtype=torch.int64)
    for b in range(B):
        for h in range(H):
            dim = torch.randperm(HD, generator=g)[:ng]
            u = (j + b + h) % ng
            qkv[b, :, 0, h] = 8.0 * torch.nn.functional.one_hot(dim[u], HD).to(F64)
            kk = torch.full((N, HD), -128.0, dtype=F64)
            kk[:, dim] = torch.where(member.t(), 0.0, -128.0).to(F64)
            qkv[b, :, 1, h] = kk
            qkv[b, :, 2, h] = v
            closed = (member.to(F64) @ v) / member.sum(dim=1, keepdim=True).to(F64)      # [groups][64]
            expect[b, :, h] = closed[u]
            ask[b, h], dims[b, h] = u, dim
    size = member.sum(dim=1)[ask].permute(0, 2, 1)                       # [B][N][H] keys behind every output row
    dyadic = (size & (size - 1)) == 0
    exact = expect.reshape(B, N, H * HD)
    case = dict(name=f"attention B={B} N={N} H={H} odd_group={odd_group} fast_pass={fast_pass}", qkv=to_bf16(qkv.reshape(B, N, 3 * H * HD)).to(device),
                n_heads=H, member=member, ask=ask, dims=dims, v=v, exact=exact, groups=groups)
    if odd_group:
        # float32 division errs by 2^-23 relative, far below half a bf16 ulp: a row of the 48-key group comes out within one
        # bf16 ulp of the exact value; every other row is dyadic and exact
        tol = torch.where(dyadic[..., None].expand(B, N, H, HD).reshape(B, N, H * HD), 0.0, 1.0) * ulp_bf16(exact)
        case["ref"], case["bound"] = exact, tol
    else:
        assert bool(dyadic.all())
        case["expect_bits"] = f64_to_bits(exact)
    return case


def attention_softmax_f64(case: dict, q_prescaled: bool) -> torch.Tensor:
    """A float64 softmax of the case's tensors (base 2 under q_prescaled, as the kernel defines it) -> [B][N][H 64]."""
    qkv = case["qkv"].cpu().to(F64)
    B, N, _ = qkv.shape
    H = case["n_heads"]
    q, k, v = qkv.reshape(B, N, 3, H, HD).permute(2, 0, 3, 1, 4)
    s = q @ k.transpose(-1, -2) * (math.log(2.0) if q_prescaled else 0.125)
    return (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B, N, H * HD)


def emulate_attention(case: dict, q_prescaled: bool, mutate=None) -> torch.Tensor:
    """The kernel's contract in float32: scores by a float32 product, weights exp2(s) / exp2(s / 8 log2 e) against the
    row maximum (exactly 1 or 0 here), bf16 weights, float32 row sum and output sum, out = o * (1 / l), one rounding.
    mutate = (kind, b, h, row, key): 'drop' that key's weight, 'double' it, or 'extra' — a key outside the row's group let
    in with zero V (only the row sum sees it).  -> bf16 [B][N][H 64]."""
    f32 = torch.float32
    qkv = case["qkv"].cpu().to(f32)
    B, N, _ = qkv.shape
    H = case["n_heads"]
    q, k, v = qkv.reshape(B, N, 3, H, HD).permute(2, 0, 3, 1, 4)
    s = q @ k.transpose(-1, -2)
    s = s - s.max(dim=-1, keepdim=True).values
    p = torch.exp2(s * (1.0 if q_prescaled else 0.125 * 1.4426950408889634))
    l_extra = torch.zeros(B, H, N, 1, dtype=f32)
    if mutate is not None:
        kind, b, h, row, key = mutate
        if kind == "drop":
            assert p[b, h, row, key] == 1
            p[b, h, row, key] = 0.0
        elif kind == "double":
            assert p[b, h, row, key] == 1
            p[b, h, row, key] = 2.0
        else:
            assert p[b, h, row, key] == 0
            l_extra[b, h, row] = 1.0
    l = p.sum(dim=-1, keepdim=True) + l_extra
    o = p.to(torch.bfloat16).to(f32) @ v
    return (o * (1.0 / l)).transpose(1, 2).reshape(B, N, H * HD).to(torch.bfloat16)


# ---- the staged GEMMs (gemm.hip gemm_kernel, gemm256_kernel): linear, patch embedding, convolution -----------------------
# Operands of two kinds.  'dense': x in multiples of 1/4 in [-2, 2], W in {+-1/4, +-1/2, +-1}, bias in multiples of 1/4,
# residual / pos_embed in multiples of 1/8 with |r| <= 4: products are multiples of 2^-4 and sum |product| <= 2 K, at K = 4096
# 2^17 units — every partial sum in any order is a float32 number.  'sparse': x from {+-1/4, +-1/2, +-1} (no zero), W with 6
# non-zeros per row from the same set at columns drawn over the whole of K, bias an odd multiple of 2^-5 with |b| <= 1: the
# pre-activation h is an odd multiple of 2^-5 with 2^-5 <= |h| < 8, every such value is a bf16 number (8 significant bits),
# so every single dropped, doubled or misplaced non-zero product (an even multiple of 2^-5, not 0) changes the output bits.
EPI_SWIGLU = 4                # VC_EPI_SWIGLU
BK = 64                       # K tile of both staged kernels
SPARSE_NNZ = 6
PM = (-1.0, -0.5, -0.25, 0.25, 0.5, 1.0)


def _ints(lo: int, hi: int, shape, g: torch.Generator) -> torch.Tensor:
    """Integers lo .. hi (inclusive) drawn on the CPU as int8: the long cases widen them on the device."""
    return torch.randint(lo, hi + 1, tuple(shape), generator=g, dtype=torch.int8)


def dyadic(lo: int, hi: int, step: float, shape, g: torch.Generator, device="cpu") -> torch.Tensor:
    """Multiples of `step` from lo step to hi step, float64 on `device`."""
    return _ints(lo, hi, shape, g).to(device).to(F64) * step


def pm_values(shape, g: torch.Generator, device="cpu") -> torch.Tensor:
    """Values from {+-1/4, +-1/2, +-1}, float64 on `device`."""
    return torch.tensor(PM, dtype=F64, device=device)[_ints(0, len(PM) - 1, shape, g).to(device).long()]


def odd_bias32(n: int, g: torch.Generator) -> torch.Tensor:
    """Odd multiples of 2^-5 with |b| <= 1."""
    return (2 * _ints(-16, 15, (n,), g).to(F64) + 1) * 2.0 ** -5


def staged_sparse_weight(n_out: int, k: int, g: torch.Generator, nnz: int = SPARSE_NNZ) -> torch.Tensor:
    """[n_out][k] with `nnz` non-zeros per row from {+-1/4, +-1/2, +-1} at columns drawn over the whole of k.  Asserted: every
    K tile of 64 holds a non-zero of some row of every 256-column tile (a K tile the kernel drops or takes twice is seen in
    every output tile)."""
    cols = torch.rand(n_out, k, generator=g).argsort(dim=1)[:, :nnz]
    w = torch.zeros(n_out, k, dtype=F64)
    w.scatter_(1, cols, pm_values((n_out, nnz), g))
    assert bool(((w != 0).sum(dim=1) == nnz).all())
    for n0 in range(0, n_out, 256):
        assert bool((w[n0:n0 + 256] != 0).any(dim=0).reshape(k // BK, BK).any(dim=1).all()), "a K tile without a non-zero"
    return w


def assert_sparse_range(h: torch.Tensor):
    """h is an odd multiple of 2^-5 with 2^-5 <= |h| < 8 (then a bf16 number)."""
    m = h * 32
    assert bool((m == torch.round(m)).all()) and bool((m.abs() % 2 == 1).all()) and bool((h.abs() < 8.0).all())
    assert is_bf16_exact(h)


def silu_mul_f64(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    return a / (1.0 + torch.exp(-a)) * b


def bound_ratio(got: torch.Tensor, case: dict) -> float:
    """max |got - ref| / bound of a case judged by a bound (what the tests print beside their assertion)."""
    val = bits_to_f64(bits_of(got)).reshape(case["ref"].shape)
    ref, bound = case["ref"].to(val.device), case["bound"].to(val.device)
    return float(((val - ref).abs() / bound).max())


def _epilogue_expectation(case: dict, h: torch.Tensor, res):
    """EPI_BIAS / EPI_RESIDUAL: bits of bf16(h (+ r)).  EPI_GELU: gelu_f64(h) under the float path's bound, 2^-8 |ref| + 2e-7
    (1 + |h|), the one xs_case(gelu_float=True) uses.  EPI_SWIGLU: see linear_case."""
    epi = case["epi"]
    if epi == EPI_GELU:
        case["ref"] = gelu_f64(h)
        case["bound"] = 2.0 ** -8 * case["ref"].abs() + 2e-7 * (1 + h.abs())
    elif epi == EPI_SWIGLU:
        hh = h.shape[-1] // 2
        a, b = h[..., :hh], h[..., hh:]
        case["ref"] = silu_mul_f64(a, b)
        case["bound"] = ulp_bf16(case["ref"]) + 2.0 ** -20 * (1 + a.abs()) * case["ref"].abs()
    else:
        case["expect_bits"] = f64_to_bits(bf16_rne(h if res is None else h + res))
    return case


def _operands(kind: str, x_shape, n_out: int, k: int, g: torch.Generator, device):
    """(x, W, bias, unit of the products and the bias) of one kind."""
    if kind == "dense":
        return dyadic(-8, 8, 0.25, x_shape, g, device), pm_values((n_out, k), g), dyadic(-8, 8, 0.25, (n_out,), g), 2.0 ** -4
    assert kind == "sparse"
    return pm_values(x_shape, g, device), staged_sparse_weight(n_out, k, g), odd_bias32(n_out, g), 2.0 ** -5


def linear_case(rows: int, k: int, n_out: int, kind: str, epi: int, seed: int, device="cpu") -> dict:
    """vc_linear_bf16 on exact operands (kinds above).  EPI_BIAS / EPI_RESIDUAL: out bits = bf16(h64 (+ r)).  EPI_GELU (sparse):
    gelu_f64(h) under 2^-8 |ref| + 2e-7 (1 + |h|).  EPI_SWIGLU (sparse; n_out is the width of the product, gate rows then
    value rows, so gate a and value b are exact): ref = a / (1 + exp(-a)) b in float64, bound = ulp_bf16(ref) + 2^-20 (1 + |a|)
    |ref|.  The second term: the exponent a * -log2(e) carries 2^-24 relative, |a| 2^-24 relative in exp2; v_exp_f32 and
    v_rcp_f32 are 1 ulp each, two multiplications: under (|a| + 4) 2^-23, and the term gives it eight times that.
    Measured (test_staged_exact_spec.py::test_swiglu_emulation_stays_inside_its_bound): the float32 emulation (torch exp2 and
    reciprocal) reaches err / bound = 0.50, all of it the rounding to bf16 (half an ulp of a full-ulp term); the float32
    term is not widened."""
    g = gen(seed)
    x, w, b, unit = _operands(kind, (rows, k), n_out, k, g, device)
    res = dyadic(-32, 32, 0.125, (rows, n_out), g, device) if epi == EPI_RESIDUAL else None
    w, b = w.to(device), b.to(device)
    h = x @ w.t() + b                                                    # exact: every partial sum is a float64 number
    # sum |product| + |bias| + |residual| <= max |x| sum |W| + ..: every partial sum, in any order, is a float32 number
    assert sum_fits_float32(x.abs().amax(dim=1, keepdim=True) * w.abs().sum(dim=1)[None, :] + b.abs() + 4.0, unit)
    if kind == "sparse":
        assert_sparse_range(h)
    assert epi in (EPI_BIAS, EPI_RESIDUAL) or kind == "sparse"
    case = dict(name=f"linear {kind} {rows}x{k}x{n_out} epi={epi}", kind=kind, epi=epi, x=to_bf16(x), w=to_bf16(w), b=to_bf16(b),
                residual=None if res is None else to_bf16(res), h=h)
    return _epilogue_expectation(case, h, res)


def _f32_products(x: torch.Tensor, w: torch.Tensor, order_seed: int, mutate=None) -> torch.Tensor:
    """sum_k x[:, k] w[:, k] in float32, the products added one by one in a random order.  mutate: ('drop' | 'double', row, col,
    k) that product of that output; ('ktile', t) K tile t taken twice, in place of its neighbour t + 1."""
    k = x.shape[1]
    src = torch.arange(k)
    if mutate is not None and mutate[0] == "ktile":
        t = mutate[1]
        src[(t + 1) * BK:(t + 2) * BK] = torch.arange(t * BK, (t + 1) * BK)
    acc = torch.zeros(x.shape[0], w.shape[0], dtype=torch.float32)
    for kk in src[torch.randperm(k, generator=gen(4000 + order_seed))].tolist():
        acc += x[:, kk, None] * w[None, :, kk]
    if mutate is not None and mutate[0] in ("drop", "double"):
        kind, r, c, kk = mutate
        acc[r, c] += {"drop": -1.0, "double": 1.0}[kind] * x[r, kk] * w[c, kk]
    return acc


def _f32_epilogue(acc: torch.Tensor, case: dict, mutate=None) -> torch.Tensor:
    """The staged kernels' epilogues on float32 pre-activations -> bf16.  mutate ('swiglu_swap', col): gate and value of that
    output column exchanged; ('rows', r1, r2): two output rows exchanged."""
    f32 = torch.float32
    epi = case["epi"]
    if epi == EPI_RESIDUAL:
        acc = acc + case["residual"].cpu().to(f32)
    elif epi == EPI_GELU:
        acc = gelu_float_path(acc.to(F64)).to(f32)
    elif epi == EPI_SWIGLU:
        hh = acc.shape[1] // 2
        a, b = acc[:, :hh].clone(), acc[:, hh:].clone()
        if mutate is not None and mutate[0] == "swiglu_swap":
            a[:, mutate[1]], b[:, mutate[1]] = acc[:, hh + mutate[1]], acc[:, mutate[1]]
        e = torch.exp2(a * torch.tensor(-1.4426950408889634, dtype=f32))
        acc = a * torch.reciprocal(1.0 + e) * b
    out = acc.to(torch.bfloat16)
    if mutate is not None and mutate[0] == "rows":
        out[[mutate[1], mutate[2]]] = out[[mutate[2], mutate[1]]]
    return out


def emulate_linear(case: dict, order_seed: int = 0, mutate=None) -> torch.Tensor:
    """gemm_kernel / gemm256_kernel's contract in float32 on the CPU: bf16 operands, the K products added one by one in a
    random order, + bias, epilogue (GELU by the float path's formula, SwiGLU by exp2 and a reciprocal), one rounding."""
    f32 = torch.float32
    acc = _f32_products(case["x"].cpu().to(f32), case["w"].cpu().to(f32), order_seed, mutate) + case["b"].cpu().to(f32)
    return _f32_epilogue(acc, case, mutate)


def patch_case(B: int, T: int, n_out: int, k_in: int, seed: int, device="cpu") -> dict:
    """vc_patch_embed_bf16 on dense operands, pos_embed [1 + T][n_out] in multiples of 1/8: out[b, 1 + t] bits =
    bf16(patches[b, t] W^T + bias + pos_embed[1 + t]); expect_bits is [B][T][n_out], the rows the kernel writes."""
    g = gen(seed)
    x, w, b, unit = _operands("dense", (B, T, k_in), n_out, k_in, g, device)
    pos = dyadic(-32, 32, 0.125, (T + 1, n_out), g, device)
    w, b = w.to(device), b.to(device)
    assert sum_fits_float32(torch.tensor(2.0 * k_in + 2.0 + 4.0), unit)
    h = x @ w.t() + b + pos[1:]
    return dict(name=f"patch_embed B={B} T={T} n={n_out} k={k_in}", x=to_bf16(x), w=to_bf16(w), b=to_bf16(b), pos=to_bf16(pos),
                expect_bits=f64_to_bits(bf16_rne(h)))


def emulate_patch(case: dict, order_seed: int = 0, mutate=None) -> torch.Tensor:
    """EPI_PATCH in float32: products in a random order, + bias, + pos_embed[1 + t], one rounding -> [B][T][n_out] bf16.
    mutate ('pos',): pos_embed[t] in place of pos_embed[1 + t]; the product mutations of _f32_products on row b T + t."""
    f32 = torch.float32
    B, T, k = case["x"].shape
    acc = _f32_products(case["x"].cpu().to(f32).reshape(B * T, k), case["w"].cpu().to(f32), order_seed, mutate) + case["b"].cpu().to(f32)
    pos = case["pos"].cpu().to(f32)
    pos = pos[:-1] if mutate is not None and mutate[0] == "pos" else pos[1:]
    return (acc.reshape(B, T, -1) + pos).to(torch.bfloat16)


def conv_gather(img: torch.Tensor, kh: int, kw: int, dy0: int, dx0: int, nudge=None) -> torch.Tensor:
    """vc_conv_taps_bf16's definition as a gather: [B][H][W][C] -> [B H W][kh kw C], k = (tap, channel); tap t of output pixel
    (y, x) is pixel (y + dy0 + t / kw, x + dx0 + t % kw) of the same image, zero outside it.  nudge = t: that tap reads the
    pixel to the right of its own (the single-defect mutant)."""
    B, H, W, C = img.shape
    out = torch.zeros(B, H, W, kh * kw, C, dtype=img.dtype, device=img.device)
    for t in range(kh * kw):
        dy, dx = dy0 + t // kw, dx0 + t % kw + (1 if nudge == t else 0)
        ys, ye, xs, xe = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
        if ys < ye and xs < xe:
            out[:, ys:ye, xs:xe, t] = img[:, ys + dy:ye + dy, xs + dx:xe + dx]
    return out.reshape(B * H * W, kh * kw * C)


def conv_case(B: int, H: int, W: int, C: int, n_out: int, kh: int, kw: int, dy0: int, dx0: int, kind: str, epi: int, seed: int,
              device="cpu", img=None, weight=None, bias=None) -> dict:
    """vc_conv_taps_bf16 on exact operands: x_rows [B H W + 1][C] (the spare row holds junk: the call must zero it), weight
    [n_out][kh kw C].  EPI_BIAS: bits of bf16(h64); EPI_GELU (sparse): the float path's bound.  A tap outside the image
    leaves its products out, which keeps a sparse h an odd multiple of 2^-5.  img / weight / bias (float64): given operands
    in place of drawn ones (the parity classes of a transposed convolution)."""
    g = gen(seed)
    k = kh * kw * C
    x, w, b, unit = _operands(kind, (B * H * W + 1, C), n_out, k, g, device)
    if img is not None:
        x = torch.cat([img.reshape(B * H * W, C).to(device), x[-1:]])
    w, b = (w if weight is None else weight).to(device), (b if bias is None else bias).to(device)
    assert sum_fits_float32(torch.tensor(2.0 * k + 2.0), unit)
    h = conv_gather(x[:-1].reshape(B, H, W, C), kh, kw, dy0, dx0) @ w.t() + b
    if kind == "sparse":
        assert_sparse_range(h)
    case = dict(name=f"conv {kind} ({B},{H},{W},{C})->{n_out} taps {kh}x{kw} at ({dy0},{dx0}) epi={epi}", kind=kind, epi=epi,
                geometry=(B, H, W, kh, kw, dy0, dx0), x_rows=to_bf16(x), w=to_bf16(w), b=to_bf16(b), residual=None, h=h)
    return _epilogue_expectation(case, h, None)


def emulate_conv(case: dict, order_seed: int = 0, mutate=None) -> torch.Tensor:
    """The implicit GEMM in float32: the (tap, channel) products in a random order, + bias, epilogue, one rounding.
    mutate ('tap', t): tap t read from the neighbouring pixel; the product mutations of _f32_products."""
    f32 = torch.float32
    B, H, W, kh, kw, dy0, dx0 = case["geometry"]
    x = case["x_rows"].cpu().to(f32)[:-1]
    cols = conv_gather(x.reshape(B, H, W, -1), kh, kw, dy0, dx0, nudge=mutate[1] if mutate is not None and mutate[0] == "tap" else None)
    acc = _f32_products(cols, case["w"].cpu().to(f32), order_seed, mutate) + case["b"].cpu().to(f32)
    return _f32_epilogue(acc, case, mutate)


# ---- add + LayerNorm (vit_ops.hip add_layernorm_kernel) ------------------------------------------------------------------
# The float32 term of the bound: LN_T 2^-24 (|gamma| (1 + max |v| / sigma) + |beta|), sigma = sqrt(var + eps).  The mean's error
# is a few 2^-24 max |v| and reaches y as |gamma| / sigma times that (the row 96 + 0.5 k: max |v| / sigma ~ 100); the variance's
# and the last three operations' are a few 2^-24 of |x-hat gamma| and |y|.  Half an ulp is what the rounding to bf16 alone
# costs next to a tie, so the constant is measured on the values BEFORE that rounding (test_staged_exact_spec.py::
# test_layernorm_emulation_stays_inside_its_bound): the float32 emulation of the kernel's sequence reaches |y32 - ref| =
# 0.43 of the term with LN_T = 8 (0.86 with 4) over the shapes and both eps of the GPU test, at C = 2048.
LN_T = 8.0
LN_WIDTHS = (8, 72, 384, 520, 1536, 2048)
LN_ROWS = (1, 5, 777)
LN_EPS = (1e-6, 1e-5)


def ln_case(rows: int, C: int, eps: float, seed: int) -> dict:
    """x + residual -> (sum rounded to bf16, LayerNorm of the rounded sum).  `rows` rows of ln_rows (one level set, one scale)
    plus a residual in multiples of 1/8, gamma in {1/2, 1, 2}, beta in {-1/2, 0, 1/2}, and three more rows: a constant row
    (x = 3 - r: y must equal beta exactly), a row 96 + 0.5 k with |k| <= 3 (a large offset), a row of +-2^-7 (variance 2^-14:
    eps decides the result).  sum_bits by bits; y against float64 LayerNorm of the rounded sum within 0.5 ulp_bf16(ref) + the
    float32 term above.  (CPU tensors; the comparators move them.)"""
    g = gen(seed)
    x = ln_rows(rows, g, width=C)[0].to(F64)
    r = dyadic(-32, 32, 0.125, (rows, C), g)
    rc = dyadic(-32, 32, 0.125, (1, C), g)
    zero = torch.zeros(1, C, dtype=F64)
    x = torch.cat([x, 3.0 - rc, 96.0 + 0.5 * dyadic(-3, 3, 1.0, (1, C), g), (2.0 * _ints(0, 1, (1, C), g).to(F64) - 1.0) * 2.0 ** -7])
    r = torch.cat([r, rc, zero, zero])
    gamma, beta = choice((0.5, 1.0, 2.0), (C,), g), choice((-0.5, 0.0, 0.5), (C,), g)
    v = bf16_rne(x + r)                                                  # (the float32 sum of two bf16 numbers is exact)
    d = v - v.mean(dim=1, keepdim=True)
    sigma = torch.sqrt((d * d).mean(dim=1, keepdim=True) + float(np.float32(eps)))
    ref = d / sigma * gamma + beta
    t = LN_T * 2.0 ** -24 * (gamma.abs() * (1 + v.abs().amax(dim=1, keepdim=True) / sigma) + beta.abs())
    assert bool((v[rows] == 3.0).all()) and bool((ref[rows] == beta).all())
    return dict(name=f"add_layernorm rows={rows}+3 C={C} eps={eps}", x=to_bf16(x), residual=to_bf16(r), gamma=to_bf16(gamma),
                beta=to_bf16(beta), eps=eps, sum_bits=f64_to_bits(v), ref=ref, bound=0.5 * ulp_bf16(ref) + t, t=t,
                const_row=rows, offset_row=rows + 1, tiny_row=rows + 2)


def emulate_layernorm(case: dict, mutate=None, rounded: bool = True) -> torch.Tensor:
    """add_layernorm_kernel's sequence in float32 on the CPU: the sum rounded to bf16; lane l sums its chunks l, l + 64, .. (8
    values each) in order, the 64 lanes combine by the xor butterfly 32, 16, .., 1; mean = sum / C; the squares of v - mean the
    same way; rstd = rsqrt(q / C + eps); ((v - mean) * rstd) * gamma + beta, every operation rounded (no contraction), one
    rounding to bf16.  mutate ('eps', value): another eps; ('skip_chunk', ch): chunk ch left out of both sums.
    -> y bf16, or (rounded=False) the float32 values before that rounding."""
    f32 = torch.float32
    v = (case["x"].cpu().to(f32) + case["residual"].cpu().to(f32)).to(torch.bfloat16).to(f32)
    rows, C = v.shape
    live = torch.zeros(256, dtype=f32)
    live[: C // 8] = 1.0
    if mutate is not None and mutate[0] == "skip_chunk":
        live[mutate[1]] = 0.0
    live = live.reshape(4, 64)[None, :, :, None]                         # chunk ch = lane + 64 k -> [k][lane]
    lanes = torch.arange(64)

    def wave_sum(t):                                                     # t [rows][C] -> [rows][1]
        t = torch.nn.functional.pad(t, (0, 2048 - C)).reshape(rows, 4, 64, 8) * live
        s = torch.zeros(rows, 64, dtype=f32)
        for k in range(4):
            for i in range(8):
                s = s + t[:, k, :, i]
        for o in (32, 16, 8, 4, 2, 1):
            s = s + s[:, lanes ^ o]
        return s[:, :1]

    eps = torch.tensor(mutate[1] if mutate is not None and mutate[0] == "eps" else case["eps"], dtype=f32)
    cf = torch.tensor(float(C), dtype=f32)
    mean = wave_sum(v) / cf
    d = v - mean
    rstd = torch.rsqrt(wave_sum(d * d) / cf + eps)
    y = d * rstd * case["gamma"].cpu().to(f32) + case["beta"].cpu().to(f32)
    return y.to(torch.bfloat16) if rounded else y
