"""The ViT kernels on exact operands: bf16 inputs for which bf16 x bf16 products, float32 accumulation and one bf16 rounding
have ONE possible result (util_vit_exact.py; the properties are proved on the CPU by test_vit_exact_spec.py).  Outputs are
pre-filled with NaN, every element is judged, and the comparison is bit equality — or, for the fused MLP, whose second
product sums rounded GELU values, a bound derived per element: one bf16 ulp of the result plus the float32 summation bound.
A dropped, doubled or misplaced term, a wrong table entry or hand-off slot, a key lost, counted twice or let in from behind
the sequence changes bits here; under the tolerances of test_vit_gpu.py it does not."""
import pytest
import torch

import util_vit_exact as U

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64


@pytest.fixture(scope="module")
def table():
    """The device's GELU table as [GT_N][2] bit patterns, indexed [(bits & 0x7fff) - (113 << 7)][sign]; its values are pinned
    by test_vit_gpu.py::test_xs_gelu_table_is_the_bf16_gelu_for_every_input."""
    from vit_colmap_amd.vit.hip_ops import gelu_table

    return U.device_table_bits(gelu_table(DEV))


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.bfloat16, device=DEV)


def _xs(case):
    from vit_colmap_amd.vit.hip_ops import XsLinear

    d = lambda t: None if t is None else t.to(DEV)
    return XsLinear(d(case["w"]), d(case["b"]), d(case["gamma"]), d(case["beta"]), U.EPS)


# ---- a. x-stationary GEMM, EPI_BIAS / EPI_RESIDUAL ------------------------------------------------------------------------
XS_SHAPES = [(rows, n) for rows in (1, 31, 33, 255, 257, 300) for n in (32, 96, 384, 1152, 1536)] + [(256 * 257 + 37, 96)]


@pytest.mark.parametrize("rows,n", XS_SHAPES)
def test_xs_linear_bits(rows, n):
    """out bits == bf16(h64 (+ residual)), h64 the float64 evaluation on the rounded operands: dense and sparse W, with and
    without the fused LayerNorm, and in place on the residual.  The last shape walks several row tiles per workgroup."""
    for kind in ("dense", "sparse"):
        for ln in (False, True):
            for epi in (U.EPI_BIAS, U.EPI_RESIDUAL):
                c = U.xs_case(rows, n, kind, ln, epi, seed=rows * 7 + n + 3 * epi + ln, device=DEV)
                lin = _xs(c)
                out = _nan(rows, n)
                lin(c["x"], epi, c["residual"], out=out)
                U.compare(out, c)
                if epi == U.EPI_RESIDUAL:
                    r2 = c["residual"].clone()
                    lin(c["x"], epi, r2, out=r2)
                    c["name"] += " in place"
                    U.compare(r2, c)


# ---- b. x-stationary GEMM, EPI_GELU ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [96, 1536, 1920])
@pytest.mark.parametrize("rows", [33, 300])
def test_xs_table_gelu_bits(rows, n, table):
    """fc1 form (LayerNorm fused, GELU from the table): out bits == table[bf16(h64)].  1920 is the last width at which
    table and bias share the LDS area."""
    from vit_colmap_amd.vit.hip_ops import gelu_table

    c = U.xs_case(rows, n, "sparse", True, U.EPI_GELU, seed=rows + n, device=DEV, table=table)
    out = _nan(rows, n)
    _xs(c)(c["x"], U.EPI_GELU, out=out, gelu_table=gelu_table(DEV))
    U.compare(out, c)


@pytest.mark.parametrize("rows,n", [(300, 1536), (33, 96)])
def test_xs_float_gelu_on_exact_pre_activations(rows, n):
    """Without a table the pre-activation is exact and only the float GELU errs: the float bound of
    test_xs_gelu_table_is_the_bf16_gelu_for_every_input, |err| <= 2^-8 |ref| + 2e-7 (1 + |h|)."""
    c = U.xs_case(rows, n, "sparse", True, U.EPI_GELU, seed=rows + n, device=DEV, gelu_float=True)
    out = _nan(rows, n)
    _xs(c)(c["x"], U.EPI_GELU, out=out)
    U.compare(out, c)


# ---- c. fused MLP ---------------------------------------------------------------------------------------------------------
def _run_mlp(case):
    from vit_colmap_amd.vit.hip_ops import FusedMlp

    p = case["p"]
    d = lambda t: t.float().to(DEV)
    mlp = FusedMlp(d(p["w1"]), d(p["b1"]), d(p["gamma"]), d(p["beta"]), d(p["w2"]), d(p["b2"]), U.EPS)
    assert torch.equal(U.device_table_bits(mlp.table), case["table"])
    x = case["x"].clone()
    mlp(x)
    return x


@pytest.mark.parametrize("rows", [1, 127, 129, 300, 128 * 256 + 128 * 3 + 5])
@pytest.mark.parametrize("n_hidden", [64, 768, 1536])
def test_fused_mlp_against_its_contract(rows, n_hidden, table):
    """x += fc2(gelu(fc1(LN(x)))) vs the contract step by step (x-hat rounded to bf16, exact h, g = table[bf16(h)], float64
    sum W2 g + b2 + x): |err| <= 2^-8 |ref| + 2 (nnz + 2) 2^-24 (sum |w2 g| + |b2| + |x|), under 1e-3 beside the ulp term."""
    c = U.mlp_case(rows, n_hidden, seed=rows + n_hidden, device=DEV, table=table)
    assert not bool(c["fblock"].any())
    assert bool(((c["p"]["w2"] != 0).sum(dim=0) >= 1).all()), "a hidden unit feeds no output"
    assert float((c["bound"] - 2.0 ** -8 * c["ref"].abs()).max()) < 1e-3
    U.compare(_run_mlp(c), c)


@pytest.mark.parametrize("rows", [129, 300])
@pytest.mark.parametrize("n_hidden", [64, 768, 1536])
def test_fused_mlp_float_path_blocks(rows, n_hidden, table):
    """One hidden unit in every third 32-chunk sits at +-16 or at h == 0: those (32 rows x 32 hidden) blocks take the float
    path (gemm.hip gelu_table_slice, slice 15).  The reference evaluates the float path's own formula (gemm.hip gelu_erf2)
    for exactly those blocks and widens their units' share of the bound by one bf16 ulp of g."""
    c = U.mlp_case(rows, n_hidden, seed=rows + n_hidden + 1, device=DEV, table=table, float_blocks=True)
    frac = float(c["fblock"].float().mean())
    assert 0.25 <= frac <= 0.75, frac                                    # at least a quarter of the blocks of each kind
    U.compare(_run_mlp(c), c)


# ---- d. attention ---------------------------------------------------------------------------------------------------------
def _attention_into(qkv, n_heads, q_prescaled, out):
    from vit_colmap_amd import _lib

    B, N, _ = qkv.shape
    _lib.check(_lib.load().vc_attention_bf16(_lib.ptr(qkv), B, N, n_heads, U.HD, int(q_prescaled), _lib.ptr(out), _lib.stream_ptr()),
               "vc_attention_bf16")
    return out


# Which pass stores the result (attention.hip:338-363): q_prescaled = 0 runs the EXACT pass alone.  Under q_prescaled = 1 the
# FAST pass runs first and a unit is recomputed by the exact pass when one of its rows fails the range test; the default
# groups hold, from N = 128 on, sets with no key in key block 0, whose rows always fail it, and every unit holds such rows:
# those cases judge the exact pass (and the redo itself).  The fast_pass cases keep every group in reach of block 0, so what
# they judge is the fast pass's own result: QT = 1 (N = 300) and QT = 2 (N = 520, 1531), the ring of three slots wrapping,
# the ragged last key block.  (1, 100, 2) has no group out of reach either way.
ATT_SHAPES = [(1, 100, 2), (1, 520, 2), (2, 300, 5), (1, 1531, 1)]
ATT_CASES = [(q, False) for q in (1, 0)] + [(1, True)]


@pytest.mark.parametrize("B,N,H", ATT_SHAPES)
@pytest.mark.parametrize("q_prescaled,fast_pass", ATT_CASES)
def test_attention_bits(B, N, H, q_prescaled, fast_pass):
    """Weights exactly 1 or 0, 1 / l exact: out bits == sum_{j in S} v[j] / |S|.  Groups: the first 64 keys, the last 64
    (ragged last key block), 64 across the block boundary, 32 spread out with key N - 1, and (not fast_pass) 32 behind key
    block 0.  fast_pass False: the exact pass from N = 128 on; fast_pass True: the fast pass (see above)."""
    c = U.attention_case(B, N, H, seed=B + N + H, device=DEV, fast_pass=fast_pass)
    assert U.leaves_fast_pass(c["groups"]) == (N >= 128 and not fast_pass)
    U.compare(_attention_into(c["qkv"], H, q_prescaled, _nan(B, N, H * U.HD)), c)


@pytest.mark.parametrize("B,N,H", [(1, 520, 2), (2, 300, 5)])
@pytest.mark.parametrize("q_prescaled,fast_pass", ATT_CASES)
def test_attention_group_of_48_keys(B, N, H, q_prescaled, fast_pass):
    """A group of 48 keys: 1/48 is not dyadic, its rows are judged at one bf16 ulp of the exact value (float32 division errs
    by 2^-23 relative, far below half a bf16 ulp); the other groups' rows still bit for bit.  Passes as in test_attention_bits."""
    c = U.attention_case(B, N, H, seed=B + N + H + 1, device=DEV, odd_group=True, fast_pass=fast_pass)
    assert U.leaves_fast_pass(c["groups"]) == (not fast_pass)
    U.compare(_attention_into(c["qkv"], H, q_prescaled, _nan(B, N, H * U.HD)), c)


# ---- e. the staged GEMMs on dense dyadic operands -------------------------------------------------------------------------
def _dyadic(shape, g, lo, hi, step):
    return (torch.randint(lo, hi + 1, shape, generator=g).to(F64) * step).to(DEV)


def _pm_weights(shape, g):
    return (U.choice((0.25, 0.5, 1.0), shape, g) * (torch.randint(0, 2, shape, generator=g) * 2 - 1).to(F64)).to(DEV)


def _linear_bits(rows, K, N, epi):
    from vit_colmap_amd.vit.hip_ops import linear

    g = U.gen(rows + K + N + epi)
    x, w = _dyadic((rows, K), g, -8, 8, 0.25), _pm_weights((N, K), g)
    b = _dyadic((N,), g, -8, 8, 0.25)
    r = _dyadic((rows, N), g, -32, 32, 0.125) if epi == U.EPI_RESIDUAL else None
    h = x @ w.t() + b + (0 if r is None else r)
    out = _nan(rows, N)
    linear(U.to_bf16(x), U.to_bf16(w), U.to_bf16(b), epi, None if r is None else U.to_bf16(r), out=out)
    U.compare(out, dict(name=f"linear {rows}x{K}x{N} epi={epi}", expect_bits=U.f64_to_bits(U.bf16_rne(h))))


@pytest.mark.parametrize("rows", [129, 1025])
@pytest.mark.parametrize("K,N", [(64, 256), (768, 768)])
@pytest.mark.parametrize("epi", [U.EPI_BIAS, U.EPI_RESIDUAL])
def test_linear_bits(rows, K, N, epi):
    """vc_linear_bf16: x in multiples of 1/4, W in {+-1/4, +-1/2, +-1} — products are multiples of 2^-4 and sum |product| <
    2^12, every partial sum is a float32 number.  These shapes run the 128 x 128 tile, with one and with twelve K steps."""
    _linear_bits(rows, K, N, epi)


@pytest.mark.parametrize("epi", [U.EPI_BIAS, U.EPI_RESIDUAL])
def test_linear_bits_on_the_256_tile(epi):
    """vc_linear_bf16 takes the 256 x 256 tile once its tiles fill half the CUs (gemm.hip vc_linear_bf16: tiles x 2 >= CUs).
    4097 rows are 17 row tiles, ragged; the width is chosen from the device's CU count so that the condition holds
    (2048 columns up to 272 CUs); hip_ops.linear_tile_rows answers for the form."""
    from vit_colmap_amd.vit.hip_ops import linear_tile_rows

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tiles_n = max(8, -(-cus // (2 * 17)))
    assert linear_tile_rows(4097, 256 * tiles_n) == 256, (cus, tiles_n)
    _linear_bits(4097, 64, 256 * tiles_n, epi)


def test_conv_taps_bits():
    """vc_conv_taps_bf16 (the 256 x 256 tile as an implicit GEMM), 3 x 3 taps on a (2, 5, 7, 64) batch -> 256 features, the
    spare row behind the batch filled with junk first.  EPI_BIAS only: the entry has no residual epilogue and refuses one."""
    from vit_colmap_amd import _lib
    from vit_colmap_amd.vit.hip_ops import conv_rows, conv_taps

    B, H, W, C, N = 2, 5, 7, 64, 256
    g = U.gen(17)
    xr = conv_rows(B, H, W, C, DEV)
    x = _dyadic(tuple(xr.shape), g, -8, 8, 0.25)
    xr.copy_(U.to_bf16(x))
    w = _pm_weights((N, 3, 3, C), g)
    b = _dyadic((N,), g, -8, 8, 0.25)
    img = x[: B * H * W].reshape(B, H, W, C)
    ref = b.reshape(1, 1, 1, N).expand(B, H, W, N).clone()
    for ty in range(3):
        for tx in range(3):
            dy, dx = ty - 1, tx - 1
            ys, ye, xs, xe = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
            ref[:, ys:ye, xs:xe] += img[:, ys + dy:ye + dy, xs + dx:xe + dx] @ w[:, ty, tx].t()
    out = _nan(B * H * W, N)
    conv_taps(xr, U.to_bf16(w.reshape(N, 9 * C)), U.to_bf16(b), B, H, W, 3, 3, -1, -1, U.EPI_BIAS, out=out)
    assert not bool(xr[B * H * W].any())
    U.compare(out, dict(name="conv_taps", expect_bits=U.f64_to_bits(U.bf16_rne(ref.reshape(B * H * W, N)))))
    with pytest.raises(_lib.HipLibraryError):
        conv_taps(xr, U.to_bf16(w.reshape(N, 9 * C)), U.to_bf16(b), B, H, W, 3, 3, -1, -1, U.EPI_RESIDUAL, out=out)


# ---- the comparisons are not vacuous: the kernels on operands with ONE defect must fail them ------------------------------
# The defects of test_vit_exact_spec.py's mutants, made in the operands the kernel receives (the reference keeps the intact ones).
def test_xs_with_one_doubled_weight_is_caught():
    c = U.xs_case(300, 384, "sparse", True, U.EPI_BIAS, seed=5, device=DEV)
    col = 200
    k = int(torch.nonzero(c["w"][col])[0])
    wrong = dict(c, w=c["w"].clone())
    wrong["w"][col, k] *= 2
    out = _nan(300, 384)
    _xs(wrong)(c["x"], U.EPI_BIAS, out=out)
    bad = U.bits_of(out) != c["expect_bits"]
    assert bool(bad[:, col].all()) and int(bad.sum()) == 300            # exactly that column, on every row
    with pytest.raises(AssertionError):
        U.compare(out, c)


def test_mlp_with_two_exchanged_w2_columns_is_caught(table):
    c = U.mlp_case(129, 768, seed=6, device=DEV, table=table)
    w2 = c["p"]["w2"]
    k1, k2 = int(torch.nonzero(w2[0] != 0)[0]), int(torch.nonzero(w2[0] == 0)[0])
    wrong = dict(c, p=dict(c["p"], w2=w2.clone()))
    wrong["p"]["w2"][:, [k1, k2]] = w2[:, [k2, k1]]
    with pytest.raises(AssertionError):
        U.compare(_run_mlp(wrong), c)


@pytest.mark.parametrize("fast_pass", [False, True])
@pytest.mark.parametrize("defect", ["key dropped", "key let in with zero V"])
def test_attention_with_one_wrong_key_is_caught(fast_pass, defect):
    """q_prescaled = 1 at N = 520 (QT = 2): a key of the ragged last block taken out of the 'last keys' group, or a key that no
    row asks for let into the first group with zero V (only that group's row sums see it) — in the exact pass's result and
    in the fast pass's."""
    B, N, H = 1, 520, 2
    c = U.attention_case(B, N, H, seed=7, device=DEV, fast_pass=fast_pass)
    qkv = c["qkv"].clone().reshape(B, N, 3, H, U.HD)
    if defect == "key dropped":
        assert N - 1 in c["groups"][1]
        qkv[0, N - 1, 1, 0, int(c["dims"][0, 0, 1])] = -128.0
    else:
        free = next(j for j in range(N - 1, 95, -1) if all(j not in s for s in c["groups"]))
        qkv[0, free, 1, 0, int(c["dims"][0, 0, 0])] = 0.0
        qkv[0, free, 2, 0] = 0.0
    with pytest.raises(AssertionError):
        U.compare(_attention_into(qkv.reshape(B, N, -1), H, 1, _nan(B, N, H * U.HD)), c)
