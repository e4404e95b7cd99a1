"""The selection, score and descriptor kernels (csrc/select.hip) across the options and shapes the C ABI accepts,
against oracle/select_oracle.py.

Integer stages (binning, top-k, NMS, keypoint coordinates, quantiser) are asserted bit-exact, on score maps that are
INPUTS of the entry or the GPU's own; float stages use the tolerances of tests/test_select_gpu.py.  Refusals are return
codes of the raw entry: the output buffers keep their sentinel, nothing was launched.

Ties.  The reference orders with `torch.topk` / `torch.argsort`, whose order among equal scores is unspecified; the
header states the total order (score descending, position ascending) and the oracle implements it with stable sorts,
so on tied maps the expectation below is the header's order, not the reference's.
"""
import numpy as np
import pytest
import torch

from oracle import select_oracle as so
from util_select import ATTAINABLE_D2, radii_near_root, reference_suppresses, tokens_from_fmap

pytestmark = pytest.mark.gpu

VC_OK, VC_ERR_INVALID_ARG, VC_ERR_UNSUPPORTED = 0, -1, -2
F32 = np.float32
SENTINEL = -7


# ---------------------------------------------------------------------------------------------------------------
# selection
# ---------------------------------------------------------------------------------------------------------------
def admission(H, W, target, bin_size, radius, kmax):
    """The entry's admission rule, restated from the header of vc_select_keypoints (in the entry's order)."""
    if min(H, W, target, bin_size, kmax) <= 0:
        return VC_ERR_INVALID_ARG
    if not (radius >= 0) or radius > 8:
        return VC_ERR_UNSUPPORTED
    nb = max(1, H // bin_size) * max(1, W // bin_size)
    cand = nb * max(1, target // nb)
    if H * W > 16384 or cand > 4096 or target > 4096:
        return VC_ERR_UNSUPPORTED
    if kmax < min(cand, target):
        return VC_ERR_INVALID_ARG
    if H * W * 8 + 80 * 1024 > 159 * 1024:
        return VC_ERR_UNSUPPORTED
    return VC_OK


def min_kmax(H, W, target, bin_size):
    nb = max(1, H // bin_size) * max(1, W // bin_size)
    return min(nb * max(1, target // nb), target)


def raw_select(score, target, bin_size, radius, kmax):
    """vc_select_keypoints on sentinel-filled buffers -> (status, yx, score, count, dbg_yx, dbg_score, dbg_count), numpy."""
    from vit_colmap_amd import _lib

    lib = _lib.load()
    s = torch.from_numpy(np.ascontiguousarray(score, F32)).cuda()
    B, H, W = s.shape
    yx = torch.full((B, kmax, 2), SENTINEL, dtype=torch.int32, device="cuda")
    sc = torch.full((B, kmax), float(SENTINEL), dtype=torch.float32, device="cuda")
    cnt = torch.full((B,), SENTINEL, dtype=torch.int32, device="cuda")
    dyx, dsc, dcnt = yx.clone(), sc.clone(), cnt.clone()
    status = lib.vc_select_keypoints(_lib.ptr(s), B, H, W, target, bin_size, radius, kmax, _lib.ptr(yx), _lib.ptr(sc),
                                     _lib.ptr(cnt), _lib.ptr(dyx), _lib.ptr(dsc), _lib.ptr(dcnt), _lib.stream_ptr())
    torch.cuda.synchronize()
    return (status,) + tuple(t.cpu().numpy() for t in (yx, sc, cnt, dyx, dsc, dcnt))


def assert_refused(score, target, bin_size, radius, kmax, code):
    status, yx, sc, cnt, dyx, dsc, dcnt = raw_select(score, target, bin_size, radius, kmax)
    assert status == code, (status, code, np.shape(score), target, bin_size, radius, kmax)
    for a in (yx, sc, cnt, dyx, dsc, dcnt):
        assert (a == SENTINEL).all()                   # a refusal launches nothing


def check_select(score, target, bin_size, radius, kmax=None):
    """Candidates, kept points, counts and the zero slots of every image of `score` (B, H, W) equal the oracle's."""
    score = np.ascontiguousarray(score, F32)
    B, H, W = score.shape
    if kmax is None:
        kmax = min_kmax(H, W, target, bin_size)
    what = (H, W, target, bin_size, radius, kmax)
    assert admission(H, W, target, bin_size, radius, kmax) == VC_OK, what
    status, yx, sc, cnt, dyx, dsc, dcnt = raw_select(score, target, bin_size, radius, kmax)
    assert status == VC_OK, (status,) + what
    kept_counts = []
    for b in range(B):
        coords, scores = so.spatial_binning_selection(score[b], target, bin_size)
        k = len(coords)
        assert dcnt[b] == k, what
        assert np.array_equal(dyx[b, :k].astype(np.int64), coords), what
        assert np.array_equal(dsc[b, :k], scores), what
        assert (dyx[b, k:] == SENTINEL).all() and (dsc[b, k:] == SENTINEL).all()   # documented: left as they were
        kept, kept_s = so.apply_nms(coords, scores, radius)
        m = len(kept)
        assert cnt[b] == m, what + (int(cnt[b]), m)
        assert np.array_equal(yx[b, :m].astype(np.int64), kept), what
        assert np.array_equal(sc[b, :m], kept_s), what
        assert not yx[b, m:].any() and not sc[b, m:].any(), what                   # slots behind the count are zero
        kept_counts.append(m)
    return kept_counts


GRIDS = [(1, 1), (1, 29), (31, 1), (3, 5), (7, 9), (16, 16), (32, 48), (33, 47), (34, 45), (17, 100), (64, 64), (85, 114),
         (79, 128), (3, 3371)]
BINS = [1, 2, 3, 5, 8, 16, 32, 200]
TARGETS = [1, 7, 100, 512, 2048, 4096]
RADII = [0.0, 0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 4.75, 8.0]


def test_selection_option_sweep():
    """Seeded draws over grid x bin size x target x radius x kmax; each is first put to the admission rule and either
    refused with the expected code or compared with the oracle.  The fixed list in front makes sure the classes its
    comments name are present whatever the draws are."""
    rs = np.random.RandomState(20240)
    draws = [
        (1, 1, 1, 1, 1.5), (1, 1, 16, 100, 8.0), (1, 29, 5, 7, 2.0), (31, 1, 8, 100, 1.0),      # 1x1, 1xN, Nx1
        (7, 9, 16, 100, 1.5), (3, 5, 200, 4096, 0.5),                                            # smaller than one bin; target > cells
        (32, 48, 16, 512, 2.5), (32, 48, 8, 7, 3.0),                                             # exactly n bins; target < bins
        (33, 47, 5, 100, 4.75), (85, 114, 16, 2048, 1.5), (79, 128, 32, 4096, 0.0),              # ragged margins; largest grid
        (79, 128, 2, 2048, 1.5), (64, 64, 1, 4096, 1.0), (17, 100, 3, 512, 8.0), (34, 45, 2, 100, 2.0),
    ]
    while len(draws) < 70:
        H, W = GRIDS[rs.randint(len(GRIDS))]
        draws.append((H, W, BINS[rs.randint(len(BINS))], TARGETS[rs.randint(len(TARGETS))], RADII[rs.randint(len(RADII))]))
    ran = refused = invalid = 0
    for i, (H, W, bin_size, target, radius) in enumerate(draws):
        kmax = min_kmax(H, W, target, bin_size) + (0 if i % 2 == 0 else 1 + rs.randint(40))     # the minimum, or more
        if i % 9 == 8:
            kmax = min_kmax(H, W, target, bin_size) - 1                                           # one short: invalid argument
        score = rs.rand(1, H, W).astype(F32)
        code = admission(H, W, target, bin_size, radius, kmax)
        if code != VC_OK:
            assert_refused(score, target, bin_size, radius, kmax, code)
            refused += 1
            invalid += code == VC_ERR_INVALID_ARG
        else:
            check_select(score, target, bin_size, radius, kmax)
            ran += 1
    assert ran >= 40 and refused - invalid >= 3 and invalid >= 3, (ran, refused, invalid)


def _tied_maps():
    rs = np.random.RandomState(7)
    H, W = 33, 47
    maps = {
        "levels3": np.floor(rs.rand(H, W) * 3) / 3,           # long ties inside bins, across bins and across the cut
        "levels17": np.floor(rs.rand(H, W) * 17) / 17,
        "zero": np.zeros((H, W)),
        "equal": np.full((H, W), 0.625),
    }
    plateau = rs.rand(H, W) * 0.5
    plateau[10:22, 12:20] = 0.75                              # one plateau across the borders of the 16-cell bins
    maps["plateau"] = plateau
    return {k: v.astype(F32) for k, v in maps.items()}


@pytest.mark.parametrize("name", ["levels3", "levels17", "zero", "equal", "plateau"])
def test_selection_ties_follow_the_total_order(name):
    """Equal scores: the per-bin rank, the merge of the bins' runs and the NMS ranking all break ties by position
    (header: score descending, then position ascending) — the oracle's stable order, not torch's unspecified one."""
    score = _tied_maps()[name][None]
    for bin_size, target, radius in ((16, 512, 1.5), (16, 100, 1.5), (8, 300, 2.5), (5, 7, 0.0), (3, 4096, 1.0), (64, 1000, 8.0),
                                     (16, 2, 0.0)):
        check_select(score, target, bin_size, radius)


def test_selection_long_nms_chains():
    """Scores falling monotonically in raster order and along the diagonals, every cell a candidate: the state of a
    point depends on its predecessor's, so the fixed point needs rounds on the order of the number of candidates."""
    H = W = 64
    idx = np.arange(H * W, dtype=np.float64).reshape(H, W)
    raster = (1.0 - idx / (H * W)).astype(F32)
    y, x = np.mgrid[0:H, 0:W]
    diag = (1.0 - ((y + x) * H + y) / (2.0 * H * H)).astype(F32)
    assert len(np.unique(raster)) == H * W and len(np.unique(diag)) == H * W
    for score in (raster, diag):
        for radius in (1.5, 8.0):
            (m,) = check_select(score[None], 4096, 64, radius)
            assert 1 < m < H * W


def test_selection_batches_equal_single_calls():
    rs = np.random.RandomState(11)
    H = W = 12
    maps = [rs.rand(H, W).astype(F32) for _ in range(3)]
    # an image whose candidates all die but one: one candidate per 4-cell bin (target = bins), each bin's maximum on the cell
    # nearest the centre, all within 4.75 cells of the strongest
    lone = (rs.rand(H, W) * 0.1).astype(F32)
    for bi, yy in enumerate((3, 5, 8)):
        for bj, xx in enumerate((3, 5, 8)):
            lone[yy, xx] = 0.5 + 0.01 * (bi * 3 + bj)
    lone[5, 5] = 1.0
    maps.insert(2, lone)
    maps.append(np.floor(rs.rand(H, W) * 4).astype(F32))          # a tied one in the same call
    batch = np.stack(maps)
    counts = check_select(batch, 9, 4, 4.75, kmax=13)
    assert counts[2] == 1 and max(counts) > 1
    _, yx, sc, cnt, *_ = raw_select(batch, 9, 4, 4.75, 13)
    for b in range(len(maps)):
        _, yx1, sc1, cnt1, *_ = raw_select(batch[b:b + 1], 9, 4, 4.75, 13)
        assert cnt1[0] == cnt[b] and np.array_equal(yx1[0], yx[b]) and np.array_equal(sc1[0], sc[b])
    check_select(batch, 144, 16, 1.5)
    check_select(batch, 50, 5, 2.0)


def test_selection_limits():
    rs = np.random.RandomState(3)
    big = rs.rand(1, 79, 128).astype(F32)                          # 10112 cells: the largest map the entry takes
    check_select(big, 4096, 16, 1.5)
    check_select(big, 2048, 8, 3.0, kmax=2048)
    assert_refused(rs.rand(1, 3, 3371).astype(F32), 512, 16, 1.5, 512, VC_ERR_UNSUPPORTED)      # 10113 cells
    assert_refused(rs.rand(1, 77, 137).astype(F32), 2048, 16, 1.5, 2048, VC_ERR_UNSUPPORTED)    # a 1920x1080 frame's grid
    small = rs.rand(1, 34, 45).astype(F32)
    assert_refused(small, 4097, 16, 1.5, 4097, VC_ERR_UNSUPPORTED)
    assert_refused(rs.rand(1, 80, 80).astype(F32), 100, 1, 1.5, 6400, VC_ERR_UNSUPPORTED)       # 6400 candidates before the cut
    assert_refused(small, 512, 16, 8.5, 512, VC_ERR_UNSUPPORTED)
    assert_refused(small, 512, 16, float("nan"), 512, VC_ERR_UNSUPPORTED)
    assert_refused(small, 512, 16, -0.5, 512, VC_ERR_UNSUPPORTED)
    assert min_kmax(34, 45, 512, 16) == 512
    assert_refused(small, 512, 16, 1.5, 511, VC_ERR_INVALID_ARG)
    assert_refused(small, 0, 16, 1.5, 16, VC_ERR_INVALID_ARG)
    assert_refused(small, 512, 0, 1.5, 512, VC_ERR_INVALID_ARG)
    check_select(small, 512, 16, 8.0)                               # the limits themselves are accepted
    check_select(small, 4096, 16, 1.5)


def test_nms_distance_rule_at_every_attainable_distance():
    """Two points at squared distance d2 (zeros elsewhere, one bin over the grid, target 2: they are the only candidates)
    and the radius at the float32 root of d2, one ulp below and one ulp above: the weaker point is suppressed iff
    `sqrt(d2) < r` in float32, the reference's comparison (vit_extractor.py:534-537).

    Before the rule was restated on integers the kernel compared `(float)d2 < r * r`; this test failed there at
    d2 = 37 (r = 6.082762718200684) and d2 = 61 (r = 7.8102498054504395), where the float32 square lies above d2 and
    the kernel dropped a point the reference keeps."""
    wrong = []
    n_cases = 0
    for d2, (a, b) in sorted(ATTAINABLE_D2.items()):
        score = np.zeros((1, 9, 9), F32)
        score[0, 0, 0] = 1.0
        score[0, a, b] = 0.5
        radii = [r for r in radii_near_root(d2, ulps=1, max_radius=8.0)] or [8.0]
        for r in radii + [8.0]:
            status, yx, sc, cnt, dyx, dsc, dcnt = raw_select(score, 2, 16, r, 2)
            assert status == VC_OK and dcnt[0] == 2
            assert np.array_equal(dyx[0], [[0, 0], [a, b]])
            want = 1 if reference_suppresses(d2, r) else 2
            kept, _ = so.apply_nms(np.array([[0, 0], [a, b]]), np.array([1.0, 0.5], F32), r)
            assert len(kept) == want
            n_cases += 1
            if cnt[0] != want or not np.array_equal(yx[0, :want], kept):
                wrong.append((d2, r, int(cnt[0]), want))
    assert n_cases > 100
    assert not wrong, wrong


# ---------------------------------------------------------------------------------------------------------------
# structure tensor and score map
# ---------------------------------------------------------------------------------------------------------------
def _st_check(got, fmap):
    C, H, W = fmap.shape
    ixx, iyy, ixy = so.structure_tensor_means(fmap)
    got = got.reshape(4, H, W)
    np.testing.assert_allclose(got[0], ixx, rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(got[1], iyy, rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(got[2], ixy, rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(got[3], fmap.mean(axis=0), rtol=1e-4, atol=1e-6)


def _offset_view(tokens, elems):
    """The same values in a slice of a flat buffer that starts 8 bytes into it: 16-byte alignment lost, so the entry takes the
    scalar path whatever C is."""
    flat = torch.empty(tokens.numel() + 16, dtype=tokens.dtype, device=tokens.device)
    view = flat[elems:elems + tokens.numel()].view(tokens.shape)
    view.copy_(tokens)
    assert flat.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 8 and view.is_contiguous()
    return view


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("C", [1, 5, 12, 91, 100, 8, 64, 520, 1536])
def test_structure_tensor_channel_counts_and_both_paths(C, dtype):
    """C % 8 != 0 runs the scalar loop, C % 8 == 0 the 16-byte loads (C > 512: a second trip of the lane loop); an aligned
    C viewed at an 8-byte offset runs the scalar loop on data the vector loop also computed."""
    from vit_colmap_amd.features import hip_select as hs

    B, H, W = 3, 5, 7
    rs = np.random.RandomState(100 + C)
    fmaps = rs.standard_normal((B, C, H, W)).astype(F32)
    toks = torch.from_numpy(np.stack([tokens_from_fmap(f) for f in fmaps])).cuda()
    if dtype == "bf16":
        toks = toks.to(torch.bfloat16)
        fmaps = toks.float().cpu().numpy().reshape(B, H * W, C).transpose(0, 2, 1).reshape(B, C, H, W)   # the rounded values
    assert toks.data_ptr() % 16 == 0
    st = hs.structure_tensor(toks, H, W).cpu().numpy()
    for b in range(B):
        _st_check(st[b], np.ascontiguousarray(fmaps[b]))
    if C % 8 == 0:
        st_scalar = hs.structure_tensor(_offset_view(toks, 2 if dtype == "f32" else 4), H, W).cpu().numpy()
        for b in range(B):
            _st_check(st_scalar[b], np.ascontiguousarray(fmaps[b]))
        np.testing.assert_allclose(st_scalar[:, :2], st[:, :2], rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(st_scalar[:, 2:], st[:, 2:], rtol=1e-4, atol=1e-6)


SCORE_GRIDS = [(1, 37), (41, 1), (2, 2), (3, 37), (5, 6), (128, 128), (79, 128)]


@pytest.mark.parametrize("grid", SCORE_GRIDS, ids=[f"{h}x{w}" for h, w in SCORE_GRIDS])
def test_score_map_all_methods_on_narrow_and_largest_grids(grid):
    from vit_colmap_amd.features import hip_select as hs

    H, W = grid
    C = 8
    rs = np.random.RandomState(H * 1000 + W)
    fmaps = rs.standard_normal((2, C, H, W)).astype(F32)
    toks = torch.from_numpy(np.stack([tokens_from_fmap(f) for f in fmaps])).cuda()
    st = hs.structure_tensor(toks, H, W)
    for method in ("harris", "dog", "combined"):
        s = hs.score_map(st, H, W, method).cpu().numpy()
        for b in range(2):
            np.testing.assert_allclose(s[b], so.distinctiveness(fmaps[b], method), rtol=1e-3, atol=2e-5, err_msg=f"{method} {grid}")
            if method != "combined" and H * W > 1:
                assert s[b].min() == 0.0 and s[b].max() == 1.0


def test_score_map_constant_features_and_cell_limit():
    from vit_colmap_amd import _lib
    from vit_colmap_amd.features import hip_select as hs

    H, W, C = 9, 13, 8
    fmap = np.full((C, H, W), 0.5, F32)
    st = hs.structure_tensor(torch.from_numpy(tokens_from_fmap(fmap)[None]).cuda(), H, W)
    got = {m: hs.score_map(st, H, W, m).cpu().numpy()[0] for m in ("harris", "dog", "combined")}
    assert not got["harris"].any()                                  # no gradient anywhere: exactly 0
    assert got["dog"].max() == 1.0 and got["dog"].min() == 0.0      # zero padding makes the border differ
    for m in got:
        np.testing.assert_allclose(got[m], so.distinctiveness(fmap, m), rtol=1e-3, atol=2e-5)
    assert so.distinctiveness(fmap, "harris").max() == 0 and so.distinctiveness(fmap, "dog").max() == 1
    np.testing.assert_allclose(got["combined"].max(), 0.5, rtol=1e-6)
    # 16385 cells: refused, nothing written
    lib = _lib.load()
    H, W = 5, 3277
    st = torch.zeros((1, 4, H * W), dtype=torch.float32, device="cuda")
    out = torch.full((1, H, W), float(SENTINEL), dtype=torch.float32, device="cuda")
    assert lib.vc_score_map(_lib.ptr(st), 1, H, W, 0, _lib.ptr(out), _lib.stream_ptr()) == VC_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------------
# descriptors
# ---------------------------------------------------------------------------------------------------------------
def _check_u8(got, ref, share=2e-3):
    diff = np.abs(got.astype(np.int32) - ref.astype(np.int32))
    assert diff.max(initial=0) <= 1 and (diff != 0).mean() < share, (int(diff.max(initial=0)), float((diff != 0).mean()))


def _grid_positions(H, W, n, rs):
    """(y, x): the four corners, the last row and column (where the +1 tap is outside), the first ones, then random cells."""
    fixed = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H - 1, 2), (2, W - 1), (0, 3), (3, 0), (H - 2, W - 2), (1, 1)]
    rest = [(int(rs.randint(H)), int(rs.randint(W))) for _ in range(n - len(fixed))]
    pos = np.array(fixed + rest, np.int64)
    assert H >= 4 and W >= 4 and (pos >= 0).all() and (pos[:, 0] < H).all() and (pos[:, 1] < W).all()
    return pos


def _make_tokens(rs, B, H, W, C, dtype):
    fmaps = rs.standard_normal((B, C, H, W)).astype(F32)
    toks = torch.from_numpy(np.stack([tokens_from_fmap(f) for f in fmaps])).cuda()
    if dtype == "bf16":
        toks = toks.to(torch.bfloat16)
        fmaps = toks.float().cpu().numpy().reshape(B, H * W, C).transpose(0, 2, 1).reshape(B, C, H, W)
    return toks, np.ascontiguousarray(fmaps)


DESCRIBE_SHAPES = [(64, None), (64, 100), (96, 1), (96, 63), (384, None), (384, 64), (768, 128), (768, 256), (1024, None),
                   (1024, 256), (1536, None), (1536, 128), (1536, 100)]


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("C,dd", DESCRIBE_SHAPES, ids=[f"C{c}-dd{d}" for c, d in DESCRIBE_SHAPES])
def test_describe_token_types_channels_and_projections(C, dd, dtype):
    """vc_describe as the product calls it (bf16 tokens) and with float32 ones; three images with counts kmax, 1 and 0, then
    a count above kmax; frames whose scale factors are not dyadic."""
    from vit_colmap_amd.features import hip_select as hs

    B, H, W, kmax = 3, 6, 7, 16
    rs = np.random.RandomState(C * 7 + (dd or 0))
    toks, fmaps = _make_tokens(rs, B, H, W, C, dtype)
    proj_np = None if dd is None else (rs.standard_normal((C, dd)) / np.sqrt(C)).astype(F32)
    proj = None if dd is None else torch.from_numpy(proj_np).cuda()
    D = C if dd is None else dd
    pos = np.stack([_grid_positions(H, W, kmax, rs) for _ in range(B)])
    yx = torch.from_numpy(pos.astype(np.int32)).cuda()
    resized, orig = ((1596, 1190), (1600, 1200)) if C % 128 == 0 else ((994, 742), (1000, 750))
    for counts in ((kmax, 1, 0), (kmax + 5, kmax, 3)):
        cnt = torch.tensor(counts, dtype=torch.int32, device="cuda")
        kp, u8, f32 = (t.cpu().numpy() for t in hs.describe(toks, H, W, yx, cnt, resized, orig, proj, want_f32=True))
        for b in range(B):
            n = min(counts[b], kmax)                                   # a count above kmax is clamped
            d = so.gather_descriptors(fmaps[b], pos[b, :n])
            if proj_np is not None:
                d = so.project(d, proj_np)
            d = so.l2_normalize(d)
            assert np.array_equal(kp[b, :n], so.map_keypoints(pos[b, :n], (H, W), resized, orig))      # float32, bit-exact
            np.testing.assert_allclose(f32[b, :n], d, rtol=1e-3, atol=1e-6)
            if n:
                _check_u8(u8[b, :n], so.quantize_u8(d))
            assert np.array_equal(so.quantize_u8(f32[b]), u8[b])                                       # quantiser exact on own floats
            assert not kp[b, n:].any() and not u8[b, n:].any() and not f32[b, n:].any()                # rows at and behind the count
            assert f32[b, :n].shape == (n, D)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_describe_zero_and_negative_rows_both_normalisations(dtype):
    """Norm 0 (the 1e-12 clamps) and descriptors with every element negative (quantise to 0), through vc_describe (L2) and
    vc_describe_at (L2 and RootSIFT)."""
    from vit_colmap_amd.features import hip_select as hs

    H, W, C, kmax = 4, 5, 96, 8
    rs = np.random.RandomState(5)
    fm = np.stack([np.zeros((C, H, W), F32), -np.abs(rs.standard_normal((C, H, W))).astype(F32) - 0.25])
    toks = torch.from_numpy(np.stack([tokens_from_fmap(f) for f in fm])).cuda()
    if dtype == "bf16":
        toks = toks.to(torch.bfloat16)
        fm = np.ascontiguousarray(toks.float().cpu().numpy().reshape(2, H * W, C).transpose(0, 2, 1).reshape(2, C, H, W))
    pos = _grid_positions(H, W, 10, rs)[:kmax]
    yx = torch.from_numpy(np.stack([pos, pos]).astype(np.int32)).cuda()
    cnt = torch.tensor([kmax, kmax], dtype=torch.int32, device="cuda")
    kp, u8, f32 = (t.cpu().numpy() for t in hs.describe(toks, H, W, yx, cnt, (70, 56), (75, 60), None, want_f32=True))
    assert not f32[0].any() and not u8[0].any()                        # 0 / max(0, 1e-12) = 0
    assert (f32[1] < 0).all() and not u8[1].any()
    np.testing.assert_allclose(f32[1], so.l2_normalize(so.gather_descriptors(fm[1], pos)), rtol=1e-3, atol=1e-6)
    # the same cells through vc_describe_at: keypoints at the cell positions (feature size == grid == original size)
    kxy = torch.from_numpy(np.stack([pos[:, ::-1], pos[:, ::-1]]).astype(F32).copy()).cuda()
    for rootsift in (False, True):
        a8, a32 = (t.cpu().numpy() for t in hs.describe_at(toks, H, W, kxy, cnt, (W, H), (W, H), None, rootsift=rootsift,
                                                           want_f32=True))
        for b in range(2):
            d = so.sample_descriptors(fm[b], pos[:, 0].astype(F32), pos[:, 1].astype(F32))
            d = so.rootsift_normalize(d) if rootsift else so.l2_normalize(d)
            np.testing.assert_allclose(a32[b], d, rtol=1e-3, atol=1e-6)
            _check_u8(a8[b], so.quantize_u8(d), 5e-3 if rootsift else 2e-3)
            assert np.array_equal(so.quantize_u8(a32[b]), a8[b])
        if rootsift:   # every element clamps to 1e-8 before the root: the uniform descriptor 1 / sqrt(C)
            np.testing.assert_allclose(a32, 1.0 / np.sqrt(C), rtol=1e-5)
        else:
            assert not a32[0].any() and not a8.any()


FRAMES = {
    # name: (feature_wh, original_wh, pixels per cell in x, in y, factors exact in float32)
    "dyadic": ((144, 112), (288, 56), 32.0, 8.0, True),       # x scale 1/2 then 1/16, y scale 2 then 1/16
    "odd": ((126, 98), (180, 70), 20.0, 10.0, False),         # x scale 0.7 then 1/14, y scale 1.4 then 1/14
}


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("C,dd", [(64, None), (384, None), (768, 128)])
@pytest.mark.parametrize("frame", ["dyadic", "odd"])
@pytest.mark.parametrize("rootsift", [False, True], ids=["l2", "rootsift"])
def test_describe_at_both_normalisations(rootsift, frame, C, dd, dtype):
    """vc_describe_at with VC_NORM_L2 (sample_descriptors + l2_normalize) and VC_NORM_ROOTSIFT: keypoints at exact cell
    centres, between cells and outside the frame on all four sides, on a non-square scale."""
    from vit_colmap_amd.features import hip_select as hs

    H, W = 7, 9
    feat_wh, orig_wh, px, py, exact = FRAMES[frame]
    ow, oh = orig_wh
    rs = np.random.RandomState(C + (dd or 0))
    toks, fmaps = _make_tokens(rs, 2, H, W, C, dtype)
    proj_np = None if dd is None else (rs.standard_normal((C, dd)) / np.sqrt(C)).astype(F32)
    proj = None if dd is None else torch.from_numpy(proj_np).cuda()
    centres = [(px * i, py * j) for i, j in ((0, 0), (3, 2), (8, 6), (8, 0), (0, 6), (4, 3))]
    between = [(float(x), float(y)) for x, y in zip(rs.uniform(0, px * 8, 12), rs.uniform(0, py * 6, 12))]
    outside = [(-0.08 * ow, 0.4 * oh), (1.1 * ow, 0.4 * oh), (0.5 * ow, -0.1 * oh), (0.5 * ow, 1.1 * oh), (-3.0, -3.0),
               (ow + 1.0, oh + 1.0), (px * 8 + 0.5, py * 6 + 0.25)]
    kp = np.array(centres + between + outside, F32)
    n, kmax = len(kp), 28
    kpb = np.zeros((2, kmax, 2), F32)
    kpb[0, :n] = kp
    kpb[1, :5] = kp[-5:]
    cnt = torch.tensor([n, 5], dtype=torch.int32, device="cuda")
    u8, f32 = (t.cpu().numpy() for t in hs.describe_at(toks, H, W, torch.from_numpy(kpb).cuda(), cnt, feat_wh, orig_wh, proj,
                                                       rootsift=rootsift, want_f32=True))
    for b, rows in ((0, kp), (1, kp[-5:])):
        fx = (rows[:, 0] * F32(feat_wh[0] / ow)) * F32(W / feat_wh[0])                  # hybrid_extractor.py:249-254
        fy = (rows[:, 1] * F32(feat_wh[1] / oh)) * F32(H / feat_wh[1])
        if b == 0:
            if exact:
                assert np.array_equal(fx[:6], [0, 3, 8, 8, 0, 4]) and np.array_equal(fy[:6], [0, 2, 6, 0, 6, 3])
            assert fx.min() < 0 and fx.max() > W - 1 and fy.min() < 0 and fy.max() > H - 1
        d = so.sample_descriptors(fmaps[b], fy, fx)
        if proj_np is not None:
            d = so.project(d, proj_np)
        m = len(rows)
        if rootsift:
            d = so.rootsift_normalize(d)
            assert np.abs(f32[b, :m] - d).max() <= 1e-3 * np.abs(d).max()
            _check_u8(u8[b, :m], so.quantize_u8(d), 5e-3)
        else:
            d = so.l2_normalize(d)
            np.testing.assert_allclose(f32[b, :m], d, rtol=1e-3, atol=1e-6)
            _check_u8(u8[b, :m], so.quantize_u8(d))
        assert np.array_equal(so.quantize_u8(f32[b]), u8[b])
        assert not u8[b, m:].any() and not f32[b, m:].any()


def test_describe_lds_limit_and_degenerate_grids():
    """C = 2048 without projection needs exactly the 64 KiB of LDS the entry admits: it runs and is right; C = 2056 is
    refused; a grid with a single row or column has no align_corners scale and is an invalid argument."""
    from vit_colmap_amd import _lib
    from vit_colmap_amd.features import hip_select as hs

    lib = _lib.load()
    H, W, kmax = 4, 5, 6
    rs = np.random.RandomState(9)
    for dtype in ("bf16", "f32"):
        toks, fmaps = _make_tokens(rs, 1, H, W, 2048, dtype)
        pos = _grid_positions(H, W, 10, rs)[:kmax]
        yx = torch.from_numpy(pos[None].astype(np.int32)).cuda()
        cnt = torch.tensor([kmax], dtype=torch.int32, device="cuda")
        kp, u8, f32 = (t.cpu().numpy()[0] for t in hs.describe(toks, H, W, yx, cnt, (56, 42), (60, 45), None, want_f32=True))
        d = so.l2_normalize(so.gather_descriptors(fmaps[0], pos))
        np.testing.assert_allclose(f32, d, rtol=1e-3, atol=1e-6)
        _check_u8(u8, so.quantize_u8(d))
        assert np.array_equal(kp, so.map_keypoints(pos, (H, W), (56, 42), (60, 45)))

    def raw(H, W, C):
        t = torch.zeros((1, H * W, C), dtype=torch.float32, device="cuda")
        yx = torch.zeros((1, kmax, 2), dtype=torch.int32, device="cuda")
        cnt = torch.ones((1,), dtype=torch.int32, device="cuda")
        kp = torch.full((1, kmax, 2), float(SENTINEL), dtype=torch.float32, device="cuda")
        u8 = torch.full((1, kmax, C), 9, dtype=torch.uint8, device="cuda")
        st = lib.vc_describe(_lib.ptr(t), 0, 1, H, W, C, _lib.ptr(yx), _lib.ptr(cnt), kmax, None, 0, 56, 42, 60, 45, _lib.ptr(kp),
                             None, _lib.ptr(u8), _lib.stream_ptr())
        kxy = torch.zeros((1, kmax, 2), dtype=torch.float32, device="cuda")
        st_at = lib.vc_describe_at(_lib.ptr(t), 0, 1, H, W, C, _lib.ptr(kxy), _lib.ptr(cnt), kmax, None, 0, 56, 42, 60, 45, 0, None,
                                   _lib.ptr(u8), _lib.stream_ptr())
        torch.cuda.synchronize()
        assert bool((kp == SENTINEL).all()) and bool((u8 == 9).all())
        return st, st_at

    assert raw(4, 5, 2056) == (VC_ERR_UNSUPPORTED, VC_ERR_UNSUPPORTED)
    assert raw(1, 12, 64) == (VC_ERR_INVALID_ARG, VC_ERR_INVALID_ARG)
    assert raw(12, 1, 64) == (VC_ERR_INVALID_ARG, VC_ERR_INVALID_ARG)
