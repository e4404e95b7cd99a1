"""GPU tests of the F / H scoring kernels (csrc/two_view.hip) through the ABI: vc_two_view_score and vc_two_view_inliers
against oracle.two_view_oracle.inliers_f32, bit for bit, on output buffers the test owns (pre-filled with sentinels, guard
elements behind them: util_two_view.run_score / run_mask), over the launch shapes, ragged and empty pairs, special models, error
thresholds and the decision boundary; and the argument checks of the two entries."""
import numpy as np
import pytest
import torch

from oracle import two_view_oracle as tv
import util_two_view as u

pytestmark = pytest.mark.gpu
MODELS = ["F", "H"]


def hypotheses_for(model, sizes, k, seed0=70):
    """One synthetic pair per size (F: planar and general scenes alternate; H: every fourth is general) -> (pts list, hyp float32 (P, k, 9)).  A pair too small to
    sample from gets the hypotheses of a 300-match scene: its models are arbitrary, its matches are what is counted."""
    pts_l, hyps = [], []
    spare = u.scene_hypotheses(model, seed0, 300, False, k)[1]
    for p, n in enumerate(sizes):
        pts, hyp = u.scene_hypotheses(model, seed0 + p, max(n, 20), p % 2 == 1 if model == "F" else p % 4 != 3, k)
        pts_l.append(pts[:n])
        hyps.append(hyp if n >= 20 else spare)
    return pts_l, np.stack(hyps)


# ---- hypothesis counts ---------------------------------------------------------------------------------------------------------
HYP_SIZES = [1000, 77, 0, 15]


@pytest.mark.parametrize("model", MODELS)
def test_counts_equal_the_oracle_for_every_launch_shape(model):
    """K on both sides of the `groups` switch at 64 (one round per wave below it; the strided loop with 1 to 9 rounds, unequal
    within a workgroup, from it) and the single-hypothesis shape of the refit, over pairs of 1000, 77, 0 and 15 matches."""
    pts_l, hyp = hypotheses_for(model, HYP_SIZES, 515)
    batch = u.device_batch(pts_l)
    want = u.ref_counts(model, hyp, pts_l)                                     # computed once; K hypotheses are a prefix
    assert len(set(want[0])) > 10 and len(set(want[1])) > 10, "the test would be comparing constants"
    assert (want[2] == 0).all()
    for K in (1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 67, 128, 512, 515):
        got = u.run_score(model, pts_l, hyp[:, :K], batch=batch)
        assert np.array_equal(got, want[:, :K]), (K, np.argwhere(got != want[:, :K])[:5])


# ---- match counts ---------------------------------------------------------------------------------------------------------------
MATCH_SIZES = [0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 513, 1000]


def match_sweep_sizes():
    """Every size once in a seeded order, between an empty first pair, two consecutive empty pairs and an empty last pair."""
    order = [MATCH_SIZES[i] for i in np.random.RandomState(17).permutation(len(MATCH_SIZES))]
    sizes = [0] + order[:7] + [0, 0] + order[7:] + [0]
    starts = np.cumsum([0] + sizes[:-1])
    assert sum(s % 64 != 0 for s in starts) >= 10                              # pair starts are not multiples of the wave
    return sizes


@pytest.mark.parametrize("model", MODELS)
def test_counts_and_masks_equal_the_oracle_for_every_pair_length(model):
    sizes = match_sweep_sizes()
    pts_l, hyp = hypotheses_for(model, sizes, 9, seed0=90)
    batch = u.device_batch(pts_l)
    want = u.ref_counts(model, hyp, pts_l)
    assert len(set(want.reshape(-1))) > 10
    got = u.run_score(model, pts_l, hyp, batch=batch)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    best = hyp[np.arange(len(sizes)), want.argmax(axis=1)]
    assert u.ref_mask(model, best, pts_l).sum() > 500
    for models in (hyp[:, 0], best):
        assert np.array_equal(u.run_mask(model, pts_l, models, batch=batch), u.ref_mask(model, models, pts_l))
    nan = np.full((len(sizes), 9), np.nan, np.float32)
    assert not u.run_mask(model, pts_l, nan, batch=batch).any()                # written everywhere (run_mask), 0 everywhere


# ---- many pairs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_counts_and_masks_equal_the_oracle_over_two_thousand_short_pairs(model):
    """A grid that is large in x: 2000 pairs of 15 to 40 matches cut from one scene in order, 8 hypotheses each."""
    rs = np.random.RandomState(23)
    sizes = rs.randint(15, 41, 2000)
    pts, pool = u.scene_hypotheses(model, 51, 1000, model == "H", 64)
    starts = rs.randint(0, len(pts) - 40, len(sizes))
    pts_l = [pts[s:s + n] for s, n in zip(starts, sizes)]
    hyp = pool[rs.randint(0, len(pool), (len(sizes), 8))]
    batch = u.device_batch(pts_l)
    want = u.ref_counts(model, hyp, pts_l)
    assert len(set(want.reshape(-1))) > 10
    got = u.run_score(model, pts_l, hyp, batch=batch)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert np.array_equal(u.run_mask(model, pts_l, hyp[:, 3], batch=batch), u.ref_mask(model, hyp[:, 3], pts_l))


# ---- special models, error thresholds -------------------------------------------------------------------------------------------
def special_models(model, m9, x0):
    out = []
    for pos, v in ((4, np.nan), (None, np.nan), (2, np.inf), (7, -np.inf), (None, 0.0)):
        s = m9.copy()
        if pos is None:
            s[:] = v
        else:
            s[pos] = v
        out.append(s)
    s = m9.copy()
    s[6:] = 0                                                 # H with a zero third row: pw = 0 for every match
    out.append(s)
    s = m9.copy()
    s[6:] = (1.0, 0.0, -x0)                                   # pw = x1 - x0: exactly 0, positive and negative on integer keypoints
    out.append(s)
    out.append(np.array([0, 0, 0, 0, 0, 0, 1, 0, -x0], np.float32))       # H: p = (0, 0, pw), so only `0 <= 0` at pw == 0 could count
    return out + list(u.scale_sweep(m9))


N_SPECIAL = 8


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("max_error", [4.0, 0.75, 0.0])
def test_special_models_and_error_thresholds(model, max_error):
    """NaN and infinite entries, the zero matrix, a vanishing and a sign-changing pw, and the power-of-two scale sweep (into
    overflow at one end, the denormal range and zero at the other) on a float pair and an integer-grid pair."""
    pts_f, m9 = u.best_hypothesis(model)
    kp1, kp2, m = u.grid_pair(14.0)
    pts_g = np.concatenate([kp1[m[:, 0]], kp2[m[:, 1]]], axis=1)
    x0 = float(kp1[7, 0])
    pw = pts_g[:, 0] - x0
    assert (pw == 0).sum() == 15 and (pw < 0).any() and (pw > 0).any()
    shift = np.array([1, 0, 14, 0, 1, 0, 0, 0, 1], np.float32)      # the grid pair's own geometry: every match fits exactly
    hyp = np.stack([np.stack(special_models(model, m9, x0) + [m9]), np.stack(special_models(model, shift if model == "H" else m9, x0) + [shift])])
    if model == "F":
        hyp[1, -1] = [0, 0, 0, 0, 0, -1, 0, 1, 0]                   # F of a pure shift in x: y2 = y1
    pts_l = [pts_f, pts_g]
    want = u.ref_counts(model, hyp, pts_l, max_error)
    got = u.run_score(model, pts_l, hyp, max_error)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert (want[:, :5] == 0).all()                                 # NaN, infinite and zero models
    assert want[1, -1] == 300                                       # residual exactly 0: an inlier at every threshold, 0 included
    if model == "H":
        assert (want[:, 5] == 0).all() and want[1, 6] <= 285 and want[1, 7] == 0      # never a match with pw == 0
    if max_error == 4.0:
        assert len(set(want[0])) >= 3 and want[0].max() > 100
    for k in (0, 4, 6, 7, hyp.shape[1] - 1, N_SPECIAL + 3, N_SPECIAL + 30, N_SPECIAL + 50):
        assert np.array_equal(u.run_mask(model, pts_l, hyp[:, k], max_error), u.ref_mask(model, hyp[:, k], pts_l, max_error)), k


# ---- the decision boundary -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_threshold_set_agrees_with_the_oracle_on_every_point(model):
    """Correspondences whose residual is the threshold to within 2e-5: a fused multiply-add anywhere in the test changes the
    answer on several per cent of them (test_two_view.py asserts at least 1 % for an emulated contraction), so this fails if the
    library loses -ffp-contract=off.  `<` in place of `<=` fails here too (a boundary point whose two sides are equal floats),
    and on the exact-fit models at max_error = 0 above."""
    m9, pts = u.threshold_set(model)
    want = tv.inliers_f32(model, m9, pts)
    got = u.run_mask(model, [pts], m9[None])
    assert np.array_equal(got, want.astype(np.uint8)), f"{int((got != want).sum())} of {len(pts)} boundary points differ"
    assert u.run_score(model, [pts], m9[None, None])[0, 0] == want.sum()


# ---- argument checks -----------------------------------------------------------------------------------------------------------
def test_argument_checks_refuse_before_anything_is_launched():
    from vit_colmap_amd import _lib

    lib = _lib.load()
    INVALID, UNSUPPORTED = _lib.VC_ERR_INVALID_ARG, _lib.VC_ERR_UNSUPPORTED
    pts_np, m9 = u.best_hypothesis("F")
    pts, off = u.device_batch([pts_np[:40]])
    hyp = torch.from_numpy(np.stack([m9, m9])[None]).cuda()
    counts = torch.full((2 + u.GUARD,), u.COUNT_SENTINEL, dtype=torch.int32, device="cuda")
    mask = torch.full((40 + u.GUARD,), u.MASK_SENTINEL, dtype=torch.uint8, device="cuda")
    misaligned = _lib.ptr(pts.reshape(-1)[1:])                                  # 4 bytes past a 16-byte boundary
    nan = float("nan")

    def untouched():
        torch.cuda.synchronize()
        return bool((counts == u.COUNT_SENTINEL).all()) and bool((mask == u.MASK_SENTINEL).all())

    score = [_lib.ptr(pts), _lib.ptr(off), 1, _lib.ptr(hyp), 2, 0, 4.0, _lib.ptr(counts), _lib.stream_ptr()]
    inl = [_lib.ptr(pts), _lib.ptr(off), 1, _lib.ptr(hyp), 0, 4.0, _lib.ptr(mask), _lib.stream_ptr()]
    cases = [(lib.vc_two_view_score, score, [(2, -1), (4, -1), (5, 2), (5, -1), (0, None), (1, None), (3, None), (7, None),
                                            (0, misaligned), (6, -1.0), (6, nan)]),
             (lib.vc_two_view_inliers, inl, [(2, -1), (4, 2), (4, -1), (0, None), (1, None), (3, None), (6, None),
                                            (0, misaligned), (5, -0.5), (5, nan)])]
    for fn, good, bad in cases:
        for pos, value in bad:
            args = list(good)
            args[pos] = value
            assert fn(*args) == INVALID, (fn.__name__, pos, value)
    for pos in (2, 4):                                                          # nothing to do: VC_OK and nothing written
        args = list(score)
        args[pos] = 0
        assert lib.vc_two_view_score(*args) == _lib.VC_OK, pos
    args = list(inl)
    args[2] = 0
    assert lib.vc_two_view_inliers(*args) == _lib.VC_OK
    args = list(score)
    args[2] = 65535 * 32 + 1
    assert lib.vc_two_view_score(*args) == UNSUPPORTED
    assert untouched()
    # the same arguments unchanged do run
    assert lib.vc_two_view_score(*score) == _lib.VC_OK and lib.vc_two_view_inliers(*inl) == _lib.VC_OK
    torch.cuda.synchronize()
    want = tv.inliers_f32("F", m9, pts_np[:40])
    assert counts.cpu().numpy().tolist() == [int(want.sum())] * 2 + [u.COUNT_SENTINEL] * u.GUARD
    assert np.array_equal(mask.cpu().numpy(), np.concatenate([want.astype(np.uint8), np.full(u.GUARD, u.MASK_SENTINEL, np.uint8)]))
