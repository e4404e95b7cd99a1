"""GPU tests of the F / H estimator around the scoring kernels (matching/_common.py, matching/two_view.py) against
oracle/two_view_oracle.py: the sampler on the device, the RANSAC tail with a refit the test owns (exact), the hypothesis half
of `_estimate`, and `verify_pairs` as a whole: index mapping around short pairs, the H branch, degenerate inputs, chunking."""
from functools import lru_cache

import numpy as np
import pytest
import torch

from oracle import two_view_oracle as tv
import util_two_view as u
from test_two_view import sampler_parity

pytestmark = pytest.mark.gpu
MODELS = ["F", "H"]
NUM_HYP = {"F": tv.NUM_HYP_F, "H": tv.NUM_HYP_H}
NAN9 = np.full(9, np.nan, np.float32)


def pair_id(i):
    """COLMAP pair ids of image ids that are not consecutive, so that the seeds (pair id mod 2^32) differ between pairs."""
    from vit_colmap_amd.database.colmap_db import pair_id_of

    return pair_id_of(3 * i + 1, 5 * i + 4)


def test_torch_sampler_equals_the_oracle_sampler_on_the_device():
    sampler_parity("cuda")


# ---- the RANSAC tail ------------------------------------------------------------------------------------------------------------
def tail_pairs(model):
    """-> list of dict(pts, hyp (K, 9), norm, kind, seed): the ragged batch of test_ransac_tail.  `seed` is set where hyp is
    exactly tv.hypotheses(model, pts, seed, K), so that tv.estimate_model applies.  Scenes chosen on the oracle (CPU)."""
    K, S = NUM_HYP[model], u.S_OF[model]

    def pair(scene, seed, kind="honest"):
        pts = u.scene_pts(*scene)
        hyp, norm = tv.hypotheses(model, pts, seed, K)
        return dict(pts=pts, hyp=hyp, norm=norm, kind=kind, seed=seed)

    taken = {"F": ((201, 200, 0.5, False), 778), "H": ((204, 120, 0.6, True), 781)}[model]       # refit 99 >= 96 / 45 >= 35
    rejected = {"F": ((200, 300, 0.3, False), 777), "H": ((247, 60, 0.0, False), 824)}[model]    # refit 197 < 198 / 17 < 18
    better = {"F": ((206, 500, 0.7, False), 783), "H": ((204, 120, 0.6, True), 781)}[model]      # refit 100 > 88 / 45 > 35
    pairs = [pair(*taken), pair(*rejected)]
    tie = pair((202, 300, 0.2, True), 779, "tie")                 # the best hypothesis copied to a later index: the lower one wins
    counts = [int(tv.inliers_f32(model, h, tie["pts"]).sum()) for h in tie["hyp"]]
    k = int(np.argmax(counts))
    tie["hyp"][K - 3] = tie["hyp"][k]
    assert k < K - 3
    tie["seed"] = None
    pairs.append(tie)
    void = pair((203, 40, 0.3, False), 780, "void")               # every hypothesis void: NaN model, empty mask, count 0
    void["hyp"][:], void["seed"] = np.nan, None
    pairs.append(void)
    pairs.append(dict(pts=np.zeros((0, 4), np.float32), hyp=np.tile(NAN9, (K, 1)), norm=None, kind="empty", seed=None))
    lone = pair((205, 40, 0.1, False), 782, "lone")               # one hypothesis that is not void
    keep = lone["hyp"][K // 3].copy()
    lone["hyp"][:], lone["seed"] = np.nan, None
    lone["hyp"][K // 3] = keep
    pairs.append(lone)
    few = pair((207, 30, 1.0, False), 784, "few")                 # pure outliers scored under models of another scene: the best
    donor = pairs[0]["hyp"]                                       # hypothesis has inliers, but fewer than a sample
    c = np.array([int(tv.inliers_f32(model, h, few["pts"]).sum()) for h in donor])
    few["hyp"][:], few["seed"] = np.nan, None
    sel = np.flatnonzero((c > 0) & (c < S))[:5]
    assert len(sel) >= 1, c.max()
    few["hyp"][10:10 + len(sel)] = donor[sel]
    pairs.append(few)
    pairs.append(pair(*better, kind="ok_false"))                  # the callback offers a better model but says ok = False
    pairs.append(pair(*taken, kind="nan_ok"))                     # the callback says ok = True and hands back NaN
    return pairs


def run_tail(model, pairs):
    """_ransac_tail with counts from _score and a refit callback that evaluates tv.refit on the CPU from the mask it is handed
    -> (final, mask, count, kbest, use) as numpy, and what the callback saw and returned."""
    from vit_colmap_amd.matching import _common

    S = u.S_OF[model]
    offs = np.cumsum([0] + [len(p["pts"]) for p in pairs])
    pts, offsets, _, _ = _common._pair_batch([p["pts"] for p in pairs], None, "cuda")
    hyp32 = torch.from_numpy(np.stack([p["hyp"] for p in pairs]).astype(np.float32)).cuda().contiguous()
    counts = _common._score(pts, offsets, hyp32, model, tv.MAX_ERROR).to(torch.int64)
    seen = {}

    def refit(mask, nbest):
        assert mask.dtype == torch.bool and mask.shape == (offs[-1],) and nbest.shape == (len(pairs),)
        mask_np = mask.cpu().numpy()
        out, ok = np.tile(NAN9, (len(pairs), 1)), np.zeros(len(pairs), bool)
        for p, pr in enumerate(pairs):
            mp = mask_np[offs[p]:offs[p + 1]]
            r = tv.refit(model, mp, pr["norm"]) if mp.sum() >= S else None
            if r is not None:
                out[p], ok[p] = r, True
            if pr["kind"] == "ok_false":
                assert r is not None
                ok[p] = False
            if pr["kind"] == "nan_ok":
                out[p], ok[p] = np.nan, True
        seen.update(mask=mask_np, nbest=nbest.cpu().numpy(), out=out, ok=ok)
        return torch.from_numpy(out).cuda(), torch.from_numpy(ok).cuda()

    res = _common._ransac_tail(hyp32, counts, lambda h: _common._score(pts, offsets, h, model, tv.MAX_ERROR),
                               lambda m: _common._mask(pts, offsets, m, model, tv.MAX_ERROR), refit)
    torch.cuda.synchronize()
    return [r.cpu().numpy() for r in res], seen, offs


def check_tail(model, pairs):
    (final, mask, count, kbest, use), seen, offs = run_tail(model, pairs)
    assert final.dtype == np.float32 and mask.dtype == bool and mask.shape == (offs[-1],)
    kinds = {}
    for p, pr in enumerate(pairs):
        pts, hyp, S = pr["pts"], pr["hyp"], u.S_OF[model]
        # the rule: most inliers, lowest index on ties; the refit is taken iff it is ok and has no fewer inliers; no inlier, no model
        c = np.array([int(tv.inliers_f32(model, h, pts).sum()) for h in hyp])
        k = int(np.argmax(c))
        best, bmask = hyp[k], tv.inliers_f32(model, hyp[k], pts)
        r, ok = seen["out"][p], bool(seen["ok"][p])
        rc = int(tv.inliers_f32(model, r, pts).sum())
        take = ok and rc >= c[k]
        want, n = (r, rc) if take else (best, int(c[k]))
        want = want if n > 0 else NAN9
        sl = slice(offs[p], offs[p + 1])
        assert np.array_equal(seen["mask"][sl], bmask) and seen["nbest"][p] == c[k], (p, pr["kind"])
        assert kbest[p] == k and bool(use[p]) == take and count[p] == n, (p, pr["kind"], kbest[p], k, use[p], take, count[p], n)
        assert np.array_equal(final[p], want, equal_nan=True), (p, pr["kind"])
        assert np.array_equal(mask[sl], tv.inliers_f32(model, want, pts)) and mask[sl].sum() == n, (p, pr["kind"])
        if pr["seed"] is not None and pr["kind"] == "honest":
            o9, omask = tv.estimate_model(model, pts, pr["seed"], len(hyp))
            assert np.array_equal(final[p], NAN9 if o9 is None else o9, equal_nan=True) and np.array_equal(mask[sl], omask), p
        kinds.setdefault(pr["kind"], []).append(dict(k=k, n=n, best=int(c[k]), rc=rc, take=take, S=S))
    return kinds


@pytest.mark.parametrize("model", MODELS)
def test_ransac_tail_follows_the_oracles_rule_exactly(model):
    kinds = check_tail(model, tail_pairs(model))
    S = u.S_OF[model]
    assert [d["take"] for d in kinds["honest"]] == [True, False]                  # one refit taken, one honestly rejected
    assert kinds["tie"][0]["k"] < NUM_HYP[model] - 3
    assert kinds["void"][0]["n"] == 0 and kinds["empty"][0]["n"] == 0
    assert kinds["lone"][0]["k"] == NUM_HYP[model] // 3 and kinds["lone"][0]["n"] >= S
    assert 0 < kinds["few"][0]["best"] < S and not kinds["few"][0]["take"]
    assert kinds["ok_false"][0]["rc"] > kinds["ok_false"][0]["best"] and not kinds["ok_false"][0]["take"]
    assert kinds["nan_ok"][0]["rc"] == 0 and not kinds["nan_ok"][0]["take"] and kinds["nan_ok"][0]["n"] > 0


@pytest.mark.parametrize("model", MODELS)
def test_ransac_tail_with_a_single_hypothesis(model):
    """K = 1, the shape in which three of a workgroup's four waves idle: a good model, a void one and a poor one."""
    pairs = tail_pairs(model)
    good, void, poor = pairs[0], pairs[3], pairs[1]
    counts = [int(tv.inliers_f32(model, h, good["pts"]).sum()) for h in good["hyp"]]
    one = [dict(good, hyp=good["hyp"][[int(np.argmax(counts))]], seed=None, kind="good"), dict(void, hyp=void["hyp"][:1]),
           dict(poor, hyp=poor["hyp"][:1], seed=None, kind="poor")]
    kinds = check_tail(model, one)
    assert kinds["good"][0]["n"] >= max(counts) and kinds["void"][0]["n"] == 0


# ---- the hypothesis half of _estimate ------------------------------------------------------------------------------------------------
HYP_SCENES = [(61, 300, 0.3, False), (62, 200, 0.3, True), (63, 1000, 0.3, False), (64, 9, 0.0, False)]


@pytest.mark.parametrize("model", MODELS)
def test_hypotheses_reproduce_their_samples_like_the_oracles(model):
    from vit_colmap_amd.matching import _common
    from vit_colmap_amd.matching import two_view as g

    K, S = NUM_HYP[model], u.S_OF[model]
    rows = [u.scene_pts(*s) for s in HYP_SCENES]
    pids = [pair_id(i) for i in range(len(rows))]
    pts, offsets, pair_of, seeds = _common._pair_batch(rows, pids, "cuda")
    hyp32, idx, _ = g._hypotheses(model, pts, offsets, pair_of, seeds, K)
    hyp32, idx = hyp32.cpu().numpy(), idx.cpu().numpy()
    assert hyp32.shape == (len(rows), K, 9) and hyp32.dtype == np.float32 and idx.shape == (len(rows), K, S)
    eq = tv.rows_f if model == "F" else tv.rows_h
    res_g, res_o, excluded, void_diff = [], [], 0, []
    for p, r in enumerate(rows):
        seed = pids[p] & 0xFFFFFFFF
        ohyp, (_, _, n1, n2) = tv.hypotheses(model, r, seed, K)
        oidx = tv.sample_indices(seed, K, S, len(r), u.SALT_OF[model])
        assert np.array_equal(idx[p], oidx), p
        gvoid, ovoid = np.isnan(hyp32[p]).any(axis=1), np.isnan(ohyp).any(axis=1)
        assert np.array_equal(gvoid, np.isnan(hyp32[p]).all(axis=1)) and np.isfinite(hyp32[p][~gvoid]).all()
        for k in range(K):
            if oidx[k, 0] < 0:
                assert gvoid[k] and ovoid[k]
                continue
            s = oidx[k]
            A, _ = eq(n1[s, 0], n1[s, 1], n2[s, 0], n2[s, 1])
            if np.linalg.cond(A) > 1e12:                       # the oracle's own system is singular to float64: either may be void
                excluded += 1
                continue
            if gvoid[k] != ovoid[k]:
                void_diff.append((p, k))
            elif not gvoid[k]:
                res_g.append(u.residual64(model, hyp32[p, k], r[s]).max())
                res_o.append(u.residual64(model, ohyp[k], r[s]).max())
    res_g, res_o = np.array(res_g), np.array(res_o)
    p99 = np.percentile(res_o, 99)
    print(f"{model}: {len(res_g)} hypotheses compared, {excluded} excluded, oracle residual p99 {p99:.3g} px max {res_o.max():.3g} px, "
          f"device max {res_g.max():.3g} px, worst ratio {np.max(res_g / np.maximum(res_o, p99)):.3g}")
    assert excluded <= 0.05 * len(rows) * K and len(res_g) >= 0.8 * len(rows) * K
    assert not void_diff, void_diff
    # 99th percentile of the oracle's residual at its own sample points over this batch, measured on the CPU:
    # F 2.6e-4 px (2042 hypotheses, 6 void, largest 1.1e-3 px), H 0.055 px (512 hypotheses; the largest, 5.6e3 px, is a sample
    # with three nearly collinear points, which is why the oracle's residual at the same points is the other yardstick)
    worse = np.flatnonzero(res_g > 4 * np.maximum(res_o, p99))
    assert len(worse) == 0, (len(worse), res_g[worse][:5], res_o[worse][:5])


# ---- verify_pairs as a whole ---------------------------------------------------------------------------------------------------
def whole_batch():
    """-> (keypoints, pair_images, pair_ids, match_lists, expected oracle config or None): synthetic scenes, a 14-match and an
    empty pair between them, the integer-grid pair identical and shifted, a pair with 20 repeated keypoints, a collapsed one."""
    scenes = [((40, 300, 0.2, True), tv.CONFIG_PLANAR_OR_PANORAMIC), "short", ((44, 300, 0.3, False), tv.CONFIG_UNCALIBRATED),
              ((51, 1000, 0.3, False), tv.CONFIG_UNCALIBRATED), "empty", ((49, 500, 0.85, False), tv.CONFIG_DEGENERATE),
              ((46, 16, 0.0, False), None), ((47, 15, 0.0, True), None), "grid0", "grid14", "repeated", "collapsed",
              ((64, 200, 0.4, True), tv.CONFIG_PLANAR_OR_PANORAMIC)]
    kps, pairs, pids, lists, expect = {}, [], [], [], []
    for i, sc in enumerate(scenes):
        want = None
        if sc == "short":
            kp1, kp2, m, _ = tv.synthetic_two_view(45, 30, 0.0, False)
            m, want = m[:14], tv.CONFIG_DEGENERATE
        elif sc == "empty":
            kp1, kp2, m, _ = tv.synthetic_two_view(45, 30, 0.0, False)
            m, want = m[:0], tv.CONFIG_DEGENERATE
        elif sc in ("grid0", "grid14"):
            kp1, kp2, m = u.grid_pair(0.0 if sc == "grid0" else 14.0)
            want = tv.CONFIG_PLANAR_OR_PANORAMIC
        elif sc == "repeated":                                  # keypoints that share coordinates, as SIFT orientations do
            kp1, kp2, m, _ = tv.synthetic_two_view(52, 120, 0.2, False)
            kp1[20:40], kp2[20:40] = kp1[:20], kp2[:20]
        elif sc == "collapsed":                                 # every match on one point
            kp1 = np.tile(np.array([[100.0, 50.0]], np.float32), (40, 1))
            kp2, m, want = kp1 + np.float32(3.0), np.stack([np.arange(40)] * 2, axis=1).astype(np.uint32), tv.CONFIG_DEGENERATE
        else:
            kp1, kp2, m, _ = tv.synthetic_two_view(*sc[0])
            want = sc[1]
        kps[2 * i], kps[2 * i + 1] = kp1, kp2
        pairs.append((2 * i, 2 * i + 1)), pids.append(pair_id(i)), lists.append(m), expect.append(want)
    return kps, pairs, pids, lists, expect


@lru_cache(maxsize=None)
def whole_oracle():
    kps, pairs, pids, lists, _ = whole_batch()
    return [tv.verify_pair(kps[a], kps[b], m, pid) for (a, b), pid, m in zip(pairs, pids, lists)]


@lru_cache(maxsize=None)
def whole_device(chunk_pairs=None):
    from vit_colmap_amd.matching.two_view import verify_pairs

    kps, pairs, pids, lists, _ = whole_batch()
    return verify_pairs(kps, pairs, pids, lists, **({} if chunk_pairs is None else dict(chunk_pairs=chunk_pairs)))


def close_to(r, o, what):
    """The tolerances of test_verify_pairs_against_oracle_on_synthetic_scenes: identical sampler and arithmetic; the 8x8 solves
    differ in the last bits between solvers (and the refit's sums between launches), which may move a borderline match."""
    assert r["config"] == o["config"], (what, r["config"], o["config"], r["n_f"], o["n_f"], r["n_h"], o["n_h"])
    assert abs(r["n_f"] - o["n_f"]) <= max(2, 0.02 * o["n_f"]) and abs(r["n_h"] - o["n_h"]) <= max(2, 0.02 * o["n_h"]), \
        (what, r["n_f"], o["n_f"], r["n_h"], o["n_h"])
    got, ref = set(map(tuple, r["inlier_matches"])), set(map(tuple, o["inlier_matches"]))
    assert len(got ^ ref) <= max(2, 0.03 * len(ref)), (what, len(got ^ ref), len(ref))


def consistent(r, kp1, kp2, m, what):
    """What a result says about itself, exactly."""
    default = dict(config=tv.CONFIG_DEGENERATE, inlier_matches=np.zeros((0, 2), np.uint32), F=np.zeros((3, 3)), H=np.zeros((3, 3)))
    if r["config"] == tv.CONFIG_DEGENERATE:
        assert all(np.array_equal(r[k], v) for k, v in default.items()) and "model" not in r and "model9" not in r, what
        return
    m = np.asarray(m, np.uint32).reshape(-1, 2)
    pts = np.concatenate([kp1[m[:, 0], :2], kp2[m[:, 1], :2]], axis=1).astype(np.float32)
    assert r["model"] in ("F", "H") and r["model9"].dtype == np.float32 and r["model9"].shape == (9,), what
    assert r["inlier_matches"].dtype == np.uint32
    assert np.array_equal(r["inlier_matches"], m[tv.inliers_f32(r["model"], r["model9"], pts)]), what
    assert len(r["inlier_matches"]) == (r["n_h"] if r["model"] == "H" else r["n_f"]), what
    assert (r["model"] == "H") == (r["n_h"] > r["n_f"]), what
    sv = np.linalg.svd(r["F"], compute_uv=False)
    assert sv[2] <= 1e-9 * sv[0] and abs(np.linalg.norm(r["F"]) - 1) < 1e-9, (what, sv)
    if r["model"] == "F":
        want = tv.stored_f(r["model9"])
        assert min(np.abs(r["F"] - want).max(), np.abs(r["F"] + want).max()) < 1e-9, what
    assert r["H"][2, 2] == 1, what


def test_verify_pairs_whole_batch_against_the_oracle():
    kps, pairs, pids, lists, expect = whole_batch()
    oracle, res = whole_oracle(), whole_device()
    assert len(res) == len(pairs)
    for i, (r, o) in enumerate(zip(res, oracle)):
        print(i, "device", r["config"], r["n_f"], r["n_h"], r.get("model"), "oracle", o["config"], o["n_f"], o["n_h"])
    for i, (r, o) in enumerate(zip(res, oracle)):
        assert expect[i] is None or o["config"] == expect[i], (i, o["config"], o["n_f"], o["n_h"])      # the oracle alone
        close_to(r, o, i)
        consistent(r, kps[2 * i], kps[2 * i + 1], lists[i], i)
    assert [len(m) for m in lists][1:5:3] == [14, 0] and res[1]["n_f"] == res[4]["n_f"] == 0
    for i in (8, 9):                                            # the integer grid: every match fits, no garbage hypothesis wins
        assert (oracle[i]["n_f"], oracle[i]["n_h"]) == (300, 300) and len(res[i]["inlier_matches"]) == 300
    assert oracle[5]["n_f"] < 125 and oracle[11]["n_f"] == 0     # degenerate by the floor; collapsed


def test_verify_pairs_takes_the_h_mask_where_h_has_more_inliers():
    """num_f = 2 starves the F estimate of a planar scene, so n_h > n_f and `inlier_matches` are H's (a call of its own:
    num_f is per call)."""
    from vit_colmap_amd.matching.two_view import verify_pairs

    kp1, kp2, m, _ = tv.synthetic_two_view(64, 200, 0.4, True)
    pid = 2147483649
    o = tv.verify_pair(kp1, kp2, m, pid, num_f=2, num_h=128)
    assert (o["config"], o["n_f"], o["n_h"]) == (tv.CONFIG_PLANAR_OR_PANORAMIC, 98, 135)
    short = np.zeros((3, 2), np.uint32)
    res = verify_pairs({0: kp1, 1: kp2}, [(0, 1), (0, 1), (0, 1)], [7, pid, 9], [short, m, short], num_f=2, num_h=128)
    r = res[1]
    close_to(r, o, "H")
    assert r["model"] == "H" and r["n_h"] > r["n_f"]
    consistent(r, kp1, kp2, m, "H")
    assert np.abs(r["H"] - o["H"]).max() <= 1e-3 * np.abs(o["H"]).max()
    for q in (0, 2):
        consistent(res[q], kp1, kp2, short, q)
        assert res[q]["n_f"] == res[q]["n_h"] == 0


def same_decision(a, b, what):
    """Two runs of the device code on the same pair: the decision is the same; counts within the tolerance of close_to (the
    refit's normal equations are summed with atomics, so two launches may differ in the last bits)."""
    assert a["config"] == b["config"] and a.get("model") == b.get("model"), what
    close_to(a, b, what)


def test_verify_pairs_returns_results_in_input_order():
    from vit_colmap_amd.matching.two_view import verify_pairs

    kps, pairs, pids, lists, _ = whole_batch()
    res = whole_device()
    perm = np.random.RandomState(31).permutation(len(pairs))
    assert not np.array_equal(perm, np.arange(len(pairs)))
    got = verify_pairs(kps, [pairs[i] for i in perm], [pids[i] for i in perm], [lists[i] for i in perm])
    for q, i in enumerate(perm):
        same_decision(got[q], res[i], (q, i))
        consistent(got[q], kps[2 * i], kps[2 * i + 1], lists[i], (q, i))


@pytest.mark.parametrize("chunk_pairs", [1, 5])
def test_verify_pairs_does_not_depend_on_the_chunk_size(chunk_pairs):
    kps, pairs, pids, lists, _ = whole_batch()
    res, got = whole_device(), whole_device(chunk_pairs)
    exact = bits = 0
    for i, (a, b) in enumerate(zip(got, res)):
        same_decision(a, b, i)
        consistent(a, kps[2 * i], kps[2 * i + 1], lists[i], i)
        exact += a["n_f"] == b["n_f"] and a["n_h"] == b["n_h"] and np.array_equal(a["inlier_matches"], b["inlier_matches"])
        bits += all(np.array_equal(a[k], b[k]) for k in ("F", "H")) and np.array_equal(a.get("model9"), b.get("model9"))
    # measured: counts and inlier matches identical on all 13 pairs; the assertion stays at same_decision because the refit's
    # normal equations are summed with atomics, whose order, and with it the last bits of the model, varies between launches
    print(f"chunk_pairs={chunk_pairs}: {exact} of {len(res)} pairs have identical counts and inlier matches, {bits} identical matrices")
