"""GPU tests of the calibrated branch: vc_essential_5pt against the numpy specification of
tests/util_essential.py on the 300 exact minimal problems, its shapes, degenerate inputs and argument checks, then
verify_pairs with cameras against the specification's rule and match_exhaustive end to end."""
from functools import lru_cache, partial

import numpy as np
import pytest
import torch

from oracle import two_view_oracle as tv
import util_essential as ue
import util_solver
from test_essential_spec import NONPLANAR, PAIR_ID, PLANAR, make_calibrated_db, scene_result

pytestmark = pytest.mark.gpu

TOL = 1e-6            # about 16 float32 ulp of the scored F_px: a smaller difference cannot change a score
MAX_MISMATCHES = 3    # problems (of 300) in which a solution may be unmatched, either way: near-double roots
# |n_e(GPU) - n_e(spec)| allowed per scene: the largest |difference| the specification itself shows on the CPU when every
# solver solution is moved by TOL in a random direction before scoring (0 on all eight scenes, four directions each), plus 1
N_E_MARGIN = 0 + 1


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_kernel(pts_n, offsets, samples):
    """numpy float64 (total, 4), int (P + 1), int (P, n_hyp, 5) -> E (P, n_hyp, 10, 3, 3), count (P, n_hyp); the outputs are
    pre-filled, so a slot the kernel never wrote cannot pass for a result."""
    from vit_colmap_amd import _lib

    lib = _lib.load()
    P, n_hyp = samples.shape[:2]
    d_pts, d_off, d_s = dev(np.asarray(pts_n, np.float64).reshape(-1, 4)), dev(np.asarray(offsets, np.int32)), dev(np.asarray(samples, np.int32))
    E = torch.full((P, n_hyp, 10, 9), 7.0, dtype=torch.float64, device="cuda")
    count = torch.full((P, n_hyp), -7, dtype=torch.int32, device="cuda")
    _lib.check(lib.vc_essential_5pt(_lib.ptr(d_pts), _lib.ptr(d_off), P, _lib.ptr(d_s), n_hyp, _lib.ptr(E), _lib.ptr(count),
                                    _lib.stream_ptr()), "vc_essential_5pt")
    torch.cuda.synchronize()
    E, count = E.cpu().numpy().reshape(P, n_hyp, 10, 3, 3), count.cpu().numpy()
    assert np.all((count >= 0) & (count <= 10))
    used = np.arange(10)[None, None, :] < count[:, :, None]
    assert np.isnan(E[~used]).all(), "a slot past the count is not NaN"
    assert np.isfinite(E[used]).all(), "a counted solution is not finite"
    assert np.allclose(np.linalg.norm(E[used].reshape(-1, 9), axis=1), 1.0, atol=1e-12)
    return E, count


@lru_cache(maxsize=None)
def minimal_problems():
    """The 300 problems as one point list (1500, 4) and the specification's solutions of each."""
    pts, sols = [], []
    for i in range(300):
        x1, x2 = ue.minimal_problem(i)
        pts.append(np.concatenate([x1, x2], axis=1))
        sols.append(ue.five_point(x1, x2))
    return np.concatenate(pts), sols


compare_with_spec = partial(util_solver.compare_with_spec, distance=ue.matrix_distance, tol=TOL)


def test_kernel_matches_the_spec_on_the_300_minimal_problems_one_hypothesis_per_pair():
    pts, sols = minimal_problems()
    E, count = run_kernel(pts, np.arange(301) * 5, np.tile(np.arange(5), (300, 1, 1)))
    bad, worst = compare_with_spec([E[i, 0, : count[i, 0]] for i in range(300)], sols)
    Et = ue.true_essential()
    truth = max(min(ue.matrix_distance(Et, e) for e in E[i, 0, : count[i, 0]]) for i in range(300) if i not in bad)
    print(f"unmatched problems {bad}, worst matched distance {worst:.3g}, worst distance to the true E {truth:.3g}, "
          f"solutions per problem {sorted(set(count[:, 0]))}")
    assert len(bad) <= MAX_MISMATCHES
    assert truth <= TOL


def test_kernel_matches_the_spec_with_ragged_pairs():
    """Pairs of 5, 495 and 1000 points over the same 1500 points, 100 hypotheses each: pair 0 samples its five points in 100
    orders (one problem, whose solution set does not depend on the order), pair 1 problems 1..99 and one void hypothesis, pair 2
    every second problem from 100 on, so that `offsets` and the sample indices both matter."""
    pts, sols = minimal_problems()
    rs = np.random.RandomState(7)
    samples = np.full((3, 100, 5), -1, np.int64)
    problem = np.full((3, 100), -1)
    samples[0, 0], problem[0] = np.arange(5), 0
    for k in range(1, 100):
        samples[0, k] = rs.permutation(5)
    for k in range(99):
        samples[1, k], problem[1, k] = 5 * k + np.arange(5), 1 + k
    for k in range(100):
        samples[2, k], problem[2, k] = 10 * k + np.arange(5), 100 + 2 * k
    E, count = run_kernel(pts, [0, 5, 500, 1500], samples)
    assert count[1, 99] == 0
    got, want = [], []
    for p in range(3):
        for k in range(100):
            if problem[p, k] >= 0:
                got.append(E[p, k, : count[p, k]])
                want.append(sols[problem[p, k]])
    bad, worst = compare_with_spec(got, want)
    print(f"unmatched hypotheses {bad}, worst matched distance {worst:.3g}")
    assert len(bad) <= MAX_MISMATCHES


def exact_pair(n_problems=8, first=40):
    return np.concatenate([np.concatenate(ue.minimal_problem(first + i), axis=1) for i in range(n_problems)])


@pytest.mark.parametrize("n_hyp", [1, 5, 64, 65, 130])
def test_every_hypothesis_of_one_pair_holds_the_true_matrix(n_hyp):
    pts = exact_pair()                                                # 40 exact correspondences of one motion
    samples = tv.sample_indices(1234 + n_hyp, n_hyp, 5, len(pts), ue.SALT_E)
    assert (samples >= 0).all()
    E, count = run_kernel(pts, [0, len(pts)], samples[None])
    Et = ue.true_essential()
    dist = [min([ue.matrix_distance(Et, e) for e in E[0, k, : count[0, k]]] + [9.0]) for k in range(n_hyp)]
    assert max(dist) <= TOL, f"hypotheses without the true E: {[k for k, d in enumerate(dist) if d > TOL]}"
    # ascending in the root variable means a fixed order: a second launch returns the same bits
    E2, count2 = run_kernel(pts, [0, len(pts)], samples[None])
    assert np.array_equal(count, count2) and np.array_equal(E, E2, equal_nan=True)


def test_void_out_of_range_repeated_and_degenerate_samples_return_and_count_nothing_infinite():
    exact = exact_pair()
    line = np.stack([np.linspace(-0.3, 0.3, 5), np.linspace(-0.2, 0.1, 5), np.linspace(-0.1, 0.3, 5), np.linspace(0.2, 0.1, 5)], axis=1)
    same = np.repeat(exact[:1], 5, axis=0)
    twice = exact[[0, 1, 2, 3, 3]]                                      # two different indices, one point
    pts = np.concatenate([exact[:3], exact, line, same, twice])
    offsets = np.cumsum([0, 3, len(exact), 5, 5, 5])
    n_hyp = 6
    samples = np.full((5, n_hyp, 5), -1, np.int64)                     # pair 0 (fewer than five points): every sample void
    samples[1, 0] = [0, 7, 14, 21, 28]                                 # valid
    samples[1, 1] = [0, 7, 14, 21, 7]                                  # repeats an index
    samples[1, 2] = [0, 7, 14, 21, len(exact)]                         # past the pair's list
    samples[1, 3] = [-1, 7, 14, 21, 28]                                # void
    samples[1, 4] = [5, 7, 14, -1, 28]                                 # -1 further back
    samples[2, :2] = samples[3, :2] = samples[4, :2] = np.arange(5)
    E, count = run_kernel(pts, offsets, samples)                       # run_kernel checks NaN slots and finite solutions
    assert (count[0] == 0).all()
    assert count[1, 0] >= 1 and min(ue.matrix_distance(ue.true_essential(), e) for e in E[1, 0, : count[1, 0]]) <= TOL
    assert (count[1, 1:] == 0).all()
    assert (count[3] == 0).all() and (count[4] == 0).all()             # identical points, a repeated point
    assert (count[2, 2:] == 0).all()                                   # collinear: any count, finite solutions only
    bad = np.full((1, 4), np.nan)
    for fill in (np.nan, np.inf, 1e200, 0.0):
        p5 = np.concatenate([exact[:4], np.full_like(bad, fill)])
        _, c = run_kernel(p5, [0, 5], np.arange(5)[None, None])
        assert c[0, 0] == 0 or fill == 1e200 or fill == 0.0


def test_argument_checks_on_device_pointers():
    from vit_colmap_amd import _lib

    lib = _lib.load()
    pts, off, s = dev(exact_pair()), dev(np.array([0, 40], np.int32)), dev(np.arange(5, dtype=np.int32).reshape(1, 1, 5))
    E = torch.zeros((1, 1, 10, 9), dtype=torch.float64, device="cuda")
    c = torch.zeros((1, 1), dtype=torch.int32, device="cuda")
    good = [_lib.ptr(pts), _lib.ptr(off), 1, _lib.ptr(s), 1, _lib.ptr(E), _lib.ptr(c), _lib.stream_ptr()]
    assert lib.vc_essential_5pt(*good) == 0
    for pos in (0, 1, 3, 5, 6):
        args = list(good)
        args[pos] = None
        assert lib.vc_essential_5pt(*args) == -1, pos
    for pos in (2, 4):
        args = list(good)
        args[pos] = -1
        assert lib.vc_essential_5pt(*args) == -1, pos
        args[pos] = 0
        assert lib.vc_essential_5pt(*args) == 0, pos
    torch.cuda.synchronize()
    assert int(c[0, 0]) >= 1


# ---- verify_pairs with cameras ------------------------------------------------------------------------------------------------
def test_verify_pairs_with_cameras_follows_the_spec_and_leaves_unflagged_pairs_alone():
    """The eight CPU scenes in one batch with two unflagged pairs (scenes 1 and planar 1 again).  n_e within N_E_MARGIN = 1 of
    the specification's (see the constant), poses within twice the specification's worst error over the scenes of the same
    kind.  The unflagged pairs equal a run without cameras in everything discrete; their float64 matrices are compared to
    rounding, because the refit's normal equations are accumulated with atomics whose order is not fixed between launches."""
    from vit_colmap_amd.matching.two_view import verify_pairs

    scenes = [(s, f, False) for s, f in NONPLANAR] + [(s, 0.3, True) for s in PLANAR]
    kps, pair_images, pids, lists = {}, [], [], []
    for q, (seed, frac, planar) in enumerate(scenes + [scenes[0], scenes[5]]):
        kp1, kp2, m, _ = tv.synthetic_two_view(seed, outlier_frac=frac, planar=planar)
        kps[2 * q], kps[2 * q + 1] = kp1, kp2
        pair_images.append((2 * q, 2 * q + 1))
        pids.append(PAIR_ID + seed)
        lists.append(m)
    K = np.tile(ue.SCENE_K, (20, 1, 1))
    prior = np.array([1] * 16 + [0] * 4, np.uint8)
    res = verify_pairs(kps, pair_images, pids, lists, cameras=(K, prior))
    plain = verify_pairs(kps, pair_images, pids, lists)
    spec = [scene_result(*sc)[0] for sc in scenes]
    worst = {False: np.zeros(2), True: np.zeros(2)}
    for sc, s in zip(scenes, spec):
        worst[sc[2]] = np.maximum(worst[sc[2]], ue.pose_errors(s["qvec"], s["tvec"]))
    for q, (sc, r, s) in enumerate(zip(scenes, res, spec)):
        rot, trans = ue.pose_errors(r["qvec"], r["tvec"])
        print(f"scene {sc}: config {r['config']} (spec {s['config']}) n_e {r['n_e']} (spec {s['n_e']}) n_f {r['n_f']} n_h {r['n_h']} "
              f"rotation {rot:.2f} translation {trans:.2f} deg (spec worst {worst[sc[2]]})")
    for q, (sc, r, s) in enumerate(zip(scenes, res, spec)):
        assert r["config"] == s["config"], sc
        assert abs(r["n_e"] - s["n_e"]) <= N_E_MARGIN, sc
        rot, trans = ue.pose_errors(r["qvec"], r["tvec"])
        assert rot <= 2 * worst[sc[2]][0] and trans <= 2 * worst[sc[2]][1], sc
        sv = np.linalg.svd(r["E"], compute_uv=False)
        assert np.allclose(sv, np.array([1, 1, 0]) / np.sqrt(2), atol=1e-9)
        assert abs(np.linalg.norm(r["qvec"]) - 1) < 1e-12 and abs(np.linalg.norm(r["tvec"]) - 1) < 1e-12
        assert r["model9"].dtype == np.float32 and r["model"] == s["model"]
        mask_model = tv.inliers_f32(r["model"], r["model9"], np.concatenate([kps[2 * q][lists[q][:, 0]], kps[2 * q + 1][lists[q][:, 1]]], axis=1))
        assert np.array_equal(lists[q][mask_model], r["inlier_matches"])       # the mask is model9's: guided matching works unchanged
    for q in (8, 9):
        r, p = res[q], plain[q]
        assert r.keys() == p.keys() and "E" not in r and "n_e" not in r
        for k in ("config", "n_f", "n_h", "inlier_matches", "model"):
            assert np.array_equal(r[k], p[k]), (q, k)
        for k in ("F", "H", "model9"):
            assert np.allclose(r[k], p[k], rtol=1e-6, atol=1e-9), (q, k)


# ---- end to end -----------------------------------------------------------------------------------------------------------------
def _rows(path):
    from vit_colmap_amd.database import ColmapDatabase

    with ColmapDatabase.open_database(str(path)) as h:
        return {(i, j): h.read_two_view_geometry(i, j) for i, j in ((1, 2), (1, 3), (2, 3))}


def test_match_exhaustive_writes_calibrated_rows_and_guided_lists_contain_the_inliers(tmp_path):
    from vit_colmap_amd.matching import match_exhaustive
    from vit_colmap_amd.utils.config import MatchingConfig

    for name in ("plain.db", "guided.db"):
        make_calibrated_db(tmp_path / name)
    s0 = match_exhaustive(database_path=str(tmp_path / "plain.db"))
    s1 = match_exhaustive(database_path=str(tmp_path / "guided.db"),
                          matching_options=MatchingConfig(guided_matching=True).to_matching_options())
    assert s0["verified_pairs"] == s1["verified_pairs"] == s1["guided_pairs"] == 3
    plain, guided = _rows(tmp_path / "plain.db"), _rows(tmp_path / "guided.db")
    for pair in ((1, 2), (1, 3)):                                      # (2, 3) is one view twice: no baseline, E is not defined
        g = plain[pair]
        assert g["config"] == tv.CONFIG_CALIBRATED and g["E"].any() and len(g["inlier_matches"]) > 100
        assert abs(np.linalg.norm(g["E"]) - 1) < 1e-12 and max(ue.pose_errors(g["qvec"], g["tvec"])) < 5
    for pair in plain:
        assert guided[pair]["config"] == plain[pair]["config"]
        assert set(map(tuple, plain[pair]["inlier_matches"])) <= set(map(tuple, guided[pair]["inlier_matches"])), pair


def test_match_exhaustive_with_the_flags_cleared_writes_todays_rows(tmp_path):
    from vit_colmap_amd.matching import match_exhaustive
    from vit_colmap_amd.matching.two_view import verify_pairs

    make_calibrated_db(tmp_path / "cleared.db", flag=False)
    seen = {}

    def todays_verify(kps, pair_images, pair_ids, lists):            # four positional arguments: `cameras=` would be a TypeError
        res = verify_pairs(kps, pair_images, pair_ids, lists)
        seen.update({(a + 1, b + 1): r for (a, b), r in zip(pair_images, res)})
        return res

    match_exhaustive(database_path=str(tmp_path / "cleared.db"), verify_fn=todays_verify)
    rows = _rows(tmp_path / "cleared.db")
    assert len(seen) == 3
    for pair, g in rows.items():
        r = seen[pair]
        assert g["config"] == r["config"] != tv.CONFIG_CALIBRATED
        assert np.array_equal(g["inlier_matches"], r["inlier_matches"])
        assert np.array_equal(g["F"], r["F"]) and np.array_equal(g["H"], r["H"])
        assert not g["E"].any() and np.array_equal(g["qvec"], [1, 0, 0, 0]) and not g["tvec"].any()
