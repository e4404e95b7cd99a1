"""GPU tests of image registration: vc_p3p against the numpy specification of tests/util_absolute_pose.py
on the 300 exact minimal problems, its shapes, degenerate inputs and argument checks; the scoring kernels bit for bit;
the RANSAC tail under this residual with a refit the test owns (exact); estimate_absolute_poses against the specification's
rule; match_exhaustive + build_seed_model end to end."""
from functools import lru_cache, partial

import numpy as np
import pytest
import torch

from oracle import two_view_oracle as tv
import util_absolute_pose as ua
import util_essential as ue
import util_solver
from test_absolute_pose_spec import read_pairs, scene_images, write_scene_db

pytestmark = pytest.mark.gpu

# A kernel solution and the specification's match may differ by 4x the larger of (measured on the CPU, see the constants in
# util_absolute_pose.py): 6.98e-12, the worst matched distance between the specification and the kernel's solver functions
# compiled for the host (tools/p3p_host.cpp) over the 300 problems, and 2.9e-12, the specification's own worst distance to
# the true pose.  The margin covers libm and instruction selection on the device; the algebra is the same.
TOL_POSE = ua.TOL_POSE            # 2.8e-11
MAX_MISMATCHES = 3                # problems (of 300) in which a solution may be unmatched, either way: near-double roots
# Samples drawn from the 40-point problem are not the 300 problems: their conditioning is whatever the sampler hits.  On those
# 265 samples the specification's own worst distance to the true pose is 5.2e-11 (the host build of the kernel's: 1.8e-11,
# both measured on the CPU); the same 4x margin over the reference's own error
TOL_TRUTH_SAMPLED = 4 * 5.2e-11
# |num_inliers(GPU) - num_inliers(spec)| allowed per problem: the largest |difference| the specification itself shows on the
# CPU when every solver solution is moved by TOL_POSE in a random direction before scoring (0 on all eight problems, four
# directions each), plus 1
N_P_MARGIN = 0 + 1


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_p3p(rays, xyz, offsets, samples):
    """numpy float64 (total, 2), (total, 3), int (P + 1), int (P, n_hyp, 3) -> list of (R, t) per (problem, hypothesis), the raw
    pose array and the counts; the outputs are pre-filled, so a slot the kernel never wrote cannot pass for a result."""
    from vit_colmap_amd import _lib

    lib = _lib.load()
    P, n_hyp = samples.shape[:2]
    d_r, d_x = dev(np.asarray(rays, np.float64).reshape(-1, 2)), dev(np.asarray(xyz, np.float64).reshape(-1, 3))
    d_off, d_s = dev(np.asarray(offsets, np.int32)), dev(np.asarray(samples, np.int32))
    pose = torch.full((P, n_hyp, 4, 12), 7.0, dtype=torch.float64, device="cuda")
    count = torch.full((P, n_hyp), -7, dtype=torch.int32, device="cuda")
    _lib.check(lib.vc_p3p(_lib.ptr(d_r), _lib.ptr(d_x), _lib.ptr(d_off), P, _lib.ptr(d_s), n_hyp, _lib.ptr(pose), _lib.ptr(count),
                          _lib.stream_ptr()), "vc_p3p")
    torch.cuda.synchronize()
    pose, count = pose.cpu().numpy(), count.cpu().numpy()
    assert np.all((count >= 0) & (count <= 4))
    used = np.arange(4)[None, None, :] < count[:, :, None]
    assert np.isnan(pose[~used]).all(), "a slot past the count is not NaN"
    assert np.isfinite(pose[used]).all(), "a counted pose is not finite"
    assert (np.abs(np.linalg.det(pose[used][:, :9].reshape(-1, 3, 3)) - 1) < 1e-9).all(), "a counted rotation is not proper"
    sets = [[[(pose[p, k, j, :9].reshape(3, 3), pose[p, k, j, 9:]) for j in range(count[p, k])] for k in range(n_hyp)] for p in range(P)]
    return sets, pose, count


@lru_cache(maxsize=None)
def minimal_problems():
    """The 300 problems as one list of 900 correspondences and the specification's solutions of each."""
    rays, xyz, sols = [], [], []
    for i in range(300):
        x, X = ua.minimal_problem(i)
        rays.append(x), xyz.append(X), sols.append(ua.p3p(x, X))
    return np.concatenate(rays), np.concatenate(xyz), sols


compare_with_spec = partial(util_solver.compare_with_spec, distance=lambda a, b: ua.pose_distance(*a, *b), tol=TOL_POSE)


def truth_distance(sols):
    return min([ua.pose_distance(R, t, ue.SCENE_R, ue.SCENE_T) for R, t in sols] + [9.0])


def test_kernel_matches_the_spec_on_the_300_minimal_problems_one_hypothesis_per_problem():
    rays, xyz, sols = minimal_problems()
    sets, _, count = run_p3p(rays, xyz, np.arange(301) * 3, np.tile(np.arange(3), (300, 1, 1)))
    got = [sets[i][0] for i in range(300)]
    bad, worst = compare_with_spec(got, sols)
    spec_bad = [i for i in range(300) if truth_distance(sols[i]) > TOL_POSE]
    truth = max(truth_distance(got[i]) for i in range(300) if i not in bad)
    print(f"unmatched problems {bad}, worst matched distance {worst:.3g}, worst distance to the true pose {truth:.3g}, "
          f"solutions per problem {sorted(set(count[:, 0]))}")
    assert len(spec_bad) <= MAX_MISMATCHES                            # the specification alone stays within the cap
    assert len(bad) <= MAX_MISMATCHES
    assert truth <= TOL_POSE


def test_kernel_matches_the_spec_with_ragged_problems():
    """Problems of 3, 297 and 600 correspondences over the same 900 rows, 100 hypotheses each: problem 0 samples its three
    points in 100 orders (one minimal problem, whose solution set does not depend on the order), problem 1 the minimal
    problems 1..99 and one void hypothesis, problem 2 every second minimal problem from 100 on, so that `offsets` and the
    sample indices both matter."""
    rays, xyz, sols = minimal_problems()
    rs = np.random.RandomState(7)
    samples = np.full((3, 100, 3), -1, np.int64)
    problem = np.full((3, 100), -1)
    samples[0, 0], problem[0] = np.arange(3), 0
    for k in range(1, 100):
        samples[0, k] = rs.permutation(3)
    for k in range(99):
        samples[1, k], problem[1, k] = 3 * k + np.arange(3), 1 + k
    for k in range(100):
        samples[2, k], problem[2, k] = 6 * k + np.arange(3), 100 + 2 * k
    sets, _, count = run_p3p(rays, xyz, [0, 3, 300, 900], samples)
    assert count[1, 99] == 0
    got, want = [], []
    for p in range(3):
        for k in range(100):
            if problem[p, k] >= 0:
                got.append(sets[p][k])
                want.append(sols[problem[p, k]])
    bad, worst = compare_with_spec(got, want)
    print(f"unmatched hypotheses {bad}, worst matched distance {worst:.3g}")
    # problem 0 is one minimal problem asked 100 times: it counts once
    assert len({int(problem.reshape(-1)[problem.reshape(-1) >= 0][i]) for i in bad}) <= MAX_MISMATCHES


@pytest.mark.parametrize("n_hyp", [1, 5, 64, 65, 130])
def test_every_hypothesis_of_one_problem_holds_the_true_pose(n_hyp):
    x, X = ua.exact_problem(40)                                        # 40 exact correspondences of one pose
    samples = tv.sample_indices(1234 + n_hyp, n_hyp, 3, 40, ua.SALT_P)
    assert (samples >= 0).all()
    sets, pose, count = run_p3p(x, X, [0, 40], samples[None])
    dist = [truth_distance(sets[0][k]) for k in range(n_hyp)]
    print(f"worst distance to the true pose {max(dist):.3g}")
    assert max(dist) <= TOL_TRUTH_SAMPLED, f"hypotheses without the true pose: {[k for k, d in enumerate(dist) if d > TOL_TRUTH_SAMPLED]}"
    # ascending in the root variable means a fixed order: a second launch returns the same bits
    _, pose2, count2 = run_p3p(x, X, [0, 40], samples[None])
    assert np.array_equal(count, count2) and np.array_equal(pose, pose2, equal_nan=True)
    # ascending in u = s2 / s1, the ratio of the depths along the unit rays of the sample's second and first point
    for k in range(n_hyp):
        i, j = samples[k, 0], samples[k, 1]
        u = [((X[j] @ R[2] + t[2]) * np.linalg.norm([*x[j], 1])) / ((X[i] @ R[2] + t[2]) * np.linalg.norm([*x[i], 1])) for R, t in sets[0][k]]
        assert u == sorted(u), k


def test_void_out_of_range_repeated_and_degenerate_samples_count_nothing():
    x, X = ua.exact_problem(40)
    x0, X0 = ua.minimal_problem(0)
    coincident_world = (x0, X0[[0, 0, 2]])
    coincident_rays = (x0[[0, 0, 2]], X0)
    collinear = (x0, np.stack([X0[0], 0.5 * (X0[0] + X0[1]), X0[1]]))
    groups = [(x[:2], X[:2]), (x, X), coincident_world, coincident_rays, collinear]
    rays, xyz = np.concatenate([g[0] for g in groups]), np.concatenate([g[1] for g in groups])
    offsets = np.cumsum([0] + [len(g[0]) for g in groups])
    n_hyp = 6
    samples = np.full((5, n_hyp, 3), -1, np.int64)                     # problem 0 (fewer than three points): every sample void
    samples[1, 0] = [0, 7, 14]                                         # valid
    samples[1, 1] = [0, 7, 7]                                          # repeats an index
    samples[1, 2] = [0, 7, 40]                                         # past the problem's list
    samples[1, 3] = [-1, 7, 14]                                        # void
    samples[1, 4] = [5, -1, 14]                                        # -1 further back
    samples[2, :2] = samples[3, :2] = samples[4, :2] = np.arange(3)
    sets, _, count = run_p3p(rays, xyz, offsets, samples)              # run_p3p checks NaN slots, finite and proper poses
    assert (count[0] == 0).all()
    assert count[1, 0] >= 1 and truth_distance(sets[1][0]) <= TOL_TRUTH_SAMPLED
    assert (count[1, 1:] == 0).all()
    assert (count[2] == 0).all() and (count[3] == 0).all() and (count[4] == 0).all()
    for fill in (np.nan, np.inf, -np.inf):
        for where in ("ray", "point"):
            xb, Xb = x0.copy(), X0.copy()
            if where == "ray":
                xb[1, 1] = fill
            else:
                Xb[2, 0] = fill
            _, _, c = run_p3p(xb, Xb, [0, 3], np.arange(3)[None, None])
            assert c[0, 0] == 0, (fill, where)
    _, _, c = run_p3p(x0, X0 * 1e200, [0, 3], np.arange(3)[None, None])    # squared distances overflow: nothing, or finite poses
    assert c[0, 0] == 0


# ---- scoring ----------------------------------------------------------------------------------------------------------------------------
def run_score(obs, xyz, offsets, hyp, max_error):
    from vit_colmap_amd import _lib

    lib = _lib.load()
    P, K = hyp.shape[:2]
    d_obs, d_off, d_h = dev(np.asarray(obs, np.float32)), dev(np.asarray(offsets, np.int32)), dev(np.asarray(hyp, np.float32))
    d_xyz = dev(np.concatenate([np.asarray(xyz, np.float32), np.full((len(xyz), 1), np.nan, np.float32)], axis=1))     # w is ignored
    counts = torch.full((P, K), -7, dtype=torch.int32, device="cuda")
    _lib.check(lib.vc_absolute_pose_score(_lib.ptr(d_obs), _lib.ptr(d_xyz), _lib.ptr(d_off), P, _lib.ptr(d_h), K, float(max_error),
                                          _lib.ptr(counts), _lib.stream_ptr()), "vc_absolute_pose_score")
    masks = []
    for k in range(K):
        mask = torch.full((len(obs),), 9, dtype=torch.uint8, device="cuda")
        models = d_h[:, k].contiguous()
        _lib.check(lib.vc_absolute_pose_inliers(_lib.ptr(d_obs), _lib.ptr(d_xyz), _lib.ptr(d_off), P, _lib.ptr(models), float(max_error),
                                                _lib.ptr(mask), _lib.stream_ptr()), "vc_absolute_pose_inliers")
        masks.append(mask)
    torch.cuda.synchronize()
    return counts.cpu().numpy(), np.stack([m.cpu().numpy() for m in masks])


def test_scores_and_masks_equal_the_spec_bit_for_bit():
    """Ragged problems of 1, 255 and 1500 correspondences x 70 hypotheses: the true pose, poses around it whose inlier sets
    differ, the mirrored camera (every point behind it), hypotheses with one NaN entry and all NaN."""
    sizes = [1, 255, 1500]
    rs = np.random.RandomState(11)
    obs, xyz = [], []
    for k, n in enumerate(sizes):
        o, X, _ = ua.registration_problem(40 + k, n, 0.3, noise=4.0)
        X[::7, 2] -= 12.0                                               # every seventh point behind the camera
        obs.append(o), xyz.append(X)
    hyp = np.zeros((3, 70, 12), np.float32)
    for p in range(3):
        for k in range(70):
            R = ua.rodrigues(rs.normal(0, 0.004 * (k % 10), 3)) @ ue.SCENE_R
            hyp[p, k] = ua.projection_matrix(ue.SCENE_K, R, ue.SCENE_T + rs.normal(0, 0.02 * (k % 7), 3))
        hyp[p, 3] = -hyp[p, 0]
        hyp[p, 5, 6] = np.nan
        hyp[p, 69] = np.nan
    offsets = np.cumsum([0] + sizes)
    obs_all, xyz_all = np.concatenate(obs), np.concatenate(xyz)
    for max_error in (12.0, 0.0):
        counts, masks = run_score(obs_all, xyz_all, offsets, hyp, max_error)
        want = np.array([[ua.score(hyp[p, k], obs[p], xyz[p], max_error) for k in range(70)] for p in range(3)])
        assert np.array_equal(counts, want)
        for k in range(70):
            assert np.array_equal(masks[k], np.concatenate([ua.inliers(hyp[p, k], obs[p], xyz[p], max_error) for p in range(3)]).astype(np.uint8)), k
    counts, _ = run_score(obs_all, xyz_all, offsets, hyp, 12.0)
    assert (counts[:, [5, 69]] == 0).all() and counts[2, 0] > 600 and len(set(counts[2])) > 10
    assert (counts[:, 3] <= np.array([1, 37, 215])).all()              # the mirrored camera can only see the points behind the true one


def test_argument_checks_on_device_pointers():
    from vit_colmap_amd import _lib

    lib = _lib.load()
    x, X = ua.exact_problem(40)
    rays, xyz, off, s = dev(x), dev(X), dev(np.array([0, 40], np.int32)), dev(np.arange(3, dtype=np.int32).reshape(1, 1, 3))
    pose = torch.zeros((1, 1, 4, 12), dtype=torch.float64, device="cuda")
    c = torch.zeros((1, 1), dtype=torch.int32, device="cuda")
    good = [_lib.ptr(rays), _lib.ptr(xyz), _lib.ptr(off), 1, _lib.ptr(s), 1, _lib.ptr(pose), _lib.ptr(c), _lib.stream_ptr()]
    assert lib.vc_p3p(*good) == 0
    for pos in (0, 1, 2, 4, 6, 7):
        args = list(good)
        args[pos] = None
        assert lib.vc_p3p(*args) == -1, pos
    for pos in (3, 5):
        args = list(good)
        args[pos] = -1
        assert lib.vc_p3p(*args) == -1, pos
        args[pos] = 0
        assert lib.vc_p3p(*args) == 0, pos
    torch.cuda.synchronize()
    assert int(c[0, 0]) >= 1

    obs, xyz4 = dev(np.zeros((40, 2), np.float32)), dev(np.ones((41, 4), np.float32))
    hyp = dev(np.zeros((1, 2, 12), np.float32))
    counts = torch.full((1, 2), -7, dtype=torch.int32, device="cuda")
    mask = torch.full((40,), 9, dtype=torch.uint8, device="cuda")
    good = [_lib.ptr(obs), _lib.ptr(xyz4), _lib.ptr(off), 1, _lib.ptr(hyp), 2, 12.0, _lib.ptr(counts), _lib.stream_ptr()]
    assert lib.vc_absolute_pose_score(*good) == 0
    for pos in (0, 1, 2, 4, 7):
        args = list(good)
        args[pos] = None
        assert lib.vc_absolute_pose_score(*args) == -1, pos
    for pos in (3, 5):
        args = list(good)
        args[pos] = -1
        assert lib.vc_absolute_pose_score(*args) == -1, pos
        args[pos] = 0
        assert lib.vc_absolute_pose_score(*args) == 0, pos
    args = list(good)
    args[6] = -1.0
    assert lib.vc_absolute_pose_score(*args) == -1
    args = list(good)
    args[1] = _lib.ptr(xyz4.reshape(-1)[1:])                            # 4 bytes past a 16-byte boundary
    assert lib.vc_absolute_pose_score(*args) == -1
    args = list(good)
    args[3] = 65535 * 32 + 1
    assert lib.vc_absolute_pose_score(*args) == -2
    good = [_lib.ptr(obs), _lib.ptr(xyz4), _lib.ptr(off), 1, _lib.ptr(hyp), 12.0, _lib.ptr(mask), _lib.stream_ptr()]
    assert lib.vc_absolute_pose_inliers(*good) == 0
    for pos in (0, 1, 2, 4, 6):
        args = list(good)
        args[pos] = None
        assert lib.vc_absolute_pose_inliers(*args) == -1, pos
    args = list(good)
    args[3] = -1
    assert lib.vc_absolute_pose_inliers(*args) == -1
    args[3] = 0
    assert lib.vc_absolute_pose_inliers(*args) == 0
    args = list(good)
    args[5] = float("nan")
    assert lib.vc_absolute_pose_inliers(*args) == -1
    torch.cuda.synchronize()
    assert (counts.cpu().numpy() == 0).all() and (mask.cpu().numpy() == 0).all()      # the zero matrix has p_w = 0: no inlier


# ---- the RANSAC tail ------------------------------------------------------------------------------------------------------------------
NAN12 = np.full(12, np.nan, np.float32)
TAIL_K = 69


def tail_problems():
    """-> list of dict(obs, xyz, hyp (69, 12), kind, refit (12,), ok): the ragged batch of the tail tests.  The correspondences
    are those of test_scores_and_masks_equal_the_spec_bit_for_bit (below a wave, a partial fourth wave, many rounds), the
    hypotheses its poses around the scene pose without the exact one; `refit` and `ok` are what the callback hands back.
    Counts measured with the specification on the CPU: the best hypothesis of the 1 / 255 / 1500 problems has 1 / 176 / 1040
    inliers, the true pose 1 / 177 / 1043, the turned pose 0; 21 hypotheses of the 1-point problem tie at 1."""
    rs = np.random.RandomState(11)
    true = ua.projection_matrix(ue.SCENE_K, ue.SCENE_R, ue.SCENE_T)
    turned = ua.projection_matrix(ue.SCENE_K, ua.rodrigues(np.array([0.0, 0.05, 0.0])) @ ue.SCENE_R, ue.SCENE_T)
    data = []
    for k, n in enumerate([1, 255, 1500]):
        o, X, _ = ua.registration_problem(40 + k, n, 0.3, noise=4.0)
        hyp = np.zeros((TAIL_K + 1, 12), np.float32)
        for j in range(TAIL_K + 1):
            R = ua.rodrigues(rs.normal(0, 0.004 * (j % 10), 3)) @ ue.SCENE_R
            hyp[j] = ua.projection_matrix(ue.SCENE_K, R, ue.SCENE_T + rs.normal(0, 0.02 * (j % 7), 3))
        data.append((o, X, hyp[1:]))                                   # j = 0 is the scene pose itself

    def problem(which, kind, refit, ok=True):
        o, X, hyp = data[which]
        return dict(obs=o, xyz=X, hyp=hyp.copy(), kind=kind, refit=refit, ok=ok)

    ps = [problem(0, "taken", true), problem(1, "taken", true), problem(2, "taken", true),      # the 1-point problem on equality
          problem(1, "rejected", turned),                              # a refit with fewer inliers
          problem(2, "ok_false", true, ok=False),                      # the callback offers a better model but says ok = False
          problem(1, "nan_ok", NAN12),                                 # the callback says ok = True and hands back NaN
          dict(obs=np.zeros((0, 2), np.float32), xyz=np.zeros((0, 3), np.float32), hyp=np.tile(NAN12, (TAIL_K, 1)), kind="empty",
               refit=NAN12, ok=False)]
    void = problem(1, "void", NAN12, ok=False)                         # every hypothesis void: NaN model, empty mask, count 0
    void["hyp"][:] = np.nan
    return ps + [void]


def run_tail(ps):
    """_ransac_tail with counts from score_poses and a refit callback that hands back the problems' own models on the CPU
    -> (final, mask, count, kbest, use) as numpy, what the callback saw, and the offsets."""
    from vit_colmap_amd.mapping.absolute_pose import pose_masks, score_poses
    from vit_colmap_amd.matching import _common

    offs = np.cumsum([0] + [len(p["obs"]) for p in ps])
    xyz4, offsets, _, _ = _common._pair_batch([np.concatenate([p["xyz"], np.ones((len(p["xyz"]), 1), np.float32)], axis=1) for p in ps],
                                              None, "cuda")
    obs = dev(np.concatenate([p["obs"] for p in ps]))
    hyp32 = dev(np.stack([p["hyp"] for p in ps]).astype(np.float32))
    score, mask = partial(score_poses, obs, xyz4, offsets, max_error=12.0), partial(pose_masks, obs, xyz4, offsets, max_error=12.0)
    counts = score(hyp32).to(torch.int64)
    seen = {}

    def refit(m, nbest):
        assert m.dtype == torch.bool and m.shape == (offs[-1],) and nbest.shape == (len(ps),)
        seen.update(mask=m.cpu().numpy(), nbest=nbest.cpu().numpy())
        return dev(np.stack([p["refit"] for p in ps])), dev(np.array([p["ok"] for p in ps]))

    res = _common._ransac_tail(hyp32, counts, score, mask, refit)
    torch.cuda.synchronize()
    return [r.cpu().numpy() for r in res], seen, offs


def check_tail(ps):
    (final, mask, count, kbest, use), seen, offs = run_tail(ps)
    assert final.dtype == np.float32 and mask.dtype == bool and mask.shape == (offs[-1],)
    kinds = {}
    for p, pr in enumerate(ps):
        obs, xyz, hyp = pr["obs"], pr["xyz"], pr["hyp"]
        # the rule: most inliers, lowest index on ties; the refit is taken iff it is ok and has no fewer inliers; no inlier, no model
        c = np.array([ua.score(h, obs, xyz) for h in hyp])
        k = int(np.argmax(c))
        rc = ua.score(pr["refit"], obs, xyz)
        take = bool(pr["ok"] and rc >= c[k])
        want, n = (pr["refit"], rc) if take else (hyp[k], int(c[k]))
        want = want if n > 0 else NAN12
        sl = slice(offs[p], offs[p + 1])
        assert np.array_equal(seen["mask"][sl], ua.inliers(hyp[k], obs, xyz)) and seen["nbest"][p] == c[k], (p, pr["kind"])
        assert kbest[p] == k and bool(use[p]) == take and count[p] == n, (p, pr["kind"], kbest[p], k, use[p], take, count[p], n)
        assert np.array_equal(final[p], want, equal_nan=True), (p, pr["kind"])
        assert np.array_equal(mask[sl], ua.inliers(want, obs, xyz)) and mask[sl].sum() == n, (p, pr["kind"])
        kinds.setdefault(pr["kind"], []).append(dict(k=k, n=n, best=int(c[k]), rc=rc, take=take, ties=int((c == c[k]).sum())))
    return kinds


def test_ransac_tail_follows_the_rule_exactly_under_the_pose_residual():
    kinds = check_tail(tail_problems())
    assert [d["take"] for d in kinds["taken"]] == [True] * 3
    assert kinds["taken"][0]["rc"] == kinds["taken"][0]["best"] == 1 and kinds["taken"][0]["ties"] > 1      # equality; lowest rank
    assert all(d["rc"] > d["best"] > 0 for d in kinds["taken"][1:])
    assert kinds["rejected"][0]["rc"] < kinds["rejected"][0]["best"] and not kinds["rejected"][0]["take"]
    assert kinds["ok_false"][0]["rc"] > kinds["ok_false"][0]["best"] and not kinds["ok_false"][0]["take"]
    assert kinds["nan_ok"][0]["rc"] == 0 and not kinds["nan_ok"][0]["take"] and kinds["nan_ok"][0]["n"] > 0
    assert kinds["void"][0]["n"] == 0 and kinds["empty"][0]["n"] == 0


def test_ransac_tail_with_a_single_pose_hypothesis():
    """K = 1, the shape in which three of a workgroup's four waves idle: every problem of the batch with one hypothesis, the
    255-point one with its best."""
    ps = tail_problems()
    best = int(np.argmax([ua.score(h, ps[1]["obs"], ps[1]["xyz"]) for h in ps[1]["hyp"]]))
    one = [dict(pr, hyp=pr["hyp"][[best if p == 1 else 0]]) for p, pr in enumerate(ps)]
    kinds = check_tail(one)
    assert [d["take"] for d in kinds["taken"]] == [True] * 3 and kinds["taken"][1]["best"] > 0
    assert not kinds["rejected"][0]["take"] and kinds["rejected"][0]["n"] > 0
    assert kinds["void"][0]["n"] == 0 and kinds["empty"][0]["n"] == 0


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------
def rule_problems():
    ps = [ua.registration_problem(60 + k, n, frac) for k, (n, frac) in
          enumerate([(100, 0.0), (160, 0.1), (220, 0.2), (280, 0.3), (340, 0.4), (400, 0.5)])]
    ps.append(ua.registration_problem(70, 20, 0.0))                    # a good pose with too few inliers to accept
    ps.append(ua.registration_problem(71, 150, 1.0))                   # all outliers
    return ps


def test_estimate_absolute_poses_follows_the_specs_rule():
    from vit_colmap_amd.mapping.absolute_pose import estimate_absolute_poses

    ps = rule_problems()
    spec = [ua.estimate_absolute_pose(o, X, ue.SCENE_K, 100 + k) for k, (o, X, _) in enumerate(ps)]
    got = estimate_absolute_poses([dict(obs=o, xyz=X, K=ue.SCENE_K, seed=100 + k) for k, (o, X, _) in enumerate(ps)], "cuda")
    worst = np.max([ua.pose_error(s["R"], s["t"]) for s in spec[:6]], axis=0)
    for k, (g, s) in enumerate(zip(got, spec)):
        rot, pos = ua.pose_error(ua.quat_to_rot(g["qvec"]), g["tvec"])
        print(f"problem {k}: success {g['success']} (spec {s['success']}) inliers {g['num_inliers']} (spec {s['num_inliers']}) "
              f"rotation {rot:.4f} deg centre {pos:.5f} (spec worst {worst})")
    assert [s["success"] for s in spec] == [True] * 6 + [False, False]
    for k, (g, s) in enumerate(zip(got, spec)):
        assert g["success"] == s["success"], k
        assert abs(g["num_inliers"] - s["num_inliers"]) <= N_P_MARGIN, k
        assert g["inlier_mask"].dtype == bool and g["inlier_mask"].shape == (len(ps[k][0]),) and g["inlier_mask"].sum() == g["num_inliers"]
        if k < 6:
            rot, pos = ua.pose_error(ua.quat_to_rot(g["qvec"]), g["tvec"])
            assert rot <= 2 * worst[0] and pos <= 2 * worst[1], k
            assert abs(np.linalg.norm(g["qvec"]) - 1) < 1e-12
    assert estimate_absolute_poses([], "cuda") == []
    empty = estimate_absolute_poses([dict(obs=np.zeros((0, 2)), xyz=np.zeros((0, 3)), K=ue.SCENE_K, seed=1)], "cuda")
    assert len(empty) == 1 and not empty[0]["success"] and empty[0]["inlier_mask"].shape == (0,)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def _two_view_bytes(path):
    import sqlite3

    con = sqlite3.connect(str(path))
    rows = con.execute("SELECT * FROM two_view_geometries ORDER BY pair_id").fetchall()
    con.close()
    return rows


def test_match_exhaustive_then_build_seed_model_end_to_end(tmp_path):
    from vit_colmap_amd.mapping import SparseModel, build_seed_model
    from vit_colmap_amd.matching import match_exhaustive
    from vit_colmap_amd.utils.config import MatchingConfig

    scene = ua.arc_scene()
    opts = MatchingConfig(compute_relative_pose=True).to_matching_options()
    write_scene_db(tmp_path / "seed.db", scene)
    match_exhaustive(database_path=str(tmp_path / "seed.db"), matching_options=opts)
    rows_before = _two_view_bytes(tmp_path / "seed.db")
    model = build_seed_model(tmp_path / "seed.db")
    assert sorted(model.images) == [1, 2, 3, 4, 5] and len(model.points3D) >= 100
    # the specification's seed model on the same database content
    spec = ua.seed_model(scene_images(scene), read_pairs(tmp_path / "seed.db"))
    a, b = spec["initial_pair"]
    spec_rot, spec_pos = ua.align_errors(spec["poses"], scene, a, b)
    rot, pos = ua.align_errors({i: (ua.quat_to_rot(im["qvec"]), im["tvec"]) for i, im in model.images.items()}, scene, a, b)
    print(f"pair {model.initial_pair}, {len(model.points3D)} points, mean track {model.mean_track_length():.2f}, rotation {rot:.4f} deg "
          f"(spec {spec_rot:.4f}), centre {pos:.5f} baselines (spec {spec_pos:.5f})")
    assert model.initial_pair == spec["initial_pair"] and len(model.points3D) == len(spec["xyz"])
    assert rot <= 2 * spec_rot and pos <= 2 * spec_pos
    for k, track in enumerate(spec["tracks"]):
        assert model.points3D[k + 1]["track"][:2] == track[:2]
    model.write_text(tmp_path / "sparse" / "seed")
    assert SparseModel.read_text(tmp_path / "sparse" / "seed") == model
    # building the model only reads: the rows are byte for byte what matching wrote
    assert len(rows_before) == 10 and _two_view_bytes(tmp_path / "seed.db") == rows_before


def test_pipeline_without_the_flag_writes_no_seed_model_and_todays_rows(tmp_path, monkeypatch):
    """Pipeline.run over a prepared database (the extractor is a stub that writes nothing) with the flag off and on.  Off:
    no sparse/seed, nothing of the mapping package imported, the same statistics.  On: the rows of two_view_geometries after
    the run are byte for byte those that matching had written when the seed step began, so the flag adds nothing to them.
    Two matching runs are not compared byte for byte: the verifier's refits accumulate with atomics, so two launches of the
    same code differ in the last bits of the stored matrices; their pairs and configurations are equal."""
    import sys

    from vit_colmap_amd.pipeline import run_pipeline as rp
    from vit_colmap_amd.utils.config import Config

    class StubExtractor:
        device = "cuda"
        prior_focal_length = False

        def extract(self, image_dir, db_path, camera_model, camera_params):
            pass

    monkeypatch.setattr(rp.Pipeline, "_make_extractor", lambda self: StubExtractor())
    scene = ua.arc_scene()
    stats, rows_at_seed_step = {}, []
    write_seed = rp.Pipeline._write_seed_model

    def snapshot_then_write(self, db_path, output_dir, device):
        rows_at_seed_step.append(_two_view_bytes(db_path))
        return write_seed(self, db_path, output_dir, device)

    monkeypatch.setattr(rp.Pipeline, "_write_seed_model", snapshot_then_write)
    import vit_colmap_amd

    if hasattr(vit_colmap_amd, "mapping"):      # restored with sys.modules, so that both name the same module for later tests
        monkeypatch.setattr(vit_colmap_amd, "mapping", vit_colmap_amd.mapping)
    monkeypatch.delitem(sys.modules, "vit_colmap_amd.mapping", raising=False)
    for name, flag in (("off", False), ("on", True)):
        write_scene_db(tmp_path / f"{name}.db", scene)
        cfg = Config()
        cfg.camera.prior_focal_length, cfg.matching.compute_relative_pose, cfg.do_reconstruction = True, True, False
        cfg.reconstruction.seed_model = flag
        p = rp.Pipeline(cfg)
        p.run(tmp_path / "images", tmp_path / name, tmp_path / f"{name}.db")
        stats[name] = p.last_stats
        if not flag:
            assert "vit_colmap_amd.mapping" not in sys.modules            # with the flag off nothing new is imported
    assert not (tmp_path / "off" / "sparse").exists() and "seed_model" not in stats["off"]
    assert sorted(f.name for f in (tmp_path / "on" / "sparse" / "seed").iterdir()) == ["cameras.txt", "images.txt", "points3D.txt"]
    s = stats["on"]["seed_model"]
    assert s["registered_images"] == 5 and s["num_points3D"] >= 100 and s["mean_track_length"] > 3 and len(s["initial_pair"]) == 2
    assert {k: v for k, v in stats["on"].items() if k != "seed_model"}.keys() == stats["off"].keys()
    on, off = _two_view_bytes(tmp_path / "on.db"), _two_view_bytes(tmp_path / "off.db")
    assert len(rows_at_seed_step) == 1 and on == rows_at_seed_step[0]          # only the run with the flag reaches the seed step
    assert len(off) == 10 and [(r[0], r[4]) for r in on] == [(r[0], r[4]) for r in off]      # (pair_id, config)
