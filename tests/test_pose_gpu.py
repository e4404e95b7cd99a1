"""GPU tests of two-view relative pose: vc_two_view_pose against the numpy specification of
tests/util_pose.py — counts, choice and midpoints exactly, the median angle to atan2's accuracy —, then verify_pairs with
`relative_pose=True` against the specification's rule fed the GPU's own models, and match_exhaustive end to end."""
from functools import lru_cache

import numpy as np
import pytest
import torch

from oracle import two_view_oracle as tv
import util_essential as ue
import util_pose as up
from vit_colmap_amd.database.colmap_db import _quat_to_rot
from test_essential_spec import NONPLANAR, PAIR_ID
from test_pose_spec import FLOOR, PAIRS, SEEDS, make_pose_db, read_rows

pytestmark = pytest.mark.gpu

LDS_KEYS = 4096       # csrc/pose.hip kLdsKeys: a pair with more inliers keeps its angle keys in the workspace
ANGLE_ULP = 64        # the median's inputs are bit-identical on both sides; the two atan2 implementations document single-digit ulp
TOL = 1e-6            # rad: test_essential_gpu's matrix tolerance, here on the pose of the same model decomposed on either side
# |n_front(GPU) - n_front(spec)| allowed per scene: the largest |difference| the specification itself shows on the CPU when the
# matrix it decomposes is moved by TOL (relative, Frobenius) in a random direction (0 on all eleven scenes, four directions
# each), plus 1
N_FRONT_MARGIN = 0 + 1
# tri_angle: the largest relative change under the same move is 7.6e-4 (the pure-rotation scenes), rounded up
TRI_REL = 1e-3
K = ue.SCENE_K


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_kernel(pairs, points=True, workspace=True):
    """pairs: list of (xn (n, 4), cand (4, 12)) -> front (P, 4), best (P,), tri (P,), midpoints (total, 3) | None; the outputs
    are pre-filled, so a slot the kernel never wrote cannot pass for a result."""
    from vit_colmap_amd import _lib

    lib = _lib.load()
    P = len(pairs)
    xn = np.concatenate([np.asarray(x, np.float64).reshape(-1, 4) for x, _ in pairs])
    offsets = np.concatenate([[0], np.cumsum([len(x) for x, _ in pairs])]).astype(np.int32)
    d_xn, d_off, d_cand = dev(xn), dev(offsets), dev(np.stack([c for _, c in pairs]).astype(np.float64))
    front = torch.full((P, 4), -7, dtype=torch.int32, device="cuda")
    best = torch.full((P,), -7, dtype=torch.int32, device="cuda")
    tri = torch.full((P,), 7.0, dtype=torch.float64, device="cuda")
    pts = torch.full((len(xn), 3), 7.0, dtype=torch.float64, device="cuda") if points else None
    ws_bytes = int(lib.vc_two_view_pose_workspace_bytes(P, len(xn))) if workspace else 0
    assert ws_bytes == (8 * len(xn) if workspace else 0)
    ws = torch.full((len(xn) + 8,), -1, dtype=torch.int64, device="cuda") if workspace else None
    _lib.check(lib.vc_two_view_pose(_lib.ptr(d_xn), _lib.ptr(d_off), P, _lib.ptr(d_cand), _lib.ptr(front), _lib.ptr(best), _lib.ptr(tri),
                                    _lib.ptr(pts), _lib.ptr(ws), ws_bytes, _lib.stream_ptr()), "vc_two_view_pose")
    torch.cuda.synchronize()
    if workspace:
        assert (ws[len(xn):] == -1).all(), "the kernel wrote past its workspace"
    return front.cpu().numpy(), best.cpu().numpy(), tri.cpu().numpy(), None if pts is None else pts.cpu().numpy(), offsets


def scene_points(rs, n, wrong=0.0, R=None, t=None):
    """n correspondences of the scene's motion (or of X2 = R X + t) in normalised coordinates with 1e-3 noise; a fraction is
    replaced by random ones.  Under a motion that is given, a point not at least 0.5 in front of the second camera is drawn again."""
    X = np.stack([rs.uniform(-3, 3, n), rs.uniform(-2, 2, n), rs.uniform(4, 9, n)], axis=1)
    given = R is not None or t is not None
    R, t = ue.SCENE_R if R is None else np.asarray(R, np.float64), ue.SCENE_T if t is None else np.asarray(t, np.float64)
    while given:                                                        # the default scene draws exactly what it always drew
        behind = (X @ R.T + t)[:, 2] < 0.5
        if not behind.any():
            break
        k = int(behind.sum())
        X[behind] = np.stack([rs.uniform(-3, 3, k), rs.uniform(-2, 2, k), rs.uniform(4, 9, k)], axis=1)
    X2 = X @ R.T + t
    xn = np.concatenate([X[:, :2] / X[:, 2:], X2[:, :2] / X2[:, 2:]], axis=1) + 1e-3 * rs.standard_normal((n, 4))
    bad = rs.uniform(size=n) < wrong
    xn[bad] = rs.uniform(-0.5, 0.5, (int(bad.sum()), 4))
    return xn


@lru_cache(maxsize=None)
def kernel_cases():
    """The ragged batch and the specification's answer for each pair, computed once."""
    rs = np.random.RandomState(21)
    four = up.e_candidates(ue.true_essential())
    true = int(np.argmax([up.triangulate(scene_points(rs, 20), c)[0].sum() for c in four]))
    nan = np.full(12, np.nan)
    away = four[true].copy()
    away[9:] = -away[9:]                                                # the true rotation with -t: every point behind both cameras
    still = four[true].copy()
    still[9:] = 0.0                                                     # t = 0
    pairs = [(scene_points(rs, n, 0.2), four) for n in (0, 1, 2, 63, 64, 65, 300, LDS_KEYS, LDS_KEYS + 1)]
    pairs[5][0][7] = np.nan                                             # a point that is not finite is in front of nothing
    pairs[5][0][9, 2] = np.inf
    pairs.append((scene_points(rs, 50, 0.2), np.stack([four[true], nan, nan, nan])))          # one candidate, three unused slots
    pairs.append((scene_points(rs, 50, 0.2), np.stack([still, nan, four[true], nan])))        # t = 0 counts nothing
    pairs.append((scene_points(rs, 50), np.stack([away, nan, still, nan])))                   # nothing in front of any candidate
    pairs.append((scene_points(rs, 50, 0.2), np.stack([nan, four[true], four[true], away])))  # a tie: the lower slot
    pairs.append((scene_points(rs, 2), np.stack([four[true], nan, nan, nan])))                # two points in front: the even median
    return pairs, [up.choose(x, c) for x, c in pairs], true


def _compare(got, want_all, points):
    front, best, tri, pts, offsets = got
    for p, (counts, b, angle, X) in enumerate(want_all):
        assert np.array_equal(front[p], counts), (p, front[p], counts)
        assert best[p] == b, p
        assert abs(tri[p] - angle) <= ANGLE_ULP * np.spacing(angle), (p, tri[p], angle, abs(tri[p] - angle) / np.spacing(angle))
        if points:
            g = pts[offsets[p]:offsets[p + 1]]
            assert np.array_equal(np.isnan(g), np.isnan(X)), p
            assert np.array_equal(np.nan_to_num(g).view(np.uint64), np.nan_to_num(X).view(np.uint64)), p      # bit for bit


def test_kernel_equals_the_specification_on_a_ragged_batch():
    pairs, want, true = kernel_cases()
    got = run_kernel(pairs)
    worst = max(abs(t - w[2]) / np.spacing(w[2]) for t, w in zip(got[2], want) if w[2] > 0)
    print(f"in front {got[0].tolist()} best {got[1].tolist()} worst angle difference {worst:.1f} ulp")
    _compare(got, want, True)
    # what the special pairs are there for
    front, best, tri = got[:3]
    assert [len(x) for x, _ in pairs[:9]] == [0, 1, 2, 63, 64, 65, 300, LDS_KEYS, LDS_KEYS + 1]
    assert best[0] == 0 and tri[0] == 0 and not front[0].any()                                  # no inliers
    assert all(best[p] == true and 0.7 * len(pairs[p][0]) <= front[p, true] < len(pairs[p][0]) for p in (6, 7, 8))
    assert best[9] == 0 and not front[9, 1:].any() and front[9, 0] > 30
    assert best[10] == 2 and front[10, 0] == 0
    assert best[11] == 0 and tri[11] == 0 and not front[11].any() and np.isnan(got[3][got[4][11]:got[4][12]]).all()
    assert best[12] == 1 and front[12, 1] == front[12, 2] > front[12, 3]
    assert front[13, 0] == 2 and best[13] == 0


def test_kernel_without_out_points_gives_the_same_numbers():
    pairs, want, _ = kernel_cases()
    _compare(run_kernel(pairs, points=False), want, False)


def test_a_pair_whose_keys_the_workspace_cannot_hold_is_flagged_and_the_others_are_not():
    pairs, want, _ = kernel_cases()
    front, best, tri, pts, offsets = run_kernel(pairs, workspace=False)
    big = 8                                                            # the pair of LDS_KEYS + 1 inliers
    assert best[big] == -1 and np.isnan(tri[big]) and np.isnan(pts[offsets[big]:offsets[big + 1]]).all()
    assert np.array_equal(front[big], want[big][0])
    keep = [p for p in range(len(pairs)) if p != big]
    _compare((front[keep], best[keep], tri[keep], None, None), [want[p] for p in keep], False)


def test_wrapper_checks_its_tensors_and_returns_the_kernels_numbers():
    from vit_colmap_amd.matching import pose

    pairs, want, _ = kernel_cases()
    xn = np.concatenate([x for x, _ in pairs[:7]])
    offsets = np.concatenate([[0], np.cumsum([len(x) for x, _ in pairs[:7]])]).astype(np.int32)
    cand = np.stack([c for _, c in pairs[:7]])
    front, best, tri, pts = pose.two_view_pose(dev(xn), dev(offsets), dev(cand), points=True)
    _compare((front.cpu().numpy(), best.cpu().numpy(), tri.cpu().numpy(), pts.cpu().numpy(), offsets), want[:7], True)
    with pytest.raises(ValueError):
        pose.two_view_pose(dev(xn.astype(np.float32)), dev(offsets), dev(cand))


# ---- verify_pairs(relative_pose=True) ---------------------------------------------------------------------------------------------
def _angle_between(a, b):
    """Angle (rad) that the chord |a - b| of two rotations (Frobenius) or two unit vectors spans."""
    a, b = np.asarray(a), np.asarray(b)
    chord = np.linalg.norm(a - b)
    return 2 * np.arcsin(min(1.0, chord / (2 * np.sqrt(2)) if a.ndim == 2 else chord / 2))


def _same_matrix(a, b):
    """Two runs of one estimate: both empty, or within TOL in Frobenius distance at unit norm (test_essential_gpu's measure)."""
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    na, nb = np.linalg.norm(a), np.linalg.norm(b)
    if na == 0 or nb == 0:
        return na == nb
    return np.linalg.norm(a / na - b / nb) <= TOL and abs(na - nb) <= TOL * nb


def _assert_same_estimates(a, b, what, pose):
    """a, b: one pair in two runs of the same code (results or database rows).  Two launches do not return the same bits — the
    refits accumulate their normal equations with atomics — so matrices are compared with `_same_matrix`.  Where H explains the
    matches (configuration 6 before the split) the points are coplanar or the motion a rotation, E and what is derived from
    it (F, model9 of an F model, qvec, tvec) are not determined by the data and repeat only as far as that noise lets them: there
    the comparison is H's alone, plus everything discrete."""
    assert np.array_equal(a["inlier_matches"], b["inlier_matches"]), what
    assert _same_matrix(a["H"], b["H"]), (what, "H")
    if tv.CONFIG_PLANAR_OR_PANORAMIC in (a["config"], b["config"]):
        return
    for k in ("F", "E", "model9"):
        if k in a or k in b:
            assert _same_matrix(a[k], b[k]), (what, k)
    if pose and "qvec" in a:
        assert _angle_between(_quat_to_rot(a["qvec"]), _quat_to_rot(b["qvec"])) <= TOL and _angle_between(a["tvec"], b["tvec"]) <= TOL, what


def test_verify_pairs_with_relative_pose_follows_the_rule_on_the_gpus_own_models():
    """Planar, pure-rotation and non-planar scenes in one batch, and scene 1 once more without priors.  Every pair gets the
    configuration the CPU specification gives its scene (tests/test_pose_spec.py asserts it there: PLANAR, PANORAMIC,
    CALIBRATED); pose, n_front and tri_angle are those of the specification's rule applied to the result's own E / H / model9
    and inliers (the estimates themselves are §4.2c / f's subject)."""
    from vit_colmap_amd.matching.two_view import verify_pairs

    scenes = [("planar", s, 0.3) for s in SEEDS] + [("rotation", s, 0.3) for s in SEEDS] + [("nonplanar", s, f) for s, f in NONPLANAR]
    kps, pair_images, pids, lists = {}, [], [], []
    expected = {"planar": tv.CONFIG_PLANAR, "rotation": tv.CONFIG_PANORAMIC, "nonplanar": tv.CONFIG_CALIBRATED}
    for q, sc in enumerate(scenes + [scenes[6]]):
        if sc[0] == "rotation":
            kp1, kp2, m, _ = up.pure_rotation_two_view(sc[1], outlier_frac=sc[2])
        else:
            kp1, kp2, m, _ = tv.synthetic_two_view(sc[1], outlier_frac=sc[2], planar=sc[0] == "planar")
        kps[2 * q], kps[2 * q + 1] = kp1, kp2
        pair_images.append((2 * q, 2 * q + 1))
        pids.append(PAIR_ID + sc[1])
        lists.append(m)
    n = len(pair_images)
    cameras = (np.tile(K, (2 * n, 1, 1)), np.array([1] * (2 * n - 2) + [0, 0], np.uint8))
    res = verify_pairs(kps, pair_images, pids, lists, cameras=cameras, relative_pose=True)
    off = verify_pairs(kps, pair_images, pids, lists, cameras=cameras)
    assert "tri_angle" not in res[-1] and "qvec" not in res[-1] and res[-1]["config"] == tv.CONFIG_UNCALIBRATED
    for q, sc in enumerate(scenes):
        r = res[q]
        before = tv.CONFIG_PLANAR_OR_PANORAMIC if r["config"] in (tv.CONFIG_PLANAR, tv.CONFIG_PANORAMIC) else r["config"]
        fed = {k: r[k] for k in ("E", "H", "model", "model9", "inlier_matches") if k in r}
        s = up.apply_pose_rule(dict(fed, config=before), kps[2 * q], kps[2 * q + 1], K, K)
        d_rot = _angle_between(_quat_to_rot(r["qvec"]), _quat_to_rot(s["qvec"]))
        d_t = _angle_between(r["tvec"], s["tvec"])
        print(f"{sc}: config {r['config']} n_front {r['n_front']} (rule {s['n_front']}) of {len(r['inlier_matches'])} tri_angle {r['tri_angle']:.6f} (rule {s['tri_angle']:.6f}) pose off the rule's by {d_rot:.2e}, {d_t:.2e} rad")
        assert r["config"] == s["config"] == expected[sc[0]], sc
        assert abs(r["n_front"] - s["n_front"]) <= N_FRONT_MARGIN, sc
        assert d_rot <= TOL and d_t <= TOL, sc
        assert abs(r["tri_angle"] - s["tri_angle"]) <= TRI_REL * s["tri_angle"], sc
        assert r["tri_angle"] >= 2 * FLOOR or r["tri_angle"] <= FLOOR / 2, sc
        assert (not r["tvec"].any()) == (r["config"] == tv.CONFIG_PANORAMIC)
        # everything the option does not own is the option-off run's; for a CALIBRATED pair the pose is choose_pose's
        o = off[q]
        assert o["config"] == before and r["model"] == o["model"] and ("E" in r) == ("E" in o)
        _assert_same_estimates(o, r, sc, pose=True)


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def test_match_exhaustive_writes_planar_panoramic_and_calibrated_rows_and_todays_rows_without_the_option(tmp_path):
    from vit_colmap_amd.matching import match_exhaustive
    from vit_colmap_amd.matching.two_view import verify_pairs
    from vit_colmap_amd.utils.config import MatchingConfig

    for name in ("on.db", "off.db", "parent.db"):
        make_pose_db(tmp_path / name)

    def parents_verify(kps, pair_images, pair_ids, lists, cameras=None):       # the parent's call: `relative_pose=` would be a TypeError
        return verify_pairs(kps, pair_images, pair_ids, lists, cameras=cameras)

    s_on = match_exhaustive(database_path=str(tmp_path / "on.db"), matching_options=MatchingConfig(compute_relative_pose=True).to_matching_options())
    s_off = match_exhaustive(database_path=str(tmp_path / "off.db"), matching_options=MatchingConfig().to_matching_options())
    match_exhaustive(database_path=str(tmp_path / "parent.db"), verify_fn=parents_verify)
    on, off, parent = (read_rows(tmp_path / name) for name in ("on.db", "off.db", "parent.db"))
    for pair, config in PAIRS.items():
        g = on[pair]
        assert g["config"] == config, pair
        assert abs(np.linalg.norm(g["qvec"]) - 1) < 1e-12
        if config == tv.CONFIG_PANORAMIC:
            assert not g["tvec"].any() and ue.pose_errors(g["qvec"], np.array([1.0, 0, 0]))[0] < 1
        else:
            assert abs(np.linalg.norm(g["tvec"]) - 1) < 1e-12 and max(ue.pose_errors(g["qvec"], g["tvec"])) < 5
    posed = [g for g in on.values() if g["config"] != tv.CONFIG_DEGENERATE]
    assert all(g["config"] != tv.CONFIG_PLANAR_OR_PANORAMIC for g in posed)
    assert s_on["pose_pairs"] == len(posed) and s_on["planar_pairs"] >= 1 and s_on["panoramic_pairs"] >= 2
    assert s_off["pose_pairs"] == s_off["planar_pairs"] == s_off["panoramic_pairs"] == 0
    assert off.keys() == parent.keys() == on.keys()
    for pair in off:
        a, b, c = off[pair], parent[pair], on[pair]
        assert a["config"] == b["config"] and a["config"] not in (tv.CONFIG_PLANAR, tv.CONFIG_PANORAMIC), pair
        _assert_same_estimates(a, b, pair, pose=True)                  # option off: the parent's rows
        split = c["config"] in (tv.CONFIG_PLANAR, tv.CONFIG_PANORAMIC)
        assert (tv.CONFIG_PLANAR_OR_PANORAMIC if split else c["config"]) == a["config"], pair
        _assert_same_estimates(a, c, pair, pose=a["config"] == tv.CONFIG_CALIBRATED)    # option on: a CALIBRATED pair keeps choose_pose's pose
        if a["config"] == tv.CONFIG_PLANAR_OR_PANORAMIC:               # an undetermined E is still an essential matrix, a pose a pose
            for g in (a, b, c):
                if g["E"].any():
                    assert np.allclose(np.linalg.svd(g["E"], compute_uv=False), np.array([1, 1, 0]) / np.sqrt(2), atol=1e-9), pair
                assert abs(np.linalg.norm(g["qvec"]) - 1) < 1e-12, pair
