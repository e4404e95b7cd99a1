"""One level above the minimal solvers, on other camera motions than the one every scene generator defaults to: forward
motion, a 90 degree roll and a 60 degree yaw (three families of tests/util_solver_families.py).  vc_two_view_pose on a ragged
batch, verify_pairs with cameras and estimate_absolute_poses, each under the comparison and the tolerances of its counterpart
on the default motion (test_pose_gpu.py, test_essential_gpu.py, test_absolute_pose_gpu.py)."""
import numpy as np
import pytest

from oracle import two_view_oracle as tv
import test_absolute_pose_gpu as tap
import test_essential_gpu as teg
import test_pose_gpu as tpg
import util_absolute_pose as ua
import util_essential as ue
import util_pose as up
import util_solver_families as uf
from test_essential_spec import PAIR_ID, pinhole

pytestmark = pytest.mark.gpu

MOTIONS = {
    "forward motion": (uf.rot(uf.Y_AXIS, 0.05), np.array([0.02, 0.01, 1.0])),
    "roll 90": (uf.rot(uf.Z_AXIS, np.pi / 2), np.array([0.5, 0.2, 0.1])),
    "yaw 60": (uf.rot(uf.Y_AXIS, 1.05), np.array([-3.0, 0, 1.5])),
}
motions = pytest.mark.parametrize("name", list(MOTIONS))


@motions
def test_two_view_pose_equals_the_specification_on_a_ragged_batch(name):
    """test_pose_gpu's comparison (counts, choice and midpoints exactly, the angle to ANGLE_ULP) on pairs of 1 to 300 points."""
    R, t = MOTIONS[name]
    rs = np.random.RandomState(31)
    E = ue.skew(t) @ R
    four = up.e_candidates(E / np.linalg.norm(E))
    pairs = [(tpg.scene_points(rs, n, 0.2, R, t), four) for n in (1, 2, 63, 64, 65, 300)]
    want = [up.choose(x, c) for x, c in pairs]
    got = tpg.run_kernel(pairs)
    print(f"in front {got[0].tolist()} best {got[1].tolist()}")
    tpg._compare(got, want, True)
    true = int(np.argmin([np.linalg.norm(c[:9].reshape(3, 3) - R) + np.linalg.norm(c[9:] - t / np.linalg.norm(t)) for c in four]))
    assert got[1][5] == true and got[0][5, true] >= 0.7 * 300


def test_verify_pairs_with_cameras_follows_the_spec_on_three_motions():
    """test_essential_gpu's comparison: the specification's configuration, n_e within N_E_MARGIN, the pose within twice the
    specification's worst error over the scenes of the same motion."""
    from vit_colmap_amd.matching.two_view import verify_pairs

    scenes = [(name, seed) for name in MOTIONS for seed in (1, 2)]
    kps, pair_images, pids, lists, spec = {}, [], [], [], []
    for q, (name, seed) in enumerate(scenes):
        R, t = MOTIONS[name]
        kp1, kp2, m, _ = tv.synthetic_two_view(seed, outlier_frac=0.3, R=R, t=t)
        kps[2 * q], kps[2 * q + 1] = kp1, kp2
        pair_images.append((2 * q, 2 * q + 1))
        pids.append(PAIR_ID + seed)
        lists.append(m)
        spec.append(ue.verify_pair_calibrated(kp1, kp2, m, PAIR_ID + seed, pinhole(), pinhole()))
    K = np.tile(ue.SCENE_K, (2 * len(scenes), 1, 1))
    res = verify_pairs(kps, pair_images, pids, lists, cameras=(K, np.ones(2 * len(scenes), np.uint8)))
    worst = {name: np.zeros(2) for name in MOTIONS}
    for (name, _), s in zip(scenes, spec):
        assert s["config"] == tv.CONFIG_CALIBRATED, name                 # the scene is one the specification calibrates
        worst[name] = np.maximum(worst[name], ue.pose_errors(s["qvec"], s["tvec"], *MOTIONS[name]))
    for (name, seed), r, s in zip(scenes, res, spec):
        rot, trans = ue.pose_errors(r["qvec"], r["tvec"], *MOTIONS[name])
        print(f"{name} seed {seed}: config {r['config']} (spec {s['config']}) n_e {r['n_e']} (spec {s['n_e']}) n_f {r['n_f']} n_h {r['n_h']} "
              f"rotation {rot:.2f} translation {trans:.2f} deg (spec worst {worst[name]})")
    for (name, seed), r, s in zip(scenes, res, spec):
        assert r["config"] == s["config"], (name, seed)
        assert abs(r["n_e"] - s["n_e"]) <= teg.N_E_MARGIN, (name, seed)
        rot, trans = ue.pose_errors(r["qvec"], r["tvec"], *MOTIONS[name])
        assert rot <= 2 * worst[name][0] and trans <= 2 * worst[name][1], (name, seed)
        assert np.allclose(np.linalg.svd(r["E"], compute_uv=False), np.array([1, 1, 0]) / np.sqrt(2), atol=1e-9)
        assert abs(np.linalg.norm(r["qvec"]) - 1) < 1e-12 and abs(np.linalg.norm(r["tvec"]) - 1) < 1e-12
        assert r["model"] == s["model"]


@motions
def test_estimate_absolute_poses_follows_the_specs_rule(name):
    """test_absolute_pose_gpu's comparison: success, num_inliers within N_P_MARGIN, the pose within twice the specification's
    worst error over the motion's problems."""
    from vit_colmap_amd.mapping.absolute_pose import estimate_absolute_poses

    R, t = MOTIONS[name]
    ps = [ua.registration_problem(80 + k, n, frac, R=R, t=t) for k, (n, frac) in enumerate([(100, 0.0), (220, 0.2), (400, 0.5)])]
    spec = [ua.estimate_absolute_pose(o, X, ue.SCENE_K, 200 + k) for k, (o, X, _) in enumerate(ps)]
    got = estimate_absolute_poses([dict(obs=o, xyz=X, K=ue.SCENE_K, seed=200 + k) for k, (o, X, _) in enumerate(ps)], "cuda")
    assert [s["success"] for s in spec] == [True] * 3
    worst = np.max([ua.pose_error(s["R"], s["t"], R, t) for s in spec], axis=0)
    for k, (g, s) in enumerate(zip(got, spec)):
        rot, pos = ua.pose_error(ua.quat_to_rot(g["qvec"]), g["tvec"], R, t)
        print(f"problem {k}: success {g['success']} inliers {g['num_inliers']} (spec {s['num_inliers']}) rotation {rot:.4f} deg "
              f"centre {pos:.5f} (spec worst {worst})")
        assert g["success"] == s["success"], k
        assert abs(g["num_inliers"] - s["num_inliers"]) <= tap.N_P_MARGIN, k
        assert g["inlier_mask"].sum() == g["num_inliers"]
        assert rot <= 2 * worst[0] and pos <= 2 * worst[1], k
