"""The calibrated branch of geometric verification on the CPU: the numpy specification's five-point solver
on 300 exact minimal problems, its decision rule on the synthetic scenes, the focal-length flag's way from the
configuration and the command line into the `cameras` table, the host plumbing of match_exhaustive with the
specification in the seams, and the argument checks of the C entry point."""
import ctypes
import sys
from functools import lru_cache

import numpy as np
import pytest

from oracle import matcher_oracle as mo
from oracle import two_view_oracle as tv
import util_essential as ue
from util_guided import twin_descriptors
from vit_colmap_amd.database.colmap_db import Camera

NONPLANAR = [(1, 0.3), (2, 0.3), (3, 0.3), (4, 0.5), (5, 0.5)]
PLANAR = [1, 2, 3]
PAIR_ID = 1 * 2147483647 + 2


def pinhole(flag=True, model="PINHOLE", params=(600.0, 600.0, 320.0, 240.0)):
    return Camera(model=model, width=640, height=480, params=list(params), has_prior_focal_length=flag)


@lru_cache(maxsize=None)
def scene_result(seed, outlier_frac, planar):
    kp1, kp2, m, is_in = tv.synthetic_two_view(seed, outlier_frac=outlier_frac, planar=planar)
    return ue.verify_pair_calibrated(kp1, kp2, m, PAIR_ID + seed, pinhole(), pinhole()), m, is_in


# ---- the solver ---------------------------------------------------------------------------------------------------------------
def test_spec_solver_finds_the_truth_in_every_minimal_problem():
    Et = ue.true_essential()
    worst, counts = 0.0, set()
    for i in range(300):
        x1, x2 = ue.minimal_problem(i)
        sols = ue.five_point(x1, x2)
        counts.add(len(sols))
        assert 1 <= len(sols) <= 10
        worst = max(worst, min(ue.matrix_distance(Et, E) for E in sols))
        h1, h2 = np.c_[x1, np.ones(5)], np.c_[x2, np.ones(5)]
        for E in sols:
            assert abs(np.linalg.norm(E) - 1) < 1e-12
            assert np.abs(np.einsum("ni,ij,nj->n", h2, E, h1)).max() < 1e-9
            assert abs(np.linalg.det(E)) < 1e-9
            assert np.abs(2 * E @ E.T @ E - np.trace(E @ E.T) * E).max() < 1e-9
    print(f"worst distance to the true E {worst:.3g}, solutions per problem {sorted(counts)}")
    assert worst < 1e-9


def test_spec_solver_returns_nothing_for_degenerate_samples():
    x1, x2 = ue.minimal_problem(0)
    assert len(ue.five_point(x1 * np.nan, x2)) == 0
    assert len(ue.five_point(x1 * 0, x2 * 0)) == 0
    for E in ue.five_point(x1[[0, 1, 2, 3, 3]], x2[[0, 1, 2, 3, 3]]):
        assert np.all(np.isfinite(E))


# ---- the rule -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,outlier_frac", NONPLANAR)
def test_non_planar_scenes_are_calibrated(seed, outlier_frac):
    r, m, is_in = scene_result(seed, outlier_frac, False)
    assert r["config"] == tv.CONFIG_CALIBRATED and r["model"] == "F"
    sv = np.linalg.svd(r["E"], compute_uv=False)
    assert np.allclose(sv, np.array([1, 1, 0]) / np.sqrt(2), atol=1e-9)
    assert abs(np.linalg.norm(r["qvec"]) - 1) < 1e-12 and abs(np.linalg.norm(r["tvec"]) - 1) < 1e-12
    got = set(map(tuple, r["inlier_matches"]))
    truth = set(map(tuple, m[is_in]))
    rot, trans = ue.pose_errors(r["qvec"], r["tvec"])
    print(f"seed {seed}: n_e {r['n_e']} n_f {r['n_f']} n_h {r['n_h']} true inliers {len(truth)} admitted {len(truth & got)} "
          f"wrong {len(got - truth)} rotation {rot:.2f} deg translation {trans:.2f} deg")
    assert len(truth & got) >= 0.98 * len(truth)
    assert len(got) == r["n_e"] >= 0.95 * r["n_f"]
    assert rot < 5 and trans < 15                                      # the pose is the scene's, not one of the three twisted ones
    assert np.allclose(r["F"], tv.stored_f(r["model9"])) and abs(np.linalg.det(r["F"])) < 1e-12


@pytest.mark.parametrize("seed", PLANAR)
def test_planar_scenes_are_planar_or_panoramic(seed):
    r, _, _ = scene_result(seed, 0.3, True)
    assert r["config"] == tv.CONFIG_PLANAR_OR_PANORAMIC
    assert r["n_h"] / max(r["n_e"], r["n_f"]) > 0.8


@pytest.mark.parametrize("cams", [
    (pinhole(False), pinhole()), (pinhole(), pinhole(False)),
    (pinhole(), pinhole(model="SIMPLE_RADIAL", params=(600.0, 320.0, 240.0, 0.01))),
    (pinhole(model="OPENCV", params=(600.0, 600.0, 320.0, 240.0, 0, 0, 1e-3, 0)), pinhole()),
], ids=["first-unflagged", "second-unflagged", "radial-distortion", "opencv-distortion"])
def test_without_two_usable_priors_the_result_is_verify_pairs(cams):
    kp1, kp2, m, _ = tv.synthetic_two_view(1)
    r = ue.verify_pair_calibrated(kp1, kp2, m, PAIR_ID, *cams)
    ref = tv.verify_pair(kp1, kp2, m, PAIR_ID)
    assert r.keys() == ref.keys()
    for k in ref:
        assert np.array_equal(r[k], ref[k]), k


def test_zero_distortion_models_are_usable_and_agree_with_pinhole():
    from vit_colmap_amd.matching.essential import camera_prior

    for cam in (pinhole(model="SIMPLE_PINHOLE", params=(600.0, 320.0, 240.0)), pinhole(model="SIMPLE_RADIAL", params=(600.0, 320.0, 240.0, 0.0)),
                pinhole(model="RADIAL", params=(600.0, 320.0, 240.0, 0.0, 0.0)), pinhole(model="OPENCV", params=(600.0, 600.0, 320.0, 240.0, 0, 0, 0, 0))):
        K, ok = ue.camera_prior(cam)
        Kp, okp, distorted = camera_prior(cam)                      # the product's reading of a camera row is the spec's
        assert ok and okp and not distorted and np.array_equal(K, ue.SCENE_K) and np.array_equal(Kp, K)
    _, okp, distorted = camera_prior(pinhole(model="RADIAL", params=(600.0, 320.0, 240.0, 0.0, 0.1)))
    assert not okp and distorted
    assert camera_prior(pinhole(False))[1:] == (False, False)


def test_pose_choice_recovers_a_known_motion():
    from vit_colmap_amd.matching.essential import choose_pose

    rs = np.random.RandomState(3)
    X = np.stack([rs.uniform(-3, 3, 40), rs.uniform(-2, 2, 40), rs.uniform(4, 9, 40)], axis=1)
    X2 = X @ ue.SCENE_R.T + ue.SCENE_T
    xn = np.concatenate([X[:, :2] / X[:, 2:], X2[:, :2] / X2[:, 2:]], axis=1)
    for E in (ue.true_essential(), -ue.true_essential()):
        q, t, _ = ue.choose_pose(E, xn)
        assert max(ue.pose_errors(q, t)) < 1e-5
        q2, t2 = choose_pose(E, xn)                                    # the product's copy
        assert np.allclose(q, q2) and np.allclose(t, t2)


# ---- the flag -----------------------------------------------------------------------------------------------------------------
def _write_images(tmp_path, n=2):
    from vit_colmap_amd.utils import image_io

    d = tmp_path / "images"
    d.mkdir()
    rs = np.random.RandomState(0)
    for k in range(n):
        image_io.imwrite(d / f"im{k}.png", rs.randint(0, 255, (64, 96, 3), dtype=np.uint8))
    return d


def _camera_flags(db_path):
    from vit_colmap_amd.database import ColmapDatabase

    with ColmapDatabase.open_database(str(db_path)) as h:
        return [h.read_camera(im.camera_id).has_prior_focal_length for im in h.read_all_images()]


@pytest.mark.parametrize("flag", [False, True])
def test_flag_reaches_the_cameras_table_from_config(tmp_path, flag):
    from vit_colmap_amd.pipeline.run_pipeline import Pipeline
    from vit_colmap_amd.utils.config import CameraConfig, Config

    assert CameraConfig().prior_focal_length is False
    images = _write_images(tmp_path)
    cfg = Config()
    cfg.extractor.extractor_type = "dummy"
    cfg.camera.prior_focal_length = flag
    cfg.do_matching = cfg.do_reconstruction = False
    Pipeline(cfg).run(images, tmp_path / "out", tmp_path / "db.db")
    assert _camera_flags(tmp_path / "db.db") == [flag, flag]


def test_flag_reaches_camera_policy_and_the_command_line(monkeypatch, tmp_path):
    from vit_colmap_amd.features.base_extractor import BaseExtractor, camera_policy
    from vit_colmap_amd.pipeline import run_pipeline as rp

    assert BaseExtractor.prior_focal_length is False
    assert camera_policy("PINHOLE", None, (48, 64))(48, 64).has_prior_focal_length is False
    assert camera_policy("PINHOLE", None, (48, 64), prior_focal_length=True)(48, 64).has_prior_focal_length is True
    assert camera_policy("PINHOLE", None, (48, 64), per_image=True, prior_focal_length=True)(20, 30).has_prior_focal_length is True
    seen = []
    monkeypatch.setattr(rp.Pipeline, "run", lambda self, *a, **k: seen.append(self.config.camera.prior_focal_length))
    base = ["prog", "--images", str(tmp_path), "--output", str(tmp_path), "--db", str(tmp_path / "x.db")]
    monkeypatch.setattr(sys, "argv", base)
    rp.main()
    monkeypatch.setattr(sys, "argv", base + ["--prior-focal-length"])
    rp.main()
    assert seen == [False, True]


# ---- the rule on the counts alone ---------------------------------------------------------------------------------------------
def _spec_decision(monkeypatch, M, n_f, n_h, n_e):
    """The specification's rule for one pair whose estimators are replaced by given inlier counts: F and E keep the first
    n rows of the match list, H the last n_h -> (verify_pair_calibrated's result, the matches)."""
    first, last = (lambda n: np.arange(M) < n), (lambda n: np.arange(M) >= M - n)
    eye9 = np.eye(3, dtype=np.float32).reshape(9)
    monkeypatch.setattr(tv, "estimate_model", lambda kind, pts, seed, n_hyp: (eye9, first(n_f) if kind == "F" else last(n_h)))
    monkeypatch.setattr(ue, "estimate_e", lambda pts, seed, K1, K2, n_hyp, perturb: (ue.true_essential(), eye9, first(n_e)))
    kp = (np.random.RandomState(M).rand(M, 2) * 400).astype(np.float32)
    m = np.stack([np.arange(M), np.arange(M)], axis=1).astype(np.uint32)
    cams = [pinhole(flag=n_e is not None)] * 2
    return ue.verify_pair_calibrated(kp, kp + np.float32(1.0), m, PAIR_ID, *cams), m


def test_pair_decision_is_the_specifications_rule_on_both_sides_of_every_threshold(monkeypatch):
    """two_view.pair_decision against util_essential.verify_pair_calibrated (and, without a prior, the oracle's verify_pair)
    for M = 40 (floor 15) and M = 100 (floor 0.25 M = 25): n_f and n_e one below and at the floor, n_e one below and at
    0.95 n_f (37 | 38 of 40, 94 | 95 of 100), n_h at and one above 0.8 n (20 | 21 of 25, 32 | 33 of 40, 80 | 81 of 100) and
    at and one above n; n_e absent included."""
    from vit_colmap_amd.matching.two_view import pair_decision

    seen = set()
    for M in (40, 100):
        for n_f in (14, 15, 24, 25, 40, 100):
            for n_e in (None, 14, 15, 24, 25, 37, 38, 40, 94, 95, 100):
                for n_h in (0, 15, 16, 20, 21, 25, 26, 32, 33, 40, 41, 80, 81, 100):
                    if max(n_f, n_h, n_e or 0) > M:
                        continue
                    res, m = _spec_decision(monkeypatch, M, n_f, n_h, n_e)
                    config, best, model = pair_decision(M, n_f, n_h, n_e)
                    assert config == res["config"], (M, n_f, n_h, n_e)
                    assert (best == "E") == ("E" in res) and (best is None) == (config == tv.CONFIG_DEGENERATE), (M, n_f, n_h, n_e)
                    if best is None:
                        assert model is None and len(res["inlier_matches"]) == 0
                        continue
                    n = n_e if best == "E" else n_f
                    mask = np.arange(M) >= M - n_h if model == "H" else np.arange(M) < n
                    assert np.array_equal(res["inlier_matches"], m[mask]), (M, n_f, n_h, n_e)
                    assert res.get("model", model) == model
                    seen.add((config, best, model))
    assert seen == {(c, b, k) for b, c0 in (("E", tv.CONFIG_CALIBRATED), ("F", tv.CONFIG_UNCALIBRATED))
                    for c, k in ((c0, "F"), (tv.CONFIG_PLANAR_OR_PANORAMIC, "F"), (tv.CONFIG_PLANAR_OR_PANORAMIC, "H"))}


# ---- match_exhaustive with the specification in the seams ------------------------------------------------------------------------
def make_calibrated_db(path, flag=True, n=160):
    """Three views of one scene (view 3: view 2 again, so pair (1, 3) is pair (1, 2) with another seed) with descriptors
    that match by index, under one PINHOLE camera with the scene's intrinsics."""
    from vit_colmap_amd.database import ColmapDatabase

    rs = np.random.RandomState(9)
    kp1, kp2, _, _ = tv.synthetic_two_view(45, n, 0.0, False)
    descs = twin_descriptors(rs, n, n, 128, 3)                        # no look-alikes: every row matches its own index
    db = ColmapDatabase(str(path))
    cam = db.db.write_camera(pinhole(flag))
    for k, (kp, d) in enumerate(zip((kp1, kp2, kp2), descs)):
        i = db.add_image(f"v{k}.png", cam)
        db.add_keypoints(i, kp)
        db.add_descriptors(i, d)
    db.db.close()


def _match_fn(block, counts, pairs, max_ratio, max_distance, cross_check):
    block, counts = np.asarray(block), np.asarray(counts)
    return [mo.match_pair(block[a, : counts[a]], block[b, : counts[b]], max_ratio, max_distance, cross_check) for a, b in pairs]


def _spec_verify_fn(calls):
    def verify_fn(kps, pair_images, pair_ids, lists, cameras=None):
        calls.append(cameras is not None)
        out = []
        for (a, b), pid, m in zip(pair_images, pair_ids, lists):
            if cameras is None:
                out.append(tv.verify_pair(kps[a], kps[b], m, pid))
                continue
            K, prior = cameras
            cams = [Camera(model="PINHOLE", params=[K[i][0, 0], K[i][1, 1], K[i][0, 2], K[i][1, 2]], has_prior_focal_length=bool(prior[i]))
                    for i in (a, b)]
            out.append(ue.verify_pair_calibrated(kps[a], kps[b], m, pid, *cams))
        return out
    return verify_fn


def test_match_exhaustive_writes_calibrated_rows_that_read_back_in_both_directions(tmp_path):
    from vit_colmap_amd.database import ColmapDatabase
    from vit_colmap_amd.database.colmap_db import _quat_to_rot
    from vit_colmap_amd.matching import match_exhaustive

    make_calibrated_db(tmp_path / "cal.db")
    calls = []
    s = match_exhaustive(database_path=str(tmp_path / "cal.db"), match_fn=_match_fn, verify_fn=_spec_verify_fn(calls), device="cpu")
    assert calls == [True] and s["verified_pairs"] == 3
    with ColmapDatabase.open_database(str(tmp_path / "cal.db")) as h:
        for i, j in ((1, 2), (1, 3)):
            g, back = h.read_two_view_geometry(i, j), h.read_two_view_geometry(j, i)
            assert g["config"] == tv.CONFIG_CALIBRATED and len(g["inlier_matches"]) > 100
            assert abs(np.linalg.norm(g["E"]) - 1) < 1e-12 and abs(np.linalg.norm(g["qvec"]) - 1) < 1e-12
            assert abs(np.linalg.norm(g["tvec"]) - 1) < 1e-12
            assert max(ue.pose_errors(g["qvec"], g["tvec"])) < 5
            R, t = _quat_to_rot(g["qvec"]), g["tvec"]
            assert ue.matrix_distance(g["E"], ue.skew(t) @ R / np.linalg.norm(ue.skew(t) @ R)) < 1e-6    # E = [t]x R
            assert np.allclose(back["E"], g["E"].T) and np.allclose(back["F"], g["F"].T)
            assert np.allclose(_quat_to_rot(back["qvec"]), R.T) and np.allclose(back["tvec"], -R.T @ t)
            assert np.array_equal(back["inlier_matches"], g["inlier_matches"][:, ::-1])


def test_match_exhaustive_without_the_flag_calls_verify_fn_as_before(tmp_path):
    from vit_colmap_amd.database import ColmapDatabase
    from vit_colmap_amd.matching import match_exhaustive

    make_calibrated_db(tmp_path / "plain.db", flag=False)
    calls = []
    match_exhaustive(database_path=str(tmp_path / "plain.db"), match_fn=_match_fn, verify_fn=_spec_verify_fn(calls), device="cpu")
    assert calls == [False]
    with ColmapDatabase.open_database(str(tmp_path / "plain.db")) as h:
        g = h.read_two_view_geometry(1, 2)
        assert g["config"] == tv.CONFIG_UNCALIBRATED and not g["E"].any() and not g["tvec"].any()
        assert np.array_equal(g["qvec"], [1, 0, 0, 0])


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------
def test_entry_point_validates_its_arguments_without_a_gpu():
    from vit_colmap_amd import _lib

    lib = _lib.load()
    assert "vc_essential_5pt" in _lib.SIGNATURES
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.vc_essential_5pt(None, None, 1, None, 1, None, None, None) == -1
    for pos in (0, 1, 3, 5, 6):
        args = [p, p, 1, p, 1, p, p, None]
        args[pos] = None
        assert lib.vc_essential_5pt(*args) == -1, pos
    assert lib.vc_essential_5pt(p, p, -1, p, 1, p, p, None) == -1
    assert lib.vc_essential_5pt(p, p, 1, p, -1, p, p, None) == -1
    assert lib.vc_essential_5pt(p, p, 0, p, 128, p, p, None) == 0           # zero work
    assert lib.vc_essential_5pt(p, p, 4, p, 0, p, p, None) == 0
    assert lib.vc_essential_5pt(p, p, 2 ** 31 - 1, p, 2 ** 31 - 1, p, p, None) == -2   # beyond the grid limit; nothing is launched


# ---- two gloo ranks: the cameras travel next to the keypoints ---------------------------------------------------------------------
def _sharded_verify_fn(kps, pair_images, pair_ids, lists, cameras=None):
    """run_sharded's seam: checks what arrives (64 x 96 images under the default PINHOLE parameters, all flagged)."""
    assert cameras is not None
    K, prior = cameras
    assert len(K) == len(prior) == len(kps) and prior.all()
    assert all(np.array_equal(k, [[96.0, 0, 48.0], [0, 96.0, 32.0], [0, 0, 1.0]]) for k in K)
    return [dict(config=tv.CONFIG_DEGENERATE, inlier_matches=np.zeros((0, 2), np.uint32), F=np.zeros((3, 3)), H=np.zeros((3, 3)),
                 n_f=0, n_h=0) for _ in pair_images]


def _dist_worker(rank, world, port, tmp, q):
    import os
    from pathlib import Path

    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from vit_colmap_amd.features.dummy_extractor import DummyExtractor
        from vit_colmap_amd.matching import match_exhaustive
        from vit_colmap_amd.pipeline.distributed import run_sharded

        tmp, calls = Path(tmp), []
        s = match_exhaustive(database_path=str(tmp / "dist.db"), distributed=True, match_fn=_match_fn,
                             verify_fn=_spec_verify_fn(calls), device="cpu")
        dummy = DummyExtractor(step=16)
        st = run_sharded(tmp / "images", tmp / "sharded.db", "PINHOLE", device="cpu", batch_size=2, prior_focal_length=True,
                         feature_fn=lambda imgs: [dummy.features_for(*im.shape[:2]) for im in imgs], match_fn=_match_fn,
                         verify_fn=_sharded_verify_fn)
        q.put(calls == [True] and s["ranks"] == 2 and s["verified_pairs"] == 3 and st["ranks"] == 2 and st["pairs"] == 3)
    finally:
        dist.destroy_process_group()


def test_two_ranks_write_the_single_process_calibrated_rows(tmp_path):
    import socket

    import torch.multiprocessing as mp

    from vit_colmap_amd.database import ColmapDatabase
    from vit_colmap_amd.matching import match_exhaustive

    for name in ("single.db", "dist.db"):
        make_calibrated_db(tmp_path / name)
    _write_images(tmp_path, 3)
    match_exhaustive(database_path=str(tmp_path / "single.db"), match_fn=_match_fn, verify_fn=_spec_verify_fn([]), device="cpu")
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_dist_worker, args=(r, 2, port, str(tmp_path), q)) for r in range(2)]
    for p in procs:
        p.start()
    results = [q.get(timeout=180) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all(results)
    with ColmapDatabase.open_database(str(tmp_path / "single.db")) as a, ColmapDatabase.open_database(str(tmp_path / "dist.db")) as b:
        for pair in ((1, 2), (1, 3), (2, 3)):
            ga, gb = a.read_two_view_geometry(*pair), b.read_two_view_geometry(*pair)
            assert ga["config"] == gb["config"]
            for k in ("inlier_matches", "F", "E", "H", "qvec", "tvec"):
                assert np.array_equal(ga[k], gb[k]), (pair, k)
        assert a.read_two_view_geometry(1, 2)["config"] == tv.CONFIG_CALIBRATED
    assert _camera_flags(tmp_path / "sharded.db") == [True, True, True]
