"""CPU tests of the growth of the seed model: the numpy specification of tests/util_mapper.py (one track,
the growth rule, the windowed scene), the kernel's per-track function compiled for the host (tools/triangulate_host.cpp)
against it, plain and under the host sanitizers, the product's host logic with the specification in its three GPU seams,
and the pipeline's flag.  No GPU."""
import os
import shutil
import subprocess
import sys
from functools import lru_cache

import numpy as np
import pytest

import util_absolute_pose as ua
import util_essential as ue
import util_mapper as um
from test_absolute_pose_spec import (read_pairs, scene_images, spec_estimate, spec_two_view_pose, truth_pairs, write_scene_db)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
HOST_BUILD = [HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off"]
SOURCE = os.path.join(ROOT, "tools", "triangulate_host.cpp")
# the growth on the 12-view windowed scene with truth_pairs rows, measured: worst rotation 1.52 deg, worst centre 0.0853
# baselines (the drift of chaining poses without bundle adjustment); the bounds are 2x, rounded up
GROW_ROT_BOUND, GROW_POS_BOUND = 3.1, 0.18


# ---- one track: the specification ------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def spec_tracks(kind):
    """The 300 tracks of a kind and the specification's result on each."""
    tracks = [(um.exact_track if kind == "exact" else um.noisy_track)(i) for i in range(300)]
    return tracks, [um.triangulate_track(t[0], t[1], t[3]) for t in tracks]


def test_spec_finds_the_true_point_of_all_300_exact_tracks():
    tracks, spec = spec_tracks("exact")
    worst = max(np.linalg.norm(s["xyz"] - t[2]) for s, t in zip(spec, tracks))
    print(f"worst distance to the true point {worst:.3g}, tracks by length {np.bincount([len(t[0]) for t in tracks]).tolist()}")
    assert all(s["count"] == len(t[0]) and s["mask"].all() and s["error"] < 1e-9 for s, t in zip(spec, tracks))
    assert worst <= um.SPEC_TRUTH_X
    assert um.TOL_X == 4 * max(um.SPEC_TRUTH_X, um.HOST_SPEC_X)
    assert {len(t[0]) for t in tracks} == set(range(2, 13))


def test_noisy_tracks_keep_their_masks_when_the_point_moves_by_the_tolerance():
    """What lets the host build and the kernel be compared mask for mask: on the specification alone, moving X by TOL_X in
    four random directions changes no mask of an accepted noisy track."""
    tracks, spec = spec_tracks("noisy")
    accepted = [i for i, s in enumerate(spec) if s["count"]]
    outliers = sum(int((~s["mask"]).sum()) for s in spec if s["count"])
    print(f"{len(accepted)} of 300 accepted, {outliers} observations outside the masks")
    assert len(accepted) >= 250 and outliers >= 100
    assert all(um.stable_under(tracks[i][0], tracks[i][1], tracks[i][3], um.TOL_X) for i in accepted)


def project(pose, X, K=ue.SCENE_K):
    p = K @ (pose[0] @ X + pose[1])
    return p[:2] / p[2]


def ring_camera(deg, radius=8.0):
    a = np.radians(deg)
    return ua.look_at(np.array([radius * np.sin(a), 0.0, -radius * np.cos(a)]), np.zeros(3))


def test_hand_built_decisions():
    poses = um.arc_cameras()
    X = np.array([0.3, -0.2, 0.5])
    views = [0, 2, 4, 6, 8]
    rows = np.stack([um.camera_row(*poses[v], ue.SCENE_K) for v in views])
    obs = np.array([project(poses[v], X) for v in views])
    # one gross outlier among five
    bad = obs.copy()
    bad[2] += [50.0, -30.0]
    r = um.triangulate_track(bad, rows, 1)
    assert r["mask"].tolist() == [True, True, False, True, True] and r["count"] == 4 and np.linalg.norm(r["xyz"] - X) < 1e-9
    # two views 1.0 degrees apart at the point: below FILTER_MIN_TRI_ANGLE (1.5); 2.0 degrees: accepted
    for deg, accepted in ((1.0, False), (2.0, True)):
        pair = [ring_camera(0.0), ring_camera(deg)]
        r = um.triangulate_track([project(p, np.zeros(3)) for p in pair], [um.camera_row(*p, ue.SCENE_K) for p in pair], 1)
        assert (r["count"] == 2) == accepted, deg
        assert np.isnan(r["xyz"]).all() != accepted and np.isnan(r["error"]) != accepted and r["mask"].all() == accepted
    # a point behind one camera (the camera of view 4 turned round): that observation is out
    flip = np.diag([-1.0, 1.0, -1.0])
    turned = (flip @ poses[4][0], flip @ poses[4][1])
    rows_b = rows.copy()
    rows_b[2] = um.camera_row(*turned, ue.SCENE_K)
    obs_b = obs.copy()
    obs_b[2] = project(turned, X)
    assert (turned[0] @ X + turned[1])[2] < 0
    r = um.triangulate_track(obs_b, rows_b, 1)
    assert r["mask"].tolist() == [True, True, False, True, True] and r["count"] == 4
    # both views at one centre
    a = ring_camera(0.0)
    b = (ua.rodrigues(np.array([0.0, 0.02, 0.0])) @ a[0], ua.rodrigues(np.array([0.0, 0.02, 0.0])) @ a[1])
    r = um.triangulate_track([project(a, X), project(b, X)], [um.camera_row(*a, ue.SCENE_K), um.camera_row(*b, ue.SCENE_K)], 1)
    assert r["count"] == 0 and np.isnan(r["xyz"]).all() and not r["mask"].any()
    # a NaN camera row, a slot out of range, a NaN pixel: each unusable
    cams = np.stack([um.camera_row(*poses[v], ue.SCENE_K) for v in range(12)])
    slots, offsets = np.array(views, np.int32), np.array([0, 5], np.int32)
    for what in ("row", "slot", "slot_negative", "pixel"):
        c, s, o = cams.copy(), slots.copy(), obs.copy()
        if what == "row":
            c[views[1], 4] = np.nan
        elif what == "slot":
            s[1] = 12
        elif what == "slot_negative":
            s[1] = -1
        else:
            o[1, 0] = np.nan
        xyz, mask, count, error = um.triangulate_tracks(o, s, offsets, c, [1])
        assert mask.tolist() == [True, False, True, True, True] and count[0] == 4 and np.linalg.norm(xyz[0] - X) < 1e-9, what
        xyz, mask, count, error = um.triangulate_tracks(o[:2], s[:2], [0, 2], c, [1])            # one usable observation left
        assert count[0] == 0 and not mask.any() and np.isnan(xyz).all() and np.isnan(error).all(), what
    # n = 0 and n = 1
    for n in (0, 1):
        r = um.triangulate_track(obs[:n], rows[:n], 1)
        assert r["count"] == 0 and r["mask"].shape == (n,) and not r["mask"].any() and np.isnan(r["xyz"]).all() and np.isnan(r["error"])


def test_hypotheses_all_pairs_up_to_eleven_observations_then_the_published_hash():
    assert um.hypothesis_pairs(0, 5) == [] and um.hypothesis_pairs(1, 5) == []
    assert um.hypothesis_pairs(3, 5) == [(0, 1), (0, 2), (1, 2)]
    assert len(um.hypothesis_pairs(11, 5)) == 55 and um.hypothesis_pairs(11, 5) == um.hypothesis_pairs(11, 6)
    # n = 12: 66 pairs, the sampler.  The pairs of seed 777, listed
    assert um.hypothesis_pairs(12, 777) == [
        (9, 10), (0, 9), (2, 5), (7, 9), (7, 10), (4, 5), (0, 10), (5, 10), (2, 11), (5, 6), (5, 7), (8, 10), (0, 9), (0, 3), (1, 11),
        (2, 10), (1, 10), (1, 6), (6, 11), (1, 8), (0, 4), (6, 10), (8, 9), (6, 8), (1, 8), (6, 11), (2, 4), (1, 2), (9, 10), (5, 9),
        (0, 10), (8, 9), (3, 8), (6, 9), (5, 6), (0, 2), (5, 7), (2, 7), (0, 7), (4, 9), (1, 11), (1, 7), (1, 11), (1, 5), (4, 5),
        (8, 9), (6, 10), (1, 10), (6, 11), (1, 5), (9, 10), (2, 6), (2, 9), (6, 7), (4, 5), (6, 9), (6, 7), (5, 8), (1, 9), (8, 11),
        (10, 11), (3, 5), (1, 4), (9, 10)]
    assert um.hypothesis_pairs(12, 777) != um.hypothesis_pairs(12, 778)
    from vit_colmap_amd.matching._common import SALT, _lowbias32

    assert SALT["T"] == um.SALT_T and len(set(SALT.values())) == len(SALT)
    import torch

    from oracle import two_view_oracle as tv

    x = torch.tensor([0, 1, 777, 0xFFFFFFFF, 0x9E3779B1], dtype=torch.int64)                      # one hash, three statements
    assert _lowbias32(x).tolist() == [um.lowbias32(int(v)) for v in x] == tv.lowbias32(x.numpy()).tolist()


# ---- the kernel's per-track function on the host -------------------------------------------------------------------------------------
def write_tracks_file(path, obs_xy, obs_cam, offsets, cams, seeds, max_error=um.MAX_ERROR, tan2=um.MIN_TRI_ANGLE_TAN2):
    """The input of tools/triangulate_host.cpp."""
    obs_xy, cams = np.ascontiguousarray(obs_xy, np.float64).reshape(-1, 2), np.ascontiguousarray(cams, np.float64).reshape(-1, 16)
    with open(path, "wb") as f:
        f.write(np.array([len(offsets) - 1, len(cams), len(obs_xy)], np.int32).tobytes())
        f.write(np.array([max_error, tan2], np.float64).tobytes())
        for a in (offsets, np.asarray(seeds, np.int64).astype(np.uint32).view(np.int32), obs_cam):
            f.write(np.ascontiguousarray(a, np.int32).tobytes())
        f.write(obs_xy.tobytes())
        f.write(cams.tobytes())


def read_points_file(path, n_tracks, total):
    raw = open(path, "rb").read()
    assert len(raw) == 36 * n_tracks + total
    xyz = np.frombuffer(raw, np.float64, 3 * n_tracks).reshape(n_tracks, 3)
    error = np.frombuffer(raw, np.float64, n_tracks, 24 * n_tracks)
    count = np.frombuffer(raw, np.int32, n_tracks, 32 * n_tracks)
    return xyz, np.frombuffer(raw, np.uint8, total, 36 * n_tracks).astype(bool), count, error


def run_host(program, tmp_path, obs_xy, obs_cam, offsets, cams, seeds, **kw):
    write_tracks_file(tmp_path / "tracks.bin", obs_xy, obs_cam, offsets, cams, seeds, **kw)
    done = subprocess.run([program, str(tmp_path / "tracks.bin"), str(tmp_path / "points.bin")], stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, text=True)
    assert done.returncode == 0, done.stderr
    return read_points_file(tmp_path / "points.bin", len(offsets) - 1, len(np.asarray(obs_xy).reshape(-1, 2))), done.stderr


def as_one_call(tracks):
    """Tracks (obs, rows, ...) with a camera row per observation -> the arrays of one call."""
    obs, rows = np.concatenate([t[0] for t in tracks]), np.concatenate([t[1] for t in tracks])
    offsets = np.concatenate([[0], np.cumsum([len(t[0]) for t in tracks])]).astype(np.int32)
    return obs, np.arange(len(obs), dtype=np.int32), offsets, rows, [t[3] for t in tracks]


_BUILT = {}


def _build(out, extra):
    proc = subprocess.run(HOST_BUILD + extra + ["-o", str(out), SOURCE], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert proc.returncode == 0, f"{out.name} does not build:\n{proc.stdout}"
    return str(out)


@pytest.fixture(scope="session")
def triangulate_host(tmp_path_factory):
    """tools/triangulate_host.cpp built with the line its source gives (once per session, test_mapper_gpu.py shares it)."""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc to build the host program with")
    if "plain" not in _BUILT:
        _BUILT["plain"] = _build(tmp_path_factory.mktemp("triangulate_host") / "triangulate_host", [])
    return _BUILT["plain"]


def test_host_build_matches_the_spec_on_the_exact_and_the_noisy_tracks(triangulate_host, tmp_path):
    worst = {}
    for kind in ("exact", "noisy"):
        tracks, spec = spec_tracks(kind)
        call = as_one_call(tracks)
        (xyz, mask, count, error), _ = run_host(triangulate_host, tmp_path, *call)
        offsets = call[2]
        for i, s in enumerate(spec):
            assert count[i] == s["count"] and np.array_equal(mask[offsets[i]:offsets[i + 1]], s["mask"]), (kind, i)
            assert np.isnan(xyz[i]).all() == (s["count"] == 0) and np.isnan(error[i]) == (s["count"] == 0), (kind, i)
        ok = count > 0
        worst[kind] = float(np.linalg.norm(xyz[ok] - np.stack([s["xyz"] for s in spec])[ok], axis=1).max())
        worst_error = float(np.abs(error[ok] - np.array([s["error"] for s in spec])[ok]).max())
        print(f"{kind}: {int(ok.sum())} accepted, worst |X_host - X_spec| {worst[kind]:.3g}, worst error difference {worst_error:.3g} px")
    assert max(worst.values()) <= um.HOST_SPEC_X


def test_host_build_under_the_sanitizers_reports_nothing(tmp_path):
    """The same program with the host half built -fsanitize=address,undefined, run on its own over both sets of tracks, the
    degenerate ones of the GPU test included in the call."""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc to build the host program with")
    program = _build(tmp_path / "triangulate_host_san", ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                                                         "-Xarch_host", "-g"])
    for kind in ("exact", "noisy"):
        tracks, spec = spec_tracks(kind)
        obs, slots, offsets, rows, seeds = as_one_call(tracks)
        slots = slots.copy()
        slots[0], slots[-1] = -1, len(rows)                      # a slot out of range at either end
        rows = rows.copy()
        rows[5] = np.nan
        offsets = np.concatenate([offsets, [offsets[-1], offsets[-1]]]).astype(np.int32)          # two empty tracks
        (xyz, mask, count, error), stderr = run_host(program, tmp_path, obs, slots, offsets, rows, list(seeds) + [1, 2])
        assert stderr == "" and count[-1] == 0 and count[-2] == 0 and not mask[0] and not mask[-1]
        assert (count[1:300] > 0).sum() >= 250


# ---- the growth rule -------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def windowed():
    scene = um.windowed_scene()
    pairs = truth_pairs(scene)
    images = scene_images(scene)
    return scene, pairs, ua.seed_model(images, pairs), um.grow_model(images, pairs)


def test_growth_registers_all_twelve_images_where_the_seed_model_registers_seven():
    scene, pairs, seed, grown = windowed()
    assert len(seed["poses"]) < 12                                   # what makes the scene: the seed model alone loses images
    assert seed["initial_pair"] == (8, 10) and sorted(seed["poses"]) == [6, 7, 8, 9, 10, 11, 12] and len(seed["xyz"]) == 213
    assert sorted(grown["poses"]) == list(range(1, 13)) and grown["registration_rounds"] >= 2
    assert grown["initial_pair"] == seed["initial_pair"] and grown["rounds"] >= grown["registration_rounds"]
    rot, pos = ua.align_errors(grown["poses"], scene, *grown["initial_pair"])
    lengths = [len(t) for t in grown["tracks"]]
    print(f"{len(grown['xyz'])} points, mean track length {np.mean(lengths):.2f}, {grown['rounds']} rounds "
          f"({grown['registration_rounds']} with a registration), worst rotation {rot:.3f} deg, worst centre {pos:.4f} baselines")
    assert rot <= GROW_ROT_BOUND and pos <= GROW_POS_BOUND
    assert len(grown["xyz"]) == len(grown["tracks"]) > 4 * len(seed["xyz"]) and min(lengths) >= 2
    # the seed's points keep their ids and the start of their tracks; every track has one keypoint per image at most and,
    # in this scene, observes one scene point
    for k, track in enumerate(seed["tracks"]):
        assert grown["tracks"][k][:len(track)] == track and np.array_equal(grown["xyz"][k], seed["xyz"][k])
    for track in grown["tracks"]:
        assert len({i for i, _ in track}) == len(track) and len({kp for _, kp in track}) == 1
    # new point ids ascend in their track's first node, round by round: deterministic
    again = um.grow_model(scene_images(scene), pairs)
    assert again["tracks"] == grown["tracks"] and np.array_equal(again["xyz"], grown["xyz"])


def test_growth_decisions_survive_a_pose_perturbation_of_the_registration_tolerance():
    """What the GPU end-to-end test may differ by in points: the accept / reject decisions of the T-steps that change when
    every registered pose is moved by TOL_POSE in a random direction before a triangulation call."""
    scene, pairs, _, grown = windowed()
    rs = np.random.RandomState(3)
    changed, tried = [0], [0]

    def both(obs_xy, obs_cam, offsets, cams, seeds):
        out = um.triangulate_tracks(obs_xy, obs_cam, offsets, cams, seeds)
        moved = cams.copy()
        d = rs.normal(size=(len(cams), 12))
        moved[:, :12] += ua.TOL_POSE * d / np.linalg.norm(d, axis=1, keepdims=True)
        other = um.triangulate_tracks(obs_xy, obs_cam, offsets, moved, seeds)
        changed[0] += int(((out[2] > 0) != (other[2] > 0)).sum())
        tried[0] += len(seeds)
        return out

    again = um.grow_model(scene_images(scene), pairs, triangulate=both)
    print(f"{changed[0]} of {tried[0]} decisions changed")
    assert again["tracks"] == grown["tracks"]
    assert changed[0] + 1 <= um.GROW_POINT_MARGIN


# ---- the product's host logic with the specification in the three GPU seams ---------------------------------------------------------------
def spec_triangulate(obs_xy, obs_cam, offsets, cams, seeds, device):
    return um.triangulate_tracks(obs_xy, obs_cam, offsets, cams, seeds)


def build_with_spec(path, build_sparse_model=None):
    if build_sparse_model is None:
        from vit_colmap_amd.mapping.grow import build_sparse_model

    return build_sparse_model(path, device="cpu", two_view_pose_fn=spec_two_view_pose, estimate_fn=spec_estimate,
                              triangulate_fn=spec_triangulate)


def assert_grown_model_follows(model, spec, atol):
    assert model.initial_pair in (spec["initial_pair"], None)
    assert sorted(model.images) == sorted(spec["poses"]) and sorted(model.points3D) == list(range(1, len(spec["xyz"]) + 1))
    for i, (R, t) in spec["poses"].items():
        assert np.allclose(ua.quat_to_rot(model.images[i]["qvec"]), R, atol=atol) and np.allclose(model.images[i]["tvec"], t, atol=atol)
    for k, (xyz, track) in enumerate(zip(spec["xyz"], spec["tracks"])):
        p = model.points3D[k + 1]
        assert np.allclose(p["xyz"], xyz, atol=atol) and p["track"] == track and p["rgb"] == (0, 0, 0)


def test_build_sparse_model_with_the_spec_in_its_seams_equals_grow_model(tmp_path):
    from vit_colmap_amd.mapping.seed import SparseModel, build_seed_model

    scene, pairs, seed, grown = windowed()
    write_scene_db(tmp_path / "w.db", scene, pairs)
    model = build_with_spec(tmp_path / "w.db")
    assert model.initial_pair == grown["initial_pair"] and model.rounds == grown["rounds"]
    assert_grown_model_follows(model, grown, 1e-12)
    for pid, p in model.points3D.items():
        assert 0 <= p["error"] < 12.0
        for i, kp in p["track"]:
            assert model.images[i]["point3D_ids"][kp] == pid
    assert sum(int((im["point3D_ids"] >= 0).sum()) for im in model.images.values()) == sum(len(t) for t in grown["tracks"])
    s = model.stats()
    assert s == dict(initial_pair=[8, 10], registered_images=12, num_points3D=len(grown["xyz"]), rounds=grown["rounds"],
                     mean_track_length=pytest.approx(np.mean([len(t) for t in grown["tracks"]])))
    model.write_text(tmp_path / "grown")
    back = SparseModel.read_text(tmp_path / "grown")
    assert back == model and model == back
    assert_grown_model_follows(back, grown, 1e-12)
    # the seed model of the same database is what it was: fewer images, no `rounds` among its statistics
    seed_model = build_seed_model(tmp_path / "w.db", device="cpu", two_view_pose_fn=spec_two_view_pose, estimate_fn=spec_estimate)
    assert sorted(seed_model.images) == sorted(seed["poses"]) and "rounds" not in seed_model.stats()
    for pid, p in seed_model.points3D.items():
        assert np.array_equal(model.points3D[pid]["xyz"], p["xyz"]) and model.points3D[pid]["track"][:len(p["track"])] == p["track"]
    # the seed model's errors propagate unchanged
    write_scene_db(tmp_path / "noflag.db", scene, pairs, flag=False)
    with pytest.raises(ValueError, match="focal-length priors"):
        build_with_spec(tmp_path / "noflag.db")


def test_inconsistent_tracks_and_planar_rows(tmp_path):
    """A component with two keypoints in one image takes no part in growth; PLANAR rows carry edges, UNCALIBRATED ones none."""
    from oracle import two_view_oracle as tv

    scene, pairs, _seed, grown = windowed()
    images = scene_images(scene)
    comps = um.components(images, pairs)
    assert all(len({i for i, _ in c}) == len(c) for c in comps)
    pairs2 = {k: dict(g) for k, g in pairs.items()}
    g = pairs2[(1, 2)]
    m = g["inlier_matches"].copy()
    m[0, 1] = m[1, 1]                                                 # keypoints m[0, 0] and m[1, 0] of image 1 meet in image 2
    g["inlier_matches"] = m
    broken = [c for c in um.components(images, pairs2) if len({i for i, _ in c}) != len(c)]
    assert len(broken) == 1 and (1, int(m[0, 0])) in broken[0] and (1, int(m[1, 0])) in broken[0]
    model2 = um.grow_model(images, pairs2)
    assert not any(set(broken[0]) & set(t) for t in model2["tracks"][len(_seed["xyz"]):])
    pairs3 = {k: dict(g, config=tv.CONFIG_PLANAR if k == (1, 2) else tv.CONFIG_UNCALIBRATED if k == (1, 3) else g["config"])
              for k, g in pairs.items()}
    c3 = um.components(images, pairs3)
    edges = {frozenset([(1, int(a)), (2, int(b))]) for a, b in pairs[(1, 2)]["inlier_matches"]}
    assert all(any(e <= set(c) for c in c3) for e in list(edges)[:20])
    write_scene_db(tmp_path / "p.db", scene, pairs3)
    assert_grown_model_follows(build_with_spec(tmp_path / "p.db"), um.grow_model(images, read_pairs(tmp_path / "p.db")), 1e-12)


# ---- the pipeline flag ------------------------------------------------------------------------------------------------------------------
def test_sparse_model_flag_is_off_by_default_and_checked_before_any_work(tmp_path, monkeypatch):
    import argparse

    from vit_colmap_amd.pipeline import run_pipeline as rp
    from vit_colmap_amd.utils.config import Config, ReconstructionConfig

    assert ReconstructionConfig().sparse_model is False and Config().reconstruction.sparse_model is False
    assert Config.from_args(argparse.Namespace(sparse_model=True)).reconstruction.sparse_model is True
    assert Config.from_args(argparse.Namespace(sparse_model=True)).reconstruction.seed_model is False
    assert Config.from_args(argparse.Namespace()).reconstruction.sparse_model is False

    def no_extractor(self):
        raise AssertionError("the extractor was built before the flags were checked")

    monkeypatch.setattr(rp.Pipeline, "_make_extractor", no_extractor)
    for missing, setup in (("prior_focal_length", lambda c: setattr(c.matching, "compute_relative_pose", True)),
                           ("compute_relative_pose", lambda c: setattr(c.camera, "prior_focal_length", True)),
                           ("do_matching", lambda c: (setattr(c.camera, "prior_focal_length", True),
                                                      setattr(c.matching, "compute_relative_pose", True), setattr(c, "do_matching", False)))):
        cfg = Config()
        cfg.reconstruction.sparse_model = True
        cfg.do_reconstruction = False
        setup(cfg)
        with pytest.raises(ValueError, match="sparse_model needs .*" + missing):
            rp.Pipeline(cfg).run(tmp_path / "images", tmp_path / "out", tmp_path / "x.db")
    assert not (tmp_path / "out" / "sparse").exists()
    seen = []
    monkeypatch.setattr(rp.Pipeline, "run", lambda self, *a, **k: seen.append((self.config.reconstruction.seed_model,
                                                                               self.config.reconstruction.sparse_model)))
    for extra in ([], ["--sparse-model"], ["--seed-model", "--sparse-model"]):
        monkeypatch.setattr(sys, "argv", ["prog", "--images", "i", "--output", "o", "--db", "d"] + extra)
        rp.main()
    assert seen == [(False, False), (False, True), (True, True)]
    # the pipeline module itself imports nothing of the mapping package, and the package does not import the growth with it
    src = open(rp.__file__).read()
    assert "mapping" not in [ln.split()[1] for ln in src.splitlines() if ln.startswith(("from ", "import "))]
    code = ("import sys; import vit_colmap_amd.mapping; import vit_colmap_amd.pipeline.run_pipeline; "
            "assert 'vit_colmap_amd.mapping.grow' not in sys.modules and 'vit_colmap_amd.mapping.triangulate' not in sys.modules")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


def test_pipeline_writes_the_grown_model_and_survives_a_scene_without_one(tmp_path, monkeypatch):
    import vit_colmap_amd.mapping.grow as grow
    from vit_colmap_amd.mapping.seed import SparseModel
    from vit_colmap_amd.pipeline import run_pipeline as rp
    from vit_colmap_amd.utils.config import Config

    scene, pairs, _, grown = windowed()
    write_scene_db(tmp_path / "w.db", scene, pairs)
    real = grow.build_sparse_model
    monkeypatch.setattr(grow, "build_sparse_model", lambda path, device="cuda": build_with_spec(path, real))
    p = rp.Pipeline(Config())
    p.last_stats = {"verified_pairs": 10}
    p._write_sparse_model(tmp_path / "w.db", tmp_path / "out", "cpu")
    assert p.last_stats["verified_pairs"] == 10 and "seed_model" not in p.last_stats
    assert p.last_stats["sparse_model"]["registered_images"] == 12 and p.last_stats["sparse_model"]["rounds"] == grown["rounds"]
    assert sorted(f.name for f in (tmp_path / "out" / "sparse" / "grown").iterdir()) == ["cameras.txt", "images.txt", "points3D.txt"]
    assert not (tmp_path / "out" / "sparse" / "seed").exists()
    assert_grown_model_follows(SparseModel.read_text(tmp_path / "out" / "sparse" / "grown"), grown, 1e-12)
    dup = ua.arc_scene(duplicate=True, n_views=2)
    write_scene_db(tmp_path / "dup.db", dup, truth_pairs(dup))
    p2 = rp.Pipeline(Config())
    warned = []
    monkeypatch.setattr(rp.logger, "warning", lambda msg, *a: warned.append(msg % a))
    p2._write_sparse_model(tmp_path / "dup.db", tmp_path / "out2", "cpu")
    assert "sparse_model" not in (p2.last_stats or {}) and not (tmp_path / "out2").exists()
    assert len(warned) == 1 and "no sparse model written" in warned[0] and "no CALIBRATED pair" in warned[0]
