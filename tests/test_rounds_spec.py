"""CPU tests of the adjustment per growth round: the numpy specification of tests/util_rounds.py (one
track re-evaluated, the rounds), the kernel's per-track routine compiled for the host (tools/refine_tracks_host.cpp) against
it, plain and under the host sanitizers, the 24-view scene that one adjustment at the end does not recover, the product's
host logic with the specification in its seams, and the pipeline's flag.  No GPU."""
import argparse
import os
import shutil
import subprocess
import sys
from functools import lru_cache

import numpy as np
import pytest

import util_absolute_pose as ua
import util_bundle as ub
import util_essential as ue
import util_mapper as um
import util_rounds as ur
from test_absolute_pose_spec import scene_images, spec_estimate, spec_two_view_pose, truth_pairs, write_scene_db
from test_bundle_spec import spec_bundle
from test_mapper_spec import spec_triangulate, spec_tracks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
HOST_BUILD = [HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off"]
SOURCE = os.path.join(ROOT, "tools", "refine_tracks_host.cpp")


# ---- the kernel's per-track routine on the host ---------------------------------------------------------------------------------------
def write_tracks_file(path, obs_xy, obs_cam, offsets, cams, init_xyz, max_error=um.MAX_ERROR, tan2=um.MIN_TRI_ANGLE_TAN2):
    """The input of tools/refine_tracks_host.cpp."""
    obs_xy, cams = np.ascontiguousarray(obs_xy, np.float64).reshape(-1, 2), np.ascontiguousarray(cams, np.float64).reshape(-1, 16)
    with open(path, "wb") as f:
        f.write(np.array([len(offsets) - 1, len(cams), len(obs_xy)], np.int32).tobytes())
        f.write(np.array([max_error, tan2], np.float64).tobytes())
        f.write(np.ascontiguousarray(offsets, np.int32).tobytes())
        f.write(np.ascontiguousarray(init_xyz, np.float64).tobytes())
        f.write(np.ascontiguousarray(obs_cam, np.int32).tobytes())
        f.write(obs_xy.tobytes())
        f.write(cams.tobytes())


def run_refine_host(program, tmp_path, obs_xy, obs_cam, offsets, cams, init_xyz, **kw):
    """-> (xyz, mask, count, error), the output file's bytes, stderr."""
    n_tracks, total = len(offsets) - 1, len(np.asarray(obs_xy).reshape(-1, 2))
    write_tracks_file(tmp_path / "refine_in.bin", obs_xy, obs_cam, offsets, cams, init_xyz, **kw)
    done = subprocess.run([program, str(tmp_path / "refine_in.bin"), str(tmp_path / "refine_out.bin")], stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, text=True)
    assert done.returncode == 0, done.stderr
    raw = open(tmp_path / "refine_out.bin", "rb").read()
    assert len(raw) == 36 * n_tracks + total
    xyz = np.frombuffer(raw, np.float64, 3 * n_tracks).reshape(n_tracks, 3)
    error = np.frombuffer(raw, np.float64, n_tracks, 24 * n_tracks)
    count = np.frombuffer(raw, np.int32, n_tracks, 32 * n_tracks)
    return (xyz, np.frombuffer(raw, np.uint8, total, 36 * n_tracks).astype(bool), count, error), raw, done.stderr


_BUILT = {}


def _build(out, extra):
    proc = subprocess.run(HOST_BUILD + extra + ["-o", str(out), SOURCE], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert proc.returncode == 0, f"{out.name} does not build:\n{proc.stdout}"
    return str(out)


@pytest.fixture(scope="session")
def refine_host(tmp_path_factory):
    """tools/refine_tracks_host.cpp built with the line its source gives (once per session, test_rounds_gpu.py shares it)."""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc to build the host program with")
    if "plain" not in _BUILT:
        _BUILT["plain"] = _build(tmp_path_factory.mktemp("refine_tracks_host") / "refine_tracks_host", [])
    return _BUILT["plain"]


@lru_cache(maxsize=None)
def start_call(kind, start):
    """The 300 tracks of a kind as one call, each started from the specification's triangulated X (`start` "own") or from that
    X moved by START_OFFSET ("moved"); a track the triangulation rejects starts from its NaN -> the call's arrays, the
    specification's triangulation, the specification's refinement."""
    tracks, tri = spec_tracks(kind)
    init = np.stack([s["xyz"] if start == "own" else ur.moved(s["xyz"], i) for i, s in enumerate(tri)])
    obs, rows = np.concatenate([t[0] for t in tracks]), np.concatenate([t[1] for t in tracks])
    offsets = np.concatenate([[0], np.cumsum([len(t[0]) for t in tracks])]).astype(np.int32)
    spec = [ur.refine_track(t[0], t[1], x) for t, x in zip(tracks, init)]
    return (obs, np.arange(len(obs), dtype=np.int32), offsets, rows, init), tri, spec


def test_host_build_matches_the_spec_from_the_triangulated_point_and_from_a_moved_one(refine_host, tmp_path):
    worst = {}
    for kind in ("exact", "noisy"):
        for start in ("own", "moved"):
            call, tri, spec = start_call(kind, start)
            (xyz, mask, count, error), _, _ = run_refine_host(refine_host, tmp_path, *call)
            offsets = call[2]
            for i, s in enumerate(spec):
                assert count[i] == s["count"] and np.array_equal(mask[offsets[i]:offsets[i + 1]], s["mask"]), (kind, start, i)
                assert np.isnan(xyz[i]).all() == (s["count"] == 0) and np.isnan(error[i]) == (s["count"] == 0), (kind, start, i)
                if start == "own":      # from the triangulator's own output: the triangulator's mask and count
                    assert count[i] == tri[i]["count"] and np.array_equal(s["mask"], tri[i]["mask"]), (kind, i)
            ok = count > 0
            worst[kind, start] = float(np.linalg.norm(xyz[ok] - np.stack([s["xyz"] for s in spec])[ok], axis=1).max())
            worst_error = float(np.abs(error[ok] - np.array([s["error"] for s in spec])[ok]).max())
            print(f"{kind}, {start}: {int(ok.sum())} accepted ({sum(t['count'] > 0 for t in tri)} triangulated), worst |X_host - X_spec| "
                  f"{worst[kind, start]:.3g}, worst error difference {worst_error:.3g} px")
            # the moved start is a start, not a rejection: nine in ten of the triangulated tracks survive it
            assert ok.sum() >= 0.9 * sum(t["count"] > 0 for t in tri)
    assert max(worst.values()) <= ur.HOST_SPEC_REFINE_X
    assert ur.TOL_REFINE_X == 4 * ur.HOST_SPEC_REFINE_X


def project(row, X):
    p = ue.SCENE_K @ (row[:9].reshape(3, 3) @ X + row[9:12])
    return p[:2] / p[2]


@lru_cache(maxsize=None)
def edge_call():
    """One call of the cases a build can get wrong -> names, obs_xy, obs_cam, offsets, cams, init_xyz."""
    poses = um.arc_cameras()
    cams = np.stack([um.camera_row(*p, ue.SCENE_K) for p in poses] + [np.full(16, np.nan)])       # slot 12: not registered
    flip = np.diag([-1.0, 1.0, -1.0])
    turned = um.camera_row(flip @ poses[4][0], flip @ poses[4][1], ue.SCENE_K)                    # view 4 turned round
    cams = np.concatenate([cams, turned[None]])                                                   # slot 13
    X = np.array([0.3, -0.2, 0.5])
    rs = np.random.RandomState(5)
    names, obs, slots, init = [], [], [], []

    def add(name, views, x0, pixels=None):
        names.append(name), slots.append(np.array(views, np.int32)), init.append(np.asarray(x0, np.float64))
        rows = cams[np.clip(views, 0, len(cams) - 1)] if len(views) else np.zeros((0, 16))
        with np.errstate(all="ignore"):
            o = np.array([project(r, X) for r in rows]).reshape(-1, 2)
        obs.append(o if pixels is None else pixels(o))

    five = [0, 2, 4, 6, 8]
    add("plain", five, X + 0.01)
    add("nan_init", five, [np.nan, X[1], X[2]])
    add("inf_init", five, [X[0], np.inf, X[2]])

    def one_inlier(o):                      # every pixel but the first 40 px off: X0 has one inlier
        o = o.copy()
        o[1:] += 40.0
        return o

    add("one_inlier", five, X, one_inlier)
    add("behind", [0, 2, 13, 6, 8], X)                                  # X is behind the turned camera: that observation is out
    add("all_behind", [13, 13], X)
    add("slot_negative_first", [-1, 2, 4, 6, 8], X)
    add("slot_past_last", [0, 2, 4, 6, 14], X)
    add("nan_camera", [0, 12, 4, 6, 8], X)

    def nan_pixel(o):
        o = o.copy()
        o[2, 1] = np.nan
        return o

    add("nan_pixel", five, X, nan_pixel)
    add("length_0", [], X)
    add("length_1", [3], X)
    add("length_2", [1, 9], X + 0.002)
    add("length_2_far", [1, 9], X + 1.0)                                # a start no observation agrees with
    add("length_70", list(rs.randint(0, 12, 70)), X + 0.02, lambda o: o + rs.normal(0, 0.5, o.shape))
    add("picks_up", five, X + 0.05)                                     # some 30 px off: fewer inliers at the start than at the end
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in slots])]).astype(np.int32)
    return names, np.concatenate(obs), np.concatenate(slots), offsets, cams, np.stack(init)


def assert_edge_decisions(names, offsets, mask, count, xyz, error):
    by = {n: k for k, n in enumerate(names)}

    def m(name):
        return mask[offsets[by[name]]:offsets[by[name] + 1]].tolist()

    for name in ("nan_init", "inf_init", "one_inlier", "all_behind", "length_0", "length_1", "length_2_far"):
        k = by[name]
        assert count[k] == 0 and not any(m(name)) and np.isnan(xyz[k]).all() and np.isnan(error[k]), name
    assert count[by["plain"]] == 5 and count[by["length_2"]] == 2 and count[by["length_70"]] >= 60
    assert m("behind") == [True, True, False, True, True] and m("slot_negative_first") == [False, True, True, True, True]
    assert m("slot_past_last") == [True, True, True, True, False] and m("nan_camera") == [True, False, True, True, True]
    assert m("nan_pixel") == [True, True, False, True, True]
    X = np.array([0.3, -0.2, 0.5])
    for name in ("plain", "behind", "slot_negative_first", "slot_past_last", "nan_camera", "nan_pixel", "length_2"):
        assert np.linalg.norm(xyz[by[name]] - X) < 1e-9, name


def test_edge_cases_in_one_call(refine_host, tmp_path):
    names, obs_xy, obs_cam, offsets, cams, init = edge_call()
    spec = ur.refine_tracks(obs_xy, obs_cam, offsets, cams, init)
    assert_edge_decisions(names, offsets, spec[1], spec[2], spec[0], spec[3])
    (xyz, mask, count, error), _, _ = run_refine_host(refine_host, tmp_path, obs_xy, obs_cam, offsets, cams, init)
    assert np.array_equal(count, spec[2]) and np.array_equal(mask, spec[1])
    ok = count > 0
    assert np.isnan(xyz[~ok]).all() and np.isnan(error[~ok]).all()
    assert np.linalg.norm(xyz[ok] - spec[0][ok], axis=1).max() <= ur.TOL_REFINE_X


def test_host_build_under_the_sanitizers_reports_nothing(tmp_path):
    """The same program with the host half built -fsanitize=address,undefined, run on its own over the four calls and the edge
    cases."""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc to build the host program with")
    program = _build(tmp_path / "refine_tracks_host_san", ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                                                           "-fno-sanitize-recover=all", "-Xarch_host", "-g"])
    for kind in ("exact", "noisy"):
        for start in ("own", "moved"):
            call, _, spec = start_call(kind, start)
            (xyz, mask, count, error), _, stderr = run_refine_host(program, tmp_path, *call)
            assert stderr == "" and np.array_equal(count, [s["count"] for s in spec])
    names, *call = edge_call()
    (xyz, mask, count, error), _, stderr = run_refine_host(program, tmp_path, *call)
    assert stderr == ""
    assert_edge_decisions(names, call[2], mask, count, xyz, error)


# ---- the rounds -------------------------------------------------------------------------------------------------------------------------
def drift(model, scene):
    """(worst rotation in degrees, worst centre in baselines) of a model's poses, its initial pair's baseline scaled to 1."""
    return ua.align_errors(ur.unit_baseline_poses(model), scene, *model["initial_pair"])


@lru_cache(maxsize=None)
def long_scene():
    scene = um.windowed_scene(n_views=24, n_points=2400, noise=1.0)
    return scene, truth_pairs(scene)


@lru_cache(maxsize=None)
def long_mapped():
    scene, pairs = long_scene()
    return ur.map_model(scene_images(scene), pairs)


def test_rounds_recover_the_24_view_scene_that_one_adjustment_does_not():
    """Fails without the feature: one adjustment at the end of the growth leaves the 24-view scene 15 degrees off."""
    scene, pairs = long_scene()
    images = scene_images(scene)
    once = ub.adjust_model(images, um.grow_model(images, pairs))
    once_rot, once_pos = drift(once, scene)
    mapped = long_mapped()
    rot, pos = drift(mapped, scene)
    print(f"adjusted once: {once_rot:.4g} deg / {once_pos:.4g} baselines after {once['report']['iterations']} linearisations; adjusted "
          f"per round: {rot:.4g} deg / {pos:.4g} in {mapped['rounds']} rounds, {len(mapped['poses'])} images, {len(mapped['xyz'])} points, "
          f"{sum(len(t) for t in mapped['tracks'])} observations")
    assert once_rot > 5.0                                           # the scene needs the feature
    assert once_rot == pytest.approx(ur.LONG_ONCE_ROT, rel=1e-3) and once_pos == pytest.approx(ur.LONG_ONCE_POS, rel=1e-3)
    assert sorted(mapped["poses"]) == list(range(1, 25))
    assert rot <= once_rot / 4 and pos <= once_pos / 4
    assert rot <= ur.LONG_ROT_BOUND and pos <= ur.LONG_POS_BOUND
    assert len(mapped["xyz"]) == ur.LONG_POINTS and len(mapped["round_reports"]) == mapped["rounds"]
    for r in mapped["round_reports"]:
        assert r["final_cost"] < r["initial_cost"] and r["iterations"] < ub.BA_MAX_ITERATIONS
    assert all(len(t) >= 2 and len(set(t)) == len(t) for t in mapped["tracks"]) and mapped["point_ids"] == sorted(set(mapped["point_ids"]))


def test_the_e_step_drops_and_picks_up_observations_on_a_scene_with_displaced_keypoints():
    scene = ur.displaced_scene(um.windowed_scene(n_views=24, n_points=2400, noise=0.5))
    images = scene_images(scene)
    m = ur.map_model(images, truth_pairs(scene))
    added, dropped, points = (sum(r[k] for r in m["round_reports"]) for k in ("added_observations", "dropped_observations", "dropped_points"))
    worst = 0.0
    for X, track in zip(m["xyz"], m["tracks"]):
        assert len(track) >= 2
        for i, kp in track:
            worst = max(worst, float(np.linalg.norm(project(um.camera_row(*m["poses"][i], scene["K"]), X) - images[i]["keypoints"][kp, :2])))
    print(f"{added} observations added, {dropped} dropped, {points} points dropped, {len(m['xyz'])} points, worst observation {worst:.4f} px, "
          f"drift {drift(m, scene)}")
    assert added > 0 and dropped > 0
    assert sorted(m["poses"]) == list(range(1, 25))
    assert worst <= ur.MAX_ERROR
    assert len(set(m["point_ids"])) == len(m["point_ids"]) == len(m["xyz"])


# ---- the product's host logic with the specification in its seams ---------------------------------------------------------------------------
def spec_refine(obs_xy, obs_cam, offsets, cams, init_xyz, device):
    return ur.refine_tracks(obs_xy, obs_cam, offsets, cams, init_xyz)


SEAMS = dict(device="cpu", two_view_pose_fn=spec_two_view_pose, estimate_fn=spec_estimate, triangulate_fn=spec_triangulate,
             bundle_fn=spec_bundle, refine_fn=spec_refine)


@lru_cache(maxsize=None)
def short_mapped():
    scene = um.windowed_scene()
    pairs = truth_pairs(scene)
    images = scene_images(scene)
    mapped = ur.map_model(images, pairs)
    return scene, pairs, mapped, ur.finish_model(images, mapped)


def assert_mapped_model_follows(model, spec, atol):
    assert sorted(model.images) == sorted(spec["poses"]) and sorted(model.points3D) == spec["point_ids"]
    for i, (R, t) in spec["poses"].items():
        assert np.allclose(ua.quat_to_rot(model.images[i]["qvec"]), R, atol=atol) and np.allclose(model.images[i]["tvec"], t, atol=atol)
    for pid, xyz, track in zip(spec["point_ids"], spec["xyz"], spec["tracks"]):
        p = model.points3D[pid]
        assert np.allclose(p["xyz"], xyz, atol=atol) and p["track"] == [tuple(n) for n in track], pid


def test_build_mapped_model_with_the_spec_in_its_seams_equals_map_model(tmp_path):
    from vit_colmap_amd.mapping.rounds import build_mapped_model, build_mapped_rounds
    from vit_colmap_amd.mapping.seed import SparseModel

    scene, pairs, mapped, done = short_mapped()
    write_scene_db(tmp_path / "w.db", scene, pairs)
    rounds_model, reports = build_mapped_rounds(tmp_path / "w.db", **SEAMS)
    assert rounds_model.rounds == mapped["rounds"] and rounds_model.initial_pair == mapped["initial_pair"]
    assert_mapped_model_follows(rounds_model, mapped, 1e-9)
    model = build_mapped_model(tmp_path / "w.db", **SEAMS)
    assert_mapped_model_follows(model, done, 1e-9)
    keys = ("iterations", "accepted_steps", "decisions", "added_observations", "dropped_observations", "dropped_points")
    assert len(model.round_adjustments) == len(mapped["round_reports"]) == mapped["rounds"]
    for got, want in zip(model.round_adjustments, mapped["round_reports"]):
        assert {k: got[k] for k in keys} == {k: want[k] for k in keys}
        assert got["initial_cost"] == pytest.approx(want["initial_cost"], rel=1e-9) and got["final_cost"] == pytest.approx(want["final_cost"], rel=1e-9)
    s = model.stats()
    assert s["registered_images"] == 12 and s["round_adjustments"] == model.round_adjustments and "bundle_adjustment" in s
    rot, pos = ua.align_errors({i: (ua.quat_to_rot(im["qvec"]), im["tvec"]) for i, im in model.images.items()}, scene, *model.initial_pair)
    print(f"12 views: {len(model.points3D)} points, {len(reports)} round adjustments, drift {rot:.4g} deg / {pos:.4g} baselines")
    model.write_text(tmp_path / "mapped")
    back = SparseModel.read_text(tmp_path / "mapped")
    assert back == model and model == back
    assert_mapped_model_follows(back, done, 1e-9)
    # a model without rounds has no such statistic
    assert "round_adjustments" not in rounds_model.stats() and SparseModel().round_adjustments is None


def test_more_registered_images_than_the_adjustment_holds_is_a_value_error():
    from types import SimpleNamespace

    from vit_colmap_amd import _lib
    from vit_colmap_amd.mapping import rounds

    n = _lib.VC_BA_MAX_CAMS + 1
    g = SimpleNamespace(poses={i: None for i in range(n)}, xyz={})
    with pytest.raises(ValueError, match="VC_BA_MAX_CAMS"):
        rounds._round_steps(g, None, None, {}, [])


# ---- the pipeline flag ------------------------------------------------------------------------------------------------------------------------
def test_adjust_rounds_flag_is_off_by_default_and_checked_before_any_work(tmp_path, monkeypatch):
    from vit_colmap_amd.pipeline import run_pipeline as rp
    from vit_colmap_amd.utils.config import Config, ReconstructionConfig

    assert ReconstructionConfig().adjust_rounds is False and Config().reconstruction.adjust_rounds is False
    assert Config.from_args(argparse.Namespace(adjust_rounds=True)).reconstruction.adjust_rounds is True
    assert Config.from_args(argparse.Namespace(adjust_rounds=True)).reconstruction.bundle_adjustment is False
    assert Config.from_args(argparse.Namespace()).reconstruction.adjust_rounds is False

    def no_extractor(self):
        raise AssertionError("the extractor was built before the flags were checked")

    monkeypatch.setattr(rp.Pipeline, "_make_extractor", no_extractor)
    cfg = Config()
    cfg.reconstruction.adjust_rounds = cfg.reconstruction.sparse_model = True
    cfg.camera.prior_focal_length, cfg.matching.compute_relative_pose, cfg.do_reconstruction = True, True, False
    with pytest.raises(ValueError, match="adjust_rounds needs .*--bundle-adjustment"):
        rp.Pipeline(cfg).run(tmp_path / "images", tmp_path / "out", tmp_path / "x.db")
    assert not (tmp_path / "out" / "sparse").exists()
    seen = []
    monkeypatch.setattr(rp.Pipeline, "run", lambda self, *a, **k: seen.append((self.config.reconstruction.bundle_adjustment,
                                                                               self.config.reconstruction.adjust_rounds)))
    for extra in ([], ["--sparse-model", "--bundle-adjustment"], ["--sparse-model", "--bundle-adjustment", "--adjust-rounds"]):
        monkeypatch.setattr(sys, "argv", ["prog", "--images", "i", "--output", "o", "--db", "d"] + extra)
        rp.main()
    assert seen == [(False, False), (True, False), (True, True)]
    code = ("import sys; import vit_colmap_amd.mapping; import vit_colmap_amd.mapping.bundle; import vit_colmap_amd.pipeline.run_pipeline; "
            "assert 'vit_colmap_amd.mapping.rounds' not in sys.modules")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


def test_pipeline_writes_the_mapped_model_beside_unchanged_grown_and_adjusted_ones(tmp_path, monkeypatch):
    import vit_colmap_amd.mapping
    import vit_colmap_amd.mapping.bundle as bundle
    import vit_colmap_amd.mapping.grow as grow
    from vit_colmap_amd.mapping.seed import SparseModel
    from vit_colmap_amd.pipeline import run_pipeline as rp
    from vit_colmap_amd.utils.config import Config

    scene, pairs, mapped, done = short_mapped()
    write_scene_db(tmp_path / "w.db", scene, pairs)
    grow_seams = {k: v for k, v in SEAMS.items() if k not in ("bundle_fn", "refine_fn")}
    # what the two directories hold today: the two builders called as the pipeline without the flag calls them
    today_grown = grow.build_sparse_model(str(tmp_path / "w.db"), **grow_seams)
    today_grown.write_text(tmp_path / "today" / "sparse" / "grown")
    bundle.build_adjusted_model(str(tmp_path / "w.db"), device="cpu", grown=today_grown, bundle_fn=spec_bundle).write_text(
        tmp_path / "today" / "sparse" / "adjusted")
    real = grow.build_sparse_model
    monkeypatch.setattr(grow, "build_sparse_model", lambda path, device="cuda": real(path, **grow_seams))
    monkeypatch.setattr(bundle, "bundle_adjust", spec_bundle)
    # with the flag off the rounds are not imported (restored afterwards, so that later tests name the same module)
    if hasattr(vit_colmap_amd.mapping, "rounds"):
        monkeypatch.setattr(vit_colmap_amd.mapping, "rounds", vit_colmap_amd.mapping.rounds)
    monkeypatch.delitem(sys.modules, "vit_colmap_amd.mapping.rounds", raising=False)
    off = rp.Pipeline(Config())
    off.last_stats = {"verified_pairs": 10}
    off._write_sparse_model(tmp_path / "w.db", tmp_path / "off", "cpu", adjust=True)
    assert "vit_colmap_amd.mapping.rounds" not in sys.modules
    assert sorted(off.last_stats) == ["bundle_adjustment", "sparse_model", "verified_pairs"]
    assert sorted(f.name for f in (tmp_path / "off" / "sparse").iterdir()) == ["adjusted", "grown"]

    import vit_colmap_amd.mapping.rounds as rounds

    real_mapped = rounds.build_mapped_model
    monkeypatch.setattr(rounds, "build_mapped_model", lambda path, device="cuda", **kw: real_mapped(path, **SEAMS, **kw))
    on = rp.Pipeline(Config())
    on.last_stats = {"verified_pairs": 10}
    on._write_sparse_model(tmp_path / "w.db", tmp_path / "on", "cpu", adjust=True, adjust_rounds=True)
    assert sorted(f.name for f in (tmp_path / "on" / "sparse").iterdir()) == ["adjusted", "grown", "mapped"]
    for which in ("off", "on"):
        for directory in ("grown", "adjusted"):
            for name in ("cameras.txt", "images.txt", "points3D.txt"):
                assert ((tmp_path / which / "sparse" / directory / name).read_bytes()
                        == (tmp_path / "today" / "sparse" / directory / name).read_bytes()), (which, directory, name)
    assert {k: v for k, v in on.last_stats.items() if k != "mapped_model"} == off.last_stats
    s = on.last_stats["mapped_model"]
    assert s["registered_images"] == 12 and len(s["round_adjustments"]) == mapped["rounds"] and s["num_points3D"] == len(done["xyz"])
    assert "round_adjustments" not in on.last_stats["bundle_adjustment"] and "round_adjustments" not in on.last_stats["sparse_model"]
    assert_mapped_model_follows(SparseModel.read_text(tmp_path / "on" / "sparse" / "mapped"), done, 1e-9)
