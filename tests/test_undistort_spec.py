"""CPU tests of keypoint undistortion: the numpy specification of tests/util_undistort.py (round trip, zero
distortion, the Jacobian, the fold), the kernel's per-keypoint routine compiled for the host (tools/undistort_host.cpp) against
it, plain and under the host sanitizers, the product's host logic with the specification in its seams (growth, adjustment,
the matcher's shared helper) and the flags.  No GPU."""
import argparse
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import util_absolute_pose as ua
import util_bundle_radial as ur
import util_undistort as uu
from test_absolute_pose_spec import spec_estimate, spec_two_view_pose, truth_pairs, write_scene_db
from test_bundle_radial_spec import distorted, set_camera_model
from test_mapper_spec import GROW_POS_BOUND, GROW_ROT_BOUND, spec_triangulate, windowed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
HOST_BUILD = [HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off"]
SOURCE = os.path.join(ROOT, "tools", "undistort_host.cpp")
# the round trip |distort(undistort(p)) - p|: the last Newton step is at most 1e-12 in normalised units (its square is at most
# 1e-24) and Newton's error after a step is far below the step, times f = 600: 6e-10 px, rounded up
ROUND_TRIP_PX = 1e-9


def one_camera(px, k):
    cam = uu.camera_row(k)
    return cam, uu.undistort(px, np.zeros(len(px), np.int32), cam[None])


# ---- the specification ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", uu.PARAMETER_SETS)
def test_round_trip_over_the_image_stays_within_the_stop_rules_bound(k):
    px = uu.probe_pixels()
    steps = []
    cam = uu.camera_row(k)
    out, valid = uu.undistort(px, np.zeros(len(px), np.int32), cam[None], steps)
    worst = float(np.abs(uu.distort(out, cam) - px.astype(np.float64)).max())
    print(f"k {k}: {len(px)} pixels, worst round trip {worst:.3g} px, at most {int(steps[0].max())} steps")
    assert valid.all() and np.isfinite(out).all()
    assert worst <= ROUND_TRIP_PX
    assert steps[0].max() < uu.MAX_STEPS
    # the distortion is not a no-op on this image: the corner moves by pixels
    assert np.abs(out - px).max() > 1.0


def test_zero_distortion_returns_the_closed_form_to_the_bit():
    px = uu.probe_pixels()
    cams = np.stack([uu.camera_row((0.0, 0.0, 0.0, 0.0))] + [np.concatenate([uu.random_camera(i)[:4], np.zeros(4)]) for i in range(5)])
    cam = np.arange(len(px), dtype=np.int32) % len(cams)
    steps = []
    out, valid = uu.undistort(px, cam, cams, steps)
    p64 = px.astype(np.float64)
    fx, fy, cx, cy = (cams[cam, i] for i in range(4))
    want = np.stack([fx * ((p64[:, 0] - cx) / fx) + cx, fy * ((p64[:, 1] - cy) / fy) + cy], axis=1)
    assert valid.all() and (steps[0] == 1).all()
    assert np.array_equal(out.view(np.uint64), want.view(np.uint64))


def test_jacobian_matches_central_differences_of_the_forward_model():
    rs = np.random.RandomState(4)
    worst = 0.0
    for k in uu.PARAMETER_SETS + [(uu.FOLD_K1, 0.0, 0.0, 0.0)] + [tuple(uu.random_camera(i)[4:]) for i in range(20)]:
        cam = uu.camera_row(k)
        x, y = rs.uniform(-0.53, 0.53, 50), rs.uniform(-0.4, 0.4, 50)
        a, b, d = uu.jacobian(x, y, cam)
        h = 1e-6
        xp, xm = uu.distort_normalised(x + h, y, cam), uu.distort_normalised(x - h, y, cam)
        yp, ym = uu.distort_normalised(x, y + h, cam), uu.distort_normalised(x, y - h, cam)
        fd = [(xp[0] - xm[0]) / (2 * h), (yp[0] - ym[0]) / (2 * h), (xp[1] - xm[1]) / (2 * h), (yp[1] - ym[1]) / (2 * h)]
        worst = max(worst, *(float(np.abs(f - j).max()) for f, j in zip(fd, (a, b, b, d))))
    print(f"worst |central difference - Jacobian| {worst:.3g}")
    # the rounding of two values of order 1 divided by 2 h = 2e-6, plus h^2 times a third derivative of order 1: 1e-10 + 1e-12;
    # 4x, rounded up
    assert worst <= 5e-10


def test_the_fold_decides_validity_exactly():
    """k1 = -0.6 alone: the distorted radius has a maximum, (2 / 3) sqrt(1 / (3 |k1|)) in normalised units; a keypoint inside it
    inverts, one outside it does not."""
    cam = uu.camera_row((uu.FOLD_K1, 0.0, 0.0, 0.0))
    r_fold = uu.fold_radius(uu.FOLD_K1) * uu.FOCAL
    ang = 2 * np.pi * np.arange(16) / 16
    for factor, inverts in ((0.95, True), (1.05, False)):
        px = np.stack([cam[2] + factor * r_fold * np.cos(ang), cam[3] + factor * r_fold * np.sin(ang)], axis=1).astype(np.float32)
        out, valid = uu.undistort(px, np.zeros(16, np.int32), cam[None])
        assert (valid == inverts).all() and np.isnan(out).all() != inverts, factor
        if inverts:
            assert np.abs(uu.distort(out, cam) - px.astype(np.float64)).max() <= ROUND_TRIP_PX
    # every pixel of the image: the count is the analytic one
    u, v = np.meshgrid(np.arange(uu.WIDTH, dtype=np.float32), np.arange(uu.HEIGHT, dtype=np.float32))
    px = np.stack([u.ravel(), v.ravel()], axis=1)
    steps = []
    out, valid = uu.undistort(px, np.zeros(len(px), np.int32), cam[None], steps)
    radius = np.hypot((px[:, 0].astype(np.float64) - cam[2]) / cam[0], (px[:, 1].astype(np.float64) - cam[3]) / cam[1])
    inside = radius <= uu.fold_radius(uu.FOLD_K1)
    print(f"{int(valid.sum())} of {len(px)} pixels invert ({100 * valid.mean():.1f} %), analytic {int(inside.sum())}, at most "
          f"{int(steps[0][valid].max())} steps")
    assert np.array_equal(valid, inside)
    assert int(valid.sum()) == int(inside.sum()) and 0.5 < valid.mean() < 0.95
    assert np.isnan(out[~valid]).all() and np.isfinite(out[valid]).all()


def test_unusable_inputs_are_invalid_and_a_slot_out_of_range_is_refused():
    cam = uu.camera_row(uu.PARAMETER_SETS[0])
    bad = np.stack([cam] * 4)
    bad[1, 0], bad[2, 4], bad[3, 2] = 0.0, np.nan, np.inf
    px = np.array([[100.0, 50.0], [100.0, 50.0], [100.0, 50.0], [100.0, 50.0], [np.nan, 3.0]], np.float32)
    out, valid = uu.undistort(px, np.array([0, 1, 2, 3, 0], np.int32), bad)
    assert valid.tolist() == [True, False, False, False, False] and np.isnan(out[1:]).all()
    for slot in (-1, 4):
        with pytest.raises(ValueError):
            uu.undistort(px[:1], np.array([slot], np.int32), bad)
    out, valid = uu.undistort(np.zeros((0, 2), np.float32), np.zeros(0, np.int32), bad)
    assert out.shape == (0, 2) and valid.shape == (0,)


# ---- the kernel's routine compiled for the host ---------------------------------------------------------------------------------------
_BUILT = {}


def _build(out, extra):
    proc = subprocess.run(HOST_BUILD + extra + ["-o", str(out), SOURCE], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert proc.returncode == 0, f"{out.name} does not build:\n{proc.stdout}"
    return str(out)


@pytest.fixture(scope="session")
def undistort_host(tmp_path_factory):
    """tools/undistort_host.cpp built with the line its source gives (once per session, test_undistort_gpu.py shares it)."""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc to build the host program with")
    if "plain" not in _BUILT:
        _BUILT["plain"] = _build(tmp_path_factory.mktemp("undistort_host") / "undistort_host", [])
    return _BUILT["plain"]


def test_host_build_header_gives_the_build_line():
    head = open(SOURCE).read()
    assert " ".join(os.path.basename(w) if w == HIPCC else w for w in HOST_BUILD) + " -o undistort_host tools/undistort_host.cpp" in head


def test_host_build_matches_the_spec_to_the_bit(undistort_host, tmp_path):
    worst = 0.0
    for name, xy, cam, cams in uu.host_cases():
        want, valid = uu.undistort(xy, cam, cams)
        (got, got_valid), _ = uu.run_host(undistort_host, tmp_path, xy, cam, cams, name)
        assert np.array_equal(got_valid, valid), name
        rel = uu.relative_difference(got, want)
        worst = max(worst, rel)
        print(f"{name}: {len(cam)} keypoints, {int(valid.sum())} valid, worst relative difference {rel:.3g}, "
              f"bits equal: {np.array_equal(got.view(np.uint64), want.view(np.uint64))}")
    assert worst <= uu.HOST_SPEC_REL
    # a slot out of range is refused, as the entry point refuses it
    uu.write_keypoints_file(tmp_path / "bad.bin", np.zeros((2, 2), np.float32), [0, 1], uu.camera_row(uu.PARAMETER_SETS[0])[None])
    done = subprocess.run([undistort_host, str(tmp_path / "bad.bin"), str(tmp_path / "bad_out.bin")], stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, text=True)
    assert done.returncode == 2 and "outside" in done.stderr and not (tmp_path / "bad_out.bin").exists()


def test_host_build_under_the_sanitizers_reports_nothing(tmp_path):
    """The same program with the host half built -fsanitize=address,undefined, run on its own over the same files, the keypoints
    beyond the fold, the NaN keypoint and the unusable cameras included."""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc to build the host program with")
    program = _build(tmp_path / "undistort_host_san", ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                                                       "-Xarch_host", "-g"])
    for name, xy, cam, cams in uu.host_cases():
        xy, cams = xy.copy(), np.concatenate([cams, cams[:1], cams[:1]])
        xy[0] = np.nan
        cams[-1, 0], cams[-2, 5] = 0.0, np.nan
        cam = cam.copy()
        cam[1], cam[2] = len(cams) - 1, len(cams) - 2
        want, valid = uu.undistort(xy, cam, cams)
        (got, got_valid), stderr = uu.run_host(program, tmp_path, xy, cam, cams, name)
        assert stderr == "" and np.array_equal(got_valid, valid) and not valid[:3].any(), name
        assert np.array_equal(got.view(np.uint64)[valid], want.view(np.uint64)[valid]) and np.isnan(got[~valid]).all(), name
    # no keypoint at all
    (got, got_valid), stderr = uu.run_host(program, tmp_path, np.zeros((0, 2), np.float32), np.zeros(0, np.int32), cams, "empty")
    assert stderr == "" and got.shape == (0, 2)


# ---- the product's host logic with the specification in the seams ----------------------------------------------------------------------
def model_poses(model):
    return {i: (ua.quat_to_rot(im["qvec"]), np.asarray(im["tvec"], np.float64)) for i, im in model.images.items()}


def grow_with_spec(path, **kw):
    from vit_colmap_amd.mapping.grow import build_sparse_model

    return build_sparse_model(path, device="cpu", two_view_pose_fn=spec_two_view_pose, estimate_fn=spec_estimate,
                              triangulate_fn=spec_triangulate, **kw)


@pytest.fixture(scope="module")
def known_db(tmp_path_factory):
    """The distorted windowed scene as a SIMPLE_RADIAL database with k = K1_TRUE, the prior flag and the truth's pairs, and its
    model grown with the option on (the specification in every seam)."""
    directory = tmp_path_factory.mktemp("undistort")
    scene = ur.distorted_windowed_scene()
    K = scene["K"]
    write_scene_db(directory / "k.db", scene, truth_pairs(scene))
    set_camera_model(directory / "k.db", "SIMPLE_RADIAL", [K[0, 0], K[0, 2], K[1, 2], ur.K1_TRUE])
    calls = []

    def counting(xy, cam, cams, device):
        calls.append((len(cam), np.array(cams)))
        return uu.spec_undistort(xy, cam, cams, device)

    return directory / "k.db", scene, grow_with_spec(directory / "k.db", known_distortion=True, undistort_fn=counting), calls


def test_without_the_option_a_known_distortion_still_loses_the_prior(known_db):
    path = known_db[0]
    with pytest.raises(ValueError, match="focal-length priors"):
        grow_with_spec(path)
    from vit_colmap_amd.mapping.seed import build_seed_model

    with pytest.raises(ValueError, match="focal-length priors"):
        build_seed_model(path, device="cpu", two_view_pose_fn=spec_two_view_pose, estimate_fn=spec_estimate)


def test_growth_on_undistorted_keypoints_follows_the_pinhole_scene(known_db):
    """The test that fails without the feature: the distorted scene, its k known, grows as the undistorted scene does."""
    path, scene, model, calls = known_db
    plain_scene, _, _, plain = windowed()
    K = scene["K"]
    # one launch over all 12 images, one slot: the camera's eight numbers
    assert len(calls) == 1 and calls[0][0] == 12 * 1200
    assert np.array_equal(calls[0][1], [[K[0, 0], K[1, 1], K[0, 2], K[1, 2], ur.K1_TRUE, 0.0, 0.0, 0.0]])
    assert sorted(model.images) == list(range(1, 13))
    assert model.initial_pair == plain["initial_pair"] == (8, 10)
    assert model.rounds == plain["rounds"] == 3 and len(model.points3D) == len(plain["xyz"]) == 1161
    rot, pos = ua.align_errors(model_poses(model), plain_scene, *model.initial_pair)
    rot0, pos0 = ua.align_errors(distorted()[2]["poses"], plain_scene, *distorted()[2]["initial_pair"])
    print(f"known k: worst rotation {rot:.3f} deg, worst centre {pos:.4f} baselines; grown under k = 0: {rot0:.3f} deg, {pos0:.4f} baselines")
    assert rot <= GROW_ROT_BOUND and pos <= GROW_POS_BOUND
    assert rot < rot0 and pos < pos0
    # the model carries the raw keypoints, as COLMAP's does, and its errors are those of the distorted projection
    for i, im in model.images.items():
        assert np.array_equal(im["xys"], scene["keypoints"][i - 1].astype(np.float64))
    (cid, cam), = model.cameras.items()
    assert cam.model == "SIMPLE_RADIAL" and cam.params[3] == ur.K1_TRUE
    errors = np.array([p["error"] for p in model.points3D.values()])
    assert np.isfinite(errors).all() and errors.max() < 12.0
    from vit_colmap_amd.mapping.seed import _pixel_errors_radial

    pid, p = next(iter(sorted(model.points3D.items())))
    poses = model_poses(model)
    own = [_pixel_errors_radial(K, (ur.K1_TRUE, 0.0), *poses[i], p["xyz"][None], model.images[i]["xys"][kp][None])[0] for i, kp in p["track"]]
    assert p["error"] == pytest.approx(float(np.mean(own)), rel=1e-12)


def test_a_keypoint_that_does_not_invert_is_in_no_track(tmp_path):
    """k = -0.6 folds inside the image: the keypoints beyond the fold leave the rows before the seed and the tracks see them."""
    from vit_colmap_amd.mapping.seed import _read_database

    scene = ur.distorted_windowed_scene()
    K = scene["K"]
    pairs = {p: dict(g) for p, g in truth_pairs(scene).items()}
    # the truth's inliers lie near the centre; three matches of pair (1, 2) are put on keypoints of image 1 beyond the fold
    cam = uu.camera_row((uu.FOLD_K1, 0.0, 0.0, 0.0))
    beyond = np.nonzero(~uu.undistort(scene["keypoints"][0], np.zeros(1200, np.int32), cam[None])[1])[0][:3]
    inside = np.nonzero(uu.undistort(scene["keypoints"][1], np.zeros(1200, np.int32), cam[None])[1])[0][:3]
    assert len(beyond) == 3
    pairs[(1, 2)]["inlier_matches"] = np.concatenate([pairs[(1, 2)]["inlier_matches"], np.stack([beyond, inside], axis=1).astype(np.uint32)])
    write_scene_db(tmp_path / "f.db", scene, pairs)
    set_camera_model(tmp_path / "f.db", "SIMPLE_RADIAL", [K[0, 0], K[0, 2], K[1, 2], uu.FOLD_K1])
    images, cameras, Kd, kps, rows, known = _read_database(tmp_path / "f.db", True, uu.spec_undistort, "cpu")
    assert all(Kd[i] is not None for i in images) and set(known["dist"].values()) == {(uu.FOLD_K1, 0.0)}
    dropped = 0
    for (i, j), g in rows.items():
        m = g["inlier_matches"].astype(np.int64)
        assert np.isfinite(kps[i][m[:, 0]]).all() and np.isfinite(kps[j][m[:, 1]]).all()
        dropped += len(pairs[(i, j)]["inlier_matches"]) - len(m)
    invalid = sum(int(np.isnan(kp[:, 0]).sum()) for kp in kps.values())
    print(f"{invalid} keypoints do not invert, {dropped} inlier matches left the rows")
    assert dropped == 3 and np.array_equal(rows[(1, 2)]["inlier_matches"], truth_pairs(scene)[(1, 2)]["inlier_matches"])
    from vit_colmap_amd.mapping.grow import _components

    assert not any(int(i) == 1 and int(kp) in set(beyond.tolist()) for nodes in _components(kps, Kd, rows) for i, kp in nodes)
    assert invalid > 0 and all(kps[i].dtype == np.float64 and np.array_equal(known["raw"][i], scene["keypoints"][i - 1]) for i in images)
    # without the option: today's five entries, float32 keypoints, no K for the distorted camera
    plain = _read_database(tmp_path / "f.db")
    assert len(plain) == 5 and all(k is None for k in plain[2].values()) and all(kp.dtype == np.float32 for kp in plain[3].values())
    # OPENCV verifies under the option and the mapper keeps refusing it
    set_camera_model_opencv(tmp_path / "f.db", [K[0, 0], K[1, 1], K[0, 2], K[1, 2], -0.1, 0.0, 1e-3, 0.0])
    assert all(k is None for k in _read_database(tmp_path / "f.db", True, uu.spec_undistort, "cpu")[2].values())


def set_camera_model_opencv(path, params):
    import sqlite3

    with sqlite3.connect(str(path)) as db:
        db.execute("UPDATE cameras SET model = ?, params = ?", (4, np.asarray(params, np.float64).tobytes()))


def recording_bundle(seen):
    """A bundle_fn that moves nothing and says what it was given."""
    def bundle_fn(cams, points, offsets, obs_cam, obs_xy, const_mask, device, **kw):
        seen.clear()
        seen.update(kw, obs_xy=np.array(obs_xy), obs_cam=np.array(obs_cam), offsets=np.array(offsets))
        report = dict(iterations=1, accepted_steps=0, initial_cost=1.0, final_cost=1.0, final_lambda=1e-4, decisions=[])
        if "cam_dist" in kw:
            row = [np.concatenate([cams[0, 12:16], kw["cam_dist"][0]])] * len(kw.get("intr_mask", [0]))
            report.update(cam_dist=np.array(kw["cam_dist"]), intrinsics=dict(before=np.array(row), after=np.array(row)))
        return cams, points, report
    return bundle_fn


def test_build_adjusted_model_hands_over_raw_observations_and_the_known_k(known_db, tmp_path):
    from vit_colmap_amd.mapping import bundle_intr
    from vit_colmap_amd.mapping.bundle import build_adjusted_model

    path, scene, grown, _ = known_db
    seen = {}
    model = build_adjusted_model(path, device="cpu", bundle_fn=recording_bundle(seen), grown=grown, known_distortion=True)
    assert sorted(seen) == ["cam_dist", "obs_cam", "obs_xy", "offsets"]
    assert np.array_equal(seen["cam_dist"], np.tile([ur.K1_TRUE, 0.0], (12, 1)))
    ids, pids = sorted(grown.images), sorted(grown.points3D)
    raw = np.array([scene["keypoints"][i - 1][kp] for pid in pids for i, kp in grown.points3D[pid]["track"]], np.float64)
    assert np.array_equal(seen["obs_xy"], raw)
    # the adjusted model keeps the camera, the raw keypoints and errors of the distorted projection (the stub moved nothing)
    (cid, cam), = model.cameras.items()
    assert list(cam.params) == list(grown.cameras[cid].params) and cam.params[3] == ur.K1_TRUE
    assert all(np.array_equal(model.images[i]["xys"], grown.images[i]["xys"]) for i in ids)
    assert len(model.points3D) == len(grown.points3D)
    for pid in pids[:50]:
        assert model.points3D[pid]["error"] == pytest.approx(grown.points3D[pid]["error"], rel=1e-9, abs=1e-12)
    # with the loss: passed on beside it
    build_adjusted_model(path, device="cpu", bundle_fn=recording_bundle(seen), grown=grown, known_distortion=True, loss="huber", loss_scale=2.0)
    assert seen["loss"] == "huber" and seen["loss_scale"] == 2.0 and "cam_dist" in seen
    # with refine_focal_length alone the groups hold k1 and k2; with refine_distortion the known k is the starting value
    build_adjusted_model(path, device="cpu", bundle_fn=recording_bundle(seen), grown=grown, known_distortion=True, refine_focal_length=True)
    assert list(seen["intr_mask"]) == [bundle_intr.HOLD_CX | bundle_intr.HOLD_CY | bundle_intr.TIED | bundle_intr.HOLD_K1 | bundle_intr.HOLD_K2]
    assert np.array_equal(seen["cam_dist"], np.tile([ur.K1_TRUE, 0.0], (12, 1))) and seen["max_iterations"] == bundle_intr.REFINE_MAX_ITERATIONS
    build_adjusted_model(path, device="cpu", bundle_fn=recording_bundle(seen), grown=grown, known_distortion=True, refine_distortion=True)
    assert not int(seen["intr_mask"][0]) & bundle_intr.HOLD_K1 and int(seen["intr_mask"][0]) & bundle_intr.HOLD_K2
    assert np.array_equal(seen["cam_dist"], np.tile([ur.K1_TRUE, 0.0], (12, 1))) and np.array_equal(seen["obs_xy"], raw)


def test_without_the_option_the_adjustment_gets_todays_keywords(tmp_path):
    from vit_colmap_amd.mapping.bundle import build_adjusted_model

    scene, pairs, _, _ = windowed()
    write_scene_db(tmp_path / "w.db", scene, pairs)
    grown = grow_with_spec(tmp_path / "w.db")
    seen = {}
    build_adjusted_model(tmp_path / "w.db", device="cpu", bundle_fn=recording_bundle(seen), grown=grown)
    assert sorted(seen) == ["obs_cam", "obs_xy", "offsets"]
    # the option on a database without distortion changes nothing: no cam_dist, the same observations
    obs = seen["obs_xy"].copy()
    from vit_colmap_amd.mapping.seed import _read_database

    called = []
    on, off = _read_database(tmp_path / "w.db", True, lambda *a: called.append(a), "cpu"), _read_database(tmp_path / "w.db")
    assert not called and len(on) == 6 and on[5]["dist"] == {} and all(np.array_equal(on[2][i], off[2][i]) for i in off[2])
    assert all(on[3][i].dtype == np.float32 and np.array_equal(on[3][i], off[3][i]) for i in off[3])
    assert all(np.array_equal(on[4][p]["inlier_matches"], off[4][p]["inlier_matches"]) for p in off[4])
    build_adjusted_model(tmp_path / "w.db", device="cpu", bundle_fn=recording_bundle(seen), grown=grown, known_distortion=True)
    assert sorted(seen) == ["obs_cam", "obs_xy", "offsets"] and np.array_equal(seen["obs_xy"], obs)


# ---- the matcher's shared helper -----------------------------------------------------------------------------------------------------------
def two_camera_db(path):
    """Four images of 40 keypoints across the 640 x 480 image: images 1 and 2 on a flagged PINHOLE camera, 3 and 4 on a flagged
    SIMPLE_RADIAL camera with k = -0.6, whose fold lies inside the image."""
    from vit_colmap_amd.database import ColmapDatabase
    from vit_colmap_amd.database.colmap_db import Camera

    rs = np.random.RandomState(8)
    db = ColmapDatabase(str(path))
    plain = db.db.write_camera(Camera(model="PINHOLE", width=640, height=480, params=[600.0, 600.0, 320.0, 240.0], has_prior_focal_length=True))
    radial = db.db.write_camera(Camera(model="SIMPLE_RADIAL", width=640, height=480, params=[600.0, 320.0, 240.0, uu.FOLD_K1],
                                       has_prior_focal_length=True))
    kps = []
    for k, cam in enumerate((plain, plain, radial, radial)):
        i = db.add_image(f"view{k}.png", cam)
        kp = np.stack([rs.uniform(0, 640, 40), rs.uniform(0, 480, 40)], axis=1).astype(np.float32)
        kp[0] = (321.0, 243.0)                                            # inverts
        kp[1] = (2.0, 3.0)                                                # beyond the fold of the radial camera
        db.add_keypoints(i, kp)
        db.add_descriptors(i, rs.randint(0, 255, (40, 32)).astype(np.uint8))
        kps.append(kp)
    db.db.close()
    return kps, uu.camera_row((uu.FOLD_K1, 0.0, 0.0, 0.0))


def run_matcher(path, known, guided=False):
    from vit_colmap_amd.matching import match_exhaustive
    from vit_colmap_amd.utils.config import MatchingConfig

    seen = dict(verify=[], guided=[], undistort=0)
    lists = np.stack([np.arange(40), np.arange(40)], axis=1).astype(np.uint32)

    def match_fn(block, counts, pairs, max_ratio, max_distance, cross_check):
        return [lists.copy() for _ in pairs]

    def verify_fn(kps, pair_images, pair_ids, match_lists, **extra):
        seen["verify"].append(dict(kps={k: np.array(v) for k, v in kps.items()}, pairs=list(pair_images), lists=[np.array(m) for m in match_lists],
                                   extra=extra))
        return [dict(config=2, inlier_matches=np.asarray(m, np.uint32), F=np.eye(3), H=np.eye(3), n_f=len(m), n_h=0, model="F",
                     model9=np.eye(3, dtype=np.float32).reshape(9)) for m in match_lists]

    def guided_fn(block, counts, keypoints_xy, pairs, models, kinds, max_error, max_ratio, max_distance, cross_check):
        seen["guided"].append(np.array(keypoints_xy))
        return [lists.copy() for _ in pairs]

    def undistort_fn(xy, cam, cams, device):
        seen["undistort"] += 1
        return uu.spec_undistort(xy, cam, cams, device)

    opts = MatchingConfig(guided_matching=guided).to_matching_options()
    if known:
        opts.known_distortion = True
    stats = match_exhaustive(str(path), matching_options=opts, device="cpu", match_fn=match_fn, verify_fn=verify_fn, guided_fn=guided_fn,
                             undistort_fn=undistort_fn)
    return stats, seen


def test_matching_helper_undistorts_only_the_distorted_cameras_keypoints(tmp_path, caplog):
    from vit_colmap_amd.database import ColmapDatabase

    kps, cam = two_camera_db(tmp_path / "two.db")
    # without the option: today's call (the distorted camera has no prior, nothing is undistorted, nothing dropped)
    stats, seen = run_matcher(tmp_path / "two.db", known=False)
    v = seen["verify"][0]
    assert seen["undistort"] == 0 and "undistort_dropped_matches" not in stats
    assert all(np.array_equal(v["kps"][k], kps[k]) for k in range(4)) and list(v["extra"]["cameras"][1]) == [1, 1, 0, 0]
    assert all(len(m) == 40 for m in v["lists"])
    os.remove(tmp_path / "two.db")
    two_camera_db(tmp_path / "two.db")
    with caplog.at_level("INFO", logger="vit_colmap_amd.matching"):
        stats, seen = run_matcher(tmp_path / "two.db", known=True, guided=True)
    v = seen["verify"][0]
    assert seen["undistort"] == 1                                                   # one launch for both images
    want = {k: uu.undistort(kps[k], np.zeros(40, np.int32), cam[None]) for k in (2, 3)}
    assert all(np.array_equal(v["kps"][k], kps[k]) for k in (0, 1))                  # the plain camera's keypoints are untouched
    for k in (2, 3):
        xy64, valid = want[k]
        assert valid[0] and not valid[1] and not valid.all()
        assert np.array_equal(v["kps"][k][valid], xy64[valid].astype(np.float32)) and np.isnan(v["kps"][k][~valid]).all()
        assert np.abs(v["kps"][k][valid] - kps[k][valid]).max() > 0.01
    K, prior = v["extra"]["cameras"]
    assert list(prior) == [1, 1, 1, 1] and np.array_equal(K[2], [[600.0, 0.0, 320.0], [0.0, 600.0, 240.0], [0.0, 0.0, 1.0]])
    # a match on a keypoint that does not invert is absent from what the verifier gets and present in the matches table
    ok = {0: np.ones(40, bool), 1: np.ones(40, bool), 2: want[2][1], 3: want[3][1]}
    dropped = 0
    for (a, b), m in zip(v["pairs"], v["lists"]):
        keep = ok[a] & ok[b]
        assert np.array_equal(m[:, 0], np.nonzero(keep)[0]) and np.array_equal(m[:, 1], np.nonzero(keep)[0])
        dropped += int((~keep).sum())
    assert dropped > 0 and stats["undistort_dropped_matches"] == dropped and stats["matches"] == 6 * 40
    assert sum("were not verified" in r.getMessage() for r in caplog.records) == 1
    assert np.isfinite(seen["guided"][0]).all()                                      # the guided kernel is given no NaN pixel
    with ColmapDatabase.open_database(str(tmp_path / "two.db")) as db:
        for a in range(1, 5):
            assert np.array_equal(db.read_keypoints(a)[:, :2], kps[a - 1])           # the database keeps the raw keypoints
            for b in range(a + 1, 5):
                assert len(db.read_matches(a, b)) == 40
                g = db.read_two_view_geometry(a, b)
                keep = ok[a - 1] & ok[b - 1]
                assert np.array_equal(g["inlier_matches"][:, 0], np.nonzero(keep)[0])  # keypoint indices, the guided lists filtered too


def test_sharded_pipeline_uses_the_same_helper_and_keeps_the_raw_keypoints_in_the_database(tmp_path):
    """run_sharded on one rank: a SIMPLE_RADIAL camera with k = -0.6 and the prior; with the option the verifier gets what the
    shared helper makes of the gathered keypoints, the database the raw ones; without it today's call."""
    from vit_colmap_amd.database import ColmapDatabase
    from vit_colmap_amd.pipeline.distributed import run_sharded
    from vit_colmap_amd.utils import image_io
    from vit_colmap_amd.utils.config import MatchingConfig

    d = tmp_path / "images"
    d.mkdir()
    rs = np.random.RandomState(9)
    feats = {}
    for k in range(3):
        image_io.imwrite(d / f"im{k}.png", np.full((48, 64, 3), k, np.uint8))
        kp = np.stack([rs.uniform(0, 640, 30), rs.uniform(0, 480, 30), rs.uniform(1, 2, 30)], axis=1).astype(np.float32)   # (x, y, scale)
        kp[0, :2], kp[1, :2] = (330.0, 250.0), (1.0, 2.0)                  # inverts; beyond the fold
        feats[k] = (kp, rs.randint(0, 255, (30, 16)).astype(np.uint8))
    lists = np.stack([np.arange(30), np.arange(30)], axis=1).astype(np.uint32)
    params = [600.0, 320.0, 240.0, uu.FOLD_K1]
    cam = uu.camera_row((uu.FOLD_K1, 0.0, 0.0, 0.0))
    for known in (False, True):
        seen, calls = [], []

        def verify_fn(kps, pair_images, pair_ids, match_lists, **extra):
            seen.append((dict(kps), [np.array(m) for m in match_lists], extra))
            return [dict(config=2, inlier_matches=np.asarray(m, np.uint32), F=np.eye(3), H=np.eye(3), n_f=len(m), n_h=0) for m in match_lists]

        def undistort_fn(xy, slots, cams, device):
            calls.append(np.array(cams))
            return uu.spec_undistort(xy, slots, cams, device)

        opts = MatchingConfig().to_matching_options()
        opts.known_distortion = known
        path = tmp_path / f"sharded{int(known)}.db"
        stats = run_sharded(d, path, "SIMPLE_RADIAL", params, feature_fn=lambda images: [feats[int(im[0, 0, 0])] for im in images],
                            matching_options=opts, match_fn=lambda block, counts, pairs, *a: [lists.copy() for _ in pairs],
                            verify_fn=verify_fn, device="cpu", prior_focal_length=True, undistort_fn=undistort_fn)
        kps, given, extra = seen[0]
        with ColmapDatabase.open_database(str(path)) as db:
            assert all(np.array_equal(db.read_keypoints(k + 1), feats[k][0]) for k in range(3))
            assert all(len(db.read_matches(a, b)) == 30 for a, b in ((1, 2), (1, 3), (2, 3)))
        if not known:
            assert not calls and extra == {} and all(len(m) == 30 for m in given) and "undistort_dropped_matches" not in stats
            assert all(np.array_equal(kps[k][:, :2], feats[k][0][:, :2]) for k in range(3))
            continue
        assert len(calls) == 1 and np.array_equal(calls[0], cam[None])
        assert list(extra["cameras"][1]) == [1, 1, 1]
        ok = {}
        for k in range(3):
            xy64, ok[k] = uu.undistort(feats[k][0][:, :2], np.zeros(30, np.int32), cam[None])
            assert ok[k][0] and not ok[k][1]
            assert np.array_equal(kps[k][ok[k]], xy64[ok[k]].astype(np.float32)) and np.isnan(kps[k][~ok[k]]).all()
        for (a, b), m in zip(((0, 1), (0, 2), (1, 2)), given):
            assert np.array_equal(m[:, 0], np.nonzero(ok[a] & ok[b])[0])
        assert stats["undistort_dropped_matches"] == sum(int((~(ok[a] & ok[b])).sum()) for a, b in ((0, 1), (0, 2), (1, 2))) > 0


# ---- the flags -----------------------------------------------------------------------------------------------------------------------------
def test_known_distortion_flag_is_off_by_default_and_needs_the_prior(tmp_path, monkeypatch):
    from vit_colmap_amd.matching.exhaustive import MatchSettings
    from vit_colmap_amd.pipeline import run_pipeline as rp
    from vit_colmap_amd.utils.config import CameraConfig, Config, FeatureMatchingOptions, SiftMatchingOptions

    assert CameraConfig().known_distortion is False and Config().camera.known_distortion is False
    assert SiftMatchingOptions().known_distortion is False and FeatureMatchingOptions().known_distortion is False
    assert Config.from_args(argparse.Namespace()).camera.known_distortion is False
    assert Config.from_args(argparse.Namespace(known_distortion=True)).camera.known_distortion is True
    assert Config.from_args(argparse.Namespace(known_distortion=True)).camera.prior_focal_length is False
    assert MatchSettings.from_options(None, None).known_distortion is False
    assert MatchSettings.from_options(FeatureMatchingOptions(known_distortion=True), None).known_distortion is True
    assert MatchSettings.from_options(None, SiftMatchingOptions(known_distortion=True)).known_distortion is True
    assert MatchSettings.from_options(FeatureMatchingOptions(known_distortion=True), None, verify=False).known_distortion is False

    def no_extractor(self):
        raise AssertionError("the extractor was built before the flags were checked")

    monkeypatch.setattr(rp.Pipeline, "_make_extractor", no_extractor)
    cfg = Config()
    cfg.camera.known_distortion, cfg.do_reconstruction = True, False
    with pytest.raises(ValueError, match="known_distortion needs .*prior_focal_length"):
        rp.Pipeline(cfg).run(tmp_path / "images", tmp_path / "out", tmp_path / "x.db")
    assert not (tmp_path / "x.db").exists()
    # the option travels on the matching options, only where it is on
    cfg.camera.prior_focal_length = True
    on, off = rp.Pipeline(cfg)._matching_options(), rp.Pipeline(Config())._matching_options()
    assert on.known_distortion and on.sift.known_distortion and not off.known_distortion and off == Config().matching.to_matching_options()
    seen = []
    monkeypatch.setattr(rp.Pipeline, "run", lambda self, *a, **k: seen.append((self.config.camera.prior_focal_length,
                                                                               self.config.camera.known_distortion, self.config.camera.params)))
    base = ["prog", "--images", "i", "--output", "o", "--db", "d"]
    for extra in ([], ["--prior-focal-length", "--known-distortion", "--camera-model", "SIMPLE_RADIAL", "--camera-params", "600,320,240,-0.15"]):
        monkeypatch.setattr(sys, "argv", base + extra)
        rp.main()
    assert seen == [(False, False, None), (True, True, [600.0, 320.0, 240.0, -0.15])]


def test_camera_params_length_is_checked_against_the_model_before_any_database(tmp_path, monkeypatch):
    from vit_colmap_amd.pipeline import run_pipeline as rp
    from vit_colmap_amd.utils.config import Config, parse_camera_params

    assert parse_camera_params("600, 320,240", "SIMPLE_PINHOLE") == [600.0, 320.0, 240.0]
    assert parse_camera_params("600,610,320,240,-0.1,0.01,1e-3,-2e-3", "OPENCV") == [600.0, 610.0, 320.0, 240.0, -0.1, 0.01, 1e-3, -2e-3]
    assert Config.from_args(argparse.Namespace(camera_model="PINHOLE", camera_params="600,600,321.5,239")).camera.params == [600.0, 600.0, 321.5, 239.0]
    assert Config.from_args(argparse.Namespace(camera_model="PINHOLE")).camera.params is None
    for model, text, count in (("SIMPLE_RADIAL", "600,320,240", 4), ("RADIAL", "600,320,240,0.1", 5), ("PINHOLE", "1,2,3,4,5", 4),
                               ("OPENCV", "600,600,320,240", 8), ("SIMPLE_PINHOLE", "", 3), ("PINHOLE", "600,600,a,240", 4),
                               ("PINHOLE", "600,600,nan,240", 4)):
        with pytest.raises(ValueError, match=f"{model} takes {count} "):
            parse_camera_params(text, model)
        with pytest.raises(ValueError, match=f"{model} takes {count} "):
            Config.from_args(argparse.Namespace(camera_model=model, camera_params=text))
    with pytest.raises(ValueError, match="unknown camera model 'FISHEYE'"):
        parse_camera_params("1,2,3", "FISHEYE")
    # a configuration built by hand is checked by the pipeline before the extractor and the database exist
    monkeypatch.setattr(rp.Pipeline, "_make_extractor", lambda self: (_ for _ in ()).throw(AssertionError("extractor built")))
    cfg = Config()
    cfg.camera.model, cfg.camera.params, cfg.do_reconstruction = "SIMPLE_RADIAL", [600.0, 320.0, 240.0], False
    with pytest.raises(ValueError, match="SIMPLE_RADIAL takes 4 "):
        rp.Pipeline(cfg).run(tmp_path / "images", tmp_path / "out", tmp_path / "x.db")
    assert not (tmp_path / "x.db").exists()
    monkeypatch.setattr(sys, "argv", ["prog", "--images", "i", "--output", "o", "--db", str(tmp_path / "y.db"), "--camera-model", "RADIAL",
                                      "--camera-params", "600,320,240"])
    with pytest.raises(ValueError, match="RADIAL takes 5 "):
        rp.main()
    assert not (tmp_path / "y.db").exists()


def test_pipeline_passes_the_option_to_both_models_only_where_it_is_on(known_db, tmp_path, monkeypatch):
    import vit_colmap_amd.mapping.bundle as bundle
    import vit_colmap_amd.mapping.grow as grow
    from vit_colmap_amd.pipeline import run_pipeline as rp
    from vit_colmap_amd.utils.config import Config

    path = known_db[0]
    real = grow.build_sparse_model
    given = []

    def build(p, device="cuda", **kw):
        given.append(dict(kw))
        return real(p, device="cpu", two_view_pose_fn=spec_two_view_pose, estimate_fn=spec_estimate, triangulate_fn=spec_triangulate,
                    undistort_fn=uu.spec_undistort, **kw)

    monkeypatch.setattr(grow, "build_sparse_model", build)
    seen = {}
    monkeypatch.setattr(bundle, "bundle_adjust", recording_bundle(seen))
    p = rp.Pipeline(Config())
    p.last_stats = {}
    p._write_sparse_model(path, tmp_path / "out", "cpu", adjust=True, known_distortion=True)
    assert given == [dict(known_distortion=True)] and "cam_dist" in seen
    assert p.last_stats["sparse_model"]["registered_images"] == 12
    a, b = ((tmp_path / "out" / "sparse" / m / "cameras.txt").read_text().splitlines() for m in ("grown", "adjusted"))
    assert a == b and a[-1].split()[1] == "SIMPLE_RADIAL" and float(a[-1].split()[-1]) == ur.K1_TRUE
    # without it: today's call, and this database has no model
    warned = []
    monkeypatch.setattr(rp.logger, "warning", lambda msg, *args: warned.append(msg % args))
    p._write_sparse_model(path, tmp_path / "out2", "cpu", adjust=True)
    assert given[-1] == {} and len(warned) == 1 and "focal-length priors" in warned[0] and not (tmp_path / "out2").exists()
