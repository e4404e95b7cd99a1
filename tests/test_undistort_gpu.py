"""GPU tests of keypoint undistortion: vc_undistort_points against the numpy specification of
tests/util_undistort.py over wave and block edges, its argument checks, the front end, and the distorted scene with its k known
from match_exhaustive to the adjusted model."""
import numpy as np
import pytest
import torch

import util_absolute_pose as ua
import util_bundle_radial as ur
import util_mapper as um
import util_undistort as uu
from oracle import two_view_oracle as tv
from test_absolute_pose_spec import read_pairs, truth_pairs
from test_bundle_radial_spec import set_camera_model
from test_mapper_gpu import write_windowed_db

pytestmark = pytest.mark.gpu

PAD = 64                                    # sentinel elements on either side of every output
SIZES = [1, 63, 64, 65, 4097]               # a lane, either side of a wave, more than one block of 256 and its tail


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def call_of(n, fold=False):
    """n keypoints of the probe's pixels: over the four parameter sets, slot i mod 4, or on the camera whose fold is in the image."""
    px = uu.probe_pixels()
    xy = px[(np.arange(n) * 37) % len(px)]
    if fold:
        return xy, np.zeros(n, np.int32), uu.camera_row((uu.FOLD_K1, 0.0, 0.0, 0.0))[None]
    return xy, (np.arange(n) % 4).astype(np.int32), np.stack([uu.camera_row(k) for k in uu.PARAMETER_SETS])


def launch(xy, cam, cams, expect=0):
    """The raw entry point with its outputs inside sentinel-filled buffers -> status, xy64, valid (numpy); asserts that nothing
    outside the outputs was written."""
    from vit_colmap_amd import _lib

    lib = _lib.load()
    n = len(cam)
    d = [dev(np.asarray(xy, np.float32)), dev(np.asarray(cam, np.int32)), dev(np.asarray(cams, np.float64))]
    out = torch.full((2 * PAD + 2 * n,), 7.0, dtype=torch.float64, device="cuda")
    valid = torch.full((2 * PAD + n,), 7, dtype=torch.uint8, device="cuda")
    status = lib.vc_undistort_points(_lib.ptr(d[0]), _lib.ptr(d[1]), n, _lib.ptr(d[2]), len(cams), _lib.ptr(out[PAD:PAD + 2 * n]),
                                     _lib.ptr(valid[PAD:PAD + n]), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert status == expect
    o, v = out.cpu().numpy(), valid.cpu().numpy()
    assert (o[:PAD] == 7.0).all() and (o[PAD + 2 * n:] == 7.0).all() and (v[:PAD] == 7).all() and (v[PAD + n:] == 7).all()
    return status, o[PAD:PAD + 2 * n].reshape(n, 2), v[PAD:PAD + n]


@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_kernel_returns_the_specifications_bits(n, fold):
    xy, cam, cams = call_of(n, fold)
    want, valid = uu.undistort(xy, cam, cams)
    _, got, got_valid = launch(xy, cam, cams)
    assert set(np.unique(got_valid).tolist()) <= {0, 1} and np.array_equal(got_valid.astype(bool), valid)
    rel = uu.relative_difference(got, want)
    print(f"{n} keypoints, fold {fold}: {int(valid.sum())} valid, worst relative difference {rel:.3g}, "
          f"bits equal: {np.array_equal(got.view(np.uint64)[valid], want.view(np.uint64)[valid])}")
    assert rel <= uu.HOST_SPEC_REL
    if n >= 63:
        assert valid.all() != fold and valid.any()
    # the front end returns the same on tensors
    from vit_colmap_amd.matching.undistort import gpu_undistort, undistort_points

    t_xy, t_valid = undistort_points(dev(xy), dev(cam), dev(cams))
    assert t_xy.dtype == torch.float64 and t_valid.dtype == torch.bool and t_xy.is_cuda and t_xy.shape == (n, 2)
    assert np.array_equal(t_xy.cpu().numpy(), got, equal_nan=True) and np.array_equal(t_valid.cpu().numpy(), valid)
    n_xy, n_valid = gpu_undistort(xy, cam, cams)
    assert np.array_equal(n_xy, got, equal_nan=True) and np.array_equal(n_valid, valid)


def test_zero_distortion_is_the_closed_form_and_two_launches_agree():
    xy, cam, _ = call_of(4097)
    cams = np.stack([np.concatenate([uu.random_camera(i)[:4], np.zeros(4)]) for i in range(4)])
    _, got, valid = launch(xy, cam, cams)
    p64 = xy.astype(np.float64)
    fx, fy, cx, cy = (cams[cam, i] for i in range(4))
    want = np.stack([fx * ((p64[:, 0] - cx) / fx) + cx, fy * ((p64[:, 1] - cy) / fy) + cy], axis=1)
    assert valid.all() and np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert np.array_equal(launch(xy, cam, cams)[1].view(np.uint64), got.view(np.uint64))


def test_argument_validation_returns_the_documented_codes_and_writes_nothing():
    from vit_colmap_amd import _lib
    from vit_colmap_amd.matching.undistort import undistort_points

    lib = _lib.load()
    xy, cam, cams = call_of(4097)
    # n = 0: success without a launch, whatever the pointers are
    assert lib.vc_undistort_points(None, None, 0, None, 0, None, None, _lib.stream_ptr()) == _lib.VC_OK
    assert launch(xy[:0], cam[:0], cams)[0] == _lib.VC_OK
    empty = undistort_points(dev(xy[:0]), dev(cam[:0]), dev(cams))
    assert empty[0].shape == (0, 2) and empty[1].shape == (0,)
    # a slot out of range, in the first lane or in the tail of the last block: nothing is written (launch checks the sentinels
    # around the outputs; the outputs themselves keep theirs)
    for at, slot in ((0, -1), (4096, 4), (65, 1 << 30)):
        bad = cam.copy()
        bad[at] = slot
        status, out, valid = launch(xy, bad, cams, expect=_lib.VC_ERR_INVALID_ARG)
        assert (out == 7.0).all() and (valid == 7).all(), (at, slot)
        with pytest.raises(_lib.HipLibraryError, match="vc_undistort_points"):
            undistort_points(dev(xy), dev(bad), dev(cams))
    # null pointers and negative sizes
    d = [dev(xy), dev(cam), dev(cams)]
    out, valid = torch.full((2 * 4097,), 7.0, dtype=torch.float64, device="cuda"), torch.full((4097,), 7, dtype=torch.uint8, device="cuda")
    p = [_lib.ptr(d[0]), _lib.ptr(d[1]), _lib.ptr(d[2]), _lib.ptr(out), _lib.ptr(valid)]
    for k in range(5):
        q = p[:k] + [None] + p[k + 1:]
        assert lib.vc_undistort_points(q[0], q[1], 4097, q[2], 4, q[3], q[4], _lib.stream_ptr()) == _lib.VC_ERR_INVALID_ARG, k
    for n, n_cams in ((-1, 4), (4097, -1), (4097, 0)):
        assert lib.vc_undistort_points(p[0], p[1], n, p[2], n_cams, p[3], p[4], _lib.stream_ptr()) == _lib.VC_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (valid == 7).all()
    # the front end refuses wrong dtypes, devices and shapes
    for args in ([d[0].double(), d[1], d[2]], [d[0], d[1].long(), d[2]], [d[0], d[1], d[2].float()], [t.cpu() for t in d],
                 [d[0][:-1], d[1], d[2]], [d[0], d[1], d[2][:, :4]]):
        with pytest.raises(ValueError, match="undistort_points needs"):
            undistort_points(*args)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
def pipeline(path, **known):
    """match_exhaustive with relative pose, then the grown and the adjusted model -> the database's configs, grown, adjusted."""
    from vit_colmap_amd.mapping.bundle import build_adjusted_model
    from vit_colmap_amd.mapping.grow import build_sparse_model
    from vit_colmap_amd.matching import match_exhaustive
    from vit_colmap_amd.utils.config import MatchingConfig

    opts = MatchingConfig(compute_relative_pose=True).to_matching_options()
    if known:
        opts.known_distortion = True
    stats = match_exhaustive(database_path=str(path), matching_options=opts)
    configs = {pair: g["config"] for pair, g in read_pairs(path).items()}
    grown = build_sparse_model(path, **known)
    return stats, configs, grown, build_adjusted_model(path, grown=grown, **known)


def errors_of(model, scene):
    return ua.align_errors({i: (ua.quat_to_rot(im["qvec"]), im["tvec"]) for i, im in model.images.items()}, scene, *model.initial_pair)


def test_distorted_scene_with_its_k_known_from_matching_to_the_adjusted_model(tmp_path):
    """The test that fails without the feature.  The distorted windowed scene as a SIMPLE_RADIAL database with k = K1_TRUE and the
    prior flag, twin descriptors, no precomputed rows; beside it, as the reference measured here, the same pipeline on the
    undistorted windowed scene's PINHOLE database.  `truth_pairs` calls every pair with a baseline CALIBRATED, the ones whose
    views share no keypoint included (five or more views apart: 0 common keypoints, where four apart share 58 or more); a row
    needs matches, so the pairs held to CALIBRATED are the truth's with a common keypoint.  The margin of 10 % is for the float32
    rounding of the undistorted keypoints changing a RANSAC count."""
    from vit_colmap_amd.mapping import SparseModel
    from vit_colmap_amd.mapping.grow import build_sparse_model

    plain_scene, scene = um.windowed_scene(), ur.distorted_windowed_scene()
    K = scene["K"]
    write_windowed_db(tmp_path / "plain.db", plain_scene)
    write_windowed_db(tmp_path / "known.db", scene)
    set_camera_model(tmp_path / "known.db", "SIMPLE_RADIAL", [K[0, 0], K[0, 2], K[1, 2], ur.K1_TRUE])
    write_windowed_db(tmp_path / "off.db", scene)
    set_camera_model(tmp_path / "off.db", "SIMPLE_RADIAL", [K[0, 0], K[0, 2], K[1, 2], ur.K1_TRUE])

    _, ref_configs, ref_grown, ref = pipeline(tmp_path / "plain.db")
    stats, configs, grown, model = pipeline(tmp_path / "known.db", known_distortion=True)
    expected = sorted(p for p, g in truth_pairs(scene).items() if g["config"] == tv.CONFIG_CALIBRATED and len(g["inlier_matches"]))
    missing = [p for p in expected if configs.get(p) != tv.CONFIG_CALIBRATED]
    ref_missing = [p for p in expected if ref_configs.get(p) != tv.CONFIG_CALIBRATED]
    (rot, pos), (ref_rot, ref_pos) = errors_of(model, plain_scene), errors_of(ref, plain_scene)
    g_rot, g_pos = errors_of(grown, plain_scene)
    print(f"known k: {len(expected) - len(missing)} of {len(expected)} expected pairs CALIBRATED (PINHOLE reference: "
          f"{len(expected) - len(ref_missing)}), {stats['undistort_dropped_matches']} matches dropped, pair {model.initial_pair}, grown "
          f"{len(grown.images)} images {len(grown.points3D)} points in {grown.rounds} rounds (reference {len(ref_grown.images)}, "
          f"{len(ref_grown.points3D)}, {ref_grown.rounds}), grown rotation {g_rot:.4f} deg centre {g_pos:.5f}; adjusted rotation {rot:.4f} deg "
          f"(reference {ref_rot:.4f}), centre {pos:.5f} baselines (reference {ref_pos:.5f}), cost "
          f"{model.bundle_adjustment['initial_cost']:.2f} -> {model.bundle_adjustment['final_cost']:.4f} (reference "
          f"{ref.bundle_adjustment['final_cost']:.4f})")
    assert len(expected) == 38 and not missing, missing
    assert sorted(grown.images) == sorted(model.images) == list(range(1, 13))
    (cid, cam), = model.cameras.items()
    assert cam.model == "SIMPLE_RADIAL" and list(cam.params) == [K[0, 0], K[0, 2], K[1, 2], ur.K1_TRUE]
    model.write_text(tmp_path / "adjusted")
    text = (tmp_path / "adjusted" / "cameras.txt").read_text().splitlines()[-1].split()
    assert text[1] == "SIMPLE_RADIAL" and float(text[-1]) == ur.K1_TRUE and SparseModel.read_text(tmp_path / "adjusted") == model
    assert rot <= 1.1 * ref_rot and pos <= 1.1 * ref_pos
    # the models carry the raw keypoints; every kept observation is within the filter's bound under the distorted projection
    assert all(np.array_equal(model.images[i]["xys"], scene["keypoints"][i - 1].astype(np.float64)) for i in model.images)
    assert all(p["error"] <= um.MAX_ERROR and len(p["track"]) >= 2 for p in model.points3D.values())
    # the same database without the option: no CALIBRATED row, no model
    from vit_colmap_amd.matching import match_exhaustive
    from vit_colmap_amd.utils.config import MatchingConfig

    off = match_exhaustive(database_path=str(tmp_path / "off.db"), matching_options=MatchingConfig(compute_relative_pose=True).to_matching_options())
    assert "undistort_dropped_matches" not in off
    assert tv.CONFIG_CALIBRATED not in {g["config"] for g in read_pairs(tmp_path / "off.db").values()}
    with pytest.raises(ValueError, match="focal-length priors"):
        build_sparse_model(tmp_path / "off.db")
