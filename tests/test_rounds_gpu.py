"""GPU tests of the adjustment per growth round: vc_refine_tracks against the kernel's per-track routine
compiled for the host, byte for byte, on the shapes at which it can go wrong and inside sentinel-filled buffers; two
launches; offsets that delimit no list; the argument checks; the front end; build_mapped_model on the 24-view scene that one
adjustment does not recover; match_exhaustive + the pipeline's step end to end on the 12-view scene."""
from functools import lru_cache

import numpy as np
import pytest
import torch

import util_absolute_pose as ua
import util_mapper as um
import util_rounds as ur
from test_absolute_pose_gpu import _two_view_bytes
from test_absolute_pose_spec import truth_pairs, write_scene_db
from test_mapper_gpu import N_CAMS, PAD, call_of, dev, write_windowed_db
from test_rounds_spec import refine_host, run_refine_host  # noqa: F401 - the fixture

pytestmark = pytest.mark.gpu


@lru_cache(maxsize=None)
def refine_call(n_tracks):
    """test_mapper_gpu.call_of's tracks (lengths 70, 0, 1, 2, 3, 11, 12 first, then 2-12, unsorted; 0.5 px noise, 15 % random
    pixels; every fifth track with an unusable observation first or last), each started from the specification's
    triangulated X moved by START_OFFSET, every seventh (6, 13, ...) from NaN -> obs_xy, obs_cam, offsets, cams, init_xyz."""
    obs_xy, obs_cam, offsets, cams, _, spec = call_of(n_tracks)
    init = np.stack([ur.moved(x, t) for t, x in enumerate(spec[0])])
    init[6::7] = np.nan
    return obs_xy, obs_cam, offsets, cams, init


def launch(obs_xy, obs_cam, offsets, cams, init, max_error=um.MAX_ERROR, tan2=um.MIN_TRI_ANGLE_TAN2):
    """The raw entry point with its outputs inside sentinel-filled buffers -> xyz, mask (uint8), count, error (numpy); asserts
    that nothing outside the outputs was written."""
    from vit_colmap_amd import _lib

    lib = _lib.load()
    T, total = len(init), len(obs_cam)
    d = [dev(obs_xy), dev(obs_cam), dev(offsets), dev(cams), dev(init)]
    bufs = dict(xyz=torch.full((2 * PAD + 3 * T,), 7.0, dtype=torch.float64, device="cuda"),
                mask=torch.full((2 * PAD + total,), 7, dtype=torch.uint8, device="cuda"),
                count=torch.full((2 * PAD + T,), -7, dtype=torch.int32, device="cuda"),
                error=torch.full((2 * PAD + T,), 7.0, dtype=torch.float64, device="cuda"))
    inner = {k: b[PAD:len(b) - PAD] for k, b in bufs.items()}
    _lib.check(lib.vc_refine_tracks(_lib.ptr(d[0]), _lib.ptr(d[1]), _lib.ptr(d[2]), T, _lib.ptr(d[3]), len(cams), _lib.ptr(d[4]),
                                    float(max_error), float(tan2), _lib.ptr(inner["xyz"]), _lib.ptr(inner["mask"]),
                                    _lib.ptr(inner["count"]), _lib.ptr(inner["error"]), _lib.stream_ptr()), "vc_refine_tracks")
    torch.cuda.synchronize()
    host = {k: b.cpu().numpy() for k, b in bufs.items()}
    for k, b in host.items():
        sentinel = -7 if k == "count" else 7
        assert (b[:PAD] == sentinel).all() and (b[len(b) - PAD:] == sentinel).all(), f"{k}: written outside the output"
    out = {k: b[PAD:len(b) - PAD] for k, b in host.items()}
    return out["xyz"].reshape(T, 3), out["mask"], out["count"], out["error"]


def as_bytes(xyz, mask, count, error):
    """The layout of the host program's output file."""
    return (np.ascontiguousarray(xyz, np.float64).tobytes() + np.ascontiguousarray(error, np.float64).tobytes()
            + np.ascontiguousarray(count, np.int32).tobytes() + np.ascontiguousarray(mask).astype(np.uint8).tobytes())


@pytest.mark.parametrize("n_tracks", [1, 63, 65, 257])
def test_kernel_returns_the_host_builds_bytes(n_tracks, refine_host, tmp_path):  # noqa: F811
    obs_xy, obs_cam, offsets, cams, init = refine_call(n_tracks)
    (h_xyz, h_mask, h_count, h_error), raw, _ = run_refine_host(refine_host, tmp_path, obs_xy, obs_cam, offsets, cams, init)
    xyz, mask, count, error = launch(obs_xy, obs_cam, offsets, cams, init)
    assert set(np.unique(mask).tolist()) <= {0, 1}, "an observation's mask was not written"
    ok = h_count > 0
    differ = float(np.abs(xyz[ok] - h_xyz[ok]).max()) if ok.any() else 0.0
    print(f"{n_tracks} tracks: {int(ok.sum())} accepted, {int(h_mask.sum())} of {len(h_mask)} observations inliers, worst |X - X_host| "
          f"{differ:.3g}, worst error difference {float(np.abs(error[ok] - h_error[ok]).max()) if ok.any() else 0.0:.3g} px")
    assert np.array_equal(count, h_count) and np.array_equal(mask.astype(bool), h_mask)
    assert as_bytes(xyz, mask, count, error) == raw
    if n_tracks >= 63:
        lengths = np.diff(offsets)
        assert {0, 1, 2, 3, 12, 70} <= set(lengths.tolist()) and ok.sum() >= n_tracks // 2
        assert not ok[6::7].any() and np.isnan(xyz[6::7]).all()                  # the NaN starts
        spec = ur.refine_tracks(obs_xy, obs_cam, offsets, cams, init)
        assert np.array_equal(spec[2], count) and np.array_equal(spec[1], mask.astype(bool))
        assert np.linalg.norm(spec[0][ok] - xyz[ok], axis=1).max() <= ur.TOL_REFINE_X


def test_two_launches_return_identical_bytes_and_bad_offsets_skip_their_track():
    obs_xy, obs_cam, offsets, cams, init = refine_call(257)
    a, b = launch(obs_xy, obs_cam, offsets, cams, init), launch(obs_xy, obs_cam, offsets, cams, init)
    assert as_bytes(*a) == as_bytes(*b)
    # one offset below 0: track 16 ends before it starts (a descending pair), track 17 starts below 0; neither is read or
    # written, so their rows of the mask keep the sentinel, and every other track is what it was
    bad = offsets.copy()
    bad[17] = -5
    assert a[2][16] > 0 and a[2][17] > 0                                # both were accepted
    xyz, mask, count, error = launch(obs_xy, obs_cam, bad, cams, init)
    for t in (16, 17):
        assert count[t] == 0 and np.isnan(xyz[t]).all() and np.isnan(error[t]), t
    assert (mask[offsets[16]:offsets[18]] == 7).all()
    same = np.array([t for t in range(257) if t not in (16, 17)])
    assert np.array_equal(count[same], a[2][same]) and np.array_equal(xyz[same], a[0][same], equal_nan=True)
    assert np.array_equal(np.delete(mask, np.arange(offsets[16], offsets[18])), np.delete(a[1], np.arange(offsets[16], offsets[18])))


def test_argument_validation_returns_the_documented_codes_without_launching():
    from vit_colmap_amd import _lib

    lib = _lib.load()
    obs_xy, obs_cam, offsets, cams, init = refine_call(63)
    d = [dev(obs_xy), dev(obs_cam), dev(offsets), dev(cams), dev(init)]
    T = len(init)
    out = [torch.full((3 * T,), 7.0, dtype=torch.float64, device="cuda"), torch.full((len(obs_cam),), 7, dtype=torch.uint8, device="cuda"),
           torch.full((T,), -7, dtype=torch.int32, device="cuda"), torch.full((T,), 7.0, dtype=torch.float64, device="cuda")]
    p = [_lib.ptr(t) for t in d]
    o = [_lib.ptr(t) for t in out]

    def call(p=p, T=T, n_cams=N_CAMS, e=4.0, tan2=1e-3, o=o):
        return lib.vc_refine_tracks(p[0], p[1], p[2], T, p[3], n_cams, p[4], e, tan2, o[0], o[1], o[2], o[3], _lib.stream_ptr())

    assert call(T=0) == _lib.VC_OK and call(p=[None] * 5, T=0, o=[None] * 4) == _lib.VC_OK
    for k in range(5):
        assert call(p=p[:k] + [None] + p[k + 1:]) == _lib.VC_ERR_INVALID_ARG, k
    for k in range(4):
        assert call(o=o[:k] + [None] + o[k + 1:]) == _lib.VC_ERR_INVALID_ARG, k
    assert call(T=-1) == _lib.VC_ERR_INVALID_ARG and call(n_cams=-1) == _lib.VC_ERR_INVALID_ARG
    for bad in (-1.0, float("nan"), float("inf")):
        assert call(e=bad) == _lib.VC_ERR_INVALID_ARG and call(tan2=bad) == _lib.VC_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert (out[0] == 7.0).all() and (out[1] == 7).all() and (out[2] == -7).all() and (out[3] == 7.0).all()     # nothing was launched


def test_front_end_returns_what_the_raw_call_returns():
    from vit_colmap_amd.mapping.triangulate import refine_tracks

    call = refine_call(257)
    raw = launch(*call)
    args = [dev(a) for a in call]
    xyz, mask, count, error = refine_tracks(*args)
    assert mask.dtype == torch.bool and count.dtype == torch.int32 and xyz.shape == (257, 3) and xyz.is_cuda
    assert as_bytes(xyz.cpu().numpy(), mask.cpu().numpy(), count.cpu().numpy(), error.cpu().numpy()) == as_bytes(*raw)
    none = refine_tracks(args[0][:0], args[1][:0], args[2][:1], args[3], args[4][:0])
    assert none[0].shape == (0, 3) and none[1].shape == (0,) and none[2].shape == (0,) and none[3].shape == (0,)
    for bad in ([args[0].float()] + args[1:], [args[0], args[1].long()] + args[2:], [a.cpu() for a in args],
                args[:3] + [args[3].cpu()] + args[4:], args[:2] + [args[2][:-1]] + args[3:], args[:4] + [args[4][:, :2]]):
        with pytest.raises(ValueError, match="refine_tracks needs"):
            refine_tracks(*bad)
    with pytest.raises(ValueError, match="ascend"):
        refine_tracks(args[0], args[1], torch.flip(args[2], [0]).contiguous(), args[3], args[4])


# ---- the loop ---------------------------------------------------------------------------------------------------------------------------
def model_drift(model, scene, pair):
    return ua.align_errors({i: (ua.quat_to_rot(im["qvec"]), im["tvec"]) for i, im in model.images.items()}, scene, *pair)


def test_build_mapped_model_recovers_the_24_view_scene(tmp_path):
    """The database rows are truth_pairs', written directly: no matcher.  The figures of the specification are the constants
    tests/test_rounds_spec.py asserts on the CPU."""
    from vit_colmap_amd.mapping.rounds import build_mapped_model

    scene = um.windowed_scene(n_views=24, n_points=2400, noise=1.0)
    write_scene_db(tmp_path / "long.db", scene, pairs=truth_pairs(scene))
    model = build_mapped_model(tmp_path / "long.db")
    rot, pos = model_drift(model, scene, model.initial_pair)
    print(f"{len(model.images)} images, {len(model.points3D)} points (spec {ur.LONG_POINTS}), {len(model.round_adjustments)} round "
          f"adjustments of {[r['iterations'] for r in model.round_adjustments]} linearisations, drift {rot:.4g} deg / {pos:.4g} baselines, "
          f"observations added {sum(r['added_observations'] for r in model.round_adjustments)}, dropped "
          f"{sum(r['dropped_observations'] for r in model.round_adjustments)}")
    assert sorted(model.images) == list(range(1, 25))
    assert rot <= ur.LONG_ONCE_ROT / 4 and pos <= ur.LONG_ONCE_POS / 4
    assert rot <= ur.LONG_ROT_BOUND and pos <= ur.LONG_POS_BOUND
    assert abs(len(model.points3D) - ur.LONG_POINTS) <= um.GROW_POINT_MARGIN
    assert all(len(p["track"]) >= 2 for p in model.points3D.values())


def test_match_exhaustive_then_the_pipelines_step_with_the_flag_end_to_end(tmp_path):
    from vit_colmap_amd.mapping import SparseModel
    from vit_colmap_amd.matching import match_exhaustive
    from vit_colmap_amd.pipeline import run_pipeline as rp
    from vit_colmap_amd.utils.config import Config, MatchingConfig

    scene = um.windowed_scene()
    write_windowed_db(tmp_path / "w.db", scene)
    match_exhaustive(database_path=str(tmp_path / "w.db"), matching_options=MatchingConfig(compute_relative_pose=True).to_matching_options())
    rows_before = _two_view_bytes(tmp_path / "w.db")
    p = rp.Pipeline(Config())
    p._write_sparse_model(tmp_path / "w.db", tmp_path / "out", "cuda", adjust=True, adjust_rounds=True)
    assert sorted(f.name for f in (tmp_path / "out" / "sparse").iterdir()) == ["adjusted", "grown", "mapped"]
    pair = tuple(p.last_stats["sparse_model"]["initial_pair"])
    mapped, adjusted = (SparseModel.read_text(tmp_path / "out" / "sparse" / name) for name in ("mapped", "adjusted"))
    rot, pos = model_drift(mapped, scene, pair)
    a_rot, a_pos = model_drift(adjusted, scene, pair)
    print(f"pair {pair}: mapped {len(mapped.images)} images, {len(mapped.points3D)} points, drift {rot:.4g} deg / {pos:.4g} baselines; adjusted "
          f"{len(adjusted.points3D)} points, {a_rot:.4g} deg / {a_pos:.4g}")
    assert sorted(mapped.images) == list(range(1, 13)) and p.last_stats["mapped_model"]["registered_images"] == 12
    assert len(p.last_stats["mapped_model"]["round_adjustments"]) == p.last_stats["mapped_model"]["rounds"]
    assert rot <= 2 * a_rot and pos <= 2 * a_pos
    assert _two_view_bytes(tmp_path / "w.db") == rows_before
