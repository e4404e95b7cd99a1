"""GPU tests of the splitting of inconsistent tracks: vc_split_tracks against the bytes of the kernel's
per-component routine compiled for the host, on the shapes at which it can go wrong and inside sentinel-filled buffers; two
launches; the argument checks; agreement with vc_triangulate_tracks on consistent tracks; the growth with the flag on a
database whose matches are swapped, and the pipeline's step."""
from functools import lru_cache

import numpy as np
import pytest
import torch

import util_absolute_pose as ua
import util_mapper as um
import util_split as us
from test_absolute_pose_gpu import _two_view_bytes
from test_absolute_pose_spec import write_scene_db
from test_mapper_gpu import call_of as tracks_of
from test_mapper_gpu import launch as launch_triangulate
from test_mapper_spec import GROW_POS_BOUND, GROW_ROT_BOUND
from test_split_spec import assert_pure, run_split_host, split_host, swapped  # noqa: F401 - split_host is a fixture

pytestmark = pytest.mark.gpu

PAD = 64                                    # sentinel elements on either side of every array the kernel writes
SPECIAL = (0, 70, 1, 2, 11, 12)             # nothing to do; more nodes than lanes in a wave; all pairs up to 55; the sampler


def sized(i, n):
    """A merged component of exactly n nodes: merged components concatenated, cut and sorted by camera again."""
    parts, have = [], 0
    while have < max(n, 1):
        parts.append(us.merged_component(1000 + 7 * i + len(parts), outliers=0.15))
        have += len(parts[-1][0])
    obs, cam, truth = (np.concatenate([p[j] for p in parts])[:n] for j in range(3))
    order = np.argsort(cam, kind="stable")
    return obs[order], cam[order], truth[order], parts[0][3], parts[0][4]


@lru_cache(maxsize=None)
def call_of(n_comps, max_points, malformed=False):
    """One call of n_comps components in an order that mixes the sizes: the SPECIAL ones first, one of 70 again in the third
    wave, the others merged components of 4 to 30 nodes with 15 % random pixels; every fifth with an unusable node first or
    last; a third with pre-filled slots, every ninth with all of them (a lone component with none).  `malformed`: three components in the middle have
    offsets that descend or are negative.  -> the arguments of util_split.split_tracks' call, the components to be rejected."""
    comps = []
    for c in range(n_comps):
        if n_comps == 1:
            comps.append(sized(0, 70))
        elif c < len(SPECIAL) or c == 150:
            comps.append(sized(c, 70 if c == 150 else SPECIAL[c]))
        else:
            comps.append(us.merged_component(2000 + 300 * max_points + c, outliers=0.15,
                                             unusable=None if c % 5 else ("first", "last")[(c // 5) % 2]))
    obs, cam, offsets, cams, seeds, label, pts = us.as_one_call(
        comps, max_points, lambda c, comp: 0 if c % 3 or n_comps == 1 else (max_points if c % 9 == 0 else 1 + c % min(2, max_points)))
    rejected = []
    if malformed:
        k = n_comps // 2
        offsets = np.concatenate([offsets[:k + 1], [offsets[k] - 3, -5], offsets[k + 1:]]).astype(np.int32)
        seeds, pts = np.insert(seeds, k, [5, 6]), np.insert(pts, k, np.full((2, max_points, 3), np.nan), axis=0)
        rejected = [k, k + 1, k + 2]
    return (obs, cam, offsets, cams, seeds, label, pts), rejected


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def padded(a, sentinel):
    a = np.ascontiguousarray(a)
    flat = np.concatenate([np.full(PAD, sentinel, a.dtype), a.reshape(-1), np.full(PAD, sentinel, a.dtype)])
    return dev(flat)


def launch(obs_xy, obs_cam, offsets, cams, seeds, node_point, points_xyz, max_error=um.MAX_ERROR, tan2=um.MIN_TRI_ANGLE_TAN2):
    """The raw entry point, every array it writes inside sentinel-filled buffers -> node_point, points_xyz, count, new, error
    (numpy, the order of util_split.split_tracks) and the buffers' bytes; asserts that nothing outside them was written."""
    from vit_colmap_amd import _lib

    lib = _lib.load()
    C, max_points = len(offsets) - 1, points_xyz.shape[1]
    d = [dev(obs_xy), dev(obs_cam), dev(np.asarray(offsets, np.int32)), dev(cams),
         dev(np.asarray(seeds, np.int64).astype(np.uint32).view(np.int32))]
    s = C * max_points
    bufs = dict(label=padded(np.asarray(node_point, np.int32), -7), pts=padded(np.asarray(points_xyz, np.float64), 7.0),
                count=torch.full((2 * PAD + s,), -7, dtype=torch.int32, device="cuda"),
                new=torch.full((2 * PAD + s,), 7, dtype=torch.uint8, device="cuda"),
                error=torch.full((2 * PAD + s,), 7.0, dtype=torch.float64, device="cuda"))
    inner = {k: b[PAD:len(b) - PAD] for k, b in bufs.items()}
    _lib.check(lib.vc_split_tracks(_lib.ptr(d[0]), _lib.ptr(d[1]), _lib.ptr(d[2]), C, _lib.ptr(d[3]), len(cams), _lib.ptr(d[4]), max_points,
                                   float(max_error), float(tan2), _lib.ptr(inner["label"]), _lib.ptr(inner["pts"]), _lib.ptr(inner["count"]),
                                   _lib.ptr(inner["new"]), _lib.ptr(inner["error"]), _lib.stream_ptr()), "vc_split_tracks")
    torch.cuda.synchronize()
    host = {k: b.cpu().numpy() for k, b in bufs.items()}
    for k, b in host.items():
        sentinel = -7 if k in ("label", "count") else 7
        assert (b[:PAD] == sentinel).all() and (b[len(b) - PAD:] == sentinel).all(), f"{k}: written outside the array"
    out = {k: b[PAD:len(b) - PAD] for k, b in host.items()}
    assert set(np.unique(out["new"]).tolist()) <= {0, 1}, "a slot's flag was not written"
    return (out["label"], out["pts"].reshape(C, max_points, 3), out["count"].reshape(C, max_points), out["new"].reshape(C, max_points),
            out["error"].reshape(C, max_points), b"".join(b.tobytes() for b in host.values()))


def assert_same_bytes(got, host, what):
    for name, g, h in zip(("node_point", "points_xyz", "count", "new", "error"), got, host):
        assert g.tobytes() == h.tobytes(), f"{what}: {name} differs from the host build"


@pytest.mark.parametrize("n_comps", [1, 63, 65, 257])
def test_kernel_returns_the_host_builds_bytes(n_comps, split_host, tmp_path):  # noqa: F811
    for max_points in (1, 2, 4):
        call, _ = call_of(n_comps, max_points)
        sizes = np.diff(call[2])
        if n_comps >= 63:
            assert set(SPECIAL) <= set(sizes.tolist()) and sizes[6:].min() >= 4 and (call[5] >= 0).sum() >= n_comps // 3
            assert (np.isfinite(call[6]).all(axis=(1, 2))).sum() >= n_comps // 10          # components with every slot full
        got = launch(*call)
        host, _ = run_split_host(split_host, tmp_path, *call)
        assert_same_bytes(got[:5], host, f"{n_comps} components, max_points {max_points}")
        label, pts, count, new, error = got[:5]
        print(f"{n_comps} components of max_points {max_points}: {int(new.sum())} points created, {int((label >= 0).sum())} of "
              f"{len(label)} nodes labelled")
        assert np.array_equal(count, [[int((label[lo:hi] == k).sum()) for k in range(max_points)] for lo, hi in zip(call[2][:-1], call[2][1:])])
        assert new.sum() >= (n_comps // 2 if n_comps >= 63 else 1) and np.array_equal(np.isnan(error), new == 0)
        assert np.array_equal(label[call[5] != -1], call[5][call[5] != -1])               # a label that was given stays
        given = np.isfinite(call[6]).all(axis=2)
        assert np.array_equal(pts[given], call[6][given]) and np.array_equal(np.isfinite(pts).all(axis=2), given | (new == 1))


def test_malformed_offsets_reject_their_components_and_two_launches_return_the_same_bytes(split_host, tmp_path):  # noqa: F811
    call, rejected = call_of(65, 4, malformed=True)
    a, b = launch(*call), launch(*call)
    assert a[5] == b[5]
    host, _ = run_split_host(split_host, tmp_path, *call)
    assert_same_bytes(a[:5], host, "malformed offsets")
    label, pts, count, new, error = a[:5]
    offsets = call[2]
    for c in rejected:
        assert not count[c].any() and not new[c].any() and np.isnan(error[c]).all() and np.isnan(pts[c]).all()
    lo, hi = offsets[rejected[0]], offsets[rejected[-1] + 1]                         # the rows no well-formed component owns
    assert hi - lo >= 4 and np.array_equal(label[lo:hi], call[5][lo:hi])             # the labels of a rejected component stay
    assert new[:rejected[0]].sum() >= 10 and new[rejected[-1] + 1:].sum() >= 10
    # the thresholds are read: a tenth of a pixel creates fewer points, and the host build agrees
    tight = launch(*call, max_error=0.1)
    host, _ = run_split_host(split_host, tmp_path, *call, max_error=0.1)
    assert_same_bytes(tight[:5], host, "max_error 0.1")
    assert tight[3].sum() < new.sum()


def test_argument_validation_returns_the_documented_codes_without_launching():
    from vit_colmap_amd import _lib

    lib = _lib.load()
    (obs_xy, obs_cam, offsets, cams, seeds, label, pts), _ = call_of(63, 4)
    d = [dev(obs_xy), dev(obs_cam), dev(offsets), dev(cams), dev(np.asarray(seeds, np.int64).astype(np.uint32).view(np.int32))]
    C = len(seeds)
    out = [torch.full((len(label),), -7, dtype=torch.int32, device="cuda"), torch.full((12 * C,), 7.0, dtype=torch.float64, device="cuda"),
           torch.full((4 * C,), -7, dtype=torch.int32, device="cuda"), torch.full((4 * C,), 7, dtype=torch.uint8, device="cuda"),
           torch.full((4 * C,), 7.0, dtype=torch.float64, device="cuda")]
    p = [_lib.ptr(t) for t in d]
    o = [_lib.ptr(t) for t in out]

    def call(p=p, C=C, n_cams=len(cams), m=4, e=4.0, tan2=1e-3, o=o):
        return lib.vc_split_tracks(p[0], p[1], p[2], C, p[3], n_cams, p[4], m, e, tan2, o[0], o[1], o[2], o[3], o[4], _lib.stream_ptr())

    assert call(C=0) == _lib.VC_OK and call(p=[None] * 5, C=0, o=[None] * 5) == _lib.VC_OK and call(C=0, m=9) == _lib.VC_OK
    for k in range(5):
        assert call(p=p[:k] + [None] + p[k + 1:]) == _lib.VC_ERR_INVALID_ARG, k
        assert call(o=o[:k] + [None] + o[k + 1:]) == _lib.VC_ERR_INVALID_ARG, k
    assert call(C=-1) == _lib.VC_ERR_INVALID_ARG and call(n_cams=-1) == _lib.VC_ERR_INVALID_ARG
    for m in (0, -1, 5, 1 << 20):
        assert call(m=m) == _lib.VC_ERR_INVALID_ARG, m
    for bad in (-1.0, float("nan"), float("inf")):
        assert call(e=bad) == _lib.VC_ERR_INVALID_ARG and call(tan2=bad) == _lib.VC_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert all((t == s).all() for t, s in zip(out, (-7, 7.0, -7, 7, 7.0)))          # nothing was launched


def test_front_end_returns_the_raw_calls_result_and_leaves_its_inputs():
    from vit_colmap_amd.mapping.triangulate import split_tracks

    call, _ = call_of(65, 4)
    raw = launch(*call)
    args = [dev(a) for a in call[:4]] + [dev(np.asarray(call[4], np.int64).astype(np.uint32).view(np.int32)), dev(call[5]), dev(call[6])]
    label, pts, count, new, error = split_tracks(*args)
    assert new.dtype == torch.bool and count.dtype == torch.int32 and label.dtype == torch.int32 and pts.shape == (65, 4, 3) and pts.is_cuda
    for g, w in zip((label, pts, count, new, error), raw[:5]):
        assert np.array_equal(g.cpu().numpy(), w.astype(bool) if g.dtype == torch.bool else w, equal_nan=g.dtype == torch.float64)
    assert np.array_equal(args[5].cpu().numpy(), call[5]) and np.array_equal(args[6].cpu().numpy(), call[6], equal_nan=True)
    none = split_tracks(args[0][:0], args[1][:0], args[2][:1], args[3], args[4][:0], args[5][:0], args[6][:0])
    assert none[0].shape == (0,) and none[1].shape == (0, 4, 3) and none[2].shape == (0, 4)
    for bad in ([args[0].float()] + args[1:], args[:5] + [args[5].long(), args[6]], [a.cpu() for a in args],
                args[:6] + [args[6][:, :, :2]], args[:6] + [torch.cat([args[6], args[6]], dim=1)], args[:5] + [args[5][:-1], args[6]]):
        with pytest.raises(ValueError, match="split_tracks needs"):
            split_tracks(*bad)
    with pytest.raises(ValueError, match="ascend"):
        split_tracks(args[0], args[1], torch.flip(args[2], [0]).contiguous(), *args[3:])


def test_consistent_tracks_with_one_slot_return_the_triangulators_bytes():
    obs_xy, obs_cam, offsets, cams, seeds, _ = tracks_of(257)
    xyz, mask, count, error, _ = launch_triangulate(obs_xy, obs_cam, offsets, cams, seeds)
    label, pts, scount, new, serror, _ = launch(obs_xy, obs_cam, offsets, cams, seeds.view(np.uint32), np.full(len(obs_cam), -1, np.int32),
                                                np.full((257, 1, 3), np.nan))
    assert pts.tobytes() == xyz.tobytes() and scount.tobytes() == count.tobytes() and serror.tobytes() == error.tobytes()
    assert np.array_equal(label == 0, mask) and (label[~mask] == -1).all() and np.array_equal(new[:, 0] == 1, count > 0)
    assert (count > 0).sum() >= 128


# ---- growth ---------------------------------------------------------------------------------------------------------------------------
def test_growth_on_the_device_splits_the_swapped_database(tmp_path):
    from vit_colmap_amd.mapping.grow import build_sparse_model

    scene, pairs, images, off, on = swapped()
    write_scene_db(tmp_path / "s.db", scene, pairs)
    model = build_sparse_model(tmp_path / "s.db", split_tracks=True)
    tracks = [model.points3D[pid]["track"] if pid in model.points3D else None for pid in range(max(model.points3D) + 1)]
    mixed, duplicated = assert_pure(tracks, [pid for pid in model.split_points if pid in model.points3D])
    rot, pos = ua.align_errors({i: (ua.quat_to_rot(im["qvec"]), im["tvec"]) for i, im in model.images.items()}, scene, *model.initial_pair)
    print(f"{len(model.images)} images, {len(model.points3D)} points (spec {len(on['xyz'])}), {model.stats()['split_points']} split points "
          f"out of {model.split_components} components, {mixed} mixed, {duplicated} duplicated, rotation {rot:.3f} deg, centre {pos:.4f}")
    assert sorted(model.images) == list(range(1, 13)) and model.split_components == on["split_components"]
    assert abs(len(model.points3D) - len(on["xyz"])) <= um.GROW_POINT_MARGIN
    assert rot <= GROW_ROT_BOUND and pos <= GROW_POS_BOUND


def test_the_pipelines_step_with_the_flag_writes_more_points_and_leaves_the_database(tmp_path):
    from vit_colmap_amd.mapping.seed import SparseModel
    from vit_colmap_amd.pipeline import run_pipeline as rp
    from vit_colmap_amd.utils.config import Config

    scene, pairs, images, off, on = swapped()
    write_scene_db(tmp_path / "s.db", scene, pairs)
    rows_before = _two_view_bytes(tmp_path / "s.db")
    points = {}
    for flag in (False, True):
        p = rp.Pipeline(Config())
        p._write_sparse_model(tmp_path / "s.db", tmp_path / f"out{int(flag)}", "cuda", **(dict(split_tracks=True) if flag else {}))
        points[flag] = len(SparseModel.read_text(tmp_path / f"out{int(flag)}" / "sparse" / "grown").points3D)
        assert ("split_points" in p.last_stats["sparse_model"]) == flag and p.last_stats["sparse_model"]["registered_images"] == 12
    print(f"sparse/grown: {points[False]} points without the flag, {points[True]} with it")
    assert points[True] > points[False] + 100
    assert _two_view_bytes(tmp_path / "s.db") == rows_before
