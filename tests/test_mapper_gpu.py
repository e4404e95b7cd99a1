"""GPU tests of the growth of the seed model: vc_triangulate_tracks against the kernel's per-track function
compiled for the host and the numpy specification of tests/util_mapper.py on the shapes at which it can go wrong, inside
sentinel-filled buffers; two launches; the front end's length sort; the argument checks; match_exhaustive +
build_sparse_model end to end and the pipeline's flag."""
import sys
from functools import lru_cache

import numpy as np
import pytest
import torch

import util_absolute_pose as ua
import util_essential as ue
import util_mapper as um
from test_absolute_pose_gpu import _two_view_bytes
from test_absolute_pose_spec import read_pairs, scene_images, write_scene_db
from test_mapper_spec import run_host, triangulate_host  # noqa: F401 - the fixture

pytestmark = pytest.mark.gpu

PAD = 64                                    # sentinel elements on either side of every output
SPECIAL = (70, 0, 1, 2, 3, 11, 12)          # more observations than lanes in a wave; rejected; all pairs up to 55; the sampler
N_CAMS = 73                                 # 72 cameras 1.2 degrees apart and one that is not registered (a NaN row)


@lru_cache(maxsize=None)
def camera_table():
    rows = [um.camera_row(*ua.look_at(np.array([8.0 * np.sin(a), 0.2 * np.cos(5 * a), -8.0 * np.cos(a)]), np.zeros(3)), ue.SCENE_K)
            for a in np.radians(1.2 * np.arange(72) - 40.0)]
    return np.stack(rows + [np.full(16, np.nan)])


@lru_cache(maxsize=None)
def call_of(n_tracks):
    """One call of n_tracks tracks in an order that mixes the lengths: the SPECIAL ones first, one of 70 again in the middle
    of the third wave, the others of 2-12 observations; 0.5 px noise, some gross outliers; every fifth track has an unusable
    observation in its first or its last slot (a slot below 0, a slot past the table, the NaN row, a NaN pixel in turn).
    -> obs_xy, obs_cam, offsets, cams, seeds and the specification's result."""
    rs = np.random.RandomState(14000 + n_tracks)
    cams = camera_table()
    lengths = [SPECIAL[t] if t < len(SPECIAL) else 70 if t == 150 else int(rs.randint(2, 13)) for t in range(n_tracks)]
    if n_tracks == 1:
        lengths = [70]
    obs, slots = [], []
    for t, n in enumerate(lengths):
        X = np.array([rs.uniform(-2, 2), rs.uniform(-1.5, 1.5), rs.uniform(-1.5, 1.5)])
        views = np.sort(rs.choice(72, n, replace=False))
        p = np.array([ue.SCENE_K @ (cams[v, :9].reshape(3, 3) @ X + cams[v, 9:12]) for v in views]).reshape(n, 3)
        o = p[:, :2] / p[:, 2:] + rs.normal(0, 0.5, (n, 2))
        wrong = rs.uniform(size=n) < 0.15
        o = np.where(wrong[:, None], np.stack([rs.uniform(0, 640, n), rs.uniform(0, 480, n)], axis=1), o)
        views = views.astype(np.int32)
        if t % 5 == 0 and n >= 1:
            where = 0 if (t // 5) % 2 == 0 else n - 1
            kind = (t // 10) % 4
            if kind == 3:
                o[where, 1] = np.nan
            else:
                views[where] = (-1, N_CAMS, N_CAMS - 1)[kind]
        obs.append(o), slots.append(views)
    obs_xy, obs_cam = np.concatenate(obs).reshape(-1, 2), np.concatenate(slots).astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    seeds = rs.randint(0, 1 << 32, n_tracks, dtype=np.uint64).astype(np.uint32).view(np.int32)
    return obs_xy, obs_cam, offsets, cams, seeds, um.triangulate_tracks(obs_xy, obs_cam, offsets, cams, seeds)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def launch(obs_xy, obs_cam, offsets, cams, seeds, max_error=um.MAX_ERROR, tan2=um.MIN_TRI_ANGLE_TAN2):
    """The raw entry point with its outputs inside sentinel-filled buffers -> xyz, mask, count, error (numpy) and the buffers'
    bytes; asserts that nothing outside the outputs was written."""
    from vit_colmap_amd import _lib

    lib = _lib.load()
    T, total = len(seeds), len(obs_cam)
    d = [dev(obs_xy), dev(obs_cam), dev(offsets), dev(cams), dev(seeds)]
    bufs = dict(xyz=torch.full((2 * PAD + 3 * T,), 7.0, dtype=torch.float64, device="cuda"),
                mask=torch.full((2 * PAD + total,), 7, dtype=torch.uint8, device="cuda"),
                count=torch.full((2 * PAD + T,), -7, dtype=torch.int32, device="cuda"),
                error=torch.full((2 * PAD + T,), 7.0, dtype=torch.float64, device="cuda"))
    inner = {k: b[PAD:len(b) - PAD] for k, b in bufs.items()}
    _lib.check(lib.vc_triangulate_tracks(_lib.ptr(d[0]), _lib.ptr(d[1]), _lib.ptr(d[2]), T, _lib.ptr(d[3]), len(cams), _lib.ptr(d[4]),
                                         float(max_error), float(tan2), _lib.ptr(inner["xyz"]), _lib.ptr(inner["mask"]),
                                         _lib.ptr(inner["count"]), _lib.ptr(inner["error"]), _lib.stream_ptr()), "vc_triangulate_tracks")
    torch.cuda.synchronize()
    host = {k: b.cpu().numpy() for k, b in bufs.items()}
    for k, b in host.items():
        sentinel = -7 if k == "count" else 7
        assert (b[:PAD] == sentinel).all() and (b[len(b) - PAD:] == sentinel).all(), f"{k}: written outside the output"
    out = {k: b[PAD:len(b) - PAD] for k, b in host.items()}
    assert set(np.unique(out["mask"]).tolist()) <= {0, 1}, "an observation's mask was not written"
    return out["xyz"].reshape(T, 3), out["mask"].astype(bool), out["count"], out["error"], b"".join(b.tobytes() for b in host.values())


def assert_follows(got, spec, offsets, what):
    xyz, mask, count, error = got
    s_xyz, s_mask, s_count, s_error = spec
    assert np.array_equal(count, s_count), what
    assert np.array_equal(mask, s_mask), what
    ok = s_count > 0
    assert np.isnan(xyz[~ok]).all() and np.isnan(error[~ok]).all() and np.isfinite(xyz[ok]).all() and np.isfinite(error[ok]).all(), what
    worst = float(np.linalg.norm(xyz[ok] - s_xyz[ok], axis=1).max()) if ok.any() else 0.0
    worst_error = float(np.abs(error[ok] - s_error[ok]).max()) if ok.any() else 0.0
    print(f"{what}: {int(ok.sum())} of {len(count)} accepted, worst |X - X_spec| {worst:.3g}, worst error difference {worst_error:.3g} px")
    assert worst <= um.TOL_X, what
    for t in np.nonzero(~ok)[0]:
        assert not mask[offsets[t]:offsets[t + 1]].any(), what
    return worst


@pytest.mark.parametrize("n_tracks", [1, 63, 65, 257])
def test_kernel_matches_the_host_build_and_the_spec(n_tracks, triangulate_host, tmp_path):  # noqa: F811
    obs_xy, obs_cam, offsets, cams, seeds, spec = call_of(n_tracks)
    lengths = np.diff(offsets)
    if n_tracks >= 63:
        assert set(SPECIAL) <= set(lengths.tolist()) and (spec[2] > 0).sum() >= n_tracks // 2
        assert spec[2][1] == 0 and spec[2][2] == 0                    # the tracks of 0 and 1 observations
    # the specification alone: its masks do not change when its X moves by the tolerance
    for t in np.nonzero(spec[2] > 0)[0]:
        lo, hi = offsets[t], offsets[t + 1]
        slots = obs_cam[lo:hi]
        rows = np.where(((slots >= 0) & (slots < N_CAMS))[:, None], cams[np.clip(slots, 0, N_CAMS - 1)], np.nan)
        assert um.stable_under(obs_xy[lo:hi], rows, int(seeds[t]) & 0xFFFFFFFF, um.TOL_X), t
    got = launch(obs_xy, obs_cam, offsets, cams, seeds)
    assert_follows(got[:4], spec, offsets, f"kernel, {n_tracks} tracks")
    host, _ = run_host(triangulate_host, tmp_path, obs_xy, obs_cam, offsets, cams, seeds.view(np.uint32))
    assert_follows(host, spec, offsets, f"host build, {n_tracks} tracks")
    ok = spec[2] > 0
    print(f"kernel against the host build: worst |X - X_host| {np.abs(got[0][ok] - host[0][ok]).max() if ok.any() else 0.0:.3g}")


def test_two_launches_return_identical_bytes_and_thresholds_are_read():
    obs_xy, obs_cam, offsets, cams, seeds, spec = call_of(257)
    a, b = launch(obs_xy, obs_cam, offsets, cams, seeds), launch(obs_xy, obs_cam, offsets, cams, seeds)
    assert a[4] == b[4]
    # a threshold of a tenth of a pixel and one of 30 degrees, against the specification under the same thresholds
    for max_error, tan2 in ((0.1, um.MIN_TRI_ANGLE_TAN2), (um.MAX_ERROR, float(np.tan(np.radians(30.0)) ** 2))):
        tight = launch(obs_xy, obs_cam, offsets, cams, seeds, max_error, tan2)
        want = um.triangulate_tracks(obs_xy, obs_cam, offsets, cams, seeds, max_error, tan2)
        assert np.array_equal(tight[2] > 0, want[2] > 0) and (tight[2] > 0).sum() < (spec[2] > 0).sum()


def test_front_end_with_the_length_sort_returns_what_the_unsorted_call_returns():
    from vit_colmap_amd.mapping.triangulate import triangulate_tracks

    obs_xy, obs_cam, offsets, cams, seeds, spec = call_of(257)
    raw = launch(obs_xy, obs_cam, offsets, cams, seeds)
    args = [dev(obs_xy), dev(obs_cam), dev(offsets), dev(cams), dev(seeds)]
    for sort in (True, False):
        xyz, mask, count, error = triangulate_tracks(*args, sort_by_length=sort)
        assert mask.dtype == torch.bool and count.dtype == torch.int32 and xyz.shape == (257, 3) and xyz.is_cuda
        assert np.array_equal(xyz.cpu().numpy(), raw[0], equal_nan=True) and np.array_equal(mask.cpu().numpy(), raw[1]), sort
        assert np.array_equal(count.cpu().numpy(), raw[2]) and np.array_equal(error.cpu().numpy(), raw[3], equal_nan=True), sort
    # nothing to do
    none = triangulate_tracks(args[0][:0], args[1][:0], args[2][:1], args[3], args[4][:0])
    assert none[0].shape == (0, 3) and none[1].shape == (0,) and none[2].shape == (0,) and none[3].shape == (0,)
    empty = triangulate_tracks(args[0][:0], args[1][:0], torch.zeros(3, dtype=torch.int32, device="cuda"), args[3], args[4][:2])
    assert torch.isnan(empty[0]).all() and empty[2].tolist() == [0, 0] and torch.isnan(empty[3]).all()
    # wrong dtypes, devices and shapes are refused in the manner of the minimal solvers' front end
    for bad in ([args[0].float()] + args[1:], [args[0], args[1].long()] + args[2:], [a.cpu() for a in args],
                args[:3] + [args[3].cpu()] + args[4:], args[:2] + [args[2][:-1]] + args[3:], args[:3] + [args[3][:, :12]] + args[4:]):
        with pytest.raises(ValueError, match="triangulate_tracks needs"):
            triangulate_tracks(*bad)
    with pytest.raises(ValueError, match="ascend"):
        triangulate_tracks(args[0], args[1], torch.flip(args[2], [0]).contiguous(), args[3], args[4])


def test_argument_validation_returns_the_documented_codes_without_launching():
    from vit_colmap_amd import _lib

    lib = _lib.load()
    obs_xy, obs_cam, offsets, cams, seeds, _ = call_of(63)
    d = [dev(obs_xy), dev(obs_cam), dev(offsets), dev(cams), dev(seeds)]
    T = len(seeds)
    out = [torch.full((3 * T,), 7.0, dtype=torch.float64, device="cuda"), torch.full((len(obs_cam),), 7, dtype=torch.uint8, device="cuda"),
           torch.full((T,), -7, dtype=torch.int32, device="cuda"), torch.full((T,), 7.0, dtype=torch.float64, device="cuda")]
    p = [_lib.ptr(t) for t in d]
    o = [_lib.ptr(t) for t in out]

    def call(p=p, T=T, n_cams=N_CAMS, e=4.0, tan2=1e-3, o=o):
        return lib.vc_triangulate_tracks(p[0], p[1], p[2], T, p[3], n_cams, p[4], e, tan2, o[0], o[1], o[2], o[3], _lib.stream_ptr())

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


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def write_windowed_db(path, scene, seed=11):
    """write_scene_db, then random descriptors for the keypoints that observe nothing.  write_scene_db gives keypoint i the same
    descriptor in every view, which suits arc_scene, where a view sees 80 % of the points; here neighbouring views share a
    fifth of them, so 1200 index matches per pair would hold too few true ones for the verifier's MIN_INLIER_RATIO (0.25) and
    no pair would be verified at all.  A keypoint at a uniform random pixel now also looks like nothing else."""
    from vit_colmap_amd.database import ColmapDatabase

    write_scene_db(path, scene)
    rs = np.random.RandomState(seed)
    with ColmapDatabase.open_database(str(path)) as db:
        for v, seen in enumerate(scene["visible"]):
            d = db.read_descriptors(v + 1).copy()
            r = np.abs(rs.standard_normal((int((~seen).sum()), d.shape[1])))
            d[~seen] = np.clip(r / np.linalg.norm(r, axis=1, keepdims=True) * 512, 0, 255).astype(np.uint8)
            db.write_descriptors(v + 1, d)


def test_match_exhaustive_then_build_sparse_model_end_to_end(tmp_path):
    from vit_colmap_amd.mapping import SparseModel, build_seed_model
    from vit_colmap_amd.mapping.grow import build_sparse_model
    from vit_colmap_amd.matching import match_exhaustive
    from vit_colmap_amd.utils.config import MatchingConfig

    scene = um.windowed_scene()
    write_windowed_db(tmp_path / "w.db", scene)
    match_exhaustive(database_path=str(tmp_path / "w.db"), matching_options=MatchingConfig(compute_relative_pose=True).to_matching_options())
    rows_before = _two_view_bytes(tmp_path / "w.db")
    seed = build_seed_model(tmp_path / "w.db")
    model = build_sparse_model(tmp_path / "w.db")
    assert len(seed.images) < 12 and sorted(model.images) == list(range(1, 13))
    # the specification's growth on the same database content
    spec = um.grow_model(scene_images(scene), read_pairs(tmp_path / "w.db"))
    a, b = spec["initial_pair"]
    spec_rot, spec_pos = ua.align_errors(spec["poses"], scene, a, b)
    rot, pos = ua.align_errors({i: (ua.quat_to_rot(im["qvec"]), im["tvec"]) for i, im in model.images.items()}, scene, a, b)
    print(f"pair {model.initial_pair}, seed model {len(seed.images)} images, grown {len(model.images)} images in {model.rounds} rounds "
          f"(spec {spec['rounds']}), {len(model.points3D)} points (spec {len(spec['xyz'])}), mean track {model.mean_track_length():.2f}, "
          f"rotation {rot:.4f} deg (spec {spec_rot:.4f}), centre {pos:.5f} baselines (spec {spec_pos:.5f})")
    assert model.initial_pair == spec["initial_pair"] == seed.initial_pair and sorted(model.images) == sorted(spec["poses"])
    assert rot <= 2 * spec_rot and pos <= 2 * spec_pos
    assert abs(len(model.points3D) - len(spec["xyz"])) <= um.GROW_POINT_MARGIN
    for pid, p in seed.points3D.items():                                # the seed's points keep their ids and coordinates
        assert np.array_equal(model.points3D[pid]["xyz"], p["xyz"]) and model.points3D[pid]["track"][:2] == p["track"][:2]
    for p in model.points3D.values():
        assert len({i for i, _ in p["track"]}) == len(p["track"]) >= 2
    model.write_text(tmp_path / "sparse" / "grown")
    assert SparseModel.read_text(tmp_path / "sparse" / "grown") == model
    # building either model only reads: the rows are byte for byte what matching wrote
    assert _two_view_bytes(tmp_path / "w.db") == rows_before


def test_pipeline_with_the_flag_writes_the_grown_model_and_without_it_todays_output(tmp_path, monkeypatch):
    from vit_colmap_amd.pipeline import run_pipeline as rp
    from vit_colmap_amd.utils.config import Config

    class StubExtractor:
        device = "cuda"
        prior_focal_length = False

        def extract(self, image_dir, db_path, camera_model, camera_params):
            pass

    monkeypatch.setattr(rp.Pipeline, "_make_extractor", lambda self: StubExtractor())
    import vit_colmap_amd.mapping

    for name in ("grow", "triangulate"):        # restored with sys.modules, so that both name the same module for later tests
        if hasattr(vit_colmap_amd.mapping, name):
            monkeypatch.setattr(vit_colmap_amd.mapping, name, getattr(vit_colmap_amd.mapping, name))
        monkeypatch.delitem(sys.modules, "vit_colmap_amd.mapping." + name, raising=False)
    scene = um.windowed_scene()
    stats = {}
    for name, flags in (("off", (False, False)), ("seed", (True, False)), ("on", (False, True))):
        write_windowed_db(tmp_path / f"{name}.db", scene)
        cfg = Config()
        cfg.camera.prior_focal_length, cfg.matching.compute_relative_pose, cfg.do_reconstruction = True, True, False
        cfg.reconstruction.seed_model, cfg.reconstruction.sparse_model = flags
        p = rp.Pipeline(cfg)
        p.run(tmp_path / "images", tmp_path / name, tmp_path / f"{name}.db")
        stats[name] = p.last_stats
        if not flags[1]:                                               # with the flag off the growth is not imported
            assert "vit_colmap_amd.mapping.grow" not in sys.modules and "vit_colmap_amd.mapping.triangulate" not in sys.modules
    assert not (tmp_path / "off" / "sparse").exists() and "sparse_model" not in stats["off"] and "seed_model" not in stats["off"]
    assert [f.name for f in (tmp_path / "seed" / "sparse").iterdir()] == ["seed"] and "sparse_model" not in stats["seed"]
    assert [f.name for f in (tmp_path / "on" / "sparse").iterdir()] == ["grown"] and "seed_model" not in stats["on"]
    assert sorted(f.name for f in (tmp_path / "on" / "sparse" / "grown").iterdir()) == ["cameras.txt", "images.txt", "points3D.txt"]
    s = stats["on"]["sparse_model"]
    assert s["registered_images"] == 12 and s["rounds"] >= 2 and s["num_points3D"] > stats["seed"]["seed_model"]["num_points3D"]
    assert stats["seed"]["seed_model"]["registered_images"] < 12 and "rounds" not in stats["seed"]["seed_model"]
    assert {k: v for k, v in stats["on"].items() if k != "sparse_model"}.keys() == stats["off"].keys()
