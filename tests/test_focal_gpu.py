"""GPU tests of the focal-length estimate from the verified pairs: vc_focal_cost against the kernel's routine
compiled for the host (tools/focal_cost_host.cpp), byte for byte, on the sizes around its chunk of 256 pairs and its block of 16
candidates, with everything that can go wrong in a call, inside sentinel-filled buffers, two launches; the argument checks;
estimate_focal_lengths on the noisy rows of the skew scene; the pipeline end to end from a camera 30 % off."""
import numpy as np
import pytest
import torch

import util_absolute_pose as ua
import util_focal as uf
from test_focal_spec import focal_cost_host, skew  # noqa: F401 - the fixture
from test_mapper_gpu import write_windowed_db

pytestmark = pytest.mark.gpu

PAD = 64                                    # sentinel elements on either side of every output
FOCAL_MARGIN = 0.01                         # §4.2k's end-to-end condition on a refined focal, relative
DRIFT_MARGIN = 2.0                          # the project's margin on a drift against a reference run's (tests/test_mapper_gpu.py)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def launch(F, pair_cam, w, cams, ratios):
    """The raw entry point with its outputs inside sentinel-filled buffers -> out_cost, out_weight (numpy) and the buffers' bytes;
    asserts that nothing outside the outputs was written."""
    from vit_colmap_amd import _lib

    lib = _lib.load()
    n_pairs, n_cams, n_cand = len(pair_cam), len(cams), len(ratios)
    d = [dev(np.asarray(F, np.float64)), dev(np.asarray(pair_cam, np.int32)), dev(np.asarray(w, np.float64)), dev(np.asarray(cams, np.float64)),
         dev(np.asarray(ratios, np.float64))]
    bufs = dict(cost=torch.full((2 * PAD + n_cams * n_cand,), 7.0, dtype=torch.float64, device="cuda"),
                weight=torch.full((2 * PAD + n_cams,), 7.0, dtype=torch.float64, device="cuda"))
    inner = {k: b[PAD:len(b) - PAD] for k, b in bufs.items()}
    _lib.check(lib.vc_focal_cost(_lib.ptr(d[0]), _lib.ptr(d[1]), _lib.ptr(d[2]), n_pairs, _lib.ptr(d[3]), n_cams, _lib.ptr(d[4]), n_cand,
                                 _lib.ptr(inner["cost"]), _lib.ptr(inner["weight"]), _lib.stream_ptr()), "vc_focal_cost")
    torch.cuda.synchronize()
    host = {k: b.cpu().numpy() for k, b in bufs.items()}
    for k, b in host.items():
        assert (b[:PAD] == 7).all() and (b[len(b) - PAD:] == 7).all(), f"{k}: written outside the output"
    return host["cost"][PAD:-PAD].reshape(n_cams, n_cand), host["weight"][PAD:-PAD], b"".join(b.tobytes() for b in host.values())


@pytest.mark.parametrize("n_pairs,n_cand", [(1, 1), (63, 64), (65, 65), (257, 65), (1000, 65)])
def test_kernel_returns_the_host_builds_bytes(n_pairs, n_cand, focal_cost_host, tmp_path):  # noqa: F811
    """Two cameras interleaved throughout; from 64 candidates on the ratios NaN, -1, inf and 0; from 255 pairs on the slots -1,
    n_cams, -5 and 2^31 - 1, the NaN, zero and overflowing F and the weights 0, NaN and -3 (uf.call_case)."""
    case = uf.call_case(n_pairs, n_cand)
    cost, weight, raw = launch(*case)
    (host_cost, host_weight), _ = uf.run_host(focal_cost_host, tmp_path, *case)
    differing = int((cost.view(np.uint64) != host_cost.view(np.uint64)).sum())
    finite = np.isfinite(host_cost)
    print(f"{n_pairs} pairs, {n_cand} candidates: {differing} of {cost.size} costs differ in a bit from the host build, "
          f"worst relative difference {np.abs(cost[finite] / host_cost[finite] - 1).max() if finite.any() else 0.0:.3g}")
    assert cost.tobytes() == host_cost.tobytes() and weight.tobytes() == host_weight.tobytes()
    assert raw == launch(*case)[2]                                    # two launches, identical bytes
    if n_cand >= 64:
        assert np.isnan(cost[:, 1:5]).all() and np.isfinite(np.delete(cost, [1, 2, 3, 4], axis=1)).all()
    if n_pairs >= 255:
        counts = np.ones(n_pairs, bool)
        counts[[3, 40, 77, 254, 5, 8, 90, 10, 11, 12]] = False
        assert weight.tolist() == [case[2][counts & (case[1] == c)].sum() for c in (0, 1)]
    if n_pairs == 1:
        assert np.isnan(cost[1]).all() and weight[1] == 0 and np.isfinite(cost[0]).all()      # the camera without a pair


def test_no_camera_and_no_usable_pair():
    F, pair_cam, w, cams, ratios = uf.call_case(257, 65)
    cost, weight, _ = launch(F, np.full(257, -1, np.int32), w, cams, ratios)
    assert np.isnan(cost).all() and not weight.any()
    cost, weight, _ = launch(F, pair_cam, w, cams[:0], ratios)
    assert cost.shape == (0, 65) and weight.shape == (0,)


def test_argument_validation_returns_the_documented_codes_without_launching():
    from vit_colmap_amd import _lib

    lib = _lib.load()
    F, pair_cam, w, cams, ratios = uf.call_case(63, 64)
    d = [dev(F), dev(pair_cam), dev(w), dev(cams), dev(ratios)]
    out = [torch.full((2 * 64,), 7.0, dtype=torch.float64, device="cuda"), torch.full((2,), 7.0, dtype=torch.float64, device="cuda")]
    p, o = [_lib.ptr(t) for t in d], [_lib.ptr(t) for t in out]

    def call(p=p, n_pairs=63, n_cams=2, n_cand=64, o=o):
        return lib.vc_focal_cost(p[0], p[1], p[2], n_pairs, p[3], n_cams, p[4], n_cand, o[0], o[1], _lib.stream_ptr())

    assert call(n_pairs=0) == call(n_cand=0) == _lib.VC_OK
    assert call(p=[None] * 5, n_pairs=0, o=[None] * 2) == call(p=[None] * 5, n_cand=0, o=[None] * 2) == _lib.VC_OK
    for k in range(5):
        assert call(p=p[:k] + [None] + p[k + 1:]) == _lib.VC_ERR_INVALID_ARG, k
    for k in range(2):
        assert call(o=o[:k] + [None] + o[k + 1:]) == _lib.VC_ERR_INVALID_ARG, k
    assert call(n_pairs=-1) == call(n_cams=-1) == call(n_cand=-1) == _lib.VC_ERR_INVALID_ARG
    assert call(p=p[:3] + [None] + p[4:], n_cams=0, o=[None] * 2) == _lib.VC_OK       # no camera: no row to write
    assert call(n_cand=16 * 65535 + 1) == _lib.VC_ERR_UNSUPPORTED
    assert call(n_pairs=2 ** 31 - 1, n_cams=2 ** 20, n_cand=64) == _lib.VC_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert (out[0] == 7.0).all() and (out[1] == 7.0).all()              # nothing was launched
    # the front end refuses wrong dtypes, devices and shapes
    from vit_colmap_amd.matching.focal import focal_cost

    for bad in ([d[0].float()] + d[1:], [d[0], d[1].long()] + d[2:], [t.cpu() for t in d], d[:3] + [d[3][:, :3]] + d[4:], [d[0][:5]] + d[1:]):
        with pytest.raises(ValueError, match="focal_cost needs"):
            focal_cost(*bad)
    cost, weight = focal_cost(d[0][:0], d[1][:0], d[2][:0], d[3], d[4])
    assert torch.isnan(cost).all() and cost.shape == (2, 64) and not weight.any()


def test_estimate_focal_lengths_on_the_noisy_rows_is_the_specifications_estimate(tmp_path):
    """The device's bound is 2 x SPEC_NOISY_REL, as in §4.2m: the two paths differ only in rounding.  Measured (1x MI355X): see
    DESIGN.md §4.2o."""
    from vit_colmap_amd.database import ColmapDatabase
    from vit_colmap_amd.matching.focal import apply_focal_estimates, estimate_focal_lengths

    scene, _, (F, w) = skew()
    cid = uf.write_rows_db(tmp_path / "noisy.db", scene, 1.3, F, w)
    spec = uf.estimate_ratio(F, w, uf.camera_of(scene, 1.3))
    with ColmapDatabase.open_database(str(tmp_path / "noisy.db")) as db:
        ids = [im.image_id for im in db.read_all_images()]
        e = estimate_focal_lengths(db, ids, "cuda")[cid]
        assert apply_focal_estimates(db, {cid: e}) == [cid]
        assert db.read_camera(cid).params[:2] == list(e["focal"]) and db.read_camera(cid).has_prior_focal_length
    rel = abs(e["ratio"] * 1.3 - 1)
    print(f"r* {e['ratio']:.9f} for {1 / 1.3:.9f}: relative error {rel:.3g} (specification {abs(spec['ratio'] * 1.3 - 1):.3g}, "
          f"r* differs from its by {abs(e['ratio'] / spec['ratio'] - 1):.3g}), cost {e['cost_min']:.4g}, median {e['cost_median']:.4g}")
    assert e["reason"] is None and e["pairs"] == len(F) and e["weight"] == w.sum()
    assert rel <= 2 * uf.SPEC_NOISY_REL
    assert e["ratio"] == spec["ratio"] and e["cost_min"] == spec["cost_min"]     # the kernel returns the specification's bytes


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
class StubExtractor:
    device = "cuda"
    prior_focal_length = False

    def extract(self, image_dir, db_path, camera_model, camera_params):
        pass


def run_pipeline(directory, name, scene, flagged, **camera):
    """The scene's database (the camera flagged or not) through Pipeline.run with --relative-pose --sparse-model
    --bundle-adjustment --refine-focal-length and the given camera options -> the pipeline, the output directory."""
    from vit_colmap_amd.database import ColmapDatabase
    from vit_colmap_amd.pipeline import run_pipeline as rp
    from vit_colmap_amd.utils.config import Config

    write_windowed_db(directory / f"{name}.db", scene)
    if not flagged:
        with ColmapDatabase.open_database(str(directory / f"{name}.db")) as db:
            db.update_camera(1, db.read_camera(1).params, False)
    cfg = Config()
    cfg.matching.compute_relative_pose, cfg.do_reconstruction = True, False
    cfg.reconstruction.sparse_model, cfg.reconstruction.bundle_adjustment, cfg.reconstruction.refine_focal_length = True, True, True
    for k, v in camera.items():
        setattr(cfg.camera, k, v)
    p = rp.Pipeline(cfg)
    p.run(directory / "images", directory / name, directory / f"{name}.db")
    return p, directory / name


def test_pipeline_end_to_end_from_a_camera_30_percent_off(tmp_path, monkeypatch):
    """The skew scene's database with the camera at 780 for 600 and no prior, under --estimate-focal-length, against the same
    run from the true camera under --prior-focal-length, which is the reference.  The adjusted focal may differ from the
    reference run's by FOCAL_MARGIN, §4.2k's condition on a focal refined from 3 % off; the drift may be DRIFT_MARGIN times the
    reference run's, the margin this suite gives a model's drift against a reference's.  Figures: DESIGN.md §4.2o."""
    from vit_colmap_amd.mapping import SparseModel
    from vit_colmap_amd.pipeline import run_pipeline as rp

    monkeypatch.setattr(rp.Pipeline, "_make_extractor", lambda self: StubExtractor())
    scene = uf.skew_scene()
    off = uf.off_scene(scene, 1.3)
    ref, ref_dir = run_pipeline(tmp_path, "ref", scene, True, prior_focal_length=True)
    est, est_dir = run_pipeline(tmp_path, "est", off, False, estimate_focal_length=True)
    # without the option the same command is refused before any work, as today: no sparse/
    with pytest.raises(ValueError, match="sparse_model needs camera.prior_focal_length"):
        run_pipeline(tmp_path, "without", off, False)
    assert not (tmp_path / "without" / "sparse").exists()
    # for the record (printed, not asserted): the same wrong camera declared trusted instead, --prior-focal-length without the option
    trusted, trusted_dir = run_pipeline(tmp_path, "trusted", off, True, prior_focal_length=True)
    if (trusted_dir / "sparse" / "adjusted").exists():
        t = SparseModel.read_text(trusted_dir / "sparse" / "adjusted")
        a, b = trusted.last_stats["sparse_model"]["initial_pair"]
        t_drift = ua.align_errors({i: (ua.quat_to_rot(im["qvec"]), im["tvec"]) for i, im in t.images.items()}, scene, a, b)
        print(f"780 declared trusted: {len(t.images)} images, {len(t.points3D)} points, focal {[round(float(v), 3) for v in list(t.cameras.values())[0].params[:2]]}, "
              f"drift {t_drift[0]:.4f} deg / {t_drift[1]:.5f} baselines, {trusted.last_stats['bundle_adjustment']['bundle_adjustment']['iterations']} linearisations")
    else:
        print(f"780 declared trusted: no adjusted model ({sorted(trusted.last_stats)})")

    def figures(directory):
        m = SparseModel.read_text(directory / "sparse" / "adjusted")
        (cam,) = m.cameras.values()
        return m, [float(v) for v in cam.params[:2]]

    (m_ref, f_ref), (m_est, f_est) = figures(ref_dir), figures(est_dir)
    drift = {}
    for name, p, m in (("ref", ref, m_ref), ("est", est, m_est)):
        a, b = p.last_stats["sparse_model"]["initial_pair"]
        drift[name] = ua.align_errors({i: (ua.quat_to_rot(im["qvec"]), im["tvec"]) for i, im in m.images.items()}, scene, a, b)
    (cid, e), = est.last_stats["focal_estimates"].items()
    print(f"estimate: r* {e['ratio']:.6f} for {1 / 1.3:.6f} ({abs(e['ratio'] * 1.3 - 1):.3%} off), focal {e['focal'][0]:.3f}, {e['pairs']} pairs, cost "
          f"{e['cost_min']:.4g}, median {e['cost_median']:.4g}; {est.last_stats['focal_reverified_pairs']} pairs verified again")
    print(f"adjusted focal: reference {f_ref[0]:.4f} {f_ref[1]:.4f}, estimated {f_est[0]:.4f} {f_est[1]:.4f} "
          f"({abs(f_est[0] / f_ref[0] - 1):.3%}, {abs(f_est[1] / f_ref[1] - 1):.3%} apart)")
    print(f"linearisations: reference {ref.last_stats['bundle_adjustment']['bundle_adjustment']['iterations']}, estimated "
          f"{est.last_stats['bundle_adjustment']['bundle_adjustment']['iterations']}")
    print(f"drift: reference {drift['ref'][0]:.4f} deg / {drift['ref'][1]:.5f} baselines, estimated {drift['est'][0]:.4f} deg / {drift['est'][1]:.5f} baselines; "
          f"{len(m_ref.points3D)} and {len(m_est.points3D)} points")
    assert sorted(m_est.images) == sorted(m_ref.images) == list(range(1, 13))
    assert e["reason"] is None and "focal_estimates" not in ref.last_stats
    for got, want in zip(f_est, f_ref):
        assert abs(got / want - 1) <= FOCAL_MARGIN
    assert drift["est"][0] <= DRIFT_MARGIN * drift["ref"][0] and drift["est"][1] <= DRIFT_MARGIN * drift["ref"][1]
