"""GPU tests of the matrix-free solver of bundle adjustment ("The solver" in DESIGN.md §4.2k): vc_ba_camera_blocks and
vc_ba_schur_product against the same routines compiled for the host (tools/bundle_pcg_host.cpp), byte for byte, on the shapes at
which they can go wrong and above the dense route's 512 cameras, inside sentinel-filled buffers; two launches; malformed offsets;
the argument checks; the front end's pcg loop against the specification of tests/util_bundle_pcg.py and against the dense loop on
the same device; a 520-camera arc that the dense solver refuses; the pipeline's step end to end."""
from functools import lru_cache

import numpy as np
import pytest
import torch

import util_absolute_pose as ua
import util_bundle as ub
import util_bundle_loss as ul
import util_bundle_pcg as up
import util_mapper as um
from test_absolute_pose_gpu import _two_view_bytes
from test_bundle_gpu import PAD, SHAPES, dev, problem_of
from test_bundle_pcg_spec import bundle_pcg_host, run_host, windowed_pcg  # noqa: F401 - the fixture
from test_bundle_spec import BA_POS_BOUND, BA_ROT_BOUND, adjusted
from test_mapper_gpu import write_windowed_db

pytestmark = pytest.mark.gpu

ABOVE_THE_CAP = (257, 513)                  # (points, cameras): the first camera count vc_ba_reduce_cameras refuses
# the front end's pcg loop against the specification's, measured relative differences of the final cost; every bound is 4x.
# The two run the same recurrence with the dot products summed in different orders (torch's on the device, numpy's) to
# |r| <= 1e-6 |r_0|, and at the minimum the cost does not move with the step to first order.
LOOP_SPEC_REL = 7.41e-16                    # the windowed problem: the same decisions and the same products per solve, [47, 47, 48, 47, 48]
LOOP_DENSE_REL = 1.48e-15                   # against bundle_adjust(solver="dense") on the same device
LOOP_HUBER_REL = 3.14e-15                   # the corrupted windowed problem under Huber 1 px: 24 accepted steps of 24
# the 520-camera arc after ARC_MAX_ITERATIONS linearisations: of its four solves three are cut at 500 products (a chain of 520
# cameras under a damping that falls is what block Jacobi preconditions worst), the first ends after 425 where the specification's
# ends after 424, and no step ends at a minimum, so the two recurrences' roundings reach the cost to first order
ARC_SPEC_REL = 1.13e-9
TORCH_OF = {"f8": torch.float64, "u1": torch.uint8}
BLOCKS = dict(U=("f8", 36), D=("f8", 36), Minv=("f8", 36), g=("f8", 6), fixed=("u1", 6))


def vectors_of(problem, seed=5):
    """Two p: one non-zero everywhere (at held parameters and at the NaN row's too), one a small step that is 0 where held."""
    mask = problem[5]
    p = np.random.RandomState(seed).normal(0, 1, (2, 6 * len(mask)))
    p[1] = np.where(np.array([[(int(m) >> i) & 1 for i in range(6)] for m in mask]).reshape(-1), 0.0, 2e-3 * p[1])
    return p


def launch(problem, lam, vectors, index=None, loss=(0, 1.0)):
    """The points pass of the linearisation into plain buffers, then the two entry points with every output inside a sentinel-filled
    buffer -> {name: numpy array} in the host program's layout and all buffers' bytes; asserts that no sentinel was touched."""
    from vit_colmap_amd import _lib

    lib = _lib.load()
    cams, points, offsets, obs_cam, obs_xy, mask = problem
    c, n, t = len(cams), len(points), len(obs_cam)
    index = index or ub.camera_index(obs_cam, offsets, c)
    d_cams, d_points, d_offsets, d_obs_cam, d_obs_xy, d_mask = dev(cams), dev(points), dev(offsets), dev(obs_cam), dev(obs_xy), dev(mask)
    x = [dev(np.asarray(a, np.int32)) for a in index]
    f64 = dict(dtype=torch.float64, device="cuda")
    vinv, gp, cost, total_cost = torch.zeros(6 * n, **f64), torch.zeros(3 * n, **f64), torch.zeros(n, **f64), torch.zeros(1, **f64)
    count, obs_ok = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(t, dtype=torch.uint8, device="cuda")
    obs_lin, obs_w = torch.zeros(32 * t, **f64), torch.zeros(t, **f64)
    p, stream = _lib.ptr, _lib.stream_ptr()
    if loss[0] == 0:
        _lib.check(lib.vc_ba_linearize_points(p(d_cams), c, p(d_mask), p(d_points), n, p(d_offsets), p(d_obs_cam), p(d_obs_xy), t, lam, p(vinv),
                                              p(gp), p(cost), p(count), p(obs_ok), p(obs_lin), p(total_cost), stream), "vc_ba_linearize_points")
    else:
        _lib.check(lib.vc_ba_linearize_points_loss(p(d_cams), c, p(d_mask), p(d_points), n, p(d_offsets), p(d_obs_cam), p(d_obs_xy), t, lam,
                                                   loss[0], loss[1], p(vinv), p(gp), p(cost), p(count), p(obs_ok), p(obs_lin), p(obs_w),
                                                   p(total_cost), stream), "vc_ba_linearize_points_loss")

    def padded(kind, size):
        return torch.full((2 * PAD + size,), 7, dtype=TORCH_OF[kind], device="cuda")

    bufs = {k: padded(kind, per * c) for k, (kind, per) in BLOCKS.items()}
    o = {k: p(b[PAD:len(b) - PAD]) for k, b in bufs.items()}
    _lib.check(lib.vc_ba_camera_blocks(c, p(d_mask), n, p(d_offsets), p(d_obs_cam), t, p(x[0]), p(x[1]), p(x[2]), lam, p(vinv), p(gp), p(obs_ok),
                                       p(obs_lin), o["U"], o["D"], o["Minv"], o["g"], o["fixed"], stream), "vc_ba_camera_blocks")
    for v, vector in enumerate(vectors):
        d_p = dev(vector)
        bufs[f"s{v}"], bufs[f"q{v}"] = padded("f8", 3 * n), padded("f8", 6 * c)
        _lib.check(lib.vc_ba_schur_product(c, n, p(d_offsets), p(d_obs_cam), t, p(x[0]), p(x[1]), p(x[2]), p(vinv), p(obs_ok), p(obs_lin),
                                           o["U"], o["fixed"], p(d_p), p(bufs[f"s{v}"][PAD:PAD + 3 * n]), p(bufs[f"q{v}"][PAD:PAD + 6 * c]), stream),
                   "vc_ba_schur_product")
    torch.cuda.synchronize()
    host = {k: b.cpu().numpy() for k, b in bufs.items()}
    for k, b in host.items():
        assert (b[:PAD] == 7).all() and (b[len(b) - PAD:] == 7).all(), f"{k}: written outside the output"
    got = {k: b[PAD:len(b) - PAD] for k, b in host.items()}
    got["s"] = np.stack([got.pop(f"s{v}") for v in range(len(vectors))]) if len(vectors) else np.zeros((0, 3 * n))
    got["q"] = np.stack([got.pop(f"q{v}") for v in range(len(vectors))]) if len(vectors) else np.zeros((0, 6 * c))
    got["vinv"], got["total_cost"], got["obs_ok"] = vinv.cpu().numpy(), total_cost.cpu().numpy(), obs_ok.cpu().numpy()
    return got, b"".join(b.tobytes() for b in host.values())


def assert_bytes_equal(got, host, what):
    for k in ("vinv", "total_cost", "obs_ok", "U", "D", "Minv", "g", "fixed", "s", "q"):
        assert got[k].tobytes() == np.ascontiguousarray(host[k]).tobytes(), f"{what}: {k} differs from the host build"


@pytest.mark.parametrize("n_points,n_cams", SHAPES + [ABOVE_THE_CAP])
def test_kernels_return_the_host_builds_bytes(n_points, n_cams, bundle_pcg_host, tmp_path):  # noqa: F811
    from vit_colmap_amd import _lib

    problem = problem_of(n_points, n_cams)
    vectors = vectors_of(problem)
    got, raw = launch(problem, ub.BA_LAMBDA0, vectors)
    host, _ = run_host(bundle_pcg_host, tmp_path, problem, ub.BA_LAMBDA0, vectors)
    assert_bytes_equal(got, host, f"{n_points} points, {n_cams} cameras")
    _, raw2 = launch(problem, ub.BA_LAMBDA0, vectors)
    assert raw == raw2                                                # two launches, identical bytes
    fixed = got["fixed"].reshape(n_cams, 6).astype(bool)
    eye = np.eye(6).reshape(36)
    assert fixed[0].all() and fixed[n_cams - 1].all()                 # the held camera and the NaN row
    for a in (0, n_cams - 1):
        assert all(np.array_equal(got[k].reshape(n_cams, 36)[a], eye) for k in ("U", "D", "Minv")) and not got["g"][6 * a:6 * a + 6].any()
    assert np.isfinite(got["q"]).all() and np.isfinite(got["s"]).all() and np.isfinite(got["Minv"]).all()
    assert np.array_equal(got["q"][0][fixed.reshape(-1)], vectors[0][fixed.reshape(-1)])          # q_i = p_i at a fixed parameter
    if n_cams > 2:
        assert list(fixed[1]) == [False, False, True, False, True, False]                          # the partly held one
    if n_cams > _lib.VC_BA_MAX_CAMS:
        assert (~fixed).sum() > 6 * _lib.VC_BA_MAX_CAMS // 2 and got["q"][0][~fixed.reshape(-1)].any()
    if n_points >= 63:
        assert (got["obs_ok"] == 0).sum() >= n_points // 10 and not got["s"][0].reshape(-1, 3)[1:3].any()     # the constant points


def test_batch_seams_of_both_camera_passes(bundle_pcg_host, tmp_path):  # noqa: F811
    problem = up.lists_problem()
    assert tuple(np.bincount(problem[3], minlength=len(up.LISTS))) == up.LISTS
    vectors = vectors_of(problem)
    got, raw = launch(problem, ub.BA_LAMBDA0, vectors)
    host, _ = run_host(bundle_pcg_host, tmp_path, problem, ub.BA_LAMBDA0, vectors)
    assert_bytes_equal(got, host, "lists of " + ", ".join(map(str, up.LISTS)))
    assert raw == launch(problem, ub.BA_LAMBDA0, vectors)[1]
    assert got["obs_ok"].all() and np.isfinite(got["q"]).all() and got["q"][1][:48].all()


def test_huber_linearisation_goes_through_both_entry_points_unchanged(bundle_pcg_host, tmp_path):  # noqa: F811
    problem = problem_of(65, 12)
    vectors = vectors_of(problem)
    got, _ = launch(problem, ub.BA_LAMBDA0, vectors, loss=(ul.HUBER, 1.0))
    host, _ = run_host(bundle_pcg_host, tmp_path, problem, ub.BA_LAMBDA0, vectors, loss=(ul.HUBER, 1.0))
    assert_bytes_equal(got, host, "huber")
    plain, _ = launch(problem, ub.BA_LAMBDA0, vectors)
    assert not np.array_equal(plain["q"], got["q"])


def test_offsets_that_delimit_nothing_skip_their_point_or_camera(bundle_pcg_host, tmp_path):  # noqa: F811
    cams, points, offsets, obs_cam, obs_xy, mask = problem_of(65, 12)
    offsets = offsets.copy()
    total = len(obs_cam)
    offsets[11], offsets[20], offsets[-1] = total + 50, -4, total + 9   # points 10 and 64 pass the arrays, 11 and 19 descend, 20 begins below 0
    problem = (cams, points, offsets, obs_cam, obs_xy, mask)
    index = [a.copy() for a in ub.camera_index(obs_cam, offsets, len(cams))]
    index[0][4] = index[0][5] + 1                                     # camera 4's list descends; camera 3's now runs into its neighbours'
    index[1][index[0][7]] = total + 100                               # an entry of camera 7's list names no observation
    index[2][int(index[1][index[0][8]])] = len(points) + 7            # the point of an observation of camera 8 is past the table
    vectors = vectors_of(problem)
    got, raw = launch(problem, ub.BA_LAMBDA0, vectors, index)
    host, _ = run_host(bundle_pcg_host, tmp_path, problem, ub.BA_LAMBDA0, vectors, index)
    assert_bytes_equal(got, host, "bad offsets")                      # the same bytes wherever anything is written
    assert raw == launch(problem, ub.BA_LAMBDA0, vectors, index)[1]
    for j in (10, 11, 19, 20, 64):
        assert not got["s"][0].reshape(-1, 3)[j].any()
    eye = np.eye(6).reshape(36)
    assert all(np.array_equal(got[k].reshape(-1, 36)[4], eye) for k in ("U", "D", "Minv")) and got["fixed"][24:30].all()     # the skipped camera
    assert np.array_equal(got["q"][0][24:30], vectors[0][24:30]) and np.isfinite(got["q"]).all()


def test_argument_validation_returns_the_documented_codes_without_launching():
    from vit_colmap_amd import _lib

    lib = _lib.load()
    cams, points, offsets, obs_cam, obs_xy, mask = problem_of(63, 3)
    c, n, t = len(cams), len(points), len(obs_cam)
    i = [_lib.ptr(dev(a)) for a in (mask, offsets, obs_cam)]
    x = [_lib.ptr(dev(a)) for a in ub.camera_index(obs_cam, offsets, c)]
    f64 = dict(dtype=torch.float64, device="cuda")
    lin_bufs = [torch.zeros(6 * n, **f64), torch.zeros(3 * n, **f64), torch.zeros(t, dtype=torch.uint8, device="cuda"), torch.zeros(32 * t, **f64)]
    lin = [_lib.ptr(b) for b in lin_bufs]
    bufs = {k: torch.full((per * c,), 7, dtype=TORCH_OF[kind], device="cuda") for k, (kind, per) in BLOCKS.items()}
    bufs.update(p=torch.full((6 * c,), 7, **f64), s=torch.full((3 * n,), 7, **f64), q=torch.full((6 * c,), 7, **f64))
    o = {k: _lib.ptr(b) for k, b in bufs.items()}
    stream = _lib.stream_ptr()

    def blk(i=i, x=x, c=c, n=n, t=t, lam=1e-4, lin=lin, o=o):
        return lib.vc_ba_camera_blocks(c, i[0], n, i[1], i[2], t, x[0], x[1], x[2], lam, lin[0], lin[1], lin[2], lin[3], o["U"], o["D"], o["Minv"],
                                       o["g"], o["fixed"], stream)

    def prod(i=i, x=x, c=c, n=n, t=t, lin=lin, o=o):
        return lib.vc_ba_schur_product(c, n, i[1], i[2], t, x[0], x[1], x[2], lin[0], lin[2], lin[3], o["U"], o["fixed"], o["p"], o["s"], o["q"],
                                       stream)

    nothing = {k: None for k in o}
    assert blk(i=[None] * 3, x=[None] * 3, c=0, lin=[None] * 4, o=nothing) == _lib.VC_OK
    assert prod(i=[None] * 3, x=[None] * 3, c=0, lin=[None] * 4, o=nothing) == _lib.VC_OK
    for k in range(3):
        assert blk(i=i[:k] + [None] + i[k + 1:]) == _lib.VC_ERR_INVALID_ARG, k
        assert blk(x=x[:k] + [None] + x[k + 1:]) == prod(x=x[:k] + [None] + x[k + 1:]) == _lib.VC_ERR_INVALID_ARG, k
    for k in (1, 2):
        assert prod(i=i[:k] + [None] + i[k + 1:]) == _lib.VC_ERR_INVALID_ARG, k
    for k in range(4):
        assert blk(lin=lin[:k] + [None] + lin[k + 1:]) == _lib.VC_ERR_INVALID_ARG, k
    for k in (0, 2, 3):
        assert prod(lin=lin[:k] + [None] + lin[k + 1:]) == _lib.VC_ERR_INVALID_ARG, k
    for k in BLOCKS:
        assert blk(o=dict(o, **{k: None})) == _lib.VC_ERR_INVALID_ARG, k
    for k in ("U", "fixed", "p", "s", "q"):
        assert prod(o=dict(o, **{k: None})) == _lib.VC_ERR_INVALID_ARG, k
    for size in ("c", "n", "t"):
        assert blk(**{size: -1}) == prod(**{size: -1}) == _lib.VC_ERR_INVALID_ARG, size
    for bad in (-1.0, float("nan"), float("inf")):
        assert blk(lam=bad) == _lib.VC_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert all((b == 7).all() for b in bufs.values())                 # nothing was launched


def test_bundle_adjust_pcg_follows_the_specification_and_the_dense_loop_on_the_windowed_problem():
    from vit_colmap_amd.mapping.bundle import bundle_adjust

    scene, _, grown, problem, adj = adjusted()
    ids, (before, _, mask) = problem[0], adj["held"]
    cams, points, report = bundle_adjust(*problem[1:], mask, "cuda", solver="pcg")
    _, _, dense = bundle_adjust(*problem[1:], mask, "cuda")
    spec = windowed_pcg()[2]
    rel = abs(report["final_cost"] - spec["final_cost"]) / spec["final_cost"]
    rel_dense = abs(report["final_cost"] - dense["final_cost"]) / dense["final_cost"]
    print(f"decisions {report['decisions']} (spec {spec['decisions']}, dense {dense['decisions']}), final cost {report['final_cost']:.12g} "
          f"(spec {spec['final_cost']:.12g}: {rel:.3g}; dense {dense['final_cost']:.12g}: {rel_dense:.3g}), pcg iterations "
          f"{report['pcg_iterations']} (spec {spec['pcg_iterations']})")
    assert report["decisions"] == spec["decisions"] and report["iterations"] == spec["iterations"]
    assert report["final_lambda"] == spec["final_lambda"] and report["initial_cost"] == spec["initial_cost"]
    assert report["solver"] == "pcg" and len(report["pcg_iterations"]) == len(report["decisions"]) and "solver" not in dense
    assert sorted(set(report) - set(dense)) == ["pcg_iterations", "solver"] and report["decisions"] == dense["decisions"]
    assert rel <= 4 * LOOP_SPEC_REL and rel_dense <= 4 * LOOP_DENSE_REL
    a, b = (ids.index(i) for i in grown["initial_pair"])
    k = int(mask[b]).bit_length() - 1
    assert np.array_equal(cams[a], before[a]) and cams[b, 9 + k - 3] == before[b, 9 + k - 3] and np.array_equal(cams[:, 12:], before[:, 12:])
    scaled, _ = ub.rescale(cams, points, a, b)
    rot, pos = ua.align_errors({i: (scaled[s, :9].reshape(3, 3), scaled[s, 9:12]) for s, i in enumerate(ids)}, scene, *grown["initial_pair"])
    print(f"rotation {rot:.4f} deg, centre {pos:.5f} baselines")
    assert rot <= BA_ROT_BOUND and pos <= BA_POS_BOUND


@lru_cache(maxsize=None)
def huber_spec():
    problem = ul.corrupted_windowed_problem()[0]
    return up.bundle_adjust(*problem, linearize=lambda *a: ul.linearize(*a, ul.HUBER, 1.0))[2]


def test_bundle_adjust_pcg_under_huber_takes_the_specifications_decisions():
    from vit_colmap_amd.mapping.bundle import bundle_adjust

    problem = ul.corrupted_windowed_problem()[0]
    _, _, report = bundle_adjust(*problem, "cuda", loss="huber", loss_scale=1.0, solver="pcg")
    spec = huber_spec()
    rel = abs(report["final_cost"] - spec["final_cost"]) / spec["final_cost"]
    print(f"decisions {report['decisions']} (spec {spec['decisions']}), final cost {report['final_cost']:.12g} (spec {spec['final_cost']:.12g}: "
          f"{rel:.3g}), pcg iterations {report['pcg_iterations']} (spec {spec['pcg_iterations']})")
    assert report["decisions"] == spec["decisions"] and report["iterations"] == spec["iterations"] and report["loss"] == "huber"
    assert rel <= 4 * LOOP_HUBER_REL


def test_an_arc_of_520_cameras_is_refused_by_the_dense_solver_and_adjusted_by_pcg():
    """The test that fails without the solver."""
    from vit_colmap_amd.mapping.bundle import bundle_adjust

    problem = up.arc_problem()
    assert len(problem[0]) == 520
    with pytest.raises(ValueError, match="VC_BA_MAX_CAMS"):
        bundle_adjust(*problem, "cuda", solver="dense")
    _, _, report = bundle_adjust(*problem, "cuda", max_iterations=up.ARC_MAX_ITERATIONS, solver="pcg")
    spec = up.arc_spec()[2]
    rel = abs(report["final_cost"] - spec["final_cost"]) / spec["final_cost"]
    print(f"cost {report['initial_cost']:.6g} -> {report['final_cost']:.12g} (spec {spec['final_cost']:.12g}: {rel:.3g}), decisions "
          f"{report['decisions']} (spec {spec['decisions']}), pcg iterations {report['pcg_iterations']} (spec {spec['pcg_iterations']})")
    assert report["initial_cost"] == spec["initial_cost"] and report["final_cost"] < 0.5 * report["initial_cost"]
    assert report["decisions"] == spec["decisions"] and rel <= 4 * ARC_SPEC_REL


def test_pipeline_step_with_the_pcg_solver_end_to_end(tmp_path):
    from vit_colmap_amd.mapping import SparseModel
    from vit_colmap_amd.mapping.bundle import build_adjusted_model
    from vit_colmap_amd.mapping.grow import build_sparse_model
    from vit_colmap_amd.matching import match_exhaustive
    from vit_colmap_amd.pipeline import run_pipeline as rp
    from vit_colmap_amd.utils.config import Config, MatchingConfig

    scene = um.windowed_scene()
    write_windowed_db(tmp_path / "w.db", scene)
    match_exhaustive(database_path=str(tmp_path / "w.db"), matching_options=MatchingConfig(compute_relative_pose=True).to_matching_options())
    rows_before = _two_view_bytes(tmp_path / "w.db")
    cfg = Config()
    cfg.reconstruction.ba_solver = "pcg"
    step = rp.Pipeline(cfg)
    step.last_stats = {}
    step._write_sparse_model(tmp_path / "w.db", tmp_path / "out", "cuda", adjust=True, solver=cfg.reconstruction.ba_solver)
    assert sorted(f.name for f in (tmp_path / "out" / "sparse").iterdir()) == ["adjusted", "grown"]
    model, grown = (SparseModel.read_text(tmp_path / "out" / "sparse" / n) for n in ("adjusted", "grown"))
    assert sorted(model.images) == list(range(1, 13))
    ba = step.last_stats["bundle_adjustment"]["bundle_adjustment"]
    assert ba["solver"] == "pcg" and ba["accepted_steps"] <= len(ba["pcg_iterations"]) <= ba["iterations"] - 1

    pair = step.last_stats["sparse_model"]["initial_pair"]           # a model read from text does not carry it

    def drift(m):
        return ua.align_errors({i: (ua.quat_to_rot(im["qvec"]), im["tvec"]) for i, im in m.images.items()}, scene, *pair)

    (rot0, pos0), (rot, pos) = drift(grown), drift(model)
    print(f"rotation {rot0:.4f} -> {rot:.4f} deg, centre {pos0:.5f} -> {pos:.5f} baselines, cost {ba['initial_cost']:.2f} -> {ba['final_cost']:.2f}, "
          f"pcg iterations {ba['pcg_iterations']}")
    assert rot <= rot0 / 4 and pos <= pos0 / 4 and rot <= BA_ROT_BOUND and pos <= BA_POS_BOUND and ba["final_cost"] < ba["initial_cost"]
    assert _two_view_bytes(tmp_path / "w.db") == rows_before          # the database rows are byte for byte what matching wrote
    # without the flag: the dense calls and the dense report's keys, on the same grown model within the solve's tolerance
    again = build_sparse_model(tmp_path / "w.db")
    dense, pcg = build_adjusted_model(tmp_path / "w.db", grown=again), build_adjusted_model(tmp_path / "w.db", grown=again, solver="pcg")
    keys = {"iterations", "accepted_steps", "initial_cost", "final_cost", "final_lambda", "filtered_observations", "filtered_points"}
    assert set(dense.stats()["bundle_adjustment"]) == keys and set(pcg.stats()["bundle_adjustment"]) == keys | {"solver", "pcg_iterations"}
    assert sorted(dense.points3D) == sorted(pcg.points3D) and dense.stats()["bundle_adjustment"]["initial_cost"] == pcg.stats()["bundle_adjustment"]["initial_cost"]
    assert abs(pcg.stats()["bundle_adjustment"]["final_cost"] / dense.stats()["bundle_adjustment"]["final_cost"] - 1) <= 4 * LOOP_DENSE_REL
