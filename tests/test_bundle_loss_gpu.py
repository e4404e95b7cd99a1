"""GPU tests of bundle adjustment under a robust loss ("The loss"): vc_ba_linearize_points_loss,
vc_ba_linearize_intrinsics_loss and vc_ba_reduce_border_loss, and vc_ba_reduce_cameras, vc_ba_step and vc_ba_step_intrinsics on
their outputs, against the same routines compiled for the host (tools/bundle_host.cpp), byte for byte, on the problems of
tests/test_bundle_gpu.py with every seventh observation 20 px off and one residual of exactly 0, inside sentinel-filled buffers;
two launches; the trivial loss against the entry point without a loss; the argument checks; the front end's loop against the
specification of tests/util_bundle_loss.py on the corrupted windowed problem; the pipeline's flags end to end."""
from functools import lru_cache

import numpy as np
import pytest
import torch

import util_bundle as ub
import util_bundle_loss as ul
import util_mapper as um
from test_bundle_gpu import OUTPUTS, PAD, TORCH_OF, dev, problem_of, step_of
from test_bundle_gpu import launch as launch_plain
from test_bundle_intr_gpu import SHAPES, groups_of, theta_step
from test_bundle_intr_spec import tied_groups, with_focal
from test_bundle_loss_spec import run_host_loss
from test_bundle_spec import bundle_host, result_shapes  # noqa: F401 - the fixture
from test_mapper_gpu import write_windowed_db

pytestmark = pytest.mark.gpu

LOSSES = [(ul.HUBER, 1.0), (ul.SOFT_L1, 1.0)]
# the final cost of the front end's loop on the corrupted windowed problem against the specification's, relative, under the cap
# of 25 linearisations (10 with the tied group), where the robust loop is still taking steps (the two loops solve the system
# with different factorisations, torch's on the device and numpy's, and every step carries that difference on), measured on an
# MI355X: Huber 1 px 3.92e-16 (costs 4634.92467351), with one tied focal group from 1.03 f 1.96e-16 (4639.02642408): one and two
# units in the last place of the cost; the bounds are 4x, rounded up
LOOP_COST_REL, LOOP_COST_REL_TIED = 1.6e-15, 8e-16


@lru_cache(maxsize=None)
def loss_problem(n_points, n_cams):
    """test_bundle_gpu.problem_of with every seventh observation displaced by 20 px (12, 16), so that both branches of Huber
    occur within a wave, and the first usable observation that is not displaced moved onto its projection: a residual of
    exactly 0 -> problem, the observation's index."""
    cams, points, offsets, obs_cam, obs_xy, mask = problem_of(n_points, n_cams)
    obs_xy = obs_xy.copy()
    obs_xy[::7] += [12.0, 16.0]
    lin = ub.linearize(cams, points, offsets, obs_cam, obs_xy, mask, ub.BA_LAMBDA0)
    zero = next(o for o in range(len(obs_cam)) if lin["ok"][o] and o % 7)
    j = int(np.searchsorted(offsets, zero, side="right") - 1)
    obs_xy[zero] = ub.observe(cams[obs_cam[zero]], points[j], np.zeros(2))[1]       # r = projection - 0 in the kernel's order
    return (cams, points, offsets, obs_cam, obs_xy, mask), zero


def launch(problem, groups, lam, dc, dtheta, loss, scale, index=None):
    """vc_ba_linearize_points_loss, vc_ba_reduce_cameras, vc_ba_step, then vc_ba_linearize_intrinsics_loss,
    vc_ba_reduce_border_loss and vc_ba_step_intrinsics, every output inside a sentinel-filled buffer -> the plain section
    {name: array} (obs_w with it), the border's section, all buffers' bytes; asserts that nothing outside the outputs was written."""
    from vit_colmap_amd import _lib

    lib = _lib.load()
    cams, points, offsets, obs_cam, obs_xy, mask = problem
    cam_group, intr_mask = groups
    c, n, t, G = len(cams), len(points), len(obs_cam), len(intr_mask)
    index = index or ub.camera_index(obs_cam, offsets, c)
    d_cams, d_points, d_offsets, d_obs_cam, d_obs_xy, d_mask = dev(cams), dev(points), dev(offsets), dev(obs_cam), dev(obs_xy), dev(mask)
    d_group, d_intr, d_dc, d_dtheta = dev(cam_group), dev(intr_mask), dev(dc), dev(dtheta)
    d_index = [dev(np.asarray(a, np.int32)) for a in index]
    x = [_lib.ptr(a) for a in d_index]
    f64 = dict(dtype=torch.float64, device="cuda")
    plain = {k: torch.full((2 * PAD + size(c, n, t),), 7, dtype=TORCH_OF[kind], device="cuda") for k, (kind, size) in OUTPUTS.items()}
    plain["obs_w"] = torch.full((2 * PAD + t,), 7, **f64)
    border = {k: torch.full((2 * PAD + int(np.prod(shape)),), 7, **f64) for k, shape in result_shapes(c, n, t, G)}
    border.update(free=torch.full((2 * PAD + 4 * G,), 7, dtype=torch.uint8, device="cuda"), valid=torch.full((2 * PAD + c,), 7, dtype=torch.uint8, device="cuda"))
    o = {k: _lib.ptr(b[PAD:len(b) - PAD]) for k, b in plain.items()}
    ob = {k: _lib.ptr(b[PAD:len(b) - PAD]) for k, b in border.items()}
    p, stream = _lib.ptr, _lib.stream_ptr()
    _lib.check(lib.vc_ba_linearize_points_loss(p(d_cams), c, p(d_mask), p(d_points), n, p(d_offsets), p(d_obs_cam), p(d_obs_xy), t, lam, loss,
                                               scale, o["vinv"], o["gp"], o["cost"], o["count"], o["obs_ok"], o["obs_lin"], o["obs_w"],
                                               o["total_cost"], stream), "vc_ba_linearize_points_loss")
    _lib.check(lib.vc_ba_reduce_cameras(c, p(d_mask), n, p(d_offsets), p(d_obs_cam), t, x[0], x[1], x[2], lam, o["vinv"], o["gp"], o["obs_ok"],
                                        o["obs_lin"], o["S"], o["g"], stream), "vc_ba_reduce_cameras")
    _lib.check(lib.vc_ba_step(p(d_cams), c, p(d_points), n, p(d_offsets), p(d_obs_cam), t, o["vinv"], o["gp"], o["obs_ok"], o["obs_lin"],
                              p(d_dc), o["cams"], o["points"], o["dx"], stream), "vc_ba_step")
    _lib.check(lib.vc_ba_linearize_intrinsics_loss(p(d_cams), c, p(d_group), G, p(d_intr), p(d_points), n, p(d_offsets), p(d_obs_cam), t,
                                                   o["vinv"], o["gp"], o["obs_ok"], o["obs_lin"], o["obs_w"], ob["xn"], ob["T"], ob["terms"],
                                                   stream), "vc_ba_linearize_intrinsics_loss")
    _lib.check(lib.vc_ba_reduce_border_loss(c, p(d_group), G, p(d_intr), n, p(d_offsets), p(d_obs_cam), t, x[0], x[1], x[2], lam, o["vinv"],
                                            o["obs_ok"], o["obs_lin"], ob["xn"], o["obs_w"], ob["T"], ob["terms"], ob["sums"], ob["B"], ob["C"],
                                            ob["h"], ob["free"], stream), "vc_ba_reduce_border_loss")
    _lib.check(lib.vc_ba_step_intrinsics(p(d_cams), c, p(d_group), G, p(d_intr), p(d_points), n, p(d_offsets), p(d_obs_cam), t, o["vinv"],
                                         o["gp"], o["obs_ok"], o["obs_lin"], ob["T"], p(d_dc), p(d_dtheta), ob["cams"], ob["points"], ob["dx"],
                                         ob["valid"], stream), "vc_ba_step_intrinsics")
    torch.cuda.synchronize()
    out = []
    for bufs in (plain, border):
        host = {k: b.cpu().numpy() for k, b in bufs.items()}
        for k, b in host.items():
            assert (b[:PAD] == 7).all() and (b[len(b) - PAD:] == 7).all(), f"{k}: written outside the output"
        out.append(host)
    raw = b"".join(b.tobytes() for host in out for b in host.values())
    return tuple({k: b[PAD:len(b) - PAD] for k, b in host.items()} for host in out) + (raw,)


def assert_bytes_equal(got, host, what, skip=()):
    for k in got:
        if k not in skip:
            assert got[k].tobytes() == np.ascontiguousarray(host[k]).tobytes(), f"{what}: {k} differs from the host build"


@pytest.mark.parametrize("loss,scale", LOSSES)
@pytest.mark.parametrize("n_points,n_cams,n_groups", SHAPES)
def test_kernels_return_the_host_builds_bytes(n_points, n_cams, n_groups, loss, scale, bundle_host, tmp_path):  # noqa: F811
    (problem, zero), groups = loss_problem(n_points, n_cams), groups_of(n_cams, n_groups)
    dc, dtheta = step_of(problem), theta_step(groups)
    plain, border, raw = launch(problem, groups, ub.BA_LAMBDA0, dc, dtheta, loss, scale)
    host, _ = run_host_loss(bundle_host, tmp_path, problem, ub.BA_LAMBDA0, dc, loss, scale, groups=groups, dtheta=dtheta)
    what = f"{n_points} points, {n_cams} cameras, {n_groups} groups, loss {loss}"
    assert_bytes_equal(plain, dict(host["plain"], obs_w=host["obs_w"]), what)
    assert_bytes_equal(border, host, what)
    assert launch(problem, groups, ub.BA_LAMBDA0, dc, dtheta, loss, scale)[2] == raw          # two launches, identical bytes
    w, ok = plain["obs_w"], plain["obs_ok"].astype(bool)
    assert np.array_equal(w == 0, ~ok) and (w[ok] > 0).all() and (w[ok] <= 1).all()
    lin = plain["obs_lin"].reshape(-1, 32)
    assert ok[zero] and w[zero] == 1.0 and not lin[zero, 12:14].any()                                # the residual of exactly 0
    moved = ok.copy()
    moved[np.arange(len(ok)) % 7 != 0] = False
    assert (w[moved] < 0.5).all()                                     # 20 px off: far out on either loss at 1 px
    if n_points >= 63:
        assert (w[ok] < 1).any() and ((w[ok] == 1).any() if loss == ul.HUBER else True)            # both branches of Huber
        unweighted = launch_plain(problem, ub.BA_LAMBDA0, dc)[0]
        assert np.array_equal(unweighted["obs_ok"], plain["obs_ok"]) and np.array_equal(unweighted["count"], plain["count"])
        assert plain["total_cost"][0] < unweighted["total_cost"][0] and not np.array_equal(unweighted["S"], plain["S"])
    S = plain["S"].reshape(6 * n_cams, 6 * n_cams)
    assert np.isfinite(S).all() and np.isfinite(plain["dx"]).all() and np.isfinite(border["B"]).all() and np.isfinite(border["C"]).all()
    xn = launch_xn_without_loss(problem, groups)
    assert border["xn"].tobytes() == xn.tobytes()                      # obs_xn stays the unscaled (x, y)


def launch_xn_without_loss(problem, groups):
    from test_bundle_intr_gpu import launch as launch_border

    return launch_border(problem, groups, ub.BA_LAMBDA0, step_of(problem), theta_step(groups))[0]["xn"]


@pytest.mark.parametrize("n_points,n_cams", [(63, 3), (257, 70)])
def test_trivial_loss_through_the_new_entry_point_is_the_entry_point_without_a_loss(n_points, n_cams):
    problem, _ = loss_problem(n_points, n_cams)
    groups = groups_of(n_cams, 2)
    dc, dtheta = step_of(problem), theta_step(groups)
    want, _ = launch_plain(problem, ub.BA_LAMBDA0, dc)
    from test_bundle_intr_gpu import launch as launch_border

    want_border, _ = launch_border(problem, groups, ub.BA_LAMBDA0, dc, dtheta)
    plain, border, _ = launch(problem, groups, ub.BA_LAMBDA0, dc, dtheta, ul.TRIVIAL, 0.5)
    for k in OUTPUTS:
        assert plain[k].tobytes() == want[k].tobytes(), k
    assert np.array_equal(plain["obs_w"], want["obs_ok"].astype(np.float64))
    assert_bytes_equal(border, want_border, "trivial loss")


def test_offsets_that_delimit_nothing_skip_their_point_or_camera(bundle_host, tmp_path):  # noqa: F811
    (cams, points, offsets, obs_cam, obs_xy, mask), _ = loss_problem(65, 12)
    offsets = offsets.copy()
    total = len(obs_cam)
    offsets[11], offsets[20], offsets[-1] = total + 50, -4, total + 9   # points 10 and 64 pass the arrays, 11 and 19 descend, 20 begins below 0
    problem = (cams, points, offsets, obs_cam, obs_xy, mask)
    index = [a.copy() for a in ub.camera_index(obs_cam, offsets, len(cams))]
    index[0][4] = index[0][5] + 1
    index[1][index[0][7]] = total + 100
    groups = groups_of(12, 2)
    dc, dtheta = step_of(problem), theta_step(groups)
    plain, border, _ = launch(problem, groups, ub.BA_LAMBDA0, dc, dtheta, ul.HUBER, 1.0, index)
    host, _ = run_host_loss(bundle_host, tmp_path, problem, ub.BA_LAMBDA0, dc, ul.HUBER, 1.0, index, groups, dtheta)
    # the rows of a skipped point are not written: there the buffers keep their fill, the host program's arrays their zeros
    per_obs = ("obs_ok", "obs_lin", "obs_w")
    assert_bytes_equal(plain, dict(host["plain"], obs_w=host["obs_w"]), "bad offsets", skip=per_obs)
    assert_bytes_equal(border, host, "bad offsets", skip=("xn",))
    written = np.zeros(total, bool)
    for j in range(65):
        if 0 <= offsets[j] <= offsets[j + 1] <= total:
            written[offsets[j]:offsets[j + 1]] = True
    assert not written.all() and (plain["obs_w"][~written] == 7).all() and (plain["obs_ok"][~written] == 7).all()
    assert np.array_equal(plain["obs_w"][written], host["obs_w"][written]) and np.array_equal(plain["obs_ok"][written], host["plain"]["obs_ok"][written])
    assert np.array_equal(plain["obs_lin"].reshape(-1, 32)[written], host["plain"]["obs_lin"][written])
    assert np.array_equal(border["xn"].reshape(-1, 2)[written], host["xn"][written]) and (border["xn"].reshape(-1, 2)[~written] == 7).all()
    for j in (10, 11, 19, 20, 64):
        assert plain["count"][j] == 0 and not plain["vinv"].reshape(-1, 6)[j].any() and not border["T"].reshape(65, 2, 12)[j].any()


def test_argument_validation_returns_the_documented_codes_without_launching():
    from vit_colmap_amd import _lib

    lib = _lib.load()
    (cams, points, offsets, obs_cam, obs_xy, mask), _ = loss_problem(63, 3)
    groups = groups_of(3, 2)
    c, n, t, G = len(cams), len(points), len(obs_cam), 2
    inputs = [dev(a) for a in (cams, mask, points, offsets, obs_cam, obs_xy, groups[0], groups[1])]
    index = [dev(a) for a in ub.camera_index(obs_cam, offsets, c)]
    bufs = {k: torch.full((size(c, n, t),), 7, dtype=TORCH_OF[kind], device="cuda") for k, (kind, size) in OUTPUTS.items()}
    bufs["obs_w"] = torch.full((t,), 7, dtype=torch.float64, device="cuda")
    bufs.update({"b_" + k: torch.full((int(np.prod(shape)),), 7, dtype=torch.float64, device="cuda") for k, shape in result_shapes(c, n, t, G)})
    bufs["b_free"] = torch.full((4 * G,), 7, dtype=torch.uint8, device="cuda")
    p, stream = _lib.ptr, _lib.stream_ptr()
    i, x, o = [p(a) for a in inputs], [p(a) for a in index], {k: p(b) for k, b in bufs.items()}

    def lin(i=i, c=c, n=n, t=t, lam=1e-4, loss=ul.HUBER, scale=1.0, o=o):
        return lib.vc_ba_linearize_points_loss(i[0], c, i[1], i[2], n, i[3], i[4], i[5], t, lam, loss, scale, o["vinv"], o["gp"], o["cost"],
                                               o["count"], o["obs_ok"], o["obs_lin"], o["obs_w"], o["total_cost"], stream)

    def intr(i=i, c=c, n=n, t=t, G=G, o=o):
        return lib.vc_ba_linearize_intrinsics_loss(i[0], c, i[6], G, i[7], i[2], n, i[3], i[4], t, o["vinv"], o["gp"], o["obs_ok"], o["obs_lin"],
                                                   o["obs_w"], o["b_xn"], o["b_T"], o["b_terms"], stream)

    def red(i=i, x=x, c=c, n=n, t=t, G=G, lam=1e-4, o=o):
        return lib.vc_ba_reduce_border_loss(c, i[6], G, i[7], n, i[3], i[4], t, x[0], x[1], x[2], lam, o["vinv"], o["obs_ok"], o["obs_lin"],
                                            o["b_xn"], o["obs_w"], o["b_T"], o["b_terms"], o["b_sums"], o["b_B"], o["b_C"], o["b_h"],
                                            o["b_free"], stream)

    nothing = {k: None for k in o}
    ok, bad = _lib.VC_OK, _lib.VC_ERR_INVALID_ARG
    assert lin(i=[None] * 8, n=0, o=nothing) == ok and intr(i=[None] * 8, n=0, o=nothing) == ok and intr(G=0) == ok
    assert red(i=[None] * 8, x=[None] * 3, G=0, o=nothing) == ok
    for loss in (-1, 3, 1 << 20):
        assert lin(loss=loss) == bad and lin(loss=loss, n=0) == bad, loss
    for scale in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        assert lin(scale=scale) == bad and lin(loss=ul.TRIVIAL, scale=scale) == bad, scale
    assert lin(o=dict(o, obs_w=None)) == bad and intr(o=dict(o, obs_w=None)) == bad and red(o=dict(o, obs_w=None)) == bad
    for k in range(6):
        assert lin(i=i[:k] + [None] + i[k + 1:]) == bad, k
    for k in ("vinv", "gp", "cost", "count", "obs_ok", "obs_lin", "total_cost"):
        assert lin(o=dict(o, **{k: None})) == bad, k
    for k in ("vinv", "gp", "obs_ok", "obs_lin", "b_xn", "b_T", "b_terms"):
        assert intr(o=dict(o, **{k: None})) == bad, k
    for k in ("vinv", "obs_ok", "obs_lin", "b_xn", "b_T", "b_terms", "b_sums", "b_B", "b_C", "b_h", "b_free"):
        assert red(o=dict(o, **{k: None})) == bad, k
    for size in ("c", "n", "t"):
        assert lin(**{size: -1}) == intr(**{size: -1}) == red(**{size: -1}) == bad, size
    for lam in (-1.0, float("nan"), float("inf")):
        assert lin(lam=lam) == bad and red(lam=lam) == bad
    assert intr(G=_lib.VC_BA_MAX_GROUPS + 1) == red(G=_lib.VC_BA_MAX_GROUPS + 1) == _lib.VC_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert all((b == 7).all() for b in bufs.values())                 # nothing was launched


@lru_cache(maxsize=None)
def spec_loops():
    """The specification's loop on the corrupted windowed problem under Huber 1 px: the plain system under the cap of 25, and with
    one tied focal group from 1.03 f under a cap of 10 -> {name: (cams, points, report)}."""
    problem = ul.corrupted_windowed_problem()[0]
    wrong = with_focal(problem, 1.03)
    groups = tied_groups(len(problem[0]))
    return dict(plain=ul.bundle_adjust(*problem, ul.HUBER, 1.0),
                tied=ul.bundle_adjust(*wrong, ul.HUBER, 1.0, 10, *groups))


def test_bundle_adjust_under_huber_follows_the_specification_on_the_corrupted_problem():
    from vit_colmap_amd.mapping.bundle import bundle_adjust

    problem = ul.corrupted_windowed_problem()[0]
    groups = tied_groups(len(problem[0]))
    runs = dict(plain=(bundle_adjust(*problem, "cuda", loss="huber", loss_scale=1.0), LOOP_COST_REL),
                tied=(bundle_adjust(*with_focal(problem, 1.03), "cuda", max_iterations=10, cam_group=groups[0], intr_mask=groups[1],
                                    loss="huber"), LOOP_COST_REL_TIED))
    for name, ((cams, points, report), bound) in runs.items():                # every figure before any assertion
        spec_cams, _, spec = spec_loops()[name]
        rel = abs(report["final_cost"] - spec["final_cost"]) / spec["final_cost"]
        print(f"{name}: decisions {report['decisions']} (spec {spec['decisions']}), cost {report['initial_cost']:.12g} -> {report['final_cost']:.12g} "
              f"(spec {spec['final_cost']:.12g}, relative difference {rel:.3g}), lambda {report['final_lambda']:.3g}, focal {cams[0, 12]:.6f} "
              f"(spec {spec_cams[0, 12]:.6f})")
    for name, ((cams, points, report), bound) in runs.items():
        spec_cams, _, spec = spec_loops()[name]
        rel = abs(report["final_cost"] - spec["final_cost"]) / spec["final_cost"]
        assert report["decisions"] == spec["decisions"] and report["iterations"] == spec["iterations"], name
        assert report["accepted_steps"] == spec["accepted_steps"] and report["final_lambda"] == spec["final_lambda"], name
        assert report["initial_cost"] == spec["initial_cost"], name     # the kernel's order is the specification's
        assert rel <= bound, name
        assert report["loss"] == "huber" and report["loss_scale"] == 1.0
    assert "intrinsics" in runs["tied"][0][2] and "intrinsics" not in runs["plain"][0][2]
    # with the trivial loss: the calls, the report's numbers and every bit of the result of the loop without the arguments
    small = ub.random_problem(7)
    a, b = bundle_adjust(*small, "cuda"), bundle_adjust(*small, "cuda", loss="trivial", loss_scale=3.0)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2]["decisions"] == b[2]["decisions"] and a[2]["final_cost"] == b[2]["final_cost"]


def test_pipeline_with_the_loss_flags_writes_the_adjusted_model_and_without_them_todays_stats(tmp_path, monkeypatch):
    from vit_colmap_amd.mapping import SparseModel
    from vit_colmap_amd.pipeline import run_pipeline as rp
    from vit_colmap_amd.utils.config import Config

    class StubExtractor:
        device = "cuda"
        prior_focal_length = False

        def extract(self, image_dir, db_path, camera_model, camera_params):
            pass

    monkeypatch.setattr(rp.Pipeline, "_make_extractor", lambda self: StubExtractor())
    scene = um.windowed_scene()
    stats = {}
    for name, loss in (("huber", "huber"), ("plain", None)):
        write_windowed_db(tmp_path / f"{name}.db", scene)
        cfg = Config()
        cfg.camera.prior_focal_length, cfg.matching.compute_relative_pose, cfg.do_reconstruction = True, True, False
        cfg.reconstruction.sparse_model, cfg.reconstruction.bundle_adjustment = True, True
        if loss:
            cfg.reconstruction.ba_loss = loss
        p = rp.Pipeline(cfg)
        p.run(tmp_path / "images", tmp_path / name, tmp_path / f"{name}.db")
        stats[name] = p.last_stats["bundle_adjustment"]
        model = SparseModel.read_text(tmp_path / name / "sparse" / "adjusted")
        assert sorted(model.images) == list(range(1, 13)) and len(model.points3D) == stats[name]["num_points3D"]
    ba, today = stats["huber"]["bundle_adjustment"], stats["plain"]["bundle_adjustment"]
    assert ba["loss"] == "huber" and ba["loss_scale"] == 1.0 and ba["final_cost"] < ba["initial_cost"]
    assert sorted(today) == ["accepted_steps", "filtered_observations", "filtered_points", "final_cost", "final_lambda", "initial_cost",
                             "iterations"]
    assert sorted(set(ba) - set(today)) == ["loss", "loss_scale"] and set(today) <= set(ba)
    assert stats["huber"].keys() == stats["plain"].keys()
