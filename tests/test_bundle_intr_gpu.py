"""GPU tests of bundle adjustment with refined intrinsics ("The border"): vc_ba_linearize_intrinsics,
vc_ba_reduce_border and vc_ba_step_intrinsics against the same routines compiled for the host (tools/bundle_host.cpp), byte
for byte, on the problems of tests/test_bundle_gpu.py under groups of every kind, inside sentinel-filled buffers; two launches;
the argument checks; the front end's loop against the specification of tests/util_bundle_intr.py on the windowed problem from
a focal 3 % off; matching, growth and the adjustment end to end from a database whose camera is 3 % off, and the pipeline's flags."""
import numpy as np
import pytest
import torch

import util_absolute_pose as ua
import util_bundle as ub
import util_bundle_intr as ui
import util_essential as ue
import util_mapper as um
from test_absolute_pose_gpu import _two_view_bytes
from test_bundle_gpu import PAD, dev, problem_of, step_of
from test_bundle_intr_spec import grown_runs, tied_groups, windowed_problem, with_focal
from test_bundle_spec import bundle_host, result_shapes, run_host  # noqa: F401 - the fixture
from test_mapper_gpu import write_windowed_db

pytestmark = pytest.mark.gpu

MAX_GROUPS = ui.MAX_GROUPS
SHAPES = [(1, 2, 1), (63, 3, 2), (65, 12, 1), (257, 70, MAX_GROUPS)]       # (points, cameras, groups)
MASKS = [ui.TIED | ui.HOLD_PRINCIPAL, ui.HOLD_FX | ui.HOLD_FY, 0, ui.TIED, ui.HOLD_CX, ui.HOLD_PRINCIPAL, ui.TIED | ui.HOLD_CY, 0]
# the front end's loop on the windowed problem from 1.03 f against the specification's: the final cost, measured 1.98e-15
# relative, and the refined focal, measured 3.8e-16 relative (the two loops solve the bordered system with different
# factorisations, torch's of the assembled matrix on the device and numpy's by blocks); the bounds are 4x, rounded up
LOOP_COST_REL, LOOP_FOCAL_REL = 8e-15, 1.6e-15


def groups_of(n_cams, G):
    """Slot a in group a mod G; group 0 tied, group 1 with fx and fy held; from three groups on the last one has no camera and
    so no observation; the last camera (the NaN row) and, from five cameras on, the middle one are in groups outside the table."""
    cam_group = (np.arange(n_cams) % G).astype(np.int32)
    if G >= 3:
        cam_group[cam_group == G - 1] = 0
    cam_group[n_cams - 1] = -1
    if n_cams >= 5:
        cam_group[n_cams // 2] = G + 3
    return cam_group, np.array(MASKS[:G], np.uint8)


def theta_step(groups, seed=2, first=None):
    """A step of the intrinsics for the step kernel: zero where a parameter is held; `first`: dtheta_0 of group 0."""
    dtheta = np.random.RandomState(seed).normal(0, 0.5, (len(groups[1]), 4))
    dtheta = np.where([ui.theta_held(m) for m in groups[1]], 0.0, dtheta)
    if first is not None:
        dtheta[0, 0] = first
    return dtheta.reshape(-1)


def launch(problem, groups, lam, dc, dtheta, index=None):
    """vc_ba_linearize_points into plain buffers, then the three entry points of the border with every output inside a
    sentinel-filled buffer -> {name: numpy array} in the host program's layout and all buffers' bytes; asserts that nothing
    outside the outputs was written."""
    from vit_colmap_amd import _lib

    lib = _lib.load()
    cams, points, offsets, obs_cam, obs_xy, mask = problem
    cam_group, intr_mask = groups
    c, n, t, G = len(cams), len(points), len(obs_cam), len(intr_mask)
    index = index or ub.camera_index(obs_cam, offsets, c)
    d_cams, d_points, d_offsets, d_obs_cam, d_obs_xy, d_mask = dev(cams), dev(points), dev(offsets), dev(obs_cam), dev(obs_xy), dev(mask)
    d_group, d_intr, d_dc, d_dtheta = dev(cam_group), dev(intr_mask), dev(dc), dev(dtheta)
    d_index = [dev(np.asarray(a, np.int32)) for a in index]
    f64 = dict(dtype=torch.float64, device="cuda")
    vinv, gp, cost, total_cost = torch.zeros(6 * n, **f64), torch.zeros(3 * n, **f64), torch.zeros(n, **f64), torch.zeros(1, **f64)
    count, obs_ok, obs_lin = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(t, dtype=torch.uint8, device="cuda"), torch.zeros(32 * t, **f64)
    sizes = {k: int(np.prod(shape)) for k, shape in result_shapes(c, n, t, G)}
    bufs = {k: torch.full((2 * PAD + size,), 7, **f64) for k, size in sizes.items()}
    bufs.update(free=torch.full((2 * PAD + 4 * G,), 7, dtype=torch.uint8, device="cuda"), valid=torch.full((2 * PAD + c,), 7, dtype=torch.uint8, device="cuda"))
    o = {k: _lib.ptr(b[PAD:len(b) - PAD]) for k, b in bufs.items()}
    p, stream = _lib.ptr, _lib.stream_ptr()
    _lib.check(lib.vc_ba_linearize_points(p(d_cams), c, p(d_mask), p(d_points), n, p(d_offsets), p(d_obs_cam), p(d_obs_xy), t, lam, p(vinv),
                                          p(gp), p(cost), p(count), p(obs_ok), p(obs_lin), p(total_cost), stream), "vc_ba_linearize_points")
    _lib.check(lib.vc_ba_linearize_intrinsics(p(d_cams), c, p(d_group), G, p(d_intr), p(d_points), n, p(d_offsets), p(d_obs_cam), t, p(vinv),
                                              p(gp), p(obs_ok), p(obs_lin), o["xn"], o["T"], o["terms"], stream), "vc_ba_linearize_intrinsics")
    _lib.check(lib.vc_ba_reduce_border(c, p(d_group), G, p(d_intr), n, p(d_offsets), p(d_obs_cam), t, p(d_index[0]), p(d_index[1]),
                                       p(d_index[2]), lam, p(vinv), p(obs_ok), p(obs_lin), o["xn"], o["T"], o["terms"], o["sums"], o["B"],
                                       o["C"], o["h"], o["free"], stream), "vc_ba_reduce_border")
    _lib.check(lib.vc_ba_step_intrinsics(p(d_cams), c, p(d_group), G, p(d_intr), p(d_points), n, p(d_offsets), p(d_obs_cam), t, p(vinv),
                                         p(gp), p(obs_ok), p(obs_lin), o["T"], p(d_dc), p(d_dtheta), o["cams"], o["points"], o["dx"],
                                         o["valid"], stream), "vc_ba_step_intrinsics")
    torch.cuda.synchronize()
    host = {k: b.cpu().numpy() for k, b in bufs.items()}
    for k, b in host.items():
        assert (b[:PAD] == 7).all() and (b[len(b) - PAD:] == 7).all(), f"{k}: written outside the output"
    return {k: b[PAD:len(b) - PAD] for k, b in host.items()}, b"".join(b.tobytes() for b in host.values())


def assert_bytes_equal(got, host, what, skip=()):
    for k in got:
        if k not in skip:
            assert got[k].tobytes() == np.ascontiguousarray(host[k]).tobytes(), f"{what}: {k} differs from the host build"


@pytest.mark.parametrize("n_points,n_cams,n_groups", SHAPES)
def test_kernels_return_the_host_builds_bytes(n_points, n_cams, n_groups, bundle_host, tmp_path):  # noqa: F811
    problem, groups = problem_of(n_points, n_cams), groups_of(n_cams, n_groups)
    # at 65 points the step takes group 0's focal below zero: its slots are not valid
    dc, dtheta = step_of(problem), theta_step(groups, first=-700.0 if n_points == 65 else None)
    got, raw = launch(problem, groups, ub.BA_LAMBDA0, dc, dtheta)
    host, _ = run_host(bundle_host, tmp_path, problem, ub.BA_LAMBDA0, dc, groups=groups, dtheta=dtheta)
    assert_bytes_equal(got, host, f"{n_points} points, {n_cams} cameras, {n_groups} groups")
    again, raw2 = launch(problem, groups, ub.BA_LAMBDA0, dc, dtheta)
    assert raw == raw2                                                # two launches, identical bytes
    m = 4 * n_groups
    B, C, free = got["B"].reshape(6 * n_cams, m), got["C"].reshape(m, m), got["free"].astype(bool)
    assert np.isfinite(B).all() and np.isfinite(C).all() and np.isfinite(got["dx"]).all()
    assert not B[:6].any() and not B[6 * (n_cams - 1):].any()         # the held camera and the NaN row
    assert not free[1] and not free[2:4].any()                        # group 0 is tied and its principal point is held
    assert np.array_equal(C[~free], np.eye(m)[~free]) and np.array_equal(C[:, ~free], np.eye(m)[:, ~free]) and not got["h"][~free].any()
    if n_points >= 63:
        assert free[0] and B[:, 0].any() and np.abs(C - C.T).max() <= 1e-9 * np.abs(C).max()
    if n_groups >= 2:
        assert not free[4:6].any() and not B[:, 4:6].any()            # group 1: fx and fy held
    if n_groups >= 3:
        assert not free[m - 4:].any() and not got["T"].reshape(n_points, n_groups, 12)[:, -1].any()       # the group without observations
    valid = got["valid"].astype(bool)
    in_group = (groups[0] >= 0) & (groups[0] < n_groups)
    assert valid[~in_group].all()                                     # a slot outside the table keeps its intrinsics: every bit
    assert got["cams"].reshape(-1, 16)[~in_group][:, 12:].tobytes() == problem[0][~in_group][:, 12:].tobytes()
    if n_points == 65:
        assert not valid[groups[0] == 0].any() and (got["cams"].reshape(-1, 16)[groups[0] == 0, 12] < 0).all()
    else:
        assert valid.all()


def test_step_without_groups_is_vc_ba_steps_through_either_entry_point():
    """One points-step and one cameras-step kernel serve both entry points: vc_ba_step_intrinsics with n_groups = 0, whatever
    cam_group holds, writes vc_ba_step's bytes and calls every candidate valid.  65 points span the wave seam."""
    from vit_colmap_amd import _lib

    lib = _lib.load()
    problem = problem_of(65, 12)
    cams, points, offsets, obs_cam, obs_xy, mask = problem
    c, n, t = len(cams), len(points), len(obs_cam)
    d_cams, d_points, d_offsets, d_obs_cam, d_obs_xy, d_mask, d_dc = (dev(a) for a in (cams, points, offsets, obs_cam, obs_xy, mask, step_of(problem)))
    d_group = dev(np.array([0, 3, -1, 2 ** 31 - 1, -2 ** 31, 1, 7, 0, 0, -5, 2, 1], np.int32))       # read by nobody: there is no table
    f64 = dict(dtype=torch.float64, device="cuda")
    vinv, gp, cost, total_cost = torch.zeros(6 * n, **f64), torch.zeros(3 * n, **f64), torch.zeros(n, **f64), torch.zeros(1, **f64)
    count, obs_ok, obs_lin = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(t, dtype=torch.uint8, device="cuda"), torch.zeros(32 * t, **f64)
    p, stream = _lib.ptr, _lib.stream_ptr()
    _lib.check(lib.vc_ba_linearize_points(p(d_cams), c, p(d_mask), p(d_points), n, p(d_offsets), p(d_obs_cam), p(d_obs_xy), t, ub.BA_LAMBDA0,
                                          p(vinv), p(gp), p(cost), p(count), p(obs_ok), p(obs_lin), p(total_cost), stream), "vc_ba_linearize_points")
    runs = []
    for with_groups in (False, True):
        bufs = {k: torch.full((2 * PAD + size,), 7, **f64) for k, size in (("cams", 16 * c), ("points", 3 * n), ("dx", 3 * n))}
        bufs["valid"] = torch.full((2 * PAD + c,), 7, dtype=torch.uint8, device="cuda")
        o = {k: p(b[PAD:len(b) - PAD]) for k, b in bufs.items()}
        if with_groups:
            _lib.check(lib.vc_ba_step_intrinsics(p(d_cams), c, p(d_group), 0, None, p(d_points), n, p(d_offsets), p(d_obs_cam), t, p(vinv), p(gp),
                                                 p(obs_ok), p(obs_lin), None, p(d_dc), None, o["cams"], o["points"], o["dx"], o["valid"], stream),
                       "vc_ba_step_intrinsics")
        else:
            _lib.check(lib.vc_ba_step(p(d_cams), c, p(d_points), n, p(d_offsets), p(d_obs_cam), t, p(vinv), p(gp), p(obs_ok), p(obs_lin), p(d_dc),
                                      o["cams"], o["points"], o["dx"], stream), "vc_ba_step")
        torch.cuda.synchronize()
        host = {k: b.cpu().numpy() for k, b in bufs.items()}
        for k, b in host.items():
            assert (b[:PAD] == 7).all() and (b[len(b) - PAD:] == 7).all(), f"{k}: written outside the output"
        runs.append({k: b[PAD:len(b) - PAD] for k, b in host.items()})
    plain, grouped = runs
    for k in ("cams", "points", "dx"):
        assert plain[k].tobytes() == grouped[k].tobytes(), k
    assert (plain["valid"] == 7).all() and (grouped["valid"] == 1).all()       # vc_ba_step has no such output
    assert np.isfinite(plain["dx"]).all() and plain["dx"].any() and plain["cams"].tobytes() != cams.tobytes()


def test_the_largest_camera_count_with_two_groups(bundle_host, tmp_path):  # noqa: F811
    from vit_colmap_amd import _lib

    n_cams = _lib.VC_BA_MAX_CAMS
    rs = np.random.RandomState(17)
    cams = np.stack([um.camera_row(*ua.look_at(np.array([8.0 * np.sin(a), 0.0, -8.0 * np.cos(a)]), np.zeros(3)), ue.SCENE_K)
                     for a in np.radians(0.2 * np.arange(n_cams) - 50.0)])
    X = np.stack([rs.uniform(-2, 2, 24), rs.uniform(-1.5, 1.5, 24), rs.uniform(-1.5, 1.5, 24)], axis=1)
    obs_cam = np.concatenate([np.sort(rs.choice(n_cams, 8, replace=False)) for _ in range(23)] + [np.array([0, n_cams - 1])]).astype(np.int32)
    offsets = np.concatenate([np.arange(0, 8 * 23 + 1, 8), [8 * 23 + 2]]).astype(np.int32)
    Xc = np.einsum("nij,nj->ni", cams[obs_cam, :9].reshape(-1, 3, 3), np.repeat(X, np.diff(offsets), axis=0)) + cams[obs_cam, 9:12]
    obs_xy = ue.SCENE_K[0, 0] * Xc[:, :2] / Xc[:, 2:] + ue.SCENE_K[:2, 2] + rs.normal(0, 0.5, (len(obs_cam), 2))
    mask = np.zeros(n_cams, np.uint8)
    mask[0] = ub.HELD_ALL
    problem = (cams, X + rs.normal(0, 0.03, X.shape), offsets, obs_cam, obs_xy, mask)
    groups = tied_groups(n_cams, 2)
    dc, dtheta = step_of(problem), theta_step(groups)
    got, _ = launch(problem, groups, ub.BA_LAMBDA0, dc, dtheta)
    host, _ = run_host(bundle_host, tmp_path, problem, ub.BA_LAMBDA0, dc, groups=groups, dtheta=dtheta)
    assert_bytes_equal(got, host, f"{n_cams} cameras")
    B = got["B"].reshape(6 * n_cams, 8)
    assert not B[:6].any() and B[6 * (n_cams - 1):, 4].any() and got["free"].tolist() == [1, 0, 0, 0, 1, 0, 0, 0] and got["valid"].all()


def test_offsets_that_delimit_nothing_skip_their_point_or_camera(bundle_host, tmp_path):  # noqa: F811
    cams, points, offsets, obs_cam, obs_xy, mask = problem_of(65, 12)
    offsets = offsets.copy()
    total = len(obs_cam)
    offsets[11], offsets[20], offsets[-1] = total + 50, -4, total + 9   # points 10 and 64 pass the arrays, 11 and 19 descend, 20 begins below 0
    problem, groups = (cams, points, offsets, obs_cam, obs_xy, mask), groups_of(12, 2)
    index = [a.copy() for a in ub.camera_index(obs_cam, offsets, len(cams))]
    index[0][4] = index[0][5] + 1                                     # camera 4's list descends; camera 3's now runs into its neighbours'
    index[1][index[0][7]] = total + 100                               # an entry of camera 7's list names no observation
    dc, dtheta = step_of(problem), theta_step(groups)
    got, _ = launch(problem, groups, ub.BA_LAMBDA0, dc, dtheta, index)
    host, _ = run_host(bundle_host, tmp_path, problem, ub.BA_LAMBDA0, dc, index, groups, dtheta)
    # the rows of a skipped point are not written: there the buffer keeps its fill, the host program's array its zeros
    assert_bytes_equal(got, host, "bad offsets", skip=("xn",))
    written = np.zeros(total, bool)
    for j in range(65):
        if 0 <= offsets[j] <= offsets[j + 1] <= total:
            written[offsets[j]:offsets[j + 1]] = True
    xn = got["xn"].reshape(-1, 2)
    assert not written.all() and (xn[~written] == 7).all() and np.array_equal(xn[written], host["xn"][written])
    for j in (10, 11, 19, 20, 64):
        assert not got["T"].reshape(65, 2, 12)[j].any() and not got["terms"].reshape(-1, 65)[:, j].any() and not got["dx"].reshape(-1, 3)[j].any()
        assert np.array_equal(got["points"].reshape(-1, 3)[j], points[j])
    assert not got["B"].reshape(72, 8)[24:30].any() and np.isfinite(got["B"]).all()                 # the skipped camera


def test_argument_validation_returns_the_documented_codes_without_launching():
    from vit_colmap_amd import _lib

    lib = _lib.load()
    problem, groups = problem_of(63, 3), groups_of(3, 2)
    cams, points, offsets, obs_cam, obs_xy, mask = problem
    c, n, t, G = len(cams), len(points), len(obs_cam), 2
    f64 = dict(dtype=torch.float64, device="cuda")
    inputs = dict(cams=dev(cams), group=dev(groups[0]), intr=dev(groups[1]), points=dev(points), offsets=dev(offsets), obs_cam=dev(obs_cam),
                  vinv=torch.zeros(6 * n, **f64), gp=torch.zeros(3 * n, **f64), obs_ok=torch.zeros(t, dtype=torch.uint8, device="cuda"),
                  obs_lin=torch.zeros(32 * t, **f64), dc=torch.zeros(6 * c, **f64), dtheta=torch.zeros(4 * G, **f64))
    inputs.update(zip(("cam_offsets", "cam_obs", "obs_point"), (dev(a) for a in ub.camera_index(obs_cam, offsets, c))))
    bufs = {k: torch.full((int(np.prod(shape)),), 7, **f64) for k, shape in result_shapes(c, n, t, G)}
    bufs.update(free=torch.full((4 * G,), 7, dtype=torch.uint8, device="cuda"), valid=torch.full((c,), 7, dtype=torch.uint8, device="cuda"))
    p, stream = _lib.ptr, _lib.stream_ptr()
    a = {k: p(v) for k, v in {**inputs, **bufs}.items()}

    def lin(c=c, n=n, t=t, G=G, **kw):
        v = {**a, **kw}
        return lib.vc_ba_linearize_intrinsics(v["cams"], c, v["group"], G, v["intr"], v["points"], n, v["offsets"], v["obs_cam"], t, v["vinv"],
                                              v["gp"], v["obs_ok"], v["obs_lin"], v["xn"], v["T"], v["terms"], stream)

    def red(c=c, n=n, t=t, G=G, lam=1e-4, **kw):
        v = {**a, **kw}
        return lib.vc_ba_reduce_border(c, v["group"], G, v["intr"], n, v["offsets"], v["obs_cam"], t, v["cam_offsets"], v["cam_obs"],
                                       v["obs_point"], lam, v["vinv"], v["obs_ok"], v["obs_lin"], v["xn"], v["T"], v["terms"], v["sums"], v["B"],
                                       v["C"], v["h"], v["free"], stream)

    def stp(c=c, n=n, t=t, G=G, **kw):
        v = {**a, **kw}
        return lib.vc_ba_step_intrinsics(v["cams"], c, v["group"], G, v["intr"], v["points"], n, v["offsets"], v["obs_cam"], t, v["vinv"], v["gp"],
                                         v["obs_ok"], v["obs_lin"], v["T"], v["dc"], v["dtheta"], v["cams_out"], v["points_out"], v["dx"],
                                         v["valid"], stream)

    a["cams_out"], a["points_out"] = p(bufs["cams"]), p(bufs["points"])
    a["cams"], a["points"] = p(inputs["cams"]), p(inputs["points"])
    nothing = {k: None for k in a}
    assert lin(n=0, **nothing) == lin(G=0, **nothing) == red(G=0, **nothing) == stp(c=0, n=0, **nothing) == _lib.VC_OK
    for k in ("cams", "group", "intr", "points", "offsets", "obs_cam", "vinv", "gp", "obs_ok", "obs_lin", "xn", "T", "terms"):
        assert lin(**{k: None}) == _lib.VC_ERR_INVALID_ARG, k
    for k in ("group", "intr", "offsets", "obs_cam", "cam_offsets", "cam_obs", "obs_point", "vinv", "obs_ok", "obs_lin", "xn", "T", "terms", "sums",
              "B", "C", "h", "free"):
        assert red(**{k: None}) == _lib.VC_ERR_INVALID_ARG, k
    for k in ("cams", "group", "intr", "points", "offsets", "obs_cam", "vinv", "gp", "obs_ok", "obs_lin", "T", "dc", "dtheta", "cams_out",
              "points_out", "dx", "valid"):
        assert stp(**{k: None}) == _lib.VC_ERR_INVALID_ARG, k
    for size in ("c", "n", "t", "G"):
        assert lin(**{size: -1}) == red(**{size: -1}) == stp(**{size: -1}) == _lib.VC_ERR_INVALID_ARG, size
    for bad in (-1.0, float("nan"), float("inf")):
        assert red(lam=bad) == _lib.VC_ERR_INVALID_ARG
    assert lin(G=MAX_GROUPS + 1) == red(G=MAX_GROUPS + 1) == stp(G=MAX_GROUPS + 1) == _lib.VC_ERR_UNSUPPORTED
    assert red(c=_lib.VC_BA_MAX_CAMS + 1) == _lib.VC_ERR_UNSUPPORTED
    assert _lib.VC_BA_MAX_GROUPS == MAX_GROUPS >= 8
    torch.cuda.synchronize()
    assert all((b == 7).all() for b in bufs.values())                 # nothing was launched
    # the front end names the limit
    from vit_colmap_amd.mapping.bundle import bundle_adjust

    with pytest.raises(ValueError, match="VC_BA_MAX_GROUPS"):
        bundle_adjust(*problem, "cuda", cam_group=np.zeros(c, np.int32), intr_mask=np.zeros(MAX_GROUPS + 1, np.uint8))


def test_bundle_adjust_with_a_tied_group_follows_the_specification_from_a_wrong_focal():
    from vit_colmap_amd.mapping.bundle import bundle_adjust

    problem = with_focal(windowed_problem(), 1.03)
    groups = tied_groups(len(problem[0]))
    cams, points, report = bundle_adjust(*problem, "cuda", cam_group=groups[0], intr_mask=groups[1])
    spec_cams, _, spec = grown_runs()["refined"]
    rel = abs(report["final_cost"] - spec["final_cost"]) / spec["final_cost"]
    rel_f = abs(cams[0, 12] - spec_cams[0, 12]) / spec_cams[0, 12]
    print(f"decisions {report['decisions']} (spec {spec['decisions']}), final cost {report['final_cost']:.12g} (spec {spec['final_cost']:.12g}, "
          f"relative difference {rel:.3g}), focal {cams[0, 12]:.9f} (spec {spec_cams[0, 12]:.9f}, relative difference {rel_f:.3g})")
    assert report["decisions"] == spec["decisions"] and report["iterations"] == spec["iterations"]
    assert report["accepted_steps"] == spec["accepted_steps"] and report["final_lambda"] == spec["final_lambda"]
    assert report["initial_cost"] == spec["initial_cost"]             # the kernel's order is the specification's
    assert rel <= LOOP_COST_REL and rel_f <= LOOP_FOCAL_REL
    assert (cams[:, 12] == cams[0, 12]).all() and np.array_equal(cams[:, 12], cams[:, 13]) and np.array_equal(cams[:, 14:], problem[0][:, 14:])
    assert np.array_equal(report["intrinsics"]["before"], problem[0][:1, 12:]) and np.array_equal(report["intrinsics"]["after"], cams[:1, 12:])
    # without groups the report has no such key (the expectations of tests/test_bundle_gpu.py hold unchanged)
    assert "intrinsics" not in bundle_adjust(*ub.random_problem(7), "cuda")[2]


def wrong_focal_scene(factor=1.03):
    scene = um.windowed_scene()
    K = scene["K"].copy()
    K[0, 0], K[1, 1] = K[0, 0] * factor, K[1, 1] * factor
    return scene, dict(scene, K=K)


@pytest.fixture(scope="module")
def end_to_end(tmp_path_factory):
    """A database whose camera is 3 % off -> matched, grown, adjusted with the focal held and with it refined (once for the two
    tests below).  Here the wrong focal also passes through E, P3P and triangulation."""
    from vit_colmap_amd.mapping.bundle import build_adjusted_model
    from vit_colmap_amd.mapping.grow import build_sparse_model
    from vit_colmap_amd.matching import match_exhaustive
    from vit_colmap_amd.utils.config import MatchingConfig

    directory = tmp_path_factory.mktemp("bundle_intr_end_to_end")
    scene, wrong = wrong_focal_scene()
    write_windowed_db(directory / "w.db", wrong)
    match_exhaustive(database_path=str(directory / "w.db"), matching_options=MatchingConfig(compute_relative_pose=True).to_matching_options())
    rows_before = _two_view_bytes(directory / "w.db")
    grown = build_sparse_model(directory / "w.db")
    held = build_adjusted_model(directory / "w.db", grown=grown)
    model = build_adjusted_model(directory / "w.db", grown=grown, refine_focal_length=True)
    return scene["K"][0, 0], grown, held, model, rows_before == _two_view_bytes(directory / "w.db"), directory


def test_match_exhaustive_then_build_adjusted_model_with_a_refined_focal_end_to_end(end_to_end):
    from vit_colmap_amd.mapping import SparseModel

    f, grown, held, model, rows_unchanged, directory = end_to_end
    (cid, cam), = model.cameras.items()
    fx, fy = (float(v) for v in cam.params[:2])
    ba = model.stats()["bundle_adjustment"]
    print(f"focal {grown.cameras[cid].params[0]:.3f} -> fx {fx:.4f} ({abs(fx - f) / f:.3%} off), fy {fy:.4f} ({abs(fy - f) / f:.3%} off), cost "
          f"{ba['initial_cost']:.2f} -> {ba['final_cost']:.4f} in {ba['iterations']} linearisations (held: {held.bundle_adjustment['final_cost']:.4f}), "
          f"{len(grown.points3D)} -> {len(model.points3D)} points")
    assert sorted(model.images) == list(range(1, 13)) and held.cameras == grown.cameras and "intrinsics" not in held.stats()["bundle_adjustment"]
    assert cam.model == "PINHOLE" and list(cam.params[2:]) == list(grown.cameras[cid].params[2:]) and (fx, fy) != tuple(grown.cameras[cid].params[:2])
    assert ba["intrinsics"][cid]["before"] == [float(v) for v in grown.cameras[cid].params] and ba["intrinsics"][cid]["after"][:2] == [fx, fy]
    assert ba["final_cost"] < held.bundle_adjustment["final_cost"] < ba["initial_cost"] and ba["accepted_steps"] >= 1
    for p in model.points3D.values():
        assert len(p["track"]) >= 2 and p["error"] <= ub.MAX_ERROR
    model.write_text(directory / "adjusted")
    assert SparseModel.read_text(directory / "adjusted") == model
    assert rows_unchanged                                             # building any of the models only reads: the rows are byte for byte what matching wrote


def test_end_to_end_the_written_focal_is_within_one_per_cent_of_the_truth(end_to_end):
    """From a camera at 618 for 600 the adjusted cameras.txt carries fx 601.74 and fy 598.11 (0.29 % and 0.32 % off; 1x MI355X,
    2026-10-20), cost 19009.62 -> 171.04 in 271 linearisations.  The model was grown under the wrong focal and starts far from
    a minimum, where the loop alternates a rejected and an accepted step: under the plain adjustment's cap of 25 linearisations
    it would end at fx 731.30, fy 553.17, which is why build_adjusted_model gives the loop REFINE_MAX_ITERATIONS here."""
    from vit_colmap_amd.mapping.bundle_intr import REFINE_MAX_ITERATIONS

    f, _, _, model, _, _ = end_to_end
    (cid, cam), = model.cameras.items()
    fx, fy = (float(v) for v in cam.params[:2])
    print(f"fx {fx:.4f} ({abs(fx - f) / f:.3%} off), fy {fy:.4f} ({abs(fy - f) / f:.3%} off)")
    assert abs(fx - f) / f <= 0.01 and abs(fy - f) / f <= 0.01
    assert 25 < model.bundle_adjustment["iterations"] < REFINE_MAX_ITERATIONS      # it ended because it converged, not at the cap


def test_pipeline_with_both_flags_changes_only_the_focal_of_the_adjusted_cameras(tmp_path, monkeypatch):
    from vit_colmap_amd.pipeline import run_pipeline as rp
    from vit_colmap_amd.utils.config import Config

    class StubExtractor:
        device = "cuda"
        prior_focal_length = False

        def extract(self, image_dir, db_path, camera_model, camera_params):
            pass

    monkeypatch.setattr(rp.Pipeline, "_make_extractor", lambda self: StubExtractor())
    scene, wrong = wrong_focal_scene()
    write_windowed_db(tmp_path / "w.db", wrong)
    cfg = Config()
    cfg.camera.prior_focal_length, cfg.matching.compute_relative_pose, cfg.do_reconstruction = True, True, False
    cfg.reconstruction.sparse_model, cfg.reconstruction.bundle_adjustment, cfg.reconstruction.refine_focal_length = True, True, True
    p = rp.Pipeline(cfg)
    p.run(tmp_path / "images", tmp_path / "out", tmp_path / "w.db")
    a, b = ((tmp_path / "out" / "sparse" / m / "cameras.txt").read_text().splitlines() for m in ("grown", "adjusted"))
    differing = [(x.split(), y.split()) for x, y in zip(a, b) if x != y]
    assert len(a) == len(b) and len(differing) == 1
    wx, wy = differing[0]                                              # id, PINHOLE, width, height, fx, fy, cx, cy
    assert wx[:4] == wy[:4] and wx[6:] == wy[6:] and wx[4] != wy[4] and wx[5] != wy[5]
    report = p.last_stats["bundle_adjustment"]["bundle_adjustment"]["intrinsics"]
    assert [repr(v) for v in report[int(wy[0])]["after"][:2]] == wy[4:6] and "intrinsics" not in p.last_stats["sparse_model"]
