"""GPU tests of bundle adjustment with radial distortion ("The distortion"): vc_ba_linearize_points_radial,
vc_ba_reduce_cameras on its outputs, vc_ba_linearize_intrinsics_radial, vc_ba_reduce_border_radial and vc_ba_step_radial against
the same routines compiled for the host (tools/bundle_host.cpp with the radial section of its problem file), byte for byte, on
the problems of tests/test_bundle_gpu.py under groups of every kind and non-zero k, inside sentinel-filled buffers; two
launches; offsets and indices that name nothing; the argument checks; the front end's loop against the specification of
tests/util_bundle_radial.py on the distorted windowed problem; matching, growth and the adjustment end to end from a
SIMPLE_RADIAL database with k = 0, and the pipeline's flag."""
import numpy as np
import pytest
import torch

import util_bundle as ub
import util_bundle_intr as ui
import util_bundle_loss as ul
import util_bundle_radial as ur
from test_absolute_pose_gpu import _two_view_bytes
from test_bundle_gpu import PAD, dev, problem_of, step_of
from test_bundle_radial_spec import K1_BOUND, K1_FREE, distorted, recovered, set_camera_model
from test_bundle_spec import bundle_host  # noqa: F401 - the fixture
from test_mapper_gpu import write_windowed_db

pytestmark = pytest.mark.gpu

MAX_GROUPS = ur.MAX_GROUPS
SHAPES = [(1, 2, 1), (63, 3, 2), (65, 12, 1), (257, 70, MAX_GROUPS)]       # (points, cameras, groups)
# group 0: one tied focal and k1 free, k2 held (refine_distortion + refine_focal_length on SIMPLE_RADIAL); group 1: the focal held,
# k1 and k2 free (refine_distortion on RADIAL); group 2: k1 and k2 held, cx held; group 3: everything free, and no camera
MASKS = [ui.TIED | ui.HOLD_PRINCIPAL | ur.HOLD_K2, ui.HOLD_FX | ui.HOLD_FY, ur.HOLD_DIST | ui.HOLD_CX, 0]
GROUP_K = np.array([[-0.12, 0.03], [0.08, -0.02], [0.05, 0.01], [0.0, 0.0]])
# the front end's loop on the distorted windowed problem against the specification's: the final cost, measured 2.51e-16
# relative, and the refined k1, measured 2.86e-15 relative (1x MI355X; the two loops solve the bordered system with different
# factorisations, torch's of the assembled matrix on the device and numpy's by blocks); the bounds are 4x, rounded up
LOOP_COST_REL, LOOP_K1_REL = 1.1e-15, 1.2e-14


def groups_of(n_cams, G):
    """Slot a in group a mod G; from three groups on the last one has no camera and so no observation; the last camera (the NaN
    row) and, from five cameras on, the middle one are in groups outside the table.  -> (cam_group, intr_mask), dist (n_cams, 2):
    every slot carries its group's non-zero k, a slot outside the table (0.02, -0.01)."""
    cam_group = (np.arange(n_cams) % G).astype(np.int32)
    if G >= 3:
        cam_group[cam_group == G - 1] = 0
    cam_group[n_cams - 1] = -1
    if n_cams >= 5:
        cam_group[n_cams // 2] = G + 3
    inside = (cam_group >= 0) & (cam_group < G)
    dist = np.where(inside[:, None], GROUP_K[np.where(inside, cam_group, 0)], [0.02, -0.01])
    return (cam_group, np.array(MASKS[:G], np.uint8)), np.ascontiguousarray(dist)


def theta_step(groups, seed=2, nan_k1=False):
    """A step of the six intrinsics: zero where a parameter is held; `nan_k1`: dtheta_4 of group 0 is NaN."""
    G = len(groups[1])
    dtheta = np.random.RandomState(seed).normal(0, 0.5, (G, 6)) * [1.0, 1.0, 1.0, 1.0, 0.01, 0.01]
    dtheta = np.where([ur.theta_held(m) for m in groups[1]], 0.0, dtheta)
    if nan_k1:
        dtheta[0, 4] = np.nan
    return dtheta.reshape(-1)


def sizes_of(c, n, t, G):
    """Every output of the five calls -> {name: (torch dtype, elements)} in the host program's names."""
    f8, rows = torch.float64, 48 * G + 36 * G * G
    return dict(vinv=(f8, 6 * n), gp=(f8, 3 * n), cost=(f8, n), total_cost=(f8, 1), obs_lin=(f8, 32 * t), obs_w=(f8, t),
                count=(torch.int32, n), obs_ok=(torch.uint8, t), S=(f8, 36 * c * c), g=(f8, 6 * c), jt=(f8, 6 * t), T=(f8, 18 * n * G),
                terms=(f8, rows * n), sums=(f8, rows), B=(f8, 36 * c * G), C=(f8, 36 * G * G), h=(f8, 6 * G), free=(torch.uint8, 6 * G),
                cams=(f8, 16 * c), dist=(f8, 2 * c), points=(f8, 3 * n), dx=(f8, 3 * n), valid=(torch.uint8, c))


def launch(problem, dist, groups, lam, dc, dtheta, loss=ul.TRIVIAL, scale=1.0, index=None):
    """The radial entry points (and vc_ba_reduce_cameras between them) with every output inside a sentinel-filled buffer ->
    {name: numpy array} in the host program's names and all buffers' bytes; asserts that nothing outside the outputs was written."""
    from vit_colmap_amd import _lib

    lib = _lib.load()
    cams, points, offsets, obs_cam, obs_xy, mask = problem
    cam_group, intr_mask = groups
    c, n, t, G = len(cams), len(points), len(obs_cam), len(intr_mask)
    index = index or ub.camera_index(obs_cam, offsets, c)
    d_cams, d_dist, d_points, d_offsets, d_obs_cam, d_obs_xy, d_mask = (dev(a) for a in (cams, dist, points, offsets, obs_cam, obs_xy, mask))
    d_group, d_intr, d_dc, d_dtheta = dev(cam_group), dev(intr_mask), dev(dc), dev(dtheta)
    d_index = [dev(np.asarray(a, np.int32)) for a in index]
    bufs = {k: torch.full((2 * PAD + size,), 7, dtype=kind, device="cuda") for k, (kind, size) in sizes_of(c, n, t, G).items()}
    o = {k: _lib.ptr(b[PAD:len(b) - PAD]) for k, b in bufs.items()}
    p, stream = _lib.ptr, _lib.stream_ptr()
    _lib.check(lib.vc_ba_linearize_points_radial(p(d_cams), c, p(d_dist), p(d_mask), p(d_points), n, p(d_offsets), p(d_obs_cam), p(d_obs_xy), t,
                                                 lam, loss, scale, o["vinv"], o["gp"], o["cost"], o["count"], o["obs_ok"], o["obs_lin"],
                                                 o["obs_w"], o["total_cost"], stream), "vc_ba_linearize_points_radial")
    _lib.check(lib.vc_ba_reduce_cameras(c, p(d_mask), n, p(d_offsets), p(d_obs_cam), t, p(d_index[0]), p(d_index[1]), p(d_index[2]), lam,
                                        o["vinv"], o["gp"], o["obs_ok"], o["obs_lin"], o["S"], o["g"], stream), "vc_ba_reduce_cameras")
    _lib.check(lib.vc_ba_linearize_intrinsics_radial(p(d_cams), c, p(d_dist), p(d_group), G, p(d_intr), p(d_points), n, p(d_offsets),
                                                     p(d_obs_cam), t, loss, scale, o["vinv"], o["gp"], o["obs_ok"], o["obs_lin"], o["obs_w"],
                                                     o["jt"], o["T"], o["terms"], stream), "vc_ba_linearize_intrinsics_radial")
    _lib.check(lib.vc_ba_reduce_border_radial(c, p(d_group), G, p(d_intr), n, p(d_offsets), p(d_obs_cam), t, p(d_index[0]), p(d_index[1]),
                                              p(d_index[2]), lam, loss, scale, o["vinv"], o["obs_ok"], o["obs_lin"], o["jt"], o["obs_w"], o["T"],
                                              o["terms"], o["sums"], o["B"], o["C"], o["h"], o["free"], stream), "vc_ba_reduce_border_radial")
    _lib.check(lib.vc_ba_step_radial(p(d_cams), c, p(d_dist), p(d_group), G, p(d_intr), p(d_points), n, p(d_offsets), p(d_obs_cam), t,
                                     o["vinv"], o["gp"], o["obs_ok"], o["obs_lin"], o["T"], p(d_dc), p(d_dtheta), o["cams"], o["dist"],
                                     o["points"], o["dx"], o["valid"], stream), "vc_ba_step_radial")
    torch.cuda.synchronize()
    host = {k: b.cpu().numpy() for k, b in bufs.items()}
    for k, b in host.items():
        assert (b[:PAD] == 7).all() and (b[len(b) - PAD:] == 7).all(), f"{k}: written outside the output"
    return {k: b[PAD:len(b) - PAD] for k, b in host.items()}, b"".join(b.tobytes() for b in host.values())


def host_arrays(host):
    """ur.read_result_file's dict flattened to the names of `sizes_of`: the plain section's points pass and reduction, the
    border's section, obs_w."""
    out = {k: host["plain"][k] for k in ("vinv", "gp", "cost", "total_cost", "obs_lin", "count", "obs_ok", "S", "g")}
    out.update({k: v for k, v in host.items() if k != "plain"})
    return out


def assert_bytes_equal(got, host, what, skip=()):
    assert sorted(got) == sorted(host)
    for k in got:
        if k not in skip:
            assert got[k].tobytes() == np.ascontiguousarray(host[k]).tobytes(), f"{what}: {k} differs from the host build"


@pytest.mark.parametrize("n_points,n_cams,n_groups", SHAPES)
def test_kernels_return_the_host_builds_bytes(n_points, n_cams, n_groups, bundle_host, tmp_path):  # noqa: F811
    problem = problem_of(n_points, n_cams)
    groups, dist = groups_of(n_cams, n_groups)
    # at 65 points the step makes group 0's k1 NaN: its slots are not valid
    dc, dtheta = step_of(problem), theta_step(groups, nan_k1=n_points == 65)
    got, raw = launch(problem, dist, groups, ub.BA_LAMBDA0, dc, dtheta)
    host, _ = ur.run_host(bundle_host, tmp_path, problem, dist, ub.BA_LAMBDA0, dc, groups, dtheta)
    assert_bytes_equal(got, host_arrays(host), f"{n_points} points, {n_cams} cameras, {n_groups} groups")
    again, raw2 = launch(problem, dist, groups, ub.BA_LAMBDA0, dc, dtheta)
    assert raw == raw2                                                # two launches, identical bytes
    m = 6 * n_groups
    B, C, free = got["B"].reshape(6 * n_cams, m), got["C"].reshape(m, m), got["free"].astype(bool)
    assert np.isfinite(B).all() and np.isfinite(C).all() and (got["obs_w"][got["obs_ok"] == 1] == 1.0).all()
    assert not B[:6].any() and not B[6 * (n_cams - 1):].any()         # the held camera and the NaN row
    # group 0: tied, the principal point and k2 held, k1 free
    assert not free[1:4].any() and not free[5] and np.array_equal(C[~free], np.eye(m)[~free]) and not got["h"][~free].any()
    if n_points >= 63:
        assert free[0] and free[4] and B[:, 4].any() and np.abs(C - C.T).max() <= 1e-9 * np.abs(C).max()
    if n_groups >= 2:                                                 # group 1: fx and fy held, k1 and k2 free
        assert not free[6:8].any() and free[8:12].all() and B[:, 10:12].any() and not B[:, 6:8].any()
    if n_groups >= 3:                                                 # group 2: k1 and k2 held; group 3: no observation
        assert not free[16:18].any() and free[12:14].all() and not free[14] and not free[m - 6:].any()
        assert not got["T"].reshape(n_points, n_groups, 18)[:, -1].any() and not got["T"].reshape(n_points, n_groups, 6, 3)[:, 2, 4:].any()
    valid = got["valid"].astype(bool)
    in_group = (groups[0] >= 0) & (groups[0] < n_groups)
    assert valid[~in_group].all() and not in_group.all()              # a slot outside the table keeps its intrinsics: every bit
    assert got["cams"].reshape(-1, 16)[~in_group][:, 12:].tobytes() == problem[0][~in_group][:, 12:].tobytes()
    assert got["dist"].reshape(-1, 2)[~in_group].tobytes() == dist[~in_group].tobytes()
    new_k = got["dist"].reshape(-1, 2)
    if n_points == 65:
        assert not valid[groups[0] == 0].any() and np.isnan(new_k[groups[0] == 0, 0]).all() and (new_k[groups[0] == 0, 1] == GROUP_K[0, 1]).all()
    else:
        assert valid.all() and np.isfinite(got["dx"]).all()
        assert (new_k[in_group, 0] != dist[in_group, 0]).any() and (new_k[groups[0] == 0, 1] == GROUP_K[0, 1]).all()


def test_huber_with_observations_on_both_sides_of_the_scale_returns_the_host_builds_bytes(bundle_host, tmp_path):  # noqa: F811
    problem = problem_of(65, 12)
    groups, dist = groups_of(12, 2)
    dc, dtheta = step_of(problem), theta_step(groups)
    got, _ = launch(problem, dist, groups, ub.BA_LAMBDA0, dc, dtheta, ul.HUBER, 2.0)
    host, _ = ur.run_host(bundle_host, tmp_path, problem, dist, ub.BA_LAMBDA0, dc, groups, dtheta, ul.HUBER, 2.0)
    assert_bytes_equal(got, host_arrays(host), "Huber at 2 px")
    w = got["obs_w"][got["obs_ok"] == 1]
    assert (w == 1.0).sum() >= 10 and (w < 1.0).sum() >= 10 and (w > 0.0).all()                      # both branches of the loss
    plain, _ = launch(problem, dist, groups, ub.BA_LAMBDA0, dc, dtheta)
    assert got["total_cost"][0] < plain["total_cost"][0] and got["B"].tobytes() != plain["B"].tobytes()


def test_offsets_that_delimit_nothing_skip_their_point_or_camera(bundle_host, tmp_path):  # noqa: F811
    cams, points, offsets, obs_cam, obs_xy, mask = problem_of(65, 12)
    offsets = offsets.copy()
    total = len(obs_cam)
    offsets[11], offsets[20], offsets[-1] = total + 50, -4, total + 9   # points 10 and 64 pass the arrays, 11 and 19 descend, 20 begins below 0
    problem = (cams, points, offsets, obs_cam, obs_xy, mask)
    groups, dist = groups_of(12, 2)
    index = [a.copy() for a in ub.camera_index(obs_cam, offsets, len(cams))]
    index[0][4] = index[0][5] + 1                                     # camera 4's list descends; camera 3's now runs into its neighbours'
    index[1][index[0][7]] = total + 100                               # an entry of camera 7's list names no observation
    dc, dtheta = step_of(problem), theta_step(groups)
    got, _ = launch(problem, dist, groups, ub.BA_LAMBDA0, dc, dtheta, index=index)
    host, _ = ur.run_host(bundle_host, tmp_path, problem, dist, ub.BA_LAMBDA0, dc, groups, dtheta, index=index)
    host = host_arrays(host)
    # the rows of a skipped point are not written: there the buffer keeps its fill, the host program's array its zeros
    per_obs = ("jt", "obs_lin", "obs_w", "obs_ok")
    assert_bytes_equal(got, host, "bad offsets", skip=per_obs)
    written = np.zeros(total, bool)
    for j in range(65):
        if 0 <= offsets[j] <= offsets[j + 1] <= total:
            written[offsets[j]:offsets[j + 1]] = True
    assert not written.all()
    for k in per_obs:
        a, b = got[k].reshape(total, -1), np.asarray(host[k]).reshape(total, -1)
        assert (a[~written] == 7).all() and a[written].tobytes() == b[written].tobytes(), k
    for j in (10, 11, 19, 20, 64):
        assert not got["T"].reshape(65, 2, 18)[j].any() and not got["terms"].reshape(-1, 65)[:, j].any() and not got["dx"].reshape(-1, 3)[j].any()
        assert np.array_equal(got["points"].reshape(-1, 3)[j], points[j]) and got["count"][j] == 0 and not got["vinv"].reshape(-1, 6)[j].any()
    assert not got["B"].reshape(72, 12)[24:30].any() and np.isfinite(got["B"]).all()                # the skipped camera


def test_argument_validation_returns_the_documented_codes_without_launching():
    from vit_colmap_amd import _lib

    lib = _lib.load()
    problem = problem_of(63, 3)
    groups, dist = groups_of(3, 2)
    cams, points, offsets, obs_cam, obs_xy, mask = problem
    c, n, t, G = len(cams), len(points), len(obs_cam), 2
    f64 = dict(dtype=torch.float64, device="cuda")
    inputs = dict(cams=dev(cams), cam_dist=dev(dist), mask=dev(mask), group=dev(groups[0]), intr=dev(groups[1]), points=dev(points),
                  offsets=dev(offsets), obs_cam=dev(obs_cam), obs_xy=dev(obs_xy), dc=torch.zeros(6 * c, **f64), dtheta=torch.zeros(6 * G, **f64))
    inputs.update(zip(("cam_offsets", "cam_obs", "obs_point"), (dev(a) for a in ub.camera_index(obs_cam, offsets, c))))
    bufs = {k: torch.full((size,), 7, dtype=kind, device="cuda") for k, (kind, size) in sizes_of(c, n, t, G).items() if k not in ("S", "g")}
    p, stream = _lib.ptr, _lib.stream_ptr()
    a = {k: p(v) for k, v in inputs.items()}
    a.update({("out_" + k if k in ("cams", "points") else k): p(v) for k, v in bufs.items()})

    def pts(c=c, n=n, t=t, lam=1e-4, loss=0, scale=1.0, **kw):
        v = {**a, **kw}
        return lib.vc_ba_linearize_points_radial(v["cams"], c, v["cam_dist"], v["mask"], v["points"], n, v["offsets"], v["obs_cam"], v["obs_xy"], t,
                                                 lam, loss, scale, v["vinv"], v["gp"], v["cost"], v["count"], v["obs_ok"], v["obs_lin"],
                                                 v["obs_w"], v["total_cost"], stream)

    def lin(c=c, n=n, t=t, G=G, loss=0, scale=1.0, **kw):
        v = {**a, **kw}
        return lib.vc_ba_linearize_intrinsics_radial(v["cams"], c, v["cam_dist"], v["group"], G, v["intr"], v["points"], n, v["offsets"],
                                                     v["obs_cam"], t, loss, scale, v["vinv"], v["gp"], v["obs_ok"], v["obs_lin"], v["obs_w"],
                                                     v["jt"], v["T"], v["terms"], stream)

    def red(c=c, n=n, t=t, G=G, lam=1e-4, loss=0, scale=1.0, **kw):
        v = {**a, **kw}
        return lib.vc_ba_reduce_border_radial(c, v["group"], G, v["intr"], n, v["offsets"], v["obs_cam"], t, v["cam_offsets"], v["cam_obs"],
                                              v["obs_point"], lam, loss, scale, v["vinv"], v["obs_ok"], v["obs_lin"], v["jt"], v["obs_w"],
                                              v["T"], v["terms"], v["sums"], v["B"], v["C"], v["h"], v["free"], stream)

    def stp(c=c, n=n, t=t, G=G, **kw):
        v = {**a, **kw}
        return lib.vc_ba_step_radial(v["cams"], c, v["cam_dist"], v["group"], G, v["intr"], v["points"], n, v["offsets"], v["obs_cam"], t,
                                     v["vinv"], v["gp"], v["obs_ok"], v["obs_lin"], v["T"], v["dc"], v["dtheta"], v["out_cams"], v["dist"],
                                     v["out_points"], v["dx"], v["valid"], stream)

    nothing = {k: None for k in a}
    assert pts(n=0, **nothing) == lin(n=0, **nothing) == lin(G=0, **nothing) == red(G=0, **nothing) == stp(c=0, n=0, **nothing) == _lib.VC_OK
    for k in ("cams", "cam_dist", "mask", "points", "offsets", "obs_cam", "obs_xy", "vinv", "gp", "cost", "count", "obs_ok", "obs_lin", "obs_w",
              "total_cost"):
        assert pts(**{k: None}) == _lib.VC_ERR_INVALID_ARG, k
    for k in ("cams", "cam_dist", "group", "intr", "points", "offsets", "obs_cam", "vinv", "gp", "obs_ok", "obs_lin", "obs_w", "jt", "T", "terms"):
        assert lin(**{k: None}) == _lib.VC_ERR_INVALID_ARG, k
    for k in ("group", "intr", "offsets", "obs_cam", "cam_offsets", "cam_obs", "obs_point", "vinv", "obs_ok", "obs_lin", "jt", "obs_w", "T", "terms",
              "sums", "B", "C", "h", "free"):
        assert red(**{k: None}) == _lib.VC_ERR_INVALID_ARG, k
    for k in ("cams", "cam_dist", "group", "intr", "points", "offsets", "obs_cam", "vinv", "gp", "obs_ok", "obs_lin", "T", "dc", "dtheta", "out_cams",
              "dist", "out_points", "dx", "valid"):
        assert stp(**{k: None}) == _lib.VC_ERR_INVALID_ARG, k
    for size in ("c", "n", "t"):
        assert pts(**{size: -1}) == lin(**{size: -1}) == red(**{size: -1}) == stp(**{size: -1}) == _lib.VC_ERR_INVALID_ARG, size
    assert lin(G=-1) == red(G=-1) == stp(G=-1) == _lib.VC_ERR_INVALID_ARG
    for bad in (-1.0, float("nan"), float("inf")):
        assert pts(lam=bad) == red(lam=bad) == _lib.VC_ERR_INVALID_ARG
    for loss, scale in ((-1, 1.0), (3, 1.0), (1, 0.0), (2, -1.0), (1, float("nan")), (0, float("inf"))):
        assert pts(loss=loss, scale=scale) == lin(loss=loss, scale=scale) == red(loss=loss, scale=scale) == _lib.VC_ERR_INVALID_ARG, (loss, scale)
    assert lin(G=MAX_GROUPS + 1) == red(G=MAX_GROUPS + 1) == stp(G=MAX_GROUPS + 1) == _lib.VC_ERR_UNSUPPORTED
    assert red(c=_lib.VC_BA_MAX_CAMS + 1) == _lib.VC_ERR_UNSUPPORTED
    assert 4 <= _lib.VC_BA_MAX_GROUPS_RADIAL == MAX_GROUPS <= _lib.VC_BA_MAX_GROUPS
    torch.cuda.synchronize()
    assert all((b == 7).all() for b in bufs.values())                 # nothing was launched
    # the front end names the limit, and wants a distortion per slot
    from vit_colmap_amd.mapping.bundle import bundle_adjust

    with pytest.raises(ValueError, match="VC_BA_MAX_GROUPS_RADIAL"):
        bundle_adjust(*problem, "cuda", cam_group=np.zeros(c, np.int32), intr_mask=np.zeros(MAX_GROUPS + 1, np.uint8), cam_dist=np.zeros((c, 2)))
    with pytest.raises(ValueError, match="cam_dist"):
        bundle_adjust(*problem, "cuda", cam_dist=np.zeros((c + 1, 2)))


def test_bundle_adjust_with_cam_dist_follows_the_specification_on_the_distorted_problem():
    """Measured (1x MI355X): decisions [True] * 5 in 6 linearisations in both loops, final cost 226.381754947 (relative difference
    2.51e-16), k1 -0.164738806877 (relative difference 2.86e-15); the test prints both figures before it asserts."""
    from vit_colmap_amd.mapping.bundle import bundle_adjust

    problem = distorted()[3]
    n = len(problem[0])
    cam_group, intr_mask = np.zeros(n, np.int32), np.array([K1_FREE], np.uint8)
    cams, points, report = bundle_adjust(*problem, "cuda", max_iterations=500, cam_group=cam_group, intr_mask=intr_mask, cam_dist=np.zeros((n, 2)))
    spec_cams, spec_dist, _, spec = recovered()["k1"]
    k1 = report["cam_dist"][0, 0]
    rel = abs(report["final_cost"] - spec["final_cost"]) / spec["final_cost"]
    rel_k = abs(k1 - spec_dist[0, 0]) / abs(spec_dist[0, 0])
    print(f"decisions {report['decisions']} (spec {spec['decisions']}), final cost {report['final_cost']:.12g} (spec {spec['final_cost']:.12g}, "
          f"relative difference {rel:.3g}), k1 {k1:.12f} (spec {spec_dist[0, 0]:.12f}, relative difference {rel_k:.3g})")
    assert report["decisions"] == spec["decisions"] and report["iterations"] == spec["iterations"]
    assert report["accepted_steps"] == spec["accepted_steps"] and report["final_lambda"] == spec["final_lambda"]
    assert report["initial_cost"] == spec["initial_cost"]             # the kernel's order is the specification's
    assert rel <= LOOP_COST_REL and rel_k <= LOOP_K1_REL
    assert (report["cam_dist"][:, 0] == k1).all() and not report["cam_dist"][:, 1].any() and np.array_equal(cams[:, 12:], problem[0][:, 12:])
    assert report["intrinsics"]["before"].shape == (1, 6) and np.array_equal(report["intrinsics"]["after"][0], [*cams[0, 12:], k1, 0.0])
    assert abs(k1 - ur.K1_TRUE) <= K1_BOUND
    # without cam_dist there is no distortion in the report, with groups or without
    plain = bundle_adjust(*ub.random_problem(7), "cuda")[2]
    assert "cam_dist" not in plain and "intrinsics" not in plain
    p7 = ub.random_problem(7)
    grouped = bundle_adjust(*p7, "cuda", cam_group=np.zeros(len(p7[0]), np.int32), intr_mask=np.array([ui.TIED | ui.HOLD_PRINCIPAL], np.uint8))[2]
    assert "cam_dist" not in grouped and grouped["intrinsics"]["after"].shape == (1, 4)


def write_radial_db(path, scene):
    """The scene as a SIMPLE_RADIAL database with k = 0 and a focal prior, as the extractors write it."""
    K = scene["K"]
    write_windowed_db(path, scene)
    set_camera_model(path, "SIMPLE_RADIAL", [K[0, 0], K[0, 2], K[1, 2], 0.0])


@pytest.fixture(scope="module")
def end_to_end(tmp_path_factory):
    """A SIMPLE_RADIAL database of the distorted scene -> matched, grown, adjusted with k held and with it refined (once for the
    tests below)."""
    from vit_colmap_amd.mapping.bundle import build_adjusted_model
    from vit_colmap_amd.mapping.grow import build_sparse_model
    from vit_colmap_amd.matching import match_exhaustive
    from vit_colmap_amd.utils.config import MatchingConfig

    directory = tmp_path_factory.mktemp("bundle_radial_end_to_end")
    write_radial_db(directory / "r.db", distorted()[0])
    match_exhaustive(database_path=str(directory / "r.db"), matching_options=MatchingConfig(compute_relative_pose=True).to_matching_options())
    rows_before = _two_view_bytes(directory / "r.db")
    grown = build_sparse_model(directory / "r.db")
    held = build_adjusted_model(directory / "r.db", grown=grown)
    model = build_adjusted_model(directory / "r.db", grown=grown, refine_distortion=True)
    return grown, held, model, rows_before == _two_view_bytes(directory / "r.db"), directory


def test_match_exhaustive_then_build_adjusted_model_with_refined_distortion_end_to_end(end_to_end):
    """From k = 0 for a true k1 of -0.15 the adjusted cameras.txt carries k1 -0.164739 (off by 0.0147, as the CPU chain; 1x MI355X),
    cost 1090.74 -> 226.3818 in 6 linearisations where k held at 0 ends at 233.3111; the bound is the CPU chain's K1_BOUND."""
    from vit_colmap_amd.mapping import SparseModel

    grown, held, model, rows_unchanged, directory = end_to_end
    (cid, cam), = model.cameras.items()
    k1 = float(cam.params[3])
    ba = model.stats()["bundle_adjustment"]
    print(f"k1 0 -> {k1:.6f} for {ur.K1_TRUE} (off by {abs(k1 - ur.K1_TRUE):.4f}), cost {ba['initial_cost']:.2f} -> {ba['final_cost']:.4f} in "
          f"{ba['iterations']} linearisations (held: {held.bundle_adjustment['final_cost']:.4f}), {len(grown.points3D)} -> {len(model.points3D)} points")
    assert sorted(model.images) == list(range(1, 13)) and held.cameras == grown.cameras and "intrinsics" not in held.stats()["bundle_adjustment"]
    assert cam.model == "SIMPLE_RADIAL" and list(cam.params[:3]) == list(grown.cameras[cid].params[:3]) and grown.cameras[cid].params[3] == 0.0
    assert abs(k1 - ur.K1_TRUE) <= K1_BOUND <= 0.5 * abs(ur.K1_TRUE)
    f, cx, cy = (float(v) for v in cam.params[:3])
    assert ba["intrinsics"][cid] == dict(before=[f, f, cx, cy, 0.0, 0.0], after=[f, f, cx, cy, k1, 0.0])
    assert ba["final_cost"] < held.bundle_adjustment["final_cost"] < ba["initial_cost"] and ba["accepted_steps"] >= 1
    for p in model.points3D.values():
        assert len(p["track"]) >= 2 and p["error"] <= ub.MAX_ERROR
    model.write_text(directory / "adjusted")
    assert SparseModel.read_text(directory / "adjusted") == model
    assert rows_unchanged                                             # building any of the models only reads: the rows are byte for byte what matching wrote


def test_pipeline_with_the_flag_changes_only_the_distortion_of_the_adjusted_cameras(tmp_path, monkeypatch):
    from vit_colmap_amd.pipeline import run_pipeline as rp
    from vit_colmap_amd.utils.config import Config

    class StubExtractor:
        device = "cuda"
        prior_focal_length = False

        def extract(self, image_dir, db_path, camera_model, camera_params):
            pass

    monkeypatch.setattr(rp.Pipeline, "_make_extractor", lambda self: StubExtractor())
    write_radial_db(tmp_path / "r.db", distorted()[0])
    cfg = Config()
    cfg.camera.prior_focal_length, cfg.matching.compute_relative_pose, cfg.do_reconstruction = True, True, False
    cfg.reconstruction.sparse_model, cfg.reconstruction.bundle_adjustment, cfg.reconstruction.refine_distortion = True, True, True
    p = rp.Pipeline(cfg)
    p.run(tmp_path / "images", tmp_path / "out", tmp_path / "r.db")
    a, b = ((tmp_path / "out" / "sparse" / m / "cameras.txt").read_text().splitlines() for m in ("grown", "adjusted"))
    differing = [(x.split(), y.split()) for x, y in zip(a, b) if x != y]
    assert len(a) == len(b) and len(differing) == 1
    wx, wy = differing[0]                                              # id, SIMPLE_RADIAL, width, height, f, cx, cy, k
    assert wx[1] == "SIMPLE_RADIAL" and wx[:7] == wy[:7] and float(wx[7]) == 0.0 and abs(float(wy[7]) - ur.K1_TRUE) <= K1_BOUND
    report = p.last_stats["bundle_adjustment"]["bundle_adjustment"]["intrinsics"]
    assert repr(report[int(wy[0])]["after"][4]) == wy[7] and "intrinsics" not in p.last_stats["sparse_model"]
