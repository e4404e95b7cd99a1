"""CPU tests of bundle adjustment: the numpy specification of tests/util_bundle.py (derivatives, the exact
scene, held parameters, the drift it removes from the grown model of the windowed scene), the kernels' routines compiled for
the host (tools/bundle_host.cpp, whose helpers here the other bundle tests share) against it, plain and under the host
sanitizers, the product's host logic with the specification in its four GPU seams, and the pipeline's flag.  No GPU."""
import os
import shutil
import subprocess
import sys
from functools import lru_cache

import numpy as np
import pytest

import util_absolute_pose as ua
import util_bundle as ub
import util_bundle_intr as ui
import util_mapper as um
from test_absolute_pose_spec import scene_images, spec_estimate, spec_two_view_pose, write_scene_db
from test_mapper_spec import spec_triangulate, windowed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
HOST_BUILD = [HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off"]
SOURCE = os.path.join(ROOT, "tools", "bundle_host.cpp")
# the adjusted poses of the 12-view windowed scene (truth_pairs rows), measured: worst rotation 0.0577 deg, worst centre 0.00461
# baselines, where the grown model has 1.52 deg and 0.0853; the bounds are 2x, rounded up
BA_ROT_BOUND, BA_POS_BOUND = 0.12, 0.0093
# central differences of the specification's own residual with step 1e-6 (rad, scene units) against its J_c and J_p on 20
# observations, measured: worst |difference| 4.0e-8 where the largest entry of the observation's Jacobians is 1.5e2, worst ratio
# 4.2e-10 (it is the rounding of two residuals, each some 640 * 2^-52 ~ 1e-13 px, divided by twice the step; a step of 1e-5
# trades it for the step's square times the third derivative and is no better); the bound is 4x the measured ratio, rounded up
FD_STEP, FD_REL_BOUND = 1e-6, 2e-9


@lru_cache(maxsize=None)
def adjusted():
    """The windowed scene's grown model, its arrays and the specification's adjusted model."""
    scene, pairs, _, grown = windowed()
    images = scene_images(scene)
    return scene, images, grown, ub.model_problem(images, grown), ub.adjust_model(images, grown)


# ---- the specification ---------------------------------------------------------------------------------------------------------------
def test_jacobians_match_central_differences_of_the_residual():
    worst = 0.0
    for i in range(20):
        cams, points, offsets, obs_cam, obs_xy, _ = ub.random_problem(i)
        o = (7 * i) % len(obs_cam)
        j = int(np.searchsorted(offsets, o, side="right") - 1)
        row, X, uv = cams[obs_cam[o]], points[j], obs_xy[o]
        usable, r, Jc, Jp = ub.observe(row, X, uv)
        assert usable and np.abs(r - ub.residual_at(row, X, uv, np.zeros(3), np.zeros(3))).max() <= 1e-10
        num_c, num_p = np.zeros((2, 6)), np.zeros((2, 3))
        for k in range(6):
            e = np.zeros(6)
            e[k] = FD_STEP
            num_c[:, k] = (ub.residual_at(row, X, uv, e[:3], e[3:]) - ub.residual_at(row, X, uv, -e[:3], -e[3:])) / (2 * FD_STEP)
        for k in range(3):
            e = np.zeros(3)
            e[k] = FD_STEP
            num_p[:, k] = (ub.residual_at(row, X + e, uv, np.zeros(3), np.zeros(3)) - ub.residual_at(row, X - e, uv, np.zeros(3), np.zeros(3))) / (2 * FD_STEP)
        scale = max(np.abs(Jc).max(), np.abs(Jp).max())
        diff = max(np.abs(num_c - Jc).max(), np.abs(num_p - Jp).max())
        worst = max(worst, diff / scale)
        assert diff <= FD_REL_BOUND * scale, (i, diff, scale)
        # a held parameter's column is zero, the others are what they were
        _, _, held, _ = ub.observe(row, X, uv, 0b100101)
        assert not held[:, [0, 2, 5]].any() and np.array_equal(held[:, [1, 3, 4]], Jc[:, [1, 3, 4]])
    print(f"worst relative difference to central differences {worst:.3g}")


def exact_problem():
    """The windowed scene's true poses and points with exact projections in every view that sees a point."""
    scene = um.windowed_scene()
    cams = np.stack([um.camera_row(R, t, scene["K"]) for R, t in scene["poses"]])
    seen = np.stack(scene["visible"], axis=1)                                # (points, views)
    keep = np.nonzero(seen.sum(axis=1) >= 2)[0]
    obs_cam = np.concatenate([np.nonzero(seen[i])[0] for i in keep]).astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum(seen[keep].sum(axis=1))]).astype(np.int32)
    points = scene["X"][keep]
    Xc = np.einsum("nij,nj->ni", cams[obs_cam, :9].reshape(-1, 3, 3), np.repeat(points, np.diff(offsets), axis=0)) + cams[obs_cam, 9:12]
    obs_xy = np.stack([cams[obs_cam, 12] * Xc[:, 0] / Xc[:, 2] + cams[obs_cam, 14], cams[obs_cam, 13] * Xc[:, 1] / Xc[:, 2] + cams[obs_cam, 15]], axis=1)
    return cams, points, offsets, obs_cam, obs_xy, ub.gauge_mask(cams, 8, 10)


def test_exact_scene_has_cost_zero_and_a_zero_step():
    """Pixels computed in another order than the specification's leave residuals of rounding size, 640 * 2^-52 ~ 1e-13 px, so
    a cost of order 1e3 observations * 1e-26 and a step of that size times the conditioning of the scene (below 1e4)."""
    cams, points, offsets, obs_cam, obs_xy, mask = exact_problem()
    lin = ub.linearize(cams, points, offsets, obs_cam, obs_xy, mask, ub.BA_LAMBDA0)
    assert len(points) > 900 and lin["ok"].all() and not lin["constant"].any() and (lin["count"] == np.diff(offsets)).all()
    S, g = ub.reduce_cameras(lin, len(cams), offsets, obs_cam, mask, *ub.camera_index(obs_cam, offsets, len(cams)), ub.BA_LAMBDA0)
    dc = ub.solve_cameras(S, g, mask)
    _, _, dX = ub.step(lin, cams, points, offsets, obs_cam, dc)
    print(f"cost {lin['total_cost']:.3g}, worst |dc| {np.abs(dc).max():.3g}, worst |dX| {np.abs(dX).max():.3g}")
    assert lin["total_cost"] <= 1e-20 and np.abs(dc).max() <= 1e-9 and np.abs(dX).max() <= 1e-9
    assert np.allclose(S, S.T, rtol=0, atol=1e-9 * np.abs(S).max()) and np.linalg.eigvalsh(S).min() > 0
    out_cams, out_points, report = ub.bundle_adjust(cams, points, offsets, obs_cam, obs_xy, mask)
    assert report["final_cost"] <= 1e-20 and np.abs(out_cams - cams).max() <= 1e-9 and np.abs(out_points - points).max() <= 1e-9


def test_with_every_camera_held_each_point_takes_its_own_gauss_newton_step():
    cams, points, offsets, obs_cam, obs_xy = adjusted()[3][1:]
    # the grown model's points are refitted already: moved by 0.01 so that a step is not the rounding of a vanished gradient
    points = points + np.random.RandomState(4).normal(0, 0.01, points.shape)
    mask = np.full(len(cams), ub.HELD_ALL, np.uint8)
    lam = ub.BA_LAMBDA0
    lin = ub.linearize(cams, points, offsets, obs_cam, obs_xy, mask, lam)
    S, g = ub.reduce_cameras(lin, len(cams), offsets, obs_cam, mask, *ub.camera_index(obs_cam, offsets, len(cams)), lam)
    assert np.array_equal(S, np.eye(6 * len(cams))) and not g.any() and not lin["W"].any()
    dc = ub.solve_cameras(S, g, mask)
    assert not dc.any()
    out_cams, _, dX = ub.step(lin, cams, points, offsets, obs_cam, dc)
    assert np.array_equal(out_cams, cams)                            # a zero step leaves every bit of a pose
    worst = 0.0
    for j in range(0, len(points), 7):
        rows = [ub.observe(cams[obs_cam[o]], points[j], obs_xy[o]) for o in range(offsets[j], offsets[j + 1])]
        J, r = np.concatenate([row[3] for row in rows]), np.concatenate([row[1] for row in rows])
        A = J.T @ J
        want = np.linalg.solve(A + lam * np.diag(np.diag(A)), -J.T @ r)
        worst = max(worst, np.abs(dX[j] - want).max() / np.abs(want).max())
    print(f"worst relative difference to the independent 3x3 step {worst:.3g}")
    assert worst <= 1e-9                                             # two solutions of a 3x3 system of condition below 1e6


def test_adjustment_removes_the_drift_of_the_grown_model():
    """The test that fails without bundle adjustment: the adjusted poses are at most a quarter of the grown model's drift away
    from the truth in both numbers (measured: a 26th and an 18th)."""
    scene, images, grown, problem, adj = adjusted()
    a, b = grown["initial_pair"]
    rot0, pos0 = ua.align_errors(grown["poses"], scene, a, b)
    rot, pos = ua.align_errors(adj["poses"], scene, a, b)
    report = adj["report"]
    print(f"rotation {rot0:.4f} -> {rot:.4f} deg, centre {pos0:.5f} -> {pos:.5f} baselines, cost {report['initial_cost']:.2f} -> "
          f"{report['final_cost']:.2f} in {report['iterations']} linearisations, {report['accepted_steps']} accepted, lambda {report['final_lambda']:.3g}; "
          f"{len(grown['xyz']) - len(adj['xyz'])} points and {sum(map(len, grown['tracks'])) - sum(map(len, adj['tracks']))} observations filtered")
    assert rot <= rot0 / 4 and pos <= pos0 / 4
    assert rot <= BA_ROT_BOUND and pos <= BA_POS_BOUND
    assert report["final_cost"] < report["initial_cost"] and report["accepted_steps"] >= 1
    assert report["iterations"] <= ub.BA_MAX_ITERATIONS and report["decisions"].count(True) == report["accepted_steps"]
    # every held parameter is bit-equal before the rescale
    before, after, mask = adj["held"]
    ids = sorted(grown["poses"])
    sa, sb = ids.index(a), ids.index(b)
    assert mask[sa] == ub.HELD_ALL and bin(mask[sb]).count("1") == 1 and mask.sum() == ub.HELD_ALL + mask[sb]
    assert np.array_equal(after[sa], before[sa])
    k = int(mask[sb]).bit_length() - 1
    assert k == 3 + int(np.argmax(np.abs(before[sb, 9:12]))) and after[sb, 9 + k - 3] == before[sb, 9 + k - 3]
    assert not np.array_equal(after[sb], before[sb]) and np.array_equal(after[:, 12:], before[:, 12:])       # intrinsics are not refined
    # the rescale: the pair's baseline is 1
    centre = {i: -adj["poses"][i][0].T @ adj["poses"][i][1] for i in (a, b)}
    assert abs(np.linalg.norm(centre[b] - centre[a]) - 1.0) <= 1e-12
    # the filter: every kept observation is within MAX_ERROR, every kept point has two or more
    assert all(len(t) >= 2 for t in adj["tracks"]) and (adj["error"] <= ub.MAX_ERROR).all()
    assert adj["point_ids"] == sorted(adj["point_ids"]) and set(adj["point_ids"]) <= set(range(1, len(grown["xyz"]) + 1))


def test_filter_drops_a_gross_observation_and_a_point_without_parallax():
    cams, points, offsets, obs_cam, obs_xy, _ = exact_problem()
    obs_xy = obs_xy.copy()
    long = int(np.nonzero(np.diff(offsets) >= 3)[0][0])
    obs_xy[offsets[long]] += [30.0, 0.0]                              # one observation of a long track goes, the point stays
    short = int(np.nonzero(np.diff(offsets) == 2)[0][0])
    obs_xy[offsets[short] + 1] += [0.0, 30.0]                         # a track of two loses one: the point goes
    keep_obs, keep_point, error = ub.filter_tracks(cams, points, offsets, obs_cam, obs_xy)
    assert not keep_obs[offsets[long]] and keep_point[long] and keep_obs[offsets[long] + 1:offsets[long + 1]].all()
    assert not keep_point[short] and not keep_obs[offsets[short]:offsets[short + 1]].any() and np.isnan(error[short])
    assert keep_point.sum() == len(points) - 1 and keep_obs.sum() == len(obs_cam) - 3
    # two cameras at one centre: no parallax
    twin = cams[[0, 0]].copy()
    X = points[:1]
    Xc = twin[0, :9].reshape(3, 3) @ X[0] + twin[0, 9:12]
    uv = np.array([twin[0, 12] * Xc[0] / Xc[2] + twin[0, 14], twin[0, 13] * Xc[1] / Xc[2] + twin[0, 15]])
    keep_obs, keep_point, _ = ub.filter_tracks(twin, X, np.array([0, 2]), np.array([0, 1]), np.stack([uv, uv]))
    assert not keep_point[0] and not keep_obs.any()


# ---- the kernels' routines on the host ---------------------------------------------------------------------------------------------------
def write_problem_file(path, problem, lam, dc, index=None, groups=None, dtheta=()):
    """The input of tools/bundle_host.cpp; `index`: cam_offsets, cam_obs, obs_point where they are not ub.camera_index's;
    `groups`: cam_group, intr_mask and with them `dtheta` for the border's section."""
    cams, points, offsets, obs_cam, obs_xy, mask = problem
    cam_group, intr_mask = groups or ((), ())
    cam_offsets, cam_obs, obs_point = index or ub.camera_index(obs_cam, offsets, len(cams))
    with open(path, "wb") as f:
        f.write(np.array([len(cams), len(points), len(obs_cam), len(intr_mask)], np.int32).tobytes())
        f.write(np.array([lam], np.float64).tobytes())
        for a in (offsets, obs_cam, cam_offsets, cam_obs, obs_point, mask, cam_group, intr_mask):
            f.write(np.ascontiguousarray(a).astype(np.int32).tobytes())
        for a in (cams, points, obs_xy, dc, dtheta):
            f.write(np.ascontiguousarray(a, np.float64).tobytes())


def result_shapes(n_cams, n_points, total, G):
    """The float64 arrays of the border's section."""
    rows = 24 * G + 16 * G * G
    return [("xn", (total, 2)), ("T", (n_points, G, 12)), ("terms", (rows, n_points)), ("sums", (rows,)), ("B", (6 * n_cams, 4 * G)),
            ("C", (4 * G, 4 * G)), ("h", (4 * G,)), ("cams", (n_cams, 16)), ("points", (n_points, 3)), ("dx", (n_points, 3))]


def read_result_file(path, n_cams, n_points, total, G=0):
    """-> the plain section; with groups the border's section, the plain one under "plain"."""
    raw = open(path, "rb").read()
    at = 0

    def take(dtype, shape):
        nonlocal at
        n = int(np.prod(shape))
        a = np.frombuffer(raw, dtype, n, at).reshape(shape)
        at += a.nbytes
        return a

    shapes = [("vinv", (n_points, 6)), ("gp", (n_points, 3)), ("cost", (n_points,)), ("total_cost", (1,)), ("S", (6 * n_cams, 6 * n_cams)),
              ("g", (6 * n_cams,)), ("cams", (n_cams, 16)), ("points", (n_points, 3)), ("dx", (n_points, 3)), ("obs_lin", (total, 32))]
    out = {name: take(np.float64, shape) for name, shape in shapes}
    out["count"], out["obs_ok"] = take(np.int32, (n_points,)), take(np.uint8, (total,))
    if G:
        out = dict({name: take(np.float64, shape) for name, shape in result_shapes(n_cams, n_points, total, G)}, plain=out)
        out["free"], out["valid"] = take(np.uint8, (4 * G,)), take(np.uint8, (n_cams,))
    assert at == len(raw)
    return out


def run_host(program, tmp_path, problem, lam, dc, index=None, groups=None, dtheta=()):
    write_problem_file(tmp_path / "problem.bin", problem, lam, dc, index, groups, dtheta)
    done = subprocess.run([program, str(tmp_path / "problem.bin"), str(tmp_path / "result.bin")], stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, text=True)
    assert done.returncode == 0, done.stderr
    G = len(groups[1]) if groups else 0
    return read_result_file(tmp_path / "result.bin", len(problem[0]), len(problem[1]), len(problem[3]), G), done.stderr


def spec_pass(problem, lam=ub.BA_LAMBDA0):
    """One linearisation, reduction, solve and step of the specification -> dict in the host program's layout; a system that
    does not factor steps with dc = 0."""
    cams, points, offsets, obs_cam, obs_xy, mask = problem
    lin = ub.linearize(cams, points, offsets, obs_cam, obs_xy, mask, lam)
    S, g = ub.reduce_cameras(lin, len(cams), offsets, obs_cam, mask, *ub.camera_index(obs_cam, offsets, len(cams)), lam)
    dc = ub.solve_cameras(S, g, mask)
    dc = np.zeros(6 * len(cams)) if dc is None else dc
    out_cams, out_points, dX = ub.step(lin, cams, points, offsets, obs_cam, dc)
    vinv = lin["vinv"].reshape(-1, 9)[:, [0, 1, 2, 4, 5, 8]]
    return dict(vinv=vinv, gp=lin["gp"], cost=lin["cost"], total_cost=np.array([lin["total_cost"]]), S=S, g=g, cams=out_cams,
                points=out_points, dx=dX, count=lin["count"], obs_ok=lin["ok"].astype(np.uint8), constant=lin["constant"], dc=dc)


def relative_differences(host, spec, what):
    """The usable counts, the usable observations and the constant points are equal -> {array: max |host - spec| / max |spec|}."""
    assert np.array_equal(host["count"], spec["count"]) and np.array_equal(host["obs_ok"], spec["obs_ok"]), what
    assert np.array_equal(~host["vinv"].any(axis=1), spec["constant"]), what
    out = {}
    for k in ("vinv", "gp", "S", "g", "dx", "cost", "cams", "points"):
        scale = np.abs(spec[k][np.isfinite(spec[k])]).max(initial=0.0)
        assert np.array_equal(np.isfinite(host[k]), np.isfinite(spec[k])), (what, k)
        diff = np.abs(np.where(np.isfinite(spec[k]), host[k] - spec[k], 0.0)).max(initial=0.0)
        out[k] = diff / scale if scale else float(diff != 0) * np.inf
    return out


SANITIZE = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-Xarch_host", "-g"]
_BUILT = {}


def _build(tmp_path_factory, name, extra=()):
    """tools/bundle_host.cpp built with the line its source gives and `extra`, once per session and name."""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc to build the host program with")
    if name not in _BUILT:
        out = tmp_path_factory.mktemp(name) / name
        proc = subprocess.run(HOST_BUILD + list(extra) + ["-o", str(out), SOURCE], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert proc.returncode == 0, f"{name} does not build:\n{proc.stdout}"
        _BUILT[name] = str(out)
    return _BUILT[name]


@pytest.fixture(scope="session")
def bundle_host(tmp_path_factory):
    """The host program (the other bundle tests share it)."""
    return _build(tmp_path_factory, "bundle_host")


def host_problems():
    """The windowed problem, the 300 random ones and the edge cases -> [(name, problem)]."""
    _, _, grown, problem, adj = adjusted()
    windowed_problem = (*problem[1:], adj["held"][2])
    return ([("windowed", windowed_problem)] + [(f"random {i}", ub.random_problem(i)) for i in range(300)]
            + sorted(ub.edge_problems().items()))


@lru_cache(maxsize=None)
def spec_passes():
    return [(name, problem, spec_pass(problem)) for name, problem in host_problems()]


def test_edge_problems_are_what_they_say():
    edge = {name: s for name, _, s in spec_passes() if not name.startswith(("windowed", "random"))}
    base = spec_pass(ub.random_problem(7))
    assert base["obs_ok"].all() and not base["constant"].any()
    for name in ("slot_first", "slot_last", "nan_pixel"):
        assert (edge[name]["obs_ok"] == 0).sum() == 1, name
    assert (edge["nan_camera"]["obs_ok"] == 0).sum() >= 2 and (edge["behind"]["obs_ok"] == 0).sum() >= 2
    for name in ("nan_camera", "empty_camera"):                      # a camera nothing moves: the identity block, a zero step
        a = 2 if name == "nan_camera" else len(edge[name]["S"]) // 6 - 1
        block = edge[name]["S"][6 * a:6 * a + 6]
        assert np.array_equal(block[:, 6 * a:6 * a + 6], np.eye(6)) and np.abs(block).sum() == 6 and not edge[name]["dc"][6 * a:6 * a + 6].any()
    s = edge["short_tracks"]
    assert s["count"][0] == 0 and s["count"][-1] == 1 and s["constant"][0] and s["constant"][-1] and not s["dx"][[0, -1]].any()
    assert s["cost"][0] == 0 and s["cost"][-1] > 0
    assert edge["camera_twice"]["obs_ok"].all() and not np.array_equal(edge["camera_twice"]["S"], base["S"])
    assert not edge["partly_held"]["dc"][[13, 15]].any() and edge["partly_held"]["dc"][[12, 14, 16, 17]].all()
    assert all(np.isfinite(s["dc"]).all() and s["dc"].any() for s in edge.values())


def test_host_build_matches_the_spec_on_the_windowed_the_random_and_the_edge_problems(bundle_host, tmp_path):
    worst = {}
    for name, problem, spec in spec_passes():
        host, _ = run_host(bundle_host, tmp_path, problem, ub.BA_LAMBDA0, spec["dc"])
        for k, v in relative_differences(host, spec, name).items():
            if v > worst.get(k, (-1.0, ""))[0]:
                worst[k] = (v, name)
    print("worst relative differences host - spec: " + ", ".join(f"{k} {v:.3g} ({name})" for k, (v, name) in sorted(worst.items())))
    assert ub.TOL_REL == 4 * ub.HOST_SPEC_REL
    assert max(worst[k][0] for k in ("vinv", "gp", "S", "g", "dx")) <= ub.HOST_SPEC_REL
    assert max(v for v, _ in worst.values()) <= ub.TOL_REL


def test_host_build_under_the_sanitizers_reports_nothing(tmp_path, tmp_path_factory):
    """The same program with the host half built -fsanitize=address,undefined, run on its own over the same problems."""
    program = _build(tmp_path_factory, "bundle_host_san", SANITIZE)
    for name, problem, spec in spec_passes():
        host, stderr = run_host(program, tmp_path, problem, ub.BA_LAMBDA0, spec["dc"])
        assert stderr == "" and np.array_equal(host["count"], spec["count"]), name
    # indices that name nothing: offsets that descend and that pass the arrays, observations of another camera or outside
    cams, points, offsets, obs_cam, obs_xy, mask = ub.random_problem(7)
    bad = offsets.copy()
    bad[3], bad[-1] = bad[4] + 1, len(obs_cam) + 5
    host, stderr = run_host(program, tmp_path, (cams, points, bad, obs_cam, obs_xy, mask), ub.BA_LAMBDA0, np.zeros(6 * len(cams)))
    assert stderr == "" and host["count"][3] == 0 and host["count"][-1] == 0 and np.isfinite(host["S"]).all()


def test_groups_leave_every_byte_of_the_plain_section(bundle_host, tmp_path):
    """The plain arrays are computed before and apart from the border: with groups the program writes the same bytes."""
    for seed, problem in ((7, ub.random_problem(7)), (8, ub.edge_problems()["short_tracks"])):
        groups = ui.random_groups(seed, len(problem[0]))
        dc = np.random.RandomState(seed).normal(0, 2e-3, 6 * len(problem[0]))
        dtheta = np.random.RandomState(seed).normal(0, 0.5, 4 * len(groups[1]))
        plain, _ = run_host(bundle_host, tmp_path, problem, ub.BA_LAMBDA0, dc)
        both, _ = run_host(bundle_host, tmp_path, problem, ub.BA_LAMBDA0, dc, groups=groups, dtheta=dtheta)
        assert len(groups[1]) >= 1 and sorted(both["plain"]) == sorted(plain) and len(plain) == 12
        for k, a in plain.items():
            assert both["plain"][k].tobytes() == a.tobytes(), (seed, k)


# ---- the product's host logic with the specification in its seams -----------------------------------------------------------------------
def spec_bundle(cams, points, offsets, obs_cam, obs_xy, const_mask, device):
    return ub.bundle_adjust(cams, points, offsets, obs_cam, obs_xy, const_mask)


def build_adjusted_with_spec(path, **kw):
    from vit_colmap_amd.mapping.bundle import build_adjusted_model

    return build_adjusted_model(path, device="cpu", two_view_pose_fn=spec_two_view_pose, estimate_fn=spec_estimate,
                                triangulate_fn=spec_triangulate, bundle_fn=spec_bundle, **kw)


def assert_adjusted_model_follows(model, spec, atol):
    assert sorted(model.images) == sorted(spec["poses"]) and sorted(model.points3D) == spec["point_ids"]
    for i, (R, t) in spec["poses"].items():
        assert np.allclose(ua.quat_to_rot(model.images[i]["qvec"]), R, atol=atol) and np.allclose(model.images[i]["tvec"], t, atol=atol)
    for pid, xyz, track, error in zip(spec["point_ids"], spec["xyz"], spec["tracks"], spec["error"]):
        p = model.points3D[pid]
        assert np.allclose(p["xyz"], xyz, atol=atol) and p["track"] == track and abs(p["error"] - error) <= 1e-6


def test_build_adjusted_model_with_the_spec_in_its_seams_equals_the_specs_pipeline(tmp_path):
    from vit_colmap_amd.mapping.grow import build_sparse_model
    from vit_colmap_amd.mapping.seed import SparseModel

    scene, images, grown, _, adj = adjusted()
    write_scene_db(tmp_path / "w.db", scene, windowed()[1])
    spec = adj                                                       # truth_pairs rows read back from a database equal
    grown_model = build_sparse_model(tmp_path / "w.db", device="cpu", two_view_pose_fn=spec_two_view_pose, estimate_fn=spec_estimate,
                                     triangulate_fn=spec_triangulate)
    before = (grown_model.stats(), {i: im["qvec"].copy() for i, im in grown_model.images.items()},
              {p: (q["xyz"].copy(), list(q["track"])) for p, q in grown_model.points3D.items()})
    model = build_adjusted_with_spec(tmp_path / "w.db")                # builds the grown model itself
    assert build_adjusted_with_spec(tmp_path / "w.db", grown=grown_model) == model          # or takes the caller's
    # the poses the product adjusts went through a quaternion and back, so the two loops start a rounding apart
    assert_adjusted_model_follows(model, spec, 1e-9)
    assert model.initial_pair == grown["initial_pair"] and model.rounds == grown["rounds"]
    for pid, p in model.points3D.items():
        for i, kp in p["track"]:
            assert model.images[i]["point3D_ids"][kp] == pid
    assert sum(int((im["point3D_ids"] >= 0).sum()) for im in model.images.values()) == sum(len(t) for t in spec["tracks"])
    s = model.stats()
    assert s["registered_images"] == 12 and s["num_points3D"] == len(spec["xyz"]) and s["rounds"] == grown["rounds"]
    ba = s["bundle_adjustment"]
    assert ba["iterations"] == spec["report"]["iterations"] and ba["accepted_steps"] == spec["report"]["accepted_steps"]
    assert ba["initial_cost"] == pytest.approx(spec["report"]["initial_cost"], rel=1e-9) and ba["final_cost"] == pytest.approx(spec["report"]["final_cost"], rel=1e-9)
    assert ba["final_lambda"] == spec["report"]["final_lambda"] and ba["filtered_points"] == len(grown["xyz"]) - len(spec["xyz"])
    # the grown model that was handed in is what it was, and has no such key
    assert "bundle_adjustment" not in grown_model.stats() and grown_model.stats() == before[0]
    assert all(np.array_equal(grown_model.images[i]["qvec"], q) for i, q in before[1].items())
    assert all(np.array_equal(grown_model.points3D[p]["xyz"], x) and grown_model.points3D[p]["track"] == t for p, (x, t) in before[2].items())
    # the text model reads back equal
    model.write_text(tmp_path / "adjusted")
    back = SparseModel.read_text(tmp_path / "adjusted")
    assert back == model and model == back
    assert_adjusted_model_follows(back, spec, 1e-9)


def test_front_end_refuses_more_cameras_than_the_kernel_holds_and_wrong_shapes():
    from vit_colmap_amd import _lib
    from vit_colmap_amd.mapping import bundle

    cams, points, offsets, obs_cam, obs_xy, mask = ub.random_problem(7)
    many = np.repeat(cams[:1], _lib.VC_BA_MAX_CAMS + 1, axis=0)
    with pytest.raises(ValueError, match="VC_BA_MAX_CAMS"):
        bundle.bundle_adjust(many, points, offsets, obs_cam, obs_xy, np.zeros(len(many), np.uint8), "cpu")
    with pytest.raises(ValueError, match="bundle_adjust needs"):
        bundle.bundle_adjust(cams, points, offsets[:-1], obs_cam, obs_xy, mask, "cpu")
    header = open(os.path.join(ROOT, "include", "vitcolmap_hip.h")).read()
    assert f"#define VC_BA_MAX_CAMS {_lib.VC_BA_MAX_CAMS}\n" in header
    batch = 64 * (4 * 4 + 18 * 8)                                     # what a workgroup keeps beside its row block
    assert 36 * _lib.VC_BA_MAX_CAMS * 8 + batch <= 160 * 1024 < 36 * 2 * _lib.VC_BA_MAX_CAMS * 8 + batch     # the CU's LDS binds
    # the product's index is the specification's
    for problem in (ub.random_problem(7), ub.edge_problems()["slot_last"], ub.edge_problems()["short_tracks"]):
        for got, want in zip(bundle.camera_index(problem[3], problem[2], len(problem[0])), ub.camera_index(problem[3], problem[2], len(problem[0]))):
            assert got.dtype == np.int32 and np.array_equal(got, want)
    assert (bundle.BA_LAMBDA0, bundle.BA_MAX_ITERATIONS, bundle.BA_REL_DECREASE, bundle.HELD_ALL) == (
        ub.BA_LAMBDA0, ub.BA_MAX_ITERATIONS, ub.BA_REL_DECREASE, ub.HELD_ALL)


# ---- the pipeline flag ------------------------------------------------------------------------------------------------------------------
def test_bundle_adjustment_flag_is_off_by_default_and_needs_the_sparse_model(tmp_path, monkeypatch):
    import argparse

    from vit_colmap_amd.pipeline import run_pipeline as rp
    from vit_colmap_amd.utils.config import Config, ReconstructionConfig

    assert ReconstructionConfig().bundle_adjustment is False and Config().reconstruction.bundle_adjustment is False
    assert Config.from_args(argparse.Namespace(bundle_adjustment=True)).reconstruction.bundle_adjustment is True
    assert Config.from_args(argparse.Namespace(bundle_adjustment=True)).reconstruction.sparse_model is False
    assert Config.from_args(argparse.Namespace()).reconstruction.bundle_adjustment is False

    def no_extractor(self):
        raise AssertionError("the extractor was built before the flags were checked")

    monkeypatch.setattr(rp.Pipeline, "_make_extractor", no_extractor)
    cfg = Config()
    cfg.reconstruction.bundle_adjustment = True
    cfg.camera.prior_focal_length, cfg.matching.compute_relative_pose, cfg.do_reconstruction = True, True, False
    with pytest.raises(ValueError, match="bundle_adjustment needs .*sparse_model"):
        rp.Pipeline(cfg).run(tmp_path / "images", tmp_path / "out", tmp_path / "x.db")
    cfg.reconstruction.sparse_model, cfg.camera.prior_focal_length = True, False          # the sparse model's own prerequisites still hold
    with pytest.raises(ValueError, match="sparse_model needs .*prior_focal_length"):
        rp.Pipeline(cfg).run(tmp_path / "images", tmp_path / "out", tmp_path / "x.db")
    assert not (tmp_path / "out" / "sparse").exists()
    seen = []
    monkeypatch.setattr(rp.Pipeline, "run", lambda self, *a, **k: seen.append((self.config.reconstruction.sparse_model,
                                                                               self.config.reconstruction.bundle_adjustment)))
    for extra in ([], ["--sparse-model"], ["--sparse-model", "--bundle-adjustment"]):
        monkeypatch.setattr(sys, "argv", ["prog", "--images", "i", "--output", "o", "--db", "d"] + extra)
        rp.main()
    assert seen == [(False, False), (True, False), (True, True)]
    code = ("import sys; import vit_colmap_amd.mapping; import vit_colmap_amd.mapping.grow; import vit_colmap_amd.pipeline.run_pipeline; "
            "assert 'vit_colmap_amd.mapping.bundle' not in sys.modules")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


def test_pipeline_writes_the_adjusted_model_beside_an_unchanged_grown_one(tmp_path, monkeypatch):
    import vit_colmap_amd.mapping
    import vit_colmap_amd.mapping.grow as grow
    from vit_colmap_amd.mapping.seed import SparseModel
    from vit_colmap_amd.pipeline import run_pipeline as rp
    from vit_colmap_amd.utils.config import Config

    scene, images, grown, _, adj = adjusted()
    write_scene_db(tmp_path / "w.db", scene, windowed()[1])
    real = grow.build_sparse_model
    monkeypatch.setattr(grow, "build_sparse_model", lambda path, device="cuda": real(path, device="cpu", two_view_pose_fn=spec_two_view_pose,
                                                                                     estimate_fn=spec_estimate, triangulate_fn=spec_triangulate))
    # with the flag off the adjustment is not imported (restored afterwards, so that later tests name the same module)
    if hasattr(vit_colmap_amd.mapping, "bundle"):
        monkeypatch.setattr(vit_colmap_amd.mapping, "bundle", vit_colmap_amd.mapping.bundle)
    monkeypatch.delitem(sys.modules, "vit_colmap_amd.mapping.bundle", raising=False)
    off = rp.Pipeline(Config())
    off.last_stats = {"verified_pairs": 10}
    off._write_sparse_model(tmp_path / "w.db", tmp_path / "off", "cpu")
    assert "vit_colmap_amd.mapping.bundle" not in sys.modules
    assert sorted(off.last_stats) == ["sparse_model", "verified_pairs"] and "bundle_adjustment" not in off.last_stats["sparse_model"]
    assert [f.name for f in (tmp_path / "off" / "sparse").iterdir()] == ["grown"]

    import vit_colmap_amd.mapping.bundle as bundle

    monkeypatch.setattr(bundle, "bundle_adjust", spec_bundle)
    on = rp.Pipeline(Config())
    on.last_stats = {"verified_pairs": 10}
    on._write_sparse_model(tmp_path / "w.db", tmp_path / "on", "cpu", adjust=True)
    assert sorted(f.name for f in (tmp_path / "on" / "sparse").iterdir()) == ["adjusted", "grown"]
    for name in ("cameras.txt", "images.txt", "points3D.txt"):       # sparse/grown is byte for byte what it is without the flag
        assert (tmp_path / "on" / "sparse" / "grown" / name).read_bytes() == (tmp_path / "off" / "sparse" / "grown" / name).read_bytes()
    assert on.last_stats["sparse_model"] == off.last_stats["sparse_model"] and on.last_stats["verified_pairs"] == 10
    ba = on.last_stats["bundle_adjustment"]
    assert ba["registered_images"] == 12 and ba["num_points3D"] == len(adj["xyz"])
    assert ba["bundle_adjustment"]["final_cost"] < ba["bundle_adjustment"]["initial_cost"]
    assert_adjusted_model_follows(SparseModel.read_text(tmp_path / "on" / "sparse" / "adjusted"), adj, 1e-9)
