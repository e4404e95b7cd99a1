"""CPU tests of the matrix-free solver of bundle adjustment ("The solver" in DESIGN.md §4.2k): the numpy specification of
tests/util_bundle_pcg.py against the dense system of tests/util_bundle.py (the right-hand side and the diagonal blocks as bytes,
the product against S p, the loop against the dense loop), the kernels' routines compiled for the host
(tools/bundle_pcg_host.cpp, whose helpers here the GPU tests share) against it, plain and under the host sanitizers, a
520-camera arc that the dense route refuses, the product's host logic with the specification in its seams, the configuration
and the command line.  No GPU."""
import os
import subprocess
import sys
from functools import lru_cache

import numpy as np
import pytest

import util_absolute_pose as ua
import util_bundle as ub
import util_bundle_pcg as up
import util_rounds as ur
from test_absolute_pose_spec import spec_estimate, spec_two_view_pose, write_scene_db
from test_bundle_spec import BA_POS_BOUND, BA_ROT_BOUND, HIPCC, HOST_BUILD, ROOT, SANITIZE, adjusted, host_problems
from test_mapper_spec import spec_triangulate, windowed

SOURCE = os.path.join(ROOT, "tools", "bundle_pcg_host.cpp")
N_VECTORS = 3


# ---- the specification against the dense system ------------------------------------------------------------------------------------
def vectors_of(k, fixed):
    """Three p of problem k from a fixed RandomState: the first two have non-zero entries at the fixed parameters, the third
    is 0 there."""
    p = np.random.RandomState(18000 + k).normal(0, 1, (N_VECTORS, len(fixed)))
    p[2, fixed] = 0.0
    return p


@lru_cache(maxsize=None)
def spec_systems():
    """Per problem of test_bundle_spec.host_problems: name, problem, the linearisation, the index, the dense S and g, the blocks,
    the three vectors and their (s, q)."""
    out = []
    for k, (name, problem) in enumerate(host_problems()):
        cams, points, offsets, obs_cam, obs_xy, mask = problem
        index = ub.camera_index(obs_cam, offsets, len(cams))
        lin = ub.linearize(cams, points, offsets, obs_cam, obs_xy, mask, ub.BA_LAMBDA0)
        S, g = ub.reduce_cameras(lin, len(cams), offsets, obs_cam, mask, *index, ub.BA_LAMBDA0)
        blocks = up.camera_blocks(lin, len(cams), offsets, obs_cam, mask, *index, ub.BA_LAMBDA0)
        p = vectors_of(k, blocks["fixed"])
        products = [up.schur_product(lin, blocks, offsets, obs_cam, index[2], v) for v in p]
        out.append(dict(name=name, problem=problem, lin=lin, index=index, S=S, g=g, blocks=blocks, p=p, s=np.stack([s for s, _ in products]),
                        q=np.stack([q for _, q in products])))
    return out


def test_blocks_and_right_hand_side_are_the_dense_systems_bytes():
    worst = 0.0
    for e in spec_systems():
        n, mask, b = len(e["problem"][0]), e["problem"][5], e["blocks"]
        assert b["g"].tobytes() == e["g"].tobytes(), e["name"]
        for a in range(n):
            assert np.ascontiguousarray(e["S"][6 * a:6 * a + 6, 6 * a:6 * a + 6]).tobytes() == np.ascontiguousarray(b["D"][a]).tobytes(), (e["name"], a)
        held = np.array([[(int(m) >> i) & 1 for i in range(6)] for m in mask], bool).reshape(-1)
        zero = np.array([not e["lin"]["Jc"][(e["problem"][3] == i // 6) & e["lin"]["ok"], :, i % 6].any() for i in range(6 * n)])
        assert np.array_equal(b["fixed"], held | zero), e["name"]
        # a fixed parameter: diagonal 1, zero row and column in U and D, g = 0
        f = b["fixed"].reshape(n, 6)
        for M in (b["U"], b["D"]):
            assert (M[f] == np.eye(6)[np.nonzero(f)[1]]).all() and (M.transpose(0, 2, 1)[f] == np.eye(6)[np.nonzero(f)[1]]).all(), e["name"]
        assert not b["g"][b["fixed"]].any()
        worst = max(worst, max(np.abs(b["Minv"][a] @ b["D"][a] - np.eye(6)).max() for a in range(n)))
    print(f"worst |M^-1 D - I| {worst:.3g}")
    assert worst <= 4 * up.MINV_IDENTITY


def test_product_matches_the_dense_s_times_p():
    worst, name = 0.0, ""
    for e in spec_systems():
        assert e["p"][:2][:, e["blocks"]["fixed"]].all() or not e["blocks"]["fixed"].any()
        for v, q in zip(e["p"], e["q"]):
            ref = e["S"] @ v
            rel = np.abs(q - ref).max() / np.abs(ref).max()
            if rel > worst:
                worst, name = rel, e["name"]
            assert np.array_equal(q[e["blocks"]["fixed"]], v[e["blocks"]["fixed"]])
    print(f"worst relative difference schur_product - S p {worst:.3g} ({name})")
    assert worst <= 4 * up.PRODUCT_DENSE_REL


def test_preconditioner_falls_back_to_the_identity():
    D = np.eye(6)
    D[3, 3] = -1.0
    assert np.array_equal(up.cholesky_inverse(D), np.eye(6))
    D[3, 3] = np.nan
    assert np.array_equal(up.cholesky_inverse(D), np.eye(6))
    A = np.random.RandomState(2).normal(size=(6, 6))
    D = A @ A.T + np.eye(6)
    assert np.abs(up.cholesky_inverse(D) @ D - np.eye(6)).max() <= 1e-12


def test_a_solve_that_breaks_down_ends_as_a_system_that_did_not_factor():
    e = spec_systems()[1]
    _, _, offsets, obs_cam, _, _ = e["problem"]
    n = len(e["blocks"]["fixed"])
    x, k = up.pcg_solve(e["lin"], e["blocks"], offsets, obs_cam, e["index"][2], product=lambda p: -p)
    assert x is None and k == 1                                       # p'q negative
    x, k = up.pcg_solve(e["lin"], e["blocks"], offsets, obs_cam, e["index"][2], product=lambda p: np.full(n, np.nan))
    assert x is None and k == 1
    quiet = dict(e["blocks"], g=np.zeros(n))
    x, k = up.pcg_solve(e["lin"], quiet, offsets, obs_cam, e["index"][2])
    assert k == 0 and not x.any()                                     # |r_0| = 0: no iteration
    x, k = up.pcg_solve(e["lin"], e["blocks"], offsets, obs_cam, e["index"][2], max_iterations=2)
    assert k == 2 and x is not None                                   # the cap is not a failure
    x, k = up.pcg_solve(e["lin"], e["blocks"], offsets, obs_cam, e["index"][2])
    dense = ub.solve_cameras(e["S"], e["g"], e["problem"][5])
    assert 0 < k < up.PCG_MAX_ITERATIONS and np.abs(x - dense).max() <= 1e-4 * np.abs(dense).max()


# ---- the kernels' routines on the host ---------------------------------------------------------------------------------------------------
def write_problem_file(path, problem, lam, p, index=None, loss=(0, 1.0)):
    """The input of tools/bundle_pcg_host.cpp; `index`: cam_offsets, cam_obs, obs_point where they are not ub.camera_index's."""
    cams, points, offsets, obs_cam, obs_xy, mask = problem
    cam_offsets, cam_obs, obs_point = index or ub.camera_index(obs_cam, offsets, len(cams))
    p = np.ascontiguousarray(p, np.float64).reshape(-1, 6 * len(cams))
    with open(path, "wb") as f:
        f.write(np.array([len(cams), len(points), len(obs_cam), len(p), loss[0]], np.int32).tobytes())
        f.write(np.array([lam, loss[1]], np.float64).tobytes())
        for a in (offsets, obs_cam, cam_offsets, cam_obs, obs_point, mask):
            f.write(np.ascontiguousarray(a).astype(np.int32).tobytes())
        for a in (cams, points, obs_xy, p):
            f.write(np.ascontiguousarray(a, np.float64).tobytes())


def read_result_file(path, n_cams, n_points, total, n_vectors):
    raw = open(path, "rb").read()
    at, out = 0, {}
    for name, dtype, shape in (("U", np.float64, (n_cams, 6, 6)), ("D", np.float64, (n_cams, 6, 6)), ("Minv", np.float64, (n_cams, 6, 6)),
                               ("g", np.float64, (6 * n_cams,)), ("s", np.float64, (n_vectors, n_points, 3)),
                               ("q", np.float64, (n_vectors, 6 * n_cams)), ("vinv", np.float64, (n_points, 6)), ("total_cost", np.float64, (1,)),
                               ("fixed", np.uint8, (6 * n_cams,)), ("obs_ok", np.uint8, (total,))):
        out[name] = np.frombuffer(raw, dtype, int(np.prod(shape)), at).reshape(shape)
        at += out[name].nbytes
    assert at == len(raw)
    return out


def run_host(program, tmp_path, problem, lam, p, index=None, loss=(0, 1.0)):
    write_problem_file(tmp_path / "pcg_problem.bin", problem, lam, p, index, loss)
    done = subprocess.run([program, str(tmp_path / "pcg_problem.bin"), str(tmp_path / "pcg_result.bin")], stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, text=True)
    assert done.returncode == 0, done.stderr
    n_vectors = int(np.asarray(p).size // max(6 * len(problem[0]), 1))
    return read_result_file(tmp_path / "pcg_result.bin", len(problem[0]), len(problem[1]), len(problem[3]), n_vectors), done.stderr


_BUILT = {}


def _build(tmp_path_factory, name, extra=()):
    """tools/bundle_pcg_host.cpp built with the line its source gives and `extra`, once per session and name."""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc to build the host program with")
    if name not in _BUILT:
        out = tmp_path_factory.mktemp(name) / name
        proc = subprocess.run(HOST_BUILD + list(extra) + ["-o", str(out), SOURCE], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert proc.returncode == 0, f"{name} does not build:\n{proc.stdout}"
        _BUILT[name] = str(out)
    return _BUILT[name]


@pytest.fixture(scope="session")
def bundle_pcg_host(tmp_path_factory):
    """The host program (the GPU tests share it)."""
    return _build(tmp_path_factory, "bundle_pcg_host")


def relative_differences(host, e, what):
    b = e["blocks"]
    assert np.array_equal(host["fixed"].astype(bool), b["fixed"]), what
    out = {}
    for k, spec in (("U", b["U"]), ("D", b["D"]), ("Minv", b["Minv"]), ("g", b["g"]), ("s", e["s"]), ("q", e["q"])):
        assert np.isfinite(host[k]).all() and np.isfinite(spec).all(), (what, k)
        scale = np.abs(spec).max(initial=0.0)
        diff = np.abs(host[k] - spec).max(initial=0.0)
        out[k] = diff / scale if scale else float(diff != 0) * np.inf
    return out


def test_host_build_matches_the_spec_on_the_windowed_the_random_and_the_edge_problems(bundle_pcg_host, tmp_path):
    worst = {}
    for e in spec_systems():
        host, _ = run_host(bundle_pcg_host, tmp_path, e["problem"], ub.BA_LAMBDA0, e["p"])
        for k, v in relative_differences(host, e, e["name"]).items():
            if v > worst.get(k, (-1.0, ""))[0]:
                worst[k] = (v, e["name"])
    print("worst relative differences host - spec: " + ", ".join(f"{k} {v:.3g} ({name})" for k, (v, name) in sorted(worst.items())))
    assert up.TOL_REL == 4 * up.HOST_SPEC_REL and up.TOL_MINV_REL == 4 * up.HOST_SPEC_MINV_REL
    assert max(v for k, (v, _) in worst.items() if k != "Minv") <= up.TOL_REL and worst["Minv"][0] <= up.TOL_MINV_REL


def test_host_build_matches_the_spec_where_lists_cross_the_batches(bundle_pcg_host, tmp_path):
    problem = up.lists_problem()
    cams, points, offsets, obs_cam, obs_xy, mask = problem
    assert tuple(np.bincount(obs_cam, minlength=len(up.LISTS))) == up.LISTS
    index = ub.camera_index(obs_cam, offsets, len(cams))
    lin = ub.linearize(cams, points, offsets, obs_cam, obs_xy, mask, ub.BA_LAMBDA0)
    blocks = up.camera_blocks(lin, len(cams), offsets, obs_cam, mask, *index, ub.BA_LAMBDA0)
    p = vectors_of(999, blocks["fixed"])
    products = [up.schur_product(lin, blocks, offsets, obs_cam, index[2], v) for v in p]
    e = dict(blocks=blocks, s=np.stack([s for s, _ in products]), q=np.stack([q for _, q in products]))
    host, _ = run_host(bundle_pcg_host, tmp_path, problem, ub.BA_LAMBDA0, p)
    worst = relative_differences(host, e, "lists")
    print("relative differences host - spec: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(worst.items())))
    assert lin["ok"].all() and blocks["fixed"][-6:].all() and not blocks["fixed"][:-6].any()
    assert max(v for k, v in worst.items() if k != "Minv") <= 4 * up.HOST_SPEC_LISTS_REL and worst["Minv"] <= 4 * up.HOST_SPEC_LISTS_MINV_REL


def malformed_inputs():
    """-> [(name, problem, index)]: offsets that descend, are negative or pass the arrays, in the points' and in the cameras'
    index; a NaN camera row; a camera without observations; a camera twice in a track."""
    cams, points, offsets, obs_cam, obs_xy, mask = ub.random_problem(7)
    total = len(obs_cam)
    out = []
    bad = offsets.copy()
    bad[3], bad[5], bad[-1] = bad[4] + 1, -2, total + 5
    out.append(("point offsets", (cams, points, bad, obs_cam, obs_xy, mask), None))
    for name, change in (("camera list descends", lambda x: x[0].__setitem__(2, x[0][3] + 1)),
                         ("camera list below zero", lambda x: x[0].__setitem__(0, -3)),
                         ("camera list past the arrays", lambda x: x[0].__setitem__(len(cams), total + 7)),
                         ("entry names no observation", lambda x: x[1].__setitem__(int(x[0][1]), total + 100)),
                         ("entry below zero", lambda x: x[1].__setitem__(int(x[0][1]) + 1, -5)),
                         ("entry of another camera", lambda x: x[1].__setitem__(int(x[0][2]), int(x[1][int(x[0][3])]))),
                         ("point of an observation past the table", lambda x: x[2].__setitem__(4, len(points) + 3)),
                         ("point of an observation below zero", lambda x: x[2].__setitem__(5, -1))):
        index = [a.copy() for a in ub.camera_index(obs_cam, offsets, len(cams))]
        change(index)
        out.append((name, (cams, points, offsets, obs_cam, obs_xy, mask), index))
    edge = ub.edge_problems()
    out += [(name, tuple(edge[name]), None) for name in ("nan_camera", "empty_camera", "camera_twice", "slot_first", "slot_last")]
    return out


def test_host_build_under_the_sanitizers_reports_nothing(tmp_path, tmp_path_factory):
    """The same program with the host half built -fsanitize=address,undefined, run on its own."""
    program = _build(tmp_path_factory, "bundle_pcg_host_san", SANITIZE)
    for e in spec_systems():
        host, stderr = run_host(program, tmp_path, e["problem"], ub.BA_LAMBDA0, e["p"])
        assert stderr == "" and np.array_equal(host["fixed"].astype(bool), e["blocks"]["fixed"]), e["name"]
    for name, problem, index in malformed_inputs():
        n = len(problem[0])
        p = np.random.RandomState(3).normal(0, 1, (2, 6 * n))
        host, stderr = run_host(program, tmp_path, problem, ub.BA_LAMBDA0, p, index)
        assert stderr == "" and all(np.isfinite(host[k]).all() for k in ("U", "D", "Minv", "g", "s", "q")), name
    # what a skipped camera and a skipped point leave: the blocks of a camera without observations, s = 0
    name, problem, index = malformed_inputs()[1]
    host, _ = run_host(program, tmp_path, problem, ub.BA_LAMBDA0, np.ones((1, 6 * len(problem[0]))), index)
    assert np.array_equal(host["D"][2], np.eye(6)) and np.array_equal(host["Minv"][2], np.eye(6)) and host["fixed"][12:18].all()
    name, problem, index = malformed_inputs()[0]
    host, _ = run_host(program, tmp_path, problem, ub.BA_LAMBDA0, np.ones((1, 6 * len(problem[0]))), index)
    assert not host["s"][0][[3, 4, 5, len(problem[1]) - 1]].any() and host["s"][0].any()


def test_host_program_refuses_a_bad_loss_and_a_bad_lambda(bundle_pcg_host, tmp_path):
    problem = ub.random_problem(7)
    for lam, loss in ((-1.0, (0, 1.0)), (float("nan"), (0, 1.0)), (1e-4, (7, 1.0)), (1e-4, (1, 0.0))):
        write_problem_file(tmp_path / "bad.bin", problem, lam, np.zeros((0, 6 * len(problem[0]))), loss=loss)
        done = subprocess.run([bundle_pcg_host, str(tmp_path / "bad.bin"), str(tmp_path / "none.bin")], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert done.returncode == 3 and not (tmp_path / "none.bin").exists()


# ---- the loop ----------------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def windowed_pcg():
    """The specification's pcg loop on the windowed problem -> cams, points, report."""
    _, _, _, problem, adj = adjusted()
    return up.bundle_adjust(*problem[1:], adj["held"][2])


def test_pcg_loop_follows_the_dense_loop_on_the_windowed_problem():
    scene, _, grown, problem, adj = adjusted()
    cams, points, report = windowed_pcg()
    dense = adj["report"]
    rel = abs(report["final_cost"] - dense["final_cost"]) / dense["final_cost"]
    print(f"decisions {report['decisions']} (dense {dense['decisions']}), final cost {report['final_cost']:.12g} (dense {dense['final_cost']:.12g}, "
          f"relative difference {rel:.3g}), pcg iterations {report['pcg_iterations']}")
    assert report["decisions"] == dense["decisions"] and report["iterations"] == dense["iterations"]
    assert report["final_lambda"] == dense["final_lambda"] and report["initial_cost"] == dense["initial_cost"]
    assert report["solver"] == "pcg" and len(report["pcg_iterations"]) == len(report["decisions"])
    assert all(0 < k <= up.PCG_MAX_ITERATIONS for k in report["pcg_iterations"])
    assert report["pcg_iterations"] == up.WINDOWED_PCG_ITERATIONS          # what DESIGN.md records
    assert rel <= 4 * up.LOOP_DENSE_REL
    ids = problem[0]
    a, b = (ids.index(i) for i in grown["initial_pair"])
    scaled, _ = ub.rescale(cams, points, a, b)
    rot, pos = ua.align_errors({i: (scaled[s, :9].reshape(3, 3), scaled[s, 9:12]) for s, i in enumerate(ids)}, scene, *grown["initial_pair"])
    print(f"rotation {rot:.4f} deg, centre {pos:.5f} baselines")
    assert rot <= BA_ROT_BOUND and pos <= BA_POS_BOUND
    before, _, mask = adj["held"]
    assert np.array_equal(cams[a], before[a]) and np.array_equal(cams[:, 12:], before[:, 12:])


def test_pcg_loop_lowers_the_cost_of_an_arc_the_dense_route_refuses():
    problem = up.arc_problem()
    cams, points, offsets, obs_cam, obs_xy, mask = problem
    assert len(cams) == up.ARC_CAMS == 520 and np.bincount(obs_cam, minlength=len(cams)).min() >= 3
    lengths = np.diff(offsets)
    assert lengths.min() >= 3 and lengths.max() <= 8 and len(points) == up.ARC_POINTS
    _, _, report = up.arc_spec()
    print(f"cost {report['initial_cost']:.6g} -> {report['final_cost']:.6g} in {report['iterations']} linearisations, decisions "
          f"{report['decisions']}, pcg iterations {report['pcg_iterations']}")
    assert report["final_cost"] < 0.5 * report["initial_cost"] and report["accepted_steps"] >= 1
    # the loop's own rule ended it: the cap on the linearisations, a decrease below BA_REL_DECREASE or a lambda past its range
    assert report["iterations"] <= up.ARC_MAX_ITERATIONS and len(report["pcg_iterations"]) == len(report["decisions"])


# ---- the product's host logic with the specification in its seams -----------------------------------------------------------------------
def spec_bundle_recording(calls):
    def fn(cams, points, offsets, obs_cam, obs_xy, const_mask, device, **kw):
        calls.append(dict(kw, n_cams=len(cams)))
        adjust = up.bundle_adjust if kw.get("solver") == "pcg" else ub.bundle_adjust
        return adjust(cams, points, offsets, obs_cam, obs_xy, const_mask)
    return fn


def test_front_end_refusals_and_what_the_seam_is_handed(tmp_path):
    from vit_colmap_amd import _lib
    from vit_colmap_amd.mapping import bundle

    cams, points, offsets, obs_cam, obs_xy, mask = ub.random_problem(7)
    many = np.repeat(cams[:1], _lib.VC_BA_MAX_CAMS + 1, axis=0)
    with pytest.raises(ValueError, match="VC_BA_MAX_CAMS"):          # the dense solver above the cap, named or by default
        bundle.bundle_adjust(many, points, offsets, obs_cam, obs_xy, np.zeros(len(many), np.uint8), "cpu", solver="dense")
    with pytest.raises(ValueError, match="VC_BA_MAX_CAMS"):
        bundle.bundle_adjust(many, points, offsets, obs_cam, obs_xy, np.zeros(len(many), np.uint8), "cpu")
    with pytest.raises(ValueError, match="unknown solver 'qr'.*dense, pcg"):
        bundle.bundle_adjust(cams, points, offsets, obs_cam, obs_xy, mask, "cpu", solver="qr")
    for border in (dict(cam_group=np.zeros(len(cams), np.int32), intr_mask=np.array([12], np.uint8)), dict(cam_dist=np.zeros((len(cams), 2)))):
        with pytest.raises(ValueError, match="border.*dense solver"):
            bundle.bundle_adjust(cams, points, offsets, obs_cam, obs_xy, mask, "cpu", solver="pcg", **border)
    # no camera cap and no S under pcg: the empty problem returns before a library is loaded
    out = bundle.bundle_adjust(many, np.zeros((0, 3)), np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros((0, 2)),
                               np.zeros(len(many), np.uint8), "cpu", solver="pcg")
    assert out[2]["solver"] == "pcg" and out[2]["pcg_iterations"] == [] and len(out[0]) == len(many)
    dense = bundle.bundle_adjust(cams, np.zeros((0, 3)), np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros((0, 2)), mask, "cpu")
    assert sorted(dense[2]) == ["accepted_steps", "decisions", "final_cost", "final_lambda", "initial_cost", "iterations", "loss", "loss_scale"]
    assert (bundle.PCG_REL_TOL, bundle.PCG_MAX_ITERATIONS, bundle.SOLVERS) == (up.PCG_REL_TOL, up.PCG_MAX_ITERATIONS, ("dense", "pcg"))

    scene = adjusted()[0]
    write_scene_db(tmp_path / "w.db", scene, windowed()[1])
    seams = dict(device="cpu", two_view_pose_fn=spec_two_view_pose, estimate_fn=spec_estimate, triangulate_fn=spec_triangulate)
    calls = []
    model = bundle.build_adjusted_model(tmp_path / "w.db", bundle_fn=spec_bundle_recording(calls), solver="pcg", **seams)
    plain = bundle.build_adjusted_model(tmp_path / "w.db", bundle_fn=spec_bundle_recording(calls), **seams)
    assert calls == [dict(solver="pcg", n_cams=12), dict(n_cams=12)]          # the dense call hands over nothing new
    ba = model.stats()["bundle_adjustment"]
    assert ba["solver"] == "pcg" and ba["pcg_iterations"] == windowed_pcg()[2]["pcg_iterations"]
    assert "solver" not in plain.stats()["bundle_adjustment"] and "pcg_iterations" not in plain.stats()["bundle_adjustment"]
    assert sorted(model.images) == sorted(plain.images) and abs(ba["final_cost"] / plain.stats()["bundle_adjustment"]["final_cost"] - 1) <= 1e-6
    for flag in ("refine_focal_length", "refine_distortion", "known_distortion"):
        with pytest.raises(ValueError, match="dense solver"):
            bundle.build_adjusted_model(tmp_path / "w.db", bundle_fn=spec_bundle_recording(calls), solver="pcg", **seams, **{flag: True})
    with pytest.raises(ValueError, match="unknown solver"):
        bundle.build_adjusted_model(tmp_path / "w.db", bundle_fn=spec_bundle_recording(calls), solver="lu", **seams)
    assert len(calls) == 2


def test_round_steps_has_no_camera_cap_under_pcg():
    from types import SimpleNamespace

    from vit_colmap_amd import _lib
    from vit_colmap_amd.mapping import rounds

    n = _lib.VC_BA_MAX_CAMS + 1

    def state():
        poses = {i: (np.eye(3), np.array([0.1 * i, 0.0, 0.0]), np.array([1.0, 0.0, 0.0, 0.0])) for i in range(1, n + 1)}
        K = {i: np.array([[600.0, 0, 320.0], [0, 600.0, 240.0], [0, 0, 1.0]]) for i in poses}
        kps = {i: np.array([[320.0, 240.0]]) for i in poses}
        return SimpleNamespace(poses=poses, xyz={1: np.array([0.0, 0.0, 5.0])}, tracks={1: [(1, 0), (2, 0)]}, K=K, kps=kps, device="cpu",
                               initial_pair=(1, 2), ids=sorted(poses), slot={i: i - 1 for i in poses}, point_of={}, comps={})

    calls = []

    def bundle_fn(cams, points, offsets, obs_cam, obs_xy, mask, device, **kw):
        calls.append(dict(kw, n_cams=len(cams)))
        return cams, points, dict(iterations=1, accepted_steps=0, initial_cost=0.0, final_cost=0.0, decisions=[])

    def refine_fn(obs, slots, offsets, table, points, device):
        return points, np.ones(len(obs), bool), np.array([2]), np.zeros(1)

    with pytest.raises(ValueError, match="VC_BA_MAX_CAMS"):
        rounds._round_steps(state(), bundle_fn, refine_fn, {}, [])
    assert calls == []
    reports = []
    rounds._round_steps(state(), bundle_fn, refine_fn, dict(solver="pcg"), reports)
    assert calls == [dict(solver="pcg", n_cams=n)] and len(reports) == 1


def test_mapped_rounds_hand_the_solver_to_every_adjustment(tmp_path):
    from vit_colmap_amd.mapping import rounds

    scene = adjusted()[0]
    write_scene_db(tmp_path / "w.db", scene, windowed()[1])
    seams = dict(device="cpu", two_view_pose_fn=spec_two_view_pose, estimate_fn=spec_estimate, triangulate_fn=spec_triangulate)

    def refine_fn(obs_xy, obs_cam, offsets, cams, init_xyz, device):
        return ur.refine_tracks(obs_xy, obs_cam, offsets, cams, init_xyz)

    for solver, want in (("pcg", dict(solver="pcg")), ("dense", {})):
        calls = []

        def bundle_fn(cams, points, offsets, obs_cam, obs_xy, mask, device, **kw):
            calls.append(kw)
            return ub.bundle_adjust(cams, points, offsets, obs_cam, obs_xy, mask, max_iterations=2)

        rounds.build_mapped_model(tmp_path / "w.db", bundle_fn=bundle_fn, refine_fn=refine_fn, solver=solver, **seams)
        assert len(calls) >= 2 and all(kw == want for kw in calls), solver
    with pytest.raises(ValueError, match="unknown solver"):
        rounds.build_mapped_model(tmp_path / "w.db", solver="lu", **seams)


# ---- configuration and command line -------------------------------------------------------------------------------------------------------
def test_ba_solver_is_dense_by_default_and_its_combinations_are_checked_before_the_extractor(tmp_path, monkeypatch):
    import argparse

    from vit_colmap_amd.pipeline import run_pipeline as rp
    from vit_colmap_amd.utils.config import Config, ReconstructionConfig

    assert ReconstructionConfig().ba_solver == "dense" and Config().reconstruction.ba_solver == "dense"
    assert Config.from_args(argparse.Namespace(ba_solver="pcg")).reconstruction.ba_solver == "pcg"
    assert Config.from_args(argparse.Namespace()).reconstruction.ba_solver == "dense"

    def no_extractor(self):
        raise AssertionError("the extractor was built before the flags were checked")

    monkeypatch.setattr(rp.Pipeline, "_make_extractor", no_extractor)

    def config(**flags):
        cfg = Config()
        cfg.camera.prior_focal_length, cfg.matching.compute_relative_pose, cfg.do_reconstruction = True, True, False
        cfg.reconstruction.sparse_model = cfg.reconstruction.bundle_adjustment = True
        cfg.reconstruction.ba_solver = "pcg"
        for k, v in flags.items():
            setattr(cfg.camera if k == "known_distortion" else cfg.reconstruction, k, v)
        return cfg

    def run(cfg):
        rp.Pipeline(cfg).run(tmp_path / "images", tmp_path / "out", tmp_path / "x.db")

    with pytest.raises(ValueError, match="ba_solver needs .*bundle_adjustment"):
        run(config(bundle_adjustment=False, sparse_model=False))
    for flag in ("refine_focal_length", "refine_distortion", "known_distortion"):
        with pytest.raises(ValueError, match="dense solver.*out of scope"):
            run(config(**{flag: True}))
    with pytest.raises(ValueError, match="unknown ba_solver 'lu'"):
        run(config(ba_solver="lu"))
    with pytest.raises(AssertionError, match="extractor was built"):   # a valid combination goes on to the extractor
        run(config())
    assert not (tmp_path / "out" / "sparse").exists()
    seen = []
    monkeypatch.setattr(rp.Pipeline, "run", lambda self, *a, **k: seen.append(self.config.reconstruction.ba_solver))
    for extra in ([], ["--ba-solver", "pcg"], ["--ba-solver", "dense"]):
        monkeypatch.setattr(sys, "argv", ["prog", "--images", "i", "--output", "o", "--db", "d", "--sparse-model", "--bundle-adjustment"] + extra)
        rp.main()
    assert seen == ["dense", "pcg", "dense"]
    monkeypatch.setattr(sys, "argv", ["prog", "--images", "i", "--output", "o", "--db", "d", "--ba-solver", "lu"])
    with pytest.raises(SystemExit):
        rp.main()


def test_pipeline_step_hands_the_solver_on_only_where_it_is_not_dense(tmp_path, monkeypatch):
    import vit_colmap_amd.mapping.bundle as bundle
    import vit_colmap_amd.mapping.grow as grow
    from vit_colmap_amd.mapping.seed import SparseModel
    from vit_colmap_amd.pipeline import run_pipeline as rp
    from vit_colmap_amd.utils.config import Config

    scene = adjusted()[0]
    write_scene_db(tmp_path / "w.db", scene, windowed()[1])
    real = grow.build_sparse_model
    monkeypatch.setattr(grow, "build_sparse_model", lambda path, device="cuda": real(path, device="cpu", two_view_pose_fn=spec_two_view_pose,
                                                                                     estimate_fn=spec_estimate, triangulate_fn=spec_triangulate))
    calls = []
    monkeypatch.setattr(bundle, "bundle_adjust", spec_bundle_recording(calls))
    stats = {}
    for name, kw in (("dense", {}), ("pcg", dict(solver="pcg"))):
        step = rp.Pipeline(Config())
        step.last_stats = {}
        step._write_sparse_model(tmp_path / "w.db", tmp_path / name, "cpu", adjust=True, **kw)
        stats[name] = step.last_stats["bundle_adjustment"]
    assert calls == [dict(n_cams=12), dict(solver="pcg", n_cams=12)]
    assert "solver" not in stats["dense"]["bundle_adjustment"] and stats["pcg"]["bundle_adjustment"]["solver"] == "pcg"
    assert stats["pcg"]["registered_images"] == 12
    # sparse/grown does not know the solver; sparse/adjusted has the same images and points within the solve's tolerance
    for f in ("cameras.txt", "images.txt", "points3D.txt"):
        assert (tmp_path / "pcg" / "sparse" / "grown" / f).read_bytes() == (tmp_path / "dense" / "sparse" / "grown" / f).read_bytes()
    a, b = (SparseModel.read_text(tmp_path / n / "sparse" / "adjusted") for n in ("dense", "pcg"))
    assert sorted(a.images) == sorted(b.images) and sorted(a.points3D) == sorted(b.points3D)
    assert max(np.abs(a.images[i]["tvec"] - b.images[i]["tvec"]).max() for i in a.images) <= 1e-5
