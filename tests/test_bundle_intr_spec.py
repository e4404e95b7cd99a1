"""CPU tests of bundle adjustment with refined intrinsics ("The border"): the numpy specification of
tests/util_bundle_intr.py (the derivative, the border against the dense normal equations, the all-held case against
tests/util_bundle.py bit for bit, recovery of a wrong focal length on the exact scene and on the grown model, the rejection of a
focal length that is not positive), the kernels' routines compiled for the host (tools/bundle_host.cpp) against it, plain
and under the host sanitizers, the product's host logic with the specification in its seams, and the pipeline's flag.  No GPU."""
import copy
import subprocess
import sys
from functools import lru_cache

import numpy as np
import pytest

import util_absolute_pose as ua
import util_bundle as ub
import util_bundle_intr as ui
from test_absolute_pose_spec import spec_estimate, spec_two_view_pose, write_scene_db
from test_bundle_spec import (BA_POS_BOUND, BA_ROT_BOUND, ROOT, SANITIZE, _build, adjusted, bundle_host, exact_problem, run_host,  # noqa: F401
                              spec_bundle, spec_pass)
from test_mapper_spec import spec_triangulate, windowed

# central differences of the specification's own residual in fx, fy, cx, cy and in the tied parameter with step 1e-3 px (the
# residual is linear in all of them, so the step only has to be large against the rounding of a residual, 640 * 2^-52 ~ 1e-13 px)
# against J_theta on 20 observations, measured: worst |difference| 3.4e-11 where the largest entry of J_theta is 1; the bound is
# 4x, rounded up
FD_STEP, FD_BOUND = 1e-3, 1.4e-10
# the bordered step (dc, dtheta, dX) against the solution of the dense damped normal equations over (c, theta, X), relative to
# the largest entry of the dense step, measured worst over the four problems of the test 5.8e-12 (the windowed problem: some 3400
# unknowns eliminated in another order); the bound is 4x, rounded up
DENSE_REL_BOUND = 2.4e-11
# the refined focal of the exact scene against the truth, relative, measured worst 1.9e-16, one unit in the last place (one tied group from
# 1.03 f and from 0.9 f, two groups from +3 % and -3 %); the bound is 4x, rounded up
EXACT_FOCAL_REL = 8e-16
# the refined focal of the grown model from 1.03 f against the one from f, relative, measured 6.2e-10; the bound is 4x, rounded up
GROWN_FOCAL_AGREE = 2.5e-9


def tied_groups(n_cams, n_groups=1, slots=None):
    """Every slot in group slot % n_groups (or `slots`), each group tied with the principal point held: the front end's mask."""
    cam_group = (np.arange(n_cams) % n_groups if slots is None else np.asarray(slots)).astype(np.int32)
    return cam_group, np.full(n_groups, ui.TIED | ui.HOLD_PRINCIPAL, np.uint8)


@lru_cache(maxsize=None)
def windowed_problem():
    _, _, _, problem, adj = adjusted()
    return (*problem[1:], adj["held"][2])


def with_focal(problem, factor):
    cams = problem[0].copy()
    cams[:, 12:14] = cams[:, 12:14] * np.asarray(factor, np.float64).reshape(-1, 1)
    return (cams,) + tuple(problem[1:])


def one_pass(problem, groups, lam=ub.BA_LAMBDA0):
    """One linearisation, both reductions, the bordered solve and the step of the specification."""
    cams, points, offsets, obs_cam, obs_xy, mask = problem
    cam_group, intr_mask = groups
    G, index = len(intr_mask), ub.camera_index(obs_cam, offsets, len(cams))
    lin = ub.linearize(cams, points, offsets, obs_cam, obs_xy, mask, lam)
    S, g = ub.reduce_cameras(lin, len(cams), offsets, obs_cam, mask, *index, lam)
    li = ui.linearize_intrinsics(lin, cams, points, offsets, obs_cam, cam_group, G, intr_mask)
    B, C, h, free = ui.reduce_border(lin, li, len(cams), cam_group, G, intr_mask, offsets, obs_cam, *index, lam)
    dc, dtheta = ui.solve_bordered(S, g, B, C, h, mask, free)
    if dc is None:
        dc, dtheta = np.zeros(6 * len(cams)), np.zeros(4 * G)
    out_cams, out_points, dX, valid = ui.step_intrinsics(lin, li, cams, points, offsets, obs_cam, cam_group, G, intr_mask, dc, dtheta)
    return dict(lin=lin, li=li, S=S, g=g, B=B, C=C, h=h, free=free, dc=dc, dtheta=dtheta, cams=out_cams, points=out_points, dx=dX, valid=valid)


# ---- the specification ---------------------------------------------------------------------------------------------------------------
def test_jtheta_matches_central_differences_of_the_residual():
    worst = 0.0
    for i in range(20):
        cams, points, offsets, obs_cam, obs_xy, _ = ub.random_problem(i)
        o = (7 * i) % len(obs_cam)
        j = int(np.searchsorted(offsets, o, side="right") - 1)
        row, X, uv = cams[obs_cam[o]], points[j], obs_xy[o]
        x, y = ui.normalised(row, X)
        for mask, columns in ((0, range(4)), (ui.TIED, (0, 2, 3))):
            J = ui.jtheta(x, y, mask)
            for k in columns:
                e = np.zeros(4)
                e[k] = FD_STEP
                num = (ui.residual_theta(row, X, uv, e, mask) - ui.residual_theta(row, X, uv, -e, mask)) / (2 * FD_STEP)
                worst = max(worst, np.abs(num - J[:, k]).max())
                assert np.abs(num - J[:, k]).max() <= FD_BOUND, (i, mask, k)
        assert not ui.jtheta(x, y, ui.TIED)[:, 1].any()                          # parameter 1 of a tied group counts as held
        held = ui.jtheta(x, y, ui.HOLD_FX | ui.HOLD_CY)                            # a held column is zero, the others are what they were
        assert not held[:, [0, 3]].any() and np.array_equal(held[:, [1, 2]], ui.jtheta(x, y, 0)[:, [1, 2]])
        assert not ui.jtheta(x, y, ui.TIED | ui.HOLD_FX)[:, :2].any()
    print(f"worst difference to central differences {worst:.3g}")


def dense_step(problem, groups, lam):
    """The damped normal equations over (c, theta, X) from the stacked Jacobian, solved by numpy; a column that nothing moves
    has the diagonal 1 -> dc, dtheta, dX."""
    cams, points, offsets, obs_cam, obs_xy, mask = problem
    cam_group, intr_mask = groups
    n_cams, G, n = len(cams), len(intr_mask), len(points)
    lin = ub.linearize(cams, points, offsets, obs_cam, obs_xy, mask, lam)
    assert lin["ok"].all() and not lin["constant"].any()
    J, r = np.zeros((2 * len(obs_cam), 6 * n_cams + 4 * G + 3 * n)), lin["r"].reshape(-1)
    for j in range(n):
        for o in range(offsets[j], offsets[j + 1]):
            a = int(obs_cam[o])
            J[2 * o:2 * o + 2, 6 * a:6 * a + 6] = lin["Jc"][o]
            g = ui.group_of(cam_group, a, G)
            if g >= 0:
                J[2 * o:2 * o + 2, 6 * n_cams + 4 * g:6 * n_cams + 4 * g + 4] = ui.jtheta(*ui.normalised(cams[a], points[j]), intr_mask[g])
            J[2 * o:2 * o + 2, 6 * n_cams + 4 * G + 3 * j:6 * n_cams + 4 * G + 3 * j + 3] = lin["Jp"][o]
    N = J.T @ J
    d = np.diag(N).copy()
    N[np.diag_indices(len(N))] = np.where(d == 0, 1.0, d + lam * d)
    x = np.linalg.solve(N, -(J.T @ r))
    return x[:6 * n_cams], x[6 * n_cams:6 * n_cams + 4 * G], x[6 * n_cams + 4 * G:].reshape(-1, 3)


def test_bordered_step_equals_the_dense_normal_equations():
    p3, pw = ub.random_problem(3), windowed_problem()
    cases = [("random 3, one tied group", p3, tied_groups(len(p3[0]))),
             ("windowed, one tied group", with_focal(pw, 1.03), tied_groups(len(pw[0]))),
             ("random 3, two groups, all four free", p3, ((np.arange(len(p3[0])) % 2).astype(np.int32), np.zeros(2, np.uint8))),
             ("random 3, fy and cx held, a slot outside", p3, (np.r_[np.zeros(len(p3[0]) - 1), [5]].astype(np.int32),
                                                              np.array([ui.HOLD_FY | ui.HOLD_CX], np.uint8)))]
    worst = 0.0
    for name, problem, groups in cases:
        got = one_pass(problem, groups)
        dc, dtheta, dX = dense_step(problem, groups, ub.BA_LAMBDA0)
        scale = max(np.abs(dc).max(), np.abs(dtheta).max(), np.abs(dX).max())
        rel = max(np.abs(got["dc"] - dc).max(), np.abs(got["dtheta"] - dtheta).max(), np.abs(got["dx"] - dX).max()) / scale
        print(f"{name}: relative difference to the dense step {rel:.3g} (|dtheta| {np.abs(dtheta).max():.3g})")
        worst = max(worst, rel)
        assert got["dtheta"].any() and rel <= DENSE_REL_BOUND, name
        assert np.array_equal(got["dtheta"] == 0, ~got["free"]), name          # what does not move steps by exactly 0
    print(f"worst {worst:.3g}")


def test_with_every_intrinsic_held_the_border_vanishes_and_the_step_is_util_bundles():
    for problem in (ub.random_problem(5), windowed_problem()):
        n_cams = len(problem[0])
        for groups in ((np.zeros(n_cams, np.int32), np.array([ui.HOLD_ALL], np.uint8)),
                       (np.zeros(n_cams, np.int32), np.array([ui.TIED | ui.HOLD_FX | ui.HOLD_PRINCIPAL], np.uint8)),
                       (np.full(n_cams, -1, np.int32), np.zeros(1, np.uint8))):        # no slot in the group: its intrinsics are held
            got, plain = one_pass(problem, groups), spec_pass(problem)
            assert not got["B"].any() and np.array_equal(got["C"], np.eye(4)) and not got["h"].any() and not got["free"].any()
            assert not got["dtheta"].any() and got["valid"].all()
            assert np.array_equal(got["dc"], plain["dc"]) and np.array_equal(got["dx"], plain["dx"])
            assert np.array_equal(got["cams"], plain["cams"]) and np.array_equal(got["points"], plain["points"])
    # the loop takes util_bundle's decisions and ends at its bits
    problem = ub.random_problem(5)
    cams, points, report = ui.bundle_adjust(*problem, np.zeros(len(problem[0]), np.int32), np.array([ui.HOLD_ALL], np.uint8))
    want_cams, want_points, want = ub.bundle_adjust(*problem)
    assert report["decisions"] == want["decisions"] and len(want["decisions"]) >= 2 and report["iterations"] == want["iterations"]
    assert report["final_cost"] == want["final_cost"] and np.array_equal(cams, want_cams) and np.array_equal(points, want_points)
    assert np.array_equal(report["intrinsics"]["before"], report["intrinsics"]["after"])


@lru_cache(maxsize=None)
def exact_runs():
    """The exact scene from a wrong focal: one tied group at 1.03 f and at 0.9 f; two groups, even and odd slots at +3 % and -3 %
    and a third group whose only slot sees nothing -> {name: (start cams, cams, points, report)}."""
    problem = exact_problem()
    n_cams = len(problem[0])
    out = {}
    for name, factor in (("1.03", 1.03), ("0.9", 0.9)):
        start = with_focal(problem, factor)
        out[name] = (start[0],) + ui.bundle_adjust(*start, *tied_groups(n_cams))
    start = with_focal(problem, np.where(np.arange(n_cams) % 2 == 0, 1.03, 0.97))
    # a thirteenth camera that no observation names, alone in group 2
    cams = np.concatenate([start[0], with_focal(problem, 1.1)[0][:1]])
    mask = np.concatenate([problem[5], [0]]).astype(np.uint8)
    cam_group, intr_mask = tied_groups(n_cams + 1, 3, np.r_[np.arange(n_cams) % 2, [2]])
    out["two groups"] = (cams,) + ui.bundle_adjust(cams, *start[1:5], mask, cam_group, intr_mask)
    return out


def test_exact_scene_recovers_the_focal_length():
    truth = exact_problem()[0]
    f, worst = truth[0, 12], 0.0
    for name, (start, cams, points, report) in exact_runs().items():
        n = len(truth)
        rel = np.abs(cams[:n, 12:14] - f).max() / f
        worst = max(worst, rel)
        print(f"{name}: cost {report['initial_cost']:.3g} -> {report['final_cost']:.3g} in {report['accepted_steps']} accepted steps, "
              f"focal relative error {rel:.3g}")
        assert report["final_cost"] < 1e-18 and rel <= EXACT_FOCAL_REL, name
        assert np.array_equal(cams[:, 12], cams[:, 13]) and np.array_equal(cams[:, 14:], start[:, 14:])       # tied; the principal point is held
        assert np.array_equal(report["intrinsics"]["before"][0], start[0, 12:16]) and np.array_equal(report["intrinsics"]["after"][0], cams[0, 12:16])
    start, cams, _, report = exact_runs()["two groups"]
    assert start[0, 12] > f > start[1, 12] and np.array_equal(cams[-1], start[-1])          # the group that sees nothing keeps every bit
    assert np.array_equal(report["intrinsics"]["after"][2], start[-1, 12:16])
    print(f"worst focal relative error {worst:.3g}")


@lru_cache(maxsize=None)
def grown_runs():
    """The windowed scene's grown model: every focal at 1.03 f and held; refined from 1.03 f; refined from f."""
    problem = windowed_problem()
    wrong = with_focal(problem, 1.03)
    groups = tied_groups(len(problem[0]))
    return dict(held=ub.bundle_adjust(*wrong), refined=ui.bundle_adjust(*wrong, *groups), refined_from_truth=ui.bundle_adjust(*problem, *groups))


def test_grown_model_refines_a_wrong_focal_length_and_removes_its_drift():
    """The test that fails without the feature: with the focal 3 % off and held, no number of rounds brings the cost down to
    what the true focal reaches; with one more unknown it does."""
    scene, _, grown, problem, adj = adjusted()
    ids, f = problem[0], problem[1][0, 12]
    a, b = grown["initial_pair"]
    sa, sb = ids.index(a), ids.index(b)
    runs = grown_runs()
    truth_held = adj["report"]["final_cost"]
    drift = {}
    for name, (cams, points, report) in runs.items():
        scaled, _ = ub.rescale(cams, points, sa, sb)
        drift[name] = ua.align_errors({i: (scaled[s, :9].reshape(3, 3), scaled[s, 9:12]) for s, i in enumerate(ids)}, scene, a, b)
        print(f"{name}: cost {report['initial_cost']:.4f} -> {report['final_cost']:.6f} in {report['iterations']} linearisations, focal "
              f"{cams[0, 12]:.6f}, rotation {drift[name][0]:.4f} deg, centre {drift[name][1]:.5f} baselines")
    f1, f0 = runs["refined"][0][0, 12], runs["refined_from_truth"][0][0, 12]
    print(f"true focal held: cost {truth_held:.6f}; the two refined focals agree to {abs(f1 - f0) / f0:.3g} relative, {abs(f1 - f) / f:.3%} off the truth")
    assert abs(f1 - f0) / f0 <= GROWN_FOCAL_AGREE
    assert runs["refined"][2]["final_cost"] < truth_held < runs["held"][2]["final_cost"]
    assert runs["refined_from_truth"][2]["final_cost"] < truth_held
    assert abs(f1 - f) / f <= 0.005
    assert drift["refined"][0] <= BA_ROT_BOUND and drift["refined"][1] <= BA_POS_BOUND
    for cams, _, _ in (runs["refined"], runs["refined_from_truth"]):
        assert (cams[:, 12] == cams[0, 12]).all() and np.array_equal(cams[:, 12], cams[:, 13]) and np.array_equal(cams[:, 14:], problem[1][:, 14:])


def test_a_step_to_a_focal_that_is_not_positive_is_rejected_and_lambda_grows():
    """Pixels mirrored through the principal point are fitted by a negative focal: with the poses held the first steps lead
    there.  Their cost is lower, so nothing but the rule rejects them."""
    cams, points, offsets, obs_cam, obs_xy, _ = exact_problem()
    obs_xy = 2 * cams[obs_cam, 14:16] - obs_xy
    cams = with_focal((cams,), 0.5)[0]
    mask = np.full(len(cams), ub.HELD_ALL, np.uint8)
    problem, groups = (cams, points, offsets, obs_cam, obs_xy, mask), tied_groups(len(cams))
    first = one_pass(problem, groups)
    lower = ub.linearize(first["cams"], first["points"], offsets, obs_cam, obs_xy, mask, ub.BA_LAMBDA0 / 10)
    assert not first["valid"].any() and first["cams"][0, 12] < 0 and lower["total_cost"] < first["lin"]["total_cost"]
    out, _, report = ui.bundle_adjust(*problem, *groups, max_iterations=12)
    print(f"decisions {report['decisions']}, lambda {report['final_lambda']:.3g}, focal {cams[0, 12]:.3g} -> {out[0, 12]:.3g}")
    assert report["decisions"][0] is False and report["final_lambda"] > ub.BA_LAMBDA0 and (out[:, 12:14] > 0).all()
    rejected = report["decisions"].index(True) if True in report["decisions"] else len(report["decisions"])
    assert rejected >= 2                                                       # lambda grew tenfold per rejection until the step was short enough


# ---- the kernels' routines on the host ---------------------------------------------------------------------------------------------------
def spec_layout(problem, groups, lam=ub.BA_LAMBDA0):
    """`one_pass` in the host program's layout."""
    s = one_pass(problem, groups, lam)
    li, G, n = s["li"], len(groups[1]), len(problem[1])
    terms = np.concatenate([li["q"].transpose(1, 2, 3, 0).reshape(16 * G, n), li["hq"].transpose(1, 2, 0).reshape(4 * G, n),
                            li["p"].transpose(1, 2, 0).reshape(4 * G, n), li["P"].transpose(1, 2, 3, 4, 0).reshape(16 * G * G, n)])
    sums = np.concatenate([ui._ordered(li[k]).reshape(-1) for k in ("q", "hq", "p", "P")])
    return dict(xn=li["xn"], T=li["T"].reshape(n, G, 12), terms=terms, sums=sums, B=s["B"], C=s["C"], h=s["h"], cams=s["cams"], points=s["points"],
                dx=s["dx"], free=s["free"].astype(np.uint8), valid=s["valid"].astype(np.uint8), dc=s["dc"], dtheta=s["dtheta"])


def relative_differences(host, spec, what):
    """The flags are equal -> {array: max |host - spec| / max |spec|}."""
    assert np.array_equal(host["free"], spec["free"]) and np.array_equal(host["valid"], spec["valid"]), what
    out = {}
    for k in ("xn", "T", "terms", "sums", "B", "C", "h", "dx", "cams", "points"):
        finite = np.isfinite(spec[k])
        assert np.array_equal(np.isfinite(host[k]), finite), (what, k)
        scale = np.abs(spec[k][finite]).max(initial=0.0)
        diff = np.abs(np.where(finite, host[k] - spec[k], 0.0)).max(initial=0.0)
        out[k] = diff / scale if scale else float(diff != 0) * np.inf
    return out


def host_problems():
    """The windowed problem from 1.03 f with one tied group, the 300 random ones with random groups, the edge cases of
    util_bundle under two groups, and random problem 7 with a slot in a group outside the table -> [(name, problem, groups)]."""
    pw = windowed_problem()
    out = [("windowed", with_focal(pw, 1.03), tied_groups(len(pw[0])))]
    out += [(f"random {i}", p, ui.random_groups(i, len(p[0]))) for i, p in ((i, ub.random_problem(i)) for i in range(300))]
    for name, p in sorted(ub.edge_problems().items()):
        out.append((name, tuple(p), ((np.arange(len(p[0])) % 2).astype(np.int32), np.array([ui.TIED | ui.HOLD_PRINCIPAL, 0], np.uint8))))
    p = ub.random_problem(7)
    out.append(("group outside", p, (np.r_[[7, -1], np.zeros(len(p[0]) - 2)].astype(np.int32), np.array([ui.HOLD_PRINCIPAL], np.uint8))))
    return out


@lru_cache(maxsize=None)
def spec_layouts():
    return [(name, problem, groups, spec_layout(problem, groups)) for name, problem, groups in host_problems()]


def test_host_build_matches_the_spec_on_the_windowed_the_random_and_the_edge_problems(bundle_host, tmp_path):  # noqa: F811
    worst = {}
    for name, problem, groups, spec in spec_layouts():
        host, _ = run_host(bundle_host, tmp_path, problem, ub.BA_LAMBDA0, spec["dc"], groups=groups, dtheta=spec["dtheta"])
        for k, v in relative_differences(host, spec, name).items():
            if v > worst.get(k, (-1.0, ""))[0]:
                worst[k] = (v, name)
    print("worst relative differences host - spec: " + ", ".join(f"{k} {v:.3g} ({name})" for k, (v, name) in sorted(worst.items())))
    assert ui.TOL_REL == 4 * ui.HOST_SPEC_REL
    assert max(v for v, _ in worst.values()) <= ui.HOST_SPEC_REL
    masks = {int(m) for _, _, groups, _ in spec_layouts() for m in groups[1]}
    assert len(masks) >= 24 and {len(groups[1]) for _, _, groups, _ in spec_layouts()} == {1, 2, 3}


def test_host_build_under_the_sanitizers_reports_nothing(tmp_path, tmp_path_factory):
    """The same program with the host half built -fsanitize=address,undefined, run on its own over the same problems and over
    offsets and indices that name nothing."""
    program = _build(tmp_path_factory, "bundle_host_san", SANITIZE)
    for name, problem, groups, spec in spec_layouts():
        host, stderr = run_host(program, tmp_path, problem, ub.BA_LAMBDA0, spec["dc"], groups=groups, dtheta=spec["dtheta"])
        assert stderr == "" and np.array_equal(host["free"], spec["free"]), name
    cams, points, offsets, obs_cam, obs_xy, mask = ub.random_problem(7)
    bad = offsets.copy()
    bad[3], bad[-1] = bad[4] + 1, len(obs_cam) + 5
    index = [a.copy() for a in ub.camera_index(obs_cam, bad, len(cams))]
    index[0][2] = index[0][3] + 1
    index[1][index[0][4]] = len(obs_cam) + 100
    groups = (np.array([0, 1, 2 ** 31 - 1, -2 ** 31] + [1] * (len(cams) - 4), np.int32), np.array([0, ui.TIED], np.uint8))
    host, stderr = run_host(program, tmp_path, (cams, points, bad, obs_cam, obs_xy, mask), ub.BA_LAMBDA0, np.zeros(6 * len(cams)), index, groups,
                            np.zeros(8))
    assert stderr == "" and not host["T"][3].any() and not host["T"][-1].any() and not host["terms"][:, [3, -1]].any()
    assert np.isfinite(host["B"]).all() and np.isfinite(host["C"]).all() and host["valid"].all()


# ---- the product's host logic with the specification in its seams -----------------------------------------------------------------------
def spec_bundle_intr(cams, points, offsets, obs_cam, obs_xy, const_mask, device, cam_group=None, intr_mask=None, max_iterations=ub.BA_MAX_ITERATIONS):
    if cam_group is None:
        return spec_bundle(cams, points, offsets, obs_cam, obs_xy, const_mask, device)
    return ui.bundle_adjust(cams, points, offsets, obs_cam, obs_xy, const_mask, cam_group, intr_mask, max_iterations)


def build_adjusted(path, **kw):
    from vit_colmap_amd.mapping.bundle import build_adjusted_model

    return build_adjusted_model(path, device="cpu", two_view_pose_fn=spec_two_view_pose, estimate_fn=spec_estimate,
                                triangulate_fn=spec_triangulate, bundle_fn=spec_bundle_intr, **kw)


def scene_with_focal(factor):
    """The windowed scene whose database carries the camera's focal at `factor` times the truth."""
    scene = dict(windowed()[0])
    K = scene["K"].copy()
    K[0, 0], K[1, 1] = K[0, 0] * factor, K[1, 1] * factor
    scene["K"] = K
    return scene


def test_build_adjusted_model_writes_the_refined_focal_and_without_the_flag_todays_model(tmp_path):
    from vit_colmap_amd.mapping.grow import build_sparse_model
    from vit_colmap_amd.mapping.seed import SparseModel

    scene, pairs = windowed()[:2]
    f = scene["K"][0, 0]
    write_scene_db(tmp_path / "w.db", scene_with_focal(1.03), pairs)
    grown = build_sparse_model(tmp_path / "w.db", device="cpu", two_view_pose_fn=spec_two_view_pose, estimate_fn=spec_estimate,
                               triangulate_fn=spec_triangulate)
    grown.write_text(tmp_path / "grown")
    grown_bytes = {n: (tmp_path / "grown" / n).read_bytes() for n in ("cameras.txt", "images.txt", "points3D.txt")}
    plain = build_adjusted(tmp_path / "w.db", grown=grown)
    refined = build_adjusted(tmp_path / "w.db", grown=grown, refine_focal_length=True)
    # the grown model that was handed in is what it was
    grown.write_text(tmp_path / "grown_after")
    assert all((tmp_path / "grown_after" / n).read_bytes() == b for n, b in grown_bytes.items())
    # without the flag: today's model, which never calls the seam with groups and whose report has no such key
    assert "intrinsics" not in plain.stats()["bundle_adjustment"] and plain.cameras == grown.cameras
    assert plain == build_adjusted(tmp_path / "w.db", grown=grown, refine_focal_length=False)
    plain.write_text(tmp_path / "plain")
    (tmp_path / "today").mkdir()
    from vit_colmap_amd.mapping import bundle_intr
    from vit_colmap_amd.mapping.bundle import build_adjusted_model
    build_adjusted_model(tmp_path / "w.db", device="cpu", bundle_fn=spec_bundle, grown=grown).write_text(tmp_path / "today")
    for n in grown_bytes:
        assert (tmp_path / "plain" / n).read_bytes() == (tmp_path / "today" / n).read_bytes()
    # with it: one PINHOLE camera, one group of fx and fy; both are refined, the principal point is not
    (cid, cam), = refined.cameras.items()
    before = grown.cameras[cid]
    report = refined.stats()["bundle_adjustment"]["intrinsics"]
    fx, fy = (float(v) for v in cam.params[:2])
    print(f"focal {before.params[0]:.3f} -> {fx:.4f}, {fy:.4f} (truth {f}), cost {refined.bundle_adjustment['final_cost']:.4f} "
          f"(held: {plain.bundle_adjustment['final_cost']:.4f})")
    # fx is within the 1 % that the end-to-end test asks of the written focal (measured 600.040, 0.007 %).  fy is not held to
    # it: the views of this scene stand at one height, so the scene's height trades against fy and the data barely say what fy
    # is (measured 591.894, 1.35 % off, from either start, also on the model grown under the true focal); it has to end nearer
    # the truth than the 3 % it started at
    assert cam.model == before.model == "PINHOLE" and len(cam.params) == 4 and abs(fx - f) / f <= 0.01 and abs(fy - f) / f < 0.03
    assert list(cam.params[2:]) == list(before.params[2:]) and fx != fy
    assert report[cid]["before"] == [float(v) for v in before.params] and report[cid]["after"] == [float(v) for v in cam.params]
    assert refined.bundle_adjustment["final_cost"] < plain.bundle_adjustment["final_cost"]
    assert all(p["error"] <= ub.MAX_ERROR for p in refined.points3D.values())
    refined.write_text(tmp_path / "refined")
    back = SparseModel.read_text(tmp_path / "refined")
    assert back == refined and [float(v) for v in back.cameras[cid].params] == [fx, fy, *before.params[2:]]
    # a model of one focal length is a tied group: the seam sees bit 4, and the camera gets one number
    seen = {}

    def tied_seam(*a, cam_group=None, intr_mask=None, max_iterations=None):
        seen.update(cam_group=cam_group, intr_mask=intr_mask, max_iterations=max_iterations)
        return spec_bundle_intr(*a, cam_group=cam_group, intr_mask=intr_mask, max_iterations=max_iterations)

    simple = copy.deepcopy(grown)
    simple.cameras[cid].model, simple.cameras[cid].params = "SIMPLE_PINHOLE", [before.params[0], before.params[2], before.params[3]]
    model = build_adjusted_model(tmp_path / "w.db", device="cpu", bundle_fn=tied_seam, grown=simple, refine_focal_length=True)
    assert list(seen["intr_mask"]) == [ui.TIED | ui.HOLD_PRINCIPAL] and not seen["cam_group"].any() and len(seen["cam_group"]) == 12
    assert seen["max_iterations"] == bundle_intr.REFINE_MAX_ITERATIONS > ub.BA_MAX_ITERATIONS and model.bundle_adjustment["iterations"] < 25
    assert len(model.cameras[cid].params) == 3 and abs(model.cameras[cid].params[0] - f) / f <= 0.01
    assert list(model.cameras[cid].params[1:]) == list(before.params[2:])
    # more cameras than the border holds: the ValueError names the limit
    many = copy.deepcopy(grown)
    for k, i in enumerate(sorted(many.images)):
        many.images[i]["camera_id"] = 100 + k
        many.cameras[100 + k] = copy.deepcopy(before)
    with pytest.raises(ValueError, match="VC_BA_MAX_GROUPS"):
        build_adjusted_model(tmp_path / "w.db", device="cpu", bundle_fn=spec_bundle_intr, grown=many, refine_focal_length=True)


def test_refine_focal_length_flag_is_off_by_default_and_needs_bundle_adjustment(tmp_path, monkeypatch):
    import argparse

    from vit_colmap_amd.pipeline import run_pipeline as rp
    from vit_colmap_amd.utils.config import Config, ReconstructionConfig

    assert ReconstructionConfig().refine_focal_length is False and Config().reconstruction.refine_focal_length is False
    assert Config.from_args(argparse.Namespace(refine_focal_length=True)).reconstruction.refine_focal_length is True
    assert Config.from_args(argparse.Namespace(refine_focal_length=True)).reconstruction.bundle_adjustment is False
    assert Config.from_args(argparse.Namespace()).reconstruction.refine_focal_length is False

    def no_extractor(self):
        raise AssertionError("the extractor was built before the flags were checked")

    monkeypatch.setattr(rp.Pipeline, "_make_extractor", no_extractor)
    cfg = Config()
    cfg.reconstruction.refine_focal_length, cfg.reconstruction.sparse_model = True, True
    cfg.camera.prior_focal_length, cfg.matching.compute_relative_pose, cfg.do_reconstruction = True, True, False
    with pytest.raises(ValueError, match="refine_focal_length needs .*bundle_adjustment"):
        rp.Pipeline(cfg).run(tmp_path / "images", tmp_path / "out", tmp_path / "x.db")
    seen = []
    monkeypatch.setattr(rp.Pipeline, "run", lambda self, *a, **k: seen.append((self.config.reconstruction.bundle_adjustment,
                                                                               self.config.reconstruction.refine_focal_length)))
    for extra in ([], ["--sparse-model", "--bundle-adjustment"], ["--sparse-model", "--bundle-adjustment", "--refine-focal-length"]):
        monkeypatch.setattr(sys, "argv", ["prog", "--images", "i", "--output", "o", "--db", "d"] + extra)
        rp.main()
    assert seen == [(False, False), (True, False), (True, True)]
    # with the flag off the border's front end is not imported
    code = ("import sys; import vit_colmap_amd.mapping.bundle; import vit_colmap_amd.pipeline.run_pipeline; "
            "assert 'vit_colmap_amd.mapping.bundle_intr' not in sys.modules")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


def test_pipeline_passes_the_flag_and_leaves_the_grown_model_alone(tmp_path, monkeypatch):
    import vit_colmap_amd.mapping.bundle as bundle
    import vit_colmap_amd.mapping.grow as grow
    from vit_colmap_amd.pipeline import run_pipeline as rp
    from vit_colmap_amd.utils.config import Config

    scene, pairs = windowed()[:2]
    write_scene_db(tmp_path / "w.db", scene_with_focal(1.03), pairs)
    real = grow.build_sparse_model
    monkeypatch.setattr(grow, "build_sparse_model", lambda path, device="cuda": real(path, device="cpu", two_view_pose_fn=spec_two_view_pose,
                                                                                     estimate_fn=spec_estimate, triangulate_fn=spec_triangulate))
    monkeypatch.setattr(bundle, "bundle_adjust", spec_bundle_intr)
    texts = {}
    for name, refine in (("held", False), ("refined", True)):
        p = rp.Pipeline(Config())
        p.last_stats = {}
        p._write_sparse_model(tmp_path / "w.db", tmp_path / name, "cpu", adjust=True, refine_focal_length=refine)
        texts[name] = {m: {n: (tmp_path / name / "sparse" / m / n).read_bytes() for n in ("cameras.txt", "images.txt", "points3D.txt")}
                       for m in ("grown", "adjusted")}
        assert ("intrinsics" in p.last_stats["bundle_adjustment"]["bundle_adjustment"]) == refine
    assert texts["held"]["grown"] == texts["refined"]["grown"]                   # sparse/grown is byte for byte unchanged
    assert texts["held"]["adjusted"]["cameras.txt"] == texts["held"]["grown"]["cameras.txt"]
    # sparse/adjusted/cameras.txt differs from sparse/grown/cameras.txt in the focal only
    a, b = (texts["refined"][m]["cameras.txt"].decode().splitlines() for m in ("grown", "adjusted"))
    assert len(a) == len(b) and [x for x, y in zip(a, b) if x != y] != []
    for x, y in zip(a, b):
        if x != y:
            wx, wy = x.split(), y.split()                                       # id, PINHOLE, width, height, fx, fy, cx, cy
            assert wx[:4] == wy[:4] and wx[6:] == wy[6:] and wx[4] != wy[4] and wx[5] != wy[5]
            assert abs(float(wy[4]) - scene["K"][0, 0]) / scene["K"][0, 0] <= 0.01 and abs(float(wy[5]) - scene["K"][0, 0]) / scene["K"][0, 0] < 0.03
