"""CPU tests of bundle adjustment under a robust loss ("The loss"): the numpy specification of
tests/util_bundle_loss.py (the gradient of the reweighted system, the trivial loss bit for bit, the special residuals, the exact
scene, the contaminated windowed scene against the plain loss), the kernels' routines compiled for the host
(tools/bundle_host.cpp with the loss extension of its problem file) against it, plain and under the host sanitizers, the
product's host logic with the specification in its seams, the configuration and the command line.  No GPU."""
import os
import subprocess
import sys
from functools import lru_cache

import numpy as np
import pytest

import util_absolute_pose as ua
import util_bundle as ub
import util_bundle_intr as ui
import util_bundle_loss as ul
from test_absolute_pose_spec import spec_estimate, spec_two_view_pose, write_scene_db
from test_bundle_intr_spec import tied_groups, windowed_problem, with_focal
from test_bundle_spec import (ROOT, SANITIZE, _build, adjusted, assert_adjusted_model_follows, bundle_host, exact_problem, host_problems,  # noqa: F401
                              read_result_file, spec_bundle, write_problem_file)
from test_mapper_spec import spec_triangulate, windowed

LOSS_CASES = [(ul.HUBER, 1.0), (ul.SOFT_L1, 1.0), (ul.HUBER, 0.25), (ul.SOFT_L1, 0.25)]
# central differences (step 1e-6 rad / scene units, as test_bundle_spec) of 0.5 rho(|r|^2) of the specification's own residual
# against (sw J_c)'(sw r) and (sw J_p)'(sw r) on 20 observations x both losses x three scales that put the residual on either
# side of s = c^2 (c = 0.5 |r|, 2 |r| and 1 px), measured: worst |difference| relative to the largest entry of the gradient
# 8.62e-8, on Huber's outer branch at a residual of 0.16 px (the step moves the residual by 1e-4 px, a thousandth of its length:
# what is left is the step's square times the third derivative of c |r|, which grows as the residual shrinks; a wrong weight
# is wrong by a number of order 1); the bound is 4x, rounded up
FD_STEP, FD_GRAD_BOUND = 1e-6, 3.5e-7
# the contaminated windowed scene (5 % of the observations displaced by 8-40 px) under the cap of 25 linearisations, measured by
# the specification: plain loss 1.9311 deg, 0.13314 baselines, 406 of the 4069 uncorrupted observations filtered, 1019 of 1161
# points kept; Huber 1 px 0.1838 deg, 0.01266 bl, 68, 1127 points; soft L1 1 px 0.2041 deg, 0.01451 bl, 67, 1131 points (the grown
# model itself: 1.520 deg, 0.0853 bl).  The bounds are 2x the robust figures, rounded up.
ROBUST_BOUNDS = {ul.HUBER: (0.37, 0.026, 136), ul.SOFT_L1: (0.41, 0.030, 134)}


# ---- the specification ---------------------------------------------------------------------------------------------------------------
def robust_cost(kind, c, r):
    return 0.5 * float(ul.loss_terms(kind, c, r[0] * r[0] + r[1] * r[1])[0])


def test_reweighted_gradient_matches_central_differences_of_the_robust_cost():
    worst, sides = 0.0, set()
    for i in range(20):
        cams, points, offsets, obs_cam, obs_xy, _ = ub.random_problem(i)
        o = (7 * i) % len(obs_cam)
        j = int(np.searchsorted(offsets, o, side="right") - 1)
        row, X, uv = cams[obs_cam[o]], points[j], obs_xy[o]
        usable, r, Jc, Jp = ub.observe(row, X, uv)
        assert usable
        norm = float(np.sqrt(r @ r))
        for kind in (ul.HUBER, ul.SOFT_L1):
            for c in (0.5 * norm, 2.0 * norm, 1.0):
                s = r[0] * r[0] + r[1] * r[1]
                sides.add((kind, bool(s <= c * c)))
                rho, w = ul.loss_terms(kind, c, s)
                sw = np.sqrt(w)
                grad_c, grad_p = (sw * Jc).T @ (sw * r), (sw * Jp).T @ (sw * r)
                num_c, num_p = np.zeros(6), np.zeros(3)
                for k in range(6):
                    e = np.zeros(6)
                    e[k] = FD_STEP
                    num_c[k] = (robust_cost(kind, c, ub.residual_at(row, X, uv, e[:3], e[3:]))
                                - robust_cost(kind, c, ub.residual_at(row, X, uv, -e[:3], -e[3:]))) / (2 * FD_STEP)
                for k in range(3):
                    e = np.zeros(3)
                    e[k] = FD_STEP
                    num_p[k] = (robust_cost(kind, c, ub.residual_at(row, X + e, uv, np.zeros(3), np.zeros(3)))
                                - robust_cost(kind, c, ub.residual_at(row, X - e, uv, np.zeros(3), np.zeros(3)))) / (2 * FD_STEP)
                scale = max(np.abs(grad_c).max(), np.abs(grad_p).max())
                diff = max(np.abs(num_c - grad_c).max(), np.abs(num_p - grad_p).max())
                worst = max(worst, diff / scale)
                assert diff <= FD_GRAD_BOUND * scale, (i, kind, c, diff, scale)
    print(f"worst relative difference of the reweighted gradient to central differences {worst:.3g}")
    assert sides == {(ul.HUBER, True), (ul.HUBER, False), (ul.SOFT_L1, True), (ul.SOFT_L1, False)}


def test_trivial_loss_through_the_loss_path_is_bit_equal_to_util_bundle():
    problem = windowed_problem()
    want = ub.linearize(*problem, ub.BA_LAMBDA0)
    got = ul.linearize(*problem, ub.BA_LAMBDA0, ul.TRIVIAL, 3.0)
    for k in ("ok", "r", "Jc", "Jp", "W", "vinv", "gp", "cost", "count", "constant"):
        assert got[k].tobytes() == want[k].tobytes(), k
    assert got["total_cost"] == want["total_cost"] and np.array_equal(got["sw"], want["ok"].astype(np.float64)) and want["ok"].all()
    groups = tied_groups(len(problem[0]))
    li, li0 = (f(lin, problem[0], problem[1], problem[2], problem[3], groups[0], 1, groups[1])
               for f, lin in ((ul.linearize_intrinsics, got), (ui.linearize_intrinsics, want)))
    assert all(li[k].tobytes() == li0[k].tobytes() for k in li0)
    # and the loop: the decisions and every bit of the result, on a problem with unusable observations too
    for p in (ub.random_problem(5), ub.edge_problems()["nan_pixel"]):
        cams, points, report = ul.bundle_adjust(*p, ul.TRIVIAL, 1.0)
        want_cams, want_points, want_report = ub.bundle_adjust(*p)
        assert report["decisions"] == want_report["decisions"] and report["final_cost"] == want_report["final_cost"]
        assert np.array_equal(cams, want_cams) and np.array_equal(points, want_points)
        lin = ul.linearize(*p, ub.BA_LAMBDA0, ul.TRIVIAL, 1.0)
        assert np.array_equal(lin["sw"], lin["ok"].astype(np.float64))


def test_special_residuals_take_the_branches_the_rule_gives():
    for c in (1.0, 0.25, 3.0):
        rho, w = ul.loss_terms(ul.HUBER, c, c * c)                   # s == c^2 exactly: the quadratic branch
        assert rho == c * c and w == 1.0
        above = 1.01 * c * c
        rho, w = ul.loss_terms(ul.HUBER, c, above)
        assert w == c / np.sqrt(above) < 1.0 and rho == (2.0 * c) * np.sqrt(above) - c * c < above
        for kind in (ul.HUBER, ul.SOFT_L1):
            rho, w = ul.loss_terms(kind, c, 0.0)                     # r = 0
            assert rho == 0.0 and w == 1.0
        # soft L1 without cancellation: a residual of rounding size keeps its square
        rho, w = ul.loss_terms(ul.SOFT_L1, c, 1e-26)
        assert rho == 1e-26 and w == 1.0 and 2.0 * c * c * (np.sqrt(1.0 + 1e-26 / (c * c)) - 1.0) == 0.0
    # an s that overflows: w = 0 and a cost that is not finite (inf under Huber, inf / inf under soft L1), no special case
    for kind in (ul.HUBER, ul.SOFT_L1):
        rho, w = ul.loss_terms(kind, 1.0, np.inf)
        assert w == 0.0 and not np.isfinite(rho) and (rho == np.inf or kind == ul.SOFT_L1)
    # an observation with a residual of exactly 0 in a linearisation
    cams, points, offsets, obs_cam, obs_xy, mask = ub.random_problem(3)
    obs_xy = obs_xy.copy()
    j = int(np.searchsorted(offsets, 4, side="right") - 1)
    obs_xy[4] = ub.observe(cams[obs_cam[4]], points[j], np.zeros(2))[1]          # the projection in the kernel's order: r = 0 exactly
    for kind in (ul.HUBER, ul.SOFT_L1):
        got = ul.linearize(cams, points, offsets, obs_cam, obs_xy, mask, ub.BA_LAMBDA0, kind, 0.25)
        assert not got["r"][4].any() and got["sw"][4] == 1.0 and (got["sw"][np.arange(len(obs_cam)) != 4] < 1.0).any()


def test_exact_scene_keeps_its_cost_of_rounding_size_under_both_losses():
    """As test_bundle_spec's exact scene: residuals of 1e-13 px, a cost of order 1e-25.  Both losses are the square there (Huber
    exactly, soft L1 to the last place), so the cost is neither 0 (a form with cancellation would make it 0) nor larger."""
    cams, points, offsets, obs_cam, obs_xy, mask = exact_problem()
    plain = ub.linearize(cams, points, offsets, obs_cam, obs_xy, mask, ub.BA_LAMBDA0)["total_cost"]
    assert 0.0 < plain <= 1e-20
    for kind in (ul.HUBER, ul.SOFT_L1):
        out_cams, out_points, report = ul.bundle_adjust(cams, points, offsets, obs_cam, obs_xy, mask, kind, 1.0)
        print(f"loss {kind}: cost {report['initial_cost']:.3g} -> {report['final_cost']:.3g} (plain {plain:.3g})")
        assert report["initial_cost"] == pytest.approx(plain, rel=1e-12) and 0.0 < report["final_cost"] <= 1e-20
        assert np.abs(out_cams - cams).max() <= 1e-9 and np.abs(out_points - points).max() <= 1e-9


@lru_cache(maxsize=None)
def contaminated_runs():
    """The corrupted windowed problem under the plain loss, Huber 1 px and soft L1 1 px -> {loss: (rotation deg, centre
    baselines, uncorrupted observations filtered, points kept, report)}."""
    scene, _, grown, model_problem, _ = adjusted()
    ids = model_problem[0]
    a, b = grown["initial_pair"]
    sa, sb = ids.index(a), ids.index(b)
    problem, bad = ul.corrupted_windowed_problem()
    cams, points, offsets, obs_cam, obs_xy, mask = problem
    is_bad = np.zeros(len(obs_cam), bool)
    is_bad[bad] = True
    out = {}
    for kind in (ul.TRIVIAL, ul.HUBER, ul.SOFT_L1):
        new_cams, new_points, report = ul.bundle_adjust(*problem, kind, 1.0)
        scaled, scaled_points = ub.rescale(new_cams, new_points, sa, sb)
        keep_obs, keep_point, _ = ub.filter_tracks(scaled, scaled_points, offsets, obs_cam, obs_xy)
        rot, pos = ua.align_errors({i: (scaled[s, :9].reshape(3, 3), scaled[s, 9:12]) for s, i in enumerate(ids)}, scene, a, b)
        out[kind] = (rot, pos, int((~keep_obs & ~is_bad).sum()), int(keep_point.sum()), report)
    return out, len(bad), len(obs_cam)


def test_robust_loss_keeps_outliers_from_setting_the_poses():
    """The test that fails without the feature: on the same corrupted problem, under the same cap, Huber 1 px and soft L1 1 px
    each leave at most a quarter of the plain loss's worst rotation, worst centre and filtered uncorrupted observations."""
    runs, n_bad, total = contaminated_runs()
    assert (n_bad, total) == (214, 4283)
    for kind, (rot, pos, dropped, kept, report) in runs.items():
        print(f"loss {kind}: rotation {rot:.4f} deg, centre {pos:.5f} baselines, {dropped} of {total - n_bad} uncorrupted observations "
              f"filtered, {kept} points kept, cost {report['initial_cost']:.1f} -> {report['final_cost']:.1f} in {report['iterations']} "
              f"linearisations, {report['accepted_steps']} accepted")
    rot0, pos0, dropped0, _, plain = runs[ul.TRIVIAL]
    # the plain loss through the loss path is today's loop
    want = ub.bundle_adjust(*ul.corrupted_windowed_problem()[0])[2]
    assert plain["decisions"] == want["decisions"] and plain["final_cost"] == want["final_cost"]
    for kind in (ul.HUBER, ul.SOFT_L1):
        rot, pos, dropped, kept, report = runs[kind]
        assert rot <= rot0 / 4 and pos <= pos0 / 4 and dropped <= dropped0 / 4, kind
        rot_bound, pos_bound, dropped_bound = ROBUST_BOUNDS[kind]
        assert rot <= rot_bound and pos <= pos_bound and dropped <= dropped_bound, kind
        assert report["iterations"] <= ub.BA_MAX_ITERATIONS and report["final_cost"] < report["initial_cost"]


# ---- the kernels' routines on the host ---------------------------------------------------------------------------------------------------
def run_host_loss(program, tmp_path, problem, lam, dc, loss, loss_scale, index=None, groups=None, dtheta=(), expect=0):
    """tools/bundle_host.cpp on a problem file that carries the loss -> (result, obs_w included; stderr), or with `expect` another
    exit status (None, stderr)."""
    write_problem_file(tmp_path / "problem.bin", problem, lam, dc, index, groups, dtheta)
    with open(tmp_path / "problem.bin", "ab") as f:
        f.write(np.array([loss], np.int32).tobytes() + np.array([loss_scale], np.float64).tobytes())
    done = subprocess.run([program, str(tmp_path / "problem.bin"), str(tmp_path / "result.bin")], stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, text=True)
    assert done.returncode == expect, done.stderr
    if expect:
        return None, done.stderr
    total = len(problem[3])
    raw = (tmp_path / "result.bin").read_bytes()
    (tmp_path / "result.bin").write_bytes(raw[:len(raw) - 8 * total])
    out = read_result_file(tmp_path / "result.bin", len(problem[0]), len(problem[1]), total, len(groups[1]) if groups else 0)
    out["obs_w"] = np.frombuffer(raw, np.float64, total, len(raw) - 8 * total)
    return out, done.stderr


def spec_layout(problem, groups, loss, loss_scale, lam=ub.BA_LAMBDA0):
    """One linearisation, both reductions, both solves and both steps of the specification under the loss, in the host
    program's layout: the plain section under "plain"; a system that does not factor steps with 0."""
    cams, points, offsets, obs_cam, obs_xy, mask = problem
    cam_group, intr_mask = groups
    G, n, index = len(intr_mask), len(points), ub.camera_index(obs_cam, offsets, len(cams))
    lin = ul.linearize(cams, points, offsets, obs_cam, obs_xy, mask, lam, loss, loss_scale)
    S, g = ub.reduce_cameras(lin, len(cams), offsets, obs_cam, mask, *index, lam)
    li = ul.linearize_intrinsics(lin, cams, points, offsets, obs_cam, cam_group, G, intr_mask)
    B, C, h, free = ui.reduce_border(lin, li, len(cams), cam_group, G, intr_mask, offsets, obs_cam, *index, lam)
    dc, dtheta = ui.solve_bordered(S, g, B, C, h, mask, free)
    if dc is None:
        dc, dtheta = np.zeros(6 * len(cams)), np.zeros(4 * G)
    plain_cams, plain_points, plain_dx = ub.step(lin, cams, points, offsets, obs_cam, dc)
    out_cams, out_points, dX, valid = ui.step_intrinsics(lin, li, cams, points, offsets, obs_cam, cam_group, G, intr_mask, dc, dtheta)
    terms = np.concatenate([li["q"].transpose(1, 2, 3, 0).reshape(16 * G, n), li["hq"].transpose(1, 2, 0).reshape(4 * G, n),
                            li["p"].transpose(1, 2, 0).reshape(4 * G, n), li["P"].transpose(1, 2, 3, 4, 0).reshape(16 * G * G, n)])
    sums = np.concatenate([ui._ordered(li[k]).reshape(-1) for k in ("q", "hq", "p", "P")])
    plain = dict(vinv=lin["vinv"].reshape(-1, 9)[:, [0, 1, 2, 4, 5, 8]], gp=lin["gp"], cost=lin["cost"], total_cost=np.array([lin["total_cost"]]),
                 S=S, g=g, cams=plain_cams, points=plain_points, dx=plain_dx, count=lin["count"], obs_ok=lin["ok"].astype(np.uint8))
    return dict(xn=li["xn"], T=li["T"].reshape(n, G, 12), terms=terms, sums=sums, B=B, C=C, h=h, cams=out_cams, points=out_points, dx=dX,
                free=free.astype(np.uint8), valid=valid.astype(np.uint8), obs_w=lin["sw"], plain=plain, dc=dc, dtheta=dtheta,
                constant=lin["constant"])


def relative_differences(host, spec, what):
    """The flags, the counts, the constant points and the pattern of obs_w == 0 are equal -> {array: max |host - spec| / max |spec|}
    over the plain section, the border's section and obs_w."""
    assert np.array_equal(host["free"], spec["free"]) and np.array_equal(host["valid"], spec["valid"]), what
    assert np.array_equal(host["plain"]["count"], spec["plain"]["count"]) and np.array_equal(host["plain"]["obs_ok"], spec["plain"]["obs_ok"]), what
    assert np.array_equal(~host["plain"]["vinv"].any(axis=1), spec["constant"]), what
    assert np.array_equal(host["obs_w"] == 0, spec["obs_w"] == 0) and np.array_equal(host["obs_w"] == 0, spec["plain"]["obs_ok"] == 0), what
    assert not host["plain"]["obs_lin"][host["plain"]["obs_ok"] == 0].any(), what      # exactly 0, not 0 times a weight that is NaN
    out = {}
    pairs = [(k, host[k], spec[k]) for k in ("xn", "T", "terms", "sums", "B", "C", "h", "dx", "cams", "points", "obs_w")]
    pairs += [("plain " + k, host["plain"][k], spec["plain"][k]) for k in ("vinv", "gp", "S", "g", "dx", "cost", "total_cost", "cams", "points")]
    for k, a, b in pairs:
        finite = np.isfinite(b)
        assert np.array_equal(np.isfinite(a), finite), (what, k)
        scale = np.abs(b[finite]).max(initial=0.0)
        diff = np.abs(np.where(finite, a - b, 0.0)).max(initial=0.0)
        out[k] = diff / scale if scale else float(diff != 0) * np.inf
    return out


def loss_problems():
    """The windowed problem from 1.03 f with one tied group, the corrupted one with fx and fy, the 300 random problems with the
    random groups and masks of test_bundle_intr_spec and the nine edge problems under two groups -> [(name, problem, groups)]."""
    pw = windowed_problem()
    pc = ul.corrupted_windowed_problem()[0]
    out = [("windowed", with_focal(pw, 1.03), tied_groups(len(pw[0]))),
           ("corrupted", pc, (np.zeros(len(pc[0]), np.int32), np.array([ui.HOLD_PRINCIPAL], np.uint8)))]
    out += [(f"random {i}", p, ui.random_groups(i, len(p[0]))) for i, p in ((i, ub.random_problem(i)) for i in range(300))]
    for name, p in sorted(ub.edge_problems().items()):
        out.append((name, tuple(p), ((np.arange(len(p[0])) % 2).astype(np.int32), np.array([ui.TIED | ui.HOLD_PRINCIPAL, 0], np.uint8))))
    return out


@lru_cache(maxsize=None)
def spec_layouts():
    return [(name, problem, groups, loss, c, spec_layout(problem, groups, loss, c))
            for name, problem, groups in loss_problems() for loss, c in LOSS_CASES]


def test_host_build_matches_the_spec_under_both_losses(bundle_host, tmp_path):  # noqa: F811
    worst, outer = {}, {}
    for name, problem, groups, loss, c, spec in spec_layouts():
        host, _ = run_host_loss(bundle_host, tmp_path, problem, ub.BA_LAMBDA0, spec["dc"], loss, c, groups=groups, dtheta=spec["dtheta"])
        for k, v in relative_differences(host, spec, (name, loss, c)).items():
            if v > worst.get(k, (-1.0, ""))[0]:
                worst[k] = (v, f"{name}, loss {loss} at {c}")
        usable = spec["obs_w"] != 0
        outer.setdefault((loss, c), []).append((int((spec["obs_w"][usable] < 1).sum()), int(usable.sum())))
    print("worst relative differences host - spec: " + ", ".join(f"{k} {v:.3g} ({name})" for k, (v, name) in sorted(worst.items())))
    for (loss, c), counts in sorted(outer.items()):
        down, usable = (sum(x) for x in zip(*counts))
        print(f"loss {loss} at {c} px: {down} of {usable} usable observations weighted down")
        if c == 0.25:
            assert down > usable / 2                                 # most observations are on the outer branch
    assert ul.TOL_REL == 4 * ul.HOST_SPEC_REL
    assert max(v for v, _ in worst.values()) <= ul.HOST_SPEC_REL
    assert len(spec_layouts()) == 311 * len(LOSS_CASES)


def test_host_build_without_the_extension_and_with_the_trivial_loss_writes_the_same_bytes(bundle_host, tmp_path):  # noqa: F811
    """A problem file that carries the trivial loss runs the loss variants: every byte of the result is the plain program's,
    and obs_w is 1 on usable observations."""
    from test_bundle_spec import run_host

    for seed, problem in ((7, ub.random_problem(7)), (8, ub.edge_problems()["short_tracks"]), (9, ub.edge_problems()["nan_camera"])):
        groups = ui.random_groups(seed, len(problem[0]))
        dc = np.random.RandomState(seed).normal(0, 2e-3, 6 * len(problem[0]))
        dtheta = np.random.RandomState(seed).normal(0, 0.5, 4 * len(groups[1]))
        for gr, dth in ((None, ()), (groups, dtheta)):
            run_host(bundle_host, tmp_path, problem, ub.BA_LAMBDA0, dc, groups=gr, dtheta=dth)
            want = (tmp_path / "result.bin").read_bytes()
            host, _ = run_host_loss(bundle_host, tmp_path, problem, ub.BA_LAMBDA0, dc, ul.TRIVIAL, 2.5, groups=gr, dtheta=dth)
            assert (tmp_path / "result.bin").read_bytes() == want, (seed, gr is None)          # run_host_loss cut obs_w off again
            ok = (host["plain"] if gr else host)["obs_ok"]
            assert np.array_equal(host["obs_w"], ok.astype(np.float64))


def test_host_build_under_the_sanitizers_reports_nothing(tmp_path, tmp_path_factory):
    """The same program with the host half built -fsanitize=address,undefined, run on its own over the same problems, over
    offsets and indices that name nothing and over losses the entry point refuses."""
    program = _build(tmp_path_factory, "bundle_host_san", SANITIZE)
    for name, problem, groups, loss, c, spec in spec_layouts():
        host, stderr = run_host_loss(program, tmp_path, problem, ub.BA_LAMBDA0, spec["dc"], loss, c, groups=groups, dtheta=spec["dtheta"])
        assert stderr == "" and np.array_equal(host["free"], spec["free"]) and np.array_equal(host["obs_w"] == 0, spec["obs_w"] == 0), name
    cams, points, offsets, obs_cam, obs_xy, mask = ub.random_problem(7)
    bad = offsets.copy()
    bad[3], bad[-1] = bad[4] + 1, len(obs_cam) + 5
    index = [a.copy() for a in ub.camera_index(obs_cam, bad, len(cams))]
    index[0][2] = index[0][3] + 1
    index[1][index[0][4]] = len(obs_cam) + 100
    groups = (np.array([0, 1, 2 ** 31 - 1, -2 ** 31] + [1] * (len(cams) - 4), np.int32), np.array([0, ui.TIED], np.uint8))
    for loss, c in LOSS_CASES:
        host, stderr = run_host_loss(program, tmp_path, (cams, points, bad, obs_cam, obs_xy, mask), ub.BA_LAMBDA0, np.zeros(6 * len(cams)),
                                     loss, c, index, groups, np.zeros(8))
        assert stderr == "" and host["plain"]["count"][3] == 0 and host["plain"]["count"][-1] == 0
        assert not host["T"][3].any() and not host["T"][-1].any() and not host["terms"][:, [3, -1]].any()
        assert np.isfinite(host["B"]).all() and np.isfinite(host["C"]).all() and np.isfinite(host["plain"]["S"]).all()
        assert not host["obs_w"][offsets[-2]:].any()                  # the track of the last point, which is skipped
    # what vc_ba_linearize_points_loss answers with VC_ERR_INVALID_ARG: one line, status 3, no sanitizer report
    problem = ub.random_problem(7)
    for loss, c in ((ul.HUBER, 0.0), (ul.HUBER, -1.0), (ul.SOFT_L1, np.nan), (ul.SOFT_L1, np.inf), (3, 1.0), (-1, 1.0)):
        _, stderr = run_host_loss(program, tmp_path, problem, ub.BA_LAMBDA0, np.zeros(6 * len(problem[0])), loss, c, expect=3)
        assert stderr.count("\n") == 1 and "is refused" in stderr, (loss, c, stderr)


# ---- the product's host logic with the specification in its seams -----------------------------------------------------------------------
def spec_bundle_loss(cams, points, offsets, obs_cam, obs_xy, const_mask, device, loss="trivial", loss_scale=1.0):
    return ul.bundle_adjust(cams, points, offsets, obs_cam, obs_xy, const_mask, ul.LOSSES[loss], loss_scale)


def build_adjusted(path, bundle_fn, **kw):
    from vit_colmap_amd.mapping.bundle import build_adjusted_model

    return build_adjusted_model(path, device="cpu", two_view_pose_fn=spec_two_view_pose, estimate_fn=spec_estimate,
                                triangulate_fn=spec_triangulate, bundle_fn=bundle_fn, **kw)


def test_build_adjusted_model_passes_the_loss_on_and_without_it_is_todays(tmp_path):
    from vit_colmap_amd.mapping.grow import build_sparse_model

    scene, images, grown, _, adj = adjusted()
    write_scene_db(tmp_path / "w.db", scene, windowed()[1])
    grown_model = build_sparse_model(tmp_path / "w.db", device="cpu", two_view_pose_fn=spec_two_view_pose, estimate_fn=spec_estimate,
                                     triangulate_fn=spec_triangulate)
    spec = ub.adjust_model(images, grown, adjust=lambda *a: ul.bundle_adjust(*a, ul.HUBER, 1.5))
    seen = []

    def seam(*a, **kw):
        seen.append((len(a), dict(kw)))
        return spec_bundle_loss(*a, **kw)

    model = build_adjusted(tmp_path / "w.db", seam, grown=grown_model, loss="huber", loss_scale=1.5)
    assert seen == [(7, dict(loss="huber", loss_scale=1.5))]
    assert_adjusted_model_follows(model, spec, 1e-9)                 # tracks and ids exactly, poses and points to 1e-9
    ba = model.stats()["bundle_adjustment"]
    assert ba["loss"] == "huber" and ba["loss_scale"] == 1.5 and ba["iterations"] == spec["report"]["iterations"]
    assert ba["final_cost"] == pytest.approx(spec["report"]["final_cost"], rel=1e-9) and "decisions" not in ba
    # without the loss arguments (and with the trivial loss named) the seam is called with today's arguments and the model is
    # byte for byte today's
    today = build_adjusted(tmp_path / "w.db", spec_bundle, grown=grown_model)
    today.write_text(tmp_path / "today")
    for name, kw in (("default", {}), ("trivial", dict(loss="trivial", loss_scale=3.0))):
        del seen[:]
        plain = build_adjusted(tmp_path / "w.db", seam, grown=grown_model, **kw)
        assert seen == [(7, {})] and plain == today and sorted(plain.stats()["bundle_adjustment"]) == sorted(today.stats()["bundle_adjustment"])
        assert "loss" not in plain.stats()["bundle_adjustment"]
        plain.write_text(tmp_path / name)
        for n in ("cameras.txt", "images.txt", "points3D.txt"):
            assert (tmp_path / name / n).read_bytes() == (tmp_path / "today" / n).read_bytes()
    assert_adjusted_model_follows(today, adj, 1e-9)
    # with the focal refined the loss goes on beside the groups
    del seen[:]

    def border_seam(*a, **kw):
        seen.append(sorted(kw))
        kw.pop("max_iterations")
        return ul.bundle_adjust(*a[:6], ul.LOSSES[kw["loss"]], kw["loss_scale"], 3, kw["cam_group"], kw["intr_mask"])

    refined = build_adjusted(tmp_path / "w.db", border_seam, grown=grown_model, refine_focal_length=True, loss="soft_l1", loss_scale=2.0)
    assert seen == [["cam_group", "intr_mask", "loss", "loss_scale", "max_iterations"]]
    assert refined.stats()["bundle_adjustment"]["loss"] == "soft_l1" and "intrinsics" in refined.stats()["bundle_adjustment"]
    for kw in (dict(loss="cauchy"), dict(loss="huber", loss_scale=0.0), dict(loss="huber", loss_scale=float("nan"))):
        with pytest.raises(ValueError, match="trivial, huber, soft_l1"):
            build_adjusted(tmp_path / "w.db", seam, grown=grown_model, **kw)


def test_front_end_names_the_losses_it_refuses():
    from vit_colmap_amd import _lib
    from vit_colmap_amd.mapping import bundle

    problem = ub.random_problem(7)
    for kw in (dict(loss="cauchy"), dict(loss=1), dict(loss="huber", loss_scale=0.0), dict(loss="soft_l1", loss_scale=float("inf")),
               dict(loss="trivial", loss_scale=-1.0), dict(loss="huber", loss_scale=None)):
        with pytest.raises(ValueError, match="trivial, huber, soft_l1"):
            bundle.bundle_adjust(*problem, "cpu", **kw)
    assert bundle.LOSSES == ul.LOSSES == dict(trivial=_lib.VC_BA_LOSS_TRIVIAL, huber=_lib.VC_BA_LOSS_HUBER, soft_l1=_lib.VC_BA_LOSS_SOFT_L1)
    header = open(os.path.join(ROOT, "include", "vitcolmap_hip.h")).read()
    for name, value in (("TRIVIAL", 0), ("HUBER", 1), ("SOFT_L1", 2)):
        assert f"#define VC_BA_LOSS_{name} {value}\n" in header
    # no cameras or no points: the report still says which loss was asked for
    cams, points, report = bundle.bundle_adjust(problem[0], problem[1][:0], problem[2][:1], problem[3][:0], problem[4][:0], problem[5], "cpu",
                                                loss="huber", loss_scale=2.0)
    assert report["loss"] == "huber" and report["loss_scale"] == 2.0 and report["iterations"] == 0


# ---- the configuration and the command line ---------------------------------------------------------------------------------------------
def test_loss_flags_round_trip_and_need_bundle_adjustment(tmp_path, monkeypatch):
    import argparse

    from vit_colmap_amd.pipeline import run_pipeline as rp
    from vit_colmap_amd.utils.config import Config, ReconstructionConfig

    assert (ReconstructionConfig().ba_loss, ReconstructionConfig().ba_loss_scale) == ("trivial", 1.0)
    cfg = Config.from_args(argparse.Namespace(ba_loss="soft_l1", ba_loss_scale=2.5))
    assert (cfg.reconstruction.ba_loss, cfg.reconstruction.ba_loss_scale, cfg.reconstruction.bundle_adjustment) == ("soft_l1", 2.5, False)
    assert Config.from_args(argparse.Namespace()).reconstruction.ba_loss == "trivial"

    def no_extractor(self):
        raise AssertionError("the extractor was built before the flags were checked")

    monkeypatch.setattr(rp.Pipeline, "_make_extractor", no_extractor)

    def config(**kw):
        cfg = Config()
        cfg.reconstruction.sparse_model = True
        cfg.camera.prior_focal_length, cfg.matching.compute_relative_pose, cfg.do_reconstruction = True, True, False
        for k, v in kw.items():
            setattr(cfg.reconstruction, k, v)
        return cfg

    for kw, message in ((dict(ba_loss="huber"), "ba_loss needs .*bundle_adjustment"),
                        (dict(ba_loss="cauchy", bundle_adjustment=True), "unknown ba_loss 'cauchy'.*trivial, huber, soft_l1"),
                        (dict(ba_loss="huber", bundle_adjustment=True, ba_loss_scale=0.0), "ba_loss_scale must be")):
        with pytest.raises(ValueError, match=message):
            rp.Pipeline(config(**kw)).run(tmp_path / "images", tmp_path / "out", tmp_path / "x.db")
    assert not (tmp_path / "out" / "sparse").exists()
    seen = []
    monkeypatch.setattr(rp.Pipeline, "run", lambda self, *a, **k: seen.append((self.config.reconstruction.bundle_adjustment,
                                                                               self.config.reconstruction.ba_loss,
                                                                               self.config.reconstruction.ba_loss_scale)))
    base = ["prog", "--images", "i", "--output", "o", "--db", "d"]
    for extra in ([], ["--sparse-model", "--bundle-adjustment"], ["--sparse-model", "--bundle-adjustment", "--ba-loss", "huber"],
                  ["--sparse-model", "--bundle-adjustment", "--ba-loss", "soft_l1", "--ba-loss-scale", "2"]):
        monkeypatch.setattr(sys, "argv", base + extra)
        rp.main()
    assert seen == [(False, "trivial", 1.0), (True, "trivial", 1.0), (True, "huber", 1.0), (True, "soft_l1", 2.0)]
    monkeypatch.setattr(sys, "argv", base + ["--ba-loss", "cauchy"])
    with pytest.raises(SystemExit):                                  # the parser names the choices
        rp.main()


def test_pipeline_passes_the_loss_to_the_adjustment_and_leaves_it_out_by_default(tmp_path, monkeypatch):
    import vit_colmap_amd.mapping.bundle as bundle
    import vit_colmap_amd.mapping.grow as grow
    from vit_colmap_amd.pipeline import run_pipeline as rp
    from vit_colmap_amd.utils.config import Config

    scene, pairs = windowed()[:2]
    write_scene_db(tmp_path / "w.db", scene, pairs)
    real = grow.build_sparse_model
    monkeypatch.setattr(grow, "build_sparse_model", lambda path, device="cuda": real(path, device="cpu", two_view_pose_fn=spec_two_view_pose,
                                                                                     estimate_fn=spec_estimate, triangulate_fn=spec_triangulate))
    seen = []

    def seam(*a, **kw):
        seen.append(dict(kw))
        return spec_bundle_loss(*a, **kw)

    monkeypatch.setattr(bundle, "bundle_adjust", seam)
    stats = {}
    for name, kw in (("plain", {}), ("huber", dict(loss="huber", loss_scale=1.0))):
        p = rp.Pipeline(Config())
        p.last_stats = {}
        p._write_sparse_model(tmp_path / "w.db", tmp_path / name, "cpu", adjust=True, **kw)
        stats[name] = p.last_stats["bundle_adjustment"]["bundle_adjustment"]
        assert (tmp_path / name / "sparse" / "adjusted" / "images.txt").exists()
    assert seen == [{}, dict(loss="huber", loss_scale=1.0)]
    assert "loss" not in stats["plain"] and stats["huber"]["loss"] == "huber" and stats["huber"]["loss_scale"] == 1.0
    assert sorted(set(stats["huber"]) - set(stats["plain"])) == ["loss", "loss_scale"]
    assert (tmp_path / "plain" / "sparse" / "grown" / "images.txt").read_bytes() == (tmp_path / "huber" / "sparse" / "grown" / "images.txt").read_bytes()
