"""CPU tests of bundle adjustment with radial distortion ("The distortion"): the numpy specification of
tests/util_bundle_radial.py (its Jacobians against central differences, zero distortion against the loop of
tests/util_bundle_intr.py, the recovery of k1 on the distorted windowed scene), the kernels' radial routines compiled for the host
(tools/bundle_host.cpp with the radial section of its problem file) against it, and the front end with the adjustment stubbed:
the masks per camera model, the errors, the params written, the six-number report and the pipeline's flag.  No GPU."""
import argparse
import copy
import sqlite3
import sys
from functools import lru_cache

import numpy as np
import pytest

import util_absolute_pose as ua
import util_bundle as ub
import util_bundle_intr as ui
import util_bundle_loss as ul
import util_bundle_radial as ur
import util_essential as ue
import util_mapper as um
from test_absolute_pose_spec import scene_images, spec_estimate, spec_two_view_pose, truth_pairs, write_scene_db
from test_bundle_intr_spec import grown_runs, tied_groups, windowed_problem, with_focal
from test_bundle_spec import bundle_host  # noqa: F401 - the fixture
from test_mapper_spec import spec_triangulate

# central differences of the specification's own projection against its J_c, J_p and J_theta on 60 observations across the
# 640x480 image with |k1| <= 0.2, |k2| <= 0.05, steps 1e-6 (pose, point, k1, k2) and 1e-3 (fx, fy, cx, cy, in which the pixel is
# linear), measured: worst |difference| / largest entry of the observation's Jacobians 4.63e-10 (the rounding of two pixels
# divided by twice the step, as in tests/test_bundle_spec.py); the bound is 4x, rounded up
FD_STEP, FD_REL_BOUND = 1e-6, 1.9e-9
# zero distortion, k1 and k2 held, against util_bundle_intr's loop on the windowed problem from a focal 3 % off: the decisions,
# the iteration count (6) and the final lambda are identical; the final cost differs by 3.7e-16 relative and the focal by 9.5e-16
# (the radial rule forms J_p and r at fx = fy = 1 first, so each number is rounded differently), measured; the bounds are 4x,
# rounded up
ZERO_COST_REL, ZERO_FOCAL_REL = 1.5e-15, 3.8e-15
# the recovery of k1 = -0.15 from 0 by the specification's chain (grow under k = 0, then the radial loop): measured -0.164739,
# off by 0.0147; with the focal also 3 % off and both freed: k1 -0.166169, off by 0.0162, focal 600.836 for 600 (0.14 %).  The
# bounds are the errors doubled and rounded up, and stay below half of |k1| = 0.075.
K1_BOUND, K1_BOUND_BOTH, FOCAL_REL_BOUND_BOTH = 0.03, 0.033, 0.0028


@lru_cache(maxsize=None)
def distorted(k2=0.0, focal=1.0):
    """The distorted windowed scene, grown under k = 0 (and a focal `focal` times the truth) by the specification -> scene,
    images, grown, the arrays of its adjustment (cams, points, offsets, obs_cam, obs_xy, const_mask)."""
    scene = ur.distorted_windowed_scene(ur.K1_TRUE, k2)
    if focal != 1.0:
        K = scene["K"].copy()
        K[0, 0], K[1, 1] = K[0, 0] * focal, K[1, 1] * focal
        scene = dict(scene, K=K)
    images = scene_images(scene)
    grown = um.grow_model(images, truth_pairs(scene))
    ids, cams, points, offsets, obs_cam, obs_xy = ub.model_problem(images, grown)
    a, b = (ids.index(i) for i in grown["initial_pair"])
    return scene, images, grown, (cams, points, offsets, obs_cam, obs_xy, ub.gauge_mask(cams, a, b))


def one_group(n_cams, mask):
    return np.zeros(n_cams, np.int32), np.array([mask], np.uint8)


K1_FREE = ui.HOLD_ALL | ur.HOLD_K2                                    # what refine_distortion gives a SIMPLE_RADIAL camera
K1_AND_FOCAL_FREE = ui.TIED | ui.HOLD_PRINCIPAL | ur.HOLD_K2          # with refine_focal_length too


@lru_cache(maxsize=None)
def recovered():
    """The specification's radial loop on the distorted problem: k1 free; k1 and the focal free from a focal 3 % off."""
    problem = distorted()[3]
    wrong = distorted(focal=1.03)[3]
    n = len(problem[0])
    return dict(k1=ur.bundle_adjust(problem[0], np.zeros((n, 2)), *problem[1:], *one_group(n, K1_FREE), max_iterations=500),
                held=ub.bundle_adjust(*problem),
                both=ur.bundle_adjust(wrong[0], np.zeros((n, 2)), *wrong[1:], *one_group(n, K1_AND_FOCAL_FREE), max_iterations=500))


# ---- the specification ---------------------------------------------------------------------------------------------------------------
def random_observation(i):
    """A camera of the arc, a pixel anywhere in the 640x480 image, a depth, |k1| <= 0.2, |k2| <= 0.05 -> row, dist, X, uv."""
    rs = np.random.RandomState(36000 + i)
    R, t = um.arc_cameras()[int(rs.randint(12))]
    row = um.camera_row(R, t, ue.SCENE_K)
    z = rs.uniform(5.0, 11.0)
    Xc = np.array([(rs.uniform(0, 640) - 320.0) / 600.0 * z, (rs.uniform(0, 480) - 240.0) / 600.0 * z, z])
    dist = np.array([rs.uniform(-0.2, 0.2), rs.uniform(-0.05, 0.05)])
    X = R.T @ (Xc - t)
    return row, dist, X, ur.project(row, dist, X) + rs.normal(0, 0.5, 2)


def test_jacobians_match_central_differences_of_the_projection():
    worst = 0.0
    for i in range(60):
        row, dist, X, uv = random_observation(i)
        usable, r, Jc, Jp, jt = ur.observe(row, dist, X, uv)
        Jt = ur.jtheta(jt, 0)
        assert usable and np.abs(r - (ur.project(row, dist, X) - uv)).max() <= 1e-10

        def pixel(w=np.zeros(3), dt=np.zeros(3), dX=np.zeros(3), dth=np.zeros(6)):
            moved = row.copy()
            moved[:9] = (ua.rodrigues(np.asarray(w, np.float64)) @ row[:9].reshape(3, 3)).reshape(9)
            moved[9:12] = row[9:12] + dt
            moved[12:16] = row[12:16] + dth[:4]
            return ur.project(moved, dist + dth[4:], X + dX)

        num_c, num_p, num_t = np.zeros((2, 6)), np.zeros((2, 3)), np.zeros((2, 6))
        for k in range(6):
            e = np.zeros(6)
            e[k] = FD_STEP
            num_c[:, k] = (pixel(w=e[:3], dt=e[3:]) - pixel(w=-e[:3], dt=-e[3:])) / (2 * FD_STEP)
            h = 1e-3 if k < 4 else FD_STEP
            e[k] = h
            num_t[:, k] = (pixel(dth=e) - pixel(dth=-e)) / (2 * h)
        for k in range(3):
            e = np.zeros(3)
            e[k] = FD_STEP
            num_p[:, k] = (pixel(dX=e) - pixel(dX=-e)) / (2 * FD_STEP)
        scale = max(np.abs(Jc).max(), np.abs(Jp).max(), np.abs(Jt).max())
        diff = max(np.abs(num_c - Jc).max(), np.abs(num_p - Jp).max(), np.abs(num_t - Jt).max())
        worst = max(worst, diff / scale)
        assert diff <= FD_REL_BOUND * scale, (i, diff, scale)
        # the masks: a held column is zero, a tied group has (xd, yd) in column 0 and nothing in column 1
        held = ur.jtheta(jt, ui.HOLD_CX | ur.HOLD_K2)
        assert not held[:, [2, 5]].any() and np.array_equal(held[:, [0, 1, 3, 4]], Jt[:, [0, 1, 3, 4]])
        tied = ur.jtheta(jt, ui.TIED | ur.HOLD_K1)
        assert np.array_equal(tied[:, 0], jt[:2]) and not tied[:, [1, 4]].any() and np.array_equal(tied[:, 5], Jt[:, 5])
    print(f"worst relative difference to central differences {worst:.3g}")


def test_zero_distortion_held_follows_the_loop_without_it_from_a_wrong_focal():
    problem = with_focal(windowed_problem(), 1.03)
    n = len(problem[0])
    cam_group, intr_mask = tied_groups(n)
    cams, dist, points, report = ur.bundle_adjust(problem[0], np.zeros((n, 2)), *problem[1:], cam_group, intr_mask | ur.HOLD_DIST,
                                                  max_iterations=ub.BA_MAX_ITERATIONS)
    ref_cams, _, ref = grown_runs()["refined"]
    rel = abs(report["final_cost"] - ref["final_cost"]) / ref["final_cost"]
    rel_f = abs(cams[0, 12] - ref_cams[0, 12]) / ref_cams[0, 12]
    print(f"{report['iterations']} linearisations, final cost {report['final_cost']:.12g} (without the distortion {ref['final_cost']:.12g}, "
          f"relative difference {rel:.3g}), focal {cams[0, 12]:.9f} ({ref_cams[0, 12]:.9f}, relative difference {rel_f:.3g})")
    assert report["decisions"] == ref["decisions"] and report["iterations"] == ref["iterations"]
    assert report["accepted_steps"] == ref["accepted_steps"] and report["final_lambda"] == ref["final_lambda"]
    assert rel <= ZERO_COST_REL and rel_f <= ZERO_FOCAL_REL
    assert not dist.any() and np.array_equal(report["intrinsics"]["after"][:, 4:], np.zeros((1, 2)))
    assert report["intrinsics"]["before"].shape == (1, 6) and np.array_equal(report["intrinsics"]["after"][0, :4], cams[0, 12:])


def test_the_chain_recovers_k1_from_zero_on_the_distorted_scene():
    """The test of the specification that fails without the feature: the grown model of the distorted scene, adjusted with k
    held at 0, keeps a cost that the freed k1 lowers, and the freed k1 ends within K1_BOUND of the truth."""
    scene, _, grown, problem = distorted()
    assert sorted(grown["poses"]) == list(range(1, 13))               # a condition on the input: k = 0 still registers every image
    assert sorted(distorted(focal=1.03)[2]["poses"]) == list(range(1, 13))
    # the regime: the outermost true keypoints move by a few pixels
    moved = max(np.abs(kp[seen].astype(np.float64) - plain[seen]).max()
                for kp, plain, seen in zip(scene["keypoints"], um.windowed_scene()["keypoints"], scene["visible"]))
    assert 1.0 <= moved <= 5.0, moved
    runs = recovered()
    k1 = runs["k1"][1][0, 0]
    print(f"k1 {k1:.6f} for {ur.K1_TRUE} (off by {abs(k1 - ur.K1_TRUE):.4f}) in {runs['k1'][3]['iterations']} linearisations, cost "
          f"{runs['k1'][3]['final_cost']:.4f} (k held at 0: {runs['held'][2]['final_cost']:.4f}); largest displacement {moved:.2f} px")
    assert K1_BOUND <= 0.5 * abs(ur.K1_TRUE) and abs(k1 - ur.K1_TRUE) <= K1_BOUND
    assert (runs["k1"][1][:, 0] == k1).all() and not runs["k1"][1][:, 1].any()                                   # one group, k2 held
    assert np.array_equal(runs["k1"][0][:, 12:], problem[0][:, 12:])                                      # fx, fy, cx, cy held
    assert runs["k1"][3]["final_cost"] < runs["held"][2]["final_cost"] and runs["k1"][3]["iterations"] < 500
    cams, dist, _, report = runs["both"]
    f = scene["K"][0, 0]
    print(f"both: k1 {dist[0, 0]:.6f} (off by {abs(dist[0, 0] - ur.K1_TRUE):.4f}), focal {cams[0, 12]:.4f} for {f} from {1.03 * f} "
          f"({abs(cams[0, 12] - f) / f:.3%} off) in {report['iterations']} linearisations")
    assert K1_BOUND_BOTH <= 0.5 * abs(ur.K1_TRUE) and abs(dist[0, 0] - ur.K1_TRUE) <= K1_BOUND_BOTH
    assert abs(cams[0, 12] - f) / f <= FOCAL_REL_BOUND_BOTH and np.array_equal(cams[:, 12], cams[:, 13])


# ---- the kernels' routines on the host ---------------------------------------------------------------------------------------------------
def spec_arrays(problem, groups, s):
    """ur.one_pass's dict in the host program's layout."""
    n, G = len(problem[1]), len(groups[1])
    lin, li = s["lin"], s["li"]
    terms = np.concatenate([li["q"].reshape(n, -1), li["hq"].reshape(n, -1), li["p"].reshape(n, -1), li["P"].reshape(n, -1)], axis=1).T
    return dict(vinv=lin["vinv"].reshape(-1, 9)[:, [0, 1, 2, 4, 5, 8]], gp=lin["gp"], cost=lin["cost"], S=s["S"], g=s["g"], obs_w=lin["sw"],
                jt=lin["jt"], T=li["T"].reshape(n, G, 18), terms=terms, sums=ui._ordered(terms.T), B=s["B"], C=s["C"], h=s["h"], cams=s["cams"],
                points=s["points"], dx=s["dx"], dist=s["dist"])


def host_cases():
    """The distorted windowed problem with k1 free from 0, 100 random problems and the nine edge problems under random groups,
    masks and distortion -> [(name, problem, dist, groups)]."""
    problem = distorted()[3]
    n = len(problem[0])
    cases = [("windowed", problem, np.zeros((n, 2)), one_group(n, K1_FREE))]
    for i in range(100):
        p = ub.random_problem(i)
        groups, dist = ur.random_groups(i, len(p[0]))
        cases.append((f"random {i}", p, dist, groups))
    for k, (name, p) in enumerate(sorted(ub.edge_problems().items())):
        groups, dist = ur.random_groups(200 + k, len(p[0]))
        cases.append((name, p, dist, groups))
    return cases


def test_host_build_matches_the_spec_on_radial_problem_files(bundle_host, tmp_path):  # noqa: F811
    worst = {}
    for name, problem, dist, groups in host_cases():
        for loss, scale in ((ul.TRIVIAL, 1.0), (ul.HUBER, 1.0)):
            s = ur.one_pass(problem, dist, groups, loss=loss, loss_scale=scale)
            host, stderr = ur.run_host(bundle_host, tmp_path, problem, dist, ub.BA_LAMBDA0, s["dc"], groups, s["dtheta"], loss, scale)
            what = (name, loss)
            assert np.array_equal(host["plain"]["obs_ok"].astype(bool), s["lin"]["ok"]) and np.array_equal(host["plain"]["count"], s["lin"]["count"]), what
            assert np.array_equal(host["free"].astype(bool), s["free"]) and np.array_equal(host["valid"].astype(bool), s["valid"]), what
            for k, v in spec_arrays(problem, groups, s).items():
                got = host["plain"][k] if k in host["plain"] and k not in ("cams", "points", "dx") else host[k]
                assert np.array_equal(np.isfinite(got), np.isfinite(v)), (what, k)
                scale_k = np.abs(v[np.isfinite(v)]).max(initial=0.0)
                diff = np.abs(np.where(np.isfinite(v), got - v, 0.0)).max(initial=0.0)
                rel = diff / scale_k if scale_k else float(diff != 0) * np.inf
                if rel > worst.get(k, (-1.0, ""))[0]:
                    worst[k] = (rel, what)
    print("worst relative differences host - spec: " + ", ".join(f"{k} {v:.3g} {what}" for k, (v, what) in sorted(worst.items())))
    for k in ("jt", "obs_w", "cost", "dist"):                        # what depends on the projection and the loss alone: the kernel's order
        assert worst[k][0] == 0.0, k
    assert ur.TOL_REL == ul.TOL_REL and max(v for v, _ in worst.values()) <= ur.TOL_REL      # the tolerance of the loss tests' pass


def test_host_build_refuses_more_groups_than_the_radial_limit(bundle_host, tmp_path):  # noqa: F811
    import subprocess

    problem = ub.random_problem(7)
    n = len(problem[0])
    groups = (np.zeros(n, np.int32), np.zeros(ur.MAX_GROUPS + 1, np.uint8))
    ur.write_problem_file(tmp_path / "many.bin", problem, np.zeros((n, 2)), ub.BA_LAMBDA0, np.zeros(6 * n), groups, np.zeros(6 * (ur.MAX_GROUPS + 1)))
    done = subprocess.run([bundle_host, str(tmp_path / "many.bin"), str(tmp_path / "many_result.bin")], stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, text=True)
    assert done.returncode == 3 and "VC_BA_MAX_GROUPS_RADIAL" in done.stderr and not (tmp_path / "many_result.bin").exists()


# ---- the front end with the adjustment stubbed -------------------------------------------------------------------------------------------
def spec_bundle_radial(cams, points, offsets, obs_cam, obs_xy, const_mask, device, cam_group=None, intr_mask=None, max_iterations=None,
                       cam_dist=None, loss="trivial", loss_scale=1.0):
    """The specification behind the front end's seam when it is given cam_dist."""
    cams, dist, points, report = ur.bundle_adjust(cams, cam_dist, points, offsets, obs_cam, obs_xy, const_mask, cam_group, intr_mask,
                                                  ul.LOSSES[loss], loss_scale, max_iterations)
    return cams, points, dict(report, cam_dist=dist)


def set_camera_model(path, model, params):
    """The database's one camera rewritten as `model` (SIMPLE_RADIAL: 2, RADIAL: 3) with `params`."""
    with sqlite3.connect(str(path)) as db:
        db.execute("UPDATE cameras SET model = ?, params = ?", ({"SIMPLE_RADIAL": 2, "RADIAL": 3}[model], np.asarray(params, np.float64).tobytes()))


@pytest.fixture(scope="module")
def radial_db(tmp_path_factory):
    """The distorted scene as a SIMPLE_RADIAL database with k = 0 and the truth's pairs, and its grown model (the specification in
    every seam)."""
    from vit_colmap_amd.mapping.grow import build_sparse_model

    directory = tmp_path_factory.mktemp("bundle_radial")
    scene = distorted()[0]
    K = scene["K"]
    write_scene_db(directory / "r.db", scene, truth_pairs(scene))
    set_camera_model(directory / "r.db", "SIMPLE_RADIAL", [K[0, 0], K[0, 2], K[1, 2], 0.0])
    grown = build_sparse_model(directory / "r.db", device="cpu", two_view_pose_fn=spec_two_view_pose, estimate_fn=spec_estimate,
                               triangulate_fn=spec_triangulate)
    return directory / "r.db", grown


def stub(seen, k=(0.011, 0.022)):
    """A bundle_fn that moves nothing but the free k of every group to `k` and says what it was given."""
    def bundle_fn(cams, points, offsets, obs_cam, obs_xy, const_mask, device, **kw):
        seen.clear()
        seen.update(kw)
        report = dict(iterations=1, accepted_steps=0, initial_cost=1.0, final_cost=1.0, final_lambda=1e-4, decisions=[])
        if "cam_dist" in kw:
            G = len(kw["intr_mask"])
            first = [int(np.nonzero(kw["cam_group"] == g)[0][0]) for g in range(G)]
            before = np.array([np.concatenate([cams[a, 12:16], kw["cam_dist"][a]]) for a in first])
            after = before.copy()
            for g, m in enumerate(kw["intr_mask"]):
                after[g, 4] = after[g, 4] if int(m) & ur.HOLD_K1 else k[0]
                after[g, 5] = after[g, 5] if int(m) & ur.HOLD_K2 else k[1]
            report.update(intrinsics=dict(before=before, after=after), cam_dist=after[kw["cam_group"], 4:])
        elif "cam_group" in kw:
            report.update(intrinsics=dict(before=ui.group_intrinsics(cams, kw["cam_group"], len(kw["intr_mask"])),
                                          after=ui.group_intrinsics(cams, kw["cam_group"], len(kw["intr_mask"]))))
        return cams, points, report
    return bundle_fn


def test_build_adjusted_model_masks_params_and_report_per_camera_model(radial_db, caplog):
    from vit_colmap_amd.mapping import bundle_intr
    from vit_colmap_amd.mapping.bundle import build_adjusted_model

    path, grown = radial_db
    (cid, cam), = grown.cameras.items()
    f, cx, cy = (float(v) for v in cam.params[:3])
    assert cam.model == "SIMPLE_RADIAL" and list(cam.params) == [f, cx, cy, 0.0] and sorted(grown.images) == list(range(1, 13))
    seen = {}
    # SIMPLE_RADIAL frees k1 alone; the focal and the principal point are held
    model = build_adjusted_model(path, device="cpu", bundle_fn=stub(seen), grown=grown, refine_distortion=True)
    assert list(seen["intr_mask"]) == [K1_FREE] and not seen["cam_group"].any() and len(seen["cam_group"]) == 12
    assert seen["cam_dist"].shape == (12, 2) and not seen["cam_dist"].any() and seen["max_iterations"] == bundle_intr.REFINE_MAX_ITERATIONS
    assert "loss" not in seen and list(model.cameras[cid].params) == [f, cx, cy, 0.011] and grown.cameras[cid].params[3] == 0.0
    report = model.stats()["bundle_adjustment"]
    assert report["intrinsics"] == {cid: dict(before=[f, f, cx, cy, 0.0, 0.0], after=[f, f, cx, cy, 0.011, 0.0])} and "cam_dist" not in report
    # with refine_focal_length too: the tied focal is free as well; the loss is passed on
    build_adjusted_model(path, device="cpu", bundle_fn=stub(seen), grown=grown, refine_distortion=True, refine_focal_length=True, loss="huber",
                         loss_scale=2.0)
    assert list(seen["intr_mask"]) == [K1_AND_FOCAL_FREE] and seen["loss"] == "huber" and seen["loss_scale"] == 2.0
    # RADIAL frees both and starts from what the camera carries
    radial = copy.deepcopy(grown)
    radial.cameras[cid].model, radial.cameras[cid].params = "RADIAL", [f, cx, cy, 0.004, -0.002]
    model = build_adjusted_model(path, device="cpu", bundle_fn=stub(seen), grown=radial, refine_distortion=True)
    assert list(seen["intr_mask"]) == [ui.HOLD_ALL] and np.array_equal(seen["cam_dist"], np.tile([0.004, -0.002], (12, 1)))
    assert list(model.cameras[cid].params) == [f, cx, cy, 0.011, 0.022]
    assert model.stats()["bundle_adjustment"]["intrinsics"][cid] == dict(before=[f, f, cx, cy, 0.004, -0.002], after=[f, f, cx, cy, 0.011, 0.022])
    # a second camera of another model keeps both held, which is said once; the first is still refined
    two = copy.deepcopy(grown)
    two.cameras[cid + 1] = copy.deepcopy(cam)
    two.cameras[cid + 1].model, two.cameras[cid + 1].params = "PINHOLE", [f, f, cx, cy]
    two.images[12]["camera_id"] = cid + 1
    with caplog.at_level("INFO", logger="vit_colmap_amd.mapping.bundle"):
        model = build_adjusted_model(path, device="cpu", bundle_fn=stub(seen), grown=two, refine_distortion=True, refine_focal_length=True)
    assert list(seen["intr_mask"]) == [K1_AND_FOCAL_FREE, ui.HOLD_PRINCIPAL | ur.HOLD_DIST] and list(seen["cam_group"]) == [0] * 11 + [1]
    assert sum("has no radial parameter" in r.getMessage() for r in caplog.records) == 1
    assert list(model.cameras[cid + 1].params) == [f, f, cx, cy] and model.cameras[cid].params[3] == 0.011
    assert len(model.stats()["bundle_adjustment"]["intrinsics"][cid + 1]["after"]) == 6
    # no camera with a radial parameter: the error names the two models
    none = copy.deepcopy(grown)
    none.cameras[cid].model, none.cameras[cid].params = "PINHOLE", [f, f, cx, cy]
    with pytest.raises(ValueError, match="SIMPLE_RADIAL.*RADIAL"):
        build_adjusted_model(path, device="cpu", bundle_fn=stub(seen), grown=none, refine_distortion=True)
    # more cameras than the radial border holds: the error names the limit
    many = copy.deepcopy(grown)
    for k, i in enumerate(sorted(many.images)[:ur.MAX_GROUPS + 1]):
        many.images[i]["camera_id"] = 100 + k
        many.cameras[100 + k] = copy.deepcopy(cam)
    with pytest.raises(ValueError, match="VC_BA_MAX_GROUPS_RADIAL"):
        build_adjusted_model(path, device="cpu", bundle_fn=stub(seen), grown=many, refine_distortion=True)
    # without the flag the seam sees today's call and the report today's keys
    plain = build_adjusted_model(path, device="cpu", bundle_fn=stub(seen), grown=grown)
    assert seen == {} and "intrinsics" not in plain.stats()["bundle_adjustment"] and plain.cameras == grown.cameras
    build_adjusted_model(path, device="cpu", bundle_fn=stub(seen), grown=grown, refine_focal_length=True)
    assert sorted(seen) == ["cam_group", "intr_mask", "max_iterations"] and list(seen["intr_mask"]) == [ui.TIED | ui.HOLD_PRINCIPAL]


def test_build_adjusted_model_with_the_spec_in_its_seam_writes_the_recovered_k1(radial_db, tmp_path):
    from vit_colmap_amd.mapping.bundle import build_adjusted_model
    from vit_colmap_amd.mapping.seed import SparseModel

    path, grown = radial_db
    (cid, cam), = grown.cameras.items()
    held = build_adjusted_model(path, device="cpu", bundle_fn=lambda *a, **kw: ub.bundle_adjust(*a[:6]), grown=grown)
    model = build_adjusted_model(path, device="cpu", bundle_fn=spec_bundle_radial, grown=grown, refine_distortion=True)
    k1 = float(model.cameras[cid].params[3])
    print(f"written k1 {k1:.6f} for {ur.K1_TRUE}, cost {model.bundle_adjustment['final_cost']:.4f} (held {held.bundle_adjustment['final_cost']:.4f}), "
          f"{len(model.points3D)} points (held {len(held.points3D)})")
    assert abs(k1 - ur.K1_TRUE) <= K1_BOUND and list(model.cameras[cid].params[:3]) == list(cam.params[:3])
    assert model.bundle_adjustment["final_cost"] < held.bundle_adjustment["final_cost"]
    assert all(p["error"] <= ub.MAX_ERROR and len(p["track"]) >= 2 for p in model.points3D.values())
    # the filter and `error` use the distorted projection: under it the kept points' mean error is lower than under k = 0
    assert np.mean([p["error"] for p in model.points3D.values()]) < np.mean([p["error"] for p in held.points3D.values()])
    model.write_text(tmp_path / "adjusted")
    assert SparseModel.read_text(tmp_path / "adjusted") == model


def test_refine_distortion_flag_is_off_by_default_and_needs_bundle_adjustment(tmp_path, monkeypatch):
    from vit_colmap_amd.pipeline import run_pipeline as rp
    from vit_colmap_amd.utils.config import Config, ReconstructionConfig

    assert ReconstructionConfig().refine_distortion is False and Config().reconstruction.refine_distortion is False
    assert Config.from_args(argparse.Namespace(refine_distortion=True)).reconstruction.refine_distortion is True
    assert Config.from_args(argparse.Namespace(refine_distortion=True)).reconstruction.bundle_adjustment is False
    assert Config.from_args(argparse.Namespace()).reconstruction.refine_distortion is False

    def no_extractor(self):
        raise AssertionError("the extractor was built before the flags were checked")

    monkeypatch.setattr(rp.Pipeline, "_make_extractor", no_extractor)
    cfg = Config()
    cfg.reconstruction.refine_distortion, cfg.reconstruction.sparse_model = True, True
    cfg.camera.prior_focal_length, cfg.matching.compute_relative_pose, cfg.do_reconstruction = True, True, False
    with pytest.raises(ValueError, match="refine_distortion needs .*bundle_adjustment"):
        rp.Pipeline(cfg).run(tmp_path / "images", tmp_path / "out", tmp_path / "x.db")
    seen = []
    monkeypatch.setattr(rp.Pipeline, "run", lambda self, *a, **k: seen.append((self.config.reconstruction.bundle_adjustment,
                                                                               self.config.reconstruction.refine_focal_length,
                                                                               self.config.reconstruction.refine_distortion,
                                                                               self.config.reconstruction.ba_loss)))
    base = ["prog", "--images", "i", "--output", "o", "--db", "d", "--sparse-model", "--bundle-adjustment"]
    for extra in ([], ["--refine-distortion"], ["--refine-distortion", "--refine-focal-length", "--ba-loss", "huber"]):
        monkeypatch.setattr(sys, "argv", base + extra)
        rp.main()
    assert seen == [(True, False, False, "trivial"), (True, False, True, "trivial"), (True, True, True, "huber")]


def test_pipeline_passes_the_flag_and_changes_only_the_distortion_field(radial_db, tmp_path, monkeypatch):
    import vit_colmap_amd.mapping.bundle as bundle
    import vit_colmap_amd.mapping.grow as grow
    from vit_colmap_amd.pipeline import run_pipeline as rp
    from vit_colmap_amd.utils.config import Config

    path, _ = radial_db
    real = grow.build_sparse_model
    monkeypatch.setattr(grow, "build_sparse_model", lambda p, device="cuda": real(p, device="cpu", two_view_pose_fn=spec_two_view_pose,
                                                                                  estimate_fn=spec_estimate, triangulate_fn=spec_triangulate))
    seen = {}
    monkeypatch.setattr(bundle, "bundle_adjust", stub(seen))
    p = rp.Pipeline(Config())
    p.last_stats = {}
    p._write_sparse_model(path, tmp_path / "out", "cpu", adjust=True, refine_distortion=True, loss="soft_l1", loss_scale=1.5)
    assert list(seen["intr_mask"]) == [K1_FREE] and seen["loss"] == "soft_l1" and seen["loss_scale"] == 1.5
    a, b = ((tmp_path / "out" / "sparse" / m / "cameras.txt").read_text().splitlines() for m in ("grown", "adjusted"))
    differing = [(x.split(), y.split()) for x, y in zip(a, b) if x != y]
    assert len(a) == len(b) and len(differing) == 1
    wx, wy = differing[0]                                              # id, SIMPLE_RADIAL, width, height, f, cx, cy, k
    assert wx[1] == "SIMPLE_RADIAL" and wx[:7] == wy[:7] and float(wx[7]) == 0.0 and float(wy[7]) == 0.011
    assert len(p.last_stats["bundle_adjustment"]["bundle_adjustment"]["intrinsics"][int(wy[0])]["after"]) == 6
