"""Adjustment per growth round: the growth of mapping/grow.py with two more steps at the end of every
round that added a point or an image, then the tail of mapping/bundle.py.  Past 20 or so views one adjustment at the end of
the growth starts too far from the minimum; one per round keeps every start close.  Specification: tests/util_rounds.py
(`map_model`).  This build's own published rule; parity with COLMAP's mapper is unpinned.  Still missing on the way to a
mapper: no local adjustment, no merging of points, no intrinsics refined inside the rounds; inconsistent components are split
only under `split_tracks` (§4.2n), and their points take no part in registration.

  A-step  one bundle_adjust (mapping/bundle.py) over every registered pose and every point on the current tracks, the gauge of
          build_adjusted_model on the initial pair, BA_MAX_ITERATIONS, poses and points only, under the configured loss, on the
          keypoints the growth uses (with known_distortion the undistorted ones, so the adjustment is the pinhole one)
  E-step  one launch of vc_refine_tracks (mapping/triangulate.py) over every point under the adjusted poses, each over all
          nodes of its component in ascending order (a seed point that lies in no consistent component: over its own track).
          An accepted point takes the new X and its track becomes the inlier nodes: observations that left MAX_ERROR are
          dropped, nodes of the component that are now inside it picked up.  A rejected point is removed; its component goes
          back to the T-step under the growth's rule

Where the work runs
  HIP     the growth's launches; per round the kernels of one bundle adjustment and one launch of vc_refine_tracks
  host    Python / numpy: the arrays of both steps, the tracks, the round reports
"""
import logging

import numpy as np

from .. import _lib
from ..matching.essential import rot_to_quat
from .bundle import HELD_ALL, build_adjusted_model, bundle_adjust, check_loss, check_solver
from .grow import _grow
from .seed import SparseModel

logger = logging.getLogger(__name__)


def _gpu_refine(obs_xy, obs_cam, offsets, cams, init_xyz, device):
    import torch

    from .triangulate import refine_tracks

    xyz, mask, count, error = refine_tracks(*(torch.from_numpy(np.ascontiguousarray(a)).to(device)
                                              for a in (obs_xy, obs_cam, offsets, cams, init_xyz)))
    return xyz.cpu().numpy(), mask.cpu().numpy(), count.cpu().numpy(), error.cpu().numpy()


def _camera_row(R, t, K):
    return np.concatenate([R.reshape(9), t, [K[0, 0], K[1, 1], K[0, 2], K[1, 2]]])


def _round_steps(g, bundle_fn, refine_fn, adjust_args, reports):
    """The A-step and the E-step on the growth's state `g` (mapping/grow.py, `_grow`), which they change in place.  `adjust_args`:
    what the A-step hands to bundle_fn beside the arrays: loss= and loss_scale= where the loss is not "trivial", solver= where it is
    not "dense"; the dense solver's limit on the cameras holds only under it."""
    reg, pids = sorted(g.poses), sorted(g.xyz)
    if adjust_args.get("solver", "dense") == "dense" and len(reg) > _lib.VC_BA_MAX_CAMS:
        raise ValueError(f"adjust_rounds: {len(reg)} registered images, the reduction kernel of the adjustment holds at most "
                         f"{_lib.VC_BA_MAX_CAMS} (VC_BA_MAX_CAMS)")
    # A-step
    rslot = {i: s for s, i in enumerate(reg)}
    cams = np.stack([_camera_row(g.poses[i][0], g.poses[i][1], g.K[i]) for i in reg])
    offsets = np.concatenate([[0], np.cumsum([len(g.tracks[p]) for p in pids])]).astype(np.int32)
    obs_cam = np.array([rslot[i] for p in pids for i, _ in g.tracks[p]], np.int32)
    obs_xy = np.array([g.kps[i][kp] for p in pids for i, kp in g.tracks[p]], np.float64).reshape(-1, 2)
    a, b = (rslot[i] for i in g.initial_pair)
    mask = np.zeros(len(reg), np.uint8)
    mask[a] = HELD_ALL
    mask[b] = 1 << (3 + int(np.argmax(np.abs(cams[b, 9:12]))))
    points = np.array([g.xyz[p] for p in pids], np.float64).reshape(-1, 3)
    cams, points, report = bundle_fn(cams, points, offsets, obs_cam, obs_xy, mask, g.device, **adjust_args)
    cams, points = np.array(cams, np.float64), np.array(points, np.float64)
    for i in reg:
        R = cams[rslot[i], :9].reshape(3, 3).copy()
        g.poses[i] = (R, cams[rslot[i], 9:12].copy(), rot_to_quat(R))
    # E-step
    table = np.full((len(g.ids), 16), np.nan)
    for i in reg:
        table[g.slot[i]] = _camera_row(g.poses[i][0], g.poses[i][1], g.K[i])
    comp_of_point = {pid: c for c, pid in g.point_of.items()}
    nodes_of = [[(int(i), int(kp)) for i, kp in g.comps[comp_of_point[p]]] if p in comp_of_point else list(g.tracks[p]) for p in pids]
    offsets = np.concatenate([[0], np.cumsum([len(ns) for ns in nodes_of])]).astype(np.int32)
    obs = np.array([g.kps[i][kp] for ns in nodes_of for i, kp in ns], np.float64).reshape(-1, 2)
    slots = np.array([g.slot[i] for ns in nodes_of for i, _ in ns], np.int32)
    X, inl, count, _ = refine_fn(obs, slots, offsets, table, points, g.device)
    added = dropped = dropped_points = 0
    for j, p in enumerate(pids):
        if count[j] > 0:
            track = [n for n, m in zip(nodes_of[j], inl[offsets[j]:offsets[j + 1]]) if m]
            before = {(int(i), int(kp)) for i, kp in g.tracks[p]}
            added += len(set(track) - before)
            dropped += len(before - set(track))
            g.xyz[p], g.tracks[p] = np.asarray(X[j], np.float64).copy(), track
        else:
            del g.xyz[p], g.tracks[p]
            if p in comp_of_point:
                del g.point_of[comp_of_point[p]]
            dropped_points += 1
    reports.append(dict(iterations=int(report["iterations"]), accepted_steps=int(report["accepted_steps"]),
                        initial_cost=float(report["initial_cost"]), final_cost=float(report["final_cost"]),
                        decisions=[bool(d) for d in report["decisions"]], added_observations=added, dropped_observations=dropped,
                        dropped_points=dropped_points))
    logger.info("Round adjustment %d: %d linearisations, cost %.6g -> %.6g, %d observations added, %d dropped, %d points dropped",
                len(reports), report["iterations"], report["initial_cost"], report["final_cost"], added, dropped, dropped_points)


def build_mapped_rounds(database_path, device="cuda", two_view_pose_fn=None, estimate_fn=None, triangulate_fn=None, bundle_fn=None,
                        refine_fn=None, loss="trivial", loss_scale=1.0, known_distortion=False, undistort_fn=None, solver="dense",
                        split_tracks=False, split_fn=None, tangential=False):
    """The model as the rounds leave it, before the tail -> (SparseModel, the round reports).  Arguments as build_mapped_model."""
    check_loss(loss, loss_scale)
    check_solver(solver)
    adjust_args = {} if loss == "trivial" else dict(loss=loss, loss_scale=float(loss_scale))
    if solver != "dense":
        adjust_args["solver"] = solver
    bundle_fn, refine_fn, reports = bundle_fn or bundle_adjust, refine_fn or _gpu_refine, []
    split_args = dict(split_tracks=True, split_fn=split_fn) if split_tracks else {}
    if tangential:                                                    # passed on only where it is on, as known_distortion is
        split_args["tangential"] = True
    model = _grow(database_path, device, two_view_pose_fn, estimate_fn, triangulate_fn, known_distortion, undistort_fn,
                  round_fn=lambda g: _round_steps(g, bundle_fn, refine_fn, adjust_args, reports), **split_args)
    return model, reports


def build_mapped_model(database_path, device="cuda", two_view_pose_fn=None, estimate_fn=None, triangulate_fn=None, bundle_fn=None,
                       refine_fn=None, refine_focal_length=False, loss="trivial", loss_scale=1.0, refine_distortion=False,
                       known_distortion=False, undistort_fn=None, solver="dense", split_tracks=False, split_fn=None,
                       tangential=False) -> SparseModel:
    """Read a matched database -> the seed model grown by rounds, adjusted and its tracks re-evaluated after every round that
    added a point or an image (the module's header), then build_adjusted_model's tail on that model with every option given:
    one more adjustment (with refine_focal_length / refine_distortion the one that refines them), the rescale to a unit
    baseline, the filter.  The result's `round_adjustments` are the rounds' reports: dict(iterations, accepted_steps,
    initial_cost, final_cost, decisions, added_observations, dropped_observations (both over the points that stay),
    dropped_points) each.  Raises the seed model's and build_adjusted_model's ValueErrors unchanged, and ValueError above
    VC_BA_MAX_CAMS registered images under the dense solver.  `solver` "pcg" ("The solver" in §4.2k): every adjustment, the
    rounds' and the tail's, solves its system by conjugate gradients and has no such limit; bundle_fn is given solver= only then.
    `refine_fn(obs_xy, obs_cam, offsets, cams, init_xyz, device) -> (xyz, mask, count, error)` on numpy arrays replaces the
    launch of vc_refine_tracks (tests); `bundle_fn` as in build_adjusted_model, in the rounds given loss= and loss_scale= where
    the loss is not "trivial" and nothing else, so the cap is BA_MAX_ITERATIONS; the other seams as in build_sparse_model.
    `split_tracks`, `split_fn` (§4.2n) as in build_sparse_model: the growth splits its inconsistent components; their points are
    adjusted with the others, the E-step evaluates each over its own track, and one it removes frees its slot for the next round.
    `tangential` ("The tangential terms" in §4.2k): OPENCV cameras are mapped; the A-steps run on undistorted keypoints and need
    nothing new, the tail is build_adjusted_model's with the flag."""
    split_args = dict(split_tracks=True, split_fn=split_fn) if split_tracks else {}
    if tangential:
        split_args["tangential"] = True
    model, reports = build_mapped_rounds(database_path, device, two_view_pose_fn, estimate_fn, triangulate_fn, bundle_fn, refine_fn,
                                         loss, loss_scale, known_distortion, undistort_fn, solver, **split_args)
    solver_args = {} if solver == "dense" else dict(solver=solver)
    if tangential:
        solver_args["tangential"] = True
    mapped = build_adjusted_model(database_path, device, bundle_fn=bundle_fn, grown=model, refine_focal_length=refine_focal_length,
                                  loss=loss, loss_scale=loss_scale, refine_distortion=refine_distortion, known_distortion=known_distortion,
                                  **solver_args)
    mapped.round_adjustments = reports
    return mapped
