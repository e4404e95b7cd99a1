"""An unknown focal length from the verified pairs: for a camera that is the same in both images of a
pair, K' F K must be an essential matrix, with two equal singular values; the scale r on the stored focal length(s) that
makes it most nearly so over all UNCALIBRATED pairs of the camera is the estimate (the self-calibration cost of Mendonça and
Cipolla).  The option is `camera.estimate_focal_length` (--estimate-focal-length), off by default.  Specification:
tests/util_focal.py.  This is the build's own published rule: parity with COLMAP is unpinned.

Where the work runs
  HIP     the cost of every pair under every candidate of a grid level and its sums per camera, one call per level
          (csrc/focal.hip, vc_focal_cost, whose header states the rule)
  host    which pairs count, the grid levels, the parabola through the last level's minimum, the cameras table
"""
import dataclasses
import logging

import numpy as np

from ._common import CONFIG_UNCALIBRATED
from .essential import camera_prior

logger = logging.getLogger(__name__)

FOCAL_MIN_PAIRS = 3
GRID_STEPS = 64                      # 65 candidates per level
GRID_LEVELS = 4                      # level 0 and three refinements
GRID_LO, GRID_SPAN = 0.25, 16.0      # level 0: r_k = 0.25 * 16^(k / 64), from a quarter to four times the stored focal


def focal_cost(F, pair_cam, w, cams, ratios):
    """F float64 (n_pairs, 9), pair_cam int32 (n_pairs,), w float64 (n_pairs,), cams float64 (n_cams, 4) = (fx0, fy0, cx, cy),
    ratios float64 (n_cand,), all on one GPU -> out_cost float64 (n_cams, n_cand), out_weight float64 (n_cams,)."""
    import torch

    from .. import _lib

    if not (F.is_cuda and F.dtype == torch.float64 and pair_cam.dtype == torch.int32 and w.dtype == torch.float64
            and cams.dtype == torch.float64 and ratios.dtype == torch.float64):
        raise ValueError("focal_cost needs float64 F, weights, cameras and ratios and int32 slots on the GPU")
    if any(t.device != F.device for t in (pair_cam, w, cams, ratios)):
        raise ValueError("focal_cost needs every tensor on the same GPU")
    n = int(pair_cam.shape[0])
    if F.shape != (n, 9) or w.shape != (n,) or cams.dim() != 2 or cams.shape[1] != 4 or ratios.dim() != 1:
        raise ValueError("focal_cost needs F (n, 9), pair_cam (n,), w (n,), cams (n_cams, 4), ratios (n_cand,)")
    n_cams, n_cand = int(cams.shape[0]), int(ratios.shape[0])
    cost = torch.full((n_cams, n_cand), float("nan"), dtype=torch.float64, device=F.device)
    weight = torch.zeros((n_cams,), dtype=torch.float64, device=F.device)
    if n == 0 or n_cand == 0 or n_cams == 0:
        return cost, weight
    F, pair_cam, w, cams, ratios = (t.contiguous() for t in (F, pair_cam, w, cams, ratios))
    _lib.check(_lib.load().vc_focal_cost(_lib.ptr(F), _lib.ptr(pair_cam), _lib.ptr(w), n, _lib.ptr(cams), n_cams, _lib.ptr(ratios),
                                         n_cand, _lib.ptr(cost), _lib.ptr(weight), _lib.stream_ptr()), "vc_focal_cost")
    return cost, weight


def gpu_focal_cost(F, pair_cam, w, cams, ratios, device="cuda"):
    """focal_cost on numpy arrays -> out_cost (n_cams, n_cand), out_weight (n_cams,): the default of the `cost_fn` seam."""
    import torch

    cost, weight = focal_cost(*(torch.from_numpy(np.ascontiguousarray(a, t)).to(device) for a, t in
                                ((np.asarray(F, np.float64).reshape(-1, 9), np.float64), (pair_cam, np.int32), (w, np.float64),
                                 (np.asarray(cams, np.float64).reshape(-1, 4), np.float64), (ratios, np.float64))))
    return cost.cpu().numpy(), weight.cpu().numpy()


def plain_camera(camera):
    """A Camera row -> (fx0, fy0, cx, cy) float64 (4,), or None where essential.camera_prior would not call it plain (an unknown
    model, a non-zero distortion parameter, a focal that is not positive and finite)."""
    K, plain, _ = camera_prior(dataclasses.replace(camera, has_prior_focal_length=True))
    return np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]]) if plain else None


def camera_pairs(db, ids):
    """The rows the estimate reads -> {camera_id: (F float64 (n, 9), w float64 (n,))} for every camera of the images `ids` (None:
    no row): the UNCALIBRATED rows, ascending in pair_id, whose two images are among `ids` and use that camera."""
    image_camera = {im.image_id: im.camera_id for im in db.read_all_images()}
    wanted = {i for i in ids if i is not None}
    rows = {image_camera[i]: ([], []) for i in wanted if i in image_camera}
    for i, j, n_inliers, config in db.read_two_view_geometry_pairs():
        if config != CONFIG_UNCALIBRATED or i not in wanted or j not in wanted:
            continue
        c = image_camera.get(i)
        if c is None or c != image_camera.get(j):
            continue
        rows[c][0].append(db.read_two_view_geometry(i, j)["F"].reshape(9))
        rows[c][1].append(float(n_inliers))
    return {c: (np.array(F, np.float64).reshape(-1, 9), np.array(w, np.float64)) for c, (F, w) in rows.items()}


def level0():
    return GRID_LO * np.power(GRID_SPAN, np.arange(GRID_STEPS + 1) / GRID_STEPS)


def refine_level(lo, hi):
    """65 log-spaced candidates from lo to hi."""
    return lo * np.power(hi / lo, np.arange(GRID_STEPS + 1) / GRID_STEPS)


def estimate_camera(F, w, cam, device="cuda", cost_fn=None):
    """The pairs of one camera, cam = (fx0, fy0, cx, cy) -> dict(ratio, pairs, weight, cost_min, cost_median, reason); `ratio`
    is None where `reason` says why there is no estimate."""
    cost_fn = cost_fn or gpu_focal_cost
    F, w = np.asarray(F, np.float64).reshape(-1, 9), np.asarray(w, np.float64).reshape(-1)
    counts = np.isfinite(w) & (w > 0) & np.isfinite(F).all(axis=1) & F.any(axis=1)
    out = dict(ratio=None, pairs=int(counts.sum()), weight=0.0, cost_min=None, cost_median=None, reason=None)
    if not counts.any():
        return dict(out, reason="no weight: no UNCALIBRATED pair of this camera has inliers and a finite F")
    slots, cams = np.zeros(len(F), np.int32), np.asarray(cam, np.float64).reshape(1, 4)
    r = level0()
    J, W = cost_fn(F, slots, w, cams, r, device)
    J, out["weight"] = np.asarray(J, np.float64)[0], float(np.asarray(W)[0])
    if not out["weight"] > 0 or not np.isfinite(J).all():
        return dict(out, reason="no weight: no UNCALIBRATED pair of this camera has inliers and a finite F")
    if out["pairs"] < FOCAL_MIN_PAIRS:
        return dict(out, reason=f"{out['pairs']} pairs, fewer than {FOCAL_MIN_PAIRS}")
    m = int(np.argmin(J))
    out["cost_median"] = float(np.median(J))
    if m == 0 or m == GRID_STEPS:
        return dict(out, cost_min=float(J[m]), reason=f"the minimum is on the edge of the grid (r = {r[m]:g})")
    for _ in range(1, GRID_LEVELS):
        r = refine_level(r[max(m - 1, 0)], r[min(m + 1, GRID_STEPS)])
        J = np.asarray(cost_fn(F, slots, w, cams, r, device)[0], np.float64)[0]
        m = int(np.argmin(J))
    x = np.log(r)
    best = x[m]
    if 0 < m < GRID_STEPS:                                     # the vertex of the parabola through the minimum and its neighbours
        h = 0.5 * (x[m + 1] - x[m - 1])
        den = J[m - 1] - 2.0 * J[m] + J[m + 1]
        if den > 0:
            best = x[m] + 0.5 * h * (J[m - 1] - J[m + 1]) / den
    return dict(out, ratio=float(np.exp(best)), cost_min=float(J[m]))


def estimate_focal_lengths(db, ids, device="cuda", cost_fn=None):
    """The cameras of the images `ids` of an open database -> {camera_id: dict(ratio, focal, pairs, weight, cost_min, cost_median,
    reason)}.  `focal` is one number for a model with one focal length (SIMPLE_*, RADIAL) and (fx, fy) for PINHOLE and OPENCV; `ratio` and `focal` are None where
    `reason` says why the camera gets no estimate, and a warning names the camera and the reason.  A camera that already has
    a focal-length prior is left out.  `cost_fn(F, pair_cam, w, cams, ratios, device) -> (out_cost, out_weight)` on numpy arrays
    replaces the launch in the CPU tests."""
    estimates = {}
    for cid, (F, w) in sorted(camera_pairs(db, ids).items()):
        camera = db.read_camera(cid)
        if camera.has_prior_focal_length:
            continue
        cam = plain_camera(camera)
        if cam is None:
            e = dict(ratio=None, pairs=0, weight=0.0, cost_min=None, cost_median=None,
                     reason=f"a {camera.model} camera with these parameters is not a plain pinhole one")
        else:
            e = estimate_camera(F, w, cam, device, cost_fn)
        e["focal"] = None
        if e["ratio"] is not None:
            pair = camera.model in ("PINHOLE", "OPENCV")
            e["focal"] = (float(e["ratio"] * cam[0]), float(e["ratio"] * cam[1])) if pair else float(e["ratio"] * cam[0])
            logger.info("camera %d: focal length %s from %d pairs (r = %.6f, cost %.3g, median of the curve %.3g)", cid,
                        e["focal"], e["pairs"], e["ratio"], e["cost_min"], e["cost_median"])
        else:
            logger.warning("camera %d: no focal length estimated: %s", cid, e["reason"])
        estimates[cid] = e
    return estimates


def apply_focal_estimates(db, estimates):
    """Writes every estimated focal length into its camera's params and sets the camera's prior_focal_length to 1 -> the ids of
    the cameras it changed, ascending."""
    changed = []
    for cid in sorted(estimates):
        r = estimates[cid]["ratio"]
        if r is None:
            continue
        camera = db.read_camera(cid)
        params = [float(v) for v in camera.params]
        for k in range(2 if camera.model in ("PINHOLE", "OPENCV") else 1):
            params[k] = r * params[k]
        db.update_camera(cid, params, True)
        changed.append(cid)
    return changed


def reverify_database(db, ids, device="cuda", verify_fn=None, relative_pose=False):
    """Every matched pair of the images `ids` verified again from the stored `matches` under the cameras as they are now; the
    rows replace the ones in place.  -> the number of verified pairs."""
    from .two_view import verify_database_pairs

    index = {i: k for k, i in enumerate(ids) if i is not None}
    merged = {}
    for i, j in db.read_matched_image_pairs():
        if i in index and j in index:
            a, b = index[i], index[j]
            m = db.read_matches(ids[min(a, b)], ids[max(a, b)])
            merged[(min(a, b), max(a, b))] = np.zeros((0, 2), np.uint32) if m is None else m
    return verify_database_pairs(db, ids, merged, device=device, verify_fn=verify_fn, relative_pose=relative_pose)
