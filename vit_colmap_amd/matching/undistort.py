"""A camera's known lens distortion: raw keypoints -> the pixels an ideal pinhole camera with the same K
would see, in front of every solver that assumes one (F, H, E, relative pose, guided matching, P3P, triangulation).  The
option is `camera.known_distortion` (--known-distortion), off by default; without it a flagged camera with a non-zero
distortion parameter has no usable prior (essential.camera_prior, which this module leaves as it is).  Specification:
tests/util_undistort.py.

Where the work runs
  HIP     the inversion of the distortion model, one keypoint per lane, every keypoint of a call in one launch
          (csrc/undistort.hip, vc_undistort_points, whose header states the rule)
  host    the camera rows -> the table of eight parameters, which images are undistorted, the packed keypoint arrays
"""
import logging

import numpy as np

from .essential import _DISTORTION_FROM

logger = logging.getLogger(__name__)

UNDISTORT_MAX_STEPS = 20             # kUndistortSteps of csrc/undistort.hip
UNDISTORT_STOP = 1e-24               # kUndistortStop: the squared length of the last Newton step, normalised units


def camera_calibration(camera):
    """A Camera row -> (K float64 (3, 3), dist float64 (4,) = (k1, k2, p1, p2), usable?).  Usable: `has_prior_focal_length`,
    a SIMPLE_PINHOLE / PINHOLE / SIMPLE_RADIAL / RADIAL / OPENCV model with all of its parameters, fx and fy positive and
    every number finite.  The distortion may be anything finite: what camera_prior refuses, this accepts."""
    model = camera.model if isinstance(camera.model, str) else getattr(camera.model, "name", str(camera.model))
    flagged = bool(getattr(camera, "has_prior_focal_length", False))
    dist = np.zeros(4)
    if model not in _DISTORTION_FROM:
        return np.eye(3), dist, False
    p = [float(v) for v in camera.params]
    n_dist = {"SIMPLE_PINHOLE": 0, "PINHOLE": 0, "SIMPLE_RADIAL": 1, "RADIAL": 2, "OPENCV": 4}[model]
    if len(p) < _DISTORTION_FROM[model] + n_dist:
        return np.eye(3), dist, False
    if model in ("PINHOLE", "OPENCV"):
        fx, fy, cx, cy = p[0], p[1], p[2], p[3]
    else:
        fx, fy, cx, cy = p[0], p[0], p[1], p[2]
    dist[:n_dist] = p[_DISTORTION_FROM[model]:_DISTORTION_FROM[model] + n_dist]
    K = np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])
    usable = flagged and fx > 0 and fy > 0 and bool(np.all(np.isfinite(K))) and bool(np.all(np.isfinite(dist)))
    return K, dist, usable


def camera_row(K, dist):
    """-> the eight numbers of a camera as vc_undistort_points reads them: fx, fy, cx, cy, k1, k2, p1, p2."""
    return np.concatenate([[K[0, 0], K[1, 1], K[0, 2], K[1, 2]], np.asarray(dist, np.float64).reshape(4)])


def undistort_points(xy, cam, cams):
    """xy float32 (n, 2) raw pixels, cam int32 (n,) slots into cams, cams float64 (n_cams, 8) (`camera_row`), all on one GPU
    -> xy64 float64 (n, 2) (NaN where invalid), valid bool (n,).  A slot outside [0, n_cams) raises (VC_ERR_INVALID_ARG)."""
    import torch

    from .. import _lib

    if not (xy.is_cuda and xy.dtype == torch.float32 and cam.dtype == torch.int32 and cams.dtype == torch.float64):
        raise ValueError("undistort_points needs float32 keypoints, int32 slots and float64 cameras on the GPU")
    if any(t.device != xy.device for t in (cam, cams)):
        raise ValueError("undistort_points needs every tensor on the same GPU")
    n = int(cam.shape[0])
    if xy.shape != (n, 2) or cam.dim() != 1 or cams.dim() != 2 or cams.shape[1] != 8:
        raise ValueError("undistort_points needs xy (n, 2), cam (n,), cams (n_cams, 8)")
    out = torch.full((n, 2), float("nan"), dtype=torch.float64, device=xy.device)
    valid = torch.zeros((n,), dtype=torch.uint8, device=xy.device)
    if n == 0:
        return out, valid.bool()
    xy, cam, cams = (t.contiguous() for t in (xy, cam, cams))
    _lib.check(_lib.load().vc_undistort_points(_lib.ptr(xy), _lib.ptr(cam), n, _lib.ptr(cams), int(cams.shape[0]), _lib.ptr(out),
                                               _lib.ptr(valid), _lib.stream_ptr()), "vc_undistort_points")
    return out, valid.bool()


def gpu_undistort(xy, cam, cams, device="cuda"):
    """undistort_points on numpy arrays -> xy64 (n, 2), valid bool (n,): the default of the `undistort_fn` seams."""
    import torch

    out, valid = undistort_points(*(torch.from_numpy(np.ascontiguousarray(a, t)).to(device)
                                    for a, t in ((xy, np.float32), (cam, np.int32), (cams, np.float64))))
    return out.cpu().numpy(), valid.cpu().numpy()


def undistort_images(keypoints, calibrations, device="cuda", undistort_fn=None):
    """keypoints {key: float32 (n, >= 2)}, calibrations {key: (K, dist)} of the images to undistort -> {key: (xy float64 (n, 2),
    valid bool (n,))}, every image of the call in one launch (one slot per distinct camera)."""
    keys = [k for k in calibrations if len(keypoints[k])]
    out = {k: (np.zeros((0, 2)), np.zeros(0, bool)) for k in calibrations}
    if not keys:
        return out
    rows, slot_of_row, slot_of = [], {}, {}
    for k in keys:
        row = camera_row(*calibrations[k])
        if row.tobytes() not in slot_of_row:
            slot_of_row[row.tobytes()] = len(rows)
            rows.append(row)
        slot_of[k] = slot_of_row[row.tobytes()]
    xy = np.concatenate([np.asarray(keypoints[k], np.float32)[:, :2] for k in keys])
    cam = np.concatenate([np.full(len(keypoints[k]), slot_of[k], np.int32) for k in keys])
    xy64, valid = (undistort_fn or gpu_undistort)(xy, cam, np.stack(rows), device)
    cuts = np.cumsum([len(keypoints[k]) for k in keys])[:-1]
    for k, p, v in zip(keys, np.split(np.asarray(xy64, np.float64), cuts), np.split(np.asarray(valid, bool), cuts)):
        out[k] = (p, v)
    return out


def undistort_for_matching(db, ids, kp_arr, kp_cnt, cam_k, cam_prior, device="cuda", undistort_fn=None):
    """What exhaustive.match_database and pipeline.distributed.run_sharded share under the option: the packed keypoints
    float32 (n, n_max, 2) + counts and the camera table (essential.camera_table) of the images `ids` (None: no row) of an
    open database -> (kp_arr, cam_k, cam_prior) in which every image whose camera is flagged, distorted and usable
    (`camera_calibration`) carries the undistorted pixels, cast to float32 (the verifier's input type; NaN where the keypoint
    does not invert: match_loaded drops the matches that touch one), its K and prior 1.  Every other image is as it was."""
    image_camera = {im.image_id: im.camera_id for im in db.read_all_images()}
    cams, todo = {}, {}
    for k, image_id in enumerate(ids):
        cid = image_camera.get(image_id)
        if cid is None:
            continue
        if cid not in cams:
            cams[cid] = camera_calibration(db.read_camera(cid))
        K, dist, usable = cams[cid]
        if usable and dist.any():
            todo[k] = (K, dist)
    kp_arr, cam_k, cam_prior = np.array(kp_arr, np.float32), np.array(cam_k, np.float64), np.array(cam_prior, np.uint8)
    done = undistort_images({k: kp_arr[k, : kp_cnt[k]] for k in todo}, todo, device, undistort_fn)
    for k, (xy64, valid) in done.items():
        kp_arr[k, : kp_cnt[k]] = np.where(valid[:, None], xy64, np.nan).astype(np.float32)
        cam_k[k], cam_prior[k] = todo[k][0], 1
    logger.info("known distortion: the keypoints of %d of %d images undistorted (%d do not invert)", len(todo), len(ids),
                sum(int((~v).sum()) for _, v in done.values()))
    return kp_arr, cam_k, cam_prior


def drop_invalid_matches(lists, pairs, kp_ok):
    """Match lists (M, 2) of the image-index pairs `pairs` -> the lists without the matches that touch a keypoint whose row of
    kp_ok bool (n, n_max) is False, and the number dropped."""
    out, dropped = [], 0
    for (a, b), m in zip(pairs, lists):
        m = np.asarray(m).reshape(-1, 2)
        idx = m.astype(np.int64)
        keep = kp_ok[int(a), idx[:, 0]] & kp_ok[int(b), idx[:, 1]]
        dropped += int((~keep).sum())
        out.append(m[keep])
    return out, dropped
