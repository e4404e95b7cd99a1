"""The seed model: an initial pair, that pair's triangulated points, every other image registered against
those points in one batched launch, written as a COLMAP text model.  The seed model itself triangulates no point after the
seed and registers once; mapping/grow.py (§4.2j) grows it by rounds of triangulation and registration and mapping/bundle.py
(§4.2k) adjusts the grown model once.  None of them is a mapper.  Specification: tests/util_absolute_pose.py (`seed_model`).  This build's own published rule;
parity with COLMAP's mapper is unpinned.

Where the work runs
  HIP     the triangulation of every candidate pair's inliers (vc_two_view_pose, one launch over all candidates) and the
          registration of every other image (mapping/absolute_pose.py, one batch)
  host    the database rows, the choice of the pair, the per-point filters (numpy on one pair's inliers), the tracks
"""
import logging
import os
from dataclasses import dataclass, field

import numpy as np

from ..database.colmap_db import Camera, ColmapDatabase, _quat_to_rot
from ..matching._common import CONFIG_CALIBRATED, CONFIG_PLANAR, MAX_ERROR
from ..matching.essential import camera_prior
from .absolute_pose import (ABS_POSE_MIN_NUM_INLIERS, FILTER_MIN_TRI_ANGLE, INIT_MIN_NUM_INLIERS, INIT_MIN_TRI_ANGLE,
                            estimate_absolute_poses)

logger = logging.getLogger(__name__)

# SIMPLE_RADIAL and RADIAL only with every distortion parameter zero (camera_prior refuses the others): the model is then grown
# under the pinhole assumption and the bundle adjustment may refine k from 0 (mapping/bundle.py, refine_distortion); with
# `known_distortion` also with a non-zero k, on undistorted keypoints.  OPENCV joins them only under `tangential`
# ("The tangential terms" in §4.2k: the adjustment then runs the _opencv entry points); without it the mapper refuses it, as it did
SEED_CAMERA_MODELS = ("SIMPLE_PINHOLE", "PINHOLE", "SIMPLE_RADIAL", "RADIAL")
TANGENTIAL_CAMERA_MODELS = SEED_CAMERA_MODELS + ("OPENCV",)


@dataclass
class SparseModel:
    """cameras {camera_id: Camera}; images {image_id: dict(qvec (w, x, y, z), tvec, camera_id, name, xys float64 (n, 2),
    point3D_ids int64 (n,), -1 where the keypoint observes no point)}, X_cam = R(qvec) X + tvec; points3D {point3D_id:
    dict(xyz, rgb, error, track [(image_id, keypoint index)])}; initial_pair (image_id, image_id) or None."""

    cameras: dict = field(default_factory=dict)
    images: dict = field(default_factory=dict)
    points3D: dict = field(default_factory=dict)
    initial_pair: tuple = None
    rounds: int = None                   # growth rounds that added a point or an image (§4.2j); None: a seed model
    bundle_adjustment: dict = None       # the report of the adjustment (§4.2k); None: a model that was not adjusted
    round_adjustments: list = None       # the reports of the adjustments per growth round (§4.2m); None: there were none
    split_components: int = None         # inconsistent components that took part in the growth (§4.2n); None: split_tracks was off
    split_points: list = None            # ids of the points made out of them, whether the model still has them or not; None as above

    def mean_track_length(self):
        return float(np.mean([len(p["track"]) for p in self.points3D.values()])) if self.points3D else 0.0

    def stats(self):
        s = dict(initial_pair=list(self.initial_pair) if self.initial_pair else None, registered_images=len(self.images),
                 num_points3D=len(self.points3D), mean_track_length=self.mean_track_length())
        s = s if self.rounds is None else dict(s, rounds=self.rounds)
        s = s if self.bundle_adjustment is None else dict(s, bundle_adjustment=dict(self.bundle_adjustment))
        s = s if self.round_adjustments is None else dict(s, round_adjustments=[dict(r) for r in self.round_adjustments])
        return s if self.split_points is None else dict(s, split_components=self.split_components,
                                                        split_points=sum(pid in self.points3D for pid in self.split_points))

    # COLMAP's text layout [recalled: colmap/src/colmap/scene/reconstruction_io.cc]; floats are written with repr, so a model
    # reads back equal
    def write_text(self, directory):
        os.makedirs(directory, exist_ok=True)
        with open(os.path.join(directory, "cameras.txt"), "w") as f:
            f.write("# Camera list with one line of data per camera:\n#   CAMERA_ID, MODEL, WIDTH, HEIGHT, PARAMS[]\n")
            f.write(f"# Number of cameras: {len(self.cameras)}\n")
            for cid in sorted(self.cameras):
                c = self.cameras[cid]
                f.write(" ".join([str(cid), c.model, str(int(c.width)), str(int(c.height))] + [repr(float(v)) for v in c.params]) + "\n")
        with open(os.path.join(directory, "images.txt"), "w") as f:
            n_obs = sum(int((im["point3D_ids"] >= 0).sum()) for im in self.images.values())
            f.write("# Image list with two lines of data per image:\n#   IMAGE_ID, QW, QX, QY, QZ, TX, TY, TZ, CAMERA_ID, NAME\n"
                    "#   POINTS2D[] as (X, Y, POINT3D_ID)\n")
            f.write(f"# Number of images: {len(self.images)}, mean observations per image: {n_obs / max(len(self.images), 1)}\n")
            for iid in sorted(self.images):
                im = self.images[iid]
                f.write(" ".join([str(iid)] + [repr(float(v)) for v in list(im["qvec"]) + list(im["tvec"])]
                                 + [str(int(im["camera_id"])), im["name"]]) + "\n")
                f.write(" ".join(f"{float(x)!r} {float(y)!r} {int(p)}" for (x, y), p in zip(im["xys"], im["point3D_ids"])) + "\n")
        with open(os.path.join(directory, "points3D.txt"), "w") as f:
            f.write("# 3D point list with one line of data per point:\n"
                    "#   POINT3D_ID, X, Y, Z, R, G, B, ERROR, TRACK[] as (IMAGE_ID, POINT2D_IDX)\n")
            f.write(f"# Number of points: {len(self.points3D)}, mean track length: {self.mean_track_length()}\n")
            for pid in sorted(self.points3D):
                p = self.points3D[pid]
                f.write(" ".join([str(pid)] + [repr(float(v)) for v in p["xyz"]] + [str(int(v)) for v in p["rgb"]]
                                 + [repr(float(p["error"]))] + [f"{int(i)} {int(k)}" for i, k in p["track"]]) + "\n")

    @classmethod
    def read_text(cls, directory):
        def lines(name):
            with open(os.path.join(directory, name)) as f:
                return [ln.rstrip("\n") for ln in f if not ln.startswith("#")]

        model = cls()
        for ln in lines("cameras.txt"):
            w = ln.split()
            if w:
                model.cameras[int(w[0])] = Camera(model=w[1], width=int(w[2]), height=int(w[3]), params=[float(v) for v in w[4:]],
                                                  camera_id=int(w[0]))
        rows = lines("images.txt")
        for head, pts in zip(rows[0::2], rows[1::2]):
            w, q = head.split(), pts.split()
            model.images[int(w[0])] = dict(
                qvec=np.array([float(v) for v in w[1:5]]), tvec=np.array([float(v) for v in w[5:8]]), camera_id=int(w[8]),
                name=" ".join(w[9:]), xys=np.array([float(v) for v in q]).reshape(-1, 3)[:, :2].copy(),
                point3D_ids=np.array([int(v) for v in q[2::3]], np.int64))
        for ln in lines("points3D.txt"):
            w = ln.split()
            if w:
                model.points3D[int(w[0])] = dict(xyz=np.array([float(v) for v in w[1:4]]), rgb=tuple(int(v) for v in w[4:7]),
                                                 error=float(w[7]), track=[(int(i), int(k)) for i, k in zip(w[8::2], w[9::2])])
        return model

    def __eq__(self, other):
        if not isinstance(other, SparseModel):
            return NotImplemented

        def cam(c):
            return (c.model, int(c.width), int(c.height), [float(v) for v in c.params])

        if {k: cam(c) for k, c in self.cameras.items()} != {k: cam(c) for k, c in other.cameras.items()}:
            return False
        if sorted(self.images) != sorted(other.images) or sorted(self.points3D) != sorted(other.points3D):
            return False
        for k, a in self.images.items():
            b = other.images[k]
            if not (np.array_equal(a["qvec"], b["qvec"]) and np.array_equal(a["tvec"], b["tvec"]) and a["camera_id"] == b["camera_id"]
                    and a["name"] == b["name"] and np.array_equal(np.asarray(a["xys"], np.float64).reshape(-1, 2), np.asarray(b["xys"], np.float64).reshape(-1, 2))
                    and np.array_equal(a["point3D_ids"], b["point3D_ids"])):
                return False
        for k, a in self.points3D.items():
            b = other.points3D[k]
            if not (np.array_equal(a["xyz"], b["xyz"]) and tuple(a["rgb"]) == tuple(b["rgb"]) and float(a["error"]) == float(b["error"])
                    and [tuple(t) for t in a["track"]] == [tuple(t) for t in b["track"]]):
                return False
        return True


def _gpu_two_view_pose(xn_rows, cand, device):
    """The one triangulation launch over all candidate pairs -> front (P, 4), tri_angle (P,), midpoints per pair."""
    import torch

    from ..matching._common import _pair_batch
    from ..matching.pose import two_view_pose

    xn, offsets, _, _ = _pair_batch(xn_rows, None, device)
    front, best, tri, pts = two_view_pose(xn, offsets, torch.from_numpy(cand).to(device), points=True)
    if bool((best < 0).any()):
        raise RuntimeError("vc_two_view_pose: the workspace did not hold the keys of every pair")
    cuts = np.cumsum([len(r) for r in xn_rows])[:-1]
    return front.cpu().numpy(), tri.cpu().numpy(), np.split(pts.cpu().numpy(), cuts)


def _normalise(pts, K1, K2):
    K1i, K2i = np.linalg.inv(K1), np.linalg.inv(K2)
    p64 = np.asarray(pts, np.float64)
    return np.concatenate([p64[:, :2] * [K1i[0, 0], K1i[1, 1]] + [K1i[0, 2], K1i[1, 2]],
                           p64[:, 2:] * [K2i[0, 0], K2i[1, 1]] + [K2i[0, 2], K2i[1, 2]]], axis=1)


def _point_angles(X, centre):
    """Angle at each point X (n, 3) between the rays to the origin and to `centre`."""
    e = X - centre
    k = np.cross(X, e)
    return np.arctan2(np.linalg.norm(k, axis=1), (X * e).sum(axis=1))


def _pixel_errors(K, R, t, xyz, obs):
    Xc = xyz @ R.T + t
    with np.errstate(all="ignore"):
        p = np.stack([K[0, 0] * Xc[:, 0] / Xc[:, 2] + K[0, 2], K[1, 1] * Xc[:, 1] / Xc[:, 2] + K[1, 2]], axis=1)
        err = np.linalg.norm(p - obs, axis=1)
    return np.where(Xc[:, 2] > 0, err, np.inf)


def _pixel_errors_radial(K, k, R, t, xyz, obs):
    """_pixel_errors under the distortion k = (k1, k2): the pixel is K (xu s, xv s, 1), s = 1 + k1 rho + k2 rho rho."""
    Xc = xyz @ R.T + t
    with np.errstate(all="ignore"):
        xu, xv = Xc[:, 0] / Xc[:, 2], Xc[:, 1] / Xc[:, 2]
        rho = xu * xu + xv * xv
        s = 1.0 + k[0] * rho + k[1] * rho * rho
        p = np.stack([K[0, 0] * (xu * s) + K[0, 2], K[1, 1] * (xv * s) + K[1, 2]], axis=1)
        err = np.linalg.norm(p - obs, axis=1)
    return np.where(Xc[:, 2] > 0, err, np.inf)


def _pixel_errors_opencv(K, k, R, t, xyz, obs):
    """_pixel_errors under the distortion k = (k1, k2, p1, p2), the forward model of csrc/undistort.hip: the radial term first, the
    tangential terms added after it."""
    Xc = xyz @ R.T + t
    with np.errstate(all="ignore"):
        xu, xv = Xc[:, 0] / Xc[:, 2], Xc[:, 1] / Xc[:, 2]
        rho = xu * xu + xv * xv
        s = 1.0 + k[0] * rho + k[1] * rho * rho
        xd = xu * s + 2.0 * k[2] * xu * xv + k[3] * (rho + 2.0 * xu * xu)
        yd = xv * s + k[2] * (rho + 2.0 * xv * xv) + 2.0 * k[3] * xu * xv
        p = np.stack([K[0, 0] * xd + K[0, 2], K[1, 1] * yd + K[1, 2]], axis=1)
        err = np.linalg.norm(p - obs, axis=1)
    return np.where(Xc[:, 2] > 0, err, np.inf)


def _read_database(database_path, known_distortion=False, undistort_fn=None, device="cuda", tangential=False):
    """The rows the seed model and its growth read -> images {image_id: Image}, cameras {camera_id: Camera}, K {image_id: (3, 3)
    or None where the camera has no usable prior or another model}, kps {image_id: float32 (n, 2)}, rows {(i, j), i < j: the
    two_view_geometries row} of every CALIBRATED or PLANAR row with inliers.
    `known_distortion`: a sixth entry follows, `known` = dict(raw {image_id: the keypoints as the database
    holds them}, dist {image_id: (k1, k2)} of the images that were undistorted).  K is then also usable for a flagged
    SIMPLE_RADIAL or RADIAL camera with a non-zero k (matching.undistort.camera_calibration; without `tangential` OPENCV stays refused:
    SEED_CAMERA_MODELS), the kps of such an image are its undistorted pixels in float64, NaN where a keypoint does not invert,
    and the rows have lost the inlier matches that touch such a keypoint, so it is in no track.  `undistort_fn(xy, cam, cams,
    device) -> (xy64, valid)` on numpy arrays replaces the launch of vc_undistort_points (tests).
    `tangential` ("The tangential terms" in §4.2k): OPENCV is a model like the other four: usable with all four distortion
    parameters zero and, under known_distortion, with any finite ones, through the same launch; `known["dist"]` then carries
    (k1, k2, p1, p2) for the images of such a camera.  Off, nothing changes."""
    models = TANGENTIAL_CAMERA_MODELS if tangential else SEED_CAMERA_MODELS
    with ColmapDatabase.open_database(str(database_path)) as db:
        images = {im.image_id: im for im in db.read_all_images()}
        cameras, K, kps, distorted = {}, {}, {}, {}
        for iid, im in images.items():
            if im.camera_id not in cameras:
                cameras[im.camera_id] = db.read_camera(im.camera_id)
            cam = cameras[im.camera_id]
            Kc, ok, _ = camera_prior(cam)
            K[iid] = Kc if ok and cam.model in models else None
            if known_distortion and K[iid] is None and cam.model in models:
                from ..matching.undistort import camera_calibration

                Kc, dist, usable = camera_calibration(cam)
                if usable:
                    K[iid], distorted[iid] = Kc, (Kc, dist)
            kp = db.read_keypoints(iid)
            kps[iid] = np.zeros((0, 2), np.float32) if kp is None else kp[:, :2]
        rows = {}
        for i, j, n, config in db.read_two_view_geometry_pairs():
            if n > 0 and config in (CONFIG_CALIBRATED, CONFIG_PLANAR) and i in images and j in images:
                rows[(i, j)] = db.read_two_view_geometry(i, j)
    if not known_distortion:
        return images, cameras, K, kps, rows
    from ..matching.undistort import undistort_images

    known = dict(raw=dict(kps), dist={iid: tuple(float(v) for v in (d if cameras[images[iid].camera_id].model == "OPENCV" else d[:2]))
                                      for iid, (_, d) in distorted.items()})
    kps, invalid = dict(kps), 0
    for iid, (xy64, valid) in undistort_images(known["raw"], distorted, device, undistort_fn).items():
        kps[iid] = np.where(valid[:, None], xy64, np.nan)
        invalid += int((~valid).sum())
    for (i, j), g in rows.items():
        m = g["inlier_matches"].astype(np.int64).reshape(-1, 2)
        keep = np.isfinite(kps[i][m[:, 0]]).all(axis=1) & np.isfinite(kps[j][m[:, 1]]).all(axis=1)
        if not keep.all():
            rows[(i, j)] = dict(g, inlier_matches=g["inlier_matches"][keep])
    logger.info("known distortion: the keypoints of %d of %d images undistorted (%d do not invert)", len(distorted), len(images), invalid)
    return images, cameras, K, kps, rows, known


def _observation_errors(K, kps, known, iid, R, t, xyz, kp):
    """The pixel error of the point(s) xyz (n, 3) at keypoint(s) `kp` of image iid: against the keypoints the solvers used or,
    for an image that was undistorted (§4.2l), by the distorted projection against the raw keypoints."""
    if known is None or iid not in known["dist"]:
        return _pixel_errors(K[iid], R, t, xyz, kps[iid][kp].astype(np.float64).reshape(-1, 2))
    errors = _pixel_errors_opencv if len(known["dist"][iid]) == 4 else _pixel_errors_radial
    return errors(K[iid], known["dist"][iid], R, t, xyz, known["raw"][iid][kp].astype(np.float64).reshape(-1, 2))


def _database(database_path, device, known_distortion, undistort_fn, tangential):
    """_read_database with `known_distortion` and `tangential` passed on only where they are on."""
    tangential_args = dict(tangential=True) if tangential else {}
    if known_distortion:
        return _read_database(database_path, True, undistort_fn, device, **tangential_args)
    return _read_database(database_path, **tangential_args)


def build_seed_model(database_path, device="cuda", two_view_pose_fn=None, estimate_fn=None, known_distortion=False,
                     undistort_fn=None, tangential=False) -> SparseModel:
    """Read a matched database -> the seed model.  Raises ValueError, naming the condition, when no pair can start it.
    `two_view_pose_fn(xn_rows, cand, device)` and `estimate_fn(problems, device)` replace the two GPU steps (tests).
    `known_distortion` (§4.2l): the model is solved on the undistorted keypoints of the flagged SIMPLE_RADIAL and RADIAL cameras
    (`_read_database`); its `xys` are the raw keypoints, as COLMAP's are, and `error` uses the distorted projection.
    `tangential`: OPENCV cameras are read as the other models are (`_read_database`)."""
    return _seed_model(_database(database_path, device, known_distortion, undistort_fn, tangential), device, two_view_pose_fn, estimate_fn)


def _seed_model(database, device, two_view_pose_fn, estimate_fn):
    two_view_pose_fn = two_view_pose_fn or _gpu_two_view_pose
    estimate_fn = estimate_fn or estimate_absolute_poses
    images, cameras, K, kps, rows = database[:5]
    known = database[5] if len(database) > 5 else None                 # the raw keypoints and k of undistorted images (§4.2l)
    raw = kps if known is None else known["raw"]
    geoms = {pair: g for pair, g in rows.items() if g["config"] == CONFIG_CALIBRATED}

    def directed(i, j):
        """The CALIBRATED geometry of (i -> j): match columns (i, j), X_j = R X_i + t; None where there is no such row."""
        g = geoms.get((min(i, j), max(i, j)))
        if g is None:
            return None
        m, R, t = g["inlier_matches"].astype(np.int64), _quat_to_rot(g["qvec"]), np.asarray(g["tvec"], np.float64)
        if i > j:
            m, R, t = m[:, ::-1], R.T, -R.T @ t
        return m, R, t

    # 1. candidate pairs, one triangulation launch
    cands = [(i, j) for (i, j), g in sorted(geoms.items())
             if np.any(g["tvec"]) and len(g["inlier_matches"]) >= INIT_MIN_NUM_INLIERS and K[i] is not None and K[j] is not None]
    if not cands:
        raise ValueError("seed model: no CALIBRATED pair with a translation, two focal-length priors and at least "
                         f"{INIT_MIN_NUM_INLIERS} inliers")
    pix, xn_rows = [], []
    cand = np.full((len(cands), 4, 12), np.nan)
    for p, (i, j) in enumerate(cands):
        m, R, t = directed(i, j)
        pix.append(np.concatenate([kps[i][m[:, 0]], kps[j][m[:, 1]]], axis=1).astype(np.float32))
        xn_rows.append(_normalise(pix[-1], K[i], K[j]))
        cand[p, 0, :9], cand[p, 0, 9:] = R.reshape(9), t
    front, tri, midpoints = two_view_pose_fn(xn_rows, cand, device)
    best = None
    for p in range(len(cands)):                                     # most points in front, the lowest pair id on ties
        if tri[p] >= INIT_MIN_TRI_ANGLE and (best is None or front[p, 0] > front[best, 0]):
            best = p
    if best is None:
        raise ValueError(f"seed model: no candidate pair reaches a triangulation angle of {np.degrees(INIT_MIN_TRI_ANGLE):.0f} degrees")

    # 2. world frame: the camera of the lower image id; points: in front, wide enough, inliers of both cameras
    a, b = cands[best]
    m, R, t = directed(a, b)
    X, pts = midpoints[best], pix[best]
    is_front = np.isfinite(X).all(axis=1)
    Xs = np.where(is_front[:, None], X, 1.0)
    keep = is_front & (_point_angles(Xs, -R.T @ t) >= FILTER_MIN_TRI_ANGLE)
    keep &= _pixel_errors(K[a], np.eye(3), np.zeros(3), Xs, pts[:, :2].astype(np.float64)) <= MAX_ERROR
    keep &= _pixel_errors(K[b], R, t, Xs, pts[:, 2:].astype(np.float64)) <= MAX_ERROR
    xyz, m = X[keep], m[keep]
    tracks = [[(a, int(ka)), (b, int(kb))] for ka, kb in m]
    point_of = {a: {int(ka): k for k, (ka, _) in enumerate(m)}, b: {int(kb): k for k, (_, kb) in enumerate(m)}}
    poses = {a: (np.array([1.0, 0.0, 0.0, 0.0]), np.zeros(3)), b: (geoms[(a, b)]["qvec"].copy(), t.copy())}

    # 3. every other image against those points, one batch
    problems, meta = [], []
    for c in sorted(images):
        if c in (a, b) or K[c] is None:
            continue
        used, kp_idx, pt_idx = set(), [], []
        for other in (a, b):
            g = directed(c, other)
            if g is None:
                continue
            for kc, ko in g[0]:
                k = point_of[other].get(int(ko))
                if k is not None and int(kc) not in used:
                    used.add(int(kc)), kp_idx.append(int(kc)), pt_idx.append(k)
        if len(kp_idx) >= ABS_POSE_MIN_NUM_INLIERS:
            problems.append(dict(obs=kps[c][kp_idx], xyz=xyz[pt_idx], K=K[c], seed=c))
            meta.append((c, kp_idx, pt_idx))
    for (c, kp_idx, pt_idx), r in zip(meta, estimate_fn(problems, device) if problems else []):
        if not r["success"]:
            continue
        poses[c] = (np.asarray(r["qvec"], np.float64), np.asarray(r["tvec"], np.float64))
        for kc, k, ok in zip(kp_idx, pt_idx, r["inlier_mask"]):
            if ok:
                tracks[k].append((c, kc))

    # 4. the model
    model = SparseModel(initial_pair=(a, b))
    for iid, (q, tv) in sorted(poses.items()):
        cid = images[iid].camera_id
        model.cameras[cid] = cameras[cid]
        model.images[iid] = dict(qvec=q, tvec=tv, camera_id=cid, name=images[iid].name, xys=raw[iid].astype(np.float64),
                                 point3D_ids=np.full(len(kps[iid]), -1, np.int64))
    for k, track in enumerate(tracks):
        errs = []
        for iid, kp in track:
            model.images[iid]["point3D_ids"][kp] = k + 1
            q, tv = poses[iid]
            errs.append(_observation_errors(K, kps, known, iid, _quat_to_rot(q), tv, xyz[k][None], kp)[0])
        model.points3D[k + 1] = dict(xyz=xyz[k].copy(), rgb=(0, 0, 0), error=float(np.mean(errs)), track=list(track))
    return model
