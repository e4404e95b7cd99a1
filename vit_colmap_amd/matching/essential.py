"""The calibrated branch of geometric verification: essential-matrix RANSAC for the pairs whose two
cameras carry a usable focal-length prior.  Specification: tests/util_essential.py.

Where the work runs
  HIP     the five-point solver, every hypothesis of every pair in one launch (csrc/essential.hip, vc_essential_5pt);
          scoring and masks by the F kernels of csrc/two_view.hip on F_px = K2^-T E K1^-1
  torch   the sampler (_common._sample_indices), K^-1, the one eight-point refit (a 9x9 and a 3x3 SVD per pair)
  host    the camera rows -> K table, the pose choice per CALIBRATED pair (numpy on the pair's inliers)
"""
import logging
from functools import partial

import numpy as np
import torch

from ._common import SALT, _mask, _ransac_tail, _sample_indices, _score, _solve_minimal

logger = logging.getLogger(__name__)

NUM_HYP_E = 128
MAX_SOLUTIONS = 10
MIN_E_F_INLIER_RATIO = 0.95        # [recalled: COLMAP's min_E_F_inlier_ratio]
_DISTORTION_FROM = {"SIMPLE_PINHOLE": 3, "PINHOLE": 4, "SIMPLE_RADIAL": 3, "RADIAL": 3, "OPENCV": 4}


def camera_prior(camera):
    """A Camera row -> (K float64 (3, 3), usable prior?, flagged but distorted?).  Usable: `has_prior_focal_length` and a
    SIMPLE_PINHOLE / PINHOLE model, or SIMPLE_RADIAL / RADIAL / OPENCV with every distortion parameter zero."""
    model = camera.model if isinstance(camera.model, str) else getattr(camera.model, "name", str(camera.model))
    flagged = bool(getattr(camera, "has_prior_focal_length", False))
    if model not in _DISTORTION_FROM:
        return np.eye(3), False, False
    p = [float(v) for v in camera.params]
    if model in ("PINHOLE", "OPENCV"):
        fx, fy, cx, cy = p[0], p[1], p[2], p[3]
    else:
        fx, fy, cx, cy = p[0], p[0], p[1], p[2]
    K = np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])
    plain = all(d == 0 for d in p[_DISTORTION_FROM[model]:]) and fx > 0 and fy > 0 and bool(np.all(np.isfinite(K)))
    return K, flagged and plain, flagged and not plain


def camera_table(db, ids, warn_distorted=True):
    """(K float64 (n, 3, 3), prior uint8 (n,)) for the images `ids` of an open database (None: no row, no prior): the form
    the cameras travel in, next to the keypoints.  A flagged camera with distortion is logged once and has no prior
    (`warn_distorted=False`: not logged, where matching/undistort.py gives it one afterwards)."""
    image_camera = {im.image_id: im.camera_id for im in db.read_all_images()}
    cams, warned = {}, set()
    K = np.tile(np.eye(3), (len(ids), 1, 1))
    prior = np.zeros(len(ids), np.uint8)
    for k, image_id in enumerate(ids):
        cid = image_camera.get(image_id)
        if cid is None:
            continue
        if cid not in cams:
            cams[cid] = camera_prior(db.read_camera(cid))
        K[k], ok, distorted = cams[cid]
        prior[k] = ok
        if distorted and warn_distorted and cid not in warned:
            warned.add(cid)
            logger.warning("camera %d has a focal-length prior and non-zero distortion: its pairs are verified without the prior",
                           cid)
    return K, prior


def solve_five_point(pts_n, offsets, samples):
    """pts_n float64 (total, 4), offsets int32 (P + 1), samples int32 (P, n_hyp, 5), all on one GPU
    -> E float64 (P, n_hyp, 10, 9) (NaN past the count), count int32 (P, n_hyp)."""
    return _solve_minimal("vc_essential_5pt", "solve_five_point needs float64 points", [pts_n], offsets, samples, MAX_SOLUTIONS, 9)


def normalise_points(p64, pair_of, K1i, K2i):
    """Pixel matches float64 (total, 4) -> normalised camera coordinates (K has no skew: one scale and one shift per axis)."""
    return torch.stack([p64[:, 0] * K1i[pair_of, 0, 0] + K1i[pair_of, 0, 2], p64[:, 1] * K1i[pair_of, 1, 1] + K1i[pair_of, 1, 2],
                        p64[:, 2] * K2i[pair_of, 0, 0] + K2i[pair_of, 0, 2], p64[:, 3] * K2i[pair_of, 1, 1] + K2i[pair_of, 1, 2]],
                       dim=1).contiguous()


def _pixel_f(E, K1i, K2i):
    """E float64 (P, n, 3, 3) -> F_px = K2^-T E K1^-1 at unit Frobenius norm, float32 (P, n, 9); NaN stays NaN."""
    F = K2i.transpose(-1, -2)[:, None] @ E @ K1i[:, None]
    F = F / torch.linalg.norm(F.reshape(F.shape[0], F.shape[1], 9), dim=-1)[:, :, None, None]
    return F.reshape(F.shape[0], F.shape[1], 9).to(torch.float32).contiguous()


def estimate_e(pts, offsets, pair_of, seeds, K1, K2, n_hyp=NUM_HYP_E, max_error=4.0):
    """All calibrated pairs at once.  pts float32 (total, 4) pixels, K1, K2 float64 (P, 3, 3) on the device
    -> E float64 (P, 3, 3) at unit norm, F_px float32 (P, 9) (NaN where none), inlier mask bool (total,), counts int64 (P,),
    the normalised points float64 (total, 4)."""
    dev = pts.device
    P = offsets.shape[0] - 1
    M = (offsets[1:] - offsets[:-1]).to(torch.int64)
    K1i, K2i = torch.linalg.inv(K1), torch.linalg.inv(K2)
    xn = normalise_points(pts.to(torch.float64), pair_of, K1i, K2i)
    idx = _sample_indices(seeds, M, n_hyp, 5, SALT["E"]).to(torch.int32).contiguous()
    sol, _ = solve_five_point(xn, offsets, idx)
    sol = sol.reshape(P, n_hyp * MAX_SOLUTIONS, 3, 3)                       # ranked by (hypothesis, solution)
    hyp32 = _pixel_f(sol, K1i, K2i)
    score = partial(_score, pts, offsets, model="F", max_error=max_error)
    counts = score(hyp32).to(torch.int64)
    e_refit = None

    def refit(mask, nbest):
        # eight-point least squares over the best hypothesis' inliers in normalised coordinates (the singular vector of A'A
        # with the smallest singular value), projected onto the essential manifold
        nonlocal e_refit
        x1, y1, x2, y2 = xn.unbind(dim=1)
        A = torch.stack([x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, torch.ones_like(x1)], dim=1)
        AtA = torch.zeros((P, 9, 9), dtype=torch.float64, device=dev).index_add_(
            0, pair_of, (A[:, :, None] * A[:, None, :]) * mask.to(torch.float64)[:, None, None])
        e_refit = project_to_essential(torch.linalg.svd(AtA).Vh[:, -1, :].reshape(P, 3, 3))
        ok = torch.isfinite(e_refit).all(dim=-1).all(dim=-1) & (nbest >= 8)
        refit32 = _pixel_f(e_refit[:, None], K1i, K2i)[:, 0]
        return torch.where(ok[:, None], refit32, torch.full_like(refit32, float("nan"))).contiguous(), ok

    final, fmask, fcount, kbest, use = _ransac_tail(hyp32, counts, score, partial(_mask, pts, offsets, model="F", max_error=max_error), refit)
    e_final = torch.where(use[:, None, None], e_refit, sol[torch.arange(P, device=dev), kbest])
    e_final = e_final / torch.linalg.norm(e_final.reshape(P, 9), dim=1).clamp(min=1e-300)[:, None, None]
    return e_final, final, fmask, fcount, xn


def project_to_essential(M):
    """Batched closest matrix with singular values (1, 1, 0), at unit Frobenius norm."""
    U, _, Vt = torch.linalg.svd(M)
    d = torch.tensor([1.0, 1.0, 0.0], dtype=M.dtype, device=M.device) / np.sqrt(2.0)
    return U @ torch.diag_embed(d.expand(M.shape[0], 3)) @ Vt


def rot_to_quat(R):
    """Rotation matrix -> unit quaternion (w, x, y, z) with w >= 0."""
    t = np.trace(R)
    if t > 0:
        s = np.sqrt(t + 1.0) * 2
        q = np.array([0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s])
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k]) * 2
        q = np.zeros(4)
        q[0] = (R[k, j] - R[j, k]) / s
        q[1 + i] = 0.25 * s
        q[1 + j] = (R[j, i] + R[i, j]) / s
        q[1 + k] = (R[k, i] + R[i, k]) / s
    q = q / np.linalg.norm(q)
    return -q if q[0] < 0 else q


def choose_pose(E, xn):
    """Of E's four decompositions (R, t), X2 = R X1 + t, the one with most of xn float64 (n, 4) (normalised inliers) in front
    of both cameras; the first on ties in the order (Ra, u), (Ra, -u), (Rb, u), (Rb, -u) -> qvec (w, x, y, z), unit tvec."""
    U, _, Vt = np.linalg.svd(np.asarray(E, np.float64).reshape(3, 3))
    if np.linalg.det(U) < 0:
        U = -U
    if np.linalg.det(Vt) < 0:
        Vt = -Vt
    W = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    u = U[:, 2]
    x1 = np.concatenate([xn[:, :2], np.ones((len(xn), 1))], axis=1)
    x2 = np.concatenate([xn[:, 2:], np.ones((len(xn), 1))], axis=1)
    best = None
    for R in (U @ W @ Vt, U @ W.T @ Vt):
        for t in (u, -u):
            a = x1 @ R.T                                      # depths d1, d2 of d2 x2 = d1 R x1 + t, least squares per point
            aa, ab, bb = (a * a).sum(1), (a * x2).sum(1), (x2 * x2).sum(1)
            at, bt = a @ t, x2 @ t
            det = aa * bb - ab * ab
            with np.errstate(all="ignore"):
                d1 = (-bb * at + ab * bt) / det
                d2 = (-ab * at + aa * bt) / det
            n = int(((d1 > 0) & (d2 > 0)).sum())
            if best is None or n > best[0]:
                best = (n, R, t)
    _, R, t = best
    return rot_to_quat(R), t / np.linalg.norm(t)
