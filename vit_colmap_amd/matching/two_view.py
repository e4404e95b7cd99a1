"""Two-view geometric verification of the putative matches — the step that follows descriptor matching inside
`pycolmap.match_exhaustive` (reference call site vit_colmap/pipeline/run_pipeline.py:351-363) and fills the
`two_view_geometries(rows, config, ...)` rows the reference's matching metrics read
(vit_colmap/utils/metrics.py:207-243).  Specification: oracle/two_view_oracle.py (the build's own RANSAC on F and H
with a published sampler; parity with COLMAP's estimator is unpinned — COLMAP is an absent third-party wheel).

Where the work runs
  HIP     scoring of every hypothesis against every match of every pair, and the inlier masks
          (csrc/two_view.hip, vc_two_view_score / vc_two_view_inliers): O(pairs x hypotheses x matches);
          the five-point solver of the calibrated branch (csrc/essential.hip; matching/essential.py)
          the triangulation behind the relative pose (csrc/pose.hip; matching/pose.py)
  torch   the minimal solvers: batched 8x8 linear systems (float64) for all pairs and hypotheses at once, the
          normal equations of the one refit, a 3x3 SVD per pair for the stored F — plumbing around the kernels
  host    gathering matched keypoints from the database, writing the rows (rank 0 only in a multi-GPU run)
All pairs are verified in one batch: nothing loops over pairs on the device side.
"""
from functools import partial

import numpy as np
import torch

from .. import _lib
from ..database.colmap_db import pair_id_of
from . import essential
from ._common import (CONFIG_CALIBRATED, CONFIG_DEGENERATE, CONFIG_PANORAMIC, CONFIG_PLANAR,  # noqa: F401 - re-exported
                      CONFIG_PLANAR_OR_PANORAMIC, CONFIG_UNCALIBRATED, CONFIG_UNDEFINED, MAX_ERROR, MAX_H_INLIER_RATIO,
                      MIN_INLIER_RATIO, MIN_NUM_INLIERS, MODEL_CODE, NUM_CANDIDATES, NUM_HYP_F, NUM_HYP_H, SALT, _mask,
                      _pair_batch, _ransac_tail, _sample_indices, _score)
from .essential import MIN_E_F_INLIER_RATIO, camera_table, choose_pose
from .pose import relative_poses


def _rows(model, x1, y1, x2, y2):
    """Equations of the parametrisation with the last matrix entry fixed to 1: A (..., n_eq, 8), b (..., n_eq)."""
    if model == "F":
        return torch.stack([x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1], dim=-1), -torch.ones_like(x1)
    z, o = torch.zeros_like(x1), torch.ones_like(x1)
    ax = torch.stack([x1, y1, o, z, z, z, -x2 * x1, -x2 * y1], dim=-1)
    ay = torch.stack([z, z, z, x1, y1, o, -y2 * x1, -y2 * y1], dim=-1)
    return torch.cat([ax, ay], dim=-2), torch.cat([x2, y2], dim=-1)


def _to_matrix(f8):
    return torch.cat([f8, torch.ones(f8.shape[:-1] + (1,), dtype=f8.dtype, device=f8.device)], dim=-1).reshape(f8.shape[:-1] + (3, 3))


def _denormalise(model, Mn, T1, T2):
    """Mn (P, K, 3, 3) in normalised coordinates -> pixel coordinates."""
    if model == "F":
        return T2.transpose(-1, -2)[:, None] @ Mn @ T1[:, None]
    return torch.linalg.inv(T2)[:, None] @ Mn @ T1[:, None]


def _hypotheses(model, pts, offsets, pair_of, seeds, n_hyp):
    """The hypothesis half of `_estimate`, all pairs at once -> hypotheses float32 (P, n_hyp, 9) in pixel coordinates (NaN
    rows for void samples and singular systems), the sample indices int64 (P, n_hyp, S) into each pair's own list (-1 where
    void) and the normalisation (T1, T2, n1, n2) that the refit works in."""
    dev = pts.device
    P = offsets.shape[0] - 1
    M = (offsets[1:] - offsets[:-1]).to(torch.int64)
    S = 8 if model == "F" else 4
    p64 = pts.to(torch.float64)

    def norm_T(xy):      # per pair: x~ = (x - mean) * sqrt(2) / mean distance
        ones = torch.ones(xy.shape[0], dtype=torch.float64, device=dev)
        cnt = torch.zeros(P, dtype=torch.float64, device=dev).index_add_(0, pair_of, ones).clamp(min=1)
        mu = torch.zeros((P, 2), dtype=torch.float64, device=dev).index_add_(0, pair_of, xy) / cnt[:, None]
        dist = torch.sqrt(((xy - mu[pair_of]) ** 2).sum(dim=1))
        md = torch.zeros(P, dtype=torch.float64, device=dev).index_add_(0, pair_of, dist) / cnt
        s = torch.where(md > 0, np.sqrt(2.0) / md, torch.ones_like(md))
        T = torch.zeros((P, 3, 3), dtype=torch.float64, device=dev)
        T[:, 0, 0] = s
        T[:, 1, 1] = s
        T[:, 0, 2] = -s * mu[:, 0]
        T[:, 1, 2] = -s * mu[:, 1]
        T[:, 2, 2] = 1.0
        return T

    T1, T2 = norm_T(p64[:, :2]), norm_T(p64[:, 2:])
    n1 = p64[:, :2] * T1[pair_of, 0, 0][:, None] + T1[pair_of, :2, 2]
    n2 = p64[:, 2:] * T2[pair_of, 0, 0][:, None] + T2[pair_of, :2, 2]

    idx = _sample_indices(seeds, M, n_hyp, S, SALT[model])                    # (P, K, S) into the pair's own list
    void = idx[:, :, 0] < 0
    g = (idx.clamp(min=0) + offsets[:-1].to(torch.int64)[:, None, None]).clamp(max=max(pts.shape[0] - 1, 0))
    A, b = _rows(model, n1[g, 0], n1[g, 1], n2[g, 0], n2[g, 1])              # (P, K, 8, 8), (P, K, 8)
    sol = torch.linalg.solve_ex(A, b.unsqueeze(-1)).result.squeeze(-1)        # singular systems give inf / nan
    hyp = _denormalise(model, _to_matrix(sol), T1, T2).reshape(P, n_hyp, 9)
    hyp = torch.where(void[:, :, None] | ~torch.isfinite(sol).all(dim=-1, keepdim=True), torch.full_like(hyp, float("nan")), hyp)
    return hyp.to(torch.float32).contiguous(), idx, (T1, T2, n1, n2)


def _estimate(model, pts, offsets, pair_of, seeds, n_hyp, max_error):
    """All pairs at once -> best model float32 (P, 9) (NaN where none), inlier mask bool (total,), counts int64 (P,)."""
    dev = pts.device
    P = offsets.shape[0] - 1
    S = 8 if model == "F" else 4
    hyp32, _, (T1, T2, n1, n2) = _hypotheses(model, pts, offsets, pair_of, seeds, n_hyp)
    score = partial(_score, pts, offsets, model=model, max_error=max_error)
    counts = score(hyp32).to(torch.int64)
    Ar, br = _rows(model, n1[:, 0], n1[:, 1], n2[:, 0], n2[:, 1])             # F: (total, 8); H: (2 total, 8) stacked x then y

    def refit(mask, nbest):
        # over the inliers of the best hypothesis: normal equations per pair (float64)
        if model == "H":
            w = torch.cat([mask, mask]).to(torch.float64)
            seg = torch.cat([pair_of, pair_of])
        else:
            w, seg = mask.to(torch.float64), pair_of
        AtA = torch.zeros((P, 8, 8), dtype=torch.float64, device=dev).index_add_(0, seg, (Ar[:, :, None] * Ar[:, None, :]) * w[:, None, None])
        Atb = torch.zeros((P, 8), dtype=torch.float64, device=dev).index_add_(0, seg, Ar * (br * w)[:, None])
        rsol = torch.linalg.solve_ex(AtA, Atb.unsqueeze(-1)).result.squeeze(-1)
        refit = _denormalise(model, _to_matrix(rsol)[:, None], T1, T2).reshape(P, 9)
        ok = torch.isfinite(rsol).all(dim=-1) & (nbest >= S)
        return torch.where(ok[:, None], refit, torch.full_like(refit, float("nan"))).to(torch.float32).contiguous(), ok

    return _ransac_tail(hyp32, counts, score, partial(_mask, pts, offsets, model=model, max_error=max_error), refit)[:3]


def _stored_f(f9):
    """float32 (9,) -> the closest rank-2 matrix at unit Frobenius norm, float64 (3, 3)."""
    U, sv, Vt = np.linalg.svd(np.nan_to_num(np.asarray(f9, np.float64)).reshape(3, 3))
    F2 = U @ np.diag([sv[0], sv[1], 0.0]) @ Vt
    n = np.linalg.norm(F2)
    return F2 / n if n > 0 else F2


def _estimate_calibrated(cal, sel, pts_np, pair_images, pair_ids, cameras, device, max_error):
    """The E estimate of the chunk's calibrated pairs `cal` (positions in `sel`) as one batch of their own
    -> {position: dict(n, E, f9, mask, xn)} (matching/essential.py)."""
    K, _ = cameras
    rows = [pts_np[q] for q in cal]
    offs = np.cumsum([0] + [len(r) for r in rows])
    pts, offsets, pair_of, seeds = _pair_batch(rows, [pair_ids[sel[q]] for q in cal], device)
    K1 = torch.from_numpy(np.stack([K[pair_images[sel[q]][0]] for q in cal]).astype(np.float64)).to(device)
    K2 = torch.from_numpy(np.stack([K[pair_images[sel[q]][1]] for q in cal]).astype(np.float64)).to(device)
    with torch.cuda.device(pts.device):
        E, f9, mask, n, xn = essential.estimate_e(pts, offsets, pair_of, seeds, K1, K2, essential.NUM_HYP_E, max_error)
    E, f9, mask, n, xn = E.cpu().numpy(), f9.cpu().numpy(), mask.cpu().numpy(), n.cpu().numpy(), xn.cpu().numpy()
    return {q: dict(n=int(n[j]), E=E[j], f9=f9[j], mask=mask[offs[j]:offs[j + 1]], xn=xn[offs[j]:offs[j + 1]])
            for j, q in enumerate(cal)}


def _relative_poses(posed, sel, results, pair_images, cameras, est_e, device, max_error):
    """Relative pose of the chunk's qualifying pairs `posed` [(position in `sel`, inlier mask)] as one batch (matching/pose.py):
    a PLANAR_OR_PANORAMIC pair is decomposed from its H, any other from E where the best model is E, else from its F."""
    entries = []
    for q, mask in posed:
        r = results[sel[q]]
        a, b = pair_images[sel[q]]
        if r["config"] == CONFIG_PLANAR_OR_PANORAMIC:
            kind, matrix = "H", r["H"]
        elif "E" in r:
            kind, matrix = "E", r["E"]
        else:
            kind, matrix = "F", np.asarray(r["model9"], np.float64).reshape(3, 3)
        entries.append(dict(config=r["config"], kind=kind, matrix=matrix, K1=cameras[0][a], K2=cameras[0][b],
                            xn=est_e[q]["xn"][mask]))
    for (q, _), pose in zip(posed, relative_poses(entries, device, max_error)):
        results[sel[q]].update(pose)


def pair_decision(M, n_f, n_h, n_e=None):
    """The rule for one pair, on the numbers alone: M putative matches, the inlier counts of its F and H and, where both
    cameras have a usable prior, of its E (None: not estimated) -> (config, best, model).  `best` is the two-view model that
    reaches max(15, 0.25 M) inliers — "E" where n_e also reaches 0.95 n_f, else "F"; (DEGENERATE, None, None) where neither
    does.  With n the count of `best`: n_h / n > 0.8 makes the pair PLANAR_OR_PANORAMIC, and n_h > n hands the inliers to H.
    `model` ("F" or "H") is the model whose mask gives `inlier_matches`: H's, or that of `best` (E's mask is that of its
    pixel F)."""
    floor = max(MIN_NUM_INLIERS, MIN_INLIER_RATIO * M)
    if n_e is not None and n_e >= floor and n_e >= MIN_E_F_INLIER_RATIO * n_f:
        best, n, config = "E", n_e, CONFIG_CALIBRATED
    elif n_f >= floor:
        best, n, config = "F", n_f, CONFIG_UNCALIBRATED
    else:
        return CONFIG_DEGENERATE, None, None
    if n_h / n > MAX_H_INLIER_RATIO:
        config = CONFIG_PLANAR_OR_PANORAMIC
    return config, best, "H" if n_h > n else "F"


@torch.no_grad()
def verify_pairs(keypoints, pair_images, pair_ids, match_lists, device="cuda", num_f=NUM_HYP_F, num_h=NUM_HYP_H,
                 max_error=MAX_ERROR, chunk_pairs: int = 1024, cameras=None, relative_pose=False):
    """keypoints: dict image index -> float32 (N, >= 2); pair_images: list of (a, b); pair_ids: COLMAP pair ids;
    match_lists: list of uint32 (M, 2).  -> list of dict(config, inlier_matches, F, H, n_f, n_h), one per pair.
    A result that is not DEGENERATE also carries the model whose mask produced `inlier_matches` — `model` ("F" or "H") and
    `model9` (float32 (9,), row-major; NOT the stored rank-2 F): what guided matching re-matches the pair under.
    `cameras`: None, or (K float64 (n, 3, 3), prior (n,)) indexed like `keypoints` (essential.camera_table).  A pair whose
    two images have a usable focal-length prior also gets an essential-matrix estimate (`n_e`); where it reaches
    max(15, 0.25 M) and 0.95 n_f inliers the best model is E: config CALIBRATED (or PLANAR_OR_PANORAMIC by the H rule on
    n_e), `E`, `qvec`, `tvec`, F from E, `model` "F" with `model9` the pixel F of E.  Every other pair: exactly as without.
    `relative_pose` (needs `cameras`): every pair with two usable priors that is not DEGENERATE gets `qvec`,
    `tvec`, `tri_angle` (rad) and `n_front` from the triangulation of its inliers under the pose candidates of its model
    (matching/pose.py), and PLANAR_OR_PANORAMIC becomes PLANAR or PANORAMIC; E, F, H, `inlier_matches`, `model` and `model9`
    are as without."""
    if not torch.cuda.is_available():
        raise _lib.HipLibraryError("geometric verification scores its hypotheses on the GPU (no CPU fallback)")
    results = [dict(config=CONFIG_DEGENERATE, inlier_matches=np.zeros((0, 2), np.uint32), F=np.zeros((3, 3)),
                    H=np.zeros((3, 3)), n_f=0, n_h=0) for _ in pair_images]
    todo = [i for i, m in enumerate(match_lists) if len(m) >= MIN_NUM_INLIERS]
    for c0 in range(0, len(todo), chunk_pairs):
        sel = todo[c0:c0 + chunk_pairs]
        pts_np = []
        for i in sel:
            a, b = pair_images[i]
            m = np.asarray(match_lists[i], np.int64).reshape(-1, 2)
            pts_np.append(np.concatenate([keypoints[a][m[:, 0], :2], keypoints[b][m[:, 1], :2]], axis=1).astype(np.float32))
        offs = np.cumsum([0] + [len(p) for p in pts_np])
        pts, offsets, pair_of, seeds = _pair_batch(pts_np, [pair_ids[i] for i in sel], device)
        P = len(sel)
        with torch.cuda.device(pts.device):
            f9, fmask, nf = _estimate("F", pts, offsets, pair_of, seeds, num_f, max_error)
            h9, hmask, nh = _estimate("H", pts, offsets, pair_of, seeds, num_h, max_error)
            # stored F: closest rank-2 matrix, unit Frobenius norm
            F = torch.nan_to_num(f9.to(torch.float64)).reshape(P, 3, 3)
            U, s, Vt = torch.linalg.svd(F)
            s = s.clone()
            s[:, 2] = 0
            F2 = U @ torch.diag_embed(s) @ Vt
            nrm = torch.linalg.norm(F2.reshape(P, 9), dim=1).clamp(min=1e-300)
            F2 = (F2 / nrm[:, None, None]).cpu().numpy()
        H = torch.nan_to_num(h9.to(torch.float64)).reshape(P, 3, 3).cpu().numpy()
        fmask, hmask, nf, nh = fmask.cpu().numpy(), hmask.cpu().numpy(), nf.cpu().numpy(), nh.cpu().numpy()
        f9_np, h9_np = f9.cpu().numpy(), h9.cpu().numpy()
        cal = [] if cameras is None else [q for q, i in enumerate(sel) if cameras[1][pair_images[i][0]] and cameras[1][pair_images[i][1]]]
        posed = []
        est_e = _estimate_calibrated(cal, sel, pts_np, pair_images, pair_ids, cameras, device, max_error) if cal else {}
        for q, i in enumerate(sel):
            r, e = results[i], est_e.get(q)
            r["n_f"], r["n_h"] = int(nf[q]), int(nh[q])
            if e is not None:
                r["n_e"] = e["n"]
            config, best, model = pair_decision(len(match_lists[i]), r["n_f"], r["n_h"], r.get("n_e"))
            if best is None:
                continue
            lo, hi = offs[q], offs[q + 1]
            r["config"], r["model"] = config, model
            r["H"] = H[q] / H[q][2, 2] if H[q][2, 2] != 0 else H[q]
            if best == "E":
                r["E"], r["F"] = e["E"], _stored_f(e["f9"])
                mask, m9 = e["mask"], e["f9"]
            else:
                r["F"] = F2[q]
                mask, m9 = fmask[lo:hi], f9_np[q]
            if model == "H":
                mask, m9 = hmask[lo:hi], h9_np[q]
            r["model9"] = m9.copy()
            r["inlier_matches"] = np.asarray(match_lists[i], np.uint32).reshape(-1, 2)[mask]
            if relative_pose and e is not None:
                posed.append((q, mask))
            elif best == "E":
                r["qvec"], r["tvec"] = choose_pose(e["E"], e["xn"][e["mask"]])
        if posed:
            _relative_poses(posed, sel, results, pair_images, cameras, est_e, device, max_error)
    return results


def read_keypoints_by_index(db, ids):
    """{image index: float32 (N, >= 2)} for every image of `ids` (empty array where the database has no keypoints)."""
    kps = {}
    for k, image_id in enumerate(ids):
        kp = None if image_id is None else db.read_keypoints(image_id)
        kps[k] = np.zeros((0, 2), np.float32) if kp is None else np.asarray(kp, np.float32)
    return kps


def verify_pair_lists(kps, ids, pairs, lists, device="cuda", verify_fn=None, cameras=None, relative_pose=False):
    """This rank's share of the verification: pairs (P, 2) image indices with their match lists -> one result dict per
    pair (verify_pairs' format).  The sampler is seeded by the COLMAP pair id, so a pair's result does not depend on the
    rank that verifies it.  `verify_fn(kps, pair_images, pair_ids, lists)` replaces verify_pairs in the CPU tests.
    `cameras` (verify_pairs' form) is handed on, to `verify_fn` as the keyword `cameras=`, only when some pair of this
    share has a usable prior on both images; `relative_pose=True` likewise, only when the option is on and
    the cameras are handed on."""
    pair_images = [(int(a), int(b)) for a, b in pairs]
    pids = [pair_id_of(ids[a], ids[b]) for a, b in pair_images]
    if cameras is not None and not any(cameras[1][a] and cameras[1][b] for a, b in pair_images):
        cameras = None
    extra = {} if cameras is None else dict(cameras=cameras)
    if relative_pose and cameras is not None:
        extra["relative_pose"] = True
    if verify_fn is not None:
        return verify_fn(kps, pair_images, pids, lists, **extra)
    return verify_pairs(kps, pair_images, pids, lists, device=device, **extra)


def write_two_view_rows(db, ids, results) -> int:
    """results {(a, b): verify_pairs result} -> two_view_geometries rows in pair order (one per matched pair, as COLMAP
    does [recalled]: pairs that fail keep config DEGENERATE and zero inlier rows).  Returns the number of verified pairs."""
    n_ok = 0
    for (a, b) in sorted(results):
        r = results[(a, b)]
        db.write_two_view_geometry(ids[a], ids[b], r["inlier_matches"], r["config"], F=r["F"], E=r.get("E"), H=r["H"],
                                   qvec=r.get("qvec"), tvec=r.get("tvec"), commit=False)
        n_ok += r["config"] != CONFIG_DEGENERATE
    db.commit()
    return int(n_ok)


def verify_database_pairs(db, ids, merged, device="cuda", verify_fn=None, relative_pose=False) -> int:
    """Single-process form: verify every matched pair of a database that is open for writing and write its rows (a row that
    is there already is replaced).  `merged`: {(a, b): uint32 (M, 2)} with a < b image indices into `ids`; `relative_pose` as
    verify_pair_lists takes it.  Returns the number of verified pairs."""
    pairs = sorted(merged)
    res = verify_pair_lists(read_keypoints_by_index(db, ids), ids, pairs, [merged[p] for p in pairs], device=device,
                            verify_fn=verify_fn, cameras=camera_table(db, ids), relative_pose=relative_pose)
    return write_two_view_rows(db, ids, dict(zip(pairs, res)))
