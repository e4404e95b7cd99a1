"""Exhaustive matching over a COLMAP database — the DB-in / DB-out contract of
`pycolmap.match_exhaustive(database_path=..., matching_options=... | sift_options=...)` that the
reference calls at vit_colmap/pipeline/run_pipeline.py:351-363, on the HIP matcher.

Reads every image's uint8 descriptors, matches all unordered pairs (a < b in image-id order) on
the GPU, and writes one `matches` row per pair (also when it is empty, as COLMAP does [recalled]).
With `verify=True` (default) the match lists are then geometrically verified (matching/two_view.py) and
`two_view_geometries` rows written, as `match_exhaustive` does inside COLMAP.
With the `guided_matching` option (off by default) every pair whose verification is not DEGENERATE is matched once more
under its estimated F or H and that list replaces the pair's inlier matches.
With the `compute_relative_pose` option (off by default) the verified pairs whose cameras have a focal-length prior get a
pose and a triangulation angle, and PLANAR_OR_PANORAMIC is split into PLANAR and PANORAMIC.

Multi-GPU (`distributed=True`, or automatically when a torch.distributed group with more than one rank exists):
rank 0 reads the database and broadcasts the descriptor blocks, the pair list is dealt round-robin over the
ranks, every rank matches its share on its own GPU, the lists are gathered to rank 0 and rank 0 alone writes
(vit_colmap_amd/dist.py).
"""
import logging
import time
from dataclasses import dataclass
from functools import partial

import numpy as np
import torch

from .. import _lib
from .. import dist as vd
from ..database.colmap_db import SqliteColmapDatabase
from ..utils.config import MatchingConfig
from .essential import camera_table
from .hip_matcher import (MODEL_KIND, exhaustive_pairs, match_pairs, match_pairs_blocked, match_pairs_guided,
                          prepare_descriptors)
from .two_view import (CONFIG_DEGENERATE, CONFIG_PANORAMIC, CONFIG_PLANAR, MAX_ERROR, read_keypoints_by_index,
                       verify_pair_lists, write_two_view_rows)
from .undistort import drop_invalid_matches, undistort_for_matching

logger = logging.getLogger(__name__)


def _sift_options(matching_options, sift_options):
    opts = matching_options if matching_options is not None else sift_options
    if opts is None:
        opts = MatchingConfig().to_matching_options()
    return getattr(opts, "sift", opts)  # FeatureMatchingOptions(.sift) or SiftMatchingOptions


def _guided_option(matching_options, sift_options) -> bool:
    """`guided_matching` of the options object: on the outer object (pycolmap 3.13) or on its SIFT options (3.12)."""
    opts = matching_options if matching_options is not None else sift_options
    return bool(getattr(opts, "guided_matching", False) or getattr(getattr(opts, "sift", None), "guided_matching", False))


def _relative_pose_option(matching_options, sift_options) -> bool:
    """`compute_relative_pose` of the options object, looked up where `guided_matching` is."""
    opts = matching_options if matching_options is not None else sift_options
    return bool(getattr(opts, "compute_relative_pose", False) or getattr(getattr(opts, "sift", None), "compute_relative_pose", False))


def _known_distortion_option(matching_options, sift_options) -> bool:
    """`known_distortion` of the options object, looked up where `guided_matching` is."""
    opts = matching_options if matching_options is not None else sift_options
    return bool(getattr(opts, "known_distortion", False) or getattr(getattr(opts, "sift", None), "known_distortion", False))


@dataclass(frozen=True)
class MatchSettings:
    """What a run reads from its options objects, looked up once."""
    max_ratio: float
    max_distance: float
    cross_check: bool
    guided: bool            # the options' guided_matching; needs `verify`
    relative_pose: bool     # the options' compute_relative_pose; needs `verify`
    known_distortion: bool = False   # the options' known_distortion; needs `verify`

    @classmethod
    def from_options(cls, matching_options=None, sift_options=None, verify: bool = True):
        sift = _sift_options(matching_options, sift_options)
        return cls(float(sift.max_ratio), float(sift.max_distance), bool(sift.cross_check),
                   verify and _guided_option(matching_options, sift_options),
                   verify and _relative_pose_option(matching_options, sift_options),
                   verify and _known_distortion_option(matching_options, sift_options))


def new_stats(images: int, pairs: int, ranks: int) -> dict:
    """The stats dict of a matching run before anything is matched."""
    return dict(images=images, pairs=pairs, matches=0, gpu_s=0.0, db_s=0.0, verified_pairs=0, ranks=ranks, guided_pairs=0,
                **pose_stats(()))


def pose_stats(results) -> dict:
    """The relative-pose totals of a run's results (an iterable of verify_pairs results)."""
    posed = [r for r in results if "tri_angle" in r]
    angles = [r["tri_angle"] for r in posed if r["config"] != CONFIG_PANORAMIC and r["n_front"] > 0]
    return dict(pose_pairs=len(posed), planar_pairs=sum(r["config"] == CONFIG_PLANAR for r in posed),
                panoramic_pairs=sum(r["config"] == CONFIG_PANORAMIC for r in posed),
                median_tri_angle_deg=float(np.degrees(np.median(angles))) if angles else 0.0)


def load_descriptor_blocks(db: SqliteColmapDatabase):
    """-> image ids (ascending), uint8 [n_images][n_max][D] (zero padded), counts int32."""
    images = db.read_all_images()
    ids = [im.image_id for im in images]
    descs = [db.read_descriptors(i) for i in ids]
    dims = {d.shape[1] for d in descs if d is not None and d.shape[0] > 0}
    if len(dims) > 1:
        raise ValueError(f"images have descriptors of different dimensions: {sorted(dims)}")
    D = dims.pop() if dims else 0
    counts = np.array([0 if d is None else d.shape[0] for d in descs], np.int32)
    n_max = int(counts.max()) if len(counts) else 0
    block = np.zeros((len(ids), max(n_max, 1), max(D, 1)), np.uint8)
    for k, d in enumerate(descs):
        if d is not None and d.shape[0] > 0:
            block[k, : d.shape[0]] = d
    return ids, block, counts, D


def _upload_blocks(block, counts, device, what):
    """uint8 blocks [n][n_max][D] + counts (host or device) -> both on `device`, checked against the kernels' limits."""
    if not torch.cuda.is_available():
        raise _lib.HipLibraryError(f"{what} is HIP-only (no CPU fallback): no GPU visible")
    d_desc = block if torch.is_tensor(block) else torch.from_numpy(np.ascontiguousarray(block))
    d_counts = counts if torch.is_tensor(counts) else torch.from_numpy(np.ascontiguousarray(counts, np.int32))
    if d_desc.shape[2] > _lib.VC_MAX_DESC_DIM:
        raise _lib.HipLibraryError(f"descriptors of {d_desc.shape[2]} bytes exceed the kernels' limit ({_lib.VC_MAX_DESC_DIM})")
    return d_desc.to(device), d_counts.to(device)


def _unpack_chunk(m, c, first_pair, what):
    """One launch's (matches [P, n_max, 2], counts [P]) on the device -> list of P uint32 (M, 2) host arrays."""
    c_np = c.cpu().numpy()
    if (c_np < 0).any():   # VC_COUNT_SELFCHECK_FAILED: the kernel's cursor check (include/vitcolmap_hip.h) — never a result
        bad = np.nonzero(c_np < 0)[0][:8] + first_pair
        raise _lib.HipLibraryError(f"{what}: consistency check failed for pairs {bad.tolist()}")
    m_np = m.cpu().numpy().view(np.uint32)
    return [m_np[p, : c_np[p]].copy() for p in range(len(c_np))]


def hip_match_blocks(block, counts, pairs, max_ratio=0.8, max_distance=0.7, cross_check=True, device="cuda",
                     pair_chunk: int = 16384):
    """uint8 blocks [n][n_max][D] + counts (host or device) and pairs int32 (P, 2) (host) -> list of P uint32 (M, 2)
    match lists, on the HIP matcher.  Blocks with more rows than one kernel block holds (VC_MAX_KEYPOINTS) are
    matched in row / column sub-blocks whose top-2 results are merged (hip_matcher.match_pairs_blocked)."""
    d_desc, d_counts = _upload_blocks(block, counts, device, "the matcher")
    n, n_max, D = d_desc.shape
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    if n_max > _lib.VC_MAX_KEYPOINTS:
        return match_pairs_blocked(d_desc, d_counts, pairs, max_ratio, max_distance, cross_check)
    prepared = prepare_descriptors(d_desc, d_counts)
    out = []
    for s in range(0, len(pairs), pair_chunk):
        chunk = torch.from_numpy(pairs[s:s + pair_chunk]).to(device)
        m, c = match_pairs(prepared, d_counts, n, n_max, D, chunk, max_ratio, max_distance, cross_check)
        out.extend(_unpack_chunk(m, c, s, "vc_match_pairs_u8"))
    return out


def check_guided_block_size(n_max: int):
    """Guided matching runs in one kernel block per image; the sub-blocked path of larger images is unguided only."""
    if n_max > _lib.VC_MAX_KEYPOINTS:
        raise _lib.HipLibraryError(f"guided matching needs at most VC_MAX_KEYPOINTS = {_lib.VC_MAX_KEYPOINTS} keypoints per "
                                   f"image (the largest image has {n_max})")


def hip_guided_blocks(block, counts, keypoints_xy, pairs, models, kinds, max_error, max_ratio=0.8, max_distance=0.7,
                      cross_check=True, device="cuda", pair_chunk: int = 16384):
    """Guided matching of `pairs` (P, 2) on the HIP matcher: uint8 blocks [n][n_max][D] + counts, keypoints float32
    [n][>= 1][2] (zero padded), models float32 (P, 9), kinds list of "F" / "H" -> list of P uint32 (M, 2) match lists."""
    d_desc, d_counts = _upload_blocks(block, counts, device, "guided matching")
    n, n_max, D = d_desc.shape
    check_guided_block_size(n_max)
    kp = np.asarray(keypoints_xy, np.float32)
    kp_block = np.zeros((n, n_max, 2), np.float32)                        # the kernel's layout: one row per descriptor row
    rows = min(n_max, kp.shape[1])
    kp_block[:, :rows] = kp[:, :rows, :2]
    d_kp = torch.from_numpy(kp_block).to(device)
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    models = np.ascontiguousarray(models, np.float32).reshape(-1, 9)
    kind = np.array([MODEL_KIND[k] for k in kinds], np.int32)
    prepared = prepare_descriptors(d_desc, d_counts)
    out = []
    for s in range(0, len(pairs), pair_chunk):
        sl = slice(s, s + pair_chunk)
        m, c = match_pairs_guided(prepared, d_counts, n, n_max, D, d_kp, torch.from_numpy(pairs[sl]).to(device),
                                  torch.from_numpy(models[sl]).to(device), torch.from_numpy(kind[sl]).to(device), max_error,
                                  max_ratio, max_distance, cross_check)
        out.extend(_unpack_chunk(m, c, s, "vc_match_pairs_guided_u8"))
    return out


def rematch_guided(block, counts, keypoints_xy, pairs, results, max_ratio, max_distance, cross_check, guided_fn) -> int:
    """The guided pass over one rank's share: every result of `results` (verify_pairs' format, parallel to `pairs`) that is
    not DEGENERATE has its `inlier_matches` replaced by the list matched under the model that produced them (`model`,
    `model9`), with the verifier's own error bound.  Returns the number of pairs re-matched."""
    sel = [i for i, r in enumerate(results) if r["config"] != CONFIG_DEGENERATE]
    if not sel:
        return 0
    missing = [i for i in sel if results[i].get("model") not in ("F", "H") or results[i].get("model9") is None]
    if missing:
        raise ValueError("guided matching needs `model` and `model9` in every verified result "
                         f"(missing for pairs {[tuple(map(int, pairs[i])) for i in missing[:8]]})")
    models = np.stack([np.asarray(results[i]["model9"], np.float32).reshape(9) for i in sel])
    kinds = [results[i]["model"] for i in sel]
    lists = guided_fn(block, counts, keypoints_xy, np.asarray(pairs, np.int32).reshape(-1, 2)[sel], models, kinds, MAX_ERROR,
                      max_ratio, max_distance, cross_check)
    for i, lst in zip(sel, lists):
        results[i]["inlier_matches"] = np.asarray(lst, np.uint32).reshape(-1, 2)
    return len(sel)


def _pack_keypoints(kps: dict, n: int):
    """{index: (N, >= 2)} -> float32 (n, max N, 2) zero padded + int32 counts: the form that travels between ranks."""
    cnt = np.array([len(kps[k]) for k in range(n)], np.int32)
    out = np.zeros((n, max(int(cnt.max()) if n else 0, 1), 2), np.float32)
    for k in range(n):
        out[k, : cnt[k]] = kps[k][:, :2]
    return out, cnt


def _unpack_keypoints(arr, cnt):
    return {k: arr[k, : cnt[k]] for k in range(len(cnt))}


def match_exhaustive(database_path: str, matching_options=None, sift_options=None, device="cuda",
                     pair_chunk: int = 16384, distributed=None, match_fn=None, verify: bool = True, verify_fn=None,
                     guided_fn=None, undistort_fn=None) -> dict:
    """Returns a small stats dict (pairs, matches, seconds); the result proper is in the database.
    Multi-rank (`distributed`): rank 0 — the only process that touches the SQLite file — reads descriptors and keypoints
    and broadcasts them; EVERY rank matches and geometrically verifies its share of the pair list (pair p -> rank
    p % world); match lists and two-view geometries are gathered to rank 0, which writes them in pair order.  An error
    on any rank (e.g. rank 0's database) is raised on all of them (dist.raise_if_any_failed).
    `match_fn(block, counts, pairs, max_ratio, max_distance, cross_check) -> list of match lists` and
    `verify_fn(keypoints, pair_images, pair_ids, lists) -> list of results` replace the HIP matcher / scorer (the CPU
    tests of the multi-rank path pass the oracles; the product never does).
    Calibrated pairs: rank 0 reads every image's camera and broadcasts a (3, 3) K and a usable-prior flag
    per image next to the keypoints; a pair with the prior on both images is also verified under an essential matrix
    (`verify_fn` then gets the keyword `cameras=(K, prior)`).
    Guided matching (the options' `guided_matching`, off by default; needs `verify`): after verification each rank
    re-matches the non-degenerate pairs of its own share under their models and the lists replace those pairs'
    `inlier_matches` (rematch_guided); `matches`, `config`, F and H are untouched.  `guided_fn(block, counts, keypoints_xy,
    pairs, models, kinds, max_error, max_ratio, max_distance, cross_check) -> list of match lists` replaces
    hip_guided_blocks in the CPU tests.
    Relative pose (the options' `compute_relative_pose`, off by default; needs `verify` and usable priors):
    `verify_fn` then also gets the keyword `relative_pose=True`; the stats gain `pose_pairs`, `planar_pairs`,
    `panoramic_pairs` and `median_tri_angle_deg` (over the posed pairs that are not PANORAMIC).
    Known distortion (the options' `known_distortion`, off by default; needs `verify`): rank 0 replaces the
    keypoints of every image whose camera is flagged and distorted by their undistorted pixels (one launch of
    vc_undistort_points) and gives the image a usable prior, so F, H, E, the relative pose and guided matching see an ideal
    pinhole camera; the matches that touch a keypoint that does not invert reach neither the verifier nor the guided lists
    (their number is logged and in the stats as `undistort_dropped_matches`), the `matches` table keeps the raw lists,
    `inlier_matches` stay keypoint indices and the stored F and H relate undistorted pixels.  `undistort_fn(xy, cam, cams,
    device) -> (xy64, valid)` on numpy arrays replaces the launch in the CPU tests."""
    return match_database(database_path, matching_options, sift_options, device, pair_chunk, distributed, match_fn, verify,
                          verify_fn, guided_fn, undistort_fn=undistort_fn)


def match_database(database_path, matching_options, sift_options, device, pair_chunk, distributed, match_fn, verify,
                   verify_fn, guided_fn, select_pairs=None, what="match_exhaustive", undistort_fn=None) -> dict:
    """The database-in / database-out entry that match_exhaustive and matching.retrieval.match_retrieval share; they differ
    only in where the pair list comes from.  `select_pairs` None: every pair (a < b), dealt to the ranks by
    dist.pairs_for_rank.  Otherwise rank 0 calls `select_pairs(block, counts, stats)` once the descriptor blocks are
    loaded -> int32 (P, 2) image-index pairs, a < b, ascending (a sub-sequence of the exhaustive list; it may add keys
    to `stats`); the list is broadcast, pair p goes to rank p % world (dist.listed_pairs_for_rank), and only the listed
    pairs are matched, verified and written.  This function reads and broadcasts; match_loaded does the rest."""
    settings = MatchSettings.from_options(matching_options, sift_options, verify)
    if distributed is None:
        distributed = vd.is_distributed()
    if distributed and not vd.is_distributed():
        raise RuntimeError("distributed=True needs an initialised torch.distributed process group with > 1 rank")
    rank, world = vd.rank_world() if distributed else (0, 1)
    if not torch.cuda.is_available() and (match_fn is None or (settings.guided and guided_fn is None)):
        raise _lib.HipLibraryError(f"{what} needs an MI355X: the matcher is HIP-only (no CPU fallback)")
    t0 = time.perf_counter()
    db = None

    def read():                                                                # rank 0 is the only reader and writer
        nonlocal db
        db = SqliteColmapDatabase(str(database_path))
        ids, block, counts, D = load_descriptor_blocks(db)
        kp_arr = kp_cnt = cam_k = cam_prior = None
        if verify and D != 0:
            kp_arr, kp_cnt = _pack_keypoints(read_keypoints_by_index(db, ids), len(ids))
            if settings.known_distortion:                                      # undistorted pixels, a prior for their images (§4.2l)
                cam_k, cam_prior = camera_table(db, ids, warn_distorted=False)
                kp_arr, cam_k, cam_prior = undistort_for_matching(db, ids, kp_arr, kp_cnt, cam_k, cam_prior, device, undistort_fn)
            else:
                cam_k, cam_prior = camera_table(db, ids)                       # focal-length priors
            if settings.relative_pose and not cam_prior.any():
                logger.warning("compute_relative_pose is set and no camera has a usable focal-length prior: it has no effect")
        return ids, D, [block, counts, kp_arr, kp_cnt, cam_k, cam_prior]

    try:
        ids, D, arrays = vd.run_guarded(read, "reading the database", distributed) or (None, None, [None] * 6)
        if distributed:
            ids, D = vd.broadcast_object((ids, D), 0)
            k = 6 if verify and D != 0 else 2                                  # keypoints and cameras travel where they are used
            arrays = [vd.broadcast_array(a, 0, device) for a in arrays[:k]] + arrays[k:]
        block, counts, kp_arr, kp_cnt, cam_k, cam_prior = arrays
        n = len(ids)
        stats = new_stats(n, n * (n - 1) // 2, world)
        if n < 2:
            return stats
        if select_pairs is None:
            all_pairs = exhaustive_pairs(n).numpy()
            my_pairs = vd.pairs_for_rank(n, rank, world)
        else:
            all_pairs = vd.run_guarded(lambda: np.ascontiguousarray(select_pairs(block, counts, stats), np.int32).reshape(-1, 2),
                                       "selecting the pairs", distributed)
            if distributed:
                all_pairs = vd.broadcast_array(all_pairs, 0, device)
            my_pairs = vd.listed_pairs_for_rank(all_pairs, rank, world)
            stats["pairs"] = len(all_pairs)
        stats = match_loaded(ids, block, counts, kp_arr, kp_cnt, (cam_k, cam_prior), all_pairs, my_pairs, settings, verify,
                             db, stats, match_fn=match_fn, verify_fn=verify_fn, guided_fn=guided_fn, device=device,
                             pair_chunk=pair_chunk, distributed=distributed, skip_empty_share=select_pairs is not None)
        stats["total_s"] = time.perf_counter() - t0
        logger.info("matched %d pairs (%d matches) on %d rank(s): gpu %.3f s, db %.3f s", stats["pairs"], stats["matches"],
                    world, stats["gpu_s"], stats["db_s"])
        return stats
    finally:
        if db is not None:
            db.close()


def _host(x):
    return x.cpu().numpy() if torch.is_tensor(x) else x


def match_loaded(ids, block, counts, kp_arr, kp_cnt, cameras, all_pairs, my_pairs, settings, verify, db, stats, *,
                 match_fn=None, verify_fn=None, guided_fn=None, device="cuda", pair_chunk: int = 16384, distributed=False,
                 write_what="writing the database", skip_empty_share=False) -> dict:
    """Match my share, verify, re-match guided, gather, rank 0 writes: the body that match_database and
    pipeline.distributed.run_sharded share.  Everything is in memory and the same on every rank: the image ids, the uint8
    descriptor blocks [n][n_max][D] + counts (host or device), the keypoints float32 [n][>= 1][2] zero padded + counts
    (host; unused without `verify`), `cameras` (K, prior) or None (essential.camera_table), the full pair list (P, 2) and
    this rank's share of it, `settings` (MatchSettings).  `db` is rank 0's open SqliteColmapDatabase (unused elsewhere).
    Seams left None default to the HIP functions, which take the blocks as they are; a caller's `match_fn` / `guided_fn`
    takes them as host arrays.  `distributed` False runs every collective step locally, whatever process group exists.
    An error on any rank is raised on every rank (`write_what` names rank 0's writing phase in the others' message).
    `skip_empty_share`: a rank whose share is empty calls neither the matcher nor the verifier.
    With `settings.known_distortion` (§4.2l) the keypoints are the undistorted ones, NaN where a keypoint does not invert: the
    matches that touch such a keypoint are dropped from what the verifier gets and from the guided lists, not from `matches`.
    Returns `stats` with the totals filled in — rank 0's, on every rank."""
    s = settings
    kp_ok = np.isfinite(_host(kp_arr)).all(axis=2) if s.known_distortion and verify and kp_arr is not None else None
    empty = not _host(counts).any()                                            # no descriptors anywhere: every pair is empty
    if s.guided and not empty:
        check_guided_block_size(int(block.shape[1]))                           # before any matching starts, on every rank
    if match_fn is None:
        match_fn, m_blocks = partial(hip_match_blocks, device=device, pair_chunk=pair_chunk), (block, counts)
    else:
        m_blocks = (_host(block), _host(counts))
    if guided_fn is None:
        guided_fn, g_blocks = partial(hip_guided_blocks, device=device, pair_chunk=pair_chunk), (block, counts)
    else:
        g_blocks = (_host(block), _host(counts))

    def match_my_share():
        if empty:
            return [np.zeros((0, 2), np.uint32) for _ in my_pairs], None
        if skip_empty_share and len(my_pairs) == 0:
            return [], ([] if verify else None)
        lists = match_fn(*m_blocks, my_pairs, s.max_ratio, s.max_distance, s.cross_check)
        if not verify:
            return lists, None
        vdev = device if (verify_fn is not None or torch.cuda.is_available()) else "cpu"
        usable = lists if kp_ok is None else drop_invalid_matches(lists, my_pairs, kp_ok)[0]
        results = verify_pair_lists(_unpack_keypoints(kp_arr, kp_cnt), ids, my_pairs, usable, device=vdev, verify_fn=verify_fn,
                                    cameras=cameras, relative_pose=s.relative_pose)
        if s.guided:
            # a keypoint that does not invert is at no pixel: it is given (0, 0) and its matches are taken out of the lists again
            rematch_guided(*g_blocks, kp_arr if kp_ok is None else np.nan_to_num(_host(kp_arr)), my_pairs, results, s.max_ratio,
                           s.max_distance, s.cross_check, guided_fn)
            if kp_ok is not None:
                for r, kept in zip(results, drop_invalid_matches([r["inlier_matches"] for r in results], my_pairs, kp_ok)[0]):
                    r["inlier_matches"] = kept
        return lists, results

    t1 = time.perf_counter()
    lists, results = vd.run_guarded(match_my_share, "matching / verification", distributed, rank0_only=False)
    stats["gpu_s"] = time.perf_counter() - t1
    merged = vd.gather_pair_lists(my_pairs, lists, dst=0, distributed=distributed)
    verified = None if results is None else vd.gather_pair_results(my_pairs, results, dst=0, distributed=distributed)

    def write():
        t2 = time.perf_counter()
        for a, b in all_pairs:                                                 # COLMAP's pair order, whatever rank matched it
            m = merged[(int(a), int(b))]
            db.write_matches(ids[a], ids[b], m, commit=False)
            stats["matches"] += len(m)
        db.commit()
        if kp_ok is not None:
            order = [(int(a), int(b)) for a, b in all_pairs]
            stats["undistort_dropped_matches"] = drop_invalid_matches([merged[p] for p in order], order, kp_ok)[1]
            logger.info("known distortion: %d of %d matches touch a keypoint that does not invert and were not verified",
                        stats["undistort_dropped_matches"], stats["matches"])
        if verified is not None:
            stats["verified_pairs"] = write_two_view_rows(db, ids, verified)
            stats["guided_pairs"] = sum(r["config"] != CONFIG_DEGENERATE for r in verified.values()) if s.guided else 0
            stats.update(pose_stats(verified.values()))
        stats["db_s"] = time.perf_counter() - t2

    vd.run_guarded(write, write_what, distributed)
    return vd.broadcast_object(stats, 0) if distributed else stats             # every rank returns rank 0's totals
