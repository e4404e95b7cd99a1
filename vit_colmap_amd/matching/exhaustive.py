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

import numpy as np
import torch

from .. import _lib
from .. import dist as vd
from ..database.colmap_db import SqliteColmapDatabase
from .hip_matcher import MODEL_KIND, exhaustive_pairs, match_pairs, match_pairs_guided, prepare_descriptors

logger = logging.getLogger(__name__)


def _sift_options(matching_options, sift_options):
    opts = matching_options if matching_options is not None else sift_options
    if opts is None:
        from ..utils.config import MatchingConfig

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


def pose_stats(results) -> dict:
    """The relative-pose totals of a run's results (an iterable of verify_pairs results)."""
    from .two_view import CONFIG_PANORAMIC, CONFIG_PLANAR

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


def hip_match_blocks(block, counts, pairs, max_ratio=0.8, max_distance=0.7, cross_check=True, device="cuda",
                     pair_chunk: int = 16384):
    """uint8 blocks [n][n_max][D] + counts (host or device) and pairs int32 (P, 2) (host) -> list of P uint32 (M, 2)
    match lists, on the HIP matcher.  Blocks with more rows than one kernel block holds (VC_MAX_KEYPOINTS) are
    matched in row / column sub-blocks whose top-2 results are merged (hip_matcher.match_pairs_blocked)."""
    if not torch.cuda.is_available():
        raise _lib.HipLibraryError("the matcher is HIP-only (no CPU fallback): no GPU visible")
    d_desc = block if torch.is_tensor(block) else torch.from_numpy(np.ascontiguousarray(block))
    d_counts = counts if torch.is_tensor(counts) else torch.from_numpy(np.ascontiguousarray(counts, np.int32))
    d_desc, d_counts = d_desc.to(device), d_counts.to(device)
    n, n_max, D = d_desc.shape
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    if D > _lib.VC_MAX_DESC_DIM:
        raise _lib.HipLibraryError(f"descriptors of {D} bytes exceed the kernels' limit ({_lib.VC_MAX_DESC_DIM})")
    if n_max > _lib.VC_MAX_KEYPOINTS:
        from .hip_matcher import match_pairs_blocked

        return match_pairs_blocked(d_desc, d_counts, pairs, max_ratio, max_distance, cross_check)
    prepared = prepare_descriptors(d_desc, d_counts)
    out = []
    for s in range(0, len(pairs), pair_chunk):
        chunk = torch.from_numpy(pairs[s:s + pair_chunk]).to(device)
        m, c = match_pairs(prepared, d_counts, n, n_max, D, chunk, max_ratio, max_distance, cross_check)
        c_np = c.cpu().numpy()
        _selfcheck(c_np, s, "vc_match_pairs_u8")
        m_np = m.cpu().numpy().view(np.uint32)
        out.extend(m_np[p, : c_np[p]].copy() for p in range(len(c_np)))
    return out


def _selfcheck(c_np, first_pair, what):
    if (c_np < 0).any():   # VC_COUNT_SELFCHECK_FAILED: the kernel's cursor check (include/vitcolmap_hip.h) — never a result
        bad = np.nonzero(c_np < 0)[0][:8] + first_pair
        raise _lib.HipLibraryError(f"{what}: consistency check failed for pairs {bad.tolist()}")


def check_guided_block_size(n_max: int):
    """Guided matching runs in one kernel block per image; the sub-blocked path of larger images is unguided only."""
    if n_max > _lib.VC_MAX_KEYPOINTS:
        raise _lib.HipLibraryError(f"guided matching needs at most VC_MAX_KEYPOINTS = {_lib.VC_MAX_KEYPOINTS} keypoints per "
                                   f"image (the largest image has {n_max})")


def hip_guided_blocks(block, counts, keypoints_xy, pairs, models, kinds, max_error, max_ratio=0.8, max_distance=0.7,
                      cross_check=True, device="cuda", pair_chunk: int = 16384):
    """Guided matching of `pairs` (P, 2) on the HIP matcher: uint8 blocks [n][n_max][D] + counts, keypoints float32
    [n][>= 1][2] (zero padded), models float32 (P, 9), kinds list of "F" / "H" -> list of P uint32 (M, 2) match lists."""
    if not torch.cuda.is_available():
        raise _lib.HipLibraryError("guided matching is HIP-only (no CPU fallback): no GPU visible")
    d_desc = block if torch.is_tensor(block) else torch.from_numpy(np.ascontiguousarray(block))
    d_counts = counts if torch.is_tensor(counts) else torch.from_numpy(np.ascontiguousarray(counts, np.int32))
    d_desc, d_counts = d_desc.to(device), d_counts.to(device)
    n, n_max, D = d_desc.shape
    check_guided_block_size(n_max)
    if D > _lib.VC_MAX_DESC_DIM:
        raise _lib.HipLibraryError(f"descriptors of {D} bytes exceed the kernels' limit ({_lib.VC_MAX_DESC_DIM})")
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
        c_np = c.cpu().numpy()
        _selfcheck(c_np, s, "vc_match_pairs_guided_u8")
        m_np = m.cpu().numpy().view(np.uint32)
        out.extend(m_np[p, : c_np[p]].copy() for p in range(len(c_np)))
    return out


def rematch_guided(block, counts, keypoints_xy, pairs, results, max_ratio, max_distance, cross_check, guided_fn) -> int:
    """The guided pass over one rank's share: every result of `results` (verify_pairs' format, parallel to `pairs`) that is
    not DEGENERATE has its `inlier_matches` replaced by the list matched under the model that produced them (`model`,
    `model9`), with the verifier's own error bound.  Returns the number of pairs re-matched."""
    from .two_view import CONFIG_DEGENERATE, MAX_ERROR

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
                     guided_fn=None) -> dict:
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
    `panoramic_pairs` and `median_tri_angle_deg` (over the posed pairs that are not PANORAMIC)."""
    return match_database(database_path, matching_options, sift_options, device, pair_chunk, distributed, match_fn, verify,
                          verify_fn, guided_fn)


def match_database(database_path, matching_options, sift_options, device, pair_chunk, distributed, match_fn, verify,
                   verify_fn, guided_fn, select_pairs=None, what="match_exhaustive") -> dict:
    """The database-in / database-out body that match_exhaustive and matching.retrieval.match_retrieval share; they differ
    only in where the pair list comes from.  `select_pairs` None: every pair (a < b), dealt to the ranks by
    dist.pairs_for_rank.  Otherwise rank 0 calls `select_pairs(block, counts, stats)` once the descriptor blocks are
    loaded -> int32 (P, 2) image-index pairs, a < b, ascending (a sub-sequence of the exhaustive list; it may add keys
    to `stats`); the list is broadcast, pair p goes to rank p % world (dist.listed_pairs_for_rank), and only the listed
    pairs are matched, verified and written."""
    sift = _sift_options(matching_options, sift_options)
    max_ratio, max_distance, cross_check = float(sift.max_ratio), float(sift.max_distance), bool(sift.cross_check)
    guided = _guided_option(matching_options, sift_options) and verify
    relative_pose = _relative_pose_option(matching_options, sift_options) and verify
    if distributed is None:
        distributed = vd.is_distributed()
    if distributed and not vd.is_distributed():
        raise RuntimeError("distributed=True needs an initialised torch.distributed process group with > 1 rank")
    rank, world = vd.rank_world() if distributed else (0, 1)
    if match_fn is None:
        if not torch.cuda.is_available():
            raise _lib.HipLibraryError(f"{what} needs an MI355X: the matcher is HIP-only (no CPU fallback)")

        def match_fn(block, counts, pairs, r, dmax, cc):
            return hip_match_blocks(block, counts, pairs, r, dmax, cc, device=device, pair_chunk=pair_chunk)

    if guided and guided_fn is None:
        if not torch.cuda.is_available():
            raise _lib.HipLibraryError("guided matching needs an MI355X: the matcher is HIP-only (no CPU fallback)")

        def guided_fn(block, counts, kp_xy, pairs, models, kinds, e, r, dmax, cc):
            return hip_guided_blocks(block, counts, kp_xy, pairs, models, kinds, e, r, dmax, cc, device=device,
                                     pair_chunk=pair_chunk)

    from .essential import camera_table
    from .two_view import CONFIG_DEGENERATE, read_keypoints_by_index, verify_pair_lists, write_two_view_rows

    t0 = time.perf_counter()
    db = None
    try:
        ids = block = counts = D = kp_arr = kp_cnt = cam_k = cam_prior = None
        err = None
        if rank == 0:                                                          # rank 0 is the only reader and writer
            try:
                db = SqliteColmapDatabase(str(database_path))
                ids, block, counts, D = load_descriptor_blocks(db)
                if verify and D != 0:
                    kp_arr, kp_cnt = _pack_keypoints(read_keypoints_by_index(db, ids), len(ids))
                    cam_k, cam_prior = camera_table(db, ids)               # focal-length priors
                    if relative_pose and not cam_prior.any():
                        logger.warning("compute_relative_pose is set and no camera has a usable focal-length prior: "
                                       "it has no effect")
            except Exception as e:  # noqa: BLE001 - handed to every rank below
                err = e
        if distributed:
            vd.raise_if_any_failed(err, "reading the database")
            ids, D = vd.broadcast_object((ids, D), 0)
            block = vd.broadcast_array(block, 0, device)
            counts = vd.broadcast_array(counts, 0, device)
            if verify and D != 0:
                kp_arr = vd.broadcast_array(kp_arr, 0, device)
                kp_cnt = vd.broadcast_array(kp_cnt, 0, device)
                cam_k = vd.broadcast_array(cam_k, 0, device)
                cam_prior = vd.broadcast_array(cam_prior, 0, device)
        elif err is not None:
            raise err
        n = len(ids)
        stats = dict(images=n, pairs=n * (n - 1) // 2, matches=0, gpu_s=0.0, db_s=0.0, verified_pairs=0, ranks=world,
                     guided_pairs=0, pose_pairs=0, planar_pairs=0, panoramic_pairs=0, median_tri_angle_deg=0.0)
        if n < 2:
            return stats
        if guided and D != 0:
            check_guided_block_size(int(np.asarray(block).shape[1]))           # before any matching starts, on every rank
        if select_pairs is None:
            all_pairs = exhaustive_pairs(n).numpy()
            my_pairs = vd.pairs_for_rank(n, rank, world)
        else:
            err = all_pairs = None
            if rank == 0:
                try:
                    all_pairs = np.ascontiguousarray(select_pairs(block, counts, stats), np.int32).reshape(-1, 2)
                except Exception as e:  # noqa: BLE001 - handed to every rank below
                    err = e
            if distributed:
                vd.raise_if_any_failed(err, "selecting the pairs")
                all_pairs = vd.broadcast_array(all_pairs, 0, device)
            elif err is not None:
                raise err
            my_pairs = vd.listed_pairs_for_rank(all_pairs, rank, world)
            stats["pairs"] = len(all_pairs)
        t1 = time.perf_counter()
        err, lists, results = None, [], None
        try:
            if D == 0:
                lists = [np.zeros((0, 2), np.uint32) for _ in my_pairs]      # no descriptors anywhere: every pair is empty
            elif select_pairs is not None and len(my_pairs) == 0:
                results = [] if verify else None                               # nothing selected fell to this rank
            else:
                lists = match_fn(block, counts, my_pairs, max_ratio, max_distance, cross_check)
                if verify:                                                     # this rank verifies the pairs it matched
                    vdev = device if (verify_fn is not None or torch.cuda.is_available()) else "cpu"
                    results = verify_pair_lists(_unpack_keypoints(kp_arr, kp_cnt), ids, my_pairs, lists, device=vdev,
                                                verify_fn=verify_fn, cameras=(cam_k, cam_prior), relative_pose=relative_pose)
                    if guided:
                        rematch_guided(block, counts, kp_arr, my_pairs, results, max_ratio, max_distance, cross_check,
                                       guided_fn)
        except Exception as e:  # noqa: BLE001
            err = e
        if distributed:
            vd.raise_if_any_failed(err, "matching / verification")
        elif err is not None:
            raise err
        stats["gpu_s"] = time.perf_counter() - t1
        merged = vd.gather_pair_lists(my_pairs, lists, dst=0) if distributed else \
            {(int(a), int(b)): m for (a, b), m in zip(my_pairs, lists)}
        verified = None
        if results is not None:
            verified = vd.gather_pair_results(my_pairs, results, dst=0) if distributed else \
                {(int(a), int(b)): r for (a, b), r in zip(my_pairs, results)}
        err = None
        if rank == 0:
            try:
                t2 = time.perf_counter()
                for a, b in all_pairs:                                         # COLMAP's pair order, whatever rank matched it
                    m = merged[(int(a), int(b))]
                    db.write_matches(ids[a], ids[b], m, commit=False)
                    stats["matches"] += len(m)
                db.commit()
                if verified is not None:
                    stats["verified_pairs"] = write_two_view_rows(db, ids, verified)
                    stats["guided_pairs"] = sum(r["config"] != CONFIG_DEGENERATE for r in verified.values()) if guided else 0
                    stats.update(pose_stats(verified.values()))
                stats["db_s"] = time.perf_counter() - t2
            except Exception as e:  # noqa: BLE001
                err = e
        if distributed:
            vd.raise_if_any_failed(err, "writing the database")
            stats = vd.broadcast_object(stats, 0)                              # every rank returns rank 0's totals
        elif err is not None:
            raise err
        stats["total_s"] = time.perf_counter() - t0
        logger.info("matched %d pairs (%d matches) on %d rank(s): gpu %.3f s, db %.3f s", stats["pairs"], stats["matches"],
                    world, stats["gpu_s"], stats["db_s"])
        return stats
    finally:
        if db is not None:
            db.close()
