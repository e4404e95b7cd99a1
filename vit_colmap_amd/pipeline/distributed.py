"""Extraction + matching sharded over the GPUs of one node — what `Pipeline.run` does when a
torch.distributed process group with more than one rank exists (one process per GPU, backend "nccl" = RCCL).

  1. every rank lists the images (sorted, as the reference does) and takes a contiguous block of them;
  2. every rank decodes and extracts its block on its own GPU, in batches of equal-size images
     (features/base_extractor.py `image_batches`); the per-image uint8 descriptor blocks, padded to a common (n_max, D),
     are ALL-GATHERED (the one collective of the data path, RCCL over xGMI), keypoints and image sizes with them;
  3. rank 0 — the only process that ever touches the SQLite file — writes the camera rows by the extractor's camera
     policy (`camera_params_for`, `camera_per_image`: `base_extractor.camera_policy`, as its `extract()` does) and ONE
     image row per readable image, in file order (reference vit_extractor.py:739: a failed image still has its row);
  4. rank 0 writes keypoints / descriptors; the exhaustive pair list is dealt round-robin, every rank matches
     and geometrically verifies its share from the gathered blocks and keypoints (no database read); the match lists
     and two-view geometries are gathered to rank 0, which writes them in pair order (matching/exhaustive.py:
     match_loaded, the body that match_exhaustive runs on what it read from a database).
An error on any rank (rank 0's database included) is raised on every rank instead of leaving the others in a collective
(dist.raise_if_any_failed).
The reference is single-process; there is no counterpart to cite beyond the plugin API it keeps
(`extract(image_dir, db_path, camera_model, camera_params)`, run_pipeline.py:343, and the match call :351-363).

`feature_fn(list of BGR arrays) -> list of (keypoints (N, k) float32, descriptors (N, D) uint8)` and
`match_fn(blocks, counts, pairs, max_ratio, max_distance, cross_check) -> list of match lists` and
`verify_fn(keypoints, pair_images, pair_ids, lists) -> list of results` default to the HIP extractor / matcher / scorer;
the world-size-2 gloo test passes host stand-ins (there is no GPU in that container).
"""
import logging
from pathlib import Path

import numpy as np
import torch

from .. import dist as vd
from ..database.colmap_db import ColmapDatabase
from ..features.base_extractor import add_image_row, camera_policy, default_camera_params, image_batches, list_images
from ..matching.essential import camera_table
from ..matching.exhaustive import MatchSettings, match_loaded, new_stats
from ..matching.hip_matcher import exhaustive_pairs
from ..matching.undistort import undistort_for_matching

logger = logging.getLogger(__name__)


def run_sharded(image_dir, db_path, camera_model, camera_params=None, feature_fn=None, matching_options=None,
                match_fn=None, do_matching=True, verify=True, device="cuda", batch_size=50, verify_fn=None,
                camera_params_for=default_camera_params, camera_per_image=False, guided_fn=None,
                prior_focal_length=False, matcher_type="exhaustive", undistort_fn=None) -> dict:
    """With the options' `known_distortion` (needs `prior_focal_length`) rank 0 undistorts the gathered
    keypoints of the flagged, distorted cameras by the helper match_database uses (matching/undistort.py) and broadcasts
    them with the camera table; the database keeps the raw keypoints.  `undistort_fn` replaces the launch (tests)."""
    settings = MatchSettings.from_options(matching_options, None, verify)
    if matcher_type != "exhaustive":
        # the in-memory path matches every pair; the choice of pairs exists database to database only
        raise ValueError(f"the sharded in-memory pipeline matches exhaustively: for matcher_type {matcher_type!r} extract to "
                         "the database first and call matching.match_retrieval on it (it runs multi-rank as well)")
    rank, world = vd.rank_world()
    image_files = list_images(Path(image_dir))
    if not image_files:
        raise ValueError(f"No images found in {image_dir}")
    n = len(image_files)
    lo, hi = vd.shard_range(n, rank, world)
    per = (n + world - 1) // world
    cdev = vd.comm_device(device)

    # ---- this rank's block ------------------------------------------------------------------------------------------
    hw = np.zeros((per, 2), np.int32)                     # (height, width) of each image, (0, 0) for an unreadable one
    feats = [None] * per
    for batch in image_batches(image_files[lo:hi], batch_size):
        for (k, _, img), r in zip(batch, feature_fn([img for _, _, img in batch])):
            hw[k] = img.shape[:2]
            feats[k] = r
    kdim = max([f[0].shape[1] for f in feats if f is not None] + [2])
    n_max, D, kdim = vd.max_over_ranks(max([len(f[0]) for f in feats if f is not None] + [1]),
                                       max([f[1].shape[1] for f in feats if f is not None] + [1]), kdim)
    desc = np.zeros((per, n_max, D), np.uint8)
    kps = np.zeros((per, n_max, kdim), np.float32)
    counts = np.zeros(per, np.int32)
    for k, f in enumerate(feats):
        if f is not None and len(f[0]):
            counts[k] = len(f[0])
            kps[k, : counts[k]] = f[0]
            desc[k, : counts[k]] = f[1]

    # ---- the collective: descriptor blocks (+ counts, keypoints, image sizes) of every rank -------------------------------
    all_desc, all_counts = vd.all_gather_descriptors(torch.from_numpy(desc).to(cdev), torch.from_numpy(counts).to(cdev))
    all_kps = vd.all_gather_rows(torch.from_numpy(kps).to(cdev))
    all_hw = vd.all_gather_rows(torch.from_numpy(hw).to(cdev)).cpu().numpy()[:n].tolist()
    all_readable = np.array([h > 0 for h, _ in all_hw])
    if not all_readable[0]:
        raise ValueError(f"Failed to read first image: {image_files[0]}")

    # ---- rank 0: camera and image rows in file order, then features ------------------------------------------------------
    stats = new_stats(int(all_readable.sum()), 0, world)
    db = None
    cnt = all_counts.cpu().numpy()
    kp_np = all_kps.cpu().numpy()

    def write_rows():
        nonlocal db
        camera_of = camera_policy(camera_model, camera_params, all_hw[0], camera_params_for, camera_per_image,
                                  prior_focal_length)
        db = ColmapDatabase(str(db_path))
        ids = [add_image_row(db, f.name, camera_of(h, w)) if h else None for f, (h, w) in zip(image_files, all_hw)]
        undistort = prior_focal_length and settings.known_distortion and do_matching
        cameras = None
        if prior_focal_length:      # (K, usable prior) per file, read back from the rows; a distorted camera may get its prior below
            cameras = camera_table(db.db, ids, warn_distorted=False) if undistort else camera_table(db.db, ids)
        d_np = all_desc.cpu().numpy()
        for k, image_id in enumerate(ids):
            if image_id is not None and cnt[k] > 0:
                db.add_keypoints(image_id, kp_np[k, : cnt[k]])
                db.add_descriptors(image_id, d_np[k, : cnt[k]])
        db.commit()
        if undistort:
            kp_u, K, prior = undistort_for_matching(db.db, ids, kp_np[:n, :, :2], cnt[:n], *cameras, device, undistort_fn)
            return ids, (K, prior), kp_u
        return ids, cameras, None

    try:
        rows = vd.run_guarded(write_rows, "writing images / features")
        if not do_matching:
            return stats
        # ---- matching + verification: images with a database row, in id order; pairs dealt round-robin -----------------
        ids, cameras, kp_u = vd.broadcast_object(rows, 0)                    # pair ids seed the verification sampler
        kp_xy = kp_np[:, :, :2] if kp_u is None else kp_u                  # undistorted where a camera's distortion is known
        keep = np.nonzero(all_readable)[0]
        if cameras is not None:                                             # calibrated pairs
            cameras = (cameras[0][keep], cameras[1][keep])
        m = len(keep)
        stats["pairs"] = m * (m - 1) // 2
        return match_loaded([ids[k] for k in keep], all_desc[torch.from_numpy(keep).to(all_desc.device)],
                            all_counts[torch.from_numpy(keep).to(all_counts.device)], kp_xy[keep], cnt[keep], cameras,
                            exhaustive_pairs(m).numpy(), vd.pairs_for_rank(m, rank, world),
                            settings, verify,
                            db.db if db is not None else None, stats, match_fn=match_fn, verify_fn=verify_fn,
                            guided_fn=guided_fn, device=device, distributed=vd.is_distributed(),
                            write_what="writing matches / two-view geometries")
    finally:
        if db is not None:
            db.db.close()
