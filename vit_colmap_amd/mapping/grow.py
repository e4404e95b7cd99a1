"""Growth of the seed model: the tracks of the match graph are triangulated under the registered poses
and the remaining images registered against the new points, in rounds, until a round adds neither a point nor an image.
It is still not a mapper: no bundle adjustment here (mapping/bundle.py adjusts the result once, §4.2k; mapping/rounds.py runs
this loop with one adjustment and one re-evaluation of the tracks per round, §4.2m), no local adjustment, no merging of
existing points (a component with two keypoints in one image is discarded, or with `split_tracks` split into up to
SPLIT_MAX_POINTS points that take no part in registration, §4.2n), no distortion inside the rounds: a SIMPLE_RADIAL or RADIAL
camera with k = 0 is grown under the pinhole assumption and mapping/bundle.py refines k afterwards; one with a known non-zero k
is, with `known_distortion`, grown on keypoints that vc_undistort_points undistorted first.  Specification: tests/util_mapper.py (`grow_model`).  This build's own published rule;
parity with COLMAP's mapper is unpinned.

Where the work runs
  HIP     the seed model's two steps (mapping/seed.py); per round one launch of vc_triangulate_tracks over every track that
          is tried (mapping/triangulate.py), with `split_tracks` one of vc_split_tracks over every inconsistent component that
          is tried, and one registration batch over every image that is tried
          (mapping/absolute_pose.py)
  host    Python / numpy: the database rows, the union-find over (image, keypoint) nodes, which tracks and images a round
          tries, the point ids and tracks, the final reprojection errors
"""
import logging
from types import SimpleNamespace

import numpy as np

from ..database.colmap_db import _quat_to_rot
from .absolute_pose import ABS_POSE_MIN_NUM_INLIERS, estimate_absolute_poses
from .seed import SparseModel, _database, _observation_errors, _seed_model

SPLIT_MAX_POINTS = 4                 # VC_SPLIT_MAX_POINTS; mapping/triangulate.py, which needs torch, has it too

logger = logging.getLogger(__name__)


def _gpu_triangulate(obs_xy, obs_cam, offsets, cams, seeds, device):
    import torch

    from .triangulate import triangulate_tracks

    xyz, mask, count, error = triangulate_tracks(*(torch.from_numpy(np.ascontiguousarray(a)).to(device)
                                                   for a in (obs_xy, obs_cam, offsets, cams, seeds)))
    return xyz.cpu().numpy(), mask.cpu().numpy(), count.cpu().numpy(), error.cpu().numpy()


def _components(kps, K, rows):
    """Union-find over the nodes (image id, keypoint index), numbered image by image; the edges are the inlier matches of the
    rows between images with a usable camera -> the consistent components (no two nodes in one image) as int64 arrays
    (m, 2) of (image id, keypoint) in ascending order, themselves ascending in their first node."""
    return _all_components(kps, K, rows)[0]


def _all_components(kps, K, rows):
    """-> (the consistent components as `_components` states them, the inconsistent ones in the same form: some image holds
    two of their nodes, which are adjacent in the ascending order)."""
    ids = sorted(kps)
    base = dict(zip(ids, np.concatenate([[0], np.cumsum([len(kps[i]) for i in ids])])))
    total = int(sum(len(kps[i]) for i in ids))
    parent = np.arange(total)
    edges = [np.stack([base[i] + g["inlier_matches"][:, 0].astype(np.int64), base[j] + g["inlier_matches"][:, 1].astype(np.int64)], axis=1)
             for (i, j), g in sorted(rows.items()) if K[i] is not None and K[j] is not None]
    touched = np.zeros(total, bool)
    for a, b in (np.concatenate(edges) if edges else np.zeros((0, 2), np.int64)):
        touched[a] = touched[b] = True
        while parent[a] != a:                                  # path halving
            parent[a] = parent[parent[a]]
            a = parent[a]
        while parent[b] != b:
            parent[b] = parent[parent[b]]
            b = parent[b]
        if a != b:
            parent[max(a, b)] = min(a, b)                      # the root of a component is its first node
    nodes = np.nonzero(touched)[0]
    root = nodes.copy()
    while True:
        up = parent[root]
        if np.array_equal(up, root):
            break
        root = up
    image_of = np.repeat(np.array(ids, np.int64), [len(kps[i]) for i in ids])
    first = np.array([base[i] for i in ids], np.int64)
    comps, broken = [], []
    order = np.argsort(root, kind="stable")                    # nodes ascend inside a component, components by their root
    for members in np.split(nodes[order], np.nonzero(np.diff(root[order]))[0] + 1) if len(nodes) else []:
        im = image_of[members]
        (comps if len(np.unique(im)) == len(im) else broken).append(np.stack([im, members - first[np.searchsorted(ids, im)]], axis=1))
    return comps, broken


def _gpu_split(obs_xy, obs_cam, offsets, cams, seeds, node_point, points_xyz, device):
    import torch

    from .triangulate import split_tracks

    out = split_tracks(*(torch.from_numpy(np.ascontiguousarray(a)).to(device)
                         for a in (obs_xy, obs_cam, offsets, cams, seeds, node_point, points_xyz)))
    return tuple(t.cpu().numpy() for t in out)


def _grow(database_path, device, two_view_pose_fn, estimate_fn, triangulate_fn, known_distortion, undistort_fn, round_fn=None,
          split_tracks=False, split_fn=None, tangential=False) -> SparseModel:
    """The growth loop of build_sparse_model, which states the arguments.  `round_fn(growth)`, if given, is called at the end of
    every round that added a point or an image (mapping/rounds.py) with the loop's state: device, images, K,
    kps (the keypoints the solvers see), ids, slot, comps, slots, initial_pair and, to change in place, poses {image id: (R, t,
    qvec)}, xyz and tracks {point id: ...} and point_of {component: point id}.  A point it removes frees its component for the
    T-step under the rule below: the component is tried again only once more of its nodes are registered than at its last
    attempt.  Point ids are never reused.  `split_tracks`, `split_fn` as build_sparse_model states them (§4.2n): the points of
    the inconsistent components are in xyz and tracks like any other but not in point_of; which slot of its component a point
    holds is kept here, and a point that round_fn removes frees its slot."""
    estimate_fn = estimate_fn or estimate_absolute_poses
    triangulate_fn = triangulate_fn or _gpu_triangulate
    database = _database(database_path, device, known_distortion, undistort_fn, tangential)     # `tangential` only where it is on
    images, cameras, K, kps, rows = database[:5]
    known = database[5] if len(database) > 5 else None
    raw = kps if known is None else known["raw"]
    seed = _seed_model(database, device, two_view_pose_fn, estimate_fn)

    poses = {i: (_quat_to_rot(im["qvec"]), np.asarray(im["tvec"], np.float64), im["qvec"]) for i, im in seed.images.items()}
    xyz = {pid: p["xyz"] for pid, p in seed.points3D.items()}
    tracks = {pid: list(p["track"]) for pid, p in seed.points3D.items()}
    comps, broken = _all_components(kps, K, rows) if split_tracks else (_components(kps, K, rows), [])
    split_fn = split_fn or _gpu_split
    comp_at = {i: {} for i in images}                          # image -> keypoint -> component
    for c, nodes in enumerate(comps):
        for i, kp in nodes:
            comp_at[int(i)][int(kp)] = c
    point_of = {}                                              # component -> point id
    for pid, track in tracks.items():
        c = comp_at[track[0][0]].get(track[0][1])
        if c is not None:
            point_of[c] = pid
    ids = sorted(images)
    slot = {i: s for s, i in enumerate(ids)}
    slots = [np.array([slot[int(i)] for i in nodes[:, 0]], np.int32) for nodes in comps]
    next_id = max(xyz, default=0) + 1
    tried_t, tried_r, rounds = np.zeros(len(comps), np.int64), {}, 0
    # the inconsistent components that take part (§4.2n): SPLIT_MAX_POINTS slots of point ids each, the seed's points that start
    # in one in its first slots; a component with more of those than slots stays out
    broken_at = {(int(i), int(kp)): c for c, nodes in enumerate(broken) for i, kp in nodes}
    held = [[] for _ in broken]
    for pid in sorted(tracks):
        if tuple(tracks[pid][0]) in broken_at:
            held[broken_at[tuple(tracks[pid][0])]].append(pid)
    broken = [nodes for nodes, h in zip(broken, held) if len(h) <= SPLIT_MAX_POINTS]
    slot_points = [h + [None] * (SPLIT_MAX_POINTS - len(h)) for h in held if len(h) <= SPLIT_MAX_POINTS]
    broken_slots = [np.array([slot[int(i)] for i in nodes[:, 0]], np.int32) for nodes in broken]
    tried_s, split_points = np.zeros(len(broken), np.int64), []
    growth = SimpleNamespace(device=device, images=images, K=K, kps=kps, ids=ids, slot=slot, comps=comps, slots=slots,
                             initial_pair=seed.initial_pair, poses=poses, xyz=xyz, tracks=tracks, point_of=point_of)
    while True:
        # T-step: every track without a point that two registered images see, in one launch
        cams = np.full((len(ids), 16), np.nan)
        for i, (R, t, _) in poses.items():
            cams[slot[i]] = np.concatenate([R.reshape(9), t, [K[i][0, 0], K[i][1, 1], K[i][0, 2], K[i][1, 2]]])
        registered = np.isfinite(cams[:, 0])
        batch = []
        for c, s in enumerate(slots):
            seen = int(registered[s].sum())
            if c not in point_of and seen >= 2 and seen > tried_t[c]:
                tried_t[c] = seen
                batch.append(c)
        new_points = 0
        if batch:
            obs = np.concatenate([np.stack([kps[int(i)][int(kp)] for i, kp in comps[c]]) for c in batch]).astype(np.float64)
            offsets = np.concatenate([[0], np.cumsum([len(comps[c]) for c in batch])]).astype(np.int32)
            seeds = np.array([((int(comps[c][0, 0]) << 16) ^ int(comps[c][0, 1])) & 0xFFFFFFFF for c in batch], np.uint32).view(np.int32)
            X, mask, count, _ = triangulate_fn(obs, np.concatenate([slots[c] for c in batch]), offsets, cams, seeds, device)
            for b, c in enumerate(batch):
                if count[b] > 0:
                    point_of[c] = next_id
                    xyz[next_id] = np.asarray(X[b], np.float64).copy()
                    tracks[next_id] = [(int(i), int(kp)) for (i, kp), m in zip(comps[c], mask[offsets[b]:offsets[b + 1]]) if m]
                    next_id += 1
                    new_points += 1
        # T-step of the inconsistent components: every one that two registered images see, all of its nodes, in one launch
        batch = []
        for c, s in enumerate(broken_slots):
            seen = int(registered[s].sum())
            if seen >= 2 and seen > tried_s[c]:
                tried_s[c] = seen
                batch.append(c)
        if batch:
            obs = np.concatenate([np.stack([kps[int(i)][int(kp)] for i, kp in broken[c]]) for c in batch]).astype(np.float64)
            offsets = np.concatenate([[0], np.cumsum([len(broken[c]) for c in batch])]).astype(np.int32)
            seeds = np.array([((int(broken[c][0, 0]) << 16) ^ int(broken[c][0, 1])) & 0xFFFFFFFF for c in batch], np.uint32).view(np.int32)
            label, pts = np.full(int(offsets[-1]), -1, np.int32), np.full((len(batch), SPLIT_MAX_POINTS, 3), np.nan)
            for b, c in enumerate(batch):
                slot_points[c] = [pid if pid in xyz else None for pid in slot_points[c]]          # a removed point frees its slot
                for k, pid in enumerate(slot_points[c]):
                    if pid is not None:
                        pts[b, k] = xyz[pid]
                        own = set(tracks[pid])
                        label[offsets[b]:offsets[b + 1]][[(int(i), int(kp)) in own for i, kp in broken[c]]] = k
            out_label, out_pts, _, made, _ = split_fn(obs, np.concatenate([broken_slots[c] for c in batch]), offsets, cams, seeds, label,
                                                      pts, device)
            for b, c in enumerate(batch):
                before, after = label[offsets[b]:offsets[b + 1]], np.asarray(out_label[offsets[b]:offsets[b + 1]])
                for k in range(SPLIT_MAX_POINTS):
                    took = [(int(i), int(kp)) for (i, kp), m in zip(broken[c], (after == k) & (before != k)) if m]
                    if made[b, k]:
                        slot_points[c][k] = next_id
                        xyz[next_id] = np.asarray(out_pts[b, k], np.float64).copy()
                        tracks[next_id] = took
                        split_points.append(next_id)
                        next_id += 1
                        new_points += 1
                    elif slot_points[c][k] is not None:
                        tracks[slot_points[c][k]].extend(took)
        # R-step: every unregistered image against the points its keypoints' tracks have, in one batch
        problems, meta = [], []
        for i in ids:
            if i in poses or K[i] is None:
                continue
            pairs = sorted((kp, point_of[c]) for kp, c in comp_at[i].items() if c in point_of)
            if len(pairs) >= ABS_POSE_MIN_NUM_INLIERS and len(pairs) > tried_r.get(i, 0):
                tried_r[i] = len(pairs)
                kp_idx, pids = [kp for kp, _ in pairs], [pid for _, pid in pairs]
                problems.append(dict(obs=kps[i][kp_idx], xyz=np.stack([xyz[pid] for pid in pids]), K=K[i], seed=i))
                meta.append((i, kp_idx, pids))
        new_images = 0
        for (i, kp_idx, pids), r in zip(meta, estimate_fn(problems, device) if problems else []):
            if not r["success"]:
                continue
            q = np.asarray(r["qvec"], np.float64)
            poses[i] = (_quat_to_rot(q), np.asarray(r["tvec"], np.float64), q)
            for kp, pid, ok in zip(kp_idx, pids, r["inlier_mask"]):
                if ok:
                    tracks[pid].append((i, kp))
            new_images += 1
        if not new_points and not new_images:
            break
        rounds += 1
        logger.info("Growth round %d: %d new points, %d new images", rounds, new_points, new_images)
        if round_fn is not None:
            round_fn(growth)

    model = SparseModel(initial_pair=seed.initial_pair, rounds=rounds)
    if split_tracks:
        model.split_components, model.split_points = len(broken), list(split_points)
    for i, (_, t, q) in sorted(poses.items()):
        cid = images[i].camera_id
        model.cameras[cid] = cameras[cid]
        model.images[i] = dict(qvec=q, tvec=t, camera_id=cid, name=images[i].name, xys=raw[i].astype(np.float64),
                               point3D_ids=np.full(len(kps[i]), -1, np.int64))
    for pid in sorted(xyz):
        errs = []
        for i, kp in tracks[pid]:
            model.images[i]["point3D_ids"][kp] = pid
            errs.append(_observation_errors(K, kps, known, i, poses[i][0], poses[i][1], xyz[pid][None], kp)[0])
        model.points3D[pid] = dict(xyz=xyz[pid].copy(), rgb=(0, 0, 0), error=float(np.mean(errs)), track=list(tracks[pid]))
    return model


def build_sparse_model(database_path, device="cuda", two_view_pose_fn=None, estimate_fn=None, triangulate_fn=None, known_distortion=False,
                       undistort_fn=None, split_tracks=False, split_fn=None, tangential=False) -> SparseModel:
    """Read a matched database -> the seed model grown by rounds.  Raises the seed model's ValueErrors unchanged.
    `two_view_pose_fn` and `estimate_fn` as in build_seed_model; `triangulate_fn(obs_xy, obs_cam, offsets, cams, seeds,
    device) -> (xyz, mask, count, error)` on numpy arrays replaces the triangulation launch (tests).
    `known_distortion`, `undistort_fn` as in build_seed_model (§4.2l): the seed and every round solve on the undistorted
    keypoints, a keypoint that does not invert is in no track, `xys` are the raw keypoints and `error` uses the distorted
    projection.
    `split_tracks` (§4.2n): a component of the match graph with two keypoints in one image, which is otherwise discarded whole,
    is split: after the triangulation launch of a round one launch of vc_split_tracks attaches free nodes to the points such a
    component has and peels new points off the rest, up to SPLIT_MAX_POINTS per component.  Those points take no part in
    registration.  `split_fn(obs_xy, obs_cam, offsets, cams, seeds, node_point, points_xyz, device) -> (node_point, points_xyz,
    count, new, error)` on numpy arrays replaces that launch (tests).  The model's statistics gain split_components (the
    inconsistent components that took part) and split_points (the points made out of them that the model has).
    `tangential` ("The tangential terms" in §4.2k) as in build_seed_model: OPENCV cameras are read as the other models are."""
    tangential_args = dict(tangential=True) if tangential else {}
    return _grow(database_path, device, two_view_pose_fn, estimate_fn, triangulate_fn, known_distortion, undistort_fn,
                 split_tracks=split_tracks, split_fn=split_fn, **tangential_args)
