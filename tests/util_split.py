"""CPU SPECIFICATION (test infrastructure, NOT product code) of the splitting of inconsistent tracks: the rule
of vc_split_tracks on one component (`split_component`), the call on plain arrays (`split_tracks`), the growth rule with it
(`grow_model`, the rule of vit_colmap_amd/mapping/grow.py under `split_tracks=True`) and the test data: databases whose
matches are swapped pairwise (`swapped_pairs`) and merged components (`merged_component`).  numpy only, on top of
tests/util_mapper.py, whose arithmetic (`_Views`), hypotheses and parallax test it uses unchanged.  This is the build's own
published rule: parity with COLMAP's recursive triangulation is unpinned.
"""
import numpy as np

import util_absolute_pose as ua
import util_essential as ue
import util_mapper as um

SPLIT_MAX_POINTS = 4                                       # VC_SPLIT_MAX_POINTS
SEED_STRIDE = 0x9E3779B9                                   # slot k draws the pairs of seed + k * SEED_STRIDE
# worst |X_host - X_spec| between this specification and split_component compiled for the host (tools/split_tracks_host.cpp,
# -O2 -ffp-contract=off) over the 540 points created on the 320 merged components of tests/test_split_spec.py (`merged_call`),
# every label and count equal (measured: 2.22e-9; as for HOST_SPEC_X of util_mapper.py, 2.1e-9, the two refits stop at
# different steps)
HOST_SPEC_SPLIT_X = 2.3e-9
# what a kernel's X may differ from this specification's by: 4x that, the project's margin for libm and instruction selection
TOL_SPLIT_X = 4 * HOST_SPEC_SPLIT_X
# growth of swapped_pairs(truth_pairs(windowed_scene()), 0.1) on this specification (tests/test_split_spec.py prints and
# asserts them): the clean scene grows 1161 points; with the swaps 112 components are inconsistent and today's rule grows
# 973 points; with the splitting 1158, 185 of them out of those components, none mixing two scene points, no scene point
# twice; all 12 images, worst rotation 1.56 deg, worst centre 0.086 baselines
SWAPPED_CLEAN_POINTS, SWAPPED_FLAG_OFF_POINTS, SWAPPED_FLAG_ON_POINTS, SWAPPED_SPLIT_POINTS = 1161, 973, 1158, 185


# ---- one component --------------------------------------------------------------------------------------------------------------
def _runs(cam):
    """-> [(lo, hi)] of the maximal stretches of adjacent equal values."""
    cuts = np.concatenate([[0], np.nonzero(np.diff(cam))[0] + 1, [len(cam)]])
    return list(zip(cuts[:-1], cuts[1:]))


def selection(w, runs, label, k, X, e2):
    """The nodes selected under X for slot k -> mask, sq, z."""
    inl, sq, z = w.inliers(X, e2)
    cand = inl & (label == -1)
    sel = np.zeros(w.n, bool)
    for lo, hi in runs:
        if (label[lo:hi] == k).any():
            continue
        idx = lo + np.nonzero(cand[lo:hi])[0]
        if len(idx):
            sel[idx[np.argmin(sq[idx])]] = True                                     # argmin: the first of equal ones
    return sel, sq, z


def split_component(obs, cam_rows, obs_cam, seed, max_points, node_point, points_xyz, max_error=um.MAX_ERROR,
                    min_tri_angle_tan2=um.MIN_TRI_ANGLE_TAN2):
    """obs (n, 2), cam_rows (n, 16) the camera of each node (NaN: not usable), obs_cam (n,) what delimits the runs, node_point
    (n,), points_xyz (max_points, 3) -> dict(node_point, points_xyz, count, new, error), the inputs left as they are."""
    obs, rows = np.asarray(obs, np.float64).reshape(-1, 2), np.asarray(cam_rows, np.float64).reshape(-1, 16)
    n = len(obs)
    label, pts = np.array(node_point, np.int32).reshape(n), np.array(points_xyz, np.float64).reshape(max_points, 3)
    new, error = np.zeros(max_points, np.uint8), np.full(max_points, np.nan)
    e2, tan2 = np.float64(max_error) * np.float64(max_error), np.float64(min_tri_angle_tan2)
    occupied = np.isfinite(pts).all(axis=1)
    with np.errstate(all="ignore"):
        w = um._Views(obs, rows) if n else None
        runs = _runs(np.asarray(obs_cam, np.int64).reshape(n)) if n else []
        for k in np.nonzero(occupied)[0] if n else []:
            label[selection(w, runs, label, k, pts[k], e2)[0]] = k
        for k in np.nonzero(~occupied)[0] if n else []:
            best, best_count = None, 0
            for p, q in um.hypothesis_pairs(n, (int(seed) + int(k) * SEED_STRIDE) & 0xFFFFFFFF):
                if not (label[p] == -1 and label[q] == -1 and w.ok[p] and w.ok[q]) or obs_cam[p] == obs_cam[q]:
                    continue
                X = w.midpoint(p, q, tan2)
                if X is None:
                    continue
                sel = selection(w, runs, label, k, X, e2)[0]
                if sel[p] and sel[q] and sel.sum() > best_count:
                    best, best_count = X, int(sel.sum())
            if best is None:
                break
            X, sel = best, selection(w, runs, label, k, best, e2)[0]
            Xr = w.refit(best, sel)
            if np.all(np.isfinite(Xr)):
                rsel = selection(w, runs, label, k, Xr, e2)[0]
                if rsel.sum() >= sel.sum():
                    X, sel = Xr, rsel
            if sel.sum() < 2 or not w.wide(X, sel, tan2):
                break
            _, sq, z = w.inliers(X, e2)
            label[sel], pts[k], new[k] = k, X, 1
            error[k] = float(np.sqrt(sq[sel] / (z[sel] * z[sel])).mean())
    count = np.array([(label == k).sum() for k in range(max_points)], np.int32)
    return dict(node_point=label, points_xyz=pts, count=count, new=new, error=error)


def split_tracks(obs_xy, obs_cam, offsets, cams, seeds, max_points, node_point, points_xyz, max_error=um.MAX_ERROR,
                 min_tri_angle_tan2=um.MIN_TRI_ANGLE_TAN2):
    """The call of vc_split_tracks on numpy arrays -> node_point (total,), points_xyz (C, max_points, 3), count, new, error
    (C, max_points); a component whose offsets are negative, descend or pass the arrays is rejected."""
    obs_xy, cams = np.asarray(obs_xy, np.float64).reshape(-1, 2), np.asarray(cams, np.float64).reshape(-1, 16)
    obs_cam, offsets = np.asarray(obs_cam, np.int64), np.asarray(offsets, np.int64)
    C = len(offsets) - 1
    label, pts = np.array(node_point, np.int32), np.array(points_xyz, np.float64).reshape(C, max_points, 3)
    count, new, error = np.zeros((C, max_points), np.int32), np.zeros((C, max_points), np.uint8), np.full((C, max_points), np.nan)
    for c in range(C):
        lo, hi = offsets[c], offsets[c + 1]
        if lo < 0 or hi < lo or hi > len(obs_cam):
            continue
        slots = obs_cam[lo:hi]
        inside = (slots >= 0) & (slots < len(cams))
        rows = np.full((hi - lo, 16), np.nan)
        rows[inside] = cams[slots[inside]]
        r = split_component(obs_xy[lo:hi], rows, slots, int(seeds[c]) & 0xFFFFFFFF, max_points, label[lo:hi], pts[c], max_error,
                            min_tri_angle_tan2)
        label[lo:hi], pts[c], count[c], new[c], error[c] = r["node_point"], r["points_xyz"], r["count"], r["new"], r["error"]
    return label, pts, count, new, error


def labels_stable_under(obs, rows, obs_cam, seed, max_points, node_point, points_xyz, tol, directions=4):
    """No label of the specification changes when a point it created moves by `tol` in `directions` random directions: the
    selection under the moved point, among the nodes that were free when the slot was peeled, is the one under the point."""
    r = split_component(obs, rows, obs_cam, seed, max_points, node_point, points_xyz)
    w, runs = um._Views(np.asarray(obs, np.float64), np.asarray(rows, np.float64)), _runs(np.asarray(obs_cam, np.int64))
    rs = np.random.RandomState(seed & 0xFFFF)
    e2 = np.float64(um.MAX_ERROR) ** 2
    created, was_free = np.nonzero(r["new"])[0], np.asarray(node_point) == -1
    with np.errstate(all="ignore"):
        for k in created:
            before = r["node_point"].copy()
            before[was_free & np.isin(before, created[created >= k])] = -1          # the labels when slot k was peeled
            for _ in range(directions):
                d = rs.normal(size=3)
                if not np.array_equal(selection(w, runs, before, k, r["points_xyz"][k] + tol * d / np.linalg.norm(d), e2)[0],
                                      was_free & (r["node_point"] == k)):
                    return False
    return True


# ---- test data ------------------------------------------------------------------------------------------------------------------
def swapped_pairs(pairs, frac, seed=91):
    """The rows of `pairs` with a share `frac` of the inlier matches of every pair of consecutive images swapped pairwise in
    their second column: wrong matches that survived verification."""
    rs, out = np.random.RandomState(seed), {}
    for k, g in sorted(pairs.items()):
        m = g["inlier_matches"].copy()
        if k[1] - k[0] == 1 and len(m) >= 4:
            n = int(frac * len(m)) // 2
            for a, b in rs.permutation(len(m))[:2 * n].reshape(n, 2):
                m[a, 1], m[b, 1] = m[b, 1], m[a, 1]          # stays one-to-one
        out[k] = dict(g, inlier_matches=m)
    return out


def arc_cams():
    """The 12 arc cameras as rows of a camera table, and a 13th that is not registered (NaN)."""
    return np.concatenate([np.stack([um.camera_row(R, t, ue.SCENE_K) for R, t in um.arc_cameras()]), np.full((1, 16), np.nan)])


def merged_component(i, outliers=0.0, unusable=None):
    """Problem i of the merged components, from RandomState(17000 + i): 2 or 3 distinct ones of um.exact_track / um.noisy_track
    (odd i: noisy; a third only while the nodes stay 30 at most) concatenated and sorted by camera, so that the tracks' nodes of one camera are adjacent; a share `outliers` of the nodes
    replaced by a uniform random pixel; `unusable` in (None, "first", "last") makes that node unusable in one of four ways (a
    slot < 0, a slot past the table, the NaN row, a NaN pixel) -> obs (n, 2), obs_cam (n,) into arc_cams(), truth (n,) the
    track of each node (-1: an outlier or unusable), the scene points (m, 3), a seed."""
    rs = np.random.RandomState(17000 + i)
    cams = arc_cams()
    obs, cam, truth, X = [], [], [], []
    for m, which in enumerate(rs.choice(300, rs.randint(2, 4), replace=False)):
        o, rows, x, _ = (um.noisy_track if i % 2 else um.exact_track)(int(which))
        if m == 2 and sum(len(a) for a in obs) + len(o) > 30:                      # 4 to 30 nodes
            break
        obs.append(o), truth.append(np.full(len(o), m)), X.append(x)
        cam.append(np.array([int(np.nonzero((cams[:12] == r).all(axis=1))[0][0]) for r in rows]))
    obs, cam, truth = np.concatenate(obs), np.concatenate(cam).astype(np.int32), np.concatenate(truth)
    order = np.argsort(cam, kind="stable")
    obs, cam, truth = obs[order].copy(), cam[order].copy(), truth[order].copy()
    wrong = rs.uniform(size=len(obs)) < outliers
    obs[wrong] = np.stack([rs.uniform(0, 640, wrong.sum()), rs.uniform(0, 480, wrong.sum())], axis=1)
    truth[wrong] = -1
    if unusable is not None:
        at = 0 if unusable == "first" else len(obs) - 1
        how = rs.randint(4)
        if how == 3:
            obs[at, rs.randint(2)] = np.nan
        else:
            cam[at] = (-1 - rs.randint(3), len(cams) + rs.randint(3), 12)[how]
        truth[at] = -1
    return obs, cam, truth, np.array(X), int(rs.randint(1 << 31))


def as_one_call(components, max_points, prefill=None):
    """[(obs, obs_cam, truth, X, seed)] -> obs_xy, obs_cam, offsets, cams, seeds, node_point (all free), points_xyz (all empty)
    of one call.  `prefill(c, component) -> slots` (0 to max_points) pre-fills that many slots of component c with the true
    points of its first tracks (track m past the component's: a point no node sees) and labels every other node of theirs."""
    obs, cam = np.concatenate([c[0] for c in components]), np.concatenate([c[1] for c in components])
    offsets = np.concatenate([[0], np.cumsum([len(c[0]) for c in components])]).astype(np.int32)
    label, pts = np.full(len(obs), -1, np.int32), np.full((len(components), max_points, 3), np.nan)
    for c, comp in enumerate(components):
        for m in range(prefill(c, comp) if prefill else 0):
            pts[c, m] = comp[3][m] if m < len(comp[3]) else np.array([0.5, 0.25 * m, 9.0])
            at = offsets[c] + np.nonzero(comp[2] == m)[0][::2]
            label[at] = m
    return obs, cam, offsets, arc_cams(), np.array([c[4] for c in components], np.int64), label, pts


# ---- the growth rule with splitting -------------------------------------------------------------------------------------------------
def grow_model(images, pairs, estimate=ua.estimate_absolute_pose, triangulate=um.triangulate_tracks, split=split_tracks,
               split_tracks_on=True, after_round=None):
    """um.grow_model with the T-step of §4.2n after its own when `split_tracks_on`: the inconsistent components keep up to
    SPLIT_MAX_POINTS slots of point indices, filled by one `split` call per round.  -> um.grow_model's dict plus
    split_components (the inconsistent components that take part) and split_points (the point indices created out of them).
    `after_round(state)` may remove points: state has poses, xyz, tracks (lists by point index; a removed point is None)."""
    seed = ua.seed_model(images, pairs, estimate)
    poses, xyz, tracks = dict(seed["poses"]), [x for x in seed["xyz"]], [list(t) for t in seed["tracks"]]
    every = um.components(images, pairs)
    comps = [c for c in every if len({i for i, _ in c}) == len(c)]
    comp_of = {node: k for k, c in enumerate(comps) for node in c}
    point_of = {}
    for k, track in enumerate(tracks):
        if track[0] in comp_of:
            point_of[comp_of[track[0]]] = k
    # the inconsistent components and their slots: the seed's points that start in one take its first slots
    broken, slot_points = [], []
    if split_tracks_on:
        for c in every:
            if len({i for i, _ in c}) == len(c):
                continue
            inside = set(c)
            held = [k for k, track in enumerate(tracks) if track[0] in inside]
            if len(held) <= SPLIT_MAX_POINTS:
                broken.append(c)
                slot_points.append(held + [None] * (SPLIT_MAX_POINTS - len(held)))
    split_points = []
    ids = sorted(images)
    slot = {i: s for s, i in enumerate(ids)}
    tried_t, tried_s, tried_r, rounds, registration_rounds = {}, {}, {}, 0, 0
    while True:
        cams = np.full((len(ids), 16), np.nan)
        for i, (R, t) in poses.items():
            cams[slot[i]] = um.camera_row(R, t, images[i]["K"])
        batch = []
        for k, c in enumerate(comps):
            registered = sum(i in poses for i, _ in c)
            if k not in point_of and registered >= 2 and registered > tried_t.get(k, 0):
                tried_t[k] = registered
                batch.append(k)
        new_points = 0
        if batch:
            nodes = [n for k in batch for n in comps[k]]
            obs = np.array([images[i]["keypoints"][kp, :2] for i, kp in nodes], np.float64)
            offsets = np.concatenate([[0], np.cumsum([len(comps[k]) for k in batch])]).astype(np.int32)
            seeds = np.array([((comps[k][0][0] << 16) ^ comps[k][0][1]) & 0xFFFFFFFF for k in batch], np.uint32).view(np.int32)
            X, mask, count, _ = triangulate(obs, np.array([slot[i] for i, _ in nodes], np.int32), offsets, cams, seeds)
            for b, k in enumerate(batch):
                if count[b] > 0:
                    point_of[k] = len(xyz)
                    xyz.append(np.asarray(X[b], np.float64))
                    tracks.append([n for n, m in zip(comps[k], mask[offsets[b]:offsets[b + 1]]) if m])
                    new_points += 1
        # the T-step of the inconsistent components
        batch = []
        for k, c in enumerate(broken):
            registered = sum(i in poses for i, _ in c)
            if registered >= 2 and registered > tried_s.get(k, 0):
                tried_s[k] = registered
                batch.append(k)
        if batch:
            nodes = [n for k in batch for n in broken[k]]
            obs = np.array([images[i]["keypoints"][kp, :2] for i, kp in nodes], np.float64)
            offsets = np.concatenate([[0], np.cumsum([len(broken[k]) for k in batch])]).astype(np.int32)
            seeds = np.array([((broken[k][0][0] << 16) ^ broken[k][0][1]) & 0xFFFFFFFF for k in batch], np.uint32).view(np.int32)
            label, pts = np.full(len(nodes), -1, np.int32), np.full((len(batch), SPLIT_MAX_POINTS, 3), np.nan)
            for b, k in enumerate(batch):
                for s, p in enumerate(slot_points[k]):
                    if p is not None and tracks[p] is None:
                        slot_points[k][s] = p = None                                 # a removed point frees its slot
                    if p is not None:
                        pts[b, s] = xyz[p]
                        for at, node in enumerate(broken[k]):
                            if node in tracks[p]:
                                label[offsets[b] + at] = s
            out_label, out_pts, _, new, _ = split(obs, np.array([slot[i] for i, _ in nodes], np.int32), offsets, cams, seeds,
                                                  SPLIT_MAX_POINTS, label, pts)
            for b, k in enumerate(batch):
                for s in range(SPLIT_MAX_POINTS):
                    took = [node for at, node in enumerate(broken[k])
                            if out_label[offsets[b] + at] == s and label[offsets[b] + at] != s]
                    if new[b, s]:
                        slot_points[k][s] = len(xyz)
                        split_points.append(len(xyz))
                        xyz.append(np.asarray(out_pts[b, s], np.float64))
                        tracks.append(took)
                        new_points += 1
                    elif slot_points[k][s] is not None:
                        tracks[slot_points[k][s]].extend(took)
        # R-step
        new_images = 0
        problems = []
        for c in ids:
            if c in poses or images[c]["K"] is None:
                continue
            kp_idx = [kp for kp in range(len(images[c]["keypoints"])) if point_of.get(comp_of.get((c, kp))) is not None]
            if len(kp_idx) >= ua.ABS_POSE_MIN_NUM_INLIERS and len(kp_idx) > tried_r.get(c, 0):
                tried_r[c] = len(kp_idx)
                problems.append((c, kp_idx, [point_of[comp_of[(c, kp)]] for kp in kp_idx]))
        results = [estimate(images[c]["keypoints"][kp_idx, :2], np.array([xyz[p] for p in pt_idx]), images[c]["K"], c)
                   for c, kp_idx, pt_idx in problems]
        for (c, kp_idx, pt_idx), r in zip(problems, results):
            if not r["success"]:
                continue
            poses[c] = (ua.quat_to_rot(r["qvec"]), np.asarray(r["tvec"], np.float64))
            for kp, p, ok in zip(kp_idx, pt_idx, r["inlier_mask"]):
                if ok:
                    tracks[p].append((c, kp))
            new_images += 1
        if not new_points and not new_images:
            break
        rounds += 1
        registration_rounds += bool(new_images)
        if after_round is not None:
            after_round(dict(poses=poses, xyz=xyz, tracks=tracks, point_of=point_of))
    return dict(initial_pair=seed["initial_pair"], poses=poses, xyz=np.array(xyz).reshape(-1, 3), tracks=tracks, rounds=rounds,
                registration_rounds=registration_rounds, split_components=len(broken), split_points=split_points)


def purity(tracks, split_points):
    """-> (mixed, duplicated) of the split points in windowed_scene, where the keypoint index is the scene point's: the tracks
    that hold two scene points, and the split points whose scene point another point of the model has as well."""
    of = {p: {kp for _, kp in tracks[p]} for p in range(len(tracks)) if tracks[p]}
    mixed = [p for p in split_points if len(of[p]) > 1]
    owners = {}
    for p, kps in of.items():
        if len(kps) == 1:
            owners.setdefault(next(iter(kps)), []).append(p)
    return len(mixed), sum(1 for p in split_points if p not in mixed and len(owners[next(iter(of[p]))]) > 1)
