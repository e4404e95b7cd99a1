"""Track triangulation: one 3D point per track of observations under known poses, every track of a call
in one launch of vc_triangulate_tracks (csrc/triangulate.hip), whose header states the rule.  Specification:
tests/util_mapper.py (`triangulate_track`).  This build's own published rule; parity with COLMAP's triangulator is unpinned.

Where the work runs
  HIP     everything about a track: hypotheses, inlier counts, the refit, the acceptance test, the mean error
  torch   with `sort_by_length`: the stable sort of the tracks by length (longest first), so that the lanes of a wave run loops
          of equal length, and the gather that undoes it on the outputs — plumbing.  Off by default: the kernel gains from it
          (0.50 against 0.70 ms on 200 000 tracks of 2-5 observations) less than the sort and the gathers cost
"""
import numpy as np
import torch

from .. import _lib
from ..matching._common import MAX_ERROR
from .absolute_pose import FILTER_MIN_TRI_ANGLE

MIN_TRI_ANGLE_TAN2 = float(np.tan(FILTER_MIN_TRI_ANGLE) ** 2)
TRI_REFIT_STEPS = 10                 # kRefitSteps of csrc/triangulate.hip


def triangulate_tracks(obs_xy, obs_cam, offsets, cams, seeds, max_error=MAX_ERROR, min_tri_angle_tan2=MIN_TRI_ANGLE_TAN2,
                       sort_by_length=False):
    """obs_xy float64 (total, 2) px, obs_cam int32 (total,) slots into cams, offsets int32 (T + 1,) ascending from 0 to total,
    cams float64 (n_cams, 16) (R row-major, t, fx, fy, cx, cy; a NaN row: not registered), seeds int32 (T,), all on one GPU
    -> xyz float64 (T, 3) (NaN where rejected), mask bool (total,), count int32 (T,), error float64 (T,) in the caller's order.
    `sort_by_length=True` launches the tracks longest first instead of in the caller's order (the result is the same)."""
    if not (obs_xy.is_cuda and obs_xy.dtype == torch.float64 and cams.dtype == torch.float64 and obs_cam.dtype == torch.int32
            and offsets.dtype == torch.int32 and seeds.dtype == torch.int32):
        raise ValueError("triangulate_tracks needs float64 observations and cameras and int32 slots / offsets / seeds on the GPU")
    dev = obs_xy.device
    if any(t.device != dev for t in (obs_cam, offsets, cams, seeds)):
        raise ValueError("triangulate_tracks needs every tensor on the same GPU")
    T, total = int(seeds.shape[0]), int(obs_cam.shape[0])
    if offsets.shape != (T + 1,) or obs_xy.shape != (total, 2) or cams.dim() != 2 or cams.shape[1] != 16:
        raise ValueError("triangulate_tracks needs obs_xy (total, 2), obs_cam (total,), offsets (T + 1,), cams (n_cams, 16), seeds (T,)")
    xyz = torch.full((T, 3), float("nan"), dtype=torch.float64, device=dev)
    mask = torch.zeros((total,), dtype=torch.uint8, device=dev)
    count = torch.zeros((T,), dtype=torch.int32, device=dev)
    error = torch.full((T,), float("nan"), dtype=torch.float64, device=dev)
    if T == 0 or total == 0:
        return xyz, mask.bool(), count, error
    off64 = offsets.to(torch.int64)
    if int(off64[0]) != 0 or int(off64[-1]) != total or bool((off64[1:] < off64[:-1]).any()):
        raise ValueError("triangulate_tracks needs offsets that ascend from 0 to the number of observations")
    lib = _lib.load()
    order = None
    if sort_by_length:
        # tracks are short and of mixed length: in the caller's order the lanes of a wave would wait for its longest track.
        # Longest first: the few waves of long tracks take longest and start at once, the short ones fill in behind them
        lengths, order = torch.sort(off64[1:] - off64[:-1], descending=True, stable=True)
        new_off = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(lengths, 0)])
        # observation j of the sorted call is observation src[j] of the caller's
        src = torch.repeat_interleave(off64[order] - new_off[:-1], lengths) + torch.arange(total, device=dev)
        obs_xy, obs_cam, offsets, seeds = obs_xy[src], obs_cam[src], new_off.to(torch.int32), seeds[order]
    obs_xy, obs_cam, offsets, cams, seeds = (t.contiguous() for t in (obs_xy, obs_cam, offsets, cams, seeds))
    _lib.check(lib.vc_triangulate_tracks(_lib.ptr(obs_xy), _lib.ptr(obs_cam), _lib.ptr(offsets), T, _lib.ptr(cams), int(cams.shape[0]),
                                         _lib.ptr(seeds), float(max_error), float(min_tri_angle_tan2), _lib.ptr(xyz), _lib.ptr(mask),
                                         _lib.ptr(count), _lib.ptr(error), _lib.stream_ptr()), "vc_triangulate_tracks")
    if order is not None:
        inverse = torch.empty_like(order)
        inverse[order] = torch.arange(T, device=dev)
        unsorted = torch.empty_like(mask)
        unsorted[src] = mask
        xyz, count, error, mask = xyz[inverse], count[inverse], error[inverse], unsorted
    return xyz, mask.bool(), count, error


def refine_tracks(obs_xy, obs_cam, offsets, cams, init_xyz, max_error=MAX_ERROR, min_tri_angle_tan2=MIN_TRI_ANGLE_TAN2):
    """The tracks of triangulate_tracks evaluated again at the points they have, one launch of
    vc_refine_tracks: init_xyz float64 (T, 3) in place of the seeds, every other tensor and the four results as there.  A track
    whose point is not finite or has fewer than two inliers is rejected; otherwise the point is refitted over its inliers and
    `mask` are the inliers of the result.  Specification: tests/util_rounds.py (`refine_track`)."""
    if not (obs_xy.is_cuda and obs_xy.dtype == torch.float64 and cams.dtype == torch.float64 and init_xyz.dtype == torch.float64
            and obs_cam.dtype == torch.int32 and offsets.dtype == torch.int32):
        raise ValueError("refine_tracks needs float64 observations, cameras and points and int32 slots / offsets on the GPU")
    dev = obs_xy.device
    if any(t.device != dev for t in (obs_cam, offsets, cams, init_xyz)):
        raise ValueError("refine_tracks needs every tensor on the same GPU")
    T, total = int(init_xyz.shape[0]), int(obs_cam.shape[0])
    if (init_xyz.shape != (T, 3) or offsets.shape != (T + 1,) or obs_xy.shape != (total, 2) or cams.dim() != 2
            or cams.shape[1] != 16):
        raise ValueError("refine_tracks needs obs_xy (total, 2), obs_cam (total,), offsets (T + 1,), cams (n_cams, 16), init_xyz (T, 3)")
    xyz = torch.full((T, 3), float("nan"), dtype=torch.float64, device=dev)
    mask = torch.zeros((total,), dtype=torch.uint8, device=dev)
    count = torch.zeros((T,), dtype=torch.int32, device=dev)
    error = torch.full((T,), float("nan"), dtype=torch.float64, device=dev)
    if T == 0 or total == 0:
        return xyz, mask.bool(), count, error
    off64 = offsets.to(torch.int64)
    if int(off64[0]) != 0 or int(off64[-1]) != total or bool((off64[1:] < off64[:-1]).any()):
        raise ValueError("refine_tracks needs offsets that ascend from 0 to the number of observations")
    lib = _lib.load()
    obs_xy, obs_cam, offsets, cams, init_xyz = (t.contiguous() for t in (obs_xy, obs_cam, offsets, cams, init_xyz))
    _lib.check(lib.vc_refine_tracks(_lib.ptr(obs_xy), _lib.ptr(obs_cam), _lib.ptr(offsets), T, _lib.ptr(cams), int(cams.shape[0]),
                                    _lib.ptr(init_xyz), float(max_error), float(min_tri_angle_tan2), _lib.ptr(xyz), _lib.ptr(mask),
                                    _lib.ptr(count), _lib.ptr(error), _lib.stream_ptr()), "vc_refine_tracks")
    return xyz, mask.bool(), count, error


SPLIT_MAX_POINTS = 4                 # VC_SPLIT_MAX_POINTS of include/vitcolmap_hip.h


def split_tracks(obs_xy, obs_cam, offsets, cams, seeds, node_point, points_xyz, max_error=MAX_ERROR,
                 min_tri_angle_tan2=MIN_TRI_ANGLE_TAN2):
    """The components of the match graph that hold more than one scene point, split into up to max_points points each
    (DESIGN.md §4.2n), one launch of vc_split_tracks, whose header states the rule: obs_xy, obs_cam, offsets (C + 1,), cams and
    seeds (C,) as triangulate_tracks has them, a row per node, the nodes of a component sorted by (image, keypoint); node_point
    int32 (total,) (-1: free, k: of slot k) and points_xyz float64 (C, max_points, 3) (a NaN row: an empty slot), max_points in
    [1, SPLIT_MAX_POINTS].  -> node_point, points_xyz (new tensors, the inputs stay), count int32, new bool and error float64
    (C, max_points).  Specification: tests/util_split.py (`split_tracks`)."""
    if not (obs_xy.is_cuda and obs_xy.dtype == torch.float64 and cams.dtype == torch.float64 and points_xyz.dtype == torch.float64
            and obs_cam.dtype == torch.int32 and offsets.dtype == torch.int32 and seeds.dtype == torch.int32
            and node_point.dtype == torch.int32):
        raise ValueError("split_tracks needs float64 observations, cameras and points and int32 slots / offsets / seeds / labels on the GPU")
    dev = obs_xy.device
    if any(t.device != dev for t in (obs_cam, offsets, cams, seeds, node_point, points_xyz)):
        raise ValueError("split_tracks needs every tensor on the same GPU")
    C, total = int(seeds.shape[0]), int(obs_cam.shape[0])
    if (offsets.shape != (C + 1,) or obs_xy.shape != (total, 2) or cams.dim() != 2 or cams.shape[1] != 16 or node_point.shape != (total,)
            or points_xyz.dim() != 3 or points_xyz.shape[0] != C or points_xyz.shape[2] != 3
            or not 1 <= points_xyz.shape[1] <= SPLIT_MAX_POINTS):
        raise ValueError("split_tracks needs obs_xy (total, 2), obs_cam and node_point (total,), offsets (C + 1,), cams (n_cams, 16), "
                         f"seeds (C,), points_xyz (C, 1 to {SPLIT_MAX_POINTS}, 3)")
    max_points = int(points_xyz.shape[1])
    node_point, points_xyz = node_point.clone().contiguous(), points_xyz.clone().contiguous()
    count = torch.zeros((C, max_points), dtype=torch.int32, device=dev)
    new = torch.zeros((C, max_points), dtype=torch.uint8, device=dev)
    error = torch.full((C, max_points), float("nan"), dtype=torch.float64, device=dev)
    if C == 0:
        return node_point, points_xyz, count, new.bool(), error
    off64 = offsets.to(torch.int64)
    if int(off64[0]) != 0 or int(off64[-1]) != total or bool((off64[1:] < off64[:-1]).any()):
        raise ValueError("split_tracks needs offsets that ascend from 0 to the number of nodes")
    lib = _lib.load()
    obs_xy, obs_cam, offsets, cams, seeds = (t.contiguous() for t in (obs_xy, obs_cam, offsets, cams, seeds))
    _lib.check(lib.vc_split_tracks(_lib.ptr(obs_xy), _lib.ptr(obs_cam), _lib.ptr(offsets), C, _lib.ptr(cams), int(cams.shape[0]),
                                   _lib.ptr(seeds), max_points, float(max_error), float(min_tri_angle_tan2), _lib.ptr(node_point),
                                   _lib.ptr(points_xyz), _lib.ptr(count), _lib.ptr(new), _lib.ptr(error), _lib.stream_ptr()),
               "vc_split_tracks")
    return node_point, points_xyz, count, new.bool(), error
