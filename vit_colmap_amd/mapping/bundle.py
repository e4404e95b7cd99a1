"""Bundle adjustment of the grown model: one global Levenberg-Marquardt over every pose and every point
by the Schur complement of the points, on the kernels of csrc/bundle.hip, whose header (include/vitcolmap_hip.h) states
the rule; then the rescale to a unit baseline and the filter of observations and points.  Specification:
tests/util_bundle.py.  This build's own published rule; parity with COLMAP's bundle adjuster and with Ceres is unpinned.
With `refine_focal_length` the adjustment also refines the focal length(s) of every camera (one group of intrinsics per
camera_id, a border of the reduced system, which mapping/bundle_intr.py, imported only then, supplies to the one loop here;
specification: tests/util_bundle_intr.py).  With `loss` "huber" or "soft_l1" the adjustment is iteratively reweighted
Gauss-Newton under that loss ("The loss" in §4.2k; specification: tests/util_bundle_loss.py): the same loop on
vc_ba_linearize_points_loss, whose outputs the other kernels take as they are.  With `refine_distortion` it also refines the radial
distortion of SIMPLE_RADIAL (k1) and RADIAL (k1, k2) cameras from the values their params carry ("The distortion" in §4.2k;
specification: tests/util_bundle_radial.py): the same loop on the _radial entry points, six unknowns per group in the border.
With `known_distortion` the grown model was solved on undistorted keypoints; the adjustment then takes the raw
observations and the known (k1, k2) of every camera as `cam_dist`, held unless refine_distortion frees them.
With `solver` "pcg" ("The solver" in §4.2k; specification: tests/util_bundle_pcg.py) the reduced system is not formed: it is
solved by preconditioned conjugate gradients on vc_ba_camera_blocks and vc_ba_schur_product, for any number of cameras, poses
and points only.
The same adjustment after every growth round, with the tracks re-evaluated, is mapping/rounds.py (§4.2m).
With `tangential` ("The tangential terms" in §4.2k; specification: tests/util_bundle_opencv.py) OPENCV cameras are adjusted too:
`cam_dist` then carries (k1, k2, p1, p2), the loop runs the _opencv entry points and the border has eight unknowns per group.
Still missing on the way to a mapper: local adjustment, merging of points.

Where the work runs
  HIP     per iteration vc_ba_linearize_points (one point per lane: residuals, Jacobians, V^-1, the cost), vc_ba_reduce_cameras
          (one workgroup per camera: the reduced system S, g) and vc_ba_step (back-substitution, the trig-free pose update)
  torch   the solve of S dc = -g (with a border: of the bordered system) in float64 on the device (cholesky_ex +
          cholesky_solve) and the loop's scalars; the accept / reject decision is the only host read of an iteration: one
          number, the candidate's cost (NaN where the system did not factor); under solver "pcg" the vector updates and dot
          products of conjugate gradients, and one more host read per product: |r|^2 for the stopping test
  host    Python / numpy: the model's arrays, the camera-major index, the gauge, the rescale, the filter
"""
import copy
import logging

import numpy as np

from ..database.colmap_db import _quat_to_rot
from ..matching._common import MAX_ERROR
from ..matching.essential import rot_to_quat
from .absolute_pose import FILTER_MIN_TRI_ANGLE
from .grow import build_sparse_model
from .seed import SparseModel, _pixel_errors, _pixel_errors_opencv, _pixel_errors_radial, _read_database

logger = logging.getLogger(__name__)

BA_LAMBDA0 = 1e-4
BA_LAMBDA_MIN, BA_LAMBDA_MAX = 1e-12, 1e12
BA_MAX_ITERATIONS = 25               # linearisations
BA_REL_DECREASE = 1e-8
HELD_ALL = 63                        # bits 0-2: the rotation, bits 3-5: the translation
LOSSES = {"trivial": 0, "huber": 1, "soft_l1": 2}      # VC_BA_LOSS_* (include/vitcolmap_hip.h)
SOLVERS = ("dense", "pcg")           # how S dc = -g is solved ("The solver" in §4.2k)
PCG_REL_TOL = 1e-6                   # |r| <= PCG_REL_TOL |r_0| ends a solve
PCG_MAX_ITERATIONS = 500             # [recalled: Ceres' default max_linear_solver_iterations]
MIN_TRI_ANGLE_TAN2 = float(np.tan(FILTER_MIN_TRI_ANGLE) ** 2)


def camera_index(obs_cam, offsets, n_cams):
    """-> cam_offsets int32 (n_cams + 1,), cam_obs int32 (total,): per camera its observations in ascending order (one whose
    slot is outside [0, n_cams) belongs to none, the tail of cam_obs is then -1), obs_point int32 (total,)."""
    obs_cam, offsets = np.asarray(obs_cam, np.int64), np.asarray(offsets, np.int64)
    total = len(obs_cam)
    inside = (obs_cam >= 0) & (obs_cam < n_cams)
    order = np.argsort(np.where(inside, obs_cam, n_cams), kind="stable")[:int(inside.sum())]
    cam_obs = np.full(total, -1, np.int32)
    cam_obs[:len(order)] = order
    cam_offsets = np.concatenate([[0], np.cumsum(np.bincount(obs_cam[inside], minlength=n_cams))]).astype(np.int32)
    lo, hi = offsets[:-1], offsets[1:]
    valid = (lo >= 0) & (hi >= lo) & (hi <= total)
    obs_point = np.full(total, -1, np.int32)
    if valid.all() and len(lo) and lo[0] == 0 and hi[-1] == total and np.array_equal(lo[1:], hi[:-1]):
        obs_point[:] = np.repeat(np.arange(len(lo), dtype=np.int32), hi - lo)
    else:
        for j in np.nonzero(valid)[0]:
            obs_point[lo[j]:hi[j]] = j
    return cam_offsets, cam_obs, obs_point


class _Buffers:
    """The outputs of one vc_ba_linearize_points call (with a loss: of vc_ba_linearize_points_loss, obs_w among them); two of
    them alternate between the current parameters and the candidate."""

    def __init__(self, torch, n_cams, n_points, total, device, with_loss=False, with_dist=0):
        f64 = dict(dtype=torch.float64, device=device)
        self.cams, self.points = torch.zeros((n_cams, 16), **f64), torch.zeros((n_points, 3), **f64)
        self.vinv, self.gp, self.cost = torch.zeros((n_points, 6), **f64), torch.zeros((n_points, 3), **f64), torch.zeros(n_points, **f64)
        self.count = torch.zeros(n_points, dtype=torch.int32, device=device)
        self.obs_ok = torch.zeros(total, dtype=torch.uint8, device=device)
        self.obs_lin = torch.zeros((total, 32), **f64)
        self.total_cost = torch.zeros(1, **f64)
        if with_loss or with_dist:
            self.obs_w = torch.zeros(total, **f64)
        if with_dist:
            # (k1, k2) beside the camera rows (the _radial entry points), or (k1, k2, p1, p2) (the _opencv ones): with_dist columns
            self.dist = torch.zeros((n_cams, int(with_dist)), **f64)


def check_loss(loss, loss_scale):
    """-> (VC_BA_LOSS_* of the name, the scale as a float); ValueError, naming the options, for anything else."""
    if loss not in LOSSES:
        raise ValueError(f"bundle_adjust: unknown loss {loss!r}, expected one of {', '.join(LOSSES)}")
    try:
        scale = float(loss_scale)
    except (TypeError, ValueError):
        scale = float("nan")
    if not 0.0 < scale < float("inf"):
        raise ValueError(f"bundle_adjust: loss_scale must be a finite positive number of pixels (got {loss_scale!r}); the losses are "
                         f"{', '.join(LOSSES)}")
    return LOSSES[loss], scale


def check_solver(solver):
    """ValueError, naming the options, for a solver that is none of SOLVERS."""
    if solver not in SOLVERS:
        raise ValueError(f"bundle_adjust: unknown solver {solver!r}, expected one of {', '.join(SOLVERS)}")


class _Pcg:
    """S dc = -g by preconditioned conjugate gradients without S ("The solver" in §4.2k): vc_ba_camera_blocks once per solve,
    vc_ba_schur_product (two launches) once per iteration, the vector updates and dot products in torch float64 on the device,
    M^-1 r a batched 6x6 product.  One host read per iteration: |r|^2, NaN where p'q is not finite and positive."""

    def __init__(self, torch, lib, n_cams, n_points, device, tol, max_iterations):
        f64 = dict(dtype=torch.float64, device=device)
        self.torch, self.lib, self.n_cams, self.tol, self.max_iterations = torch, lib, n_cams, float(tol), int(max_iterations)
        self.U, self.D, self.Minv = (torch.zeros((n_cams, 36), **f64) for _ in range(3))
        self.g, self.q = torch.zeros(6 * n_cams, **f64), torch.zeros(6 * n_cams, **f64)
        self.fixed = torch.zeros(6 * n_cams, dtype=torch.uint8, device=device)
        self.s = torch.zeros((max(n_points, 1), 3), **f64)
        self.nan = torch.full((), float("nan"), **f64)

    def solve(self, launch_blocks, launch_product):
        """launch_blocks(self) and launch_product(self, p) call the two entry points on the current linearisation -> (x, a 0-dim
        bool tensor: the solve ended well, the number of products)."""
        torch = self.torch
        launch_blocks(self)
        free = self.fixed == 0
        Minv = self.Minv.view(-1, 6, 6)

        def precondition(r):
            return (Minv * r.view(-1, 1, 6)).sum(dim=2).reshape(-1)

        x = torch.zeros_like(self.g)
        r = torch.where(free, -self.g, torch.zeros_like(self.g))
        rr0 = float(torch.dot(r, r).item())
        if rr0 == 0.0:
            return x, torch.ones((), dtype=torch.bool, device=x.device), 0
        if not np.isfinite(rr0):
            return x, torch.zeros((), dtype=torch.bool, device=x.device), 0
        bound = self.tol * float(np.sqrt(rr0))
        z = precondition(r)
        p, rz = z.clone(), torch.dot(r, z)
        k, well = 0, True
        while k < self.max_iterations:
            k += 1
            launch_product(self, p.contiguous())
            pq = torch.dot(p, self.q)
            alpha = rz / pq
            x = x + alpha * p
            r = r - alpha * self.q
            rr = float(torch.where(torch.isfinite(pq) & (pq > 0), torch.dot(r, r), self.nan).item())    # the iteration's host read
            if not np.isfinite(rr):
                well = False
                break
            if float(np.sqrt(rr)) <= bound:
                break
            z = precondition(r)
            rz_new = torch.dot(r, z)
            p, rz = z + (rz_new / rz) * p, rz_new
        # a non-finite x stays non-finite under every later update, so one test here is the rule's test after every update
        ended_well = torch.isfinite(x).all() & torch.tensor(well, device=x.device)
        return torch.where(free, x, torch.zeros_like(x)), ended_well, k


def bundle_adjust(cams, points, offsets, obs_cam, obs_xy, const_mask, device="cuda", max_iterations=BA_MAX_ITERATIONS, cam_group=None,
                  intr_mask=None, loss="trivial", loss_scale=1.0, cam_dist=None, solver="dense", pcg_tol=PCG_REL_TOL,
                  pcg_max_iterations=PCG_MAX_ITERATIONS):
    """cams float64 (n_cams, 16) as vc_triangulate_tracks has them, points float64 (n_points, 3), offsets int32 (n_points + 1,),
    obs_cam int32 (total,), obs_xy float64 (total, 2), const_mask uint8 (n_cams,) (bit i: pose parameter i is held), numpy
    -> cams, points (numpy, adjusted) and the report dict(iterations, accepted_steps, initial_cost, final_cost, final_lambda,
    decisions).  Raises ValueError above VC_BA_MAX_CAMS cameras.
    cam_group int32 (n_cams,) and intr_mask uint8 (n_groups,), both or neither: the intrinsics of every group of cameras are
    refined too (mapping/bundle_intr.py; bits 0-3 of a group's mask: fx, fy, cx, cy held, bit 4: fx and fy tied; a slot whose
    group is outside [0, n_groups) keeps its intrinsics), the report gains `intrinsics` = dict(before, after), (n_groups, 4)
    each.  Raises ValueError above VC_BA_MAX_GROUPS groups.
    loss "trivial", "huber" or "soft_l1" with loss_scale in px ("The loss" in §4.2k): with "trivial" exactly today's calls;
    otherwise vc_ba_linearize_points_loss and, with groups, the border's _loss entry points; the costs of the report are the
    robust ones.  The report carries loss and loss_scale.  Raises ValueError for an unknown loss or a scale that is not finite
    and positive.
    cam_dist float64 (n_cams, 2): (k1, k2) of every slot ("The distortion" in §4.2k; COLMAP's SIMPLE_RADIAL and RADIAL).  The same
    loop then runs the _radial entry points, with any loss; bits 5 and 6 of a group's mask hold k1 and k2; without groups every
    slot is in one group whose six intrinsics are all held.  The report gains `cam_dist`, the adjusted (n_cams, 2), and its
    `intrinsics` are (n_groups, 6): (fx, fy, cx, cy, k1, k2).  Raises ValueError above VC_BA_MAX_GROUPS_RADIAL groups.  Without
    cam_dist exactly the calls and the report described above.
    cam_dist float64 (n_cams, 4): (k1, k2, p1, p2) of every slot ("The tangential terms" in §4.2k; COLMAP's OPENCV).  The loop runs
    the _opencv entry points; bit 7 of a group's mask holds p1 and p2 together; the report's `cam_dist` is (n_cams, 4) and its
    `intrinsics` are (n_groups, 8): (fx, fy, cx, cy, k1, k2, p1, p2).  Raises ValueError above VC_BA_MAX_GROUPS_OPENCV groups.
    solver "dense" or "pcg" ("The solver" in §4.2k).  "dense" is everything above, the ValueError above VC_BA_MAX_CAMS included.
    "pcg" solves S dc = -g by preconditioned conjugate gradients (block-Jacobi, |r| <= pcg_tol |r_0| or pcg_max_iterations
    products) on vc_ba_camera_blocks and vc_ba_schur_product: S is not allocated and there is no limit on the cameras; a solve
    that ends on a p'q that is not finite and positive, or on a non-finite x, is what a system that did not factor is.  The report
    gains `solver` and `pcg_iterations`, one count per solve.  With cam_group, intr_mask or cam_dist "pcg" raises ValueError:
    the border needs the dense solver.  Raises ValueError for an unknown solver."""
    import torch

    from .. import _lib

    cams = np.ascontiguousarray(cams, np.float64).reshape(-1, 16)
    points = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    offsets, obs_cam = np.ascontiguousarray(offsets, np.int32), np.ascontiguousarray(obs_cam, np.int32)
    obs_xy, const_mask = np.ascontiguousarray(obs_xy, np.float64).reshape(-1, 2), np.ascontiguousarray(const_mask, np.uint8)
    n_cams, n_points, total = len(cams), len(points), len(obs_cam)
    loss_kind, loss_scale = check_loss(loss, loss_scale)
    check_solver(solver)
    pcg = solver == "pcg"
    if pcg and (cam_group is not None or intr_mask is not None or cam_dist is not None):
        raise ValueError("bundle_adjust: solver 'pcg' solves the cameras' system alone; cam_group, intr_mask and cam_dist add a border "
                         "to it, which needs the dense solver (solver='dense')")
    if not pcg and n_cams > _lib.VC_BA_MAX_CAMS:
        raise ValueError(f"bundle_adjust: {n_cams} cameras, the reduction kernel holds at most {_lib.VC_BA_MAX_CAMS} (VC_BA_MAX_CAMS)")
    if offsets.shape != (n_points + 1,) or obs_xy.shape != (total, 2) or const_mask.shape != (n_cams,):
        raise ValueError("bundle_adjust needs offsets (n_points + 1,), obs_cam (total,), obs_xy (total, 2), const_mask (n_cams,)")
    border = None
    radial = cam_dist is not None
    if radial:
        cam_dist = np.ascontiguousarray(cam_dist, np.float64)
        if cam_dist.shape not in ((n_cams, 2), (n_cams, 4)):
            raise ValueError("bundle_adjust needs cam_dist (n_cams, 2): k1, k2 of every camera slot, or (n_cams, 4): k1, k2, p1, p2")
        if cam_group is None and intr_mask is None:
            from .bundle_intr import HOLD_ALL_OPENCV, HOLD_ALL_RADIAL

            cam_group = np.zeros(n_cams, np.int32)
            intr_mask = np.array([HOLD_ALL_OPENCV if cam_dist.shape[1] == 4 else HOLD_ALL_RADIAL], np.uint8)
    if cam_group is not None or intr_mask is not None:
        if cam_group is None or intr_mask is None:
            raise ValueError("bundle_adjust needs cam_group and intr_mask together")
        from .bundle_intr import Border

        border = Border(cams, cam_group, intr_mask, with_loss=loss_kind != 0, cam_dist=cam_dist, loss=(loss_kind, loss_scale))
    report = dict(iterations=0, accepted_steps=0, initial_cost=0.0, final_cost=0.0, final_lambda=BA_LAMBDA0, decisions=[], loss=loss,
                  loss_scale=loss_scale)
    if pcg:
        report.update(solver=solver, pcg_iterations=[])
    if n_cams == 0 or n_points == 0:
        return cams.copy(), points.copy(), report if border is None else border.report(report, cams, cam_dist)
    lib = _lib.load()
    dev = torch.device(device)

    def on_device(a):
        return torch.from_numpy(a).to(dev)

    cam_offsets, cam_obs, obs_point = (on_device(a) for a in camera_index(obs_cam, offsets, n_cams))
    d_offsets, d_obs_cam, d_obs_xy, d_mask = on_device(offsets), on_device(obs_cam), on_device(obs_xy), on_device(const_mask)
    free = on_device(np.array([[not (int(m) >> i) & 1 for i in range(6)] for m in const_mask], bool).reshape(-1))
    cur, cand = (_Buffers(torch, n_cams, n_points, total, dev, with_loss=loss_kind != 0, with_dist=cam_dist.shape[1] if radial else 0)
                 for _ in range(2))
    cur.cams.copy_(on_device(cams)), cur.points.copy_(on_device(points))
    if radial:
        cur.dist.copy_(on_device(cam_dist))
    if not pcg:
        S = torch.zeros((6 * n_cams, 6 * n_cams), dtype=torch.float64, device=dev)
        g = torch.zeros(6 * n_cams, dtype=torch.float64, device=dev)
    dx = torch.zeros((n_points, 3), dtype=torch.float64, device=dev)
    p, stream = _lib.ptr, _lib.stream_ptr()
    if border is not None:
        border.upload(on_device, d_offsets, d_obs_cam, (cam_offsets, cam_obs, obs_point))

    def linearize(b, lam):
        if radial:
            entry = "vc_ba_linearize_points_opencv" if cam_dist.shape[1] == 4 else "vc_ba_linearize_points_radial"
            _lib.check(getattr(lib, entry)(p(b.cams), n_cams, p(b.dist), p(d_mask), p(b.points), n_points, p(d_offsets),
                                           p(d_obs_cam), p(d_obs_xy), total, float(lam), loss_kind, loss_scale, p(b.vinv),
                                           p(b.gp), p(b.cost), p(b.count), p(b.obs_ok), p(b.obs_lin), p(b.obs_w),
                                           p(b.total_cost), stream), entry)
            return
        if loss_kind != 0:
            _lib.check(lib.vc_ba_linearize_points_loss(p(b.cams), n_cams, p(d_mask), p(b.points), n_points, p(d_offsets), p(d_obs_cam),
                                                       p(d_obs_xy), total, float(lam), loss_kind, loss_scale, p(b.vinv), p(b.gp), p(b.cost),
                                                       p(b.count), p(b.obs_ok), p(b.obs_lin), p(b.obs_w), p(b.total_cost), stream),
                       "vc_ba_linearize_points_loss")
            return
        _lib.check(lib.vc_ba_linearize_points(p(b.cams), n_cams, p(d_mask), p(b.points), n_points, p(d_offsets), p(d_obs_cam), p(d_obs_xy),
                                              total, float(lam), p(b.vinv), p(b.gp), p(b.cost), p(b.count), p(b.obs_ok), p(b.obs_lin),
                                              p(b.total_cost), stream), "vc_ba_linearize_points")

    def launch_blocks(s):
        _lib.check(lib.vc_ba_camera_blocks(n_cams, p(d_mask), n_points, p(d_offsets), p(d_obs_cam), total, p(cam_offsets), p(cam_obs),
                                           p(obs_point), float(lam), p(cur.vinv), p(cur.gp), p(cur.obs_ok), p(cur.obs_lin), p(s.U), p(s.D),
                                           p(s.Minv), p(s.g), p(s.fixed), stream), "vc_ba_camera_blocks")

    def launch_product(s, vector):
        _lib.check(lib.vc_ba_schur_product(n_cams, n_points, p(d_offsets), p(d_obs_cam), total, p(cam_offsets), p(cam_obs), p(obs_point),
                                           p(cur.vinv), p(cur.obs_ok), p(cur.obs_lin), p(s.U), p(s.fixed), p(vector), p(s.s), p(s.q), stream),
                   "vc_ba_schur_product")

    lam = BA_LAMBDA0
    linearize(cur, lam)
    cost = initial = float(cur.total_cost.item())
    iterations, decisions, pcg_counts = 1, [], []
    solve = _Pcg(torch, lib, n_cams, n_points, dev, pcg_tol, pcg_max_iterations) if pcg else None
    while iterations < max_iterations:
        if pcg:
            x, factored, products = solve.solve(launch_blocks, launch_product)
            pcg_counts.append(products)
            x = torch.where(free & factored, x, torch.zeros_like(x)).contiguous()
        else:
            _lib.check(lib.vc_ba_reduce_cameras(n_cams, p(d_mask), n_points, p(d_offsets), p(d_obs_cam), total, p(cam_offsets), p(cam_obs),
                                                p(obs_point), float(lam), p(cur.vinv), p(cur.gp), p(cur.obs_ok), p(cur.obs_lin), p(S), p(g),
                                                stream), "vc_ba_reduce_cameras")
            # the system A x = -rhs and which of its unknowns move: the cameras', or with a border the cameras' and the intrinsics'
            A, rhs, moves = (S, g, free) if border is None else border.system(cur, lam, S, g, free)
            L, info = torch.linalg.cholesky_ex(A)
            x = torch.cholesky_solve(-rhs[:, None], L)[:, 0]
            factored = (info == 0) & torch.isfinite(x).all()
            # a parameter that does not move steps by exactly 0; a system that did not factor still takes a (finite, zero) step
            # through the kernels, whose cost is then replaced by NaN: the decision stays one scalar read
            x = torch.where(moves & factored, x, torch.zeros_like(x)).contiguous()
        if border is None:
            _lib.check(lib.vc_ba_step(p(cur.cams), n_cams, p(cur.points), n_points, p(d_offsets), p(d_obs_cam), total, p(cur.vinv), p(cur.gp),
                                      p(cur.obs_ok), p(cur.obs_lin), p(x), p(cand.cams), p(cand.points), p(dx), stream), "vc_ba_step")
            usable = factored
        else:
            usable = factored & border.step(cur, cand, x, dx)
        lower = max(lam / 10, BA_LAMBDA_MIN)
        linearize(cand, lower)
        iterations += 1
        c = float(torch.where(usable, cand.total_cost[0], torch.full_like(cand.total_cost[0], float("nan"))).item())
        accepted = bool(np.isfinite(c) and c < cost)
        decisions.append(accepted)
        if accepted:
            decrease = (cost - c) / cost
            cur, cand, cost, lam = cand, cur, c, lower
            if decrease < BA_REL_DECREASE:
                break
        else:
            lam = lam * 10
            if lam > BA_LAMBDA_MAX or iterations >= max_iterations:
                break
            linearize(cur, lam)
            iterations += 1
    out_cams = cur.cams.cpu().numpy()
    report = dict(iterations=iterations, accepted_steps=int(sum(decisions)), initial_cost=initial, final_cost=cost, final_lambda=lam,
                  decisions=decisions, loss=loss, loss_scale=loss_scale)
    if pcg:
        report.update(solver=solver, pcg_iterations=pcg_counts)
    return out_cams, cur.points.cpu().numpy(), (report if border is None else
                                                border.report(report, out_cams, cur.dist.cpu().numpy() if radial else None))


def _wide(X, centres, tan2=MIN_TRI_ANGLE_TAN2):
    """Some pair of the centres sees X under enough parallax (the test of §4.2j)."""
    gq = X - centres
    dots = gq @ gq.T
    cross2 = (np.cross(gq[:, None, :], gq[None, :, :]) ** 2).sum(axis=2)
    return bool(np.any(np.triu(np.ones_like(dots, bool), 1) & ((dots <= 0) | (cross2 >= tan2 * dots * dots))))


def build_adjusted_model(database_path, device="cuda", two_view_pose_fn=None, estimate_fn=None, triangulate_fn=None, bundle_fn=None,
                         grown=None, refine_focal_length=False, loss="trivial", loss_scale=1.0, refine_distortion=False,
                         known_distortion=False, undistort_fn=None, solver="dense", split_tracks=False, split_fn=None,
                         tangential=False) -> SparseModel:
    """Read a matched database -> the grown model (build_sparse_model, or `grown` where the caller has built it already; it
    is not changed), adjusted once over all poses and points, rescaled to a unit baseline of the initial pair and filtered.
    Raises the seed model's ValueErrors unchanged.  `bundle_fn(cams, points, offsets, obs_cam, obs_xy, const_mask, device) ->
    (cams, points, report)` on numpy arrays replaces the adjustment (tests), the other three as in build_sparse_model.
    `refine_focal_length`: the adjustment also refines the focal length(s) of every camera of the registered images (one
    group per camera_id: one parameter where the model has one focal length, fx and fy for PINHOLE and OPENCV; the principal
    point is held); bundle_fn is then also given cam_group=, intr_mask= and max_iterations=REFINE_MAX_ITERATIONS (the same
    loop under a higher cap: a model grown under a wrong focal starts far from a minimum), the model's cameras carry the refined values, the
    filter and `error` use them and the report gains `intrinsics` {camera_id: dict(before, after)}.  Raises ValueError above
    VC_BA_MAX_GROUPS cameras.
    `loss`, `loss_scale`: the loss of the adjustment ("The loss" in §4.2k); bundle_fn is given loss= and loss_scale= only when
    the loss is not "trivial", and `stats()["bundle_adjustment"]` carries them then.  The filter stays MAX_ERROR px on the
    unweighted error.  Raises ValueError for an unknown loss or a scale that is not finite and positive.
    `refine_distortion` ("The distortion" in §4.2k): the adjustment also refines the radial distortion, one group per camera_id as
    for the focal: k1 of a SIMPLE_RADIAL camera, k1 and k2 of a RADIAL one, from the values in the camera's params (0 where the
    pipeline wrote them); every other model keeps both held, which is logged once per camera, and where no registered camera
    has a radial parameter a ValueError names the two models.  Alone the flag holds fx, fy, cx, cy; with refine_focal_length both
    are free.  bundle_fn is then also given cam_group=, intr_mask= (bit 5: k1 held, bit 6: k2 held), max_iterations=
    REFINE_MAX_ITERATIONS and cam_dist= (n_cams, 2), and its report carries `cam_dist`; the cameras carry the refined k (params[3],
    or params[3:5]), the filter and `error` use the distorted projection and `intrinsics` has six numbers per camera: fx, fy, cx,
    cy, k1, k2.  Raises ValueError above VC_BA_MAX_GROUPS_RADIAL cameras.
    `known_distortion` (§4.2l; `undistort_fn` as in build_sparse_model, used only where `grown` is not given): the model was grown on
    undistorted keypoints and its `xys` are the raw ones, so the adjustment gets the raw observations and, where a registered
    camera has a non-zero k, cam_dist= the known (k1, k2) of every slot: held without refine_distortion (with refine_focal_length
    alone the groups then carry bits 5 and 6 and the limit is VC_BA_MAX_GROUPS_RADIAL), the starting values with it, as
    before.  The filter and `error` use the distorted projection.  Without the option exactly the calls described above.
    `solver` ("The solver" in §4.2k): "dense", exactly the calls described above, or "pcg": bundle_fn is then also given
    solver="pcg", `stats()["bundle_adjustment"]` carries solver and pcg_iterations, and there is no limit on the registered images.
    With refine_focal_length, refine_distortion or known_distortion "pcg" raises ValueError: they add a border to the system or
    take the _radial (or _opencv) entry points, which need the dense solver.  Raises ValueError for an unknown solver.
    `split_tracks`, `split_fn` (§4.2n) as in build_sparse_model, which is given them only where the flag is on and `grown` is not
    given; the model keeps the grown model's split_components and split_points either way.
    `tangential` ("The tangential terms" in §4.2k): build_sparse_model is given it, so OPENCV cameras are mapped, and where a
    registered camera is OPENCV the adjustment takes the four-number path: cam_dist= is (n_cams, 4), (k1, k2, p1, p2) of every slot
    (p = 0 for the other models), the groups carry bit 7 (HOLD_TANGENTIAL: p1 and p2 held) beside bits 5 and 6, and the limit is
    VC_BA_MAX_GROUPS_OPENCV.  With refine_distortion an OPENCV camera frees k1, k2, p1 and p2 and gets them back in params[4:8];
    SIMPLE_RADIAL and RADIAL cameras beside it keep bit 7 and their p at 0, every other model holds all four; `intrinsics` has eight
    numbers per camera.  With known_distortion alone the known four are held; with refine_focal_length alone the groups carry bits
    5, 6 and 7.  The filter and `error` use the full distorted projection.  Where no registered camera is OPENCV, and with the flag
    off, exactly the calls described above."""
    bundle_fn = bundle_fn or bundle_adjust
    check_loss(loss, loss_scale)
    check_solver(solver)
    if solver != "dense" and (refine_focal_length or refine_distortion or known_distortion):
        raise ValueError(f"solver {solver!r} adjusts poses and points only: refine_focal_length, refine_distortion and known_distortion go "
                         "through the border of the system or the _radial entry points, which need the dense solver (out of scope of pcg)")
    solver_args = {} if solver == "dense" else dict(solver=solver)
    loss_args = {} if loss == "trivial" else dict(loss=loss, loss_scale=float(loss_scale))
    if grown is None:
        known_args = dict(known_distortion=True, undistort_fn=undistort_fn) if known_distortion else {}
        if split_tracks:
            known_args.update(split_tracks=True, split_fn=split_fn)
        if tangential:
            known_args.update(tangential=True)
        grown = build_sparse_model(database_path, device, two_view_pose_fn, estimate_fn, triangulate_fn, **known_args)
    ids, pids = sorted(grown.images), sorted(grown.points3D)
    slot = {i: s for s, i in enumerate(ids)}
    known_dist = None
    # the four-number path ("The tangential terms" in §4.2k): only where a registered camera is OPENCV
    opencv = bool(tangential) and any(grown.cameras[grown.images[i]["camera_id"]].model == "OPENCV" for i in ids)
    n_dist = 4 if opencv else 2
    if known_distortion:
        from ..matching.undistort import camera_calibration

        calibration = {i: camera_calibration(grown.cameras[grown.images[i]["camera_id"]]) for i in ids}
        K = {i: c[0] for i, c in calibration.items()}
        if any(c[1].any() for c in calibration.values()):
            known_dist = np.array([calibration[i][1][:n_dist] for i in ids], np.float64).reshape(-1, n_dist)
    elif opencv:
        _, _, K, _, _ = _read_database(database_path, tangential=True)
    else:
        _, _, K, _, _ = _read_database(database_path)
    cams = np.stack([np.concatenate([_quat_to_rot(grown.images[i]["qvec"]).reshape(9), np.asarray(grown.images[i]["tvec"], np.float64),
                                     [K[i][0, 0], K[i][1, 1], K[i][0, 2], K[i][1, 2]]]) for i in ids])
    points = np.array([grown.points3D[pid]["xyz"] for pid in pids], np.float64).reshape(-1, 3)
    tracks = [grown.points3D[pid]["track"] for pid in pids]
    offsets = np.concatenate([[0], np.cumsum([len(t) for t in tracks])]).astype(np.int32)
    obs_cam = np.array([slot[i] for t in tracks for i, _ in t], np.int32)
    obs_xy = np.array([grown.images[i]["xys"][kp] for t in tracks for i, kp in t], np.float64).reshape(-1, 2)

    # the gauge: the pair's first image held, of the second the translation coordinate of largest magnitude
    # [recalled: COLMAP holds one coordinate of the second image]
    a, b = (slot[i] for i in grown.initial_pair)
    mask = np.zeros(len(ids), np.uint8)
    mask[a] = HELD_ALL
    mask[b] = 1 << (3 + int(np.argmax(np.abs(cams[b, 9:12]))))
    dist = None
    if refine_distortion:
        from .. import _lib
        from .bundle_intr import (HOLD_CX, HOLD_CY, HOLD_FX, HOLD_FY, HOLD_K1, HOLD_K2, HOLD_TANGENTIAL, REFINE_MAX_ITERATIONS, TIED,
                                  has_one_focal, is_opencv, radial_parameters)

        cids = sorted({grown.images[i]["camera_id"] for i in ids})
        n_radial = [radial_parameters(grown.cameras[c]) for c in cids]
        free_all = [opencv and is_opencv(grown.cameras[c]) for c in cids]       # an OPENCV camera frees k1, k2, p1 and p2
        if not any(n_radial) and not any(free_all):
            raise ValueError("refine_distortion: no registered camera has a radial parameter to refine; the camera models with one are "
                             "SIMPLE_RADIAL (k) and RADIAL (k1, k2)" + (" and OPENCV (k1, k2, p1, p2)" if tangential else ""))
        if opencv and len(cids) > _lib.VC_BA_MAX_GROUPS_OPENCV:
            raise ValueError(f"refine_distortion: the registered images have {len(cids)} cameras, the OPENCV border kernels hold at most "
                             f"{_lib.VC_BA_MAX_GROUPS_OPENCV} groups of intrinsics (VC_BA_MAX_GROUPS_OPENCV)")
        if not opencv and len(cids) > _lib.VC_BA_MAX_GROUPS_RADIAL:
            raise ValueError(f"refine_distortion: the registered images have {len(cids)} cameras, the radial border kernels hold at most "
                             f"{_lib.VC_BA_MAX_GROUPS_RADIAL} groups of intrinsics (VC_BA_MAX_GROUPS_RADIAL)")
        for c, n, every in zip(cids, n_radial, free_all):
            if not n and not every:
                logger.info("refine_distortion: camera %d is %s, which has no radial parameter here; its k1 and k2 stay held", c,
                            grown.cameras[c].model)
        cam_group = np.array([cids.index(grown.images[i]["camera_id"]) for i in ids], np.int32)
        # the focal as refine_focal_length frees it, or held; then k1 (SIMPLE_RADIAL, RADIAL) and k2 (RADIAL)
        focal = [HOLD_CX | HOLD_CY | (TIED if has_one_focal(grown.cameras[c]) else 0) if refine_focal_length else
                 HOLD_FX | HOLD_FY | HOLD_CX | HOLD_CY for c in cids]
        intr_mask = np.array([f | (HOLD_K1 if n < 1 else 0) | (HOLD_K2 if n < 2 else 0) for f, n in zip(focal, n_radial)], np.uint8)
        group_dist = np.array([[float(v) for v in list(grown.cameras[c].params[3:3 + n]) + [0.0] * (n_dist - n)] for c, n in zip(cids, n_radial)])
        if opencv:                                                   # every model but OPENCV keeps bit 7 and its p at 0
            intr_mask = np.array([f if every else m | HOLD_TANGENTIAL for f, m, every in zip(focal, intr_mask, free_all)], np.uint8)
            for g, (c, every) in enumerate(zip(cids, free_all)):
                if every:
                    group_dist[g] = [float(v) for v in grown.cameras[c].params[4:8]]
        cams, points, report = bundle_fn(cams, points, offsets, obs_cam, obs_xy, mask, device, cam_group=cam_group, intr_mask=intr_mask,
                                         max_iterations=REFINE_MAX_ITERATIONS, cam_dist=group_dist[cam_group], **loss_args)
        dist = np.array(report["cam_dist"], np.float64).reshape(-1, n_dist)
    elif refine_focal_length:
        from .. import _lib
        from .bundle_intr import HOLD_CX, HOLD_CY, HOLD_K1, HOLD_K2, HOLD_TANGENTIAL, REFINE_MAX_ITERATIONS, TIED, has_one_focal

        cids = sorted({grown.images[i]["camera_id"] for i in ids})
        limit, name = ((_lib.VC_BA_MAX_GROUPS, "VC_BA_MAX_GROUPS") if known_dist is None else
                       (_lib.VC_BA_MAX_GROUPS_OPENCV, "VC_BA_MAX_GROUPS_OPENCV") if opencv else
                       (_lib.VC_BA_MAX_GROUPS_RADIAL, "VC_BA_MAX_GROUPS_RADIAL"))
        if len(cids) > limit:
            raise ValueError(f"refine_focal_length: the registered images have {len(cids)} cameras, the border kernels hold at most "
                             f"{limit} groups of intrinsics ({name})")
        cam_group = np.array([cids.index(grown.images[i]["camera_id"]) for i in ids], np.int32)
        intr_mask = np.array([HOLD_CX | HOLD_CY | (TIED if has_one_focal(grown.cameras[c]) else 0) for c in cids], np.uint8)
        if known_dist is None:
            cams, points, report = bundle_fn(cams, points, offsets, obs_cam, obs_xy, mask, device, cam_group=cam_group, intr_mask=intr_mask,
                                             max_iterations=REFINE_MAX_ITERATIONS, **loss_args)
        else:                                                    # the known k stays held beside the free focal (§4.2l)
            cams, points, report = bundle_fn(cams, points, offsets, obs_cam, obs_xy, mask, device, cam_group=cam_group,
                                             intr_mask=intr_mask | np.uint8(HOLD_K1 | HOLD_K2 | (HOLD_TANGENTIAL if opencv else 0)),
                                             max_iterations=REFINE_MAX_ITERATIONS,
                                             cam_dist=known_dist, **loss_args)
            dist = known_dist
    elif known_dist is not None:
        cams, points, report = bundle_fn(cams, points, offsets, obs_cam, obs_xy, mask, device, cam_dist=known_dist, **loss_args)
        dist = known_dist
    else:
        cams, points, report = bundle_fn(cams, points, offsets, obs_cam, obs_xy, mask, device, **loss_args, **solver_args)
    cams, points = np.array(cams, np.float64), np.array(points, np.float64)

    # every t and X rescaled so that the pair's baseline is 1 again (§4.2i)
    centre = [-(cams[s, :9].reshape(3, 3).T @ cams[s, 9:12]) for s in (a, b)]
    scale = 1.0 / np.linalg.norm(centre[1] - centre[0])
    cams[:, 9:12] = cams[:, 9:12] * scale
    points = points * scale

    model = SparseModel(initial_pair=grown.initial_pair, rounds=grown.rounds,
                        bundle_adjustment={k: v for k, v in report.items()
                                           if k not in ("decisions", "intrinsics", "loss", "loss_scale", "cam_dist")})
    model.bundle_adjustment.update(loss_args)
    model.split_components, model.split_points = grown.split_components, grown.split_points
    model.cameras = copy.deepcopy(grown.cameras)
    if refine_distortion:
        # the cameras carry the refined k: params[3] of SIMPLE_RADIAL, params[3:5] of RADIAL; the filter and `error` use it
        # and params[4:8] of OPENCV (k1, k2, p1, p2)
        for g, (cid, n, every) in enumerate(zip(cids, n_radial, free_all)):
            cam = model.cameras[cid]
            if every:
                cam.params = list(cam.params[:4]) + [float(v) for v in report["intrinsics"]["after"][g][4:8]] + list(cam.params[8:])
            else:
                cam.params = list(cam.params[:3]) + [float(v) for v in report["intrinsics"]["after"][g][4:4 + n]] + list(cam.params[3 + n:])
    if refine_focal_length:
        # the cameras carry the refined focal length(s); the filter below and `error` use the refined K
        for g, cid in enumerate(cids):
            fx, fy = (float(v) for v in report["intrinsics"]["after"][g][:2])
            cam = model.cameras[cid]
            cam.params = [fx] + list(cam.params[1:]) if has_one_focal(cam) else [fx, fy] + list(cam.params[2:])
    if refine_focal_length or refine_distortion:
        K = {i: np.array([[cams[slot[i], 12], 0.0, cams[slot[i], 14]], [0.0, cams[slot[i], 13], cams[slot[i], 15]], [0.0, 0.0, 1.0]]) for i in ids}
        model.bundle_adjustment["intrinsics"] = {cid: dict(before=[float(v) for v in report["intrinsics"]["before"][g]],
                                                           after=[float(v) for v in report["intrinsics"]["after"][g]])
                                                 for g, cid in enumerate(cids)}
    for i in ids:
        im, R = grown.images[i], cams[slot[i], :9].reshape(3, 3)
        model.images[i] = dict(qvec=rot_to_quat(R), tvec=cams[slot[i], 9:12].copy(), camera_id=im["camera_id"], name=im["name"],
                               xys=np.array(im["xys"], np.float64), point3D_ids=np.full(len(im["xys"]), -1, np.int64))
    # the filter: observations beyond MAX_ERROR px under the final poses, then points left with fewer than two observations or
    # without a pair of enough parallax
    dropped_obs = 0
    for j, pid in enumerate(pids):
        rows = cams[obs_cam[offsets[j]:offsets[j + 1]]]
        if dist is None:
            err = np.array([_pixel_errors(K[i], row[:9].reshape(3, 3), row[9:12], points[j][None], obs_xy[o][None])[0]
                            for o, row, (i, _) in zip(range(offsets[j], offsets[j + 1]), rows, tracks[j])])
        else:
            errors = _pixel_errors_opencv if dist.shape[1] == 4 else _pixel_errors_radial
            err = np.array([errors(K[i], dist[slot[i]], row[:9].reshape(3, 3), row[9:12], points[j][None], obs_xy[o][None])[0]
                            for o, row, (i, _) in zip(range(offsets[j], offsets[j + 1]), rows, tracks[j])])
        keep = err <= MAX_ERROR
        dropped_obs += int((~keep).sum())
        if keep.sum() < 2:
            continue
        centres = -np.einsum("nji,nj->ni", rows[keep, :9].reshape(-1, 3, 3), rows[keep, 9:12])
        if not _wide(points[j], centres):
            continue
        track = [node for node, k in zip(tracks[j], keep) if k]
        for i, kp in track:
            model.images[i]["point3D_ids"][kp] = pid
        model.points3D[pid] = dict(xyz=points[j].copy(), rgb=(0, 0, 0), error=float(err[keep].mean()), track=[(int(i), int(kp)) for i, kp in track])
    model.bundle_adjustment.update(filtered_observations=dropped_obs, filtered_points=len(pids) - len(model.points3D))
    logger.info("Bundle adjustment: %d linearisations, %d accepted steps, cost %.6g -> %.6g", report["iterations"],
                report["accepted_steps"], report["initial_cost"], report["final_cost"])
    return model
