"""Bundle adjustment with refined intrinsics ("The border"): the loop of mapping/bundle.py over the poses,
the points and (fx, fy, cx, cy) of every group of cameras.  The intrinsics are a handful of parameters shared by many images:
they join the reduced camera system as a border, [[S, B], [B', C]] (dc, dtheta) = -(g, h), and all per-observation work stays
parallel over points.  Imported only when `bundle_adjust` is given groups; include/vitcolmap_hip.h states the rule.
Specification: tests/util_bundle_intr.py.  This build's own published rule; parity with COLMAP and Ceres is unpinned.

Where the work runs
  HIP     what mapping/bundle.py runs per iteration, with vc_ba_step_intrinsics in the place of vc_ba_step, and between the
          two reductions vc_ba_linearize_intrinsics (one point per lane: T, q, hq and the point's products with V^-1) and
          vc_ba_reduce_border (one wave per ordered sum over the points: C, h; one wave per camera: B)
  torch   the assembly of the bordered system from S, B and C, its solve in float64 on the device (cholesky_ex +
          cholesky_solve) and the loop's scalars; the decision is still one host read per iteration: the candidate's cost, NaN
          where the system did not factor or a focal length of the candidate is not finite and positive
"""
import numpy as np

from .bundle import BA_LAMBDA0, BA_LAMBDA_MAX, BA_LAMBDA_MIN, BA_REL_DECREASE, _Buffers, camera_index

HOLD_FX, HOLD_FY, HOLD_CX, HOLD_CY, TIED = 1, 2, 4, 8, 16              # the bits of a group's intr_mask (include/vitcolmap_hip.h)
# The cap on linearisations that build_adjusted_model gives the loop when it refines the focal (the loop's rule is unchanged and
# still ends when an accepted step lowers the cost by less than BA_REL_DECREASE).  A focal that needs refining has also gone
# through E, P3P and triangulation, so the grown model starts far from a minimum, where the loop alternates a rejected and an
# accepted step: with the camera 3 % off on the windowed scene it needs 166 linearisations with one tied focal and 271 with fx
# and fy (133 with the focal held), measured; BA_MAX_ITERATIONS = 25 ends it at a focal 22 % off.  The cap is about twice the
# worst measured; from a model grown under the true focal the loop ends after 6 as before.
REFINE_MAX_ITERATIONS = 500


def has_one_focal(camera):
    """The camera's model has one focal parameter, params[0] (PINHOLE and OPENCV have fx, fy)."""
    model = camera.model if isinstance(camera.model, str) else getattr(camera.model, "name", str(camera.model))
    return model in ("SIMPLE_PINHOLE", "SIMPLE_RADIAL", "RADIAL")


def _group_intrinsics(cams, cam_group, n_groups):
    """-> float64 (n_groups, 4): (fx, fy, cx, cy) of the first slot of each group, NaN for a group without a slot."""
    out = np.full((n_groups, 4), np.nan)
    for a in range(len(cams) - 1, -1, -1):
        if 0 <= cam_group[a] < n_groups:
            out[cam_group[a]] = cams[a, 12:16]
    return out


def bundle_adjust_intrinsics(cams, points, offsets, obs_cam, obs_xy, const_mask, cam_group, intr_mask, device, max_iterations):
    """The arrays of `bundle.bundle_adjust`, validated by it, and cam_group int32 (n_cams,) (a slot whose group is outside
    [0, n_groups) keeps its intrinsics), intr_mask uint8 (n_groups,) (bits 0-3: fx, fy, cx, cy held; bit 4: fx and fy tied)
    -> cams, points, report; the report gains intrinsics = dict(before (n_groups, 4), after (n_groups, 4))."""
    import torch

    from .. import _lib

    cam_group, intr_mask = np.ascontiguousarray(cam_group, np.int32), np.ascontiguousarray(intr_mask, np.uint8)
    n_cams, n_points, total, G = len(cams), len(points), len(obs_cam), len(intr_mask)
    if cam_group.shape != (n_cams,) or intr_mask.ndim != 1 or G < 1:
        raise ValueError("bundle_adjust needs cam_group (n_cams,) and intr_mask (n_groups,) with n_groups >= 1")
    if G > _lib.VC_BA_MAX_GROUPS:
        raise ValueError(f"bundle_adjust: {G} groups of intrinsics, the border kernels hold at most {_lib.VC_BA_MAX_GROUPS} (VC_BA_MAX_GROUPS)")
    before = _group_intrinsics(cams, cam_group, G)
    report = dict(iterations=0, accepted_steps=0, initial_cost=0.0, final_cost=0.0, final_lambda=BA_LAMBDA0, decisions=[],
                  intrinsics=dict(before=before, after=before.copy()))
    if n_cams == 0 or n_points == 0:
        return cams.copy(), points.copy(), report
    lib = _lib.load()
    dev = torch.device(device)

    def on_device(a):
        return torch.from_numpy(a).to(dev)

    cam_offsets, cam_obs, obs_point = (on_device(a) for a in camera_index(obs_cam, offsets, n_cams))
    d_offsets, d_obs_cam, d_obs_xy, d_mask = on_device(offsets), on_device(obs_cam), on_device(obs_xy), on_device(const_mask)
    d_group, d_intr = on_device(cam_group), on_device(intr_mask)
    free_c = on_device(np.array([[not (int(m) >> i) & 1 for i in range(6)] for m in const_mask], bool).reshape(-1))
    cur, cand = _Buffers(torch, n_cams, n_points, total, dev), _Buffers(torch, n_cams, n_points, total, dev)
    cur.cams.copy_(on_device(cams)), cur.points.copy_(on_device(points))
    f64 = dict(dtype=torch.float64, device=dev)
    nc, nt, rows = 6 * n_cams, 4 * G, 24 * G + 16 * G * G
    M, rhs = torch.zeros((nc + nt, nc + nt), **f64), torch.zeros(nc + nt, **f64)
    S, g = torch.zeros((nc, nc), **f64), torch.zeros(nc, **f64)
    B, C, h = torch.zeros((nc, nt), **f64), torch.zeros((nt, nt), **f64), torch.zeros(nt, **f64)
    free_t = torch.zeros(nt, dtype=torch.uint8, device=dev)
    obs_xn, T = torch.zeros((total, 2), **f64), torch.zeros((n_points, G, 12), **f64)
    terms, sums = torch.zeros((rows, n_points), **f64), torch.zeros(rows, **f64)
    dx, valid = torch.zeros((n_points, 3), **f64), torch.zeros(n_cams, dtype=torch.uint8, device=dev)
    p, stream = _lib.ptr, _lib.stream_ptr()

    def linearize(b, lam):
        _lib.check(lib.vc_ba_linearize_points(p(b.cams), n_cams, p(d_mask), p(b.points), n_points, p(d_offsets), p(d_obs_cam), p(d_obs_xy),
                                              total, float(lam), p(b.vinv), p(b.gp), p(b.cost), p(b.count), p(b.obs_ok), p(b.obs_lin),
                                              p(b.total_cost), stream), "vc_ba_linearize_points")

    lam = BA_LAMBDA0
    linearize(cur, lam)
    cost = initial = float(cur.total_cost.item())
    iterations, decisions = 1, []
    nan = torch.full((), float("nan"), **f64)
    while iterations < max_iterations:
        _lib.check(lib.vc_ba_reduce_cameras(n_cams, p(d_mask), n_points, p(d_offsets), p(d_obs_cam), total, p(cam_offsets), p(cam_obs),
                                            p(obs_point), float(lam), p(cur.vinv), p(cur.gp), p(cur.obs_ok), p(cur.obs_lin), p(S), p(g),
                                            stream), "vc_ba_reduce_cameras")
        _lib.check(lib.vc_ba_linearize_intrinsics(p(cur.cams), n_cams, p(d_group), G, p(d_intr), p(cur.points), n_points, p(d_offsets),
                                                  p(d_obs_cam), total, p(cur.vinv), p(cur.gp), p(cur.obs_ok), p(cur.obs_lin), p(obs_xn), p(T),
                                                  p(terms), stream), "vc_ba_linearize_intrinsics")
        _lib.check(lib.vc_ba_reduce_border(n_cams, p(d_group), G, p(d_intr), n_points, p(d_offsets), p(d_obs_cam), total, p(cam_offsets),
                                           p(cam_obs), p(obs_point), float(lam), p(cur.vinv), p(cur.obs_ok), p(cur.obs_lin), p(obs_xn), p(T),
                                           p(terms), p(sums), p(B), p(C), p(h), p(free_t), stream), "vc_ba_reduce_border")
        M[:nc, :nc], M[:nc, nc:], M[nc:, :nc], M[nc:, nc:] = S, B, B.T, C
        rhs[:nc], rhs[nc:] = g, h
        L, info = torch.linalg.cholesky_ex(M)
        x = torch.cholesky_solve(-rhs[:, None], L)[:, 0]
        factored = (info == 0) & torch.isfinite(x).all()
        # a parameter that does not move steps by exactly 0; a system that did not factor still takes a (finite, zero) step
        # through the kernels, whose cost is then replaced by NaN: the decision stays one scalar read
        free = torch.cat([free_c, free_t.bool()]) & factored
        x = torch.where(free, x, torch.zeros_like(x))
        dc, dtheta = x[:nc].contiguous(), x[nc:].contiguous()
        _lib.check(lib.vc_ba_step_intrinsics(p(cur.cams), n_cams, p(d_group), G, p(d_intr), p(cur.points), n_points, p(d_offsets),
                                             p(d_obs_cam), total, p(cur.vinv), p(cur.gp), p(cur.obs_ok), p(cur.obs_lin), p(T), p(dc),
                                             p(dtheta), p(cand.cams), p(cand.points), p(dx), p(valid), stream), "vc_ba_step_intrinsics")
        lower = max(lam / 10, BA_LAMBDA_MIN)
        linearize(cand, lower)
        iterations += 1
        c = float(torch.where(factored & valid.bool().all(), cand.total_cost[0], nan).item())
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
                  decisions=decisions, intrinsics=dict(before=before, after=_group_intrinsics(out_cams, cam_group, G)))
    return out_cams, cur.points.cpu().numpy(), report
