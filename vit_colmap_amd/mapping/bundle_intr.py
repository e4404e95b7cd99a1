"""Bundle adjustment with refined intrinsics ("The border"): what the loop of mapping/bundle.py needs to run
over the poses, the points and (fx, fy, cx, cy) of every group of cameras (`Border`; the loop itself is there, once).  The intrinsics are a handful of parameters shared by many images:
they join the reduced camera system as a border, [[S, B], [B', C]] (dc, dtheta) = -(g, h), and all per-observation work stays
parallel over points.  Imported only when `bundle_adjust` is given groups; include/vitcolmap_hip.h states the rule.
Specification: tests/util_bundle_intr.py.  This build's own published rule; parity with COLMAP and Ceres is unpinned.

Where the work runs
  HIP     what mapping/bundle.py runs per iteration, with vc_ba_step_intrinsics in the place of vc_ba_step, and between the
          two reductions vc_ba_linearize_intrinsics (one point per lane: T, q, hq and the point's products with V^-1) and
          vc_ba_reduce_border (one wave per ordered sum over the points: C, h; one wave per camera: B)
  torch   the assembly of the bordered system from S, B and C here; its solve in float64 on the device (cholesky_ex +
          cholesky_solve) and the loop's scalars in mapping/bundle.py; the decision is still one host read per iteration: the candidate's cost, NaN
          where the system did not factor or a focal length of the candidate is not finite and positive
"""
import numpy as np

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


HOLD_K1, HOLD_K2 = 32, 64                                              # with the distortion: bits 5 and 6 hold k1 and k2
HOLD_ALL_RADIAL = HOLD_FX | HOLD_FY | HOLD_CX | HOLD_CY | HOLD_K1 | HOLD_K2
HOLD_TANGENTIAL = 0x80                                                 # with the tangential terms: bit 7 holds p1 and p2, both
HOLD_ALL_OPENCV = HOLD_ALL_RADIAL | HOLD_TANGENTIAL


def radial_parameters(camera):
    """How many radial parameters the camera's model has for the adjustment to refine: 1 for SIMPLE_RADIAL (k = params[3]), 2 for
    RADIAL (k1, k2 = params[3:5]), 0 for every other model."""
    model = camera.model if isinstance(camera.model, str) else getattr(camera.model, "name", str(camera.model))
    return {"SIMPLE_RADIAL": 1, "RADIAL": 2}.get(model, 0)


def is_opencv(camera):
    """The camera's model is OPENCV: k1, k2, p1, p2 = params[4:8] ("The tangential terms" in §4.2k)."""
    model = camera.model if isinstance(camera.model, str) else getattr(camera.model, "name", str(camera.model))
    return model == "OPENCV"


def _group_intrinsics(cams, cam_group, n_groups, cam_dist=None):
    """-> float64 (n_groups, 4): (fx, fy, cx, cy) of the first slot of each group, NaN for a group without a slot; with cam_dist
    (n_cams, 2) (n_groups, 6): k1, k2 after them; with cam_dist (n_cams, 4) (n_groups, 8): k1, k2, p1, p2."""
    out = np.full((n_groups, 4 if cam_dist is None else 4 + np.shape(cam_dist)[1]), np.nan)
    for a in range(len(cams) - 1, -1, -1):
        if 0 <= cam_group[a] < n_groups:
            out[cam_group[a]] = cams[a, 12:16] if cam_dist is None else np.concatenate([cams[a, 12:16], cam_dist[a]])
    return out


class Border:
    """What refined intrinsics add to the loop of `bundle.bundle_adjust`: cam_group int32 (n_cams,) (a slot whose group is outside
    [0, n_groups) keeps its intrinsics) and intr_mask uint8 (n_groups,) (bits 0-3: fx, fy, cx, cy held; bit 4: fx and fy tied),
    checked here; the border's device buffers; per iteration the bordered system of the current linearisation and the step
    under (dc, dtheta); `intrinsics` = dict(before (n_groups, 4), after (n_groups, 4)) in the report.
    With cam_dist (n_cams, 2) ("The distortion" in §4.2k) the unknowns of a group are (fx, fy, cx, cy, k1, k2): N = 6 in the place of
    4 in every shape, bits 5 and 6 of the mask hold k1 and k2, the _radial entry points run under loss = (kind, scale) and the
    buffers carry dist beside cams; the report's `intrinsics` are (n_groups, 6) and it gains `cam_dist`.
    With cam_dist (n_cams, 4) ("The tangential terms" in §4.2k) they are (fx, fy, cx, cy, k1, k2, p1, p2): N = 8, bit 7 of the mask
    holds p1 and p2 together, the _opencv entry points run and obs_jt has ten numbers per observation; the limit is
    VC_BA_MAX_GROUPS_OPENCV, and the terms buffer is sized by the G in use ((80 + 64 G) G rows per point)."""

    def __init__(self, cams, cam_group, intr_mask, with_loss=False, cam_dist=None, loss=(0, 1.0)):
        from .. import _lib

        self._lib, self.with_loss = _lib, with_loss                           # with a loss: the _loss entry points and the buffer's obs_w
        self.radial, self.loss = cam_dist is not None, loss
        self.opencv = self.radial and np.shape(cam_dist)[1] == 4                 # the _opencv entry points in the place of the _radial ones
        self.N, self.entry = (8, "opencv") if self.opencv else (6, "radial") if self.radial else (4, None)
        self.cam_group, self.intr_mask = np.ascontiguousarray(cam_group, np.int32), np.ascontiguousarray(intr_mask, np.uint8)
        self.n_cams, self.G = len(cams), len(self.intr_mask)
        if self.cam_group.shape != (self.n_cams,) or self.intr_mask.ndim != 1 or self.G < 1:
            raise ValueError("bundle_adjust needs cam_group (n_cams,) and intr_mask (n_groups,) with n_groups >= 1")
        if self.opencv and self.G > _lib.VC_BA_MAX_GROUPS_OPENCV:
            raise ValueError(f"bundle_adjust: {self.G} groups of intrinsics with tangential distortion, the OPENCV border kernels hold at "
                             f"most {_lib.VC_BA_MAX_GROUPS_OPENCV} (VC_BA_MAX_GROUPS_OPENCV)")
        if self.radial and not self.opencv and self.G > _lib.VC_BA_MAX_GROUPS_RADIAL:
            raise ValueError(f"bundle_adjust: {self.G} groups of intrinsics with distortion, the radial border kernels hold at most "
                             f"{_lib.VC_BA_MAX_GROUPS_RADIAL} (VC_BA_MAX_GROUPS_RADIAL)")
        if self.G > _lib.VC_BA_MAX_GROUPS:
            raise ValueError(f"bundle_adjust: {self.G} groups of intrinsics, the border kernels hold at most {_lib.VC_BA_MAX_GROUPS} (VC_BA_MAX_GROUPS)")
        self.before = _group_intrinsics(cams, self.cam_group, self.G, cam_dist)

    def report(self, report, cams, cam_dist=None):
        out = dict(report, intrinsics=dict(before=self.before, after=_group_intrinsics(cams, self.cam_group, self.G, cam_dist)))
        return dict(out, cam_dist=np.array(cam_dist, np.float64)) if self.radial else out

    def upload(self, on_device, offsets, obs_cam, index):
        """The loop's device tensors offsets, obs_cam and index = (cam_offsets, cam_obs, obs_point); the border's own are made."""
        import torch

        self.offsets, self.obs_cam, self.index = offsets, obs_cam, index
        self.group, self.intr = on_device(self.cam_group), on_device(self.intr_mask)
        self.n_points, self.total = len(offsets) - 1, len(obs_cam)
        f64 = dict(dtype=torch.float64, device=offsets.device)
        u8 = dict(dtype=torch.uint8, device=offsets.device)
        N = self.N
        nc, nt, rows = 6 * self.n_cams, N * self.G, (N * N + 2 * N) * self.G + N * N * self.G * self.G
        self.M, self.rhs = torch.zeros((nc + nt, nc + nt), **f64), torch.zeros(nc + nt, **f64)
        self.B, self.C, self.h = torch.zeros((nc, nt), **f64), torch.zeros((nt, nt), **f64), torch.zeros(nt, **f64)
        self.free_t, self.valid = torch.zeros(nt, **u8), torch.zeros(self.n_cams, **u8)
        # per observation what the B pass rebuilds J_theta from: (x, y), or with the distortion obs_jt's six (OPENCV: ten) numbers
        self.obs_xn = torch.zeros((self.total, 10 if self.opencv else 6 if self.radial else 2), **f64)
        self.T = torch.zeros((self.n_points, self.G, 3 * N), **f64)
        self.terms, self.sums = torch.zeros((rows, self.n_points), **f64), torch.zeros(rows, **f64)

    def system(self, cur, lam, S, g, free):
        """The border of the current linearisation -> [[S, B], [B', C]], (g, h) and which of (dc, dtheta) move."""
        import torch

        _lib, n_cams, G, n_points, total, nc = self._lib, self.n_cams, self.G, self.n_points, self.total, 6 * self.n_cams
        lib, p, stream = _lib.load(), _lib.ptr, _lib.stream_ptr()
        if self.radial:
            kind, scale = self.loss
            linearize, reduce = f"vc_ba_linearize_intrinsics_{self.entry}", f"vc_ba_reduce_border_{self.entry}"
            _lib.check(getattr(lib, linearize)(p(cur.cams), n_cams, p(cur.dist), p(self.group), G, p(self.intr), p(cur.points),
                                               n_points, p(self.offsets), p(self.obs_cam), total, kind, scale, p(cur.vinv),
                                               p(cur.gp), p(cur.obs_ok), p(cur.obs_lin), p(cur.obs_w), p(self.obs_xn), p(self.T),
                                               p(self.terms), stream), linearize)
            _lib.check(getattr(lib, reduce)(n_cams, p(self.group), G, p(self.intr), n_points, p(self.offsets), p(self.obs_cam), total,
                                            *(p(a) for a in self.index), float(lam), kind, scale, p(cur.vinv), p(cur.obs_ok),
                                            p(cur.obs_lin), p(self.obs_xn), p(cur.obs_w), p(self.T), p(self.terms), p(self.sums),
                                            p(self.B), p(self.C), p(self.h), p(self.free_t), stream), reduce)
        elif self.with_loss:
            _lib.check(lib.vc_ba_linearize_intrinsics_loss(p(cur.cams), n_cams, p(self.group), G, p(self.intr), p(cur.points), n_points,
                                                           p(self.offsets), p(self.obs_cam), total, p(cur.vinv), p(cur.gp), p(cur.obs_ok),
                                                           p(cur.obs_lin), p(cur.obs_w), p(self.obs_xn), p(self.T), p(self.terms), stream),
                       "vc_ba_linearize_intrinsics_loss")
            _lib.check(lib.vc_ba_reduce_border_loss(n_cams, p(self.group), G, p(self.intr), n_points, p(self.offsets), p(self.obs_cam), total,
                                                    *(p(a) for a in self.index), float(lam), p(cur.vinv), p(cur.obs_ok), p(cur.obs_lin),
                                                    p(self.obs_xn), p(cur.obs_w), p(self.T), p(self.terms), p(self.sums), p(self.B), p(self.C),
                                                    p(self.h), p(self.free_t), stream), "vc_ba_reduce_border_loss")
        else:
            _lib.check(lib.vc_ba_linearize_intrinsics(p(cur.cams), n_cams, p(self.group), G, p(self.intr), p(cur.points), n_points, p(self.offsets),
                                                      p(self.obs_cam), total, p(cur.vinv), p(cur.gp), p(cur.obs_ok), p(cur.obs_lin), p(self.obs_xn),
                                                      p(self.T), p(self.terms), stream), "vc_ba_linearize_intrinsics")
            _lib.check(lib.vc_ba_reduce_border(n_cams, p(self.group), G, p(self.intr), n_points, p(self.offsets), p(self.obs_cam), total,
                                               *(p(a) for a in self.index), float(lam), p(cur.vinv), p(cur.obs_ok), p(cur.obs_lin), p(self.obs_xn),
                                               p(self.T), p(self.terms), p(self.sums), p(self.B), p(self.C), p(self.h), p(self.free_t), stream),
                       "vc_ba_reduce_border")
        M, rhs = self.M, self.rhs
        M[:nc, :nc], M[:nc, nc:], M[nc:, :nc], M[nc:, nc:] = S, self.B, self.B.T, self.C
        rhs[:nc], rhs[nc:] = g, self.h
        return M, rhs, torch.cat([free, self.free_t.bool()])

    def step(self, cur, cand, x, dx):
        """The candidate under x = (dc, dtheta) -> whether all its focal lengths are finite and positive (a device scalar)."""
        _lib, nc = self._lib, 6 * self.n_cams
        p, dc, dtheta = _lib.ptr, x[:nc].contiguous(), x[nc:].contiguous()
        if self.radial:
            step = f"vc_ba_step_{self.entry}"
            _lib.check(getattr(_lib.load(), step)(p(cur.cams), self.n_cams, p(cur.dist), p(self.group), self.G, p(self.intr), p(cur.points),
                                                  self.n_points, p(self.offsets), p(self.obs_cam), self.total, p(cur.vinv), p(cur.gp),
                                                  p(cur.obs_ok), p(cur.obs_lin), p(self.T), p(dc), p(dtheta), p(cand.cams), p(cand.dist),
                                                  p(cand.points), p(dx), p(self.valid), _lib.stream_ptr()), step)
            return self.valid.bool().all()
        _lib.check(_lib.load().vc_ba_step_intrinsics(p(cur.cams), self.n_cams, p(self.group), self.G, p(self.intr), p(cur.points), self.n_points,
                                                     p(self.offsets), p(self.obs_cam), self.total, p(cur.vinv), p(cur.gp), p(cur.obs_ok),
                                                     p(cur.obs_lin), p(self.T), p(dc), p(dtheta), p(cand.cams), p(cand.points), p(dx),
                                                     p(self.valid), _lib.stream_ptr()), "vc_ba_step_intrinsics")
        return self.valid.bool().all()
