"""Helpers of the F / H verification tests (test_two_view.py, test_two_view_scoring_gpu.py, test_two_view_estimate_gpu.py):
scenes and hypotheses from oracle/two_view_oracle.py, the scoring kernels called through the ABI on buffers the test owns
(sentinel-filled, with guard elements), the power-of-two scale sweep with its float64 validity conditions, and the threshold
set: correspondences on the decision boundary, where a fused multiply-add changes the answer."""
from functools import lru_cache

import numpy as np

from oracle import two_view_oracle as tv

S_OF = {"F": 8, "H": 4}
SALT_OF = {"F": tv.SALT_F, "H": tv.SALT_H}
GUARD = 8                                  # elements allocated after every output buffer
COUNT_SENTINEL, MASK_SENTINEL = -7, 9      # what the outputs hold before the launch
FLT_MAX, FLT_MIN = float(np.finfo(np.float32).max), float(np.finfo(np.float32).tiny)
SCALE_EXPONENTS = list(range(-120, 121, 4))


def scene_pts(seed, n, outliers=0.3, planar=False):
    kp1, kp2, m, _ = tv.synthetic_two_view(seed, n, outliers, planar)
    return np.concatenate([kp1[m[:, 0]], kp2[m[:, 1]]], axis=1).astype(np.float32)


@lru_cache(maxsize=None)
def scene_hypotheses(model, seed, n, planar, k):
    """-> (pts (n, 4), hypotheses float32 (k, 9)) of one synthetic pair: the true model, its neighbours and models fitted to
    samples with outliers.  Shared between tests: never written to."""
    pts = scene_pts(seed, n, 0.3, planar)
    hyp, _ = tv.hypotheses(model, pts, 1000 + seed, k)
    pts.setflags(write=False), hyp.setflags(write=False)
    return pts, hyp


def best_hypothesis(model, seed=3, n=300, planar=None, k=64):
    """A valid model: the hypothesis of a scene with most inliers."""
    pts, hyp = scene_hypotheses(model, seed, n, model == "H" if planar is None else planar, k)
    counts = [int(tv.inliers_f32(model, h, pts).sum()) for h in hyp]
    return pts, hyp[int(np.argmax(counts))].copy()


def grid_pair(shift=0.0, nx=20, ny=15, pitch=14.0):
    """Integer keypoints on a token grid (ViT keypoints) matched one to one; image 2 is image 1 moved by `shift` px in x."""
    x, y = np.meshgrid(7.0 + pitch * np.arange(nx), 7.0 + pitch * np.arange(ny))
    kp1 = np.stack([x.reshape(-1), y.reshape(-1)], axis=1).astype(np.float32)
    kp2 = kp1 + np.array([shift, 0.0], np.float32)
    m = np.stack([np.arange(len(kp1))] * 2, axis=1).astype(np.uint32)
    return kp1, kp2, m


def ref_counts(model, hyp, pts_list, max_error=tv.MAX_ERROR):
    """hyp (P, K, 9) -> int (P, K) by the oracle, one model at a time."""
    return np.array([[int(tv.inliers_f32(model, h, pts, max_error).sum()) for h in hp] for hp, pts in zip(hyp, pts_list)],
                    np.int64).reshape(len(pts_list), hyp.shape[1])


def ref_mask(model, models, pts_list, max_error=tv.MAX_ERROR):
    """models (P, 9) -> uint8 (total,) by the oracle."""
    return np.concatenate([tv.inliers_f32(model, m, pts, max_error) for m, pts in zip(models, pts_list)] + [np.zeros(0, bool)]).astype(np.uint8)


# ---- the ABI on buffers the test owns ------------------------------------------------------------------------------------------
def device_batch(pts_list):
    """-> (pts tensor (total + GUARD, 4) whose guard rows are NaN, offsets int32 tensor) on the GPU."""
    import torch

    pts = np.concatenate(list(pts_list) + [np.full((GUARD, 4), np.nan, np.float32)]).astype(np.float32)
    offs = np.concatenate([[0], np.cumsum([len(p) for p in pts_list])]).astype(np.int32)
    return torch.from_numpy(pts).cuda(), torch.from_numpy(offs).cuda()


def _checked(buf, n, sentinel, what):
    got = buf.cpu().numpy()
    assert (got[n:] == sentinel).all(), f"{what}: a guard element was overwritten"
    assert not (got[:n] == sentinel).any(), f"{what}: {int((got[:n] == sentinel).sum())} elements were never written"
    return got[:n]


def run_score(model, pts_list, hyp, max_error=tv.MAX_ERROR, batch=None):
    """vc_two_view_score on pre-filled counts with guard elements -> int32 (P, K)."""
    import torch

    from vit_colmap_amd import _lib
    from vit_colmap_amd.matching._common import MODEL_CODE

    lib = _lib.load()
    P, K = hyp.shape[:2]
    pts, offsets = batch if batch is not None else device_batch(pts_list)
    d_h = torch.from_numpy(np.ascontiguousarray(hyp, np.float32)).cuda()
    counts = torch.full((P * K + GUARD,), COUNT_SENTINEL, dtype=torch.int32, device="cuda")
    _lib.check(lib.vc_two_view_score(_lib.ptr(pts), _lib.ptr(offsets), P, _lib.ptr(d_h), K, MODEL_CODE[model], float(max_error),
                                     _lib.ptr(counts), _lib.stream_ptr()), "vc_two_view_score")
    torch.cuda.synchronize()
    return _checked(counts, P * K, COUNT_SENTINEL, "counts").reshape(P, K)


def run_mask(model, pts_list, models, max_error=tv.MAX_ERROR, batch=None):
    """vc_two_view_inliers on a pre-filled mask with guard elements -> uint8 (total,)."""
    import torch

    from vit_colmap_amd import _lib
    from vit_colmap_amd.matching._common import MODEL_CODE

    lib = _lib.load()
    total = sum(len(p) for p in pts_list)
    pts, offsets = batch if batch is not None else device_batch(pts_list)
    d_m = torch.from_numpy(np.ascontiguousarray(models, np.float32)).cuda()
    mask = torch.full((total + GUARD,), MASK_SENTINEL, dtype=torch.uint8, device="cuda")
    _lib.check(lib.vc_two_view_inliers(_lib.ptr(pts), _lib.ptr(offsets), len(pts_list), _lib.ptr(d_m), MODEL_CODE[model],
                                       float(max_error), _lib.ptr(mask), _lib.stream_ptr()), "vc_two_view_inliers")
    torch.cuda.synchronize()
    got = _checked(mask, total, MASK_SENTINEL, "mask")
    assert ((got == 0) | (got == 1)).all()
    return got


# ---- the power-of-two scale sweep ----------------------------------------------------------------------------------------------
def scale_sweep(m9):
    """float32 (9,) -> float32 (len(SCALE_EXPONENTS), 9): the model times 2^k (entries overflow to inf and fall into the
    denormal range and to zero at the ends)."""
    with np.errstate(over="ignore", under="ignore"):
        return np.stack([(np.asarray(m9, np.float64) * 2.0 ** k).astype(np.float32) for k in SCALE_EXPONENTS])


def _terms64(model, m, pts, max_error):
    """The evaluation of inliers_f32 in float64 -> (products, sums, den, bound): every product and every sum it forms,
    the denominator and t2 * denominator, per point."""
    m = np.asarray(m, np.float64).reshape(9)
    x1, y1, x2, y2 = (pts[:, i].astype(np.float64) for i in range(4))
    t2 = float(np.float32(max_error) * np.float32(max_error))
    prods, sums = [], []

    def mul(a, b):
        prods.append(a * b)
        return prods[-1]

    def add(*v):
        s = v[0]
        for w in v[1:]:
            s = s + w
            sums.append(s)
        return s

    with np.errstate(all="ignore"):
        r0 = add(mul(m[0], x1), mul(m[1], y1), m[2])
        r1 = add(mul(m[3], x1), mul(m[4], y1), m[5])
        r2 = add(mul(m[6], x1), mul(m[7], y1), m[8])
        if model == "F":
            ft0 = add(mul(m[0], x2), mul(m[3], y2), m[6])
            ft1 = add(mul(m[1], x2), mul(m[4], y2), m[7])
            c = add(mul(x2, r0), mul(y2, r1), r2)
            den = add(mul(r0, r0), mul(r1, r1), mul(ft0, ft0), mul(ft1, ft1))
            mul(c, c)
            bound = mul(t2, den)
        else:
            dx = add(r0, -mul(x2, r2))
            dy = add(r1, -mul(y2, r2))
            add(mul(dx, dx), mul(dy, dy))
            den = mul(r2, r2)
            bound = mul(t2, den)
    return prods, sums, den, bound


def sweep_conditions(model, m9, k, pts, max_error=tv.MAX_ERROR):
    """For the model times 2^k, per point and in float64 -> (safe, dead).
    safe: the scaled entries are exact and no intermediate of the float32 evaluation overflows or underflows, so the scaled
          decision is the unscaled one (a power of two changes no rounding).  Only products can underflow with loss (a float
          sum in the denormal range is exact), so every product must be 0 or at least 4 FLT_MIN, and every product and sum at
          most FLT_MAX / 4: the factors 4 cover the float32 rounding of the intermediates that the float64 evaluation skips.
    dead: the bound t2 * den (H: t2 * pw^2) certainly overflows (>= 4 FLT_MAX), or the denominator is certainly 0: for F, den
          below an eighth of the smallest denormal, so that every one of its terms rounds to 0; for H, whose rule tests pw
          itself, a third row that is all zero.  No inlier."""
    with np.errstate(over="ignore", under="ignore"):
        scaled = (np.asarray(m9, np.float64) * 2.0 ** k).astype(np.float32)
    exact = bool(np.all(scaled.astype(np.float64) == np.asarray(m9, np.float64) * 2.0 ** k))
    prods, sums, den, bound = _terms64(model, scaled, pts, max_error)
    with np.errstate(all="ignore"):
        safe = np.full(len(pts), exact)
        for v in prods:
            safe &= (v == 0) | (np.abs(v) >= 4 * FLT_MIN)
        for v in prods + sums:
            safe &= np.abs(v) <= FLT_MAX / 4
        dead = (bound >= 4 * FLT_MAX) | ((den < 2.0 ** -152) if model == "F" else np.full(len(pts), not scaled[6:].any()))
    return safe, dead


# ---- the threshold set ---------------------------------------------------------------------------------------------------------
def residual64(model, m9, pts):
    """Pixels, float64 from the float32 matrix: Sampson distance for F, transfer distance image 1 -> image 2 for H."""
    m = np.asarray(m9, np.float32).astype(np.float64).reshape(3, 3)
    p = np.asarray(pts, np.float64)
    x1 = np.concatenate([p[..., :2], np.ones(p.shape[:-1] + (1,))], axis=-1)
    x2 = np.concatenate([p[..., 2:], np.ones(p.shape[:-1] + (1,))], axis=-1)
    a = x1 @ m.T
    with np.errstate(all="ignore"):
        if model == "F":
            b = x2 @ m
            c = (x2 * a).sum(axis=-1)
            return np.abs(c) / np.sqrt(a[..., 0] ** 2 + a[..., 1] ** 2 + b[..., 0] ** 2 + b[..., 1] ** 2)
        return np.hypot(a[..., 0] / a[..., 2] - p[..., 2], a[..., 1] / a[..., 2] - p[..., 3])


@lru_cache(maxsize=None)
def threshold_set(model, n_keep=4096, per_base=8, seed=5, max_error=tv.MAX_ERROR):
    """-> (model float32 (9,), pts float32 (n_keep, 4)): correspondences whose residual under the model is the threshold to
    within 2e-5 relative.  Built from the oracle alone: base matches are the inliers of the best hypothesis of a scene; for
    each, x2 moves along a seeded direction, the radius at which the float64 residual equals max_error is found by bisection,
    and the float32 point is placed at that radius times (1 + u), u uniform in +-2e-5."""
    rs = np.random.RandomState(seed)
    pts, m9 = best_hypothesis(model, seed=51, n=1000, k=64)
    base = pts[tv.inliers_f32(model, m9, pts, 0.5 * max_error)].astype(np.float64)
    base = base[rs.permutation(len(base))[:n_keep // per_base]]
    base = np.repeat(base, per_base, axis=0)
    ang = rs.uniform(0, 2 * np.pi, len(base))
    d = np.stack([np.cos(ang), np.sin(ang)], axis=1)

    def res(r):
        q = base.copy()
        q[:, 2:] += r[:, None] * d
        return residual64(model, m9, q)

    lo, hi = np.zeros(len(base)), np.full(len(base), 1.0)
    for _ in range(12):                                       # the residual along a ray from an inlier grows without bound
        hi = np.where(res(hi) < max_error, 2 * hi, hi)
    ok = res(hi) >= max_error
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        below = res(mid) < max_error
        lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
    r = hi * (1 + rs.uniform(-2e-5, 2e-5, len(base)))
    out = base.copy()
    out[:, 2:] += r[:, None] * d
    out = out[ok].astype(np.float32)
    out.setflags(write=False)
    return m9, out


def contracted_inliers(model, m9, pts, max_error=tv.MAX_ERROR):
    """What inliers_f32 becomes when every `a * b + c` of its expressions is fused: the product enters the sum unrounded and the
    sum is rounded once (emulated in float64, where a product of two float32 is exact).  Left to right as the expressions are
    written: in `a*b + c*d + e` the first product is rounded, the second is fused into the sum."""
    f, d = np.float32, np.float64
    m = np.asarray(m9, np.float32).reshape(9)
    x1, y1, x2, y2 = (pts[:, i].astype(np.float32) for i in range(4))
    t2 = f(f(max_error) * f(max_error))

    def fma(a, b, c):
        return (a.astype(d) * b.astype(d) + c.astype(d)).astype(f)

    def lin(a, x, b, y, c):                                   # a*x + b*y + c
        return fma(b, y, (a * x).astype(f)) + c

    with np.errstate(all="ignore"):
        m_ = [np.full_like(x1, v) for v in m]
        r0, r1, r2 = lin(m_[0], x1, m_[1], y1, m_[2]), lin(m_[3], x1, m_[4], y1, m_[5]), lin(m_[6], x1, m_[7], y1, m_[8])
        if model == "F":
            ft0, ft1 = lin(m_[0], x2, m_[3], y2, m_[6]), lin(m_[1], x2, m_[4], y2, m_[7])
            c = lin(x2, r0, y2, r1, r2)
            den = fma(ft1, ft1, fma(ft0, ft0, fma(r1, r1, r0 * r0)))
            bound = t2 * den
            return (den > 0) & (bound < np.inf) & (c * c <= bound)
        dx, dy = fma(-x2, r2, r0), fma(-y2, r2, r1)
        bound = t2 * (r2 * r2)
        return (r2 != 0) & (bound < np.inf) & (fma(dy, dy, dx * dx) <= bound)
