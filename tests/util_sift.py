"""numpy float32 restatement of the SIFT extractor (csrc/sift.hip, features/sift_extractor.py): the spec the
kernels are tested against.  COLMAP's `SiftExtractionOptions` defaults computed the way VLFeat's `vl_sift` does
[recalled]; parity with COLMAP itself is unpinned.

The pyramid, the DoG and the detection decisions (extremum test, Newton refinement, acceptance) use the same
host-computed taps and the same float32 operation order as the kernels, so they agree bit for bit.  Orientation
and descriptor use numpy's exp / atan2 / sqrt / sin / cos and sum in another order than the GPU; they agree within
the tolerances of tests/test_sift_gpu.py.  Test infrastructure: the package never imports it.
"""
import math

import numpy as np

F = np.float32
UBC_PERM = (0, 7, 6, 5, 4, 3, 2, 1)   # COLMAP's VLFeat -> UBC orientation-bin permutation [recalled]
MIN_OCTAVE_SIZE = 8                   # octaves smaller than this in either dimension are not computed
TWO_PI = F(2 * math.pi)


def gaussian_taps(sigma):
    """Half-width ceil(4 sigma), exp(-x^2 / (2 sigma^2)) normalised in float64, then float32."""
    r = max(int(math.ceil(4.0 * sigma)), 1)
    x = np.arange(-r, r + 1, dtype=np.float64)
    k = np.exp(-x * x / (2.0 * sigma * sigma))
    return (k / k.sum()).astype(np.float32)


def level_sigmas(S, first_octave, sigman=0.5):
    """(base smoothing, [incremental smoothing of levels s = 0 .. S+1]); base is None when no smoothing is needed."""
    sigma0 = 1.6 * 2 ** (1 / S)
    s_min = -1
    sa = sigma0 * 2.0 ** (s_min / S)
    sb = sigman * 2.0 ** (-first_octave)
    base = math.sqrt(sa * sa - sb * sb) if sa > sb else None
    d0 = sigma0 * math.sqrt(1.0 - 2.0 ** (-2.0 / S))
    return base, [d0 * 2.0 ** (s / S) for s in range(s_min + 1, S + 2)]


def resized_dims(w, h, max_image_size):
    if max(w, h) <= max_image_size:
        return w, h
    scale = max_image_size / max(w, h)
    return int(w * scale), int(h * scale)


def grey(bgr, max_image_size=3200, size=None):
    """uint8 BGR (h, w, 3) -> float32 grey in [0, 1] at the working size (bilinear, half-pixel centres, when larger
    than max_image_size), or at size = (w, h) when given (as vc_sift_grey's out_w, out_h)."""
    b, g, r = (bgr[..., c].astype(F) for c in range(3))
    g8 = np.floor(F(0.2126) * r + F(0.7152) * g + F(0.0722) * b + F(0.5))
    h, w = g8.shape
    nw, nh = size if size is not None else resized_dims(w, h, max_image_size)
    if (nw, nh) != (w, h):
        def coef(n_out, n_in):
            f = ((np.arange(n_out, dtype=np.float64) + 0.5) * (n_in / n_out) - 0.5).astype(F)
            f = np.clip(f, F(0), F(n_in - 1))
            i0 = np.floor(f).astype(np.int64)
            return i0, np.minimum(i0 + 1, n_in - 1), f - i0.astype(F)
        x0, x1, ax = coef(nw, w)
        y0, y1, ay = coef(nh, h)
        top = g8[y0][:, x0] * (F(1) - ax) + g8[y0][:, x1] * ax
        bot = g8[y1][:, x0] * (F(1) - ax) + g8[y1][:, x1] * ax
        g8 = top * (F(1) - ay)[:, None] + bot * ay[:, None]
    return g8 / F(255)


def upsample(img):
    """VLFeat's 2x linear upsampling: dst[2x] = src[x], dst[2x+1] = (src[x] + src[x+1]) / 2, last sample replicated;
    rows first, then columns."""
    def rows(a):
        h, w = a.shape
        out = np.empty((h, 2 * w), F)
        out[:, 0::2] = a
        out[:, 1:2 * w - 1:2] = F(0.5) * (a[:, :-1] + a[:, 1:])
        out[:, 2 * w - 1] = a[:, w - 1]
        return out
    return rows(rows(img).T).T.copy()


def blur(img, taps):
    """Separable convolution, edge replicate, rows then columns; acc = acc + t[k] * x[i + k - r] for k = 0 .. 2r."""
    r = (len(taps) - 1) // 2
    h, w = img.shape
    pad = np.pad(img, ((0, 0), (r, r)), mode="edge")
    acc = np.zeros((h, w), F)
    for k in range(2 * r + 1):
        acc = acc + taps[k] * pad[:, k:k + w]
    pad = np.pad(acc, ((r, r), (0, 0)), mode="edge")
    out = np.zeros((h, w), F)
    for k in range(2 * r + 1):
        out = out + taps[k] * pad[k:k + h, :]
    return out


def pyramid(base, S=3, first_octave=-1, num_octaves=4):
    """Working grey image -> [(o, levels (S+3, h, w), dog (S+2, h, w))] for the octaves large enough to compute."""
    img = upsample(base) if first_octave == -1 else base
    if first_octave not in (-1, 0):
        raise ValueError("first_octave must be -1 or 0")
    sb, inc = level_sigmas(S, first_octave)
    out = []
    cur = blur(img, gaussian_taps(sb)) if sb is not None else img
    for o in range(first_octave, first_octave + num_octaves):
        h, w = cur.shape
        if min(h, w) < MIN_OCTAVE_SIZE:
            break
        levels = [cur]
        for sd in inc:
            levels.append(blur(levels[-1], gaussian_taps(sd)))
        levels = np.stack(levels)
        out.append((o, levels, levels[1:] - levels[:-1]))
        cur = levels[S][0::2, 0::2][: h // 2, : w // 2].copy()
    return out


def _extrema(dog, S, prefilter):
    """Strict 26-neighbour extrema at DoG levels 1 .. S (s = 0 .. S-1), 1-pixel border excluded -> (j, y, x) in raster
    order."""
    L, h, w = dog.shape
    found = []
    for j in range(1, S + 1):
        c = dog[j, 1:h - 1, 1:w - 1]
        is_max = c >= prefilter
        is_min = c <= -prefilter
        for dj in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if dj == dy == dx == 0:
                        continue
                    nb = dog[j + dj, 1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx]
                    is_max &= c > nb
                    is_min &= c < nb
        ys, xs = np.nonzero(is_max | is_min)
        found.append(np.stack([np.full(len(ys), j), ys + 1, xs + 1], 1))
    return np.concatenate(found) if found else np.zeros((0, 3), np.int64)


def _solve3(A, b):
    """VLFeat's 3x3 Gaussian elimination with partial pivoting, vectorised over rows, float32."""
    n = len(b)
    A, b = A.copy(), b.copy()
    alive = np.ones(n, bool)
    for j in range(3):
        cand = np.abs(A[:, j:, j])
        piv = j + np.argmax(cand, axis=1)
        maxa = A[np.arange(n), piv, j]
        sing = alive & (np.abs(maxa) < F(1e-10))
        b[sing] = 0
        alive &= ~sing
        idx = np.nonzero(alive)[0]
        if len(idx) == 0:
            break
        pi, ma = piv[idx], maxa[idx]
        rj, ri = A[idx, j, :].copy(), A[idx, pi, :].copy()
        A[idx, pi, :] = rj
        A[idx, j, :] = ri
        A[idx, j, j:] = A[idx, j, j:] / ma[:, None]
        bj, bi = b[idx, j].copy(), b[idx, pi].copy()
        b[idx, pi] = bj
        b[idx, j] = bi / ma
        for ii in range(j + 1, 3):
            x = A[idx, ii, j].copy()
            A[idx, ii, j:] = A[idx, ii, j:] - x[:, None] * A[idx, j, j:]
            b[idx, ii] = b[idx, ii] - x * b[idx, j]
    for i in (2, 1):
        x = b[:, i].copy()
        for ii in range(i - 1, -1, -1):
            b[:, ii] = b[:, ii] - x * A[:, ii, i]
    return b


def prefilter_of(peak_threshold):
    return F(0.8 * float(F(peak_threshold)))


def edge_limit_of(edge_threshold):
    r = float(F(edge_threshold))
    return F((r + 1.0) * (r + 1.0) / r)


def detect(dog, S, peak_threshold, edge_threshold, refine=True):
    """-> float32 (N, 8): x, y, s (refined, octave units; s in level units), sigma (octave units), j (DoG level),
    y0, x0 (unrefined extremum), 0.  Rows in (j, y0, x0) raster order."""
    ext = _extrema(dog, S, prefilter_of(peak_threshold))
    L, h, w = dog.shape
    sigma0 = F(1.6 * 2 ** (1 / S))
    out = np.zeros((len(ext), 8), F)
    if len(ext) == 0:
        return out
    j0, y0, x0 = ext[:, 0], ext[:, 1], ext[:, 2]
    if not refine:
        out[:, 0], out[:, 1], out[:, 2] = x0, y0, j0 - 1
        out[:, 3] = sigma0 * np.exp2((j0 - 1).astype(F) / F(S))
        out[:, 4], out[:, 5], out[:, 6] = j0, y0, x0
        return out
    x, y = x0.copy(), y0.copy()
    dx = np.zeros_like(x)
    dy = np.zeros_like(x)
    active = np.ones(len(x), bool)
    n = len(x)
    Dx = Dy = Ds = Dxx = Dyy = Dss = Dxy = Dxs = Dys = None
    B = np.zeros((n, 3), F)
    G = np.zeros((n, 3), F)
    H = np.zeros((n, 3, 3), F)
    for _ in range(5):
        a = np.nonzero(active)[0]
        x[a] += dx[a]
        y[a] += dy[a]
        xa, ya, ja = x[a], y[a], j0[a]

        def at(ddx, ddy, dds):
            return dog[ja + dds, ya + ddy, xa + ddx]
        c = at(0, 0, 0)
        gx = F(0.5) * (at(1, 0, 0) - at(-1, 0, 0))
        gy = F(0.5) * (at(0, 1, 0) - at(0, -1, 0))
        gs = F(0.5) * (at(0, 0, 1) - at(0, 0, -1))
        hxx = at(1, 0, 0) + at(-1, 0, 0) - F(2) * c
        hyy = at(0, 1, 0) + at(0, -1, 0) - F(2) * c
        hss = at(0, 0, 1) + at(0, 0, -1) - F(2) * c
        hxy = F(0.25) * (at(1, 1, 0) + at(-1, -1, 0) - at(-1, 1, 0) - at(1, -1, 0))
        hxs = F(0.25) * (at(1, 0, 1) + at(-1, 0, -1) - at(-1, 0, 1) - at(1, 0, -1))
        hys = F(0.25) * (at(0, 1, 1) + at(0, -1, -1) - at(0, -1, 1) - at(0, 1, -1))
        Hm = np.stack([np.stack([hxx, hxy, hxs], 1), np.stack([hxy, hyy, hys], 1), np.stack([hxs, hys, hss], 1)], 1)
        b = _solve3(Hm, np.stack([-gx, -gy, -gs], 1))
        H[a], B[a], G[a] = Hm, b, np.stack([gx, gy, gs], 1)
        ndx = np.where((b[:, 0] > F(0.6)) & (xa < w - 2), 1, 0) + np.where((b[:, 0] < F(-0.6)) & (xa > 1), -1, 0)
        ndy = np.where((b[:, 1] > F(0.6)) & (ya < h - 2), 1, 0) + np.where((b[:, 1] < F(-0.6)) & (ya > 1), -1, 0)
        dx[a], dy[a] = ndx, ndy
        active[a] = (ndx != 0) | (ndy != 0)
        if not active.any():
            break
    c = dog[j0, y, x]
    val = c + F(0.5) * (G[:, 0] * B[:, 0] + G[:, 1] * B[:, 1] + G[:, 2] * B[:, 2])
    hxx, hyy, hxy = H[:, 0, 0], H[:, 1, 1], H[:, 0, 1]
    tr = hxx + hyy
    det = hxx * hyy - hxy * hxy
    with np.errstate(divide="ignore", invalid="ignore"):
        score = tr * tr / det
    xn = x.astype(F) + B[:, 0]
    yn = y.astype(F) + B[:, 1]
    sn = (j0 - 1).astype(F) + B[:, 2]
    good = ((np.abs(val) >= F(peak_threshold)) & (det > 0) & (score < edge_limit_of(edge_threshold))
            & (np.abs(B) < F(1.5)).all(1) & (xn >= 0) & (xn <= F(w - 1)) & (yn >= 0) & (yn <= F(h - 1))
            & (sn >= F(-1)) & (sn <= F(S + 1)))
    out[:, 0], out[:, 1], out[:, 2] = xn, yn, sn
    out[:, 3] = sigma0 * np.exp2(sn / F(S))
    out[:, 4], out[:, 5], out[:, 6] = j0, y0, x0
    return out[good]


def gradient(level):
    """Central differences x 0.5 (edge replicate) -> (magnitude, angle in [0, 2 pi))."""
    p = np.pad(level, 1, mode="edge")
    gx = F(0.5) * (p[1:-1, 2:] - p[1:-1, :-2])
    gy = F(0.5) * (p[2:, 1:-1] - p[:-2, 1:-1])
    mod = np.sqrt(gx * gx + gy * gy)
    ang = np.arctan2(gy, gx)
    ang = np.where(ang < 0, ang + TWO_PI, ang).astype(F)
    return mod, np.where(ang >= TWO_PI, F(0), ang).astype(F)


def orientations(mod, ang, kp, max_peaks=4):
    """VLFeat's 36-bin orientation histogram -> up to max_peaks (VLFeat: 4) angles, in bin order."""
    h, w = mod.shape
    xk, yk, sigma = F(kp[0]), F(kp[1]), F(kp[3])
    xi, yi = int(np.floor(xk + F(0.5))), int(np.floor(yk + F(0.5)))
    sw = F(1.5) * sigma
    W = max(int(np.floor(F(3) * sw)), 1)
    y_lo, y_hi = max(-W, -yi), min(W, h - 1 - yi)
    x_lo, x_hi = max(-W, -xi), min(W, w - 1 - xi)
    ys, xs = np.mgrid[y_lo:y_hi + 1, x_lo:x_hi + 1]
    ddx = (xi + xs).astype(F) - xk
    ddy = (yi + ys).astype(F) - yk
    r2 = ddx * ddx + ddy * ddy
    m = r2 < F(W * W + 0.6)
    wgt = np.exp(-r2 / (F(2) * sw * sw))
    md = mod[yi + ys, xi + xs] * wgt
    fbin = F(36) * ang[yi + ys, xi + xs] / TWO_PI
    b = np.floor(fbin - F(0.5)).astype(np.int64)
    rb = fbin - b.astype(F) - F(0.5)
    hist = np.bincount(((b + 36) % 36)[m], ((F(1) - rb) * md)[m], 36)
    hist += np.bincount(((b + 1) % 36)[m], (rb * md)[m], 36)
    hist = hist.astype(F)
    for _ in range(6):
        hist = (np.roll(hist, 1) + hist + np.roll(hist, -1)) / F(3)
    maxh = hist.max()
    angles = []
    for i in range(36):
        h0, hm, hp = hist[i], hist[(i - 1) % 36], hist[(i + 1) % 36]
        if h0 > F(0.8) * maxh and h0 > hm and h0 > hp:
            di = F(-0.5) * (hp - hm) / (hp + hm - F(2) * h0)
            angles.append(F(TWO_PI * (F(i) + di + F(0.5)) / F(36)))
            if len(angles) == max_peaks:
                break
    return angles


def descriptor(mod, ang, kp, angle0, normalization="L1_ROOT"):
    """VLFeat's 4x4x8 descriptor (magnification 3, window 2 bins, trilinear), L2 / clamp 0.2 / L2, optional L1_ROOT,
    UBC bin order -> float32 (128,) before quantisation."""
    h, w = mod.shape
    xk, yk, sigma = F(kp[0]), F(kp[1]), F(kp[3])
    xi, yi = int(np.floor(xk + F(0.5))), int(np.floor(yk + F(0.5)))
    sbp = F(3) * sigma
    W = int(np.floor(F(math.sqrt(2.0)) * sbp * F(2.5) + F(0.5)))
    ct0, st0 = F(np.cos(F(angle0))), F(np.sin(F(angle0)))
    y_lo, y_hi = max(-W, 1 - yi), min(W, h - yi - 2)
    x_lo, x_hi = max(-W, 1 - xi), min(W, w - xi - 2)
    hist = np.zeros(128, np.float64)
    if y_lo <= y_hi and x_lo <= x_hi:
        ys, xs = np.mgrid[y_lo:y_hi + 1, x_lo:x_hi + 1]
        md = mod[yi + ys, xi + xs]
        th = ang[yi + ys, xi + xs] - F(angle0)
        th = np.where(th < 0, th + TWO_PI, th).astype(F)
        th = np.where(th >= TWO_PI, th - TWO_PI, th).astype(F)
        dx = (xi + xs).astype(F) - xk
        dy = (yi + ys).astype(F) - yk
        nx = (ct0 * dx + st0 * dy) / sbp
        ny = (-st0 * dx + ct0 * dy) / sbp
        nt = F(8) * th / TWO_PI
        win = np.exp(-(nx * nx + ny * ny) / F(8))
        bx = np.floor(nx - F(0.5)).astype(np.int64)
        by = np.floor(ny - F(0.5)).astype(np.int64)
        bt = np.floor(nt).astype(np.int64)
        rx = nx - (bx.astype(F) + F(0.5))
        ry = ny - (by.astype(F) + F(0.5))
        rt = nt - bt.astype(F)
        wm = win * md
        for ix in (0, 1):
            for iy in (0, 1):
                for it in (0, 1):
                    cx, cy = bx + ix, by + iy
                    ok = (cx >= -2) & (cx < 2) & (cy >= -2) & (cy < 2)
                    wt = wm * np.abs(F(1 - ix) - rx) * np.abs(F(1 - iy) - ry) * np.abs(F(1 - it) - rt)
                    idx = (cy + 2) * 32 + (cx + 2) * 8 + (bt + it) % 8
                    hist += np.bincount(idx[ok], wt[ok].astype(np.float64), 128)
    v = hist.astype(F)
    v = v / (np.sqrt((v * v).sum(dtype=F)) + F(np.finfo(F).eps))
    v = np.minimum(v, F(0.2))
    v = v / (np.sqrt((v * v).sum(dtype=F)) + F(np.finfo(F).eps))
    if normalization == "L1_ROOT":
        v = np.sqrt(v / max(v.sum(dtype=F), F(np.finfo(F).tiny)))
    out = np.empty(128, F)
    for c in range(16):
        for k in range(8):
            out[8 * c + UBC_PERM[k]] = v[8 * c + k]
    return out


def quantize(v):
    """COLMAP's FeatureDescriptorsToUnsignedByte: min(255, round(512 v)), halves rounded up (v >= 0)."""
    return np.minimum(F(255), np.floor(F(512) * np.asarray(v, F) + F(0.5))).astype(np.uint8)


def affine_rows(x, y, sigma, theta):
    """COLMAP's 6-column keypoint: x + 0.5, y + 0.5, s cos, -s sin, s sin, s cos."""
    c, s = np.cos(theta).astype(F), np.sin(theta).astype(F)
    return np.stack([x + F(0.5), y + F(0.5), sigma * c, -sigma * s, sigma * s, sigma * c], 1).astype(F)


def select_rows(octave_rows, max_num_features):
    """Keep whole octaves from the coarsest down while the row count fits; the octave that overflows is truncated in its
    own order.  octave_rows: per-octave row counts, finest first -> per-octave kept counts."""
    keep = [0] * len(octave_rows)
    left = max_num_features
    for i in range(len(octave_rows) - 1, -1, -1):
        keep[i] = min(octave_rows[i], left)
        left -= keep[i]
    return keep


def extract_grey(g, opts, scale=(1.0, 1.0), return_stages=False):
    """Working grey image (float32, [0, 1]) -> (rows (N, 6) float32, descriptors (N, 128) uint8)."""
    S = opts.octave_resolution
    per_oct = []
    stages = []
    for o, levels, dog in pyramid(g, S, opts.first_octave, opts.num_octaves):
        kps = detect(dog, S, opts.peak_threshold, opts.edge_threshold)
        grads = {}
        rows, descs = [], []
        for kp in kps:
            j = int(kp[4])
            if j not in grads:
                grads[j] = gradient(levels[j])
            mod, ang = grads[j]
            angles = [F(0)] if opts.upright else orientations(mod, ang, kp)[: opts.max_num_orientations]
            for a in angles:
                descs.append(quantize(descriptor(mod, ang, kp, a, opts.normalization)))
                rows.append((kp[0], kp[1], kp[3], a))
        k = 2.0 ** o
        r = np.array(rows, F).reshape(-1, 4)
        aff = affine_rows(r[:, 0] * F(k), r[:, 1] * F(k), r[:, 2] * F(k), r[:, 3])
        aff[:, [0, 2, 3]] *= F(scale[0])
        aff[:, [1, 4, 5]] *= F(scale[1])
        per_oct.append((aff, np.array(descs, np.uint8).reshape(-1, 128)))
        stages.append(dict(o=o, levels=levels, dog=dog, kps=kps))
    keep = select_rows([len(a) for a, _ in per_oct], opts.max_num_features)
    rows = np.concatenate([a[:k] for (a, _), k in zip(per_oct, keep)]) if per_oct else np.zeros((0, 6), F)
    desc = np.concatenate([d[:k] for (_, d), k in zip(per_oct, keep)]) if per_oct else np.zeros((0, 128), np.uint8)
    return (rows, desc, stages) if return_stages else (rows, desc)


def extract(bgr, opts, return_stages=False):
    """uint8 BGR image -> (rows (N, 6), descriptors (N, 128) uint8) in original-image pixels."""
    h, w = bgr.shape[:2]
    g = grey(bgr, opts.max_image_size)
    sx, sy = w / g.shape[1], h / g.shape[0]
    return extract_grey(g, opts, (sx, sy), return_stages)
