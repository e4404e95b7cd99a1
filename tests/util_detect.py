"""Specification of the device detectors of csrc/detect.hip (FAST-9/16 and Shi-Tomasi GFTT) in numpy — the role
tests/util_sift.py plays for SIFT.  Both functions restate OpenCV's algorithms from memory
(`cv2.FastFeatureDetector_create(threshold=10, nonmaxSuppression=True)`, `cv2.goodFeaturesToTrack(qualityLevel=0.01,
minDistance=7, blockSize=7)`); parity with OpenCV itself cannot be pinned where there is no cv2.  Where
OpenCV leaves an order open the rule below is this project's own, and says so."""
import numpy as np

from test_host_logic import checkerboard

# radius-3 circle, (dx, dy), in OpenCV's order
CIRCLE = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0),
          (-3, 1), (-2, 2), (-1, 3)]
MIN_SIZE = 8


def grey_u8(bgr):
    """OpenCV's fixed-point BGR2GRAY: (1868 B + 9617 G + 4899 R + 8192) >> 14 [recalled]."""
    b, g, r = (bgr[..., i].astype(np.int32) for i in range(3))
    return ((b * 1868 + g * 9617 + r * 4899 + 8192) >> 14).astype(np.uint8)


# ---- FAST ------------------------------------------------------------------------------------------------------------
def fast_score(grey):
    """S = max over the 16 arcs of 9 contiguous circle pixels of max(min(c - p), min(p - c)), 0 within 3 of the edge."""
    h, w = grey.shape
    s = np.zeros((h, w), np.int32)
    if h < 7 or w < 7:
        return s
    p = grey[3:h - 3, 3:w - 3].astype(np.int32)
    d = np.stack([grey[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx].astype(np.int32) - p for dx, dy in CIRCLE])
    best = np.zeros_like(p)
    for k in range(16):
        arc = d[[(k + i) % 16 for i in range(9)]]
        best = np.maximum(best, np.maximum(arc.min(0), (-arc).min(0)))
    s[3:h - 3, 3:w - 3] = best
    return s


def fast_score_bruteforce(grey, y, x):
    """The definition: the largest t for which 9 contiguous circle pixels are all > p + t or all < p - t, plus one
    (0 if there is no such t >= 0)."""
    p = int(grey[y, x])
    c = [int(grey[y + dy, x + dx]) for dx, dy in CIRCLE]
    best = -1
    for t in range(0, 256):
        ok = any(all(c[(k + i) % 16] > p + t for i in range(9)) or all(c[(k + i) % 16] < p - t for i in range(9))
                 for k in range(16))
        if ok:
            best = t
    return best + 1


def fast_detect(grey, threshold=10, max_keypoints=2048):
    """-> (xy float32 (N, 2) in raster order, total before the limit, scores of the kept).  A corner has S > threshold
    and S strictly above its 8 neighbours.  The limit keeps the largest S; among equal S the EARLIER raster position
    wins.  That tie rule is this project's: the reference orders by `np.argsort` over tied integer responses, which
    numpy leaves undefined."""
    s = fast_score(grey)
    s = np.where(s > threshold, s, 0)
    h, w = s.shape
    pad = np.pad(s, 1)
    nb = np.stack([pad[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy) != (0, 0)]).max(0)
    ys, xs = np.nonzero((s > 0) & (s > nb))
    sc = s[ys, xs]
    total = len(ys)
    if total > max_keypoints:
        order = np.sort(np.lexsort((xs, ys, -sc))[:max_keypoints])
        ys, xs, sc = ys[order], xs[order], sc[order]
    return np.stack([xs, ys], axis=1).astype(np.float32).reshape(-1, 2), total, sc


# ---- GFTT ------------------------------------------------------------------------------------------------------------
def sobel(grey):
    """3x3 Sobel, reflect-101 borders, int32."""
    p = np.pad(grey.astype(np.int32), 1, mode="reflect")
    h, w = grey.shape

    def at(dy, dx):
        return p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]

    gx = (at(-1, 1) + 2 * at(0, 1) + at(1, 1)) - (at(-1, -1) + 2 * at(0, -1) + at(1, -1))
    gy = (at(1, -1) + 2 * at(1, 0) + at(1, 1)) - (at(-1, -1) + 2 * at(-1, 0) + at(-1, 1))
    return gx, gy


def box_sum(a, block_size):
    """Sum over the block_size x block_size window centred on the pixel, the image extended by reflect-101; int32."""
    r = block_size // 2
    p = np.pad(a, r, mode="reflect")
    h, w = a.shape
    out = np.zeros_like(a)
    for dy in range(block_size):
        for dx in range(block_size):
            out += p[dy:dy + h, dx:dx + w]
    return out


def min_eigenvalue(grey, block_size=7):
    """Shi-Tomasi response without OpenCV's 1 / (4 blockSize 255) scale (it cancels against the relative threshold):
    float32, in exactly this order of operations."""
    gx, gy = sobel(grey)
    a, b, c = (box_sum(m, block_size).astype(np.float32) for m in (gx * gx, gx * gy, gy * gy))
    ha, hc = np.float32(0.5) * a, np.float32(0.5) * c
    dm = ha - hc
    return (ha + hc) - np.sqrt(dm * dm + b * b)


def gftt_candidates(grey, quality_level=0.01, block_size=7):
    """-> (ys, xs, lambda) of the candidates in rank order: lambda descending, the LATER raster position first among
    equals (OpenCV's comparator falls back to the higher address [recalled])."""
    lam = min_eigenvalue(grey, block_size)
    h, w = lam.shape
    mx = lam.max()
    if not mx > 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32)
    lam = np.where(lam < np.float32(quality_level) * mx, np.float32(0), lam)
    pad = np.pad(lam, 1, mode="constant", constant_values=-np.inf)
    dil = np.stack([pad[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)]).max(0)
    m = (lam != 0) & (lam == dil)
    m[0] = m[-1] = False
    m[:, 0] = m[:, -1] = False
    ys, xs = np.nonzero(m)
    v = lam[ys, xs]
    order = np.lexsort((-(ys * w + xs), -v))
    return ys[order], xs[order], v[order]


def greedy_plain(ys, xs, min_distance, max_corners):
    """The sequential greedy pass, O(n^2): accepted iff no accepted candidate at squared distance < min_distance^2."""
    acc = []
    for i in range(len(ys)):
        y, x = int(ys[i]), int(xs[i])
        if all((ys[j] - y) ** 2 + (xs[j] - x) ** 2 >= min_distance ** 2 for j in acc):
            acc.append(i)
            if len(acc) == max_corners:
                break
    return acc


def greedy_grid(ys, xs, min_distance, max_corners):
    """The same pass with the accepted points binned in cells of min_distance pixels."""
    acc, cell = [], {}
    for i in range(len(ys)):
        y, x = int(ys[i]), int(xs[i])
        cy, cx = y // min_distance, x // min_distance
        ok = all((py - y) ** 2 + (px - x) ** 2 >= min_distance ** 2
                 for yy in (cy - 1, cy, cy + 1) for xx in (cx - 1, cx, cx + 1) for py, px in cell.get((yy, xx), ()))
        if ok:
            cell.setdefault((cy, cx), []).append((y, x))
            acc.append(i)
            if len(acc) == max_corners:
                break
    return acc


def greedy_rounds(ys, xs, min_distance, max_corners):
    """The parallel form the kernel uses: per round, from the states of the round before, an undecided candidate is
    rejected when an accepted one of higher rank is in range and accepted when no undecided one of higher rank is."""
    n = len(ys)
    state = np.zeros(n, np.int8)        # 0 undecided, 1 accepted, 2 rejected
    pts = np.stack([ys, xs], axis=1).astype(np.int64)
    while (state == 0).any():
        nxt = state.copy()
        for i in np.nonzero(state == 0)[0]:
            d = ((pts[:i] - pts[i]) ** 2).sum(1) < min_distance ** 2
            if (d & (state[:i] == 1)).any():
                nxt[i] = 2
            elif not (d & (state[:i] == 0)).any():
                nxt[i] = 1
        state = nxt
    return list(np.nonzero(state == 1)[0][:max_corners])


def gftt_detect(grey, max_corners=2048, quality_level=0.01, min_distance=7, block_size=7):
    """-> (xy float32 (N, 2) in acceptance order, number of candidates)."""
    ys, xs, _ = gftt_candidates(grey, quality_level, block_size)
    acc = greedy_grid(ys, xs, min_distance, max_corners)
    return np.stack([xs[acc], ys[acc]], axis=1).astype(np.float32).reshape(-1, 2), len(ys)


# ---- inputs ----------------------------------------------------------------------------------------------------------
def noisy_checkerboard(k, w=640, h=480, amp=40):
    """tests/test_e2e_gpu.py `synthetic_image` with the noise amplitude as a parameter (amp = 40 is that helper)."""
    rs = np.random.RandomState(1000 + k)
    img = np.roll(checkerboard(w, h), (7 * k, 5 * k), (1, 0)).astype(np.int16)
    img += rs.randint(-amp, amp + 1, img.shape).astype(np.int16)
    return np.clip(img, 0, 255).astype(np.uint8)


def rectangles(w=640, h=480, seed=5):
    """A few rotated rectangles on a flat ground with +-3 noise: real corners rather than noise."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.full((h, w), 90.0)
    for cx, cy, a, b, ang, val in [(150, 120, 80, 40, 0.3, 200), (420, 160, 60, 60, 0.8, 30), (300, 340, 110, 35, -0.5, 160),
                                   (520, 380, 50, 70, 1.2, 230), (110, 360, 45, 45, 0.1, 10)]:
        u = (xx - cx) * np.cos(ang) + (yy - cy) * np.sin(ang)
        v = -(xx - cx) * np.sin(ang) + (yy - cy) * np.cos(ang)
        img[(np.abs(u) <= a) & (np.abs(v) <= b)] = val
    img = img[..., None] + rs.randint(-3, 4, (h, w, 3))
    return np.clip(img, 0, 255).astype(np.uint8)
