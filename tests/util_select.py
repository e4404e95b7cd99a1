"""Shared helpers of the selection / preprocessing option tests (numpy only; no GPU, no product import)."""
import numpy as np

from oracle import preprocess_oracle as po

F32 = np.float32

# every squared distance two grid cells can have with |dy|, |dx| <= 8, and one (dy, dx) that attains it
ATTAINABLE_D2 = {}
for _a in range(9):
    for _b in range(_a, 9):
        if _a or _b:
            ATTAINABLE_D2.setdefault(_a * _a + _b * _b, (_a, _b))


def reference_suppresses(d2: int, radius: float) -> bool:
    """The reference's NMS comparison restated (vit_extractor.py:534-537): `torch.sqrt(d2) < nms_radius`, float32."""
    d = np.sqrt(F32(d2))
    return bool(d > 0 and d < F32(radius))


def radii_near_root(d2: int, ulps: int = 3, max_radius: float = np.inf):
    """The float32 radii within `ulps` of sqrt(d2), as Python floats; `max_radius` = 8 keeps those the ABI accepts."""
    r = np.sqrt(F32(d2))
    out = [r]
    lo = hi = r
    for _ in range(ulps):
        lo = np.nextafter(lo, F32(-np.inf), dtype=F32)
        hi = np.nextafter(hi, F32(np.inf), dtype=F32)
        out += [lo, hi]
    return sorted(float(x) for x in out if 0 <= x <= max_radius)


def patch_windows_fit(h: int, w: int, oh: int, ow: int, patch: int = 14) -> np.ndarray:
    """Per patch of an (h, w) -> (oh, ow) resize: does its source window fit the padded-patch kernel's LDS staging
    (`3 (xs1 - xs0 + 1) + 6 <= 96` bytes per row and `ys1 - ys0 + 1 <= 24` rows)?  Bounds from the oracle's coefficients."""
    x0, x1, _, _ = po._coefs(ow, w)
    y0, y1, _, _ = po._coefs(oh, h)
    nx = x1[patch - 1::patch] - x0[0::patch] + 1
    ny = y1[patch - 1::patch] - y0[0::patch] + 1
    return (ny[:, None] <= 24) & (3 * nx[None, :] + 6 <= 96)


def bf16_round(x: np.ndarray) -> np.ndarray:
    """float32 -> nearest bfloat16 (ties to even), returned as float32."""
    u = np.ascontiguousarray(x, F32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(F32).reshape(np.shape(x))


def tokens_from_fmap(fmap: np.ndarray) -> np.ndarray:
    """(C, H, W) -> (H*W, C): the ViT's own layout."""
    C, H, W = fmap.shape
    return np.ascontiguousarray(fmap.reshape(C, H * W).T)
