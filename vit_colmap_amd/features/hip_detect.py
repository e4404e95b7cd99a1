"""Torch-tensor front end of the classical detectors (vit_colmap_amd/csrc/detect.hip): FAST and GFTT for the hybrid
extractor, batched over same-size images.  Tensors are plumbing for device memory; the arithmetic runs in the C-ABI
library and there is no CPU fallback.  Specification: tests/util_detect.py.
"""
import torch

from .. import _lib

MIN_SIZE = 8                      # VC_DETECT_MIN_SIZE: smaller images have no keypoints and launch nothing
GFTT_MAX_CANDIDATES = 16384       # VC_DETECT_GFTT_MAX_CANDIDATES


def _check_images(images_bgr):
    if not images_bgr.is_cuda:
        raise _lib.HipLibraryError("images must live on the GPU (the detectors are HIP-only, no CPU fallback)")
    assert images_bgr.dtype == torch.uint8 and images_bgr.dim() == 4 and images_bgr.shape[3] == 3, images_bgr.shape
    return images_bgr.contiguous()


def _empty(B, K, dev):
    zeros = torch.zeros((B,), dtype=torch.int32, device=dev)
    return torch.zeros((B, K, 2), dtype=torch.float32, device=dev), zeros, zeros.clone()


def fast(images_bgr: torch.Tensor, max_keypoints: int = 2048, threshold: int = 10):
    """uint8 BGR (B, h, w, 3) -> (xy float32 (B, max_keypoints, 2) in raster order, rows past the count zero; count int32
    (B,); total int32 (B,) = corners before the limit).  FAST-9/16 with non-maximum suppression; the limit keeps the
    largest scores, the earlier raster position among equal ones."""
    images_bgr = _check_images(images_bgr)
    lib = _lib.load()
    B, h, w, _ = images_bgr.shape
    dev = images_bgr.device
    K = int(max_keypoints)
    if min(h, w) < MIN_SIZE:
        return _empty(B, K, dev)
    ws_bytes = lib.vc_detect_fast_workspace_bytes(B, h, w)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
    xy = torch.empty((B, K, 2), dtype=torch.float32, device=dev)
    count = torch.empty((B,), dtype=torch.int32, device=dev)
    total = torch.empty((B,), dtype=torch.int32, device=dev)
    _lib.check(lib.vc_detect_fast(_lib.ptr(images_bgr), B, h, w, int(threshold), K, _lib.ptr(ws), ws_bytes, _lib.ptr(xy),
                                  _lib.ptr(count), _lib.ptr(total), _lib.stream_ptr()), "vc_detect_fast")
    return xy, count, total


def gftt(images_bgr: torch.Tensor, max_corners: int = 2048, quality_level: float = 0.01, min_distance: int = 7,
         block_size: int = 7, cand_cap: int = 4096):
    """uint8 BGR (B, h, w, 3) -> (xy float32 (B, max_corners, 2) in acceptance order, rows past the count zero; count
    int32 (B,); candidates int32 (B,)).  Shi-Tomasi corners with the greedy minimum-distance pass.  `cand_cap` sizes the
    candidate list; the number found is read back (the one read-back of this call) and the call is repeated with more
    room when the list overflowed.  More than GFTT_MAX_CANDIDATES candidates in one image raise."""
    images_bgr = _check_images(images_bgr)
    lib = _lib.load()
    B, h, w, _ = images_bgr.shape
    dev = images_bgr.device
    K = int(max_corners)
    if min(h, w) < MIN_SIZE:
        return _empty(B, K, dev)
    cap = max(1, min(int(cand_cap), GFTT_MAX_CANDIDATES))
    while True:
        ws_bytes = lib.vc_detect_gftt_workspace_bytes(B, h, w, cap)
        ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
        xy = torch.empty((B, K, 2), dtype=torch.float32, device=dev)
        count = torch.empty((B,), dtype=torch.int32, device=dev)
        cand = torch.empty((B,), dtype=torch.int32, device=dev)
        _lib.check(lib.vc_detect_gftt(_lib.ptr(images_bgr), B, h, w, float(quality_level), int(min_distance), int(block_size),
                                      K, cap, _lib.ptr(ws), ws_bytes, _lib.ptr(xy), _lib.ptr(count), _lib.ptr(cand),
                                      _lib.stream_ptr()), "vc_detect_gftt")
        found = int(cand.max().item())
        if found <= cap:
            return xy, count, cand
        if found > GFTT_MAX_CANDIDATES:
            raise _lib.HipLibraryError(f"vc_detect_gftt: {found} corner candidates in one image, the selection kernel ranks "
                                       f"at most {GFTT_MAX_CANDIDATES} (raise quality_level or split the image)")
        cap = min(GFTT_MAX_CANDIDATES, max(found, 2 * cap))
