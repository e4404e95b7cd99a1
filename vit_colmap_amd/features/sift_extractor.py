"""SIFT extractor with COLMAP's default extraction options, computed as VLFeat's `vl_sift` does, on the HIP kernels of
csrc/sift.hip — the baseline half of the reference's ViT-vs-SIFT comparison (reference
vit_colmap/features/colmap_sift_extractor.py, a call into pycolmap.extract_features).

What runs where
  host     file listing, image decode, SQLite writes; tap tables; per-octave row counts (one read-back per octave)
  HIP      grey conversion, resize and 2x upsampling; Gaussian levels; DoG; extremum test, Newton refinement and
           acceptance; orientation histograms; descriptors with normalisation and quantisation (csrc/sift.hip)
  PyTorch  device buffers and the copy of the kept rows into the padded output

Specification: tests/util_sift.py.  Parity with COLMAP's own output is unpinned.
"""
import math
from dataclasses import dataclass
from pathlib import Path
from typing import Optional

import numpy as np
import torch

from .. import _lib
from .base_extractor import BaseExtractor, extract_to_database, host_rows

SIGMA0_BASE = 1.6
SIGMA_NOMINAL = 0.5
MIN_OCTAVE_SIZE = 8          # octaves smaller than this in either dimension are not computed
MAX_TAP_RADIUS = 64          # VC_SIFT_MAX_RADIUS
NORMALIZATIONS = {"L2": 0, "L1_ROOT": 1}
LEVEL_BYTES_BUDGET = 2 << 30  # device bytes of pyramid buffers per launch group


@dataclass
class SiftOptions:
    """COLMAP's SiftExtractionOptions (names and defaults [recalled]); the options that are not built are refused."""
    max_image_size: int = 3200
    max_num_features: int = 8192
    first_octave: int = -1
    num_octaves: int = 4
    octave_resolution: int = 3
    peak_threshold: float = 0.02 / 3
    edge_threshold: float = 10.0
    max_num_orientations: int = 2
    upright: bool = False
    normalization: str = "L1_ROOT"
    estimate_affine_shape: bool = False
    domain_size_pooling: bool = False
    darkness_adaptivity: bool = False

    def validate(self):
        for name in ("estimate_affine_shape", "domain_size_pooling", "darkness_adaptivity"):
            if getattr(self, name):
                raise ValueError(f"SiftOptions.{name} is not implemented")
        if self.normalization not in NORMALIZATIONS:
            raise ValueError(f"normalization must be one of {sorted(NORMALIZATIONS)}, got {self.normalization!r}")
        if self.first_octave not in (-1, 0):
            raise ValueError(f"first_octave must be -1 or 0, got {self.first_octave}")
        if not 1 <= self.octave_resolution <= 8:
            raise ValueError(f"octave_resolution must be in 1 .. 8, got {self.octave_resolution}")
        if self.num_octaves < 1 or self.max_image_size < 1 or self.max_num_features < 1:
            raise ValueError("num_octaves, max_image_size and max_num_features must be positive")
        if not 1 <= self.max_num_orientations <= 4:
            raise ValueError(f"max_num_orientations must be in 1 .. 4, got {self.max_num_orientations}")
        if not (self.peak_threshold >= 0 and self.edge_threshold > 0):
            raise ValueError("peak_threshold must be >= 0 and edge_threshold > 0")
        return self


def gaussian_taps(sigma):
    """Half-width ceil(4 sigma), exp(-x^2 / (2 sigma^2)) normalised in float64, passed to the kernels as float32."""
    r = max(int(math.ceil(4.0 * sigma)), 1)
    x = np.arange(-r, r + 1, dtype=np.float64)
    k = np.exp(-x * x / (2.0 * sigma * sigma))
    return (k / k.sum()).astype(np.float32)


def level_sigmas(S, first_octave):
    """(base smoothing or None, incremental smoothing of levels s = 0 .. S+1) of VLFeat's scale space."""
    sigma0 = SIGMA0_BASE * 2.0 ** (1.0 / S)
    sa = sigma0 * 2.0 ** (-1.0 / S)
    sb = SIGMA_NOMINAL * 2.0 ** (-first_octave)
    base = math.sqrt(sa * sa - sb * sb) if sa > sb else None
    d0 = sigma0 * math.sqrt(1.0 - 2.0 ** (-2.0 / S))
    return base, [d0 * 2.0 ** (s / S) for s in range(0, S + 2)]


def working_size(w, h, max_image_size):
    """COLMAP's downscale rule: scale = max_image_size / max(w, h), sizes truncated."""
    if max(w, h) <= max_image_size:
        return w, h
    scale = max_image_size / max(w, h)
    return int(w * scale), int(h * scale)


def octave_sizes(w, h, opts):
    """[(o, h_o, w_o)] of the octaves that are computed for a working image of w x h."""
    hh, ww = (2 * h, 2 * w) if opts.first_octave == -1 else (h, w)
    out = []
    for o in range(opts.first_octave, opts.first_octave + opts.num_octaves):
        if min(hh, ww) < MIN_OCTAVE_SIZE:
            break
        out.append((o, hh, ww))
        hh, ww = hh // 2, ww // 2
    return out


def camera_params_for(camera_model: str, width: int, height: int) -> list:
    """COLMAP ImageReader defaults [recalled]: focal length 1.2 * max(w, h), principal point at the centre."""
    f, cx, cy = 1.2 * max(width, height), width / 2.0, height / 2.0
    if camera_model == "SIMPLE_PINHOLE":
        return [f, cx, cy]
    if camera_model == "PINHOLE":
        return [f, f, cx, cy]
    if camera_model == "SIMPLE_RADIAL":
        return [f, cx, cy, 0.0]
    if camera_model == "RADIAL":
        return [f, cx, cy, 0.0, 0.0]
    if camera_model == "OPENCV":
        return [f, f, cx, cy, 0.0, 0.0, 0.0, 0.0]
    raise ValueError(f"Unsupported camera model: {camera_model}")


# ---- thin wrappers of the C ABI (device tensors in, device tensors out) ---------------------------------------------
def _taps_arg(sigma):
    t = gaussian_taps(sigma)
    r = (len(t) - 1) // 2
    if r > MAX_TAP_RADIUS:
        raise _lib.HipLibraryError(f"Gaussian of sigma {sigma:.3f} needs {r} taps per side (> {MAX_TAP_RADIUS})")
    return np.ascontiguousarray(t), r


def grey(images_bgr, out_h, out_w, upsample):
    lib = _lib.load()
    B, h, w, _ = images_bgr.shape
    f = 2 if upsample else 1
    out = torch.empty((B, f * out_h, f * out_w), dtype=torch.float32, device=images_bgr.device)
    _lib.check(lib.vc_sift_grey(_lib.ptr(images_bgr), B, h, w, out_h, out_w, int(upsample), _lib.ptr(out),
                                _lib.stream_ptr()), "vc_sift_grey")
    return out


def blur(src, tmp, dst, sigma):
    """src, tmp, dst: (B, h, w) float32 views; dst = G_sigma * src, rows then columns."""
    lib = _lib.load()
    B, h, w = src.shape
    taps, r = _taps_arg(sigma)
    _lib.check(lib.vc_sift_blur(_lib.ptr(src), _lib.ptr(tmp), _lib.ptr(dst), B, h, w,
                                taps.ctypes.data_as(_lib._f32p), r, _lib.stream_ptr()), "vc_sift_blur")


class _Octave:
    """Device buffers of one octave of a batch: levels (S+3, B, h, w), DoG (S+2, B, h, w), one scratch image."""

    def __init__(self, B, h, w, S, device):
        self.levels = torch.empty((S + 3, B, h, w), dtype=torch.float32, device=device)
        self.dog = torch.empty((S + 2, B, h, w), dtype=torch.float32, device=device)
        self.tmp = torch.empty((B, h, w), dtype=torch.float32, device=device)


def _detect(oc, S, opts, cap, refine=True):
    lib = _lib.load()
    L, B, h, w = oc.dog.shape
    dev = oc.dog.device
    while True:
        rows_ws = torch.empty((B, S, h), dtype=torch.int32, device=dev)
        kp = torch.empty((B, cap, 8), dtype=torch.float32, device=dev)
        count = torch.empty((B,), dtype=torch.int32, device=dev)
        _lib.check(lib.vc_sift_detect(_lib.ptr(oc.dog), B, h, w, L, float(opts.peak_threshold),
                                      float(opts.edge_threshold), int(refine), _lib.ptr(rows_ws), cap, _lib.ptr(kp),
                                      _lib.ptr(count), _lib.stream_ptr()), "vc_sift_detect")
        n = count.cpu()
        if int(n.max()) <= cap:
            return kp, count, n
        cap = int(n.max())


def pyramid_octaves(images_bgr, opts):
    """Generator over the octaves of a batch: (o, _Octave) after the levels and the DoG are built.  The buffers of one
    octave are reused by nothing else while it is current."""
    B, h, w, _ = images_bgr.shape
    S = opts.octave_resolution
    ww, wh = working_size(w, h, opts.max_image_size)
    sizes = octave_sizes(ww, wh, opts)
    if not sizes:
        return
    base_sigma, inc = level_sigmas(S, opts.first_octave)
    dev = images_bgr.device
    img = grey(images_bgr, wh, ww, opts.first_octave == -1)
    lib = _lib.load()
    for i, (o, hh, w_o) in enumerate(sizes):
        oc = _Octave(B, hh, w_o, S, dev)
        if i == 0:
            if base_sigma is None:
                oc.levels[0].copy_(img)
            else:
                blur(img, oc.tmp, oc.levels[0], base_sigma)
            del img
        else:
            _lib.check(lib.vc_sift_downsample(_lib.ptr(prev.levels[S]), B, prev.levels.shape[2], prev.levels.shape[3],
                                              _lib.ptr(oc.levels[0]), _lib.stream_ptr()), "vc_sift_downsample")
        for s, sd in enumerate(inc):
            blur(oc.levels[s], oc.tmp, oc.levels[s + 1], sd)
        _lib.check(lib.vc_sift_dog(_lib.ptr(oc.levels), S + 3, B, hh, w_o, _lib.ptr(oc.dog), _lib.stream_ptr()),
                   "vc_sift_dog")
        yield o, oc
        prev = oc


def extract_device(images_bgr: torch.Tensor, opts: Optional[SiftOptions] = None):
    """uint8 BGR (B, h, w, 3) on the GPU -> dict(keypoints (B, max_num_features, 6) float32, descriptors
    (B, max_num_features, 128) uint8, count (B,) int32), rows past count zero.  Keypoints in original-image pixels."""
    opts = (opts or SiftOptions()).validate()
    if not images_bgr.is_cuda:
        raise _lib.HipLibraryError("images must live on the GPU (the SIFT path is HIP-only, no CPU fallback)")
    assert images_bgr.dtype == torch.uint8 and images_bgr.dim() == 4 and images_bgr.shape[3] == 3
    images_bgr = images_bgr.contiguous()
    lib = _lib.load()
    B, h, w, _ = images_bgr.shape
    S = opts.octave_resolution
    dev = images_bgr.device
    ww, wh = working_size(w, h, opts.max_image_size)
    sx, sy = w / ww, h / wh
    n_ori = 1 if opts.upright else opts.max_num_orientations
    per_octave = []   # (rows (B, rcap, 6), desc (B, rcap, 128), row counts host (B,))
    for o, oc in pyramid_octaves(images_bgr, opts):
        hh, w_o = oc.levels.shape[2:]
        kp, count, n = _detect(oc, S, opts, cap=max(1024, hh * w_o // 64))
        m = max(int(n.max()), 1)
        if m < kp.shape[1]:                  # orientation / descriptor grids are sized by the keypoints found
            kp = kp[:, :m].contiguous()
        cap = kp.shape[1]
        angles = torch.empty((B, cap, 4), dtype=torch.float32, device=dev)
        n_angles = torch.empty((B, cap), dtype=torch.int32, device=dev)
        _lib.check(lib.vc_sift_orient(_lib.ptr(oc.levels), S + 3, B, hh, w_o, _lib.ptr(kp), _lib.ptr(count), cap, n_ori,
                                      int(opts.upright), _lib.ptr(angles), _lib.ptr(n_angles), _lib.stream_ptr()),
                   "vc_sift_orient")
        rcap = cap * n_ori
        rows = torch.empty((B, rcap, 6), dtype=torch.float32, device=dev)
        desc = torch.empty((B, rcap, 128), dtype=torch.uint8, device=dev)
        rcount = torch.empty((B,), dtype=torch.int32, device=dev)
        offs = torch.empty((B, cap), dtype=torch.int32, device=dev)
        _lib.check(lib.vc_sift_describe(_lib.ptr(oc.levels), S + 3, B, hh, w_o, _lib.ptr(kp), _lib.ptr(count), cap,
                                        _lib.ptr(angles), _lib.ptr(n_angles), n_ori, NORMALIZATIONS[opts.normalization],
                                        float(2.0 ** o), float(sx), float(sy), _lib.ptr(offs), rcap, _lib.ptr(rows),
                                        _lib.ptr(desc), _lib.ptr(rcount), _lib.stream_ptr()), "vc_sift_describe")
        per_octave.append(((rows, desc), rcount))
    rc = torch.stack([r for _, r in per_octave]).cpu().numpy() if per_octave else None      # (octaves, B)
    (out_kp, out_desc), count = _gather_octaves([t for t, _ in per_octave], rc, opts.max_num_features, B, dev,
                                                ((6, torch.float32), (128, torch.uint8)))
    return dict(keypoints=out_kp, descriptors=out_desc, count=count)


def _gather_octaves(per_octave, row_counts, K, B, dev, columns):
    """Per-octave padded tensors (finest octave first; per_octave[i][j] is (B, cap_i, columns[j][0])) and their host row
    counts (octaves, B) -> one zero-padded (B, K, width) tensor per column and count (B,) int32 on the device, the rows
    of each image chosen by `select_rows`."""
    outs = [torch.zeros((B, K, width), dtype=dtype, device=dev) for width, dtype in columns]
    counts = np.zeros(B, np.int32)
    if per_octave:
        for b in range(B):
            keep = select_rows(row_counts[:, b].tolist(), K)
            at = 0
            for tensors, k in zip(per_octave, keep):
                if k:
                    for out, t in zip(outs, tensors):
                        out[b, at:at + k] = t[b, :k]
                    at += k
            counts[b] = at
    return outs, torch.from_numpy(counts).to(dev)


def detect_device(images_bgr: torch.Tensor, max_num_features: int):
    """SIFT as a detector only: uint8 BGR (B, h, w, 3) on the GPU -> (xy float32 (B, max_num_features, 2) in
    original-image pixels, rows past the count zero; count (B,) int32).  The points are columns 0 and 1 of the rows
    `extract_device(images_bgr, SiftOptions(max_num_features=max_num_features, upright=True))` returns, bit for bit:
    the same pyramid, extremum kernels and `select_rows`, the position (x 2^o + 0.5) scale_x in the three float32
    operations of the descriptor kernel; the orientation and descriptor kernels are not run.

    Known deviation from the reference's `cv2.SIFT_create(nfeatures=N)`: OpenCV keeps the N strongest responses, this
    keeps whole octaves from the coarsest down (COLMAP's rule, the one csrc/sift.hip implements)."""
    opts = SiftOptions(max_num_features=int(max_num_features), upright=True).validate()
    if not images_bgr.is_cuda:
        raise _lib.HipLibraryError("images must live on the GPU (the SIFT path is HIP-only, no CPU fallback)")
    assert images_bgr.dtype == torch.uint8 and images_bgr.dim() == 4 and images_bgr.shape[3] == 3
    images_bgr = images_bgr.contiguous()
    B, h, w, _ = images_bgr.shape
    dev = images_bgr.device
    ww, wh = working_size(w, h, opts.max_image_size)
    scale = torch.tensor([w / ww, h / wh], dtype=torch.float32, device=dev)
    per_octave, row_counts = [], []
    for o, oc in pyramid_octaves(images_bgr, opts):
        hh, w_o = oc.levels.shape[2:]
        kp, _, n = _detect(oc, opts.octave_resolution, opts, cap=max(1024, hh * w_o // 64))
        xy = kp[:, :max(int(n.max()), 1), :2]
        per_octave.append((((xy * float(2.0 ** o)) + 0.5) * scale,))
        row_counts.append(n.numpy())
    (out_xy,), count = _gather_octaves(per_octave, np.stack(row_counts) if row_counts else None, opts.max_num_features, B,
                                       dev, ((2, torch.float32),))
    return out_xy, count


def select_rows(octave_rows, max_num_features):
    """COLMAP's max_num_features rule: keep whole octaves from the coarsest down while the row count fits; the octave
    that overflows is truncated in its own order.  Per-octave row counts (finest first) -> kept counts."""
    keep = [0] * len(octave_rows)
    left = max_num_features
    for i in range(len(octave_rows) - 1, -1, -1):
        keep[i] = min(int(octave_rows[i]), left)
        left -= keep[i]
    return keep


class SiftExtractor(BaseExtractor):
    """COLMAP-default SIFT on the GPU, written into a COLMAP database like the reference's ColmapSiftExtractor: one
    camera per image (CameraMode.AUTO); `camera_params` is ignored, as the reference wrapper ignores it."""
    camera_params_for = staticmethod(camera_params_for)
    camera_per_image = True

    def __init__(self, options: Optional[SiftOptions] = None, device: str | None = None, batch_size: int = 16):
        self.options = (options or SiftOptions()).validate()
        self.batch_size = batch_size
        self.device = torch.device(device) if device is not None else torch.device(
            "cuda" if torch.cuda.is_available() else "cpu")

    def _require_gpu(self):
        if self.device.type != "cuda" or not torch.cuda.is_available():
            raise _lib.HipLibraryError("SiftExtractor needs an MI355X: the SIFT path is HIP-only (no CPU fallback)")

    def _group_size(self, h, w):
        """Images per launch group so that the pyramid buffers of the first octave stay under LEVEL_BYTES_BUDGET."""
        ww, wh = working_size(w, h, self.options.max_image_size)
        f = 4 if self.options.first_octave == -1 else 1
        per_image = (2 * self.options.octave_resolution + 6) * 4 * f * ww * wh
        return max(1, min(self.batch_size, LEVEL_BYTES_BUDGET // max(per_image, 1)))

    @torch.inference_mode()
    def _run_batch(self, images_bgr_np):
        """list of equal-size BGR uint8 arrays -> list of (keypoints (N, 6) float32, descriptors (N, 128) uint8)."""
        self._require_gpu()
        h, w = images_bgr_np[0].shape[:2]
        g = self._group_size(h, w)
        out = []
        for s in range(0, len(images_bgr_np), g):
            batch = torch.from_numpy(np.ascontiguousarray(np.stack(images_bgr_np[s:s + g]))).to(self.device)
            res = extract_device(batch, self.options)
            out.extend(host_rows(res["count"], res["keypoints"], res["descriptors"]))
        return out

    def _run_inference(self, image_bgr: np.ndarray):
        """Single image -> (keypoints (N, 6) float32 in COLMAP's affine form, descriptors (N, 128) uint8)."""
        return self._run_batch([image_bgr])[0]

    def extract(self, image_dir: Path, db_path: Path, camera_model: str,
                camera_params: Optional[list[float]] = None) -> None:
        self._require_gpu()
        print(f"SIFT extraction: {image_dir} into {db_path}")
        extract_to_database(self, image_dir, db_path, camera_model, camera_params)
