"""Hybrid extractor: keypoints from a classical detector, descriptors from the ViT token grid — MI355X implementation
of the reference's `vit_colmap/features/hybrid_extractor.py` (class `ViTExtractor` there, never selected by the
reference's pipeline).  Same constructor arguments and the same
`_run_inference(image_bgr) -> (keypoints float32 (N, 2), descriptors uint8 (N, D))` contract.

What runs where
  HIP    keypoint DETECTION with `detector_backend="hip"` (the default where cv2 is not importable): SIFT extrema from
         the project's own front end (csrc/sift.hip through `sift_extractor.detect_device`), FAST and GFTT from
         csrc/detect.hip.  The points stay on the device between detection and `vc_describe_at`; a batch of equal-size
         images is one upload, one detection, one ViT forward and one `describe_at` (`_run_batch`).
  HIP    preprocessing, the DINOv2 forward (as ViTExtractor), and `_extract_descriptors_at_keypoints`
         (hybrid_extractor.py:224-294): bilinear sampling of the token grid at the sub-pixel keypoints, optional projection,
         RootSIFT normalisation, uint8 quantiser — csrc/select.hip `vc_describe_at`; no CPU fallback.
  host   detection with `detector_backend="cv2"` (OpenCV's SIFT / FAST / GFTT / ORB as in the reference,
         hybrid_extractor.py:110-180; the default where cv2 imports) or with a `keypoint_fn(image_bgr) -> (N, 2) float32`,
         which wins over both; these run image by image.  ORB has no device implementation.

The device detectors follow tests/util_detect.py and tests/util_sift.py; their parity with OpenCV's is unpinned
(DESIGN.md §4.8).
"""
from pathlib import Path
from typing import Callable, Optional

import numpy as np
import torch

from .. import _lib
from ..utils import image_io
from . import hip_detect, hip_select
from .base_extractor import BaseExtractor, default_camera_params, extract_to_database, host_rows, list_images
from .vit_extractor import PATCH, ViTExtractor

HIP_DETECTORS = ("sift", "fast", "gftt")
HIP_BATCH_SIZE = 16


class HybridViTExtractor(BaseExtractor):
    batch_size = 1                                             # per-image inference, as the reference (host detection)
    detector_backend = None                                    # "hip" | "cv2" | "keypoint_fn", set by __init__
    camera_params_for = staticmethod(default_camera_params)   # one camera, of the first image's size (extract_to_database)
    camera_per_image = False

    def __init__(self, weights_path: Optional[str] = None, model_name: str = "dinov2_vitb14", num_keypoints: int = 2048,
                 descriptor_dim: int = 256, device: Optional[str] = None, detector_type: str = "sift", *,
                 keypoint_fn: Optional[Callable[[np.ndarray], np.ndarray]] = None, precision: str = "bf16",
                 projection=None, seed: int = 0, detector_backend: str = "auto"):
        if detector_type not in ("sift", "fast", "gftt", "orb"):
            raise ValueError(f"Unknown detector type: {detector_type}")          # hybrid_extractor.py:130
        if detector_backend not in ("auto", "hip", "cv2"):
            raise ValueError(f"detector_backend must be 'auto', 'hip' or 'cv2', got {detector_backend!r}")
        self.detector_type = detector_type
        self.num_keypoints = num_keypoints
        self.descriptor_dim = descriptor_dim
        self.keypoint_fn = keypoint_fn
        if keypoint_fn is not None:
            detector_backend = "keypoint_fn"
        elif detector_backend == "auto":
            detector_backend = "cv2" if _cv2_importable() else "hip"
        if detector_backend == "hip" and detector_type not in HIP_DETECTORS:       # before the backbone is built
            raise _lib.HipLibraryError(f"detector_type={detector_type!r} is OpenCV-only and OpenCV is not in use: the "
                                       f"detectors that run on the device are {', '.join(HIP_DETECTORS)}")
        self.detector_backend = detector_backend
        print(f"Initializing Hybrid extractor: {model_name}")
        print(f"Keypoint detector: {detector_type.upper()}")
        # the backbone, its preprocessing and the projection handling are ViTExtractor's
        self._vit = ViTExtractor(weights_path=weights_path, model_name=model_name, num_keypoints=num_keypoints,
                                 descriptor_dim=descriptor_dim, device=device, precision=precision, projection=projection, seed=seed)
        self.device = self._vit.device
        self.patch_size = PATCH
        if detector_backend == "cv2":
            self.detector = self._create_detector()
        elif detector_backend == "hip":
            self.batch_size = HIP_BATCH_SIZE

    @property
    def descriptor_projection(self):
        return self._vit.descriptor_projection

    # ---- detection on the device ------------------------------------------------------------------------------------------
    def detect_device(self, images_bgr: torch.Tensor):
        """uint8 BGR (B, h, w, 3) on the GPU -> (xy float32 (B, num_keypoints, 2) in pixels, count int32 (B,)), on the GPU."""
        if self.detector_type == "sift":
            from .sift_extractor import detect_device  # noqa: PLC0415

            return detect_device(images_bgr, self.num_keypoints)
        if self.detector_type == "fast":                       # hybrid_extractor.py:113-116: threshold 10, with NMS
            return hip_detect.fast(images_bgr, self.num_keypoints, threshold=10)[:2]
        if self.detector_type == "gftt":                       # hybrid_extractor.py:160-166
            return hip_detect.gftt(images_bgr, self.num_keypoints, quality_level=0.01, min_distance=7, block_size=7)[:2]
        raise _lib.HipLibraryError(f"detector_type={self.detector_type!r} has no device implementation "
                                   f"(those that have: {', '.join(HIP_DETECTORS)})")

    # ---- detection: OpenCV on the host, as in the reference ---------------------------------------------------------
    def _create_detector(self):
        try:
            import cv2  # noqa: PLC0415
        except ImportError:
            raise _lib.HipLibraryError("OpenCV is not importable: pass keypoint_fn=<callable image_bgr -> (N, 2) float32> "
                                       "(keypoint detection is host work outside the accelerated path)") from None
        if self.detector_type == "sift":
            return cv2.SIFT_create(nfeatures=self.num_keypoints)
        if self.detector_type == "fast":
            return cv2.FastFeatureDetector_create(threshold=10, nonmaxSuppression=True)
        if self.detector_type == "gftt":
            return cv2.goodFeaturesToTrack
        return cv2.ORB_create(nfeatures=self.num_keypoints)

    def _detect_keypoints(self, image_bgr: np.ndarray) -> np.ndarray:
        if self.keypoint_fn is not None:
            return np.asarray(self.keypoint_fn(image_bgr), np.float32).reshape(-1, 2)
        import cv2  # noqa: PLC0415

        gray = cv2.cvtColor(image_bgr, cv2.COLOR_BGR2GRAY)
        if self.detector_type == "gftt":
            corners = self.detector(gray, maxCorners=self.num_keypoints, qualityLevel=0.01, minDistance=7)
            return np.zeros((0, 2), np.float32) if corners is None else corners.reshape(-1, 2).astype(np.float32)
        kps = self.detector.detect(gray, None)
        kps = sorted(kps, key=lambda k: -k.response)[: self.num_keypoints]
        return np.array([k.pt for k in kps], np.float32).reshape(-1, 2)

    # ---- descriptors at the keypoints: HIP --------------------------------------------------------------------------------
    def _describe_device(self, batch: torch.Tensor, keypoints_xy: torch.Tensor, count: torch.Tensor) -> torch.Tensor:
        """uint8 BGR (B, h, w, 3), keypoints (B, kmax, 2) float32 in pixels, count (B,) int32, all on the GPU -> uint8
        (B, kmax, D), rows past the count zero.  One ViT forward and one `describe_at` for the batch."""
        h, w = batch.shape[1:3]
        h_new, w_new = (h // PATCH) * PATCH, (w // PATCH) * PATCH
        tokens, hp, wp = self._vit._tokens(batch)
        C = tokens.shape[-1]
        proj = None
        if C > self.descriptor_dim:
            if self._vit.descriptor_projection is None:
                # the reference fits the projection on the first image's descriptors (hybrid_extractor.py:296-323); the
                # fit itself is ViTExtractor's (PCA when there are enough samples, seeded random projection otherwise)
                self._vit._ensure_projection(tokens, hp, wp, (w, h), (w_new, h_new))
            proj = self._vit.descriptor_projection
        return hip_select.describe_at(tokens, hp, wp, keypoints_xy, count, (w_new, h_new), (w, h), proj, rootsift=True)

    def _upload(self, images_bgr_np) -> torch.Tensor:
        return torch.from_numpy(np.ascontiguousarray(np.stack(images_bgr_np))).to(self.device)

    @torch.inference_mode()
    def describe_batch(self, images_bgr_np, keypoints_list):
        """Equal-size BGR uint8 arrays + their keypoints (N_i, 2) float32 in pixels -> list of uint8 (N_i, D)."""
        self._vit._require_gpu()
        kmax = max(max((len(k) for k in keypoints_list), default=0), 1)
        kp = np.zeros((len(images_bgr_np), kmax, 2), np.float32)
        cnt = np.zeros(len(images_bgr_np), np.int32)
        for i, k in enumerate(keypoints_list):
            cnt[i] = len(k)
            kp[i, : len(k)] = np.asarray(k, np.float32).reshape(-1, 2)
        u8 = self._describe_device(self._upload(images_bgr_np), torch.from_numpy(kp).to(self.device),
                                   torch.from_numpy(cnt).to(self.device)).cpu().numpy()
        return [u8[i, : cnt[i]].copy() for i in range(len(images_bgr_np))]

    def _run_inference(self, image_bgr: np.ndarray):
        if self.detector_backend == "hip":
            keypoints, descriptors = self._run_batch([image_bgr])[0]
            if len(keypoints) == 0:
                print("Warning: No keypoints detected")
            return keypoints, descriptors
        keypoints = self._detect_keypoints(image_bgr)
        if len(keypoints) == 0:
            print("Warning: No keypoints detected")
            D = min(self.descriptor_dim, self._vit.model.arch.dim)
            return keypoints, np.zeros((0, D), np.uint8)
        return keypoints, self.describe_batch([image_bgr], [keypoints])[0]

    @torch.inference_mode()
    def _run_batch(self, images_bgr_np):
        """list of equal-size BGR uint8 arrays -> list of (keypoints (N, 2) float32, descriptors (N, D) uint8).  With the
        device detectors: one upload, detection, one ViT forward and one `describe_at` per HIP_BATCH_SIZE images (a
        caller such as `run_sharded` may hand over more); the keypoints reach the host only with the results.  With host
        detection: image by image."""
        if self.detector_backend != "hip":
            return [self._run_inference(img) for img in images_bgr_np]
        self._vit._require_gpu()
        out = []
        for s in range(0, len(images_bgr_np), HIP_BATCH_SIZE):
            batch = self._upload(images_bgr_np[s:s + HIP_BATCH_SIZE])
            xy, count = self.detect_device(batch)
            out.extend(host_rows(count, xy, self._describe_device(batch, xy, count)))
        return out

    def set_projection(self, projection):
        self._vit.set_projection(projection)

    def sync_projection(self, image_dir):
        """Multi-GPU runs: rank 0 fits the projection from the first file through this class's own path (`_run_batch`
        of that one image, which is what a single process's first batch fits from: `_ensure_projection` reads the
        first image's tokens only) and broadcasts it, so that every rank projects with the same matrix."""
        from .. import dist as vd  # noqa: PLC0415

        if not vd.is_distributed():
            return
        rank, _ = vd.rank_world()
        if rank == 0 and self.descriptor_projection is None:
            files = list_images(Path(image_dir))
            first = image_io.imread(files[0]) if files else None
            if first is not None:
                self._run_batch([first])
        have = vd.broadcast_array(np.array([self.descriptor_projection is not None], np.int32), 0, str(self.device))
        if int(have[0]):
            p = vd.broadcast_array(self.descriptor_projection.cpu().numpy() if rank == 0 else None, 0, str(self.device))
            self.set_projection(p)

    def extract(self, image_dir: Path, db_path: Path, camera_model: str, camera_params: Optional[list] = None) -> None:
        """Same side effects as the reference's extract (hybrid_extractor.py:345-443): `extract_to_database`."""
        extract_to_database(self, image_dir, db_path, camera_model, camera_params)


def _cv2_importable() -> bool:
    try:
        import cv2  # noqa: F401, PLC0415
    except ImportError:
        return False
    return True
