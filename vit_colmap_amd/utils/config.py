"""Configuration dataclasses — same field names and defaults as reference
vit_colmap/utils/config.py:9-198, without the pycolmap dependency: the option objects returned by
`to_matching_options()` are the plain classes below, consumed by
vit_colmap_amd.matching.match_exhaustive."""
import logging
from dataclasses import dataclass, field
from typing import Optional


@dataclass
class LogConfig:
    """config.py:9-25"""

    level: int = logging.INFO
    format: str = "[%(asctime)s][%(filename)s:%(lineno)d][%(levelname)s] %(message)s"
    datefmt: str = "%H:%M:%S"

    def apply(self):
        logging.basicConfig(level=self.level, format=self.format, datefmt=self.datefmt, force=True)


@dataclass
class CameraConfig:
    """config.py:28-52"""

    model: str = "SIMPLE_PINHOLE"
    width: Optional[int] = None
    height: Optional[int] = None
    params: Optional[list[float]] = None
    prior_focal_length: bool = False   # the intrinsics are trusted: pairs are also verified under E (not set by the reference)
    estimate_focal_length: bool = False   # the focal length is unknown: it is estimated from the UNCALIBRATED pairs after matching, the camera is flagged and every pair verified again (§4.2o)
    known_distortion: bool = False     # with prior_focal_length: a non-zero distortion in `params` is trusted too, keypoints are undistorted in front of the solvers (§4.2l)

    def get_default_params(self, width: int, height: int) -> list[float]:
        if self.params is not None:
            return self.params
        from ..features.base_extractor import default_camera_params

        try:
            return default_camera_params(self.model, width, height)
        except ValueError:
            raise ValueError(f"Unsupported camera model: {self.model}")


CAMERA_PARAM_NAMES = {"SIMPLE_PINHOLE": "f, cx, cy", "PINHOLE": "fx, fy, cx, cy", "SIMPLE_RADIAL": "f, cx, cy, k",
                      "RADIAL": "f, cx, cy, k1, k2", "OPENCV": "fx, fy, cx, cy, k1, k2, p1, p2"}


def parse_camera_params(text, model) -> list[float]:
    """--camera-params: a comma-separated list of floats (or a sequence of numbers) for `model` -> the list; ValueError, naming
    the model and the count it takes, for another length, an unknown model or something that is no finite number."""
    if model not in CAMERA_PARAM_NAMES:
        raise ValueError(f"camera_params: unknown camera model {model!r}, expected one of {', '.join(CAMERA_PARAM_NAMES)}")
    names = CAMERA_PARAM_NAMES[model]
    want = len(names.split(", "))
    fields = [w.strip() for w in text.split(",")] if isinstance(text, str) else list(text)
    try:
        params = [float(w) for w in fields]
    except (TypeError, ValueError):
        params = None
    if params is None or len(params) != want or not all(abs(v) < float("inf") for v in params):
        raise ValueError(f"camera_params: camera model {model} takes {want} finite numbers ({names}), got {text!r}")
    return params


@dataclass
class SiftMatchingOptions:
    """The fields of pycolmap's SiftMatchingOptions that the reference sets (config.py:72-94)."""

    max_ratio: float = 0.8
    max_distance: float = 0.7
    cross_check: bool = True
    use_gpu: bool = True
    num_threads: int = -1
    guided_matching: bool = False   # pycolmap 3.12 keeps the option here [recalled]
    compute_relative_pose: bool = False   # carried as guided_matching is (COLMAP: TwoViewGeometryOptions [recalled])
    known_distortion: bool = False   # carried likewise: CameraConfig.known_distortion on its way to the matcher (§4.2l)


@dataclass
class FeatureMatchingOptions:
    """Shape of pycolmap 3.13's FeatureMatchingOptions (config.py:70-81): `.sift` sub-options."""

    use_gpu: bool = True
    num_threads: int = -1
    guided_matching: bool = False   # pycolmap 3.13 moved the option to the outer object [recalled]
    compute_relative_pose: bool = False
    known_distortion: bool = False
    sift: SiftMatchingOptions = field(default_factory=SiftMatchingOptions)


@dataclass
class MatchingConfig:
    """config.py:55-96"""

    use_gpu: bool = True
    max_ratio: float = 0.8
    max_distance: float = 0.7
    cross_check: bool = True
    num_threads: int = -1  # -1 means auto-detect
    guided_matching: bool = False  # re-match verified pairs under their F or H model (not set by the reference)
    compute_relative_pose: bool = False  # pose, triangulation angle, PLANAR / PANORAMIC of the pairs with priors (not set by it)
    matcher_type: str = "exhaustive"  # "exhaustive": every pair; "retrieval": each image against its nearest images only
    num_neighbors: int = 20  # images per image that matcher_type "retrieval" matches (at most VC_MAX_NEIGHBOURS)

    def to_matching_options(self) -> FeatureMatchingOptions:
        opts = FeatureMatchingOptions(use_gpu=self.use_gpu, num_threads=self.num_threads,
                                      guided_matching=self.guided_matching,
                                      compute_relative_pose=self.compute_relative_pose)
        opts.sift.max_ratio = self.max_ratio
        opts.sift.max_distance = self.max_distance
        opts.sift.cross_check = self.cross_check
        opts.sift.use_gpu = self.use_gpu
        opts.sift.num_threads = self.num_threads
        opts.sift.guided_matching = self.guided_matching
        opts.sift.compute_relative_pose = self.compute_relative_pose
        return opts

    def _to_sift_options_legacy(self) -> SiftMatchingOptions:
        return SiftMatchingOptions(max_ratio=self.max_ratio, max_distance=self.max_distance,
                                   cross_check=self.cross_check, use_gpu=self.use_gpu,
                                   num_threads=self.num_threads, guided_matching=self.guided_matching,
                                   compute_relative_pose=self.compute_relative_pose)


@dataclass
class ReconstructionConfig:
    """config.py:99-112.  Incremental mapping is outside the hot path; the options
    object is only built when pycolmap is importable."""

    min_num_matches: int = 15
    multiple_models: bool = True
    seed_model: bool = False     # write output_dir/sparse/seed: an initial pair, its points, every other image registered (§4.2i)
    sparse_model: bool = False   # write output_dir/sparse/grown: the seed model grown by rounds of triangulation and registration (§4.2j)
    split_tracks: bool = False   # with sparse_model: tracks with two keypoints in one image are split into up to 4 points, not discarded (§4.2n)
    bundle_adjustment: bool = False   # with sparse_model: write output_dir/sparse/adjusted, the grown model bundle-adjusted once (§4.2k)
    refine_focal_length: bool = False   # with bundle_adjustment: the adjustment also refines every camera's focal length(s) (§4.2k)
    ba_loss: str = "trivial"     # with bundle_adjustment: the loss of the adjustment, "trivial", "huber" or "soft_l1" (§4.2k, "The loss")
    ba_loss_scale: float = 1.0   # px: the residual at which the loss leaves the square
    refine_distortion: bool = False   # with bundle_adjustment: it also refines k of SIMPLE_RADIAL, k1 and k2 of RADIAL cameras (§4.2k)
    ba_solver: str = "dense"     # with bundle_adjustment: how the reduced camera system is solved, "dense" (Cholesky of S, at most VC_BA_MAX_CAMS images) or "pcg" (conjugate gradients without S, no limit; §4.2k, "The solver")
    tangential_distortion: bool = False   # with seed_model or sparse_model: OPENCV cameras are mapped and adjusted under k1, k2, p1, p2 (§4.2k, "The tangential terms")
    adjust_rounds: bool = False   # with bundle_adjustment: write output_dir/sparse/mapped, grown with an adjustment and a re-evaluation of the tracks per round (§4.2m)

    def to_mapper_options(self):
        import pycolmap  # noqa: PLC0415 - optional, third party

        opts = pycolmap.IncrementalPipelineOptions()
        opts.min_num_matches = self.min_num_matches
        opts.multiple_models = self.multiple_models
        return opts


@dataclass
class ExtractorConfig:
    """config.py:115-120"""

    extractor_type: str = "vit"  # "vit" or "colmap_sift"
    vit_weights_path: Optional[str] = None
    detector_type: str = "sift"  # keypoint detector of extractor_type "hybrid": "sift", "fast" or "gftt"


@dataclass
class Config:
    """config.py:123-198"""

    log: LogConfig = field(default_factory=LogConfig)
    camera: CameraConfig = field(default_factory=CameraConfig)
    extractor: ExtractorConfig = field(default_factory=ExtractorConfig)
    matching: MatchingConfig = field(default_factory=MatchingConfig)
    reconstruction: ReconstructionConfig = field(default_factory=ReconstructionConfig)
    do_matching: bool = True
    do_reconstruction: bool = True

    def __post_init__(self):
        self.log.apply()

    @classmethod
    def from_args(cls, args):
        config = cls()
        if hasattr(args, "camera_model"):
            config.camera.model = args.camera_model
        if getattr(args, "prior_focal_length", False):
            config.camera.prior_focal_length = True
        if getattr(args, "known_distortion", False):
            config.camera.known_distortion = True
        if getattr(args, "estimate_focal_length", False):
            config.camera.estimate_focal_length = True
        if getattr(args, "camera_params", None) is not None:
            config.camera.params = parse_camera_params(args.camera_params, config.camera.model)
        if hasattr(args, "extractor") and args.extractor:
            config.extractor.extractor_type = args.extractor
        elif hasattr(args, "use_colmap_sift") and args.use_colmap_sift:
            config.extractor.extractor_type = "colmap_sift"
        if hasattr(args, "vit_weights") and args.vit_weights:
            config.extractor.vit_weights_path = str(args.vit_weights)
        elif hasattr(args, "model") and args.model:
            config.extractor.vit_weights_path = str(args.model)
        if hasattr(args, "detector") and args.detector:
            config.extractor.detector_type = args.detector
        if hasattr(args, "use_gpu"):
            config.matching.use_gpu = args.use_gpu
        if getattr(args, "guided_matching", False):
            config.matching.guided_matching = True
        if getattr(args, "relative_pose", False):
            config.matching.compute_relative_pose = True
        if getattr(args, "seed_model", False):
            config.reconstruction.seed_model = True
        if getattr(args, "sparse_model", False):
            config.reconstruction.sparse_model = True
        if getattr(args, "split_tracks", False):
            config.reconstruction.split_tracks = True
        if getattr(args, "bundle_adjustment", False):
            config.reconstruction.bundle_adjustment = True
        if getattr(args, "refine_focal_length", False):
            config.reconstruction.refine_focal_length = True
        if getattr(args, "refine_distortion", False):
            config.reconstruction.refine_distortion = True
        if getattr(args, "tangential_distortion", False):
            config.reconstruction.tangential_distortion = True
        if getattr(args, "adjust_rounds", False):
            config.reconstruction.adjust_rounds = True
        if getattr(args, "ba_loss", None):
            config.reconstruction.ba_loss = args.ba_loss
        if getattr(args, "ba_loss_scale", None) is not None:
            config.reconstruction.ba_loss_scale = float(args.ba_loss_scale)
        if getattr(args, "ba_solver", None):
            config.reconstruction.ba_solver = args.ba_solver
        if getattr(args, "matcher", None):
            config.matching.matcher_type = args.matcher
        if getattr(args, "num_neighbors", None) is not None:
            config.matching.num_neighbors = args.num_neighbors
        if hasattr(args, "skip_matching"):
            config.do_matching = not args.skip_matching
        if hasattr(args, "skip_reconstruction"):
            config.do_reconstruction = not args.skip_reconstruction
        if hasattr(args, "verbose") and args.verbose:
            config.log.level = logging.DEBUG
            config.log.apply()
        return config

    def summary(self) -> str:
        lines = [
            "Configuration:",
            f"  Extractor: {self.extractor.extractor_type}",
            f"  Camera model: {self.camera.model}",
            f"  Matching: {'enabled' if self.do_matching else 'disabled'}",
            f"  Reconstruction: {'enabled' if self.do_reconstruction else 'disabled'}",
            f"  GPU matching: {'enabled' if self.matching.use_gpu else 'disabled'}",
            f"  Min matches: {self.reconstruction.min_num_matches}",
        ]
        return "\n".join(lines)
