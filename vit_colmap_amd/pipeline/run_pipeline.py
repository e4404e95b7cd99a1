"""Pipeline dispatcher for the hot path: extractor choice by `config.extractor.extractor_type`,
extraction into the COLMAP database, exhaustive matching (reference
vit_colmap/pipeline/run_pipeline.py:274-370, CLI :420-513).

Incremental mapping and plots stay outside the accelerated path; the database metrics and their
JSON / CSV export (§8f-3) are in utils/metrics.py and utils/export.py.  `do_reconstruction=True` hands the database to pycolmap if it
is importable and otherwise logs that the step is skipped.
"""
import argparse
import logging
from pathlib import Path
from typing import Optional

from ..database.colmap_db import ColmapDatabase
from ..features.base_extractor import BaseExtractor
from ..features.dummy_extractor import DummyExtractor
from ..utils.config import CAMERA_PARAM_NAMES, Config, parse_camera_params

logger = logging.getLogger(__name__)

MATCHER_TYPES = ("exhaustive", "retrieval")   # MatchingConfig.matcher_type / --matcher
BA_SOLVERS = ("dense", "pcg")                 # ReconstructionConfig.ba_solver / --ba-solver (mapping.bundle.SOLVERS)
BA_LOSSES = ("trivial", "huber", "soft_l1")   # ReconstructionConfig.ba_loss / --ba-loss (mapping.bundle.LOSSES)


class Pipeline:
    def __init__(self, config: Optional[Config] = None):
        self.config = config if config is not None else Config()
        self.last_stats = {}

    def _make_extractor(self) -> BaseExtractor:
        kind = self.config.extractor.extractor_type
        if kind == "dummy":                                   # run_pipeline.py:321-323
            logger.info("Using Dummy extractor")
            return DummyExtractor(step=32)
        if kind == "colmap_sift":                             # :323-325 — third-party C++ SIFT
            raise NotImplementedError(
                f"extractor_type={kind!r} is outside the accelerated hot path (SURVEY.md §2); "
                "use the reference implementation for it")
        if kind == "sift":                                    # COLMAP-default SIFT on the HIP kernels (csrc/sift.hip)
            logger.info("Using SIFT extractor")
            from ..features.sift_extractor import SiftExtractor

            return SiftExtractor()
        if kind == "trainable_vit":                           # :326-333
            logger.info("Using Trainable ViT extractor")
            from ..features.trainable_vit_extractor import TrainableViTExtractor

            return TrainableViTExtractor(weights_path=self.config.extractor.vit_weights_path, num_keypoints=20480,
                                         nms_radius=1, score_threshold=0.4)
        if kind == "hybrid":                                  # classical keypoints + ViT descriptors, detection on the device
            logger.info("Using Hybrid extractor (%s keypoints)", self.config.extractor.detector_type)
            from ..features.hybrid_extractor import HybridViTExtractor

            return HybridViTExtractor(weights_path=self.config.extractor.vit_weights_path,
                                      detector_type=self.config.extractor.detector_type, detector_backend="hip")
        logger.info("Using ViT extractor")                     # :335-339 (any other value -> ViT)
        from ..features.vit_extractor import ViTExtractor

        return ViTExtractor(weights_path=self.config.extractor.vit_weights_path)

    def run(self, image_dir: Path, output_dir: Path, db_path: Path, dataset: Optional[str] = None,
            scene: Optional[str] = None, results_dir: Optional[Path] = None):
        image_dir, output_dir, db_path = Path(image_dir), Path(output_dir), Path(db_path)
        camera_model = self.config.camera.model
        camera_params = self.config.camera.params
        output_dir.mkdir(parents=True, exist_ok=True)
        db_path.parent.mkdir(parents=True, exist_ok=True)

        matcher_type, num_neighbors = self.config.matching.matcher_type, self.config.matching.num_neighbors
        if matcher_type not in MATCHER_TYPES:
            raise ValueError(f"unknown matcher_type {matcher_type!r}: expected one of {', '.join(MATCHER_TYPES)}")
        if matcher_type == "retrieval" and int(num_neighbors) < 1:
            raise ValueError(f"num_neighbors must be at least 1 (got {num_neighbors})")
        seed_model = bool(getattr(self.config.reconstruction, "seed_model", False))
        sparse_model = bool(getattr(self.config.reconstruction, "sparse_model", False))
        bundle_adjustment = bool(getattr(self.config.reconstruction, "bundle_adjustment", False))
        if bundle_adjustment and not sparse_model:              # it adjusts the grown model (§4.2k)
            raise ValueError("bundle_adjustment needs reconstruction.sparse_model (--sparse-model)")
        refine_focal_length = bool(getattr(self.config.reconstruction, "refine_focal_length", False))
        if refine_focal_length and not bundle_adjustment:       # it is one more unknown of that adjustment (§4.2k)
            raise ValueError("refine_focal_length needs reconstruction.bundle_adjustment (--bundle-adjustment)")
        refine_distortion = bool(getattr(self.config.reconstruction, "refine_distortion", False))
        if refine_distortion and not bundle_adjustment:         # k1 (and k2) are further unknowns of that adjustment (§4.2k)
            raise ValueError("refine_distortion needs reconstruction.bundle_adjustment (--bundle-adjustment)")
        split_tracks = bool(getattr(self.config.reconstruction, "split_tracks", False))
        if split_tracks and not sparse_model:                   # it is a step of that model's growth (§4.2n)
            raise ValueError("split_tracks needs reconstruction.sparse_model (--sparse-model)")
        tangential = bool(getattr(self.config.reconstruction, "tangential_distortion", False))
        if tangential and not (seed_model or sparse_model):     # it lets OPENCV cameras into those models (§4.2k, "The tangential terms")
            raise ValueError("tangential_distortion needs reconstruction.seed_model (--seed-model) or reconstruction.sparse_model "
                             "(--sparse-model)")
        adjust_rounds = bool(getattr(self.config.reconstruction, "adjust_rounds", False))
        if adjust_rounds and not bundle_adjustment:             # it is that adjustment after every growth round (§4.2m)
            raise ValueError("adjust_rounds needs reconstruction.bundle_adjustment (--bundle-adjustment)")
        ba_loss =str(getattr(self.config.reconstruction, "ba_loss", "trivial"))
        ba_loss_scale = float(getattr(self.config.reconstruction, "ba_loss_scale", 1.0))
        if ba_loss not in BA_LOSSES:
            raise ValueError(f"unknown ba_loss {ba_loss!r}: expected one of {', '.join(BA_LOSSES)}")
        if ba_loss != "trivial" and not bundle_adjustment:      # it is the loss of that adjustment (§4.2k)
            raise ValueError("ba_loss needs reconstruction.bundle_adjustment (--bundle-adjustment)")
        if not 0.0 < ba_loss_scale < float("inf"):
            raise ValueError(f"ba_loss_scale must be a finite positive number of pixels (got {ba_loss_scale})")
        loss_args = {} if ba_loss == "trivial" else dict(loss=ba_loss, loss_scale=ba_loss_scale)
        known_distortion = bool(getattr(self.config.camera, "known_distortion", False))
        if known_distortion and not self.config.camera.prior_focal_length:   # it is what makes the intrinsics trusted (§4.2l)
            raise ValueError("known_distortion needs camera.prior_focal_length (--prior-focal-length)")
        estimate_focal_length = bool(getattr(self.config.camera, "estimate_focal_length", False))
        if estimate_focal_length and known_distortion:         # an estimated focal length is not a known camera (§4.2o)
            raise ValueError("estimate_focal_length cannot be combined with camera.known_distortion (--known-distortion): an "
                             "estimated focal length is not a known camera")
        ba_solver = str(getattr(self.config.reconstruction, "ba_solver", "dense"))
        if ba_solver not in BA_SOLVERS:
            raise ValueError(f"unknown ba_solver {ba_solver!r}: expected one of {', '.join(BA_SOLVERS)}")
        if ba_solver != "dense" and not bundle_adjustment:      # it is how that adjustment solves its system (§4.2k, "The solver")
            raise ValueError("ba_solver needs reconstruction.bundle_adjustment (--bundle-adjustment)")
        if ba_solver != "dense" and (refine_focal_length or refine_distortion or known_distortion):
            raise ValueError(f"ba_solver {ba_solver!r} adjusts poses and points only: refine_focal_length, refine_distortion and "
                             "known_distortion go through the border of the system or the _radial entry points, which need the dense "
                             "solver (out of scope of pcg)")
        solver_args = {} if ba_solver == "dense" else dict(solver=ba_solver)   # passed on only where it is not the default
        if camera_params is not None and camera_model in CAMERA_PARAM_NAMES:   # the count, before any database is created
            camera_params = parse_camera_params(camera_params, camera_model)
        known_args = dict(known_distortion=True) if known_distortion else {}
        if tangential:                                          # travels with it: passed on only where it is on
            known_args["tangential"] = True
        rounds_args = dict(adjust_rounds=True) if adjust_rounds else {}   # passed on only where it is on, as known_distortion is
        if split_tracks:                                        # likewise; it goes wherever the growth runs
            rounds_args["split_tracks"] = True
        for wanted, name in ((seed_model, "seed_model"), (sparse_model, "sparse_model")):
            if not wanted:                                      # both read calibrated rows with a pose (§4.2i, §4.2j)
                continue
            for on, flag in ((self.config.camera.prior_focal_length or estimate_focal_length,   # either makes rows CALIBRATED (§4.2o)
                              "camera.prior_focal_length (--prior-focal-length)"),
                             (self.config.matching.compute_relative_pose, "matching.compute_relative_pose (--relative-pose)"),
                             (self.config.do_matching, "do_matching (no --skip-matching)")):
                if not on:
                    raise ValueError(f"{name} needs {flag}")

        extractor = self._make_extractor()
        extractor.prior_focal_length = bool(self.config.camera.prior_focal_length)
        from .. import dist as vd

        if vd.is_distributed():
            # one process per GPU (torchrun): images and pairs sharded, one descriptor all-gather, rank 0 writes (§8e)
            from .distributed import run_sharded

            if not hasattr(extractor, "_run_batch"):
                raise NotImplementedError(f"{type(extractor).__name__} has no batched device path to shard")
            logger.info("Extracting + matching on %d ranks...", vd.rank_world()[1])
            if hasattr(extractor, "sync_projection"):
                extractor.sync_projection(image_dir)      # the PCA / random projection is fitted once, on rank 0
            self.last_stats = run_sharded(image_dir, db_path, camera_model, camera_params, feature_fn=extractor._run_batch,
                                          camera_params_for=extractor.camera_params_for,
                                          camera_per_image=extractor.camera_per_image,
                                          prior_focal_length=extractor.prior_focal_length,
                                          matching_options=self._matching_options(),
                                          do_matching=self.config.do_matching, device=str(getattr(extractor, "device", "cuda")),
                                          matcher_type=matcher_type)
            if vd.rank_world()[0] != 0:
                return None
        else:
            logger.info("Extracting features...")
            extractor.extract(image_dir, db_path, camera_model, camera_params)
            with ColmapDatabase.open_database(str(db_path)) as db_check:
                num_imgs = ColmapDatabase.get_db_count(db_check, "num_images")
                logger.info(f"Extracted features for {num_imgs} images")

            if self.config.do_matching:
                from ..matching import match_exhaustive, match_retrieval

                logger.info("Running feature matching...")
                opts = self._matching_options()
                if matcher_type == "retrieval":
                    self.last_stats = match_retrieval(database_path=str(db_path), matching_options=opts,
                                                      num_neighbors=num_neighbors)
                else:
                    self.last_stats = match_exhaustive(database_path=str(db_path), matching_options=opts)
        if self.config.do_matching:
            with ColmapDatabase.open_database(str(db_path)) as db_check:
                num_pairs = ColmapDatabase.get_db_count(db_check, "num_matched_image_pairs")
                logger.info(f"Matched {num_pairs} image pairs ({db_check.num_verified_image_pairs()} geometrically verified)")

        if estimate_focal_length and self.config.do_matching:   # under torchrun only rank 0 arrives here
            self._estimate_focal_lengths(db_path, str(getattr(extractor, "device", "cuda")))
        if seed_model:
            self._write_seed_model(db_path, output_dir, str(getattr(extractor, "device", "cuda")), **known_args)
        if sparse_model:
            if refine_distortion:
                self._write_sparse_model(db_path, output_dir, str(getattr(extractor, "device", "cuda")), adjust=True,
                                         refine_focal_length=refine_focal_length, refine_distortion=True, **loss_args, **known_args,
                                         **rounds_args)
            elif refine_focal_length:
                self._write_sparse_model(db_path, output_dir, str(getattr(extractor, "device", "cuda")), adjust=True, refine_focal_length=True,
                                         **loss_args, **known_args, **rounds_args)
            else:
                self._write_sparse_model(db_path, output_dir, str(getattr(extractor, "device", "cuda")), adjust=bundle_adjustment, **loss_args,
                                         **known_args, **rounds_args, **solver_args)

        reconstructions = None
        if self.config.do_reconstruction:
            try:
                import pycolmap  # noqa: PLC0415
            except ImportError:
                logger.warning("3D reconstruction skipped: pycolmap is not installed and incremental mapping is "
                               "outside the accelerated path")
            else:
                with ColmapDatabase.open_database(str(db_path)) as db_check:
                    n_verified = db_check.num_verified_image_pairs()
                if n_verified == 0:
                    # the mapper only reads two_view_geometries: on a database without verified pairs it returns no model
                    # and says nothing
                    logger.warning("no geometrically verified image pair in the database (two_view_geometries is empty): "
                                   "incremental mapping will not find an initial pair")
                sparse_dir = output_dir / "sparse"
                sparse_dir.mkdir(parents=True, exist_ok=True)
                reconstructions = pycolmap.incremental_mapping(
                    database_path=str(db_path), image_path=str(image_dir), output_path=str(sparse_dir),
                    options=self.config.reconstruction.to_mapper_options())
        if dataset and scene:                                   # run_pipeline.py:406-415
            self.extract_and_export_metrics(db_path, output_dir, reconstructions, dataset, scene, results_dir)
        return reconstructions

    def _matching_options(self):
        """The matching options with `camera.known_distortion` on them (§4.2l), set only where it is on."""
        opts = self.config.matching.to_matching_options()
        if getattr(self.config.camera, "known_distortion", False):
            opts.known_distortion = opts.sift.known_distortion = True
        return opts

    def _estimate_focal_lengths(self, db_path, device, cost_fn=None, verify_fn=None):
        """`camera.estimate_focal_length` (§4.2o): the focal length of every camera without a prior from its UNCALIBRATED rows
        (`last_stats["focal_estimates"]`), written into the cameras table with the prior flag; if any camera changed, every
        matched pair is verified again from the stored `matches`, with `relative_pose` as configured, and its row replaced
        (`last_stats["focal_reverified_pairs"]`).  `cost_fn` and `verify_fn` replace the launches in the CPU tests."""
        from ..matching.focal import apply_focal_estimates, estimate_focal_lengths, reverify_database

        with ColmapDatabase.open_database(str(db_path)) as db:
            ids = [im.image_id for im in db.read_all_images()]
            estimates = estimate_focal_lengths(db, ids, device, cost_fn)
            changed = apply_focal_estimates(db, estimates)
            self.last_stats = dict(self.last_stats or {}, focal_estimates=estimates)
            if changed:
                if self.config.matching.guided_matching:
                    logger.warning("estimate_focal_length: the pairs are verified again from the stored matches; their rows "
                                   "carry the verifier's inliers, not the guided lists")
                n = reverify_database(db, ids, device, verify_fn, bool(self.config.matching.compute_relative_pose))
                self.last_stats["focal_reverified_pairs"] = n
                logger.info("Estimated the focal length of %d camera(s); %d pairs verified again (%d verified)", len(changed),
                            ColmapDatabase.get_db_count(db, "num_matched_image_pairs"), n)

    def _write_seed_model(self, db_path, output_dir, device, known_distortion=False, tangential=False):
        """output_dir/sparse/seed and `last_stats["seed_model"]`; a scene without an admissible initial pair writes nothing.
        `known_distortion`: passed on only where it is on (§4.2l); `tangential` likewise ("The tangential terms" in §4.2k)."""
        from ..mapping import build_seed_model

        known_args = dict(known_distortion=True) if known_distortion else {}
        if tangential:
            known_args["tangential"] = True
        try:
            model = build_seed_model(str(db_path), device=device, **known_args)
        except ValueError as e:
            logger.warning("no seed model written: %s", e)
            return
        model.write_text(str(Path(output_dir) / "sparse" / "seed"))
        self.last_stats = dict(self.last_stats or {}, seed_model=model.stats())
        logger.info("Seed model: pair %s, %d images, %d points", *[model.stats()[k] for k in
                                                                    ("initial_pair", "registered_images", "num_points3D")])

    def _write_sparse_model(self, db_path, output_dir, device, adjust=False, refine_focal_length=False, loss="trivial", loss_scale=1.0,
                            refine_distortion=False, known_distortion=False, adjust_rounds=False, solver="dense", split_tracks=False,
                            tangential=False):
        """output_dir/sparse/grown and `last_stats["sparse_model"]`; a scene without an admissible initial pair writes nothing.
        `adjust`: also output_dir/sparse/adjusted and `last_stats["bundle_adjustment"]`, the grown model bundle-adjusted;
        `refine_focal_length`: that adjustment also refines the cameras' focal lengths; `loss`, `loss_scale`: its loss, passed on
        only where it is not the trivial one; `refine_distortion`: it also refines k1 (k2) of SIMPLE_RADIAL and RADIAL cameras;
        `known_distortion`: both models are built on undistorted keypoints (§4.2l), passed on only where it is on;
        `adjust_rounds` (with `adjust`): also output_dir/sparse/mapped and `last_stats["mapped_model"]`, the model grown with an
        adjustment and a re-evaluation of its tracks after every round (§4.2m), under the same options; the other two models are
        built and written as without it.  `solver`: how the adjustments solve their system ("The solver" in §4.2k), passed on
        only where it is not "dense".  `split_tracks`: the growth of the grown and of the mapped model splits its inconsistent
        components (§4.2n), passed on only where it is on; the adjusted model is the grown one adjusted, so it has their points too.
        `tangential`: OPENCV cameras are mapped and adjusted ("The tangential terms" in §4.2k), passed on to all three builders only
        where it is on."""
        from ..mapping.grow import build_sparse_model

        known_args = dict(known_distortion=True) if known_distortion else {}
        if tangential:
            known_args["tangential"] = True
        split_args = dict(split_tracks=True) if split_tracks else {}
        try:
            model = build_sparse_model(str(db_path), device=device, **known_args, **split_args)
        except ValueError as e:
            logger.warning("no sparse model written: %s", e)
            return
        model.write_text(str(Path(output_dir) / "sparse" / "grown"))
        self.last_stats = dict(self.last_stats or {}, sparse_model=model.stats())
        logger.info("Sparse model: pair %s, %d images, %d points, %d rounds", *[model.stats()[k] for k in
                                                                                 ("initial_pair", "registered_images", "num_points3D", "rounds")])
        if adjust:
            from ..mapping.bundle import build_adjusted_model

            loss_args = {} if loss == "trivial" else dict(loss=loss, loss_scale=loss_scale)
            solver_args = {} if solver == "dense" else dict(solver=solver)
            if refine_distortion:
                adjusted = build_adjusted_model(str(db_path), device=device, grown=model, refine_focal_length=refine_focal_length,
                                                refine_distortion=True, **loss_args, **known_args)
            elif refine_focal_length:
                adjusted = build_adjusted_model(str(db_path), device=device, grown=model, refine_focal_length=True, **loss_args, **known_args)
            else:
                adjusted = build_adjusted_model(str(db_path), device=device, grown=model, **loss_args, **known_args, **solver_args)
            adjusted.write_text(str(Path(output_dir) / "sparse" / "adjusted"))
            self.last_stats = dict(self.last_stats, bundle_adjustment=adjusted.stats())
            logger.info("Adjusted model: %d images, %d points, cost %.6g -> %.6g", len(adjusted.images), len(adjusted.points3D),
                        adjusted.bundle_adjustment["initial_cost"], adjusted.bundle_adjustment["final_cost"])
            if adjust_rounds:
                from ..mapping.rounds import build_mapped_model

                refine_args = dict(refine_focal_length=refine_focal_length, refine_distortion=refine_distortion)
                mapped = build_mapped_model(str(db_path), device=device, **{k: v for k, v in refine_args.items() if v}, **loss_args,
                                            **known_args, **solver_args, **split_args)
                mapped.write_text(str(Path(output_dir) / "sparse" / "mapped"))
                self.last_stats = dict(self.last_stats, mapped_model=mapped.stats())
                logger.info("Mapped model: %d images, %d points, %d round adjustments", len(mapped.images), len(mapped.points3D),
                            len(mapped.round_adjustments))

    def extract_and_export_metrics(self, db_path, output_dir, reconstructions, dataset, scene, results_dir=None):
        """Database metrics -> `{results_dir}/{dataset}/{scene}/{extractor}.json` + summary.csv row
        (reference run_pipeline.py:211-271; reconstruction metrics stay empty: the mapper is out of scope)."""
        from ..utils.export import export_metrics, extract_all_metrics

        try:
            kind = self.config.extractor.extractor_type
            kind = "sift" if kind == "colmap_sift" else kind
            cfg = {"camera_model": self.config.camera.model, "min_num_matches": self.config.reconstruction.min_num_matches,
                   "matching_max_ratio": self.config.matching.max_ratio, "matching_use_gpu": self.config.matching.use_gpu}
            metrics = extract_all_metrics(db_path, dataset, scene, kind, cfg)
            if results_dir:
                export_metrics(metrics, Path(results_dir), formats=["json", "csv"])
            return metrics
        except Exception as e:  # noqa: BLE001 - reporting must never fail the run (run_pipeline.py:267-271)
            logger.error(f"Failed to extract/export metrics: {e}")
            return None


def main() -> None:
    """Same flags as the reference CLI for the path (run_pipeline.py:426-495)."""
    ap = argparse.ArgumentParser(description="vit-colmap hot path on MI355X")
    ap.add_argument("--images", type=Path, required=True)
    ap.add_argument("--output", type=Path, required=True)
    ap.add_argument("--db", type=Path, required=True)
    ap.add_argument("--camera-model", dest="camera_model", default="SIMPLE_PINHOLE")
    ap.add_argument("--prior-focal-length", dest="prior_focal_length", action="store_true",
                    help="mark the cameras as calibrated: pairs are also verified under an essential matrix")
    ap.add_argument("--estimate-focal-length", dest="estimate_focal_length", action="store_true",
                    help="the focal length is unknown: after matching it is estimated per camera from the fundamental matrices of "
                         "the verified pairs (one scale on the stored focal length, a quarter to four times it), the camera is "
                         "marked calibrated and every pair is verified again; stands in for --prior-focal-length in front of "
                         "--seed-model and --sparse-model (not with --known-distortion)")
    ap.add_argument("--camera-params", dest="camera_params", default=None, metavar="P1,P2,...",
                    help="the intrinsics of --camera-model as a comma-separated list in COLMAP's order (SIMPLE_RADIAL: f,cx,cy,k; "
                         "OPENCV: fx,fy,cx,cy,k1,k2,p1,p2); by default f = max(w, h) and the image centre")
    ap.add_argument("--known-distortion", dest="known_distortion", action="store_true",
                    help="with --prior-focal-length: trust a non-zero distortion in --camera-params too; keypoints are undistorted "
                         "on the GPU in front of verification, relative pose, registration and triangulation")
    ap.add_argument("--extractor", choices=["vit", "trainable_vit", "hybrid", "sift", "colmap_sift", "dummy"], default="vit")
    ap.add_argument("--detector", choices=["sift", "fast", "gftt"], default="sift",
                    help="keypoint detector of --extractor hybrid (runs on the GPU)")
    ap.add_argument("--vit-weights", dest="vit_weights", type=Path, default=None)
    ap.add_argument("--skip-matching", dest="skip_matching", action="store_true")
    ap.add_argument("--guided-matching", dest="guided_matching", action="store_true",
                    help="re-match every verified pair under its estimated F or H (COLMAP's guided_matching)")
    ap.add_argument("--relative-pose", dest="relative_pose", action="store_true",
                    help="pose, triangulation angle and the PLANAR / PANORAMIC split of the pairs whose cameras have a "
                         "focal-length prior (COLMAP's compute_relative_pose)")
    ap.add_argument("--seed-model", dest="seed_model", action="store_true",
                    help="write output/sparse/seed: an initial pair, its triangulated points and every other image registered "
                         "against them (needs --prior-focal-length and --relative-pose)")
    ap.add_argument("--sparse-model", dest="sparse_model", action="store_true",
                    help="write output/sparse/grown: the seed model grown by rounds of track triangulation and registration "
                         "(needs --prior-focal-length and --relative-pose)")
    ap.add_argument("--split-tracks", dest="split_tracks", action="store_true",
                    help="with --sparse-model: a track that a wrong match fused with another (two of its keypoints in one image) is "
                         "split into up to 4 points instead of being discarded")
    ap.add_argument("--bundle-adjustment", dest="bundle_adjustment", action="store_true",
                    help="with --sparse-model: also write output/sparse/adjusted, the grown model after one global bundle "
                         "adjustment, rescaled to a unit baseline and filtered")
    ap.add_argument("--refine-focal-length", dest="refine_focal_length", action="store_true",
                    help="with --bundle-adjustment: the adjustment also refines the focal length(s) of every camera; the "
                         "adjusted model's cameras.txt carries the refined values")
    ap.add_argument("--refine-distortion", dest="refine_distortion", action="store_true",
                    help="with --bundle-adjustment: the adjustment also refines the radial distortion, k of SIMPLE_RADIAL cameras and "
                         "k1, k2 of RADIAL ones, from the values in the database (0 as the extractors write them)")
    ap.add_argument("--tangential-distortion", dest="tangential_distortion", action="store_true",
                    help="with --seed-model or --sparse-model: OPENCV cameras are mapped and, with --bundle-adjustment, adjusted under "
                         "their full distortion k1, k2, p1, p2 (with --refine-distortion all four are refined)")
    ap.add_argument("--adjust-rounds", dest="adjust_rounds", action="store_true",
                    help="with --bundle-adjustment: also write output/sparse/mapped, the model grown with a bundle adjustment and a "
                         "re-evaluation of every track after each growth round; what long sequences need")
    ap.add_argument("--ba-loss", dest="ba_loss", choices=list(BA_LOSSES), default="trivial",
                    help="with --bundle-adjustment: the loss of the adjustment; huber and soft_l1 keep observations that are tens "
                         "of pixels off their point from setting the poses")
    ap.add_argument("--ba-loss-scale", dest="ba_loss_scale", type=float, default=1.0, metavar="PX",
                    help="the residual in pixels at which --ba-loss leaves the square")
    ap.add_argument("--ba-solver", dest="ba_solver", choices=list(BA_SOLVERS), default="dense",
                    help="with --bundle-adjustment: dense factors the reduced camera system (at most 512 registered images); pcg solves "
                         "it by preconditioned conjugate gradients without forming it and has no such limit (poses and points only: "
                         "not with --refine-focal-length, --refine-distortion or --known-distortion)")
    ap.add_argument("--matcher", choices=list(MATCHER_TYPES), default="exhaustive",
                    help="exhaustive: every image pair; retrieval: each image against its --num-neighbors nearest images")
    ap.add_argument("--num-neighbors", dest="num_neighbors", type=int, default=20,
                    help="images per image that --matcher retrieval matches (at most 64)")
    ap.add_argument("--skip-reconstruction", dest="skip_reconstruction", action="store_true")
    ap.add_argument("--dataset", default=None)
    ap.add_argument("--scene", default=None)
    ap.add_argument("--export-metrics", dest="export_metrics", type=Path, default=None)
    ap.add_argument("-v", "--verbose", action="store_true")
    args = ap.parse_args()
    config = Config.from_args(args)
    logging.getLogger(__name__).info(config.summary())
    Pipeline(config).run(args.images, args.output, args.db, args.dataset, args.scene, args.export_metrics)
