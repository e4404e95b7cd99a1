"""Image registration and the seed model, imported only when `ReconstructionConfig.seed_model` or
`sparse_model` is set; the growth of the seed model (§4.2j: `mapping.grow`, `mapping.triangulate`) is imported only with the latter,
the bundle adjustment of the grown model (§4.2k: `mapping.bundle`) only with `bundle_adjustment`, its border of refined
focal lengths (`mapping.bundle_intr`) only with `refine_focal_length`, and the adjustment per growth round (§4.2m:
`mapping.rounds`) only with `adjust_rounds`."""
from .absolute_pose import estimate_absolute_poses, score_poses, solve_p3p
from .seed import SparseModel, build_seed_model

__all__ = ["SparseModel", "build_seed_model", "estimate_absolute_poses", "score_poses", "solve_p3p"]
