"""Image registration and the seed model.  Imported only when `ReconstructionConfig.seed_model` is set."""
from .absolute_pose import estimate_absolute_poses, score_poses, solve_p3p
from .seed import SparseModel, build_seed_model

__all__ = ["SparseModel", "build_seed_model", "estimate_absolute_poses", "score_poses", "solve_p3p"]
