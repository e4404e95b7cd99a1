from .exhaustive import match_exhaustive
from .hip_matcher import (exhaustive_pairs, knn_top2, match_pairs, match_pairs_guided, mutual_ratio, prepare_descriptors,
                          theta_table)
from .retrieval import global_descriptors, match_retrieval, nearest_images, pool_descriptors, retrieval_pairs

__all__ = ["exhaustive_pairs", "global_descriptors", "knn_top2", "match_exhaustive", "match_pairs", "match_pairs_guided",
           "match_retrieval", "mutual_ratio", "nearest_images", "pool_descriptors", "prepare_descriptors", "retrieval_pairs",
           "theta_table"]
