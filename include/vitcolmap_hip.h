/*
 * vitcolmap_hip.h — C ABI of libvitcolmap_hip.so (gfx950 / MI355X).
 *
 * The drop-in boundary for the hot path of randyjhc/vit-colmap: everything the reference
 * computes between "ViT patch tokens" and "rows in the COLMAP database", plus the exhaustive
 * descriptor matcher.  The reference has no FFI of its own (it is pure Python calling torch and
 * pycolmap), so each entry point cites the reference *method* it replaces; INTEGRATION.md shows
 * the ctypes stub a maintainer of the reference would add at that call site.
 *
 * Conventions
 *   - Every pointer is a DEVICE pointer owned by the caller unless marked [host].
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Calls only enqueue
 *     work on it; they never synchronise, allocate or free (safe under hipGraph capture).
 *   - Return value: VC_OK (0) or a negative VC_ERR_* code.  No exceptions cross the boundary,
 *     there is no global mutable state, and calls on distinct streams are independent.
 *   - Layouts are row-major, densely packed.  "tokens" = (images, H*W, C) float32, i.e. the
 *     ViT's own output order (token index = y*W + x, reference vit_extractor.py:150-156 builds
 *     its (C,H,W) view from exactly this tensor).
 */
#ifndef VITCOLMAP_HIP_H_
#define VITCOLMAP_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VC_ABI_VERSION 1

#define VC_OK 0
#define VC_ERR_INVALID_ARG (-1) /* null pointer, negative size, misaligned buffer            */
#define VC_ERR_UNSUPPORTED (-2) /* size outside what the kernels cover (see each function)   */
#define VC_ERR_LAUNCH (-3)      /* hipLaunchKernel reported an error (see vc_last_hip_error) */
#define VC_ERR_WORKSPACE (-4)   /* caller's workspace is too small                           */

#define VC_MAX_KEYPOINTS 2048 /* rows per image the matcher kernels accept                  */
#define VC_MAX_DESC_DIM 1024  /* descriptor bytes per row (255^2 * D must stay below 2^26)  */
#define VC_MAX_NEIGHBOURS 64  /* neighbours per image the retrieval search returns          */

typedef void* vc_stream_t;

int vc_abi_version(void);
const char* vc_status_string(int status);
/* hipError_t of the last failed launch on the calling thread (0 if none). */
int vc_last_hip_error(void);

/* ------------------------------------------------------------------------------------------
 * Matcher — replaces pycolmap.match_exhaustive's per-pair arithmetic
 * (reference call site: vit_colmap/pipeline/run_pipeline.py:351-363; options
 * vit_colmap/utils/config.py:64-96).  Specification: oracle/matcher_oracle.py.
 * ------------------------------------------------------------------------------------------ */

/* Bytes of the MFMA-ready ("prepared") copy of n_images descriptor blocks of n_max x d uint8. */
size_t vc_prepared_bytes(int n_images, int n_max, int d);

/*
 * Re-tile uint8 descriptor blocks for the matcher: desc [n_images][n_max][d] uint8,
 * counts [n_images] int32 (valid rows per image, 0..n_max) -> prepared (vc_prepared_bytes).
 * Rows >= counts[i] are neutralised (similarity 0 with everything).
 * Limits: 1 <= n_max <= VC_MAX_KEYPOINTS, 1 <= d <= VC_MAX_DESC_DIM.
 */
int vc_prepare_descriptors(const uint8_t* desc, const int32_t* counts, int n_images, int n_max,
                           int d, void* prepared, vc_stream_t stream);

/*
 * Match image pairs: for every p < n_pairs, images a = pairs[2p], b = pairs[2p+1]:
 * int32 similarities, per-row and per-column best / second best (lowest index wins ties),
 * angle + ratio tests, optional cross check; writes the matches ordered by row index to
 * out_matches[p][0..out_counts[p]) as (row in a, row in b) uint32 pairs.
 * out_matches: [n_pairs][n_max][2] uint32; out_counts: [n_pairs] int32.
 * out_counts[p] == VC_COUNT_SELFCHECK_FAILED (-1): the persistent kernel's consistency check failed for that pair — the
 * waves of its workgroup disagreed on the tile-ring cursors, which the source makes identical by construction (a
 * toolchain fault of this kind is documented in profiles/r03_matcher_looped_miscompile.md); the pair's list is undefined.
 * Never produced by a correct build: callers treat it as an error (the Python host raises HipLibraryError).
 */
#define VC_COUNT_SELFCHECK_FAILED (-1)
int vc_match_pairs_u8(const void* prepared, const int32_t* counts, int n_images, int n_max, int d,
                      const int32_t* pairs, int n_pairs, float max_ratio, float max_distance,
                      int cross_check, uint32_t* out_matches, int32_t* out_counts,
                      vc_stream_t stream);

/*
 * Guided matching (COLMAP's `guided_matching` option; the build's own published rule, DESIGN.md §4.2e — parity with
 * COLMAP unpinned): vc_match_pairs_u8 on similarities masked by a two-view model.  For pair p, image a = pairs[2p] is
 * image 1.  A candidate (i, j) is admissible iff vc_two_view_inliers would call (keypoint i of a, keypoint j of b) an
 * inlier of models[p] under max_error (VC_MODEL_FUNDAMENTAL: Sampson error, VC_MODEL_HOMOGRAPHY: transfer error from
 * image 1 to image 2; float32 in the same operation order, so a NaN model admits nothing); the similarity of every
 * other candidate is replaced by 0, the value that neither matches nor serves as a runner-up, and the match rule of
 * vc_match_pairs_u8 runs on the result.  Specification: tests/util_guided.py (oracle/matcher_oracle.py on the masked
 * matrix, mask from oracle/two_view_oracle.py inliers_f32).
 *   keypoints_xy  [n_images][n_max][2] float32 (x, y), 8-byte aligned; rows >= counts[image] are ignored
 *   models        [n_pairs][9] float32, row-major
 *   model_kind    [n_pairs] int32: VC_MODEL_FUNDAMENTAL, VC_MODEL_HOMOGRAPHY, or -1: the pair is skipped (count 0)
 * Limits, argument checks and output layout as vc_match_pairs_u8; max_error >= 0.  One workgroup per pair.
 */
int vc_match_pairs_guided_u8(const void* prepared, const int32_t* counts, int n_images, int n_max, int d,
                             const float* keypoints_xy, const int32_t* pairs, int n_pairs, const float* models,
                             const int32_t* model_kind, float max_error, float max_ratio, float max_distance,
                             int cross_check, uint32_t* out_matches, int32_t* out_counts, vc_stream_t stream);

/*
 * One-way search on raw descriptors: for each of the n1 rows of d1, index of the most similar
 * of the n2 rows of d2 (-1 if every similarity is 0), its similarity and the runner-up's.
 * workspace: at least vc_knn_workspace_bytes(n1, n2, d) bytes, 16-byte aligned.
 */
size_t vc_knn_workspace_bytes(int n1, int n2, int d);
int vc_knn_top2_u8(const uint8_t* d1, int n1, const uint8_t* d2, int n2, int d, int32_t* out_idx,
                   int32_t* out_best, int32_t* out_second, void* workspace,
                   size_t workspace_bytes, vc_stream_t stream);

/*
 * Angle / ratio tests and cross check on two one-way results (12 = rows of image 1 against
 * image 2, 21 = the transpose).  out_pairs: [n1][2] uint32, out_count: [1] int32.
 * With cross_check == 0 the *21 pointers may be NULL.
 */
int vc_mutual_ratio(const int32_t* idx12, const int32_t* best12, const int32_t* second12, int n1,
                    const int32_t* idx21, const int32_t* best21, const int32_t* second21, int n2,
                    float max_ratio, float max_distance, int cross_check, uint32_t* out_pairs,
                    int32_t* out_count, vc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Retrieval matching: the two device steps that choose WHICH image pairs are matched, in place
 * of all n (n - 1) / 2 — the build's own published rule (COLMAP's vocabulary-tree matcher and hloc's pairs-from-retrieval
 * play this part there; parity with either is not claimed).  Specification: tests/util_retrieval.py.  All integer, so
 * the neighbour lists equal the specification bit for bit on every device and rank.
 * ------------------------------------------------------------------------------------------ */

/*
 * Pooling: out_sums[i][c] = sum over the rows r < counts[i] of desc[i][r][c], int32 (at most 255 * 2048).
 * desc [n_images][n_max][d] uint8, counts [n_images] int32 (values outside 0..n_max are clamped to it),
 * out_sums [n_images][d] int32, overwritten.  One read of the blocks, several workgroups per image.
 * Limits: 1 <= n_max <= VC_MAX_KEYPOINTS, 1 <= d <= VC_MAX_DESC_DIM (VC_ERR_UNSUPPORTED above).
 */
int vc_pool_descriptors_u8(const uint8_t* desc, const int32_t* counts, int n_images, int n_max, int d,
                           int32_t* out_sums, vc_stream_t stream);

/*
 * Nearest images: score[i][j] = sum over c of q[i][c] q[j][c] in int32 (v_mfma_i32_32x32x32_i8); for every row i with
 * valid[i] != 0 the k best j != i with valid[j] != 0, by score descending, then index ascending.
 *   q          [n][d_pad] int8, 16-byte aligned; d_pad % 32 == 0 (pad the columns with zeros), d_pad <= VC_MAX_DESC_DIM
 *   valid      [n] int32
 *   out_idx    [n][k] int32: the neighbours in rank order; -1 behind the last candidate and in every slot of an invalid row
 *   out_score  [n][k] int32: their scores; INT32_MIN wherever out_idx is -1
 *   workspace  vc_retrieval_workspace_bytes(n, d_pad, k) bytes, 8-byte aligned: at most 16 n k 8-byte keys, never n x n
 *              (VC_ERR_WORKSPACE when shorter; the query returns 0 for a shape the entry refuses)
 * Limits: 1 <= k <= VC_MAX_NEIGHBOURS, n <= 2^20, d_pad <= VC_MAX_DESC_DIM: VC_ERR_UNSUPPORTED beyond.
 */
size_t vc_retrieval_workspace_bytes(int n, int d_pad, int k);
int vc_retrieval_topk_i8(const int8_t* q, const int32_t* valid, int n, int d_pad, int k, int32_t* out_idx,
                         int32_t* out_score, void* workspace, size_t workspace_bytes, vc_stream_t stream);

/* Test hooks: out[s] = theta(s) = angle assigned to integer similarity s, for s in [0, n).
 * vc_theta_table reads the table the pair kernel's acceptance tests use (generated at build time by
 * csrc/gen_theta_table.c, clamped at s = 512^2); vc_theta_eval evaluates the same expression on the device. */
int vc_theta_table(float* out, int n, vc_stream_t stream);
int vc_theta_eval(float* out, int n, vc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Two-view geometric verification, scoring half — the step that follows descriptor matching inside
 * pycolmap.match_exhaustive (reference call site vit_colmap/pipeline/run_pipeline.py:351-363) and fills the
 * two_view_geometries table the reference's metrics read (vit_colmap/utils/metrics.py:207-243).
 * Specification: oracle/two_view_oracle.py.  Hypotheses are produced above the ABI (8x8 linear solves);
 * everything that is O(pairs x hypotheses x matches) runs here.
 *   pts      [total][4] float32 (x1, y1, x2, y2): the matched keypoints of all pairs, concatenated; 16-byte aligned
 *   offsets  [n_pairs + 1] int32: pair p owns pts[offsets[p] .. offsets[p+1])
 *   model    VC_MODEL_FUNDAMENTAL: row-major F, inlier iff (x2' F x1)^2 <= e^2 den, den = |F x1|_xy^2 + |F' x2|_xy^2  (Sampson)
 *            VC_MODEL_HOMOGRAPHY : row-major H, inlier iff |(H x1)_xy - x2 (H x1)_w|^2 <= e^2 (H x1)_w^2      (transfer)
 *            float32 in the specification's operation order; a zero denominator (den, (H x1)_w) or a bound e^2 den,
 *            e^2 (H x1)_w^2 that is not finite has no inlier: F: den > 0 and e^2 den < inf; H: (H x1)_w != 0 and
 *            e^2 (H x1)_w^2 < inf.  NaN compares false.
 * vc_two_view_score:   hypotheses [n_pairs][n_hyp][9] -> out_counts [n_pairs][n_hyp] (NaN hypotheses count 0)
 * vc_two_view_inliers: models [n_pairs][9] -> out_mask [total] uint8
 * ------------------------------------------------------------------------------------------ */
#define VC_MODEL_FUNDAMENTAL 0
#define VC_MODEL_HOMOGRAPHY 1
int vc_two_view_score(const float* pts, const int32_t* offsets, int n_pairs, const float* hypotheses, int n_hyp,
                      int model, float max_error, int32_t* out_counts, vc_stream_t stream);
int vc_two_view_inliers(const float* pts, const int32_t* offsets, int n_pairs, const float* models, int model,
                        float max_error, uint8_t* out_mask, vc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Calibrated two-view geometry, the minimal solver: every real essential matrix E with
 * x2' E x1 = 0 for five correspondences, for n_hyp samples of each of n_pairs image pairs.  float64 throughout.
 * Specification: tests/util_essential.py.
 *   pts_n      [total][4] float64 (x1, y1, x2, y2) in normalised camera coordinates (K^-1 applied), all pairs concatenated
 *   offsets    [n_pairs + 1] int32: pair p owns pts_n[offsets[p] .. offsets[p+1])
 *   samples    [n_pairs][n_hyp][5] int32 indices into the pair's own list; samples[..][0] < 0: the hypothesis is void
 *   out_E      [n_pairs][n_hyp][10][9] float64: row-major 3x3 at unit Frobenius norm, ascending in the solver's root
 *              variable; the slots past out_count are NaN.  A root of magnitude 1 of that variable, where the solver's two
 *              root ranges used to meet, is inside the first range (which ends at 1 + 2^-10) and is returned once.
 *   out_count  [n_pairs][n_hyp] int32: number of real solutions, 0 .. 10.  0 for a void sample, an index outside the
 *              pair's list, a repeated index or point, non-finite points and a singular elimination; a matrix that is
 *              not finite is never counted.
 * Every iterative part runs a bounded number of steps.  n_pairs * n_hyp above 64 * (2^31 - 1): VC_ERR_UNSUPPORTED.
 * ------------------------------------------------------------------------------------------ */
int vc_essential_5pt(const double* pts_n, const int32_t* offsets, int n_pairs, const int32_t* samples, int n_hyp,
                     double* out_E, int32_t* out_count, vc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Two-view relative pose: every inlier of every pair triangulated under each of the pair's
 * (at most four) pose candidates (R, t), X2 = R X1 + t, in one launch.  float64 throughout, in the operation order of the
 * specification tests/util_pose.py, so everything but the angle equals it bit for bit.
 *   pts_n          [total][4] float64 (x1, y1, x2, y2): the pairs' INLIERS in normalised camera coordinates, concatenated
 *   offsets        [n_pairs + 1] int32: pair p owns pts_n[offsets[p] .. offsets[p+1]); any number of inliers per pair
 *   cand           [n_pairs][4][12] float64: R row-major, then t (unit norm); NaN in the first element: unused slot
 *   out_front      [n_pairs][4] int32: points with finite positive depth in both cameras; 0 for an unused slot and for t = 0
 *   out_best       [n_pairs] int32: the slot with most points in front, the lowest on ties
 *   out_tri_angle  [n_pairs] float64: median over the best candidate's in-front points of the angle between the rays to
 *                  the point from the two camera centres (rad; the mean of the two middle values for an even count; 0 for none)
 *   out_points     [total][3] float64 or NULL: the midpoint of each inlier under the best candidate in camera-1 coordinates,
 *                  NaN where it is not in front
 *   workspace      vc_two_view_pose_workspace_bytes(n_pairs, total) bytes, 8-byte aligned: the angle keys of the pairs
 *                  with more than 4096 inliers (smaller pairs keep them in LDS).  NULL only with workspace_bytes 0.  A pair
 *                  whose keys the workspace cannot hold gets out_best -1, out_tri_angle NaN, out_points NaN.
 * ------------------------------------------------------------------------------------------ */
size_t vc_two_view_pose_workspace_bytes(int n_pairs, int total);
int vc_two_view_pose(const double* pts_n, const int32_t* offsets, int n_pairs, const double* cand, int32_t* out_front,
                     int32_t* out_best, double* out_tri_angle, double* out_points, void* workspace, size_t workspace_bytes,
                     vc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Image registration: absolute pose from 2D-3D correspondences, for n_hyp samples of each of
 * n_prob registration problems (one problem: one image against the model's points).  Specification:
 * tests/util_absolute_pose.py.
 *   offsets    [n_prob + 1] int32: problem p owns rows offsets[p] .. offsets[p+1]) of the per-correspondence arrays
 * vc_p3p — the minimal solver, float64 throughout: every pose (R, t), X_cam = R X + t, that maps three world points onto
 * their three image rays with positive depths.
 *   rays_n     [total][2] float64: the image points in normalised camera coordinates (K^-1 applied)
 *   xyz        [total][3] float64: the world points
 *   samples    [n_prob][n_hyp][3] int32 indices into the problem's own list; samples[..][0] < 0: the hypothesis is void
 *   out_pose   [n_prob][n_hyp][4][12] float64: R row-major then t, ascending in the solver's root variable (the depth
 *              ratio s2 / s1 along the unit rays of the sample's second and first point); the slots past out_count are NaN.
 *              At most four DISTINCT poses.  Two geometries that used to lose poses are solved: two points equally far from
 *              the camera (s2 / s1 = 1, on the seam of the solver's two root ranges: the first now ends at 1 + 2^-10, the
 *              pose is returned once), and a third ray perpendicular to the side between the first two points in the camera
 *              frame (two poses share s2 / s1, a double root: the solver then eliminates under another labelling of the
 *              three points and sorts the poses back into this order).
 *   out_count  [n_prob][n_hyp] int32: 0 .. 4.  0 for a void sample, an index outside the problem's list, a repeated index,
 *              two coincident world points or rays, collinear world points, non-finite input and a quartic without a
 *              finite non-zero coefficient; a pose that is not finite and proper (|det R - 1| < 1e-9) is never counted.
 * Every iterative part runs a bounded number of steps.  n_prob * n_hyp above 64 * (2^31 - 1): VC_ERR_UNSUPPORTED.
 * vc_absolute_pose_score / vc_absolute_pose_inliers — float32, no division, in the specification's operation order:
 * p = P (X, 1); inlier iff p_w > 0 and |p_xy - obs p_w|^2 <= max_error^2 p_w^2.
 *   obs        [total][2] float32 pixels, 8-byte aligned
 *   xyz4       [total][4] float32 world points, w ignored, 16-byte aligned
 *   hyp        [n_prob][n_hyp][12] float32: row-major 3x4 pixel projection matrices P = K [R | t] -> out_counts
 *              [n_prob][n_hyp] (a NaN hypothesis counts 0).  n_prob above 65535 * 32: VC_ERR_UNSUPPORTED.
 *   models     [n_prob][12] -> out_mask [total] uint8
 * ------------------------------------------------------------------------------------------ */
int vc_p3p(const double* rays_n, const double* xyz, const int32_t* offsets, int n_prob, const int32_t* samples, int n_hyp,
           double* out_pose, int32_t* out_count, vc_stream_t stream);
int vc_absolute_pose_score(const float* obs, const float* xyz4, const int32_t* offsets, int n_prob, const float* hyp, int n_hyp,
                           float max_error, int32_t* out_counts, vc_stream_t stream);
int vc_absolute_pose_inliers(const float* obs, const float* xyz4, const int32_t* offsets, int n_prob, const float* models,
                             float max_error, uint8_t* out_mask, vc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Track triangulation: one 3D point per track of observations under known camera poses, every
 * track in one launch, one track per lane, float64 in single operations in the specification's order
 * (tests/util_mapper.py; the only library call is sqrt).  This build's own published rule: parity with COLMAP's triangulator
 * is unpinned.
 *   obs_xy     [total][2] float64 pixels
 *   obs_cam    [total] int32: the observation's slot into cams
 *   offsets    [n_tracks + 1] int32: track t owns rows offsets[t] .. offsets[t+1]) of the per-observation arrays, in any
 *              order and of any length; a negative or descending pair of offsets rejects the track and nothing of it is read
 *   cams       [n_cams][16] float64: R row-major (9), t (3), fx, fy, cx, cy; X_cam = R X + t.  A row with a non-finite entry is
 *              an image that is not registered.  NULL only with n_cams 0
 *   seeds      [n_tracks] int32, read as 32 unsigned bits: the sampler's seed of a track of 12 or more observations
 *   max_error_px, min_tri_angle_tan2   the inlier threshold and tan^2 of the least angle between two rays at the point
 *   out_xyz    [n_tracks][3] float64, NaN where the track is rejected
 *   out_mask   [total] uint8: the inlier observations; a track writes its own rows only, 0 where it is rejected
 *   out_count  [n_tracks] int32: the inliers, 0 where rejected
 *   out_error  [n_tracks] float64: the mean pixel error of the inliers, NaN where rejected
 * The rule for a track of n observations:
 *   usable      an observation whose slot is in [0, n_cams), whose camera row and pixel are finite; any other is never an
 *               inlier and never part of a hypothesis
 *   hypotheses  pairs (p, q), p < q, of observation indices: all in lexicographic order while n (n - 1) / 2 <= 64; otherwise
 *               64 pairs, p = lowbias32(seed * 0x9E3779B1 + h * 0x85EBCA6B + 0xC3C3C3C3) mod n,
 *               q = (p + 1 + lowbias32(the same argument + 0xC2B2AE35) mod (n - 1)) mod n, swapped so that p < q (32-bit)
 *   one of them the midpoint of the rays c + s d, d = R' ((u - cx) / fx, (v - cy) / fy, 1), c = -R' t, valid iff both depths
 *               s, r are finite and positive and the parallax test passes at X for the two centres: with g = X - c_p,
 *               h = X - c_q, g.h <= 0 or |g x h|^2 >= min_tri_angle_tan2 (g.h)^2
 *   inlier      Xc = R X + t; Xc_z > 0 and (fx Xc_x + cx Xc_z - u Xc_z)^2 + (fy Xc_y + cy Xc_z - v Xc_z)^2 <= e^2 Xc_z^2; a
 *               hypothesis counts only if p and q are inliers; most inliers win, the lowest index on ties
 *   refit       at most 10 Gauss-Newton steps on X over the winner's inliers (3x3 normal equations by the adjugate), a step
 *               kept only if it lowers the cost, the first one not kept ends it; taken iff finite with no fewer inliers
 *   accepted    at least two inliers, some pair of which passes the parallax test at the final X
 * n_tracks == 0: VC_OK whatever the pointers are.  A null pointer, a negative size, a threshold that is negative or not
 * finite: VC_ERR_INVALID_ARG.
 * ------------------------------------------------------------------------------------------ */
int vc_triangulate_tracks(const double* obs_xy, const int32_t* obs_cam, const int32_t* offsets, int n_tracks, const double* cams,
                          int n_cams, const int32_t* seeds, double max_error_px, double min_tri_angle_tan2, double* out_xyz,
                          uint8_t* out_mask, int32_t* out_count, double* out_error, vc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Track refinement: every track of a call evaluated again at a point it already has, after the
 * poses moved (one bundle adjustment per growth round).  The arrays, the thresholds, the outputs, the launch shape and the
 * arithmetic are vc_triangulate_tracks'; init_xyz [n_tracks][3] float64 takes the place of the seeds and of the hypotheses.
 * Specification: tests/util_rounds.py (`refine_track`).  The rule for a track:
 *   usable      as above; an init_xyz with a non-finite entry rejects the track
 *   start       the inliers of X0 = init_xyz over every usable observation (the inlier test above); fewer than two reject
 *   refit       as above, from X0 over those inliers; taken iff finite with no fewer inliers over all usable observations
 *   accepted    as above; out_mask are the inliers of the final X: observations that left the threshold are dropped, nodes
 *               that are now inside it are picked up
 * n_tracks == 0: VC_OK whatever the pointers are.  A null pointer, a negative size, a threshold that is negative or not
 * finite: VC_ERR_INVALID_ARG.  A negative or descending pair of offsets rejects the track and nothing of it is read.
 * ------------------------------------------------------------------------------------------ */
int vc_refine_tracks(const double* obs_xy, const int32_t* obs_cam, const int32_t* offsets, int n_tracks, const double* cams, int n_cams,
                     const double* init_xyz, double max_error_px, double min_tri_angle_tan2, double* out_xyz, uint8_t* out_mask,
                     int32_t* out_count, double* out_error, vc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Track splitting: a component of the match graph that holds more than one scene point (two of
 * its nodes lie in one image) is split into up to max_points points, every component of a call in one launch, one component
 * per lane.  Arrays, thresholds, launch shape and arithmetic (usable, midpoint, parallax test, inlier test, refit) are
 * vc_triangulate_tracks'.  Specification: tests/util_split.py (`split_component`).  This build's own published rule: parity
 * with COLMAP's recursive triangulation is unpinned.
 *   obs_xy, obs_cam, cams, n_cams, max_error_px, min_tri_angle_tan2   as vc_triangulate_tracks has them, a row per node
 *   offsets     [n_comps + 1] int32: component t owns rows offsets[t] .. offsets[t+1]) of the per-node arrays.  The caller
 *               sorts the nodes of a component by (image, keypoint), so that the nodes of one image are adjacent
 *   seeds       [n_comps] int32, read as 32 unsigned bits
 *   max_points  in [1, VC_SPLIT_MAX_POINTS]: the slots of every component
 *   node_point  [total] int32, in and out: -1 a free node; k in [0, max_points) a node of slot k; any other value a node that
 *               is never free, belongs to no slot and is never written
 *   points_xyz  [n_comps][max_points][3] float64, in and out: a slot is occupied iff its three numbers are finite
 *   out_count   [n_comps][max_points] int32: the nodes that carry each slot after the call
 *   out_new     [n_comps][max_points] uint8: 1 for a slot this call created
 *   out_error   [n_comps][max_points] float64: the mean pixel error of the nodes of a slot this call created, NaN otherwise
 * The rule for a component of n nodes:
 *   run         a maximal stretch of adjacent nodes with equal obs_cam
 *   selection   under a point X, for slot k: in every run that holds no node of slot k, among its free usable nodes that
 *               pass the inlier test at X the one with the smallest sq = (..)^2 + (..)^2 of that test (one camera row and
 *               hence one Xc_z per run: the smallest pixel error), the lowest index on ties.  With runs of length 1 it is
 *               the inlier set
 *   attach      every slot k occupied on input, in ascending order: the nodes selected under X_k take label k; X_k stays
 *   peel        every slot k empty on input, in ascending order: hypotheses are the pairs of vc_triangulate_tracks over all n
 *               nodes under the seed seed + k * 0x9E3779B9 (32-bit), tried only if p and q are free, usable and of
 *               different obs_cam; one counts iff its midpoint is valid and p and q are in the selection under it, its score
 *               is the size of that selection, the largest wins, the lowest index on ties; the refit of
 *               vc_triangulate_tracks over the winner's selection, taken iff finite with no smaller a selection; accepted
 *               iff at least two nodes are selected, some pair of which passes the parallax test at the final X.  Accepted:
 *               the selected nodes take label k, points_xyz[k] = X.  Rejected: the slot stays empty and no later slot is tried
 * n_comps == 0: VC_OK whatever the pointers are.  A null pointer, a negative size, a max_points outside [1, 4], a threshold
 * that is negative or not finite: VC_ERR_INVALID_ARG without a launch.  A negative or descending pair of offsets rejects the
 * component: nothing of it is read, its labels and points stay, its outputs are 0 / 0 / NaN.  Offsets past the arrays are the
 * caller's to exclude, as for vc_triangulate_tracks: the call is not told their length.
 * ------------------------------------------------------------------------------------------ */
#define VC_SPLIT_MAX_POINTS 4
int vc_split_tracks(const double* obs_xy, const int32_t* obs_cam, const int32_t* offsets, int n_comps, const double* cams, int n_cams,
                    const int32_t* seeds, int max_points, double max_error_px, double min_tri_angle_tan2, int32_t* node_point,
                    double* points_xyz, int32_t* out_count, uint8_t* out_new, double* out_error, vc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Keypoint undistortion: the pixel an ideal pinhole camera with the same K would see in place of
 * a raw keypoint of a camera with known distortion, one keypoint per lane, float64 in single operations in the written order
 * (left to right, the usual precedence; no fused multiply-add, no library call).  Specification: tests/util_undistort.py.
 *   xy         [n][2] float32: raw pixel keypoints as the database holds them
 *   cam        [n] int32: the keypoint's slot into cams
 *   cams       [n_cams][8] float64: fx, fy, cx, cy, k1, k2, p1, p2, COLMAP's OPENCV parameterisation; SIMPLE_RADIAL and RADIAL
 *              are the cases p1 = p2 = 0, SIMPLE_RADIAL also k2 = 0
 *   out_xy     [n][2] float64: (fx x + cx, fy y + cy) with (x, y) the undistorted normalised point; NaN where invalid
 *   out_valid  [n] uint8: 1 where the iteration stopped, else 0
 * The rule for a keypoint (u, v), every value float64:
 *   start      xd = (u - cx) / fx, yd = (v - cy) / fy, (x, y) = (xd, yd)
 *   iterate    rho = x x + y y, s = 1 + k1 rho + k2 rho rho, e = 2 (k1 + 2 k2 rho)
 *              gx = x s + 2 p1 x y + p2 (rho + 2 x x) - xd, gy = y s + p1 (rho + 2 y y) + 2 p2 x y - yd
 *              a = s + x x e + 2 p1 y + 6 p2 x, b = x y e + 2 p1 x + 2 p2 y, d = s + y y e + 6 p1 y + 2 p2 x
 *              det = a d - b b; not det > 0 (NaN included) at any iterate: the keypoint is invalid
 *   step       sx = (d gx - b gy) / det, sy = (a gy - b gx) / det, x = x - sx, y = y - sy
 *   stop       valid once sx sx + sy sy <= 1e-24, within at most 20 steps (a bound: 12 were the most met); invalid otherwise
 * With every distortion parameter zero the first step is exactly 0 and out_xy = fx ((u - cx) / fx) + cx.
 * n == 0: VC_OK whatever the pointers are, nothing launched.  A null pointer, a negative size, n_cams == 0 with n > 0, or
 * a slot of cam outside [0, n_cams): VC_ERR_INVALID_ARG, nothing written.  The slots are device data, so this entry point,
 * unlike the others, waits for the stream once (a one-flag check kernel) before the launch that writes.
 * ------------------------------------------------------------------------------------------ */
int vc_undistort_points(const float* xy, const int32_t* cam, int n, const double* cams, int n_cams, double* out_xy,
                        uint8_t* out_valid, vc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Focal length from the verified pairs: the self-calibration cost of Mendonca and Cipolla.  For a
 * camera that is the same in both images of a pair K' F K is an essential matrix, whose two non-zero singular values are
 * equal; the call returns, per camera and candidate scale r on its stored focal length(s), the weighted mean over the
 * camera's pairs of (s1 - s2) / (s1 + s2).  float64 in single operations in the written order (left to right, the usual
 * precedence; no fused multiply-add), the only library call is sqrt, no atomics: two calls return the same bytes.  The grid
 * search is the caller's (vit_colmap_amd/matching/focal.py).  Specification: tests/util_focal.py.  This build's own published
 * rule: parity with COLMAP is unpinned.
 *   F          [n_pairs][9] float64: the stored fundamental matrix, row-major, x2' F x1 = 0 in pixels
 *   pair_cam   [n_pairs] int32: the pair's slot into cams, -1 for a pair that is not used; a slot outside [-1, n_cams) is
 *              treated as -1 (it is checked before it indexes anything)
 *   w          [n_pairs] float64: the pair's weight (its number of inlier matches); a weight that is not finite and positive
 *              makes the pair not count
 *   cams       [n_cams][4] float64: fx0, fy0, cx, cy as the database stores them
 *   ratios     [n_cand] float64: the candidates r; the camera is tried at (r fx0, r fy0)
 *   out_cost   [n_cams][n_cand] float64: J[c][k]; NaN in the column of a ratio that is not finite and positive and in the row
 *              of a camera without weight (0 / 0); every NaN written is the one of the NAN macro
 *   out_weight [n_cams] float64: the sum of the weights of the camera's pairs that count
 * The rule, every value float64:
 *   per pair   g = F T, a = T' g with T = [[1, 0, cx], [0, 1, cy], [0, 0, 1]]: g_i2 = f_i0 cx + f_i1 cy + f_i2,
 *              a_2j = cx g_0j + cy g_1j + g_2j, the other entries copied; n2 = the sum of a_ij a_ij, row-major from 0;
 *              a = a / sqrt(n2); a norm that is 0 or not finite: the pair does not count
 *   candidate  d = (r fx0, r fy0, 1), e_ij = (d_i a_ij) d_j; c2 = the sum of e_ij e_ij, row-major from 0;
 *              m_ij = e_0i e_0j + e_1i e_1j + e_2i e_2j, m2 = the sum of m_ij m_ij, row-major from 0; c1 = (c2 c2 - m2) 0.5
 *              disc = c2 c2 - 4 c1, 0 where that is not > 0; l1 = (c2 + sqrt(disc)) 0.5; l2 = c1 / l1, 0 where that is not > 0
 *              cost = (sqrt(l1) - sqrt(l2)) / (sqrt(l1) + sqrt(l2))
 *   sums       per camera and candidate the terms w cost, and per camera the weights w, of the pairs that count: within a chunk
 *              of 256 consecutive pairs of the call added from 0 in pair order, the chunk sums added from 0 in chunk order;
 *              J = the sum of the terms / the sum of the weights
 * n_pairs == 0 or n_cand == 0: VC_OK whatever the pointers are, nothing launched, nothing written.  A negative size, or a null
 * pointer that a size needs (F, pair_cam, w, ratios; with n_cams > 0 also cams, out_cost, out_weight): VC_ERR_INVALID_ARG,
 * nothing launched.  n_cand above 16 * 65535: VC_ERR_UNSUPPORTED.  The partial sums, ceil(n_pairs / 256) * n_cams * (n_cand + 1)
 * float64, are allocated on the stream; above 1 GiB: VC_ERR_WORKSPACE.
 * ------------------------------------------------------------------------------------------ */
int vc_focal_cost(const double* F, const int32_t* pair_cam, const double* w, int n_pairs, const double* cams, int n_cams,
                  const double* ratios, int n_cand, double* out_cost, double* out_weight, vc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Bundle adjustment: the three steps of one Levenberg-Marquardt iteration over every pose and
 * every point, by the Schur complement of the points; float64 in single operations in the written order, the only library
 * call is sqrt, no atomics: two calls return the same bytes.  The caller solves S dc = -g between the last two and runs the
 * loop (vit_colmap_amd/mapping/bundle.py).  Specification: tests/util_bundle.py.  This build's own published rule: parity
 * with COLMAP / Ceres is unpinned.  These three never refine an intrinsic (the border below does); the loss is the plain
 * squared pixel error.
 *   cams        [n_cams][16] float64 as vc_triangulate_tracks has them: R row-major, t, fx, fy, cx, cy
 *   const_mask  [n_cams] uint8: bit i set = pose parameter i is held (0-2 the rotation w, 3-5 the translation)
 *   points      [n_points][3] float64
 *   offsets     [n_points + 1] int32, obs_cam [total] int32, obs_xy [total][2] float64: the point-major tracks of
 *               vc_triangulate_tracks.  Offsets that are negative, descend or pass total: the point is skipped, nothing of it
 *               is read, its outputs are 0 (its candidate is the point itself)
 *   cam_offsets [n_cams + 1] int32, cam_obs [total] int32: per camera the indices of its observations in ascending order;
 *               obs_point [total] int32: the point of each observation.  Offsets that are negative, descend or pass total:
 *               the camera is skipped (its block is that of a camera without observations).  An entry of cam_obs that is no
 *               usable observation of that camera inside its point's track is passed over
 *   lambda      the damping, finite and not negative
 * The rule, per observation of point X in camera (R, t):
 *   usable      rule 1 of vc_triangulate_tracks (slot in [0, n_cams), finite row and pixel) and Xc_z > 0; any other observation
 *               contributes nothing anywhere (obs_ok 0, obs_lin 0)
 *   residual    Y = R X, Xc = Y + t, r = (fx Xc_x / Xc_z + cx - u, fy Xc_y / Xc_z + cy - v)
 *   J_p         fu (R_0k - xu R_2k), fv (R_1k - xv R_2k) with fu = fx / z, fv = fy / z, xu = Xc_x / z, xv = Xc_y / z
 *   J_c         the pose perturbed on the left, Xc(w, dt) = Rot(w) Y + t + dt: J_pi [ -[Y]x | I ], row u = (-(au Y_1),
 *               fu Y_2 + au Y_0, -(fu Y_1), fu, 0, -au), row v = (-(fv Y_2 + av Y_1), av Y_0, fv Y_0, 0, fv, -av), au = fu xu,
 *               av = fv xv; the columns of held parameters are 0
 *   obs_lin     [total][32]: J_c row u (6), row v (6), r (2), W = J_c' J_p row-major (18)
 * vc_ba_linearize_points: per point in track order V = sum J_p' J_p, g_p = sum J_p' r, cost = 0.5 sum |r|^2; V_ii += lambda
 * V_ii; V^-1 by the adjugate, stored 00 01 02 11 12 22.  A point with fewer than two usable observations, or whose damped V
 * has a determinant that is not finite and positive, is constant for this linearisation: V^-1 = 0.  out_total_cost [1]: the
 * costs added in point order (a second launch of one wave).
 * vc_ba_reduce_cameras: out_S [6 n_cams][6 n_cams] row-major, out_g [6 n_cams].  Per camera a over its observations in
 * ascending order: U_a = sum J_c' J_c; Y = W V^-1; g_a = sum J_c' r - sum Y g_p; S_ab = delta_ab U_a - sum Y W_b' over the
 * track of the observation's point in track order (b = a and a camera twice in a track included); U_ii += lambda U_ii.  A held
 * parameter, or one with U_ii = 0 (no usable observation moves it), has the diagonal 1 and zero rows and columns.  One
 * workgroup per camera, entry e of block b owned by lane (36 b + e) mod 64, the row block in LDS: n_cams <= VC_BA_MAX_CAMS
 * (the CU's 160 KiB of LDS bind before the dense S does), VC_ERR_UNSUPPORTED above.
 * vc_ba_step: dc [6 n_cams] the solution of S dc = -g.  out_dx = -V^-1 (g_p + sum W' dc) over the track in track order,
 * out_points = points + out_dx; out_cams: q = (1, w / 2) / |(1, w / 2)|, R(q) R, t + dt, the intrinsics copied.
 * A size of 0 (n_points for the first, n_cams for the second, both for the third): VC_OK whatever the pointers are.  A null
 * pointer that a size needs, a negative size, a lambda that is negative or not finite: VC_ERR_INVALID_ARG.
 * ------------------------------------------------------------------------------------------ */
#define VC_BA_MAX_CAMS 512
int vc_ba_linearize_points(const double* cams, int n_cams, const uint8_t* const_mask, const double* points, int n_points,
                           const int32_t* offsets, const int32_t* obs_cam, const double* obs_xy, int total, double lambda,
                           double* out_vinv, double* out_gp, double* out_cost, int32_t* out_count, uint8_t* out_obs_ok,
                           double* out_obs_lin, double* out_total_cost, vc_stream_t stream);
int vc_ba_reduce_cameras(int n_cams, const uint8_t* const_mask, int n_points, const int32_t* offsets, const int32_t* obs_cam, int total,
                         const int32_t* cam_offsets, const int32_t* cam_obs, const int32_t* obs_point, double lambda,
                         const double* vinv, const double* gp, const uint8_t* obs_ok, const double* obs_lin, double* out_S,
                         double* out_g, vc_stream_t stream);
int vc_ba_step(const double* cams, int n_cams, const double* points, int n_points, const int32_t* offsets, const int32_t* obs_cam,
               int total, const double* vinv, const double* gp, const uint8_t* obs_ok, const double* obs_lin, const double* dc,
               double* out_cams, double* out_points, double* out_dx, vc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Bundle adjustment without the dense S ("The solver"): what preconditioned conjugate gradients on
 * S dc = -g need, for any number of cameras.  Both entry points take the index arrays and the outputs of vc_ba_linearize_points
 * (or of vc_ba_linearize_points_loss, as they are) exactly as vc_ba_reduce_cameras does; same arithmetic conventions, no
 * atomics, every sum has one owner lane and runs in list order: two calls return the same bytes.  Specification:
 * tests/util_bundle_pcg.py.
 * vc_ba_camera_blocks, per camera a over its observations in ascending order (one wave per camera):
 *   out_U     [n_cams][36]  U_a = sum J_c' J_c, U_ii += lambda U_ii
 *   out_g     [6 n_cams]    g_a = sum J_c' r - sum Y g_p, Y = W V^-1: the bytes of vc_ba_reduce_cameras' out_g
 *   out_D     [n_cams][36]  D_a = S_aa = U_a - sum Y W_a' over the elements of the point's track whose camera is a, in track
 *                           order (the observation itself and a camera twice in a track included): the bytes of the diagonal
 *                           block of vc_ba_reduce_cameras' out_S
 *   out_fixed [6 n_cams]    uint8, 1 where the parameter is held or its undamped U_ii is 0: there the diagonal of U_a and D_a is 1
 *                           (rows and columns are 0, as no usable observation moves it) and g is 0
 *   out_Minv  [n_cams][36]  D_a^-1 column by column: D = L L' by rows, L y = e_k, L' x = y, every sum subtracted from its first
 *                           term left to right; the identity where a pivot is not finite and positive
 * vc_ba_schur_product: out_q [6 n_cams] = S p without S, two launches.  Entries of p at fixed parameters are read as 0.
 *   points    one point per lane, track order: s_j = V_j^-1 (sum over usable observations W_o' p_cam(o)) into workspace_s
 *             [n_points][3]; 0 for a constant point and for a point whose offsets delimit nothing
 *   cameras   one workgroup per camera over its list in ascending order: q_a = U_a p_a - sum W_o s_point(o), the row of U_a left
 *             to right; q_i = p_i at a fixed parameter.  U and fixed are vc_ba_camera_blocks' (U carries the damping).
 * This equals out_S p of vc_ba_reduce_cameras up to rounding (the sum is associated differently).  No limit on n_cams.
 * n_cams = 0: VC_OK whatever the pointers are.  A null pointer that a size needs, a negative size, for vc_ba_camera_blocks a
 * lambda that is negative or not finite: VC_ERR_INVALID_ARG, nothing is launched.  Offsets that are negative, descend or pass
 * total skip their point or camera as above (a skipped camera has the blocks of one without observations); every index is checked.
 * ------------------------------------------------------------------------------------------ */
int vc_ba_camera_blocks(int n_cams, const uint8_t* const_mask, int n_points, const int32_t* offsets, const int32_t* obs_cam, int total,
                        const int32_t* cam_offsets, const int32_t* cam_obs, const int32_t* obs_point, double lambda, const double* vinv,
                        const double* gp, const uint8_t* obs_ok, const double* obs_lin, double* out_U, double* out_D, double* out_Minv,
                        double* out_g, uint8_t* out_fixed, vc_stream_t stream);
int vc_ba_schur_product(int n_cams, int n_points, const int32_t* offsets, const int32_t* obs_cam, int total, const int32_t* cam_offsets,
                        const int32_t* cam_obs, const int32_t* obs_point, const double* vinv, const uint8_t* obs_ok, const double* obs_lin,
                        const double* U, const uint8_t* fixed, const double* p, double* workspace_s, double* out_q, vc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Bundle adjustment with refined intrinsics ("The border"): the three entry points above never move
 * an intrinsic; these three add theta_g = (fx, fy, cx, cy) of every group of cameras as a border of the reduced system,
 *   [[S, B], [B', C]] (dc, dtheta) = -(g, h),  S and g from vc_ba_reduce_cameras unchanged,
 * which the caller assembles and solves.  Same arithmetic conventions; no atomics, every sum has one owner and the written
 * order, two calls return the same bytes.  Specification: tests/util_bundle_intr.py.  This build's own rule, parity unpinned.
 *   cam_group   [n_cams] int32: the group of each camera slot; outside [0, n_groups): the slot's intrinsics are held
 *   intr_mask   [n_groups] uint8: bits 0-3 set = fx, fy, cx, cy held; bit 4 = tied: fx and fy are one parameter, column 0 of
 *               J_theta is d r / d fx + d r / d fy, parameter 1 counts as held, the step of parameter 0 goes to both
 *   vinv, gp, obs_ok, obs_lin: what vc_ba_linearize_points wrote for the same parameters and damping
 * Per usable observation (obs_ok set, slot in the table): x = Xc_x / Xc_z, y = Xc_y / Xc_z, J_theta = [[x, 0, 1, 0],
 * [0, y, 0, 1]], held columns 0; tied: column 0 = (x, y), column 1 = 0.
 * vc_ba_linearize_intrinsics (one point per lane, the groups outside, the track inside):
 *   out_obs_xn [total][2]   (x, y) of a usable observation, 0 otherwise
 *   out_T      [n_points][n_groups][12]   T_jg = sum J_theta' J_p (4x3 row-major) over the group's observations in track order
 *   out_terms  [24 G + 16 G^2][n_points], G = n_groups, entry-major: rows 16 g + 4 i + k: q_jg = sum J_theta' J_theta; 16 G + 4 g
 *              + i: hq_jg = sum J_theta' r; 20 G + 4 g + i: T_jg V_j^-1 g_pj; 24 G + 16 (g G + g') + 4 i + k: T_jg V_j^-1 T_jg''
 *              (T V^-1 formed first, as Y = W V^-1 is).  A skipped point has T and its terms 0.
 * vc_ba_reduce_border:
 *   out_sums   [24 G + 16 G^2]: every row of the terms added over the points in ascending order (one wave per row, the total
 *              cost's scheme)
 *   out_C      [4 G][4 G], out_h [4 G]: Q_g = sum_j q_jg with Q_ii += lambda Q_ii; C_gg' = delta_gg' Q_g - sum_j T V^-1 T';
 *              h_g = sum_j hq_jg - sum_j T V^-1 g_p (the two sums kept apart).  A held parameter, parameter 1 of a tied group
 *              and one with Q_ii = 0 have the diagonal 1, zero rows and columns, h = 0 and out_free [4 G] uint8 = 0
 *   out_B      [6 n_cams][4 G]: per camera a over cam_obs in ascending order B_ag = sum [g = g(a)] J_c' J_theta - sum Y T_j(o)g',
 *              Y = W V^-1 as vc_ba_reduce_cameras forms it, the two sums kept apart; one wave per camera, entry 24 g + 4 r + i
 *              of the row block owned by lane (24 g + 4 r + i) mod 64 in a register
 * vc_ba_step_intrinsics: dtheta [4 G] (a parameter that does not move: 0).  out_dx = -V^-1 (g_p + sum W' dc + sum_g T_jg'
 * dtheta_g), the cameras in track order, then the groups ascending; out_cams: vc_ba_step's pose update, then (fx, fy, cx, cy)
 * += dtheta of the slot's group (tied: dtheta_0 to fx and fy); out_valid [n_cams] uint8: 0 where the slot's group is in
 * [0, n_groups) and its new fx or fy is not finite or not positive (the loop rejects such a candidate).
 * n_groups <= VC_BA_MAX_GROUPS (a lane of the B pass keeps ceil(24 G / 64) = 3 entries in registers and the terms grow with
 * 16 G^2 numbers per point), VC_ERR_UNSUPPORTED above; vc_ba_reduce_border also above VC_BA_MAX_CAMS.  A size of 0 (n_points or
 * n_groups for the first, n_groups for the second, n_cams and n_points for the third): VC_OK.  A null pointer that a size
 * needs, a negative size, a bad lambda: VC_ERR_INVALID_ARG without a launch.  Offsets as above; every index is checked.
 * ------------------------------------------------------------------------------------------ */
#define VC_BA_MAX_GROUPS 8
int vc_ba_linearize_intrinsics(const double* cams, int n_cams, const int32_t* cam_group, int n_groups, const uint8_t* intr_mask,
                               const double* points, int n_points, const int32_t* offsets, const int32_t* obs_cam, int total,
                               const double* vinv, const double* gp, const uint8_t* obs_ok, const double* obs_lin, double* out_obs_xn,
                               double* out_T, double* out_terms, vc_stream_t stream);
int vc_ba_reduce_border(int n_cams, const int32_t* cam_group, int n_groups, const uint8_t* intr_mask, int n_points, const int32_t* offsets,
                        const int32_t* obs_cam, int total, const int32_t* cam_offsets, const int32_t* cam_obs, const int32_t* obs_point,
                        double lambda, const double* vinv, const uint8_t* obs_ok, const double* obs_lin, const double* obs_xn,
                        const double* T, const double* terms, double* out_sums, double* out_B, double* out_C, double* out_h,
                        uint8_t* out_free, vc_stream_t stream);
int vc_ba_step_intrinsics(const double* cams, int n_cams, const int32_t* cam_group, int n_groups, const uint8_t* intr_mask,
                          const double* points, int n_points, const int32_t* offsets, const int32_t* obs_cam, int total, const double* vinv,
                          const double* gp, const uint8_t* obs_ok, const double* obs_lin, const double* T, const double* dc,
                          const double* dtheta, double* out_cams, double* out_points, double* out_dx, uint8_t* out_valid,
                          vc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Bundle adjustment under a robust loss ("The loss"): iteratively reweighted Gauss-Newton.  This
 * build's own published rule; parity with Ceres' loss functions is unpinned.  For a usable observation with the unweighted
 * residual r = (ru, rv) let s = ru ru + rv rv and c = loss_scale (px); float64, single operations in the written order, sqrt the
 * only library call:
 *   VC_BA_LOSS_TRIVIAL   rho = s, w = 1
 *   VC_BA_LOSS_HUBER     s <= c c: rho = s, w = 1; otherwise q = sqrt(s), rho = (2 c) q - c c, w = c / q
 *   VC_BA_LOSS_SOFT_L1   q = sqrt(1 + s / (c c)), rho = 2 s / (1 + q), w = 1 / q   (= 2 c^2 (q - 1) without its cancellation)
 * sw = sqrt(w).  The observation's rows of J_c and of J_p and r are each multiplied by sw (a held column of J_c stays exactly 0)
 * before anything is formed from them; W, V, g_p, U, S, g, the border's T, q, hq, B, C, h and the steps are the arithmetic
 * above on the scaled values, so the gradient (sw J)' (sw r) = rho' J' r is exact and the loss' second-order term is dropped
 * (the system stays positive semidefinite).  cost_j = 0.5 sum rho in track order.  With w = 1 every product is exact: the
 * trivial loss returns the bytes of the entry point without a loss.  A residual whose s overflows takes what this arithmetic
 * gives (w = 0, a cost that is not finite: the loop rejects the candidate); Cauchy is not offered: its cost needs log.
 *
 * vc_ba_linearize_points_loss: vc_ba_linearize_points with loss, loss_scale and out_obs_w [total]: sw of a usable observation, 0
 * of any other of a track (observations outside every track are not written).  out_obs_lin holds the scaled J_c, r and W, so
 * vc_ba_reduce_cameras, vc_ba_step and vc_ba_step_intrinsics are called on its outputs as they are.
 * vc_ba_linearize_intrinsics_loss, vc_ba_reduce_border_loss: the two entry points above with obs_w [total] as the points pass
 * wrote it; the recomputed J_p and every column of J_theta (the constant 1 of cx, cy too) are multiplied by obs_w[o];
 * out_obs_xn stays the unscaled (x, y).
 * A loss outside 0-2, a loss_scale that is not finite or not positive, a null out_obs_w / obs_w that total needs:
 * VC_ERR_INVALID_ARG without a launch; everything else as the entry points without a loss.
 * ------------------------------------------------------------------------------------------ */
#define VC_BA_LOSS_TRIVIAL 0
#define VC_BA_LOSS_HUBER 1
#define VC_BA_LOSS_SOFT_L1 2
int vc_ba_linearize_points_loss(const double* cams, int n_cams, const uint8_t* const_mask, const double* points, int n_points,
                                const int32_t* offsets, const int32_t* obs_cam, const double* obs_xy, int total, double lambda, int loss,
                                double loss_scale, double* out_vinv, double* out_gp, double* out_cost, int32_t* out_count,
                                uint8_t* out_obs_ok, double* out_obs_lin, double* out_obs_w, double* out_total_cost, vc_stream_t stream);
int vc_ba_linearize_intrinsics_loss(const double* cams, int n_cams, const int32_t* cam_group, int n_groups, const uint8_t* intr_mask,
                                    const double* points, int n_points, const int32_t* offsets, const int32_t* obs_cam, int total,
                                    const double* vinv, const double* gp, const uint8_t* obs_ok, const double* obs_lin, const double* obs_w,
                                    double* out_obs_xn, double* out_T, double* out_terms, vc_stream_t stream);
int vc_ba_reduce_border_loss(int n_cams, const int32_t* cam_group, int n_groups, const uint8_t* intr_mask, int n_points, const int32_t* offsets,
                             const int32_t* obs_cam, int total, const int32_t* cam_offsets, const int32_t* cam_obs, const int32_t* obs_point,
                             double lambda, const double* vinv, const uint8_t* obs_ok, const double* obs_lin, const double* obs_xn,
                             const double* obs_w, const double* T, const double* terms, double* out_sums, double* out_B, double* out_C,
                             double* out_h, uint8_t* out_free, vc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Bundle adjustment with radial distortion ("The distortion"): COLMAP's SIMPLE_RADIAL (k2 held at 0)
 * and RADIAL camera models.  The distortion travels beside the 16-number camera row, which does not change:
 *   cam_dist    [n_cams][2] float64: (k1, k2) of each camera slot
 * This build's own published rule; parity with COLMAP / Ceres is unpinned.  Specification: tests/util_bundle_radial.py.
 * float64, single operations in the written order (left to right, the usual precedence), sqrt the only library call, no atomics.
 * For camera row c = (R, t, fx, fy, cx, cy) and the point X:
 *   Y = R X, Xc = Y + t, iu = 1 / Xc_z, xu = Xc_x / Xc_z, xv = Xc_y / Xc_z,
 *   nu_k = iu (R_0k - xu R_2k), nv_k = iu (R_1k - xv R_2k)                         (the pinhole J_p at fx = fy = 1)
 *   rho = xu xu + xv xv,  s = 1 + k1 rho + k2 rho rho,  e = 2 (k1 + 2 k2 rho)
 *   d00 = s + xu xu e,  d01 = xu xv e,  d11 = s + xv xv e                           (the 2x2 Jacobian of (xu, xv) -> (xu s, xv s))
 *   xd = xu s, yd = xv s,  r = (fx xd + cx - u, fy yd + cy - v)
 *   J_p row u = fx (d00 nu + d01 nv), row v = fy (d01 nu + d11 nv)
 *   J_c likewise from the pinhole rows at fx = fy = 1: au = iu xu, av = iu xv,
 *       mu = (-(au Y_1), iu Y_2 + au Y_0, -(iu Y_1), iu, 0, -au), mv = (-(iu Y_2 + av Y_1), av Y_0, iu Y_0, 0, iu, -av),
 *       row u = fx (d00 mu + d01 mv), row v = fy (d01 mu + d11 mv)
 *   pu = fx xu rho, pv = fy xv rho, qu = pu rho, qv = pv rho
 *   J_theta, six columns (fx, fy, cx, cy, k1, k2): row u = (xd, 0, 1, 0, pu, qu), row v = (0, yd, 0, 1, pv, qv); tied: column 0 =
 *   (xd, yd), column 1 = 0; a held column is 0.
 * An observation is usable under the conditions of vc_ba_linearize_points and finite k1, k2 of its camera.  Every entry point
 * takes the loss (loss, loss_scale as vc_ba_linearize_points_loss; VC_BA_LOSS_TRIVIAL is the plain case: sw = 1 and every product
 * with it is exact) and the weight array obs_w.
 *
 * vc_ba_linearize_points_radial: vc_ba_linearize_points_loss under the projection above; its outputs mean what they mean there,
 * so vc_ba_reduce_cameras runs on them as it is.
 * vc_ba_linearize_intrinsics_radial, vc_ba_reduce_border_radial, vc_ba_step_radial: the border with six unknowns per group,
 * theta_g = (fx, fy, cx, cy, k1, k2); the layouts of the three entry points of "The border" with 6 in the place of 4:
 *   intr_mask   bits 0-4 as there; bit 5 = k1 held, bit 6 = k2 held
 *   out_obs_jt  [total][6]: (xd, yd, pu, pv, qu, qv) of a usable observation (unscaled by the loss), 0 otherwise: what the B pass
 *               rebuilds J_theta from
 *   out_T       [n_points][n_groups][18] (6x3 row-major)
 *   out_terms   [48 G + 36 G^2][n_points]: rows 36 g + 6 i + k: q_jg; 36 G + 6 g + i: hq_jg; 42 G + 6 g + i: T V^-1 g_p;
 *               48 G + 36 (g G + g') + 6 i + k: T_jg V^-1 T_jg''
 *   out_sums    [48 G + 36 G^2], out_C [6 G][6 G], out_h [6 G], out_free [6 G], out_B [6 n_cams][6 G] (entry 36 g + 6 r + i of a
 *               camera's row block owned by lane (36 g + 6 r + i) mod 64)
 *   vc_ba_step_radial: dtheta [6 G]; out_dist [n_cams][2] = cam_dist + (dtheta_4, dtheta_5) of the slot's group (copied where
 *               the slot has none); out_valid: 0 where the slot's group is in the table and its new fx or fy is not finite or not
 *               positive, or its new k1 or k2 is not finite.
 * n_groups <= VC_BA_MAX_GROUPS_RADIAL (the terms grow with 36 G^2 numbers per point and a lane of the B pass keeps
 * ceil(36 G / 64) = 3 entries in registers), VC_ERR_UNSUPPORTED above; sizes of 0, null pointers, negative sizes, a bad loss and a
 * bad lambda as the entry points above; every index is checked; skipped points and cameras write nothing.
 * ------------------------------------------------------------------------------------------ */
#define VC_BA_MAX_GROUPS_RADIAL 4
int vc_ba_linearize_points_radial(const double* cams, int n_cams, const double* cam_dist, const uint8_t* const_mask, const double* points,
                                  int n_points, const int32_t* offsets, const int32_t* obs_cam, const double* obs_xy, int total, double lambda,
                                  int loss, double loss_scale, double* out_vinv, double* out_gp, double* out_cost, int32_t* out_count,
                                  uint8_t* out_obs_ok, double* out_obs_lin, double* out_obs_w, double* out_total_cost, vc_stream_t stream);
int vc_ba_linearize_intrinsics_radial(const double* cams, int n_cams, const double* cam_dist, const int32_t* cam_group, int n_groups,
                                      const uint8_t* intr_mask, const double* points, int n_points, const int32_t* offsets,
                                      const int32_t* obs_cam, int total, int loss, double loss_scale, const double* vinv, const double* gp,
                                      const uint8_t* obs_ok, const double* obs_lin, const double* obs_w, double* out_obs_jt, double* out_T,
                                      double* out_terms, vc_stream_t stream);
int vc_ba_reduce_border_radial(int n_cams, const int32_t* cam_group, int n_groups, const uint8_t* intr_mask, int n_points,
                               const int32_t* offsets, const int32_t* obs_cam, int total, const int32_t* cam_offsets, const int32_t* cam_obs,
                               const int32_t* obs_point, double lambda, int loss, double loss_scale, const double* vinv, const uint8_t* obs_ok,
                               const double* obs_lin, const double* obs_jt, const double* obs_w, const double* T, const double* terms,
                               double* out_sums, double* out_B, double* out_C, double* out_h, uint8_t* out_free, vc_stream_t stream);
int vc_ba_step_radial(const double* cams, int n_cams, const double* cam_dist, const int32_t* cam_group, int n_groups, const uint8_t* intr_mask,
                      const double* points, int n_points, const int32_t* offsets, const int32_t* obs_cam, int total, const double* vinv,
                      const double* gp, const uint8_t* obs_ok, const double* obs_lin, const double* T, const double* dc, const double* dtheta,
                      double* out_cams, double* out_dist, double* out_points, double* out_dx, uint8_t* out_valid, vc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Bundle adjustment with radial and tangential distortion ("The tangential terms"): COLMAP's OPENCV
 * camera model, (fx, fy, cx, cy, k1, k2, p1, p2).  The distortion travels beside the 16-number camera row:
 *   cam_dist    [n_cams][4] float64: (k1, k2, p1, p2) of each camera slot
 * This build's own published rule; parity with COLMAP / Ceres is unpinned.  Specification: tests/util_bundle_opencv.py.  The
 * forward model and its symmetric Jacobian are the ones vc_undistort_keypoints inverts, in its order of operations: the radial
 * term first, the tangential terms added after it.
 * float64, single operations in the written order (left to right, the usual precedence), sqrt the only library call, no atomics.
 * With Y, Xc, iu, (xu, xv), (nu; nv), (mu; mv) as in the radial rule above (ba_project on the row at fx = fy = 1):
 *   rho = xu xu + xv xv,  s = 1 + k1 rho + k2 rho rho,  e = 2 (k1 + 2 k2 rho)
 *   xd = xu s + 2 p1 xu xv + p2 (rho + 2 xu xu)
 *   yd = xv s + p1 (rho + 2 xv xv) + 2 p2 xu xv
 *   d00 = s + xu xu e + 2 p1 xv + 6 p2 xu
 *   d01 = xu xv e + 2 p1 xu + 2 p2 xv
 *   d11 = s + xv xv e + 6 p1 xv + 2 p2 xu
 *   r = (fx xd + cx - u, fy yd + cy - v)
 *   J_p row u = fx (d00 nu + d01 nv), row v = fy (d01 nu + d11 nv); J_c row u = fx (d00 mu + d01 mv), row v = fy (d01 mu + d11 mv)
 *   J_theta, eight columns (fx, fy, cx, cy, k1, k2, p1, p2):
 *     row u = (xd, 0, 1, 0, fx xu rho, (fx xu rho) rho, fx 2 xu xv,          fx (rho + 2 xu xu))
 *     row v = (0, yd, 0, 1, fy xv rho, (fy xv rho) rho, fy (rho + 2 xv xv),  fy 2 xu xv)
 *   tied: column 0 = (xd, yd), column 1 = 0; a held column is 0.
 * An observation is usable under the conditions of vc_ba_linearize_points and finite k1, k2, p1, p2 of its camera.  Every entry
 * point takes the loss and obs_w as the _radial ones do.
 *
 * vc_ba_linearize_points_opencv writes exactly the arrays of vc_ba_linearize_points_loss: vc_ba_reduce_cameras, vc_ba_step and
 * the entry points of the solver without S run on them as they are.
 * vc_ba_linearize_intrinsics_opencv, vc_ba_reduce_border_opencv, vc_ba_step_opencv: the border with eight unknowns per group,
 * theta_g = (fx, fy, cx, cy, k1, k2, p1, p2); the layouts of "The border" with 8 in the place of 4:
 *   intr_mask   bits 0-6 as in the radial rule; bit 7 = p1 and p2 held, both
 *   out_obs_jt  [total][10]: xd, yd, then the entries of the k1, k2, p1 and p2 columns of J_theta, (row u, row v) of each, of a
 *               usable observation (unscaled by the loss), 0 otherwise: what the B pass rebuilds J_theta from
 *   out_T       [n_points][n_groups][24] (8x3 row-major)
 *   out_terms   [80 G + 64 G^2][n_points]: rows 64 g + 8 i + k: q_jg; 64 G + 8 g + i: hq_jg; 72 G + 8 g + i: T V^-1 g_p;
 *               80 G + 64 (g G + g') + 8 i + k: T_jg V^-1 T_jg''
 *   out_sums    [80 G + 64 G^2], out_C [8 G][8 G], out_h [8 G], out_free [8 G], out_B [6 n_cams][8 G] (entry 48 g + 8 r + i of a
 *               camera's row block owned by lane (48 g + 8 r + i) mod 64)
 *   vc_ba_step_opencv: dtheta [8 G]; out_dist [n_cams][4] = cam_dist + dtheta_4 .. dtheta_7 of the slot's group (copied where the
 *               slot has none); out_valid: 0 where the slot's group is in the table and its new fx or fy is not finite or not
 *               positive, or one of its four new distortion numbers is not finite.
 * n_groups <= VC_BA_MAX_GROUPS_OPENCV (the terms grow with 64 G^2 numbers per point, 1344 rows at G = 4, and a lane of the B pass
 * keeps ceil(48 G / 64) = 3 entries in registers), VC_ERR_UNSUPPORTED above; sizes of 0, null pointers, negative sizes, a bad loss
 * and a bad lambda as the _radial entry points; every index is checked; skipped points and cameras write nothing.
 * ------------------------------------------------------------------------------------------ */
#define VC_BA_MAX_GROUPS_OPENCV 4
int vc_ba_linearize_points_opencv(const double* cams, int n_cams, const double* cam_dist, const uint8_t* const_mask, const double* points,
                                  int n_points, const int32_t* offsets, const int32_t* obs_cam, const double* obs_xy, int total, double lambda,
                                  int loss, double loss_scale, double* out_vinv, double* out_gp, double* out_cost, int32_t* out_count,
                                  uint8_t* out_obs_ok, double* out_obs_lin, double* out_obs_w, double* out_total_cost, vc_stream_t stream);
int vc_ba_linearize_intrinsics_opencv(const double* cams, int n_cams, const double* cam_dist, const int32_t* cam_group, int n_groups,
                                      const uint8_t* intr_mask, const double* points, int n_points, const int32_t* offsets,
                                      const int32_t* obs_cam, int total, int loss, double loss_scale, const double* vinv, const double* gp,
                                      const uint8_t* obs_ok, const double* obs_lin, const double* obs_w, double* out_obs_jt, double* out_T,
                                      double* out_terms, vc_stream_t stream);
int vc_ba_reduce_border_opencv(int n_cams, const int32_t* cam_group, int n_groups, const uint8_t* intr_mask, int n_points,
                               const int32_t* offsets, const int32_t* obs_cam, int total, const int32_t* cam_offsets, const int32_t* cam_obs,
                               const int32_t* obs_point, double lambda, int loss, double loss_scale, const double* vinv, const uint8_t* obs_ok,
                               const double* obs_lin, const double* obs_jt, const double* obs_w, const double* T, const double* terms,
                               double* out_sums, double* out_B, double* out_C, double* out_h, uint8_t* out_free, vc_stream_t stream);
int vc_ba_step_opencv(const double* cams, int n_cams, const double* cam_dist, const int32_t* cam_group, int n_groups, const uint8_t* intr_mask,
                      const double* points, int n_points, const int32_t* offsets, const int32_t* obs_cam, int total, const double* vinv,
                      const double* gp, const uint8_t* obs_ok, const double* obs_lin, const double* T, const double* dc, const double* dtheta,
                      double* out_cams, double* out_dist, double* out_points, double* out_dx, uint8_t* out_valid, vc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Keypoint selection + descriptors over the ViT token grid — replaces
 * ViTExtractor._dense_to_sparse and helpers (reference vit_colmap/features/vit_extractor.py:168-653).
 * Specification: oracle/select_oracle.py.  All functions are batched over n_images.
 * ------------------------------------------------------------------------------------------ */
#define VC_DTYPE_F32 0
#define VC_DTYPE_BF16 1

#define VC_METHOD_HARRIS 0   /* vit_extractor.py:281-348 */
#define VC_METHOD_DOG 1      /* vit_extractor.py:350-394 */
#define VC_METHOD_COMBINED 2 /* vit_extractor.py:271-277 */

/*
 * tokens [n_images][H*W][C] (float32 or bfloat16, token = y*W + x) -> st [n_images][4][H*W]:
 * channel means of gx^2, gy^2, gx*gy (forward differences, zero at the last column / row) and
 * the channel mean of the features (vit_extractor.py:298-309, 365).
 */
int vc_structure_tensor(const void* tokens, int token_dtype, int n_images, int H, int W, int C,
                        float* st, vc_stream_t stream);

/* st -> score [n_images][H*W] in [0,1] (method: VC_METHOD_*).  H*W <= 16384 cells, VC_ERR_UNSUPPORTED above.
 * NOTE the two cell limits: this entry scores up to 16384 cells, vc_select_keypoints below takes 10112 at most.  A
 * 1920x1080 frame (77 x 137 = 10549 cells) is scored here and then refused there. */
int vc_score_map(const float* st, int n_images, int H, int W, int method, float* score,
                 vc_stream_t stream);

/*
 * score -> kept keypoints in score order: spatial binning with per-bin top-k (bin_size cells),
 * global top-`target`, greedy NMS at `nms_radius` cells (vit_extractor.py:404-543).
 * Total order everywhere: score descending, then position ascending.
 * out_yx [n_images][kmax][2] (y, x), out_score [n_images][kmax], out_count [n_images]; the kernel writes every slot
 * (zeros behind the kept points), so the buffers may be handed over uninitialised.
 * dbg_cand_* (all NULL or all non-NULL, same shapes): the candidate list before NMS (slots behind it are left as they were).
 * NMS rule, as the reference states it (vit_extractor.py:534-537): a kept point suppresses the later points at squared cell
 * distance d2 > 0 with sqrtf((float)d2) < nms_radius, both in float32.  The entry turns the radius into the largest such d2 with
 * the host's IEEE sqrtf and the kernel compares integers.  (This is not d2 < nms_radius^2: at nms_radius = sqrtf(37) the float32
 * square is above 37, yet distance^2 37 is kept.)
 * Limits: target <= 4096 and at most 4096 candidates before the global cut (bins * max(1, target / bins));
 * H*W*8 + 80 KiB <= 159 KiB, i.e. H*W <= 10112 cells (vc_score_map goes on to 16384: see there); 0 <= nms_radius <= 8;
 * all of these VC_ERR_UNSUPPORTED.  kmax >= min(target, candidates), else VC_ERR_INVALID_ARG.  A refusal launches nothing.
 */
int vc_select_keypoints(const float* score, int n_images, int H, int W, int target, int bin_size,
                        float nms_radius, int kmax, int32_t* out_yx, float* out_score,
                        int32_t* out_count, int32_t* dbg_cand_yx, float* dbg_cand_score,
                        int32_t* dbg_cand_count, vc_stream_t stream);

/*
 * Descriptors at the kept grid points: bilinear gather with the reference's grid_sample arithmetic
 * (vit_extractor.py:545-586), optional projection desc @ proj ([C][dd] float32, NULL = none;
 * vit_extractor.py:651), L2 normalisation (:243), uint8 quantisation clip(d*512, 0, 255) truncated
 * (:250), and pixel coordinates (x + 0.5) * (resized_w / W) * (orig_w / resized_w) (:229-236).
 * out_kp [n_images][kmax][2] float32 (x, y); out_desc_f32 (may be NULL) and out_desc_u8
 * [n_images][kmax][dd or C]; rows >= count[i] are zero-filled (vc_prepare_descriptors reads them).
 */
int vc_describe(const void* tokens, int token_dtype, int n_images, int H, int W, int C,
                const int32_t* yx, const int32_t* count, int kmax, const float* proj, int dd,
                int resized_w, int resized_h, int orig_w, int orig_h, float* out_kp,
                float* out_desc_f32, uint8_t* out_desc_u8, vc_stream_t stream);

/*
 * Descriptors at GIVEN sub-pixel keypoints — replaces ViTExtractor._extract_descriptors_at_keypoints of the reference's
 * hybrid extractor (vit_colmap/features/hybrid_extractor.py:224-294; the OpenCV detectors that produce the keypoints
 * stay on the host).  keypoints_xy [n_images][kmax][2] float32 (x, y) in original-image pixels; the sampling position is
 * x * (feat_w / orig_w) * (W / feat_w) as the reference computes it, then the same grid_sample arithmetic, optional
 * projection and quantiser as vc_describe.  normalisation: VC_NORM_L2, or VC_NORM_ROOTSIFT = L1-normalise, sqrt(clamp(., 1e-8)),
 * L2-normalise (:285-288).  out_desc_f32 may be NULL; rows >= count[i] are zero-filled.
 */
#define VC_NORM_L2 0
#define VC_NORM_ROOTSIFT 1
int vc_describe_at(const void* tokens, int token_dtype, int n_images, int H, int W, int C, const float* keypoints_xy,
                   const int32_t* count, int kmax, const float* proj, int dd, int feat_w, int feat_h, int orig_w,
                   int orig_h, int normalisation, float* out_desc_f32, uint8_t* out_desc_u8, vc_stream_t stream);

/* The quantiser alone: out[i] = (uint8) clip(in[i] * 512, 0, 255)   (vit_extractor.py:250). */
int vc_quantize_u8(const float* in, uint8_t* out, size_t n, vc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Keypoints + descriptors from dense head outputs — replaces the post-model part of
 * TrainableViTExtractor._run_inference (reference vit_colmap/features/trainable_vit_extractor.py:170-267;
 * _simple_nms :114-138).  Specification: oracle/trainable_oracle.py.  Batched over same-size images.
 *   kp_map        [n_images][4][H][W] float32: score logit, dx, dy, orientation (model output "keypoints")
 *   desc_map      float32 descriptor map (model output "descriptors", unit norm), element (image i, channel c,
 *                 cell p = y W + x) at i desc_image_stride + c desc_channel_stride + p desc_pixel_stride, so both
 *                 the reference's [D][H][W] (strides D H W, H W, 1) and a channels-last map (H W D, 1, D) are accepted
 *   score = sigmoid(logit) (correctly rounded float32); candidate iff score equals the maximum of its
 *   (2 nms_radius + 1)^2 window (-inf outside the map) and score > score_threshold; the kmax best by (score
 *   descending, position ascending) are kept (trainable_vit_extractor.py:181-210).
 *   out_keypoints [n_images][kmax][6] float32: x = clamp((((col + dx) + 0.5) 4) scale_x, 0, x_max), y likewise,
 *                 1, orientation, score, 0  (:219-254; scale_x = float32(orig_w / resized_w), x_max = orig_w - 1)
 *   out_desc      [n_images][kmax][D] uint8 = trunc(clip((d + 1) 127.5, 0, 255))  (:265-267)
 *   out_count     [n_images] int32; rows >= count are zero (whole blocks for vc_prepare_descriptors)
 *   workspace     vc_heatmap_workspace_bytes(n_images, H, W, kmax) bytes, 16-byte aligned.  kmax <= 65536.
 */
size_t vc_heatmap_workspace_bytes(int n_images, int H, int W, int kmax);
int vc_heatmap_keypoints(const float* kp_map, const float* desc_map, long long desc_image_stride,
                         long long desc_channel_stride, long long desc_pixel_stride, int n_images, int H, int W,
                         int D, int nms_radius, float score_threshold, int kmax, float scale_x, float scale_y,
                         float x_max, float y_max, void* workspace, float* out_keypoints, uint8_t* out_desc,
                         int32_t* out_count, vc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Image preprocessing — replaces reference vit_extractor.py:117-132 (BGR->RGB, resize to
 * multiples of 14 with cv2.INTER_LINEAR, /255, ImageNet mean/std), batched.
 * ------------------------------------------------------------------------------------------ */
#define VC_LAYOUT_NCHW 0    /* out [n][3][out_h][out_w]                                        */
#define VC_LAYOUT_PATCHES 1 /* out [n][(out_h/14)*(out_w/14)][3*14*14], element (c, dy, dx)    */
#define VC_LAYOUT_PATCHES_PAD 2 /* the same with rows padded to VC_PATCH_K_PADDED elements, zeros in the
                                   padding: the A operand of vc_patch_embed_bf16                  */
#define VC_PATCH_K_PADDED 640

/*
 * images_bgr [n_images][h][w][3] uint8 -> model input (float32 or bfloat16, VC_DTYPE_*).
 * The frame is resized only if (out_h, out_w) != (h, w).  resized_bgr_or_null (optional,
 * [n_images][out_h][out_w][3] uint8) receives the resized 8-bit frame for inspection.
 */
int vc_preprocess_u8(const uint8_t* images_bgr, int n_images, int h, int w, int out_h, int out_w,
                     int out_dtype, int layout, void* out, uint8_t* resized_bgr_or_null,
                     vc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * ViT glue (bf16): y = LayerNorm(x + residual) in one pass — the two memory-bound ops between
 * the GEMMs of a DINOv2 block (the model behind reference vit_extractor.py:135-146).
 * x, residual, y: [rows][C] bfloat16; gamma, beta: [C] bfloat16; statistics in float32.
 * residual_or_null == NULL: plain LayerNorm.  sum_out_or_null (may alias neither input) receives
 * x + residual rounded to bfloat16, i.e. the new residual stream.  C % 8 == 0, C <= 2048,
 * all pointers 16-byte aligned.
 * ------------------------------------------------------------------------------------------ */
int vc_add_layernorm_bf16(const void* x, const void* residual_or_null, const void* gamma,
                          const void* beta, float eps, int rows, int C, void* sum_out_or_null,
                          void* y_out, vc_stream_t stream);

/* Plain LayerNorm over rows that come in groups of group_rows (one image's tokens), dropping the FIRST row of every group
 * (the class token, which nothing downstream reads: reference vit_extractor.py:140-142 takes x_norm_patchtokens):
 * x [n_groups][group_rows][C] -> y [n_groups][group_rows - 1][C], dense.  Same arithmetic as vc_add_layernorm_bf16. */
int vc_layernorm_drop_first_bf16(const void* x, const void* gamma, const void* beta, float eps, int n_groups,
                                 int group_rows, int C, void* y_out, vc_stream_t stream);

/*
 * Multi-head self-attention forward, head_dim 64 (DINOv2 ViT-S/B/L): softmax(Q K^T / 8) V.
 * qkv [batch][n_tokens][3][n_heads][64] bfloat16 (the fused qkv projection's output as it is),
 * out [batch][n_tokens][n_heads*64] bfloat16 (what the output projection reads).  16-byte aligned.
 * q_prescaled != 0: the q part of qkv already carries the factor (1/8) * log2(e) (fold it into the rows of the qkv
 * projection that produce q, weights and bias): the kernel then subtracts the row maximum inside the matrix product and
 * evaluates exp2 of the accumulator directly — one float instruction less per score, same softmax.  The maximum is that of
 * the first 64 keys; if later scores of any row in a block of 128 or 256 query rows exceed it so far that the row's sum of
 * exp2(score - maximum) passes 64 * n_tokens, the block is recomputed with the running maximum and rescale, at about twice
 * the time for that block.  NaN inputs give NaN rows.
 */
int vc_attention_bf16(const void* qkv, int batch, int n_tokens, int n_heads, int head_dim, int q_prescaled,
                      void* out, vc_stream_t stream);

/*
 * Layouts of a 384-wide bf16 activation tensor [rows][384] between the kernels of a ViT-S block (vc_attention_bf16_l,
 * vc_linear_xs_bf16_l, vc_mlp_bf16_l).  VC_ACT_ROW_MAJOR: rows of 768 bytes.  VC_ACT_FRAGMENT: the order in which the
 * 32x32x16 MFMA reads the tensor as its B operand — ceil(rows / 32) blocks of 24 KiB, element (m, k) at byte
 *   ((m >> 5) * 24 + (k >> 4)) * 1024 + (((k >> 3) & 1) * 32 + (m & 31)) * 16 + (k & 7) * 2;
 * the buffer holds vc_act_fragment_bytes(rows) bytes, i.e. the row count padded to a multiple of 32.  The kernels never
 * read the padding's content and may write into it.  The values are the same in both layouts, bit for bit.
 */
#define VC_ACT_ROW_MAJOR 0
#define VC_ACT_FRAGMENT 1
size_t vc_act_fragment_bytes(long long rows);
/* vc_attention_bf16 with out in `out_layout`: VC_ACT_FRAGMENT needs n_heads * 64 == 384 (VC_ERR_UNSUPPORTED otherwise);
 * out is then one tensor of batch * n_tokens rows (a wave's 32 queries may lie in two of its 32-row blocks). */
int vc_attention_bf16_l(const void* qkv, int batch, int n_tokens, int n_heads, int head_dim, int q_prescaled,
                        void* out, int out_layout, vc_stream_t stream);

/*
 * Linear layer with fused epilogue (bf16 in, float32 accumulate on MFMA, bf16 out):
 *   out = epi(x W^T + bias),  x [rows][k_in], weight [n_out][k_in] (torch.nn.Linear layout),
 *   bias [n_out], out [rows][n_out].
 * epilogue: VC_EPI_BIAS     out = x W^T + b                    (attn.qkv)
 *           VC_EPI_GELU     out = gelu_erf(x W^T + b)          (mlp.fc1; exact GELU, erf to 1.5e-7)
 *           VC_EPI_RESIDUAL out = residual + x W^T + b         (attn.proj, mlp.fc2: the block's
 *                           residual-stream update; residual [rows][n_out], may alias out)
 * The pre-activation is NOT rounded to bf16 before GELU / the residual add (one rounding less than
 * the unfused sequence).  n_out % 128 == 0, k_in % 64 == 0, pointers 16-byte aligned,
 * residual_or_null non-NULL exactly for VC_EPI_RESIDUAL.
 *           VC_EPI_SWIGLU   the gated activation of DINOv2's SwiGLU FFN (mlp.w12 of the ViT-g models) fused into the
 *                           product.  weight [n_out][k_in] and bias [n_out] exactly as mlp.w12 stores them: with
 *                           H = n_out / 2, rows 0 .. H-1 produce the gate a, rows H .. 2H-1 the value b,
 *                             a[m][j] = x[m] W[j]^T + bias[j],   b[m][j] = x[m] W[H + j]^T + bias[H + j],
 *                           and out is [rows][H], HALF as wide as the product:
 *                             out[m][j] = silu(a[m][j]) * b[m][j],   silu(a) = a / (1 + exp(-a)).
 *                           Both pre-activations stay in float32 until the one rounding of the product (NOT rounded to
 *                           bf16 before, as above); a gate far below zero gives 0, far above zero a * b, never NaN.
 *                           residual_or_null must be NULL (VC_ERR_INVALID_ARG otherwise), n_out % 256 == 0 (so
 *                           H % 128 == 0; VC_ERR_UNSUPPORTED otherwise), out must not alias x.  No copy or permutation of
 *                           the weight: a tile fetches its W operand from the two row ranges.
 * Two tile forms behind the one entry: a 256 x 256 persistent tile (one workgroup per CU, 128 KiB staging ring) when
 * n_out % 256 == 0 and its tiles fill at least half the device's CUs, ceil(rows / 256) * (n_out / 256) * 2 >= CUs (128
 * tiles on 256 CUs) — the ViT-B / ViT-L / ViT-g layers on a batch of frames — and a 128 x 128 tile otherwise, for every
 * epilogue (VC_EPI_SWIGLU: a tile then makes 128 resp. 64 output columns); same arithmetic, the accumulation order over
 * k_in is the same in both.  vc_linear_tile_rows answers which form a shape takes.
 * Replaces the nn.Linear / GELU / residual-add calls inside the hub model's blocks
 * (reference vit_extractor.py:135-146).
 */
#define VC_EPI_BIAS 0
#define VC_EPI_GELU 1
#define VC_EPI_RESIDUAL 2
#define VC_EPI_SWIGLU 4 /* (3 is taken inside the library: the patch-embedding epilogue, not accepted here) */
int vc_linear_bf16(const void* x, const void* weight, const void* bias, const void* residual_or_null,
                   void* out, int rows, int n_out, int k_in, int epilogue, vc_stream_t stream);

/* The tile form vc_linear_bf16 takes for [rows] x [n_out] on the current device, by the rule above: 256 or 128 (the rows of
 * a tile), or a negative VC_ERR_* status (n_out % 128 != 0: VC_ERR_UNSUPPORTED).  Host code only, nothing is launched. */
int vc_linear_tile_rows(int rows, int n_out);

/*
 * Convolution over a channels-last image batch as an implicit GEMM on the 256 x 256 tile (the convolutional heads of the
 * trainable extractor: reference vit_colmap/model/vit_feature_model.py:12-29 UpsampleBlock — ConvTranspose2d(4, stride 2,
 * pad 1) as four 2 x 2-tap products, one per output parity — and :96-120 trunk / heads, Conv2d 3 x 3 pad 1; eval-mode
 * BatchNorm folded into weight and bias by the caller):
 *   out[(b, y, x)][n] = epi( sum over taps t = (ty, tx), channels c of
 *                            x[b][y + dy0 + ty][x + dx0 + tx][c] * weight[n][(ty * kw + tx) * c_in + c]  + bias[n] ),
 * pixels outside the image contribute zero.  x [batch * height * width + 1][c_in] bf16: the image batch followed by ONE spare
 * row, which this call overwrites with zeros (taps outside the image read it); weight [n_out][kh * kw * c_in] bf16, bias
 * [n_out] bf16, out [batch * height * width][n_out] bf16.  epilogue VC_EPI_BIAS or VC_EPI_GELU.  n_out % 256 == 0,
 * c_in % 64 == 0, kh * kw <= 16, the batch below 4 GiB, 16-byte aligned pointers.  A 3 x 3 pad-1 convolution is
 * (kh, kw, dy0, dx0) = (3, 3, -1, -1).
 * out_parity: -1 = out as above.  2 i + j (0..3) = this call is parity class (i, j) of a stride-2 transposed convolution: row
 * (b, y, x) is written to pixel (2 y + i, 2 x + j) of out [batch][2 height][2 width][n_out]; the four calls of a layer
 * (taps (kh, kw, dy0, dx0) = (2, 2, i - 1, j - 1)) fill that tensor without an interleaving copy.
 */
int vc_conv_taps_bf16(void* x, const void* weight, const void* bias, void* out, int batch, int height, int width, int c_in,
                      int n_out, int kh, int kw, int dy0, int dx0, int out_parity, int epilogue, vc_stream_t stream);

/*
 * The same linear layer for k_in == 384 (ViT-S: attn.qkv, attn.proj, mlp.fc1), "x-stationary":
 * each wave keeps its 32 token rows in registers for the whole launch and only the weights stream
 * (csrc/gemm.hip).  Optionally fuses the LayerNorm that precedes the layer in a pre-norm block:
 *   out = epi(LayerNorm(x) W^T + b)   computed as   epi(((x - mean) rstd) (W diag(gamma))^T + (b + W beta)).
 *
 * vc_linear_xs_prepare (once per layer): weight [n_out][384] float32, bias [n_out] float32 or NULL,
 *   ln_gamma / ln_beta [384] float32 or both NULL  ->  weight_tiled (vc_linear_xs_weight_bytes bytes:
 *   bf16 in MFMA fragment order, piece (nb, ks) = features 32 nb..+32 x k 16 ks..+16, lane 32 h + r holds
 *   W'[32 nb + r][16 ks + 8 h .. +8]) and bias_folded [n_out] float32.
 * vc_linear_xs_bf16: x [rows][384] bf16, out [rows][n_out] bf16, epilogue as vc_linear_bf16;
 *   fuse_layernorm != 0 normalises each x row first (two-pass float32 statistics, eps = ln_eps; the
 *   weights must have been prepared with that LayerNorm's gamma / beta).  residual may alias out.
 *   n_out % 32 == 0, n_out <= 4096, 16-byte aligned pointers.  Launches one persistent workgroup per CU; an output of 2 GiB
 *   or more is written by consecutive launches over row ranges (the kernel's result store takes 32-bit byte offsets).
 */
size_t vc_linear_xs_weight_bytes(int n_out, int k_in);
int vc_linear_xs_prepare(const float* weight, const float* bias_or_null, const float* ln_gamma_or_null,
                         const float* ln_beta_or_null, int n_out, int k_in, void* weight_tiled,
                         float* bias_folded, vc_stream_t stream);
int vc_linear_xs_bf16(const void* x, const void* weight_tiled, const float* bias_folded,
                      const void* residual_or_null, void* out, int rows, int n_out, int k_in, int epilogue,
                      int fuse_layernorm, float ln_eps, const void* gelu_table_or_null, vc_stream_t stream);
/* vc_linear_xs_bf16 with the layouts of x, the residual and out (above).  All VC_ACT_ROW_MAJOR: vc_linear_xs_bf16.
 * Otherwise x is VC_ACT_FRAGMENT and the call is one of the two a ViT-S block makes: VC_EPI_BIAS with fuse_layernorm and a
 * row-major out (attn.qkv), or VC_EPI_RESIDUAL without LayerNorm, n_out == 384 and out VC_ACT_FRAGMENT, the residual in
 * either layout (attn.proj; a residual in fragment order may alias out).  Anything else: VC_ERR_UNSUPPORTED. */
int vc_linear_xs_bf16_l(const void* x, const void* weight_tiled, const float* bias_folded,
                        const void* residual_or_null, void* out, int rows, int n_out, int k_in, int epilogue,
                        int fuse_layernorm, float ln_eps, const void* gelu_table_or_null, int x_layout,
                        int residual_layout, int out_layout, vc_stream_t stream);
/*
 * GELU table for VC_EPI_GELU (optional): with a table the epilogue evaluates the GELU as the standard bf16
 * pipeline does — on the bf16-ROUNDED pre-activation, result rounded to bf16, bit for bit
 * bf16(0.5 x (1 + erff(x / sqrt 2))) — by an LDS lookup: a handful of integer instructions and one ds_read_u16 per value instead of
 * ~150 float instructions per 32x32 block (fewer issue slots beside the MFMAs; float and integer VALU overlap
 * with the matrix pipe alike, profiles/r02_overlap_probe.md).  Without a table
 * (NULL) the GELU is evaluated in float32 on the unrounded pre-activation.  vc_gelu_table_bytes() bytes,
 * 16-byte aligned, filled once by vc_gelu_table_bf16; used when n_out * 4 + table <= 16 KiB.
 */
size_t vc_gelu_table_bytes(void);
int vc_gelu_table_bf16(void* table, vc_stream_t stream);

/*
 * DINOv2 patch embedding + position embedding in one GEMM (the conv 14x14 / 14 of the hub model as a
 * matrix product over padded patches):
 *   out[b][1 + t][:] = patches[b][t][:] W^T + bias + pos_embed[1 + t][:]      t = 0 .. tokens-1
 * patches [n_images][tokens][k_in] bf16 (vc_preprocess_u8 with VC_LAYOUT_PATCHES_PAD, k_in = VC_PATCH_K_PADDED),
 * weight [n_out][k_in] bf16 (conv weight flattened (c, dy, dx), zero padded), bias [n_out] bf16,
 * pos_embed [1 + tokens][n_out] bf16 (already interpolated to this grid), out [n_images][1 + tokens][n_out] bf16.
 * Row 0 of every image (the class token + pos_embed[0]) is NOT written here.  n_out % 128 == 0, k_in % 64 == 0.
 */
int vc_patch_embed_bf16(const void* patches, const void* weight, const void* bias, const void* pos_embed,
                        void* out, int n_images, int tokens, int n_out, int k_in, vc_stream_t stream);

/*
 * Fused MLP of a pre-norm block for dim == 384 (ViT-S):  x += fc2(gelu(fc1(LayerNorm(x))))  in one kernel — the
 * hidden tensor never exists in memory (csrc/gemm.hip: mlp2_kernel).
 * GELU as in vc_linear_xs_bf16 with a table.
 * vc_mlp_prepare (once per block): w1 [n_hidden][384], b1 [n_hidden], LayerNorm gamma / beta [384] (or both NULL),
 *   w2 [384][n_hidden], b2 [384], all float32  ->  weights_tiled (vc_mlp_weight_bytes bytes, stage order), b1_folded
 *   [n_hidden] float32, b2_out [384] float32.  n_hidden % 32 == 0, n_hidden <= 1536.
 * vc_mlp_bf16: x_inout [rows][384] bf16, updated in place.  gelu_table from vc_gelu_table_bf16.  Row ranges of less than
 *   2 GiB per launch, as in vc_linear_xs_bf16.
 */
size_t vc_mlp_weight_bytes(int n_hidden, int dim);
int vc_mlp_prepare(const float* w1, const float* b1_or_null, const float* ln_gamma_or_null,
                   const float* ln_beta_or_null, const float* w2, const float* b2_or_null, int n_hidden, int dim,
                   void* weights_tiled, float* b1_folded, float* b2_out, vc_stream_t stream);
int vc_mlp_bf16(void* x_inout, const void* weights_tiled, const float* b1_folded, const float* b2,
                const void* gelu_table, int rows, int n_hidden, int dim, float ln_eps, vc_stream_t stream);
/* vc_mlp_bf16 with layouts (above): both VC_ACT_ROW_MAJOR or both VC_ACT_FRAGMENT update x_inout in place (out_or_null NULL
 * or x_inout); x VC_ACT_FRAGMENT with out VC_ACT_ROW_MAJOR leaves x_inout as it is and writes the rows to out_or_null, a
 * buffer of its own (the last block of the stack).  Row-major in, fragment order out: VC_ERR_INVALID_ARG. */
int vc_mlp_bf16_l(void* x_inout, void* out_or_null, const void* weights_tiled, const float* b1_folded, const float* b2,
                  const void* gelu_table, int rows, int n_hidden, int dim, float ln_eps, int x_layout, int out_layout,
                  vc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * SIFT with COLMAP's default SiftExtractionOptions, computed as VLFeat's vl_sift does — replaces the
 * pycolmap.extract_features call of the reference's ColmapSiftExtractor
 * (vit_colmap/features/colmap_sift_extractor.py).  Specification: tests/util_sift.py; driven stage by
 * stage by vit_colmap_amd/features/sift_extractor.py.  Batched over same-size images; the levels of one
 * octave are level-major, levels [n_levels][n_images][h][w] float32, S = n_levels - 3 = n_dog_levels - 2.
 * ------------------------------------------------------------------------------------------ */
#define VC_SIFT_MAX_RADIUS 64   /* Gaussian taps per side (taps = 2 radius + 1)                     */
#define VC_SIFT_NORM_L2 0
#define VC_SIFT_NORM_L1_ROOT 1

/* images_bgr [n][h][w][3] uint8 -> grey [n][H][W] float32 in [0, 1]: uint8 grey = floor(0.2126 R + 0.7152 G +
 * 0.0722 B + 0.5), bilinear (half-pixel centres) to out_h x out_w <= h x w when they differ, / 255; with upsample = 1,
 * VLFeat's 2x linear upsampling on top (H = 2 out_h, W = 2 out_w), else H = out_h, W = out_w. */
int vc_sift_grey(const uint8_t* images_bgr, int n_images, int h, int w, int out_h, int out_w, int upsample, float* out,
                 vc_stream_t stream);
/* dst = separable Gaussian of src ([n][h][w] each), rows then columns through tmp ([n][h][w]), edge replicate.
 * taps [host] 2 radius + 1 float32 weights, 1 <= radius <= VC_SIFT_MAX_RADIUS. */
int vc_sift_blur(const float* src, float* tmp, float* dst, int n_images, int h, int w, const float* taps, int radius,
                 vc_stream_t stream);
/* dst [n][h/2][w/2] = src [n][h][w] at even (y, x): the first level of the next octave. */
int vc_sift_downsample(const float* src, int n_images, int h, int w, float* dst, vc_stream_t stream);
/* dog [n_levels - 1][n][h][w] = levels[l + 1] - levels[l]. */
int vc_sift_dog(const float* levels, int n_levels, int n_images, int h, int w, float* dog, vc_stream_t stream);
/* Strict 26-neighbour extrema of DoG levels 1 .. S with |D| >= 0.8 peak_threshold, 1-pixel border excluded; with
 * refine = 1 VLFeat's Newton refinement and acceptance (peak, edge ratio, offset, inside the octave), with refine = 0
 * the raw extrema.  row_counts: workspace [n][S][h] int32.  out_keypoints [n][cap][8] float32 = x, y, s, sigma (octave
 * units), j, y0, x0, 0 in (j, y0, x0) raster order of the unrefined extremum; out_count [n] = number found, which may
 * exceed cap (only the first cap are written: call again with a larger cap). */
int vc_sift_detect(const float* dog, int n_images, int h, int w, int n_dog_levels, float peak_threshold,
                   float edge_threshold, int refine, int32_t* row_counts, int cap, float* out_keypoints,
                   int32_t* out_count, vc_stream_t stream);
/* 36-bin orientation histograms of keypoints [n][cap][8] (min(count, cap) per image) on their Gaussian level j:
 * out_angles [n][cap][4] (peaks in bin order), out_n_angles [n][cap] = min(peaks, max_orientations) (1 and angle 0 when
 * upright).  1 <= max_orientations <= 4. */
int vc_sift_orient(const float* levels, int n_levels, int n_images, int h, int w, const float* keypoints,
                   const int32_t* count, int cap, int max_orientations, int upright, float* out_angles,
                   int32_t* out_n_angles, vc_stream_t stream);
/* One row per (keypoint, orientation), in keypoint order: out_rows [n][row_cap][6] float32 = COLMAP's affine keypoint
 * ((x 2^o + 0.5) scale_x, (y 2^o + 0.5) scale_y, s cos, -s sin, s sin, s cos with s = sigma 2^o; columns 0, 2, 3 times
 * scale_x, 1, 4, 5 times scale_y), out_desc [n][row_cap][128] uint8 (VLFeat 4x4x8, L2 / clamp 0.2 / L2, optional
 * L1_ROOT, min(255, round(512 v)), UBC bin order), out_row_count [n].  octave_scale = 2^o.  row_offsets: workspace
 * [n][cap] int32.  row_cap >= cap * max_orientations (VC_ERR_WORKSPACE otherwise). */
int vc_sift_describe(const float* levels, int n_levels, int n_images, int h, int w, const float* keypoints,
                     const int32_t* count, int cap, const float* angles, const int32_t* n_angles, int max_orientations,
                     int normalization, float octave_scale, float scale_x, float scale_y, int32_t* row_offsets,
                     int row_cap, float* out_rows, uint8_t* out_desc, int32_t* out_row_count, vc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Classical detectors of the hybrid extractor — replace the OpenCV calls of the reference's
 * vit_colmap/features/hybrid_extractor.py:110-180 (cv2.FastFeatureDetector, cv2.goodFeaturesToTrack).
 * Specification: tests/util_detect.py, a numpy restatement of OpenCV's algorithms (parity with OpenCV
 * itself is unpinned).  Batched over same-size images; both convert to 8-bit grey with
 * OpenCV's fixed-point BGR2GRAY, (1868 B + 9617 G + 4899 R + 8192) >> 14, and equal the specification exactly.
 * Images under VC_DETECT_MIN_SIZE pixels in either dimension: VC_ERR_UNSUPPORTED.  Workspaces must be 16-byte
 * aligned; the *_workspace_bytes queries return 0 for sizes the entries refuse.
 * ------------------------------------------------------------------------------------------ */
#define VC_DETECT_MIN_SIZE 8
#define VC_DETECT_GFTT_MAX_CANDIDATES 16384 /* candidates per image the selection kernel ranks in LDS */

size_t vc_detect_fast_workspace_bytes(int n_images, int h, int w);
/* FAST-9/16 with non-maximum suppression.  images_bgr [n][h][w][3] uint8.  Score of a pixel p, integer: S = max over
 * the 16 arcs of 9 contiguous pixels c_k of the radius-3 circle of max(min_k(c_k - p), min_k(p - c_k)); S <= threshold
 * (0 .. 254) counts as 0, and so does every pixel closer than 3 to the edge.  A corner is kept iff S is strictly
 * greater than S of its 8 neighbours.  If more than max_keypoints are kept, those with the largest S stay, the
 * earlier raster position first among equal S (a 256-bin histogram per image finds the cut).  out_xy
 * [n][max_keypoints][2] float32 (x, y) in raster order, rows past the count zero; out_count [n] = rows written,
 * out_total [n] = corners before the limit. */
int vc_detect_fast(const uint8_t* images_bgr, int n_images, int h, int w, int threshold, int max_keypoints, void* workspace,
                   size_t workspace_bytes, float* out_xy, int32_t* out_count, int32_t* out_total, vc_stream_t stream);

size_t vc_detect_gftt_workspace_bytes(int n_images, int h, int w, int cand_cap);
/* Shi-Tomasi corners.  gx, gy = 3x3 Sobel of the grey image (reflect-101), int32; a, b, c = sums of gx^2, gx gy, gy^2
 * over the block_size x block_size window (3, 5 or 7; product images extended by reflect-101), int32; lambda =
 * (0.5 a + 0.5 c) - sqrt((0.5 a - 0.5 c)^2 + b^2) in float32, in this order, no fused multiply-add.  lambda <
 * quality_level * max(lambda) (float32 product, max over the image) counts as 0.  Candidates: lambda != 0 and equal to
 * the maximum of its 3x3 neighbourhood, outermost rows and columns excluded; none if max(lambda) <= 0.  Ranked by
 * lambda descending, the LATER raster position first among equals; a candidate is accepted iff no accepted candidate of
 * higher rank lies at squared distance < min_distance^2 (1 .. 64); the first max_corners accepted are written.
 * out_xy [n][max_corners][2] float32 (x, y) in acceptance order, rows past the count zero; out_count [n];
 * out_candidates [n] = candidates found, which may exceed cand_cap (<= VC_DETECT_GFTT_MAX_CANDIDATES): then out_count
 * is 0 for that image and the call must be repeated with a larger cand_cap. */
int vc_detect_gftt(const uint8_t* images_bgr, int n_images, int h, int w, float quality_level, int min_distance,
                   int block_size, int max_corners, int cand_cap, void* workspace, size_t workspace_bytes, float* out_xy,
                   int32_t* out_count, int32_t* out_candidates, vc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VITCOLMAP_HIP_H_ */
