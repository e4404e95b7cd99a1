// Two-view geometric verification, the scoring half (gfx950): inlier counts of many fundamental-matrix or
// homography hypotheses against the putative matches of many image pairs, and the inlier mask of one model
// per pair.  This is the step that follows descriptor matching inside pycolmap.match_exhaustive and fills the
// `two_view_geometries` table the reference's metrics read (vit_colmap/utils/metrics.py:207-243).
// Hypotheses come from 8x8 linear solves on the host side of the ABI (vit_colmap_amd/matching/two_view.py);
// what is O(pairs x hypotheses x matches) runs here.  Specification: oracle/two_view_oracle.py (float32
// arithmetic in exactly this operation order; the library is built with -ffp-contract=off).
//
// Residuals (no division, so host oracle and device agree bit for bit):
//   F: Sampson error  (x2' F x1)^2 <= t^2 * den  with den = |F x1|_xy^2 + |F' x2|_xy^2
//   H: forward transfer error  |p_xy - x2 p_w|^2 <= t^2 * p_w^2  with p = H x1
// A denominator that is zero, or whose bound t^2 * denominator is not finite, has no inliers: `inf <= inf` and `0 <= 0`
// would otherwise count every match of an overflowing or an all-zero hypothesis.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vitcolmap_hip.h"
#include "inlier_count.h"

namespace {

__device__ __forceinline__ bool inlier_f(const float (&m)[9], float x1, float y1, float x2, float y2, float t2) {
  const float fx0 = m[0] * x1 + m[1] * y1 + m[2];
  const float fx1 = m[3] * x1 + m[4] * y1 + m[5];
  const float fx2 = m[6] * x1 + m[7] * y1 + m[8];
  const float ft0 = m[0] * x2 + m[3] * y2 + m[6];
  const float ft1 = m[1] * x2 + m[4] * y2 + m[7];
  const float c = x2 * fx0 + y2 * fx1 + fx2;
  const float den = fx0 * fx0 + fx1 * fx1 + ft0 * ft0 + ft1 * ft1;
  const float bound = t2 * den;
  return den > 0.f && bound < INFINITY && c * c <= bound;          // NaN hypotheses compare false
}

__device__ __forceinline__ bool inlier_h(const float (&m)[9], float x1, float y1, float x2, float y2, float t2) {
  const float p0 = m[0] * x1 + m[1] * y1 + m[2];
  const float p1 = m[3] * x1 + m[4] * y1 + m[5];
  const float pw = m[6] * x1 + m[7] * y1 + m[8];
  const float dx = p0 - x2 * pw;
  const float dy = p1 - y2 * pw;
  const float bound = t2 * (pw * pw);
  return pw != 0.f && bound < INFINITY && dx * dx + dy * dy <= bound;
}

struct Matches { const float4* __restrict__ pts; };                 // (x1, y1, x2, y2) per match

template <bool (*Inlier)(const float (&)[9], float, float, float, float, float)>
struct MatchRule {
  static constexpr int W = 9;
  using Data = Matches;
  static bool usable(Data d) { return d.pts && ((uintptr_t)d.pts) % 16 == 0; }
  static __device__ __forceinline__ bool inlier(const float (&m)[9], Data d, int i, float t2) {
    const float4 q = d.pts[i];
    asm volatile("" ::"v"(q.w));   // keeps the 16-byte load whole: left alone, H loads (x2, y2) apart, behind its pw test
    return Inlier(m, q.x, q.y, q.z, q.w, t2);
  }
};
using RuleF = MatchRule<inlier_f>;
using RuleH = MatchRule<inlier_h>;

}  // namespace

extern "C" {

int vc_two_view_score(const float* pts, const int32_t* offsets, int n_pairs, const float* hypotheses, int n_hyp,
                      int model, float max_error, int32_t* out_counts, vc_stream_t stream) {
  if (model != VC_MODEL_FUNDAMENTAL && model != VC_MODEL_HOMOGRAPHY) return VC_ERR_INVALID_ARG;
  const auto launch = model == VC_MODEL_FUNDAMENTAL ? vc::launch_inlier_count<RuleF> : vc::launch_inlier_count<RuleH>;
  return launch({(const float4*)pts}, offsets, n_pairs, hypotheses, n_hyp, max_error, out_counts, stream);
}

int vc_two_view_inliers(const float* pts, const int32_t* offsets, int n_pairs, const float* models, int model,
                        float max_error, uint8_t* out_mask, vc_stream_t stream) {
  if (model != VC_MODEL_FUNDAMENTAL && model != VC_MODEL_HOMOGRAPHY) return VC_ERR_INVALID_ARG;
  const auto launch = model == VC_MODEL_FUNDAMENTAL ? vc::launch_inlier_mask<RuleF> : vc::launch_inlier_mask<RuleH>;
  return launch({(const float4*)pts}, offsets, n_pairs, models, max_error, out_mask, stream);
}

}  // extern "C"
