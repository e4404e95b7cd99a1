// Inlier counts of many hypotheses against the correspondences of many problems, and the inlier mask of one model per
// problem: the kernels every RANSAC-shaped estimator scores with (two_view.hip: F and H, absolute_pose.hip: P).  A Rule has
// W, the floats per model; Data, the correspondences' device pointers, passed by value; usable(Data) on the host: every pointer
// set and aligned for its vector load; inlier(m[W], Data, i, t2) on the device: correspondence i under model m, t2 the squared
// error bound.  `offsets` (n_prob + 1) delimits each problem's correspondences.
#pragma once
#include "common.h"

namespace vc {

// grid (n_prob, hypothesis groups); 4 waves per workgroup, one hypothesis per wave and round, lanes over the correspondences
template <typename Rule>
__global__ __launch_bounds__(256) void inlier_count_kernel(typename Rule::Data d, const int32_t* __restrict__ offsets,
                                                           const float* __restrict__ hyp, int K, float t2,
                                                           int32_t* __restrict__ counts) {
  const int p = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lo = offsets[p], hi = offsets[p + 1];
  for (int k = blockIdx.y * 4 + wave; k < K; k += gridDim.y * 4) {
    float m[Rule::W];
#pragma unroll
    for (int i = 0; i < Rule::W; ++i) m[i] = hyp[((size_t)p * K + k) * Rule::W + i];
    int n = 0;
    for (int base = lo; base < hi; base += 64) {   // whole waves: the ballot needs every lane (base is wave-uniform)
      const int i = base + lane;
      const bool in = i < hi && Rule::inlier(m, d, i, t2);
      n += __popcll(__ballot(in));
    }
    if (lane == 0) counts[(size_t)p * K + k] = n;
  }
}

// one workgroup per problem
template <typename Rule>
__global__ __launch_bounds__(256) void inlier_mask_kernel(typename Rule::Data d, const int32_t* __restrict__ offsets,
                                                          const float* __restrict__ models, float t2, uint8_t* __restrict__ mask) {
  const int p = blockIdx.x;
  const int lo = offsets[p], hi = offsets[p + 1];
  float m[Rule::W];
#pragma unroll
  for (int i = 0; i < Rule::W; ++i) m[i] = models[(size_t)p * Rule::W + i];
  for (int i = lo + threadIdx.x; i < hi; i += blockDim.x) mask[i] = Rule::inlier(m, d, i, t2) ? 1 : 0;
}

// hyp (n_prob, n_hyp, W) -> out_counts (n_prob, n_hyp).  Nothing to do is VC_OK whatever the pointers are.
template <typename Rule>
int launch_inlier_count(typename Rule::Data d, const int32_t* offsets, int n_prob, const float* hyp, int n_hyp, float max_error,
                        int32_t* out_counts, vc_stream_t stream) {
  if (n_prob < 0 || n_hyp < 0) return VC_ERR_INVALID_ARG;
  if (n_prob == 0 || n_hyp == 0) return VC_OK;
  if (!Rule::usable(d) || !offsets || !hyp || !out_counts || !(max_error >= 0.f)) return VC_ERR_INVALID_ARG;
  if (n_prob > 65535 * 32) return VC_ERR_UNSUPPORTED;
  const int groups = n_hyp >= 64 ? 16 : (n_hyp + 3) / 4;
  hipLaunchKernelGGL(inlier_count_kernel<Rule>, dim3(n_prob, groups), dim3(256), 0, (hipStream_t)stream, d, offsets, hyp, n_hyp,
                     max_error * max_error, out_counts);
  return check_launch();
}

// models (n_prob, W) -> out_mask, one byte per correspondence
template <typename Rule>
int launch_inlier_mask(typename Rule::Data d, const int32_t* offsets, int n_prob, const float* models, float max_error,
                       uint8_t* out_mask, vc_stream_t stream) {
  if (n_prob < 0) return VC_ERR_INVALID_ARG;
  if (n_prob == 0) return VC_OK;
  if (!Rule::usable(d) || !offsets || !models || !out_mask || !(max_error >= 0.f)) return VC_ERR_INVALID_ARG;
  hipLaunchKernelGGL(inlier_mask_kernel<Rule>, dim3(n_prob), dim3(256), 0, (hipStream_t)stream, d, offsets, models,
                     max_error * max_error, out_mask);
  return check_launch();
}

}  // namespace vc
