// What the minimal solvers share (essential.hip: five-point E, absolute_pose.hip: P3P): float64, one hypothesis per lane, one
// wave per workgroup, no barrier, real roots by derivative bracketing.  Here are the pieces of that bracketing, whose operations
// and their order do not depend on where a list lives (a coefficient list is anything with operator[]: a register array whose
// loops unroll, or a strided list in LDS), and the kernel shell: which hypothesis a lane has, what a void sample is, where the
// solutions go.  A Solver has kSample, the indices per sample; kMaxSolutions; kWidth, the doubles per solution; kWorkDoubles,
// the run-time indexed doubles a lane needs (lane-interleaved LDS; 0: none); Data, the correspondences' device pointers, passed
// by value; usable(Data) on the host: every pointer set; solve(Data, lo, sample, work, stride, out) on the device: the solutions
// of correspondences lo + sample[i] to `out` -> their number.  `offsets` (n_prob + 1) delimits each problem's correspondences.
#pragma once
#include <math.h>
#include <stdint.h>

#include "common.h"

namespace vc {

constexpr int kSolverWave = 64;
constexpr int kBisections = 64;
// Both solvers look for a root variable of magnitude up to 1 in the polynomial itself and for a larger one through its
// reciprocal in the reversed polynomial.  A root on the seam between the two (P3P: two points equally far from the camera) shows
// either range only a rounding-sized value at its end, of either sign, so no sign change brackets it.  The direct range therefore
// reaches past the seam, to kSeamEnd, and a reversed root counts only below 1 / kSeamEnd: a root at 1 is inside the direct
// range and is reported once.  The new seam lies at no value that a symmetry of the scene produces.
constexpr double kSeamEnd = 1.0 + 1.0 / 1024.0;
constexpr double kSeamInv = 1.0 / kSeamEnd;

// sum c[i] t^i over i <= degree
template <typename C>
__host__ __device__ __forceinline__ double horner(const C& c, int degree, double t) {
  double v = c[degree];
  for (int i = degree - 1; i >= 0; --i) v = v * t + c[i];
  return v;
}

// coef[i] = a[i + k] binomial(i + k, k) for i <= degree: the k-th derivative of sum a[i] t^i, over k!
template <typename C, typename A>
__host__ __device__ __forceinline__ void derivative_coefficients(C& coef, int degree, int k, const A& a) {
  double binom = 1.0;
  for (int i = 0; i <= degree; ++i) {
    coef[i] = a[i + k] * binom;
    binom = binom * (double)(i + 1 + k) / (double)(i + 1);
  }
}

// One monotone piece [lo, hi] of the polynomial c, f_lo and f_hi its values at the ends -> the root a sign change brackets,
// bisected at most kBisections times (fewer when no double is left between the ends); NaN when there is no sign change.
template <typename C>
__host__ __device__ __forceinline__ double root_of_piece(const C& c, int degree, double lo, double hi, double f_lo, double f_hi) {
  double root = NAN;
  if ((f_lo < 0.0) != (f_hi < 0.0) && hi > lo) {
    double l = lo, h = hi;
    const bool neg = f_lo < 0.0;
    for (int it = 0; it < kBisections; ++it) {
      const double mid = 0.5 * (l + h);
      if (!(mid > l && mid < h)) break;
      if ((horner(c, degree, mid) < 0.0) == neg) l = mid; else h = mid;
    }
    root = 0.5 * (l + h);
  }
  return root;
}

// Hypothesis h = problem * n_hyp + k per lane.  A sample is void, and counts 0, when its problem's offset is negative or an
// index is outside [0, m) or occurs twice.  out (total, kMaxSolutions, kWidth): NaN past the count; out_count (total).
template <typename Solver>
__global__ __launch_bounds__(kSolverWave) void minimal_solver_kernel(typename Solver::Data d, const int32_t* __restrict__ offsets,
                                                                     long long total, const int32_t* __restrict__ samples, int n_hyp,
                                                                     double* __restrict__ out, int32_t* __restrict__ out_count) {
  double* work = nullptr;
  if constexpr (Solver::kWorkDoubles > 0) {                  // a solver that asks for none has no LDS allocation
    __shared__ double lds[Solver::kWorkDoubles][kSolverWave];
    work = &lds[0][threadIdx.x];
  }
  const long long h = (long long)blockIdx.x * kSolverWave + threadIdx.x;
  if (h >= total) return;
  const int prob = (int)(h / n_hyp);
  const long long lo = offsets[prob], m = (long long)offsets[prob + 1] - lo;
  int s[Solver::kSample];
  bool valid = lo >= 0;
#pragma unroll
  for (int i = 0; i < Solver::kSample; ++i) {
    s[i] = samples[h * Solver::kSample + i];
    valid = valid && s[i] >= 0 && s[i] < m;
#pragma unroll
    for (int j = 0; j < i; ++j) valid = valid && s[i] != s[j];
  }
  double* o = out + h * (Solver::kMaxSolutions * Solver::kWidth);   // the solutions go straight to their slots: no per-lane array
  const int count = valid ? Solver::solve(d, lo, s, work, kSolverWave, o) : 0;
#pragma unroll
  for (int k = 0; k < Solver::kMaxSolutions; ++k)
    if (k >= count)
#pragma unroll
      for (int i = 0; i < Solver::kWidth; ++i) o[Solver::kWidth * k + i] = NAN;
  out_count[h] = count;
}

// samples (n_prob, n_hyp, kSample) -> out (n_prob, n_hyp, kMaxSolutions, kWidth), out_count (n_prob, n_hyp).  Nothing to do is
// VC_OK whatever the pointers are.
template <typename Solver>
int launch_minimal_solver(typename Solver::Data d, const int32_t* offsets, int n_prob, const int32_t* samples, int n_hyp,
                          double* out, int32_t* out_count, vc_stream_t stream) {
  if (n_prob < 0 || n_hyp < 0) return VC_ERR_INVALID_ARG;
  if (n_prob == 0 || n_hyp == 0) return VC_OK;
  if (!Solver::usable(d) || !offsets || !samples || !out || !out_count) return VC_ERR_INVALID_ARG;
  const long long total = (long long)n_prob * n_hyp;
  const long long blocks = (total + kSolverWave - 1) / kSolverWave;
  if (blocks > 2147483647LL) return VC_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(minimal_solver_kernel<Solver>, dim3((unsigned)blocks), dim3(kSolverWave), 0, (hipStream_t)stream, d, offsets,
                     total, samples, n_hyp, out, out_count);
  return check_launch();
}

}  // namespace vc
