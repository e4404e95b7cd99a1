// Focal length from the verified pairs (gfx950): the self-calibration cost of Mendonça and Cipolla for every
// UNCALIBRATED pair of a camera under every candidate focal length of a call.  For a camera that is the same in both images
// K' F K is an essential matrix, whose two non-zero singular values are equal; vc_focal_cost returns, per camera and
// candidate scale r on the stored focal length(s), the inlier-weighted mean of (s1 - s2) / (s1 + s2) over the camera's pairs.
// The grid search around it is host code (vit_colmap_amd/matching/focal.py).  Specification: tests/util_focal.py.
//
// float64.  focal_pair_kernel: one lane per pair of a chunk of kFocalChunk pairs, one workgroup per (chunk, block of
// kFocalCands candidates).  A lane forms A = T' F T once, keeps its nine entries in registers across its candidates and
// leaves w * cost per candidate in LDS; then one lane per (camera, candidate) adds the chunk's terms of its camera in pair
// order and writes the partial sum it alone owns.  focal_sum_kernel: one lane per (camera, candidate) adds the partial sums in
// chunk order and divides by the weight.  No atomics: the order of every sum is fixed, so two calls return the same bytes and
// so does the host build (tools/focal_cost_host.cpp includes this file and runs the same two loops).
// Every operation is a single float64 one in the order include/vitcolmap_hip.h states (-ffp-contract=off); sqrt, the only
// library call, is correctly rounded on both sides.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/vitcolmap_hip.h"
#include "common.h"

namespace {

constexpr int kFocalChunk = 256;                // FOCAL_CHUNK: pairs per partial sum, and the lanes of a workgroup
constexpr int kFocalCands = 16;                 // candidates per workgroup of the first kernel
constexpr int kFocalPad = 2;                   // doubles: the 16 candidates of one pair fall into 16 different LDS bank pairs
constexpr int kFocalCamLanes = kFocalChunk / kFocalCands;   // cameras reduced at a time in the second half of that kernel
constexpr size_t kFocalMaxPartial = (size_t)1 << 30;        // bytes of partial sums a call may ask for

// F (9, row-major) and the principal point -> A = T' F T at unit Frobenius norm, T = [[1, 0, cx], [0, 1, cy], [0, 0, 1]];
// false where the norm is not finite or is 0 (such a pair has weight 0).
__host__ __device__ __forceinline__ bool focal_pair_matrix(const double* f, double cx, double cy, double* a) {
  const double g2 = f[0] * cx + f[1] * cy + f[2], g5 = f[3] * cx + f[4] * cy + f[5], g8 = f[6] * cx + f[7] * cy + f[8];
  a[0] = f[0], a[1] = f[1], a[2] = g2;
  a[3] = f[3], a[4] = f[4], a[5] = g5;
  a[6] = cx * f[0] + cy * f[3] + f[6];
  a[7] = cx * f[1] + cy * f[4] + f[7];
  a[8] = cx * g2 + cy * g5 + g8;
  double n2 = 0.0;
  for (int i = 0; i < 9; ++i) n2 = n2 + a[i] * a[i];
  const double norm = sqrt(n2);
  const bool ok = norm > 0.0 && norm <= 1.7976931348623157e308;   // finite and not 0; false for NaN
  for (int i = 0; i < 9; ++i) a[i] = a[i] / norm;
  return ok;
}

// A at unit norm, d = (d0, d1, 1) -> (s1 - s2) / (s1 + s2) of E = diag(d) A diag(d).  E has rank 2, so the squares of s1 and s2
// are the roots of x^2 - c2 x + c1 with c2 = tr(E'E) and c1 = (tr(E'E)^2 - tr((E'E)^2)) / 2.
__host__ __device__ __forceinline__ double focal_pair_cost(const double* a, double d0, double d1) {
  const double d[3] = {d0, d1, 1.0};
  double e[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) e[3 * i + j] = (d[i] * a[3 * i + j]) * d[j];
  double c2 = 0.0;
  for (int i = 0; i < 9; ++i) c2 = c2 + e[i] * e[i];
  double m2 = 0.0;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const double m = e[i] * e[j] + e[3 + i] * e[3 + j] + e[6 + i] * e[6 + j];
      m2 = m2 + m * m;
    }
  const double c1 = (c2 * c2 - m2) * 0.5;
  double disc = c2 * c2 - 4.0 * c1;
  disc = disc > 0.0 ? disc : 0.0;
  const double l1 = (c2 + sqrt(disc)) * 0.5;
  double l2 = c1 / l1;
  l2 = l2 > 0.0 ? l2 : 0.0;                                   // also for NaN
  const double s1 = sqrt(l1), s2 = sqrt(l2);
  return (s1 - s2) / (s1 + s2);
}

__host__ __device__ __forceinline__ bool focal_ratio_ok(double r) { return r > 0.0 && r <= 1.7976931348623157e308; }

// The weighted mean of a camera under a candidate; every NaN (a ratio that is not finite and positive, a camera without weight,
// a cost that is one) leaves as the one NaN of the NAN macro, so that host and device return the same bytes there too.
__host__ __device__ __forceinline__ double focal_mean(double sum, double sum_w, double ratio) {
  const double mean = sum / sum_w;
  return focal_ratio_ok(ratio) && mean == mean ? mean : NAN;
}

// Pair p of the call -> its camera slot (-1: the pair does not count), A and its weight.  The slot is checked before it indexes
// the camera table; a weight that is not finite and positive, or an A without a norm, makes the pair not count.
__host__ __device__ __forceinline__ int focal_load_pair(const double* F, const int32_t* pair_cam, const double* w, const double* cams,
                                                        int n_cams, long long p, double* a, double& weight) {
  const int slot = pair_cam[p];
  weight = 0.0;
  if (slot < 0 || slot >= n_cams) return -1;
  const double wp = w[p];
  if (!focal_ratio_ok(wp)) return -1;
  double f[9];
  for (int i = 0; i < 9; ++i) f[i] = F[9 * p + i];
  const double* c = cams + 4 * (long long)slot;
  if (!focal_pair_matrix(f, c[2], c[3], a)) return -1;
  weight = wp;
  return slot;
}

// grid (chunks, ceil(n_cand / kFocalCands)), kFocalChunk lanes.  part_cost [chunks][n_cams][n_cand], part_weight [chunks][n_cams]
// (written by the workgroups of candidate block 0).
__global__ __launch_bounds__(kFocalChunk) void focal_pair_kernel(const double* __restrict__ F, const int32_t* __restrict__ pair_cam,
                                                                 const double* __restrict__ w, int n_pairs,
                                                                 const double* __restrict__ cams, int n_cams,
                                                                 const double* __restrict__ ratios, int n_cand,
                                                                 double* __restrict__ part_cost, double* __restrict__ part_weight) {
  __shared__ double s_term[kFocalCands][kFocalChunk + kFocalPad];
  __shared__ double s_weight[kFocalChunk];
  __shared__ int s_slot[kFocalChunk];
  const int lane = threadIdx.x, chunk = blockIdx.x, k0 = blockIdx.y * kFocalCands;
  const long long p = (long long)chunk * kFocalChunk + lane;
  double a[9], weight = 0.0;
  int slot = -1;
  if (p < n_pairs) slot = focal_load_pair(F, pair_cam, w, cams, n_cams, p, a, weight);
  s_slot[lane] = slot;
  s_weight[lane] = weight;
  if (slot >= 0) {
    const double fx0 = cams[4 * (long long)slot], fy0 = cams[4 * (long long)slot + 1];
    for (int k = 0; k < kFocalCands; ++k) {
      double term = 0.0;
      if (k0 + k < n_cand) {
        const double r = ratios[k0 + k];
        if (focal_ratio_ok(r)) term = weight * focal_pair_cost(a, r * fx0, r * fy0);
      }
      s_term[k][lane] = term;
    }
  }
  __syncthreads();
  // one owner per (camera, candidate): the chunk's terms of the camera in pair order
  const int k = lane % kFocalCands;
  for (int c = lane / kFocalCands; c < n_cams; c += kFocalCamLanes) {
    double sum = 0.0, sum_w = 0.0;
    for (int q = 0; q < kFocalChunk; ++q) {
      if (s_slot[q] == c) {
        sum = sum + s_term[k][q];
        sum_w = sum_w + s_weight[q];
      }
    }
    if (k0 + k < n_cand) part_cost[((long long)chunk * n_cams + c) * n_cand + k0 + k] = sum;
    if (blockIdx.y == 0 && k == 0) part_weight[(long long)chunk * n_cams + c] = sum_w;
  }
}

// one lane per (camera, candidate): the partial sums in chunk order, divided by the camera's weight
__global__ __launch_bounds__(kFocalChunk) void focal_sum_kernel(const double* __restrict__ part_cost, const double* __restrict__ part_weight,
                                                                int n_chunks, int n_cams, const double* __restrict__ ratios, int n_cand,
                                                                double* __restrict__ out_cost, double* __restrict__ out_weight) {
  const long long i = (long long)blockIdx.x * kFocalChunk + threadIdx.x;
  if (i >= (long long)n_cams * n_cand) return;
  const int c = (int)(i / n_cand), k = (int)(i % n_cand);
  double sum = 0.0, sum_w = 0.0;
  for (int chunk = 0; chunk < n_chunks; ++chunk) {
    sum = sum + part_cost[((long long)chunk * n_cams + c) * n_cand + k];
    sum_w = sum_w + part_weight[(long long)chunk * n_cams + c];
  }
  out_cost[i] = focal_mean(sum, sum_w, ratios[k]);
  if (k == 0) out_weight[c] = sum_w;
}

}  // namespace

extern "C" {

int vc_focal_cost(const double* F, const int32_t* pair_cam, const double* w, int n_pairs, const double* cams, int n_cams,
                  const double* ratios, int n_cand, double* out_cost, double* out_weight, vc_stream_t stream) {
  if (n_pairs < 0 || n_cams < 0 || n_cand < 0) return VC_ERR_INVALID_ARG;
  if (n_pairs == 0 || n_cand == 0) return VC_OK;
  if (!F || !pair_cam || !w || !ratios) return VC_ERR_INVALID_ARG;
  if (n_cams == 0) return VC_OK;                               // no row to write
  if (!cams || !out_cost || !out_weight) return VC_ERR_INVALID_ARG;
  const hipStream_t s = (hipStream_t)stream;
  const int n_chunks = (int)(((long long)n_pairs + kFocalChunk - 1) / kFocalChunk);
  const int cand_blocks = (n_cand + kFocalCands - 1) / kFocalCands;
  if (cand_blocks > 65535) return VC_ERR_UNSUPPORTED;         // the grid's second dimension
  const size_t rows = (size_t)n_chunks * (size_t)n_cams;
  if (rows > kFocalMaxPartial / sizeof(double) / ((size_t)n_cand + 1)) return VC_ERR_WORKSPACE;
  double* part = nullptr;
  hipError_t e = hipMallocAsync((void**)&part, rows * ((size_t)n_cand + 1) * sizeof(double), s);
  if (e != hipSuccess) return vc::fail(e);
  double* part_weight = part + rows * (size_t)n_cand;
  hipLaunchKernelGGL(focal_pair_kernel, dim3((unsigned)n_chunks, (unsigned)cand_blocks), dim3(kFocalChunk), 0, s, F, pair_cam, w, n_pairs,
                     cams, n_cams, ratios, n_cand, part, part_weight);
  e = hipGetLastError();
  if (e == hipSuccess) {
    const long long cells = (long long)n_cams * n_cand;
    hipLaunchKernelGGL(focal_sum_kernel, dim3((unsigned)((cells + kFocalChunk - 1) / kFocalChunk)), dim3(kFocalChunk), 0, s, part,
                       part_weight, n_chunks, n_cams, ratios, n_cand, out_cost, out_weight);
    e = hipGetLastError();
  }
  const hipError_t freed = hipFreeAsync(part, s);
  if (e != hipSuccess) return vc::fail(e);
  if (freed != hipSuccess) return vc::fail(freed);
  return VC_OK;
}

}  // extern "C"
