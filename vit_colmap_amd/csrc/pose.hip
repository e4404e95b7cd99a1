// Two-view relative pose (gfx950): every inlier of every pair is triangulated under each of the pair's
// (at most four) pose candidates (R, t), X2 = R X1 + t; the candidate with most points in front of both cameras wins (the
// lowest slot on ties), and the median triangulation angle of its in-front points is selected exactly.  One launch for all
// pairs, in the ragged layout of vc_two_view_score / vc_essential_5pt.  Specification: tests/util_pose.py — float64 in
// exactly its order of single operations (the library is built with -ffp-contract=off), so counts, choice and midpoints
// equal the specification's bit for bit; only atan2 is another implementation.
//
// One workgroup of four waves per pair.  Phase 1: wave w counts the in-front points of candidate w, lanes striding over
// the inliers, ballot + popcount.  Phase 2: all 256 threads triangulate under the winner, write the midpoints and one
// order-preserving 64-bit key per inlier (all ones where the point is not in front, which sorts last).  Phase 3: the median
// by a byte-wise radix select over the keys (eight passes of a 256-bin LDS histogram per selected rank; no sort).  The keys
// of a pair of at most kLdsKeys inliers stay in LDS; a larger pair keeps them in the caller's workspace.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/vitcolmap_hip.h"
#include "common.h"

namespace {

constexpr int kThreads = 256;      // four waves: one per candidate in phase 1; 256 = the histogram's bins
constexpr int kLdsKeys = 4096;     // inliers per pair whose keys stay in LDS (32 KiB)
constexpr unsigned long long kNotInFront = ~0ull;

struct Cand {
  double r00, r01, r02, r10, r11, r12, r20, r21, r22, t0, t1, t2;
  bool used;                       // slot filled (no NaN in the first element) and t != 0
};

__device__ __forceinline__ Cand load_cand(const double* __restrict__ c) {
  Cand k;
  k.r00 = c[0], k.r01 = c[1], k.r02 = c[2], k.r10 = c[3], k.r11 = c[4], k.r12 = c[5], k.r20 = c[6], k.r21 = c[7], k.r22 = c[8];
  k.t0 = c[9], k.t1 = c[10], k.t2 = c[11];
  k.used = !(k.r00 != k.r00) && (k.t0 != 0.0 || k.t1 != 0.0 || k.t2 != 0.0);
  return k;
}

// least-squares depths of d2 x2 = d1 R x1 + t along the rays x1 = (x, y, 1), x2 = (u, v, 1); true iff the point is in front
__device__ __forceinline__ bool depths(const Cand& k, double x, double y, double u, double v, double& d1, double& d2) {
  const double a0 = k.r00 * x + k.r01 * y + k.r02;
  const double a1 = k.r10 * x + k.r11 * y + k.r12;
  const double a2 = k.r20 * x + k.r21 * y + k.r22;
  const double aa = a0 * a0 + a1 * a1 + a2 * a2;
  const double ab = a0 * u + a1 * v + a2;
  const double bb = u * u + v * v + 1.0;
  const double at = a0 * k.t0 + a1 * k.t1 + a2 * k.t2;
  const double bt = u * k.t0 + v * k.t1 + k.t2;
  const double det = aa * bb - ab * ab;
  d1 = (-bb * at + ab * bt) / det;
  d2 = (-ab * at + aa * bt) / det;
  return fabs(d1) < INFINITY && fabs(d2) < INFINITY && d1 > 0.0 && d2 > 0.0;      // NaN compares false
}

// non-negative and negative doubles alike -> keys that compare like the values
__device__ __forceinline__ unsigned long long key_of(double a) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(a);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double value_of(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k));
}

// The key of rank `rank` (0-based, ascending) among keys[0 .. n): one byte per pass from the top; every thread of the
// workgroup calls it with the same arguments.  hist: 256 bins; sel: {chosen bin, rank inside it}.
template <typename KeyPtr>
__device__ unsigned long long select_rank(KeyPtr keys, int n, unsigned rank, unsigned* hist, unsigned* sel) {
  const int tid = threadIdx.x, lane = tid & 63;
  unsigned long long prefix = 0;
  for (int pass = 0; pass < 8; ++pass) {
    const int shift = 56 - 8 * pass;
    const unsigned long long mask = pass == 0 ? 0ull : ~0ull << (shift + 8);
    hist[tid] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += kThreads) {
      const unsigned long long k = keys[i];
      if ((k & mask) == prefix) atomicAdd(&hist[(unsigned)(k >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid < 64) {                                    // wave 0: lane l owns bins 4l .. 4l + 3
      const unsigned h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2], h3 = hist[4 * lane + 3];
      const unsigned sum = h0 + h1 + h2 + h3;
      unsigned inc = sum;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const unsigned up = __shfl_up(inc, d);
        if (lane >= d) inc += up;
      }
      const unsigned exc = inc - sum;
      if (rank >= exc && rank < inc) {                 // exactly one lane: rank < the number of keys under the prefix
        unsigned r = rank - exc, bin = 4 * lane;
        if (r >= h0) {
          r -= h0, ++bin;
          if (r >= h1) {
            r -= h1, ++bin;
            if (r >= h2) r -= h2, ++bin;
          }
        }
        sel[0] = bin, sel[1] = r;
      }
    }
    __syncthreads();
    prefix |= (unsigned long long)sel[0] << shift;
    rank = sel[1];
  }
  return prefix;
}

template <typename KeyPtr>
__device__ double median_of_front(KeyPtr keys, int n, int n_front, unsigned* hist, unsigned* sel) {
  const double hi = value_of(select_rank(keys, n, (unsigned)(n_front / 2), hist, sel));
  if (n_front & 1) return hi;
  const double lo = value_of(select_rank(keys, n, (unsigned)(n_front / 2 - 1), hist, sel));
  return 0.5 * (lo + hi);
}

// phase 2 for the keys' address space at hand: midpoints, keys
template <typename KeyPtr>
__device__ void triangulate_best(const Cand& k, const double* __restrict__ pts_n, long long lo, int n, KeyPtr keys,
                                 double* __restrict__ out_points) {
  const double c0 = -(k.r00 * k.t0 + k.r10 * k.t1 + k.r20 * k.t2);      // the second camera's centre, -R' t
  const double c1 = -(k.r01 * k.t0 + k.r11 * k.t1 + k.r21 * k.t2);
  const double c2 = -(k.r02 * k.t0 + k.r12 * k.t1 + k.r22 * k.t2);
  for (int i = threadIdx.x; i < n; i += kThreads) {
    const double* q = pts_n + (lo + i) * 4;
    const double x = q[0], y = q[1], u = q[2], v = q[3];
    double d1, d2;
    const bool front = depths(k, x, y, u, v, d1, d2);
    double X0 = NAN, X1 = NAN, X2 = NAN;
    unsigned long long key = kNotInFront;
    if (front) {
      const double w0 = d2 * u - k.t0, w1 = d2 * v - k.t1, w2 = d2 - k.t2;
      X0 = 0.5 * (d1 * x + (k.r00 * w0 + k.r10 * w1 + k.r20 * w2));
      X1 = 0.5 * (d1 * y + (k.r01 * w0 + k.r11 * w1 + k.r21 * w2));
      X2 = 0.5 * (d1 + (k.r02 * w0 + k.r12 * w1 + k.r22 * w2));
      const double e0 = X0 - c0, e1 = X1 - c1, e2 = X2 - c2;
      const double k0 = X1 * e2 - X2 * e1, k1 = X2 * e0 - X0 * e2, k2 = X0 * e1 - X1 * e0;
      key = key_of(atan2(sqrt(k0 * k0 + k1 * k1 + k2 * k2), X0 * e0 + X1 * e1 + X2 * e2));
    }
    keys[i] = key;
    if (out_points) {
      double* o = out_points + (lo + i) * 3;
      o[0] = X0, o[1] = X1, o[2] = X2;
    }
  }
}

__global__ __launch_bounds__(kThreads) void two_view_pose_kernel(const double* __restrict__ pts_n, const int32_t* __restrict__ offsets,
                                                                 const double* __restrict__ cand, int32_t* __restrict__ out_front,
                                                                 int32_t* __restrict__ out_best, double* __restrict__ out_tri_angle,
                                                                 double* __restrict__ out_points, unsigned long long* ws_keys,
                                                                 unsigned long long ws_count) {
  __shared__ unsigned long long s_keys[kLdsKeys];
  __shared__ unsigned s_hist[kThreads];
  __shared__ unsigned s_sel[2];
  __shared__ int s_front[4];
  const int p = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long lo = offsets[p], hi = offsets[p + 1];
  const int n = lo >= 0 && hi > lo ? (int)(hi - lo) : 0;

  // ---- phase 1: candidate `wave`, whole waves (the ballot needs every lane; base is wave-uniform) ----
  {
    const Cand k = load_cand(cand + ((size_t)p * 4 + wave) * 12);
    int count = 0;
    if (k.used) {
      for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        bool front = false;
        if (i < n) {
          const double* q = pts_n + (lo + i) * 4;
          double d1, d2;
          front = depths(k, q[0], q[1], q[2], q[3], d1, d2);
        }
        count += __popcll(__ballot(front));
      }
    }
    if (lane == 0) {
      s_front[wave] = count;
      out_front[(size_t)p * 4 + wave] = count;
    }
  }
  __syncthreads();
  int best = 0, n_front = s_front[0];
  if (s_front[1] > n_front) best = 1, n_front = s_front[1];
  if (s_front[2] > n_front) best = 2, n_front = s_front[2];
  if (s_front[3] > n_front) best = 3, n_front = s_front[3];

  if (n_front == 0) {                                  // nothing in front of any candidate: slot 0, angle 0, no points
    if (out_points)
      for (long long i = (long long)tid; i < 3LL * n; i += kThreads) out_points[lo * 3 + i] = NAN;
    if (tid == 0) out_best[p] = 0, out_tri_angle[p] = 0.0;
    return;
  }
  // ---- phases 2 and 3 under the winner ----
  const Cand k = load_cand(cand + ((size_t)p * 4 + best) * 12);
  double median;
  if (n <= kLdsKeys) {
    triangulate_best(k, pts_n, lo, n, s_keys, out_points);
    median = median_of_front(s_keys, n, n_front, s_hist, s_sel);
  } else if ((unsigned long long)hi <= ws_count) {
    unsigned long long* keys = ws_keys + lo;
    triangulate_best(k, pts_n, lo, n, keys, out_points);
    median = median_of_front(keys, n, n_front, s_hist, s_sel);
  } else {                                             // the workspace does not hold this pair's keys: no result
    if (out_points)
      for (long long i = (long long)tid; i < 3LL * n; i += kThreads) out_points[lo * 3 + i] = NAN;
    if (tid == 0) out_best[p] = -1, out_tri_angle[p] = NAN;
    return;
  }
  if (tid == 0) out_best[p] = best, out_tri_angle[p] = median;
}

}  // namespace

extern "C" {

size_t vc_two_view_pose_workspace_bytes(int n_pairs, int total) {
  if (n_pairs < 0 || total < 0) return 0;
  return (size_t)total * sizeof(unsigned long long);
}

int vc_two_view_pose(const double* pts_n, const int32_t* offsets, int n_pairs, const double* cand, int32_t* out_front,
                     int32_t* out_best, double* out_tri_angle, double* out_points, void* workspace, size_t workspace_bytes,
                     vc_stream_t stream) {
  if (n_pairs < 0) return VC_ERR_INVALID_ARG;
  if (n_pairs == 0) return VC_OK;
  if (!pts_n || !offsets || !cand || !out_front || !out_best || !out_tri_angle) return VC_ERR_INVALID_ARG;
  if ((!workspace && workspace_bytes != 0) || ((uintptr_t)workspace) % 8 != 0) return VC_ERR_INVALID_ARG;
  hipLaunchKernelGGL(two_view_pose_kernel, dim3((unsigned)n_pairs), dim3(kThreads), 0, (hipStream_t)stream, pts_n, offsets, cand,
                     out_front, out_best, out_tri_angle, out_points, (unsigned long long*)workspace,
                     (unsigned long long)(workspace_bytes / sizeof(unsigned long long)));
  return vc::check_launch();
}

}  // extern "C"
