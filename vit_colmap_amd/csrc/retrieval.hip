// Retrieval matching for gfx950 (MI355X): the two device steps that choose which image pairs are matched at all
// (DESIGN.md §4.2h).  Specification: tests/util_retrieval.py (bit-exact target; everything here is integer).
//
//   vc_pool_descriptors_u8   sums[i][c] = sum over the rows r < counts[i] of desc[i][r][c], int32: one read of the
//                            descriptor blocks, several workgroups per image, partial sums joined by integer atomics
//                            (exact and order independent).
//   vc_retrieval_topk_i8     score[i][j] = q[i] . q[j] on v_mfma_i32_32x32x32_i8 and, per row, the k best valid j != i
//                            by (score descending, index ascending).  No n x n buffer: a wave owns 32 rows, walks the
//                            column tiles of its column range and keeps the rows' running lists in LDS; a second kernel
//                            merges the lists of the column ranges.
//
// Running top-k: (score, index) is packed into one 64-bit key, (score + 2^24) << 32 | (2^32 - 1 - index), so that "larger
// key" is "better neighbour" and keys of one row never tie; 0 is the empty slot.  A list of k <= 64 keys lives one key
// per lane: inserting is a ballot (how many keys are larger), a one-lane shift and a select.  A score is offered to its
// row's list only when it beats the row's current k-th key, which after the first tiles is rare.
//
// Assumption: a wave's 32 lists in LDS belong to that wave alone, and its lanes exchange data through them (lane k - 1
// writes a row's threshold, every lane reads it back) with no barrier.  That is sound because a wave issues its LDS
// instructions in program order and LDS completes them in that order, so a read issued after a write of the same wave
// sees it; `volatile` keeps the compiler from caching a list entry in a register or reordering the accesses.  No other
// wave touches these addresses, which is why the workgroup needs no __syncthreads().
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vitcolmap_hip.h"
#include "common.h"
#include "device.h"

namespace {

using vc::v16i;
using vc::v4i;
typedef unsigned long long u64;

__host__ __device__ inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

// ---------------------------------------------------------------------------------------
// pooling
// ---------------------------------------------------------------------------------------
constexpr int kPoolThreads = 256;
constexpr int kPoolTargetGroups = 2048;   // workgroups wanted in flight (8 per CU of a 256-CU part)
constexpr int kPoolMinRows = 32;          // rows per workgroup below which another split only adds atomics

template <int W> struct PoolWord;
template <> struct PoolWord<16> { typedef uint4 type; };
template <> struct PoolWord<4> { typedef uint32_t type; };
template <> struct PoolWord<1> { typedef uint8_t type; };

template <int W>
__device__ __forceinline__ void pool_add(int (&acc)[W], const typename PoolWord<W>::type& v) {
  if constexpr (W == 1) {
    acc[0] += (int)v;
  } else {
    uint32_t w[W / 4];
    if constexpr (W == 16) { w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w; } else { w[0] = v; }
#pragma unroll
    for (int i = 0; i < W / 4; ++i) {
      acc[4 * i + 0] += (int)(w[i] & 0xffu);
      acc[4 * i + 1] += (int)((w[i] >> 8) & 0xffu);
      acc[4 * i + 2] += (int)((w[i] >> 16) & 0xffu);
      acc[4 * i + 3] += (int)(w[i] >> 24);
    }
  }
}

// One workgroup sums rows [split * rows_per_split, +rows_per_split) of image blockIdx.x, cut at counts[image].
// W = bytes per load (d % W == 0, the block W-byte aligned).  A thread owns one W-byte column chunk and every
// rows_per_pass-th row, so a wave reads whole consecutive rows.
template <int W>
__global__ __launch_bounds__(kPoolThreads) void pool_kernel(const uint8_t* __restrict__ desc, const int32_t* __restrict__ counts,
                                                            int n_max, int d, int rows_per_split, int32_t* __restrict__ out) {
  typedef typename PoolWord<W>::type word_t;
  __shared__ int32_t sums[VC_MAX_DESC_DIM];
  const int img = blockIdx.x, tid = threadIdx.x;
  int cnt = counts[img];
  cnt = cnt < 0 ? 0 : (cnt > n_max ? n_max : cnt);          // never past the block
  const int r0 = blockIdx.y * rows_per_split;
  const int r1 = min(r0 + rows_per_split, cnt);
  if (r0 >= r1) return;                                      // (the whole workgroup)
  for (int c = tid; c < d; c += kPoolThreads) sums[c] = 0;
  __syncthreads();
  const int cpr = d / W;                                     // column chunks per row
  const int lanes_c = min(cpr, kPoolThreads);
  const int rows_per_pass = kPoolThreads / lanes_c;
  const int my_c = tid % lanes_c, my_r = tid / lanes_c;
  const uint8_t* base = desc + (size_t)img * n_max * d;
  if (my_r < rows_per_pass) {
    for (int cc = my_c; cc < cpr; cc += lanes_c) {
      int acc[W];
#pragma unroll
      for (int b = 0; b < W; ++b) acc[b] = 0;
      const uint8_t* col = base + (size_t)cc * W;
      int r = r0 + my_r;
      for (; r + 3 * rows_per_pass < r1; r += 4 * rows_per_pass) {   // four loads in flight
        const word_t v0 = *(const word_t*)(col + (size_t)r * d);
        const word_t v1 = *(const word_t*)(col + (size_t)(r + rows_per_pass) * d);
        const word_t v2 = *(const word_t*)(col + (size_t)(r + 2 * rows_per_pass) * d);
        const word_t v3 = *(const word_t*)(col + (size_t)(r + 3 * rows_per_pass) * d);
        pool_add<W>(acc, v0);
        pool_add<W>(acc, v1);
        pool_add<W>(acc, v2);
        pool_add<W>(acc, v3);
      }
      for (; r < r1; r += rows_per_pass) pool_add<W>(acc, *(const word_t*)(col + (size_t)r * d));
#pragma unroll
      for (int b = 0; b < W; ++b) atomicAdd(&sums[cc * W + b], acc[b]);
    }
  }
  __syncthreads();
  for (int c = tid; c < d; c += kPoolThreads) atomicAdd(&out[(size_t)img * d + c], sums[c]);
}

// ---------------------------------------------------------------------------------------
// top-k
// ---------------------------------------------------------------------------------------
constexpr int kTopkWaves = 4;                      // waves per workgroup, 32 rows each
constexpr int kTile = 32;                          // MFMA tile edge
constexpr int kRowsPerGroup = kTopkWaves * kTile;
constexpr int kMaxImages = 1 << 20;                // indices and n * k stay far inside 32 bits
constexpr int kMaxSplits = 16;                     // column ranges per row tile (bounds the workspace: 16 n k keys)
constexpr int kTargetGroups = 512;
constexpr int kScoreBias = 1 << 24;                // |score| <= 127^2 * 1024 < 2^24
static_assert(127 * 127 * VC_MAX_DESC_DIM < kScoreBias, "biased scores must stay positive");
static_assert(VC_MAX_NEIGHBOURS <= 64, "a list is one key per lane");

__device__ __forceinline__ u64 make_key(int score, int j) {
  return ((u64)(uint32_t)(score + kScoreBias) << 32) | (u64)(0xFFFFFFFFu - (uint32_t)j);
}

// `mine` = the list's key of this lane (descending over the lanes, 0 from lane k on) -> the list with `key` inserted
// and the last key dropped.  Wave-uniform `key`; a key below the whole list changes nothing.
__device__ __forceinline__ u64 list_insert(u64 mine, u64 key, int lane, int k) {
  const int pos = __popcll(__ballot(mine > key));
  const u64 up = __shfl_up(mine, 1);
  const u64 v = lane < pos ? mine : (lane == pos ? key : up);
  return lane < k ? v : 0;
}

// Column tiles per column range, and the number of ranges, for n images: enough workgroups for the chip at small n,
// one range at large n.  A function of n alone, so the workspace size needs no device.
__host__ __device__ inline int col_tiles_per_split(int n) {
  const int want = min(kMaxSplits, max(1, kTargetGroups / ceil_div(n, kRowsPerGroup)));
  return ceil_div(ceil_div(n, kTile), want);
}
__host__ __device__ inline int splits_of(int n) { return ceil_div(ceil_div(n, kTile), col_tiles_per_split(n)); }

// grid (row groups, column ranges).  partial [splits][n][k] keys, descending, 0 = empty.
__global__ __launch_bounds__(kTopkWaves * 64) void topk_kernel(const int8_t* __restrict__ q, const int32_t* __restrict__ valid, int n,
                                                               int d_pad, int k, int tiles_per_split, u64* __restrict__ partial) {
  extern __shared__ u64 topk_lists[];                         // [waves][32 rows][k]
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, h = lane >> 5, c = lane & 31;
  const int R0 = (blockIdx.x * kTopkWaves + wave) * kTile;
  if (R0 >= n) return;                                        // (the waves share no barrier)
  volatile u64* lists = topk_lists + (size_t)wave * kTile * k;
  for (int i = lane; i < kTile * k; i += 64) lists[i] = 0;
  const int ks = d_pad / 32;
  const int ct0 = blockIdx.y * tiles_per_split;
  const int ct1 = min(ct0 + tiles_per_split, ceil_div(n, kTile));
  // operand fragment of lane 32 h + c at k-step kk: bytes [32 kk + 16 h, +16) of row (tile base + c); rows past n read
  // row n - 1 (their scores are never used)
  const int8_t* ap = q + (size_t)min(R0 + c, n - 1) * d_pad + 16 * h;
  for (int ct = ct0; ct < ct1; ++ct) {
    const int j = ct * kTile + c;
    const int jc = min(j, n - 1);
    const int8_t* bp = q + (size_t)jc * d_pad + 16 * h;
    const bool j_ok = j < n && valid[jc] != 0;
    v16i acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0;
    int kk = 0;
    for (; kk + 4 <= ks; kk += 4) {                            // eight loads in flight ahead of four MFMAs
      v4i a[4], b[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        a[u] = *(const v4i*)(ap + 32 * (kk + u));
        b[u] = *(const v4i*)(bp + 32 * (kk + u));
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[u], b[u], acc, 0, 0, 0);
    }
    for (; kk < ks; ++kk) {
      const v4i a = *(const v4i*)(ap + 32 * kk);
      const v4i b = *(const v4i*)(bp + 32 * kk);
      acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, acc, 0, 0, 0);
    }
    // acc[4 q + i] = score of row 8 q + 4 h + i against column c
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rl0 = 8 * (r >> 2) + (r & 3);
      const int rl = rl0 + 4 * h;
      const u64 key = (j_ok && j != R0 + rl && R0 + rl < n) ? make_key(acc[r], j) : 0;   // rows past n offer nothing
      u64 pending = __ballot(key > lists[rl * k + k - 1]);
      while (pending) {
        const int src = __ffsll((long long)pending) - 1;
        pending &= pending - 1;
        const u64 cand = __shfl(key, src);
        const int row = rl0 + 4 * (src >> 5);
        if (cand > lists[row * k + k - 1]) {                  // the row's threshold may have risen since the ballot
          const u64 mine = list_insert(lane < k ? lists[row * k + lane] : 0, cand, lane, k);
          if (lane < k) lists[row * k + lane] = mine;
        }
      }
    }
  }
  u64* out = partial + ((size_t)blockIdx.y * n + R0) * k;
  const int rows = min(kTile, n - R0);
  for (int i = lane; i < rows * k; i += 64) out[i] = lists[i];
}

// One wave per row: the k best keys over the row's `splits` partial lists -> index and score.
__global__ __launch_bounds__(256) void topk_merge_kernel(const u64* __restrict__ partial, const int32_t* __restrict__ valid, int n, int k,
                                                         int splits, int32_t* __restrict__ out_idx, int32_t* __restrict__ out_score) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  u64 mine = 0;
  if (valid[row] != 0) {
    for (int s = 0; s < splits; ++s) {
      const u64 theirs = lane < k ? partial[((size_t)s * n + row) * k + lane] : 0;
      for (int e = 0; e < k; ++e) {
        const u64 cand = __shfl(theirs, e);
        if (cand == 0 || cand <= __shfl(mine, k - 1)) break;  // descending: nothing further of this list gets in
        mine = list_insert(mine, cand, lane, k);
      }
    }
  }
  if (lane < k) {
    out_idx[(size_t)row * k + lane] = mine ? (int32_t)(0xFFFFFFFFu - (uint32_t)mine) : -1;
    out_score[(size_t)row * k + lane] = mine ? (int32_t)(uint32_t)(mine >> 32) - kScoreBias : INT32_MIN;
  }
}

bool topk_shape_supported(int n, int d_pad, int k) {
  return n >= 1 && n <= kMaxImages && d_pad >= 32 && d_pad <= VC_MAX_DESC_DIM && d_pad % 32 == 0 && k >= 1 && k <= VC_MAX_NEIGHBOURS;
}

}  // namespace

extern "C" {

int vc_pool_descriptors_u8(const uint8_t* desc, const int32_t* counts, int n_images, int n_max, int d, int32_t* out_sums,
                           vc_stream_t stream) {
  if (n_images < 0 || n_max <= 0 || d <= 0) return VC_ERR_INVALID_ARG;
  if (n_images == 0) return VC_OK;
  if (!desc || !counts || !out_sums) return VC_ERR_INVALID_ARG;
  if (n_max > VC_MAX_KEYPOINTS || d > VC_MAX_DESC_DIM) return VC_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const hipError_t e = hipMemsetAsync(out_sums, 0, (size_t)n_images * d * sizeof(int32_t), s);
  if (e != hipSuccess) return vc::fail(e);
  const int w = (d % 16 == 0 && (uintptr_t)desc % 16 == 0) ? 16 : ((d % 4 == 0 && (uintptr_t)desc % 4 == 0) ? 4 : 1);
  // grid.y is the row split; images beyond one grid's x limit go in further launches
  const int splits = max(1, min(ceil_div(kPoolTargetGroups, n_images), ceil_div(n_max, kPoolMinRows)));
  const int rows_per_split = ceil_div(n_max, splits);
  const size_t image_bytes = (size_t)n_max * d;
  for (int i0 = 0; i0 < n_images; i0 += 65535) {
    const dim3 grid(min(65535, n_images - i0), splits);
    const uint8_t* dp = desc + (size_t)i0 * image_bytes;
    const int32_t* cp = counts + i0;
    int32_t* op = out_sums + (size_t)i0 * d;
    if (w == 16) hipLaunchKernelGGL(pool_kernel<16>, grid, dim3(kPoolThreads), 0, s, dp, cp, n_max, d, rows_per_split, op);
    else if (w == 4) hipLaunchKernelGGL(pool_kernel<4>, grid, dim3(kPoolThreads), 0, s, dp, cp, n_max, d, rows_per_split, op);
    else hipLaunchKernelGGL(pool_kernel<1>, grid, dim3(kPoolThreads), 0, s, dp, cp, n_max, d, rows_per_split, op);
  }
  return vc::check_launch();
}

size_t vc_retrieval_workspace_bytes(int n, int d_pad, int k) {
  if (!topk_shape_supported(n, d_pad, k)) return 0;
  return (size_t)splits_of(n) * n * k * sizeof(u64);
}

int vc_retrieval_topk_i8(const int8_t* q, const int32_t* valid, int n, int d_pad, int k, int32_t* out_idx, int32_t* out_score,
                         void* workspace, size_t workspace_bytes, vc_stream_t stream) {
  if (n < 0 || d_pad <= 0 || k < 1) return VC_ERR_INVALID_ARG;
  if (n == 0) return VC_OK;
  if (!q || !valid || !out_idx || !out_score || !workspace) return VC_ERR_INVALID_ARG;
  if (d_pad % 32 != 0 || (uintptr_t)q % 16 != 0 || (uintptr_t)workspace % 8 != 0) return VC_ERR_INVALID_ARG;
  if (!topk_shape_supported(n, d_pad, k)) return VC_ERR_UNSUPPORTED;
  if (workspace_bytes < vc_retrieval_workspace_bytes(n, d_pad, k)) return VC_ERR_WORKSPACE;
  const int lds_bytes = kTopkWaves * kTile * k * (int)sizeof(u64);
  static vc::PerDeviceOnce configured;
  if (int st = vc::allow_dynamic_lds(configured, kTopkWaves * kTile * VC_MAX_NEIGHBOURS * (int)sizeof(u64), topk_kernel)) return st;
  hipStream_t s = (hipStream_t)stream;
  u64* partial = (u64*)workspace;
  const int splits = splits_of(n);
  hipLaunchKernelGGL(topk_kernel, dim3(ceil_div(n, kRowsPerGroup), splits), dim3(kTopkWaves * 64), lds_bytes, s, q, valid, n, d_pad, k,
                     col_tiles_per_split(n), partial);
  hipLaunchKernelGGL(topk_merge_kernel, dim3(ceil_div(n, 4)), dim3(256), 0, s, partial, valid, n, k, splits, out_idx, out_score);
  return vc::check_launch();
}

}  // extern "C"
