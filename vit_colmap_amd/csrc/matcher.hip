// Exhaustive descriptor matcher for gfx950 (MI355X): int8 MFMA similarity tiles with the
// per-row / per-column top-2 searches, the angle + ratio tests and the cross check fused
// into one kernel per image pair.
//
// Replaces the per-pair arithmetic of pycolmap.match_exhaustive (reference call site
// vit_colmap/pipeline/run_pipeline.py:351-363, options vit_colmap/utils/config.py:64-96).
// Specification: oracle/matcher_oracle.py (bit-exact target).
// Guided matching (vc_match_pairs_guided_u8, COLMAP's `guided_matching`): the same search on similarities masked by the
// pair's fundamental matrix or homography, the geometric test fused into the tile epilogue.
//
// Data layout
//   prepared image = n_tiles x KS fragments of 1 KiB + n_tiles*32 int32 row sums, where
//   fragment (tile, kk) holds, for lane l = 32*h + c, the 16 bytes [32*kk + 16*h, +16) of
//   descriptor row 32*tile + c, each byte XOR 0x80 (uint8 -> biased int8).  That is exactly
//   the A/B operand of v_mfma_i32_32x32x32_i8, so a fragment is one coalesced 1 KiB
//   global_load_lds (B side, shared by the workgroup through LDS) or one 16 B/lane register
//   load (A side, kept in VGPRs for a whole pass).
//   s(i,j) = sum (a-128)(b-128) + 128*(rowsum_a[i] + rowsum_b[j]) - 16384*D   (exact, int32);
//   the correction is folded into the accumulator's initial value.
//
// Top-2 without index registers: a similarity fits 26 bits (255^2 * 1024 < 2^26), so
//   key = (s << 6) | (63 - t)   with t = column-tile number (row search) or the lane's local
//   row number (column search) orders by (s desc, index asc) under one unsigned max, and
//   best' = max(best, key), second' = med3(best, second, key) is the whole update.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vitcolmap_hip.h"
#include "common.h"
#include "device.h"

namespace {

using vc::v16i;
using vc::v4i;
typedef unsigned int u32;

constexpr int kWaves = 8;                    // waves per workgroup: one workgroup per CU
constexpr int kThreads = kWaves * 64;
constexpr int kTile = 32;                    // MFMA tile edge
static_assert(VC_MAX_KEYPOINTS <= 64 * 32, "the row search packs the column-tile number into 6 bits");
constexpr int kFragBytes = 1024;             // 64 lanes x 16 B

__host__ __device__ constexpr int ceil_div(int a, int b) { return (a + b - 1) / b; }
// 32-row tiles per prepared image, rounded up to a whole pass of the pair kernel (8 waves x 2
// row tiles) so that every tile index a workgroup touches exists; the extra tiles hold
// neutral rows (all-zero descriptors: similarity 0 with everything).
__host__ __device__ constexpr int tiles_of(int n_max) { return ceil_div(ceil_div(n_max, kTile), 16) * 16; }
__host__ __device__ inline int ksteps_of(int d) { return ceil_div(d, 32); }
// K steps in the "head" of a descriptor for the exact early-out of pair2_kernel (== ks: no early-out for that length)
constexpr int kHeadSteps12 = 4;   // head k-steps of a 384-byte descriptor (a multiple of the window below)
constexpr int kWindow12 = 4;      // B window registers (fragments) at KS = 12
__host__ __device__ constexpr int head_steps_of(int ks) { return ks == 12 ? kHeadSteps12 : (ks == 8 ? 4 : ks); }   // multiples of BWindow::NB
// prepared image = fragments | row sums int32 [n_pad] | packed head / tail row sums int32 [n_pad] | per-tile tail norm bounds int32 [n_tiles]
//   packed word   = (head << 16) | tail: sums of the row's bytes over the first head_steps_of(ks) * 32 dimensions and over the rest
//                   (field widths: packed_sums_fit() below, asserted for every length the early-out kernels are built for)
//   tail norm     = max over the tile's 32 rows of ceil(sqrt(sum of squared bytes over the remaining dimensions))
__host__ __device__ constexpr bool packed_sums_fit(int ks) {   // head < 2^15 (the word stays positive), tail < 2^16
  return head_steps_of(ks) == ks || (255 * 32 * head_steps_of(ks) < (1 << 15) && 255 * 32 * (ks - head_steps_of(ks)) < (1 << 16));
}
static_assert(packed_sums_fit(8) && packed_sums_fit(12), "head / tail row sums must fit the packed word");
__host__ __device__ inline int packed_head(int word) { return word >> 16; }
__host__ __device__ inline int packed_tail(int word) { return word & 0xffff; }
__host__ __device__ inline size_t image_bytes(int n_tiles, int ks) {
  return (size_t)n_tiles * ks * kFragBytes + (size_t)n_tiles * kTile * sizeof(int32_t) * 2 + (size_t)n_tiles * sizeof(int32_t);
}

// ---------------------------------------------------------------------------------------
// cross-lane helpers (wave64; reductions run inside each 32-lane half)
// ---------------------------------------------------------------------------------------
template <int CTRL>
__device__ inline u32 dpp_mov(u32 v) {
  return (u32)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, false);
}
__device__ inline u32 umax(u32 a, u32 b) { return a > b ? a : b; }
__device__ inline u32 umin(u32 a, u32 b) { return a < b ? a : b; }
__device__ inline u32 umed3(u32 a, u32 b, u32 c) {
  // median of three: with a >= b it is the new runner-up after seeing c
  return umax(umin(a, b), umin(umax(a, b), c));
}
// max over the 32 lanes that share lane>>5; every lane of the half receives it
__device__ inline u32 half_max(u32 v) {
  v = umax(v, dpp_mov<0x128>(v));  // row_ror:8
  v = umax(v, dpp_mov<0x124>(v));  // row_ror:4
  v = umax(v, dpp_mov<0x122>(v));  // row_ror:2
  v = umax(v, dpp_mov<0x121>(v));  // row_ror:1
  v = umax(v, (u32)__builtin_amdgcn_ds_swizzle((int)v, 0x401F));  // lane ^ 16
  return v;
}

// ---------------------------------------------------------------------------------------
// theta / accept — identical arithmetic to oracle/matcher_oracle.c
// ---------------------------------------------------------------------------------------
__host__ __device__ inline float theta(int s) {
  float x = (float)s * (1.0f / (512.0f * 512.0f));
  x = x > 1.0f ? 1.0f : x;
  return (float)acos((double)x);
}

__device__ inline bool accept_dev(int best, int second, float max_ratio, float max_distance) {
  if (best <= 0) return false;
  const float tb = theta(best);
  if (tb > max_distance) return false;
  const float ts = theta(second);
  if (tb >= max_ratio * ts) return false;
  return true;
}

// theta(s) for every s in [0, 512^2], generated at build time by gen_theta_table.c (same expression as
// theta(); compared entry by entry on the device and against the oracle in tests/test_matcher_gpu.py).
// With it the acceptance tests of a row are two L2-resident loads, a multiply and two compares: no
// double-precision acos in the pair kernel, hence no register pressure from it around the pair loop.
__device__ const uint32_t kThetaBits[512 * 512 + 1] = {
#include "theta_table.inc"
};
__device__ __forceinline__ float theta_tab(int s) {
  return __uint_as_float(kThetaBits[umin((u32)s, 512u * 512u)]);   // (unsigned clamp: no index is ever out of the table)
}
// accept_dev with table angles.  `s_low` (relevance_threshold): a best <= s_low is rejected whatever the
// runner-up is, so those rows never touch the table (on non-matching image pairs that is every row).
__device__ __forceinline__ bool accept_tab(int best, int second, float max_ratio, float max_distance, int s_low) {
  if (best <= 0 || best <= s_low) return false;
  const float tb = theta_tab(best);
  const float ts = theta_tab(second);
  if (tb > max_distance) return false;
  if (tb >= max_ratio * ts) return false;
  return true;
}
// the two rules as finalise_pair takes them: ok = accept(best, second)
struct AcceptAcos {
  float max_ratio, max_distance;
  __device__ __forceinline__ bool operator()(int best, int second) const { return accept_dev(best, second, max_ratio, max_distance); }
};
struct AcceptTable {
  float max_ratio, max_distance;
  int s_low;
  __device__ __forceinline__ bool operator()(int best, int second) const {
    return accept_tab(best, second, max_ratio, max_distance, s_low);
  }
};

// ---------------------------------------------------------------------------------------
// prepare: uint8 [n_images][n_max][d] -> fragment-major biased int8 + row sums
// ---------------------------------------------------------------------------------------
__global__ void prepare_kernel(const uint8_t* __restrict__ desc, const int32_t* __restrict__ counts,
                               int n_max, int d, int n_tiles, int ks, uint8_t* __restrict__ prepared) {
  const int img = blockIdx.y;
  const int tile = blockIdx.x;
  const int count = counts ? min(max(counts[img], 0), n_max) : n_max;
  const uint8_t* src = desc + (size_t)img * n_max * d;
  uint8_t* dst_img = prepared + (size_t)img * image_bytes(n_tiles, ks);
  uint8_t* dst = dst_img + (size_t)tile * ks * kFragBytes;
  int32_t* rowsum = (int32_t*)(dst_img + (size_t)n_tiles * ks * kFragBytes) + tile * kTile;
  const bool vec_ok = (d % 16 == 0) && (((uintptr_t)src) % 16 == 0);

  for (int chunk = threadIdx.x; chunk < ks * 64; chunk += blockDim.x) {
    const int kk = chunk >> 6, lane = chunk & 63;
    const int c = lane & 31, h = lane >> 5;
    const int row = tile * kTile + c;
    const int k0 = kk * 32 + 16 * h;
    uint4 out;
    if (row < count && vec_ok && k0 + 16 <= d) {
      uint4 v = *(const uint4*)(src + (size_t)row * d + k0);
      out = make_uint4(v.x ^ 0x80808080u, v.y ^ 0x80808080u, v.z ^ 0x80808080u, v.w ^ 0x80808080u);
    } else {
      uint8_t b[16];
      for (int t = 0; t < 16; ++t) {
        const int k = k0 + t;
        // padded k contributes 0 (int8 0); a padded ROW is uint8 0 = int8 -128 on real k
        b[t] = (k >= d) ? 0x00 : (row < count ? (uint8_t)(src[(size_t)row * d + k] ^ 0x80) : 0x80);
      }
      out = *(uint4*)b;
    }
    *(uint4*)(dst + (size_t)chunk * 16) = out;
  }
  int32_t* rowsum_head = (int32_t*)(dst_img + (size_t)n_tiles * ks * kFragBytes) + (size_t)n_tiles * kTile + tile * kTile;
  int32_t* tailnorm = (int32_t*)(dst_img + (size_t)n_tiles * ks * kFragBytes) + (size_t)2 * n_tiles * kTile + tile;
  __shared__ int s_tn;
  if (threadIdx.x == 0) s_tn = 0;
  __syncthreads();
  const int d_head = min(d, head_steps_of(ks) * 32);
  // Row sums: eight lanes per row, 16 bytes per load, byte sums and sums of squares by v_dot4 (one lane walking a row byte by
  // byte made this kernel 42 us per batch of 50 x 512 x 384: 12 k dependent byte loads per lane).  The vector path needs whole
  // 16-byte chunks on either side of the head / tail boundary; otherwise one lane of the group takes the byte loop.
  const bool sum_vec = vec_ok && (d_head % 16 == 0);
  for (int idx = threadIdx.x; idx < kTile * 8; idx += blockDim.x) {
    const int c = idx >> 3, t8 = idx & 7;
    const int row = tile * kTile + c;
    u32 sum = 0, head = 0, ss = 0;
    if (row < count) {
      if (sum_vec) {
        for (int j = t8; j < d / 16; j += 8) {
          const uint4 v = *(const uint4*)(src + (size_t)row * d + 16 * j);
          const u32 w[4] = {v.x, v.y, v.z, v.w};
          u32 cs = 0, cq = 0;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            cs = __builtin_amdgcn_udot4(w[q], 0x01010101u, cs, false);
            cq = __builtin_amdgcn_udot4(w[q], w[q], cq, false);
          }
          sum += cs;
          if (16 * j < d_head) head += cs; else ss += cq;
        }
      } else if (t8 == 0) {
        for (int k = 0; k < d; ++k) {
          const u32 v = src[(size_t)row * d + k];
          sum += v;
          if (k < d_head) head += v; else ss += v * v;
        }
      }
    }
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) {          // the eight lanes of a row are neighbours in one wave
      sum += (u32)__shfl_xor((int)sum, o);
      head += (u32)__shfl_xor((int)head, o);
      ss += (u32)__shfl_xor((int)ss, o);
    }
    if (t8 == 0) {
      rowsum[c] = (int32_t)sum;
      // the early-out kernels read ONE word per row: head sum and tail sum packed (packed_sums_fit)
      rowsum_head[c] = head_steps_of(ks) < ks ? (int32_t)((head << 16) | (sum - head)) : (int32_t)head;
      int tn = (int)ceil(sqrt((double)ss));
      while ((long long)tn * tn < (long long)ss) ++tn;   // an upper bound of the Euclidean norm of the tail, whatever sqrt rounded to
      atomicMax(&s_tn, tn);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) *tailnorm = s_tn;
}

// ---------------------------------------------------------------------------------------
// The pair kernel
// ---------------------------------------------------------------------------------------
// One workgroup (8 waves, 2 per SIMD) per image pair (a, b).
//   * wave w keeps RT 32-row tiles of image a as MFMA A-fragments in registers for a pass
//     (RT = 2: 8 x 64 = 512 rows per pass, so a 512-keypoint image needs ONE pass over b);
//   * image b streams through an LDS ring of NS tile slots (12 KiB per slot at D = 384),
//     one wave issuing the 1 KiB global_load_lds pieces of a whole tile, PF = NS-1 tiles
//     ahead; the only in-loop synchronisation is one raw s_barrier per tile and a
//     vmcnt(0) in the wave whose tile is due (no wave has more than one tile in flight);
//   * per-row top-2 lives in registers as packed keys, per-column top-2 is merged across
//     waves with two LDS atomics per lane and tile (order independent, see col_merge).
constexpr int kLdsBytes = 160 * 1024;
// end-of-pass row reduction: per wave 16 rows x (32 + 1 pad) entries of {best key, second key}
constexpr int kRowScratchEntries = 16 * 33;
constexpr int kRowScratchBytes = kRowScratchEntries * 8;
constexpr int kMaxSlots = 8;  // PF <= 7 keeps "one tile in flight per wave" true for 8 waves

// K-step counts with a compiled kernel; a descriptor is zero-padded up to the next one.
#define VC_KS_LIST 2, 4, 8, 12, 16, 24, 32
constexpr int kKsList[] = {VC_KS_LIST};
constexpr int kMaxKs2 = 12;   // RT = 2 (512 rows per pass) while its register budget holds (A fragments: 2*KS*4 VGPRs)
constexpr int row_tiles_of(int ks) { return ks <= kMaxKs2 ? 2 : 1; }   // long descriptors: one row tile per wave
constexpr int kMaxPad = tiles_of(VC_MAX_KEYPOINTS) * kTile;   // rows of the largest prepared image

// The dynamic LDS of a pair kernel is laid out ONCE, by a constexpr plan that both sides use: the kernel takes every
// pointer from it, the host the fixed size (the plan with an empty ring), from that the number of ring slots, and the
// launch's LDS size (`end`).  vc::LdsCursor hands out consecutive regions; all offsets are in bytes from the start of LDS.
using vc::LdsCursor;
// pair_kernel:      [ring NS x KS KiB][colbest u64 x n_pad][colsecond u32 x n_pad]
//                   [cterm i32 x n_pad][m21 i32 x n_pad][rbest, rsecond, ridx i32 x n_pad]
//                   [crow6 i32 x 8 waves x 64 rows][row-reduce scratch 8 waves x 4224 B][wave_count 8 ints]
// guided matching adds: column keypoint y (x lives in m21, which the tile loop leaves alone) and the row terms of
// every wave's RT * 32 rows
struct PairLds {
  u32 colbest, colsecond;        // [n_pad] column search: (s << 32 | ~row) and the runner-up's s
  u32 cterm;                     // [n_pad] column terms 128*rb + 32640*D
  u32 m21;                       // [n_pad] accepted row of every column (cross check); GUIDED: column keypoint x until then
  u32 rbest, rsecond, ridx;      // [n_pad] row results
  u32 crow6;                     // [wave][64] row terms 128*ra - 49024*D
  u32 rscratch;                  // [wave][kRowScratchEntries] uint2: reduce_rows
  u32 wave_count;                // [kWaves] append_ordered
  u32 gcy;                       // GUIDED: [n_pad] column keypoint y
  u32 growg;                     // GUIDED: [wave][RT*32] v4i row terms of the geometric test
  u32 end;
};
__host__ __device__ constexpr PairLds pair_lds(u32 ring_bytes, int n_pad, int rt, bool guided) {
  LdsCursor c{ring_bytes};
  PairLds l{};
  l.colbest = c.take(n_pad * 8, 8);
  l.colsecond = c.take(n_pad * 4);
  l.cterm = c.take(n_pad * 4);
  l.m21 = c.take(n_pad * 4);
  l.rbest = c.take(n_pad * 4);
  l.rsecond = c.take(n_pad * 4);
  l.ridx = c.take(n_pad * 4);
  l.crow6 = c.take(kWaves * 64 * 4, 16);
  l.rscratch = c.take(kWaves * kRowScratchBytes, 8);
  l.wave_count = c.take(kWaves * 4);
  l.gcy = c.take(guided ? n_pad * 4 : 0);
  l.growg = c.take(guided ? kWaves * rt * kTile * 16 : 0, 16);
  l.end = c.take(0, 16);
  return l;
}
// Ring slots that fit beside `fixed_bytes` (0 = the kernel does not fit).  Two row tiles per wave and the persistent
// kernel need three slots, one row tile two.
constexpr int min_slots(int rt, bool persistent) { return (rt == 2 || persistent) ? 3 : 2; }
constexpr int slots_beside(u32 fixed_bytes, int ks, int least) {
  long ns = ((long)kLdsBytes - (long)fixed_bytes) / ((long)ks * kFragBytes);
  if (ns > kMaxSlots) ns = kMaxSlots;
  return ns >= least ? (int)ns : 0;
}
constexpr int plan_slots(int ks, int n_pad, int rt, bool guided) {
  return slots_beside(pair_lds(0, n_pad, rt, guided).end, ks, min_slots(rt, false));
}
constexpr bool pair_lds_ok(int ks, int rt, bool guided) {
  const PairLds l = pair_lds(plan_slots(ks, kMaxPad, rt, guided) * ks * kFragBytes, kMaxPad, rt, guided);
  return l.end <= (u32)kLdsBytes && l.colbest % 8 == 0 && l.rscratch % 8 == 0 && l.crow6 % 16 == 0 && l.growg % 16 == 0;
}
template <int... KS>   // the instantiations: row_tiles_of(KS) unguided, one row tile guided (vc_match_pairs_guided_u8)
constexpr bool pair_lds_ok() { return ((pair_lds_ok(KS, row_tiles_of(KS), false) && pair_lds_ok(KS, 1, true)) && ...); }
static_assert(pair_lds_ok<VC_KS_LIST>(), "pair_kernel's LDS plan: size and alignment at the largest block, every length");

__device__ inline void wg_barrier() {
  // LDS writes/atomics of this wave are complete before it arrives; LDS-DMA stays in flight
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// One 1 KiB LDS-DMA piece: 64 lanes x 16 B, global source per lane, LDS destination =
// wave-uniform byte address `lds_dst` + lane*16.  Issued from inline asm on purpose: hipcc
// treats the builtin form as an LDS write that may alias every later ds_read and inserts
// s_waitcnt vmcnt(0) before the next LDS read of the issuing wave, which drains the prefetch
// it has just started.  Hidden in asm, the copy is invisible to the compiler's counters; the
// kernel waits for it by hand (vmcnt(0) in the issuing wave, then the workgroup barrier).
__device__ __forceinline__ void glds16(const void* gsrc, u32 lds_dst_any) {
  // The destination is wave-uniform by construction, but under SGPR pressure the compiler may have computed it
  // with vector instructions; an explicit v_readfirstlane (which it cannot fold away) puts it where M0 can take it.
  // (The value is laundered through an empty asm so that the builtin is not folded away as "already uniform"; the
  // v_readfirstlane itself is the compiler's, which knows the wait state it needs after the VALU write of its
  // source — one written in asm right behind a v_mov read a stale register.)
  asm volatile("" : "+v"(lds_dst_any));
  vc::lds_dma16(gsrc, (u32)__builtin_amdgcn_readfirstlane((int)lds_dst_any));
}

// One 256-byte LDS-DMA piece (64 lanes x 4 B; inactive lanes copy nothing): LDS destination = `lds_dst` + lane*4.
__device__ __forceinline__ void glds4(const void* gsrc, u32 lds_dst_any) {
  asm volatile("" : "+v"(lds_dst_any));
  vc::lds_dma4(gsrc, (u32)__builtin_amdgcn_readfirstlane((int)lds_dst_any));
}

// Producer side of the ring.  The KS pieces of a tile are dealt to NP producer waves, M pieces
// each (KS = 12: waves 0..5 issue 2 pieces per tile), so no wave is held up for a whole tile's
// worth of LDS-DMA issue.  Every producer wave has the same number of pieces in flight per tile,
// which makes "my pieces of tile t have landed" a counted wait: vmcnt(M * tiles issued after t).
// PW: the waves that may produce (pair2_kernel: the four EARLY waves only — they wait at the barrier for the late half
// anyway, so neither the issue of the pieces nor the wait for them to land sits on the late waves' critical path).
template <int KS, int PW = kWaves>
struct Producer {
  static constexpr int M = (KS + PW - 1) / PW;
  static constexpr int NP = KS / M;
  static_assert(NP * M == KS && NP <= PW, "pieces must divide evenly over the producer waves");
};

template <int KS, int PW = kWaves>
__device__ __forceinline__ void stage_tile(const uint8_t* __restrict__ tile_src, u32 slot_lds, int wave, int lane) {
  constexpr int M = Producer<KS, PW>::M;
  if (wave < Producer<KS, PW>::NP) {
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const int kk = wave * M + m;
      glds16(tile_src + kk * kFragBytes + lane * 16, slot_lds + kk * kFragBytes);
    }
  }
}

// Wait until this wave's pieces of the oldest tile in flight have landed; `younger` tiles
// (0..7) were issued after it.  s_waitcnt takes an immediate, hence the switch.
template <int KS, int PW = kWaves>
__device__ __forceinline__ void wait_tile(int wave, int younger) {
  constexpr int M = Producer<KS, PW>::M;
  if (wave < Producer<KS, PW>::NP) {
#define VC_W(n) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((n) * M) : "memory")
    // binary decision tree: three scalar branches per call instead of a chain of eight
    if (younger < 4) {
      if (younger < 2) { if (younger == 0) VC_W(0); else VC_W(1); }
      else             { if (younger == 2) VC_W(2); else VC_W(3); }
    } else {
      if (younger < 6) { if (younger == 4) VC_W(4); else VC_W(5); }
      else             { if (younger == 6) VC_W(6); else VC_W(7); }
    }
#undef VC_W
  }
}

// MFMA phase: similarity tiles of the wave's RT row tiles against one column tile.
// acc = sum (a-128)(b-128) over k (C operand 0); the bias terms are added in the epilogue.
// `mid()` runs after the first fragment group's MFMAs have been issued: the matrix pipe is busy for
// the next ~128 cycles, which hides the issue cost of the LDS-DMA pieces placed there (in-kernel
// stamps showed the producer waves' staging on the critical path when it sat right after the barrier).
template <int KS, int RT, typename Mid>
__device__ __forceinline__ void mfma_phase(const v4i (&afrag)[RT][KS], v16i (&acc)[RT], const uint8_t* slot,
                                           int lane, Mid mid) {
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[rt][r] = 0;
  // K loop in groups of G fragments, the next group's LDS reads issued ahead of this group's
  // MFMAs; sched_barrier keeps the compiler from hoisting every read to the top (which costs
  // 4*KS registers and spills).
  constexpr int G = (RT * KS >= 24) ? 2 : (KS < 4 ? KS : 4);  // smaller groups where registers are tight
  constexpr int NG = KS / G;
  static_assert(KS % G == 0, "KS must be a multiple of the fragment group");
  const uint8_t* src = slot + lane * 16;
  // the wave that feeds the matrix pipe wins issue arbitration against its SIMD partner's epilogue
  __builtin_amdgcn_s_setprio(1);
  v4i bf[2][G];
#pragma unroll
  for (int i = 0; i < G; ++i) bf[0][i] = *(const v4i*)(src + i * kFragBytes);
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    if (g + 1 < NG) {
#pragma unroll
      for (int i = 0; i < G; ++i) bf[(g + 1) & 1][i] = *(const v4i*)(src + ((g + 1) * G + i) * kFragBytes);
    }
#pragma unroll
    for (int i = 0; i < G; ++i)
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        acc[rt] = __builtin_amdgcn_mfma_i32_32x32x32_i8(afrag[rt][g * G + i], bf[g & 1][i], acc[rt], 0, 0, 0);
      }
    __builtin_amdgcn_sched_barrier(0);
    if (g == 0) mid();
  }
  __builtin_amdgcn_s_setprio(0);
}

// Epilogue phase: top-2 updates for one column tile.
//
// Exact int32 arithmetic on biased bytes: with a' = a-128, b' = b-128,
//   s = sum a'b' + 128*ra + 128*rb - 16384*D = acc + rterm[i] + ct[j]          (one v_add3_u32)
//   ct[j] = 128*rb[j] + 32640*D (per lane),  rterm[i] = 128*ra[i] - 49024*D (per register, LDS).
//
// Irrelevant similarities.  The launch passes s_low such that a similarity s <= s_low can never
// influence the match list (see relevance_thresholds() for the proof sketch): it is too small to
// be an accepted best, and as a runner-up it can never fail the ratio test of an acceptable best.
// The searches may therefore ignore any such element.  Per 32x32 tile: one max over the lane's
// 16 similarities, and only if some lane of the wave holds a relevant one, the actual updates:
//   row search    key = s << 6 | (63 - column tile)          v_lshl_or, v_med3, v_max
//   column search key = s << 6 | (63 - local row code)       v_lshl_or, v_med3, v_max
// (s < 2^26: 255^2 * 1024 < 2^26.)  s_low = -1 disables the shortcut (every s >= 0 is relevant),
// which is what the one-way API uses because it reports best / second for every row.
//
// The lane's column result goes to LDS with two atomics (col_merge), valid in any order:
//   best64  = max over keys (s << 32 | ~row): highest s, lowest row on ties
//   second  = max over { every lane's second } U { every best that is not THE best }: a best that
//             loses its max contributes itself, one that wins contributes the value it displaced.
//
// Guided matching (GUIDED, pair_kernel<..., GUIDED = true>): the update pass first replaces every similarity whose candidate
// (row keypoint, column keypoint) fails the pair's geometric test by 0 — the value that never matches and never
// is a runner-up — so both searches see the masked matrix.  The relevance test of pass 1 stays on the unmasked
// similarities: masking only lowers a value, so a tile that is irrelevant unmasked is irrelevant masked.
// The test is inlier_f / inlier_h of two_view.hip without their guards on a zero denominator and an overflowing bound
// (specification: oracle/two_view_oracle.py inliers_f32), float32 in the same operation order, factorised into terms of the row (LDS, GuidedWave::rowg, written once per pass), terms
// of the lane's column (once per tile) and what is left per candidate:
//   F  row (fx0, fx1, fx2, r = fx0 fx0 + fx1 fx1)   column (x2, y2, q0 = ft0 ft0, q1 = ft1 ft1)
//      c = x2 fx0 + y2 fx1 + fx2,  den = (r + q0) + q1,  admissible iff c c <= t2 den
//   H  row (p0, p1, pw, e = pw != 0 ? t2 (pw pw) : NaN)   column (x2, y2)
//      dx = p0 - x2 pw,  dy = p1 - y2 pw,  admissible iff dx dx + dy dy <= e
// A NaN model makes every comparison false: nothing is admissible.
struct GuidedWave {          // wave-uniform state of the geometric test
  bool is_f;                 // VC_MODEL_FUNDAMENTAL, else VC_MODEL_HOMOGRAPHY
  float t2;
  float m[9];                // the pair's model, row-major
  const v4i* rowg;           // [RT*32] row terms of this wave's rows (float bits)
  const int* cx;             // [n_pad] column keypoints of image b (float bits)
  const int* cy;
};
struct NoGuide {};

__device__ __forceinline__ v4i guided_row_terms(const GuidedWave& g, float x1, float y1) {
  const float (&m)[9] = g.m;
  const float a0 = m[0] * x1 + m[1] * y1 + m[2];
  const float a1 = m[3] * x1 + m[4] * y1 + m[5];
  const float a2 = m[6] * x1 + m[7] * y1 + m[8];
  // F: a = F x1 and the row's share of the Sampson denominator; H: a = H x1 = (p0, p1, pw) and the right-hand side
  const float w = g.is_f ? a0 * a0 + a1 * a1 : (a2 != 0.f ? g.t2 * (a2 * a2) : __int_as_float(0x7fc00000));
  v4i r;
  r[0] = __float_as_int(a0); r[1] = __float_as_int(a1); r[2] = __float_as_int(a2); r[3] = __float_as_int(w);
  return r;
}

template <bool IS_F>
__device__ __forceinline__ int guided_mask(int v, const v4i row, float x2, float y2, float q0, float q1, float t2) {
  const float r0 = __int_as_float(row[0]), r1 = __int_as_float(row[1]), r2 = __int_as_float(row[2]), r3 = __int_as_float(row[3]);
  bool adm;
  if (IS_F) {
    const float cc = x2 * r0 + y2 * r1 + r2;
    const float den = (r3 + q0) + q1;
    adm = cc * cc <= t2 * den;
  } else {
    const float dx = r0 - x2 * r2;
    const float dy = r1 - y2 * r2;
    adm = dx * dx + dy * dy <= r3;
  }
  return adm ? v : 0;
}

template <int RT, bool FUSED, bool GUIDED = false, bool IS_F = false, typename Guide = NoGuide>
__device__ __forceinline__ void epilogue_phase(const v16i (&acc)[RT], u32 (&rbest)[RT][16], u32 (&rsec)[RT][16],
                                               const int* rterm_wave, const int* cterm,
                                               unsigned long long* colbest, u32* colsecond, int jt,
                                               int c, int h, u32 row_base, int s_low, bool (&dense)[RT],
                                               const Guide guide = Guide()) {
  const int ct = cterm[jt * kTile + c];
  const u32 jcode = 63u - (u32)jt;
  u32 cb = 0, cs2 = 0;
  bool any_hit = false;
  float gx2 = 0.f, gy2 = 0.f, gq0 = 0.f, gq1 = 0.f;   // GUIDED: terms of the lane's column
  if constexpr (GUIDED) {
    gx2 = __int_as_float(guide.cx[jt * kTile + c]);
    gy2 = __int_as_float(guide.cy[jt * kTile + c]);
    if (IS_F) {
      const float ft0 = guide.m[0] * gx2 + guide.m[3] * gy2 + guide.m[6];
      const float ft1 = guide.m[1] * gx2 + guide.m[4] * gy2 + guide.m[7];
      gq0 = ft0 * ft0;
      gq1 = ft1 * ft1;
    }
  }
  // Two regimes, chosen per row tile from what the previous column tile looked like (wave-uniform):
  //   sparse: pass 1 computes the lane's largest similarity only (24 VALU); if some lane is
  //           relevant, pass 2 recomputes the similarities and updates (and switches to dense);
  //   dense : one pass that updates and tracks the maximum (SIFT-like descriptors sit at
  //           cos ~0.64, right at the threshold: there almost every tile is relevant).
  // Pass 1 runs for all row tiles first, with every LDS read of the row terms issued up front:
  // measured with in-kernel stamps, the epilogue was LDS-latency-bound (890 cycles per tile for
  // ~70 instructions) when each row tile waited for its own reads.
  bool update[RT];
  bool all_dense = true;
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) { update[rt] = dense[rt]; all_dense = all_dense && dense[rt]; }
  if (!all_dense) {
    v4i cr[RT][4];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int q = 0; q < 4; ++q) cr[rt][q] = *(const v4i*)(rterm_wave + rt * kTile + 8 * q + 4 * h);
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      int m = -1;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int v0 = acc[rt][4 * q + 0] + cr[rt][q][0] + ct, v1 = acc[rt][4 * q + 1] + cr[rt][q][1] + ct;
        const int v2 = acc[rt][4 * q + 2] + cr[rt][q][2] + ct, v3 = acc[rt][4 * q + 3] + cr[rt][q][3] + ct;
        m = max(max(m, max(v0, v1)), max(v2, v3));
      }
      update[rt] = update[rt] || __any(m > s_low);
    }
  }
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    if (update[rt]) {
      any_hit = true;
      // the row terms are (re-)read through a pointer the optimiser cannot identify with pass 1's,
      // or it keeps all 16 live across the branch and spills
      const int* rterm2 = rterm_wave;
      asm volatile("" : "+v"(rterm2));
      int m = -1;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const v4i cr = *(const v4i*)(rterm2 + rt * kTile + 8 * q + 4 * h);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int r = 4 * q + i;
          int v = acc[rt][r] + cr[i] + ct;
          if constexpr (GUIDED)
            v = guided_mask<IS_F>(v, guide.rowg[rt * kTile + 8 * q + 4 * h + i], gx2, gy2, gq0, gq1, guide.t2);
          m = max(m, v);
          const u32 rk = ((u32)v << 6) | jcode;
          rsec[rt][r] = umed3(rbest[rt][r], rsec[rt][r], rk);
          rbest[rt][r] = umax(rbest[rt][r], rk);
          if (FUSED) {
            const u32 ck = ((u32)v << 6) | (u32)(63 - (rt * kTile + (r & 3) + 8 * (r >> 2)));
            cs2 = umed3(cb, cs2, ck);
            cb = umax(cb, ck);
          }
        }
        // four rows' terms at a time: hoisted, the 16 LDS reads of a row tile hold 64 registers and spill
        if constexpr (GUIDED) __builtin_amdgcn_sched_barrier(0);
      }
      dense[rt] = __any(m > s_low);
    }
  }
  if (FUSED && any_hit) {
    if (cb != 0) {
      const int j = jt * kTile + c;
      const u32 sb = cb >> 6;
      const u32 grow = row_base + (63u - (cb & 63u)) + 4u * h;
      const unsigned long long key = ((unsigned long long)sb << 32) | (unsigned long long)(0xFFFFFFFFu - grow);
      const unsigned long long old = atomicMax(&colbest[j], key);
      u32 cand = key > old ? (u32)(old >> 32) : sb;
      cand = umax(cand, cs2 >> 6);
      atomicMax(&colsecond[j], cand);
    }
  }
}

// ---------------------------------------------------------------------------------------
// Phases of the persistent kernel (pair2_kernel): accumulators that start from the row term
// ---------------------------------------------------------------------------------------
// MFMA phase with C = row term: acc[rt][4q + i] starts at rterm[32 rt + 8 q + 4 h + i] (the row that register
// holds in the 32x32 MFMA C layout), read from the wave's LDS slice straight into the accumulator registers,
// so the result is sum (a-128)(b-128) + 128 ra - 49024 D and the column term is all that is left to add.
// B operands come through a rolling window of NB fragment registers, D = NB - 1 k-steps ahead of the MFMAs that use them
// (stamps: with one two-fragment group of look-ahead a wave alone on the pipe ran its 24 MFMAs in ~1300 cycles instead
// of 768 — every group waited for an LDS read issued 128 pipe cycles earlier).
// Not kept (measured): letting the window run on into the NEXT tile of the ring (12 more registers live
// across the epilogue: spills, and any spill reload near the tile loop makes the compiler wait for vmcnt, which drains the
// LDS-DMA ring), and eight symmetric waves that issue the next tile's first reads in front of the barrier (12.3 M
// pairs/s against 14.1 M with the staggered halves).
template <int KS>
struct BWindow {
  static constexpr int NB = KS == 12 ? kWindow12 : (KS >= 4 ? 4 : KS);
  static constexpr int D = NB - 1;
  static_assert(KS % NB == 0 && head_steps_of(KS) % NB == 0, "window positions must line up at the head boundary");
};

// steps K0..K1-1 of a tile whose window is refilled up to fragment NF-1; `mid()` runs behind the MFMAs of step 0 (the
// matrix pipe is busy for the next 64 cycles, which hides part of the issue cost of the LDS-DMA pieces placed there)
template <int KS, int K0, int K1, int NF, typename Mid>
__device__ __forceinline__ void mfma_steps(const v4i (&afrag)[2][KS], v16i (&acc)[2], v4i (&bf)[BWindow<KS>::NB],
                                           const uint8_t* src, Mid mid) {
  constexpr int NB = BWindow<KS>::NB, D = BWindow<KS>::D;
#pragma unroll
  for (int k = K0; k < K1; ++k) {
    const int f = k + D;
    if (NB > 1 && f < NF) bf[f % NB] = *(const v4i*)(src + f * kFragBytes);
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
      acc[rt] = __builtin_amdgcn_mfma_i32_32x32x32_i8(afrag[rt][k], bf[k % NB], acc[rt], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
    if (NB == 1 && k + 1 < NF) bf[0] = *(const v4i*)(src + (k + 1) * kFragBytes);
    if (k == 0) mid();
  }
}

// MFMA phase of one column tile.  EARLY (descriptors of 129..384 bytes): the accumulators start from the HEAD row term
// and the first KH k-steps give, per element, s_head - (head column term).  The rest of the dot product is bounded by
// Cauchy-Schwarz on the bytes themselves: sum over the tail of a b <= |a_tail| |b_tail| <= TNa TNb (per-tile maxima of
// the rounded-up tail norms, from prepare_kernel), and the tail's share of the bias terms is known exactly — it is what
// the head row / column terms leave out.  If no lane holds  acc > s_low - cth - TNa TNb  the whole 32x32 tile stays at
// or below the relevance threshold whatever the tail holds: its remaining KS - KH MFMAs per row tile and its epilogue
// are skipped (nothing it could contribute would change the match list, see relevance_threshold()).  Otherwise the
// tile simply goes on: the tail MFMAs run on the same accumulators and the difference between the full and the head row
// term (`rdelta`, one LDS word per register) is added afterwards — a failed test costs the test and 32 additions, no
// MFMA is repeated.  Returns 3 if the wave's two row tiles were cut short (the epilogue skips them), else 0.
template <int KS, bool EARLY, typename Mid>
__device__ __forceinline__ int mfma_phase2(const v4i (&afrag)[2][KS], v16i (&acc)[2], const uint8_t* slot,
                                           const int* rterm_wave, const int* rterm_head_wave, const int* rdelta_wave,
                                           int lane, int h, int thr_early, Mid mid) {
  constexpr int RT = 2;
  constexpr int KH = head_steps_of(KS);
  constexpr int NB = BWindow<KS>::NB, D = BWindow<KS>::D;
  const uint8_t* src = slot + lane * 16;
  // (no s_setprio here: raising the MFMA phase's priority paid on earlier kernels; on this one it costs the dense path 4 %)
  v4i bf[NB];
#pragma unroll
  for (int i = 0; i < (NB > 1 ? D : 1); ++i) bf[i] = *(const v4i*)(src + i * kFragBytes);
  const int* rterm = EARLY ? rterm_head_wave : rterm_wave;
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const v4i cr = *(const v4i*)(rterm + rt * kTile + 8 * q + 4 * h);
      acc[rt][4 * q + 0] = cr[0]; acc[rt][4 * q + 1] = cr[1]; acc[rt][4 * q + 2] = cr[2]; acc[rt][4 * q + 3] = cr[3];
    }
  int cut = 0;
  mfma_steps<KS, 0, KH, KS>(afrag, acc, bf, src, mid);
  auto nothing = []() {};
  if (EARLY) {
    // one test for both row tiles of the wave (threshold from the larger of their two tail bounds)
    int m = max(acc[0][0], acc[1][0]);
#pragma unroll
    for (int r = 1; r < 16; ++r) m = max(m, max(acc[0][r], acc[1][r]));
    if (__any(m > thr_early)) {   // may matter after all: the tail, then the part of the row term the head left out
      mfma_steps<KS, KH, KS, KS>(afrag, acc, bf, src, nothing);
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const v4i dr = *(const v4i*)(rdelta_wave + rt * kTile + 8 * q + 4 * h);
          acc[rt][4 * q + 0] += dr[0]; acc[rt][4 * q + 1] += dr[1]; acc[rt][4 * q + 2] += dr[2]; acc[rt][4 * q + 3] += dr[3];
        }
    } else {
      cut = 3;
    }
  } else if (KH < KS) {
    mfma_steps<KS, KH, KS, KS>(afrag, acc, bf, src, nothing);
  }
  return cut;
}

// per-column search state of pair2_kernel: one LDS address serves both atomics of the column merge
struct ColState {
  unsigned long long best;   // (s << 32) | ~row: highest s, lowest row on ties
  u32 second;
  u32 pad;
};

// Epilogue with the row term already inside the accumulators: s = acc + ct (ct: the lane's column term).
//   relevance: some lane holds acc > s_low - ct                       (8 v_max3 + 1 compare per 32x32 tile)
//   update   : key = (acc << 6) + ((ct << 6) | code)                  (one v_lshl_add per key)
// The relevance test is cheap enough to run on every tile, so there is no separate "dense" regime here.
// `ct` is read from LDS by the caller BEFORE the MFMA phase that precedes this call: read here it queued behind
// the other waves' fragment reads (stamps: ~450 of an epilogue's 660 cycles).  Column merge as in epilogue_phase.
__device__ __forceinline__ bool epilogue_phase2(const v16i (&acc)[2], u32 (&rbest)[2][16], u32 (&rsec)[2][16],
                                                int ct, ColState* col,
                                                int jt, int c, int h, u32 row_base, int s_low, int cut) {
  constexpr int RT = 2;
  const int thr = s_low == 0x7fffffff ? s_low : s_low - ct;   // acc > thr  <=>  acc + ct > s_low (|ct| < 2^27: no overflow)
  const u32 ctj = ((u32)ct << 6) + (63u - (u32)jt);           // key = (acc << 6) + ctj   (acc + ct >= 0)
  u32 cb = 0, cs2 = 0;
  bool hit = false;
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    if ((cut >> rt) & 1) continue;   // cut short by the early-out: proven irrelevant, accumulators incomplete
    int m = acc[rt][0];
#pragma unroll
    for (int r = 1; r < 16; r += 2) m = max(m, r + 1 < 16 ? max(acc[rt][r], acc[rt][r + 1]) : acc[rt][r]);
    if (__any(m > thr)) {
      hit = true;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const u32 rk = ((u32)acc[rt][r] << 6) + ctj;
        rsec[rt][r] = umed3(rbest[rt][r], rsec[rt][r], rk);
        rbest[rt][r] = umax(rbest[rt][r], rk);
        const u32 ck = (rk & ~63u) | (u32)(63 - (rt * kTile + (r & 3) + 8 * (r >> 2)));
        cs2 = umed3(cb, cs2, ck);
        cb = umax(cb, ck);
      }
      // Keep the updates INSIDE the branch: without these ties the optimiser sinks the 32 med3 / max below the
      // join with a zero key on the other path, i.e. runs them for every tile (seen in the ISA).
#pragma unroll
      for (int r = 0; r < 16; r += 4)
        asm volatile("" : "+v"(rbest[rt][r]), "+v"(rbest[rt][r + 1]), "+v"(rbest[rt][r + 2]), "+v"(rbest[rt][r + 3]),
                          "+v"(rsec[rt][r]), "+v"(rsec[rt][r + 1]), "+v"(rsec[rt][r + 2]), "+v"(rsec[rt][r + 3]));
    }
  }
  if (cb != 0) {
    const int j = jt * kTile + c;
    const u32 sb = cb >> 6;
    const u32 grow = row_base + (63u - (cb & 63u)) + 4u * h;
    const unsigned long long key = ((unsigned long long)sb << 32) | (unsigned long long)(0xFFFFFFFFu - grow);
    const unsigned long long old = atomicMax(&col[j].best, key);
    u32 cand = key > old ? (u32)(old >> 32) : sb;
    cand = umax(cand, cs2 >> 6);
    atomicMax(&col[j].second, cand);
  }
  return hit;
}

// ---------------------------------------------------------------------------------------
// What follows the tile loop: the row results of a pass (both pair kernels), then the match list (pair_kernel; pair2_kernel
// keeps these steps written out, see there)
// ---------------------------------------------------------------------------------------
// Row results of a pass: store(row, best, second, idx) for every row < n1 of the wave's RT row tiles.
// Each row's candidates sit in 32 lanes (one per column residue c).  Transpose through a
// wave-private LDS slice, 16 rows per round: lane (c, h) writes its {best, second} keys of
// 8 registers, then lane L re-reads row L>>2, columns 8*(L&3) .. +7 in ascending order
// (strict '>' keeps the lowest column on ties) and the four partial results of a row are
// folded with two quad-permute steps.  No workgroup barrier: the slice belongs to the wave
// and its LDS operations execute in order.
// SKIP_UNSEEN: a round whose 16 rows never saw a relevant similarity stores nothing (the caller has preset the
// (0, 0, -1) defaults); the one-way API reports every row.
template <int RT, bool SKIP_UNSEEN, typename Store>
__device__ __forceinline__ void reduce_rows(const u32 (&rbest)[RT][16], const u32 (&rsec)[RT][16], uint2* rscratch,
                                            int lane, int c, int h, int tile0, int n1, Store store) {
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      u32 seen = 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) seen |= rbest[rt][8 * half + j];
      if (SKIP_UNSEEN && !__any(seen != 0)) continue;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int r = 8 * half + j;
        rscratch[(j + 8 * h) * 33 + c] = make_uint2(rbest[rt][r], rsec[rt][r]);
      }
      const int rl = lane >> 2, qd = lane & 3;       // row of the round, column quarter
      u32 rb = 0, rs = 0, rc = 0;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const uint2 en = rscratch[rl * 33 + qd * 8 + e];
        const bool gt = en.x > rb;
        rs = gt ? umax(rb, en.y) : umax(rs, en.x);
        rc = gt ? (u32)(qd * 8 + e) : rc;
        rb = umax(rb, en.x);
      }
      // fold quarters: the lower quarter absorbs the higher one (strict '>': lower column wins)
#pragma unroll
      for (int step = 0; step < 2; ++step) {
        u32 pb, ps, pc;
        if (step == 0) { pb = dpp_mov<0xB1>(rb); ps = dpp_mov<0xB1>(rs); pc = dpp_mov<0xB1>(rc); }   // quad_perm [1,0,3,2]
        else           { pb = dpp_mov<0x4E>(rb); ps = dpp_mov<0x4E>(rs); pc = dpp_mov<0x4E>(rc); }   // quad_perm [2,3,0,1]
        const bool gt = pb > rb;
        rs = gt ? umax(rb, ps) : umax(rs, pb);
        rc = gt ? pc : rc;
        rb = umax(rb, pb);
      }
      // row of this lane's result inside the wave's RT*32 rows (see the MFMA C layout)
      const int jj = rl & 7, hh = rl >> 3;
      const int lrow = (jj & 3) + 16 * half + 8 * (jj >> 2) + 4 * hh;
      if (qd == 0) {
        const int row = (tile0 + rt) * kTile + lrow;
        if (row < n1) {
          const int sb = (int)(rb >> 6);
          store(row, sb, sb > 0 ? (int)(rs >> 6) : 0, sb > 0 ? (63 - (int)(rb & 63)) * kTile + (int)rc : -1);
        }
      }
    }
  }
}

// Ordered compaction, one chunk of kThreads candidates: every thread with `ok` stores (i, j) behind those of the lower
// threads, starting at out[2 * base]; returns the base of the next chunk.  Called by all kWaves waves of the workgroup
// (two barriers); wave_count: kWaves ints of LDS.  `lane` and `wave` are the caller's own values: recomputed here from
// threadIdx they change the register allocation of pair2_kernel<12> around its pair loop (measured slower on sparse input).
__device__ __forceinline__ int append_ordered(bool ok, int i, int j, int base, int* wave_count, uint32_t* out, int lane,
                                              int wave) {
  const unsigned long long mask = __ballot(ok);
  if (lane == 0) wave_count[wave] = __popcll(mask);
  __syncthreads();
  int before = base, chunk_total = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    const int wc = wave_count[w];
    before += w < wave ? wc : 0;
    chunk_total += wc;
  }
  if (ok) {
    const int pos = before + __popcll(mask & ((1ull << lane) - 1ull));
    out[2 * pos] = (uint32_t)i;
    out[2 * pos + 1] = (uint32_t)j;
  }
  __syncthreads();
  return base + chunk_total;
}

// Angle + ratio tests, cross check, ordered compaction of one pair: returns the number of matches written to `out`.
//   accept(best, second): AcceptTable or AcceptAcos;  column(j): column j's search result as a ColState, whichever way
//   the kernel keeps it
// The column pass leaves in m21[j] the row that column j accepts (or -1); row i matches its best column j if it accepts
// it and, with the cross check, m21[j] == i.  Called by the whole workgroup behind a barrier that publishes the searches'
// results; `tid` is the caller's (laundered) thread index, `lane` and `wave` its own too (see append_ordered).
template <typename Accept, typename Column>
__device__ __forceinline__ int finalise_pair(Accept accept, Column column, int* m21, const int* rbest_s, const int* rsecond_s,
                                             const int* ridx_s, int n1, int n2, int cross_check, int tid, int lane, int wave,
                                             int* wave_count, uint32_t* out) {
  if (cross_check) {
    for (int j = tid; j < n2; j += kThreads) {
      const ColState cs = column(j);
      const int row = (int)(0xFFFFFFFFu - (u32)cs.best);
      m21[j] = accept((int)(cs.best >> 32), (int)cs.second) ? row : -1;
    }
    __syncthreads();
  }
  int base = 0;
  for (int i0 = 0; i0 < n1; i0 += kThreads) {
    const int i = i0 + tid;
    bool ok = false;
    int j = -1;
    if (i < n1) {
      j = ridx_s[i];
      ok = accept(rbest_s[i], rsecond_s[i]);
      if (ok && cross_check) ok = (m21[j] == i);
    }
    base = append_ordered(ok, i, j, base, wave_count, out, lane, wave);
  }
  return base;
}

// Launch arguments of guided matching (pair_kernel<..., GUIDED = true>); the unguided kernels carry none.
template <bool GUIDED>
struct GuidedArgs {};
template <>
struct GuidedArgs<true> {
  const float* keypoints;   // [n_images][n_max][2]; rows >= counts are never read
  const float* models;      // [n_pairs][9] row-major
  const int32_t* kind;      // [n_pairs]: VC_MODEL_FUNDAMENTAL, VC_MODEL_HOMOGRAPHY, anything else: the pair is skipped
  float t2;                 // max_error squared (float32 product)
};

// GUIDED (FUSED only): guided matching, the similarities pass the pair's geometric test first (epilogue_phase).
template <int KS, int RT, bool FUSED, bool GUIDED = false>
__global__ __launch_bounds__(kThreads, 2) void pair_kernel(
    const uint8_t* __restrict__ prepared, const int32_t* __restrict__ counts, int n_tiles_img, int d,
    const int32_t* __restrict__ pairs, float max_ratio, float max_distance, int cross_check,
    int n_max, int ns, int s_low, uint32_t* __restrict__ out_matches, int32_t* __restrict__ out_counts,
    // !FUSED: one-way outputs (rows of A against B)
    int32_t* __restrict__ o_idx, int32_t* __restrict__ o_best, int32_t* __restrict__ o_second,
    const GuidedArgs<GUIDED> ga) {
  static_assert(FUSED || !GUIDED, "guided matching exists for the fused match list only");
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int n_pad = n_tiles_img * kTile;
  uint8_t* ring = smem;
  const PairLds lds = pair_lds((u32)ns * (KS * kFragBytes), n_pad, RT, GUIDED);
  unsigned long long* colbest = (unsigned long long*)(smem + lds.colbest);
  u32* colsecond = (u32*)(smem + lds.colsecond);
  int* cterm = (int*)(smem + lds.cterm);
  int* m21 = (int*)(smem + lds.m21);
  int* rbest_s = (int*)(smem + lds.rbest);
  int* rsecond_s = (int*)(smem + lds.rsecond);
  int* ridx_s = (int*)(smem + lds.ridx);
  int* crow6 = (int*)(smem + lds.crow6);
  int* wave_count = (int*)(smem + lds.wave_count);
  int* gcy = (int*)(smem + lds.gcy);
  v4i* growg = (v4i*)(smem + lds.growg);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 31, h = lane >> 5;
  uint2* rscratch = (uint2*)(smem + lds.rscratch) + wave * kRowScratchEntries;  // this wave's slice

  const int p = blockIdx.x;
  const int img_a = pairs[2 * p], img_b = pairs[2 * p + 1];
  const int n1 = min(max(counts[img_a], 0), n_max);
  const int n2 = min(max(counts[img_b], 0), n_max);
  const size_t img_stride = image_bytes(n_tiles_img, KS);
  const uint8_t* a_frags = prepared + (size_t)img_a * img_stride;
  const uint8_t* b_frags = prepared + (size_t)img_b * img_stride;
  const int32_t* a_rowsum = (const int32_t*)(a_frags + (size_t)n_tiles_img * KS * kFragBytes);
  const int32_t* b_rowsum = (const int32_t*)(b_frags + (size_t)n_tiles_img * KS * kFragBytes);

  // Pass 0's A fragments and row sums depend only on the pair indices: issue them now so that
  // their latency overlaps the (dependent) count lookups, the LDS initialisation and the first
  // LDS-DMA pieces instead of following them.
  v4i afrag[RT][KS];
  {
    const int tile0 = wave * RT;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int kk = 0; kk < KS; ++kk)
        afrag[rt][kk] = *(const v4i*)(a_frags + ((size_t)(tile0 + rt) * KS + kk) * kFragBytes + lane * 16);
  }
  int rowsum0 = 0;
  if (lane < RT * kTile) rowsum0 = a_rowsum[wave * RT * kTile + lane];

  constexpr int kRowsPerPass = kWaves * RT * kTile;
  const int n_ct = ceil_div(n2, kTile);  // column tiles of b that hold valid rows
  const int n_pass = ceil_div(n1, kRowsPerPass);
  int kind = VC_MODEL_FUNDAMENTAL;
  if constexpr (GUIDED) kind = ga.kind[p];
  const bool skipped = kind != VC_MODEL_FUNDAMENTAL && kind != VC_MODEL_HOMOGRAPHY;   // GUIDED: a skipped pair has count 0
  const int total = skipped ? 0 : n_pass * n_ct;   // tiles consumed, in order (pass, jt)
  const int pf = ns - 1;

  GuidedWave gw;
  if constexpr (GUIDED) {
    gw.is_f = kind == VC_MODEL_FUNDAMENTAL;
    gw.t2 = ga.t2;
#pragma unroll
    for (int i = 0; i < 9; ++i) gw.m[i] = ga.models[(size_t)p * 9 + i];
    gw.rowg = growg + wave * RT * kTile;
    gw.cx = m21;
    gw.cy = gcy;
  }

  if (total == 0) {  // an empty image: nothing can match (uniform exit)
    if (FUSED) { if (tid == 0) out_counts[p] = 0; }
    else for (int i = tid; i < n1; i += kThreads) { o_idx[i] = -1; o_best[i] = 0; o_second[i] = 0; }
    return;
  }

  // ---- per-pair LDS state ----------------------------------------------------------------
  for (int j = tid; j < n_ct * kTile; j += kThreads) {
    cterm[j] = 128 * b_rowsum[j] + 32640 * d;
    colbest[j] = 0ull;
    colsecond[j] = 0u;
    if constexpr (GUIDED) {   // padded columns hold similarity 0: their keypoint is never decisive
      const float2 kp = j < n2 ? *(const float2*)(ga.keypoints + ((size_t)img_b * n_max + j) * 2) : make_float2(0.f, 0.f);
      m21[j] = __float_as_int(kp.x);
      gcy[j] = __float_as_int(kp.y);
    }
  }
  if (FUSED)  // defaults for rows whose reduction round is skipped (ordered by the tile barriers)
    for (int i = tid; i < n1; i += kThreads) { rbest_s[i] = 0; rsecond_s[i] = 0; ridx_s[i] = -1; }
  const int rbias = -49024 * d;
  int* crow6_wave = crow6 + wave * 64;
  const u32 ring_lds = vc::lds_addr(ring);

  // producer / consumer cursors over the tile sequence
  int prod_seq = 0, prod_jt = 0, prod_slot = 0;
  for (; prod_seq < pf && prod_seq < total; ++prod_seq) {
    stage_tile<KS>(b_frags + (size_t)prod_jt * KS * kFragBytes, ring_lds + (u32)prod_slot * (KS * kFragBytes), wave, lane);
    if (++prod_jt == n_ct) prod_jt = 0;
    if (++prod_slot == ns) prod_slot = 0;
  }
  int cons_seq = 0, cons_slot = 0;
  // The two waves of a SIMD (w and w+4) run half a tile apart: while waves 0-3 issue the MFMAs of
  // tile t, waves 4-7 run the VALU epilogue of tile t-1, and vice versa, so the matrix pipe and the
  // vector pipe of a SIMD work at the same time instead of being fought over in lockstep.
  const bool late = wave >= kWaves / 2;

  for (int pass = 0; pass < n_pass; ++pass) {
    const int tile0 = (pass * kWaves + wave) * RT;  // first 32-row tile of a owned by this wave
    // A fragments stay in registers for the whole pass (every tile index exists: tiles_of());
    // pass 0's were requested at kernel entry.
    u32 rbest[RT][16], rsec[RT][16];
    int rowsum = rowsum0;
    if (pass > 0) {
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int kk = 0; kk < KS; ++kk)
          afrag[rt][kk] = *(const v4i*)(a_frags + ((size_t)(tile0 + rt) * KS + kk) * kFragBytes + lane * 16);
      if (lane < RT * kTile) rowsum = a_rowsum[tile0 * kTile + lane];
    }
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int r = 0; r < 16; ++r) { rbest[rt][r] = 0; rsec[rt][r] = 0; }
    // row term of this lane's row (lane <-> row tile0*32 + lane of the wave's RT*32 rows)
    if (lane < RT * kTile) crow6_wave[lane] = 128 * rowsum + rbias;
    if constexpr (GUIDED) {   // consumed (stored to LDS) before the tile loop: no load of this wave's own is in flight inside it
      if (lane < RT * kTile) {
        const int row = tile0 * kTile + lane;
        const float2 kp = row < n1 ? *(const float2*)(ga.keypoints + ((size_t)img_a * n_max + row) * 2) : make_float2(0.f, 0.f);
        growg[wave * RT * kTile + lane] = guided_row_terms(gw, kp.x, kp.y);
      }
    }
    const u32 row_base = (u32)(tile0 * kTile);
    bool dense[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) dense[rt] = false;
    v16i acc[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[rt][r] = 0;

    // one iteration = one column tile: wait for it, barrier, then the two phases in the order of
    // this wave's half
#define VC_TILE_HEAD()                                                                              \
    wait_tile<KS>(wave, prod_seq - cons_seq - 1);                                                   \
    wg_barrier();                                                                                   \
    const uint8_t* slot = ring + (size_t)cons_slot * KS * kFragBytes;                               \
    if (++cons_slot == ns) cons_slot = 0;                                                           \
    ++cons_seq;
    // refill of the slot freed by the previous iteration; legal anywhere after the barrier
    auto produce = [&]() {
      if (prod_seq < total) {
        stage_tile<KS>(b_frags + (size_t)prod_jt * KS * kFragBytes,
                       ring_lds + (u32)prod_slot * (KS * kFragBytes), wave, lane);
        ++prod_seq;
        if (++prod_jt == n_ct) prod_jt = 0;
        if (++prod_slot == ns) prod_slot = 0;
      }
    };

    // the model kind is uniform over the workgroup: one scalar branch per tile
#define VC_EPILOGUE(ejt, eth)                                                                                                  \
    if constexpr (GUIDED) {                                                                                                    \
      if (gw.is_f)                                                                                                             \
        epilogue_phase<RT, FUSED, true, true>(acc, rbest, rsec, crow6_wave, cterm, colbest, colsecond, ejt, c, h, row_base,   \
                                              eth, dense, gw);                                                                 \
      else                                                                                                                     \
        epilogue_phase<RT, FUSED, true, false>(acc, rbest, rsec, crow6_wave, cterm, colbest, colsecond, ejt, c, h, row_base,  \
                                               eth, dense, gw);                                                                \
    } else {                                                                                                                   \
      epilogue_phase<RT, FUSED>(acc, rbest, rsec, crow6_wave, cterm, colbest, colsecond, ejt, c, h, row_base, eth, dense);     \
    }
    {
    // Staggered halves (late = waves 4-7): one loop, the epilogue shared, only the MFMA phase
    // placed before or after it.  The late half runs the epilogue of tile jt-1; for jt = 0 that
    // call is neutralised by an unreachable threshold (its accumulators are not defined yet).
    for (int jt = 0; jt < n_ct; ++jt) {
      VC_TILE_HEAD()
      if (!late) mfma_phase<KS, RT>(afrag, acc, slot, lane, produce);
      const int ejt = late ? (jt > 0 ? jt - 1 : 0) : jt;
      const int eth = (late && jt == 0) ? 0x7fffffff : s_low;
      VC_EPILOGUE(ejt, eth)
      if (late) mfma_phase<KS, RT>(afrag, acc, slot, lane, produce);
    }
    if (late) { VC_EPILOGUE(n_ct - 1, s_low) }
    }
#undef VC_TILE_HEAD
#undef VC_EPILOGUE

    // ---- row results of this pass ------------------------------------------------------
    reduce_rows<RT, FUSED>(rbest, rsec, rscratch, lane, c, h, tile0, n1, [&](int row, int best, int second, int idx) {
      if (FUSED) { rbest_s[row] = best; rsecond_s[row] = second; ridx_s[row] = idx; }
      else { o_idx[row] = idx; o_best[row] = best; o_second[row] = second; }
    });
  }  // passes

  if (!FUSED) return;
  __syncthreads();

  // ---- angle + ratio tests, cross check, ordered compaction -----------------------------
  auto finalise = [&](auto accept) {
    return finalise_pair(accept, [&](int j) { return ColState{colbest[j], colsecond[j], 0u}; }, m21, rbest_s, rsecond_s, ridx_s,
                         n1, n2, cross_check, tid, lane, wave, wave_count, out_matches + (size_t)p * n_max * 2);
  };
  int n_matches;
  if constexpr (GUIDED) n_matches = finalise(AcceptTable{max_ratio, max_distance, s_low});
  else n_matches = finalise(AcceptAcos{max_ratio, max_distance});
  if (tid == 0) out_counts[p] = n_matches;
}

// ---------------------------------------------------------------------------------------
// The persistent pair kernel (KS <= 12, two row tiles per wave): what vc_match_pairs_u8 launches.
// ---------------------------------------------------------------------------------------
// Same arithmetic, tile loop and LDS layout as pair_kernel<KS, 2, true>; what differs is everything AROUND
// the tile loop, which is where a workgroup of pair_kernel spent a third of its time with the matrix pipe idle
// (measured: a launch with epilogue, staging and finalisation compiled out still ran at 55 % of the int8 peak):
//   * one workgroup per CU walks a CONTIGUOUS range of the pair list.  The exhaustive list is ordered by
//     image a, so consecutive pairs share it: the A fragments (96 VGPRs per wave, 192 KiB per workgroup) are
//     re-fetched only when a (or the row pass) changes, not once per pair;
//   * the B ring never drains: the producer cursor runs over the flattened (pair, pass, column tile) sequence,
//     so the first tiles of the next pair are already in LDS while the current one is finalised;
//   * the next pair's column sums are fetched into registers before the current pair's tile loop;
//   * the angle / ratio tests read theta from a table (accept_tab) — no double-precision acos, so the
//     finalisation is short and its registers do not collide with the fragments that stay live across it;
//   * the accumulators start from the row term (read from LDS as the MFMA's C operand) instead of zero: the
//     relevance test of a 32x32 tile is then a maximum over the lane's 16 accumulators against a per-lane
//     threshold (9 VALU instead of 24), and an update key is one shift-add.
// Block -> range mapping: blocks b and b + 8 share an XCD (round robin), so ranges are dealt such that each
// XCD owns a contiguous eighth of the pair list (neighbouring pairs share image a in that XCD's L2).
struct PairInfo {     // wave-uniform description of one pair with work (n_ct * n_pass > 0)
  int p;              // index in the pair list (>= hi: none)
  int a, n1, n2, n_ct, n_pass;
  const uint8_t* b_frags;
};

constexpr int kPairWindow = 32;      // pairs-with-work described in LDS at a time (half a wave builds the list)
constexpr int kProd2 = kWaves / 2;   // LDS-DMA pieces are issued by the early half (waves 0..3)
constexpr int kTilesPerBarrier = 2;

// pair2_kernel's dynamic LDS (see pair_lds): the ring, column records of 16 bytes, column terms, m21 + row results, three
// row-term arrays per wave (full, head, full - head), row-reduce scratch, head column terms + tile bounds of b, the copy
// of the NEXT pair's column sums / tile bounds (LDS-DMA), the pair window
struct Pair2Lds {
  u32 col;                       // [n_pad] ColState
  u32 cterm;                     // [n_pad] (kept out of the 16-byte column records: a stride-16 read is 4-way bank conflicted, -3 %)
  u32 m21, rbest, rsecond, ridx; // [n_pad] as in PairLds
  u32 crow6;                     // [wave][64] row terms 128*ra - 49024*D
  u32 rscratch;                  // [wave][kRowScratchEntries] uint2: reduce_rows
  u32 pair_flag;                 // [1] some tile of the current pair was relevant (not next to cursor_chk: hipcc then resets
                                 //     all three words with one 12-byte store of constants it keeps across the pair loop, and spills)
  u32 wave_count;                // [kWaves] append_ordered
  u32 cursor_chk;                // [2] max, min over the waves' ring cursors
  // early-out state (head_steps_of(KS) < KS): head column terms, tail norm bounds of b's tiles, head row terms per wave
  u32 cterm_h;                   // [n_pad]
  u32 tnb;                       // [n_pad / 32]
  u32 crow6h;                    // [wave][64] HEAD row terms 128*ra_head - 49024*D_head
  // column sums (packed with the early-out) and tile bounds of the NEXT pair's image b, copied in by LDS-DMA while the
  // current pair runs (no global load, hence no compiler vmcnt wait, at a pair boundary)
  u32 auxw;                      // [n_pad]
  u32 auxt;                      // [n_pad / 32]
  u32 winfo;                     // [kPairWindow] int4 {p, a, b, n1 | n2 << 16}: pairs with work, in order
  u32 wmeta;                     // [4] [0]: entries in the window
  u32 crow6d;                    // [wave][64] full minus head row term (added when the early-out test fails)
  u32 end;
};
__host__ __device__ constexpr Pair2Lds pair2_lds(u32 ring_bytes, int n_pad) {
  LdsCursor c{ring_bytes};
  Pair2Lds l{};
  l.col = c.take(n_pad * 16, 16);
  l.cterm = c.take(n_pad * 4);
  l.m21 = c.take(n_pad * 4);
  l.rbest = c.take(n_pad * 4);
  l.rsecond = c.take(n_pad * 4);
  l.ridx = c.take(n_pad * 4);
  l.crow6 = c.take(kWaves * 64 * 4, 16);
  l.rscratch = c.take(kWaves * kRowScratchBytes, 8);
  l.pair_flag = c.take(4);
  l.wave_count = c.take(kWaves * 4);
  l.cursor_chk = c.take(2 * 4);
  l.cterm_h = c.take(n_pad * 4);
  l.tnb = c.take(n_pad / kTile * 4);
  l.crow6h = c.take(kWaves * 64 * 4, 16);
  l.auxw = c.take(n_pad * 4, 16);
  l.auxt = c.take(n_pad / kTile * 4);
  l.winfo = c.take(kPairWindow * 16, 16);
  l.wmeta = c.take(4 * 4);
  l.crow6d = c.take(kWaves * 64 * 4, 16);
  l.end = c.take(0, 16);
  return l;
}
constexpr int plan_slots2(int ks, int n_pad) { return slots_beside(pair2_lds(0, n_pad).end, ks, min_slots(2, true)); }
constexpr bool pair2_lds_ok(int ks) {
  const Pair2Lds l = pair2_lds(plan_slots2(ks, kMaxPad) * ks * kFragBytes, kMaxPad);
  return l.end <= (u32)kLdsBytes && l.col % 16 == 0 && l.rscratch % 8 == 0 && l.crow6 % 16 == 0 && l.crow6h % 16 == 0 &&
         l.crow6d % 16 == 0 && l.auxw % 16 == 0 && l.winfo % 16 == 0;
}
static_assert(pair2_lds_ok(2) && pair2_lds_ok(4) && pair2_lds_ok(8) && pair2_lds_ok(12),
              "pair2_kernel's LDS plan: size and alignment at the largest block");
// Which lengths ever need the fallback to pair_kernel<KS, 2, true> (vc_match_pairs_u8): only those whose plan does not
// fit at the largest block.
constexpr bool persistent_always_fits(int ks) { return ks <= kMaxKs2 && plan_slots2(ks, kMaxPad) > 0; }
static_assert(persistent_always_fits(2) && persistent_always_fits(4) && persistent_always_fits(8), "no fallback below KS = 12");
static_assert(!persistent_always_fits(12), "KS = 12 at 2048 rows leaves two ring slots: the fallback is live");

template <int KS>
__global__ __launch_bounds__(kThreads, 2) void pair2_kernel(
    const uint8_t* __restrict__ prepared, const int32_t* __restrict__ counts, int n_tiles_img, int d,
    const int32_t* __restrict__ pairs, int n_pairs, float max_ratio, float max_distance, int cross_check,
    int n_max, int ns, int s_low, uint32_t* __restrict__ out_matches, int32_t* __restrict__ out_counts) {
  static_assert(kWaves == 8, "the persistent kernel is written for eight-wave workgroups");
  constexpr int RT = 2;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int n_pad = n_tiles_img * kTile;
  uint8_t* ring = smem;
  const Pair2Lds lds = pair2_lds((u32)ns * (KS * kFragBytes), n_pad);
  ColState* col = (ColState*)(smem + lds.col);
  int* cterm = (int*)(smem + lds.cterm);
  int* m21 = (int*)(smem + lds.m21);
  int* rbest_s = (int*)(smem + lds.rbest);
  int* rsecond_s = (int*)(smem + lds.rsecond);
  int* ridx_s = (int*)(smem + lds.ridx);
  int* crow6 = (int*)(smem + lds.crow6);
  int* wave_count = (int*)(smem + lds.wave_count);
  int* cterm_h = (int*)(smem + lds.cterm_h);
  int* tnb = (int*)(smem + lds.tnb);
  int* crow6h = (int*)(smem + lds.crow6h);
  int* auxw = (int*)(smem + lds.auxw);
  int* auxt = (int*)(smem + lds.auxt);
  int4* winfo = (int4*)(smem + lds.winfo);
  int* wmeta = (int*)(smem + lds.wmeta);
  int* crow6d = (int*)(smem + lds.crow6d);
  constexpr int KH = head_steps_of(KS);
  constexpr bool kEarlyOut = KH < KS;
  const int d_head = min(d, KH * 32);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 31, h = lane >> 5;
  uint2* rscratch = (uint2*)(smem + lds.rscratch) + wave * kRowScratchEntries;  // this wave's slice
  int* crow6_wave = crow6 + wave * 64;
  int* crow6h_wave = crow6h + wave * 64;
  int* crow6d_wave = crow6d + wave * 64;
  const size_t img_stride = image_bytes(n_tiles_img, KS);
  const size_t frag_bytes_img = (size_t)n_tiles_img * KS * kFragBytes;
  // readfirstlane written out here rather than vc::lds_addr: through the helper the compiler moves the address-space cast
  // behind the readfirstlane and allocates this kernel's SGPRs differently
  const u32 ring_lds = (u32)__builtin_amdgcn_readfirstlane((int)vc::lds_offset(ring));

  // this workgroup's range of the pair list
  const int G = gridDim.x;
  const int cid = (G % 8 == 0) ? (int)(blockIdx.x % 8) * (G / 8) + (int)(blockIdx.x / 8) : (int)blockIdx.x;
  const int lo = (int)(((long long)cid * n_pairs) / G);
  const int hi = (int)(((long long)(cid + 1) * n_pairs) / G);

  // ---- the pairs of the range that have work, kPairWindow at a time ------------------------------------------------
  // One wave reads 64 pairs and their counts at once, writes zero counts for those with an empty image and lists the
  // others in LDS; the per-pair description is then an LDS read.  (Read pair by pair with scalar loads, two dependent
  // round trips sat between every two pairs.)  fetch() is called by all waves at the same points, between pairs.
  int w_i = 0, w_n = 0, w_base = lo;   // wave-uniform
  auto fetch = [&]() -> PairInfo {
    PairInfo r;
    r.p = hi; r.a = 0; r.n1 = 0; r.n2 = 0; r.n_ct = 0; r.n_pass = 0; r.b_frags = prepared;
    while (w_i == w_n) {
      if (w_base >= hi) return r;
      __syncthreads();   // nobody is still reading the list this round replaces
      if (wave == kWaves - 1) {
        const int q = lane < kPairWindow ? w_base + lane : hi;
        int a = 0, b = 0, n1 = 0, n2 = 0;
        if (q < hi) {
          a = pairs[2 * q]; b = pairs[2 * q + 1];
          n1 = min(max(counts[a], 0), n_max); n2 = min(max(counts[b], 0), n_max);
        }
        const bool work = q < hi && n1 > 0 && n2 > 0;
        if (q < hi && !work) out_counts[q] = 0;   // an empty image: nothing can match
        const unsigned long long mask = __ballot(work);
        if (work) winfo[__popcll(mask & ((1ull << lane) - 1ull))] = make_int4(q, a, b, n1 | (n2 << 16));
        if (lane == 0) wmeta[0] = __popcll(mask);
      }
      __syncthreads();
      w_n = __builtin_amdgcn_readfirstlane(wmeta[0]);
      w_i = 0;
      w_base = min(w_base + kPairWindow, hi);
    }
    const int4 e = winfo[w_i++];
    r.p = __builtin_amdgcn_readfirstlane(e.x);
    r.a = __builtin_amdgcn_readfirstlane(e.y);
    const int b = __builtin_amdgcn_readfirstlane(e.z);
    const int nn = __builtin_amdgcn_readfirstlane(e.w);
    r.n1 = nn & 0xffff; r.n2 = nn >> 16;
    r.n_ct = ceil_div(r.n2, kTile);
    r.n_pass = ceil_div(r.n1, kWaves * 2 * kTile);
    r.b_frags = prepared + (size_t)b * img_stride;
    return r;
  };
  PairInfo cur = fetch();
  if (cur.p >= hi) return;
  PairInfo nxt = fetch();

  // ---- producer: a stream of column tiles over (pair, pass, tile), PF tiles ahead of the consumer ----------
  // It sweeps the current pair's image b once per row pass, then moves on to the NEXT pair (whose description is
  // already in registers), so the ring stays full across the pair boundary.  It never runs more than one pair
  // ahead: a next pair shorter than the ring leaves it idle until the consumer gets there.
  const int tpb = ns >= 6 ? kTilesPerBarrier : 1;   // a short ring (large blocks) keeps its depth: one tile per barrier
  const int pf = ns - tpb;
  const uint8_t* p_src = cur.b_frags;      // next tile to stage
  const uint8_t* p_base = cur.b_frags;
  int p_left = cur.n_ct, p_nct = cur.n_ct, p_sweeps = cur.n_pass;
  bool p_on_next = false, p_active = true;
  int prod_seq = 0, prod_slot = 0, cons_seq = 0, cons_slot = 0;
  auto produce = [&]() {
    if (p_active) {
      stage_tile<KS, kProd2>(p_src, ring_lds + (u32)prod_slot * (KS * kFragBytes), wave, lane);
      ++prod_seq;
      if (++prod_slot == ns) prod_slot = 0;
      p_src += KS * kFragBytes;
      if (--p_left == 0) {
        if (--p_sweeps > 0) {
          p_src = p_base; p_left = p_nct;
        } else if (!p_on_next && nxt.p < hi) {
          p_on_next = true;
          p_src = p_base = nxt.b_frags; p_left = p_nct = nxt.n_ct; p_sweeps = nxt.n_pass;
        } else {
          p_active = false;
        }
      }
    }
  };
  for (int i = 0; i < pf; ++i) produce();

  int* pair_flag = (int*)(smem + lds.pair_flag);   // "some tile of the current pair was relevant"
  // Cursor check: prod_seq / cons_seq exist once per wave (SGPRs) and must agree across the workgroup — `two`, the slot
  // indices and the counted waits are all derived from them.  Every wave folds its pair of cursors into a max and a min
  // word at the end of a pair's tile loop; if they differ the pair's count is written as -1 instead of a match count.
  int* cursor_chk = (int*)(smem + lds.cursor_chk);   // [2]: max, min over the waves
  // with the early-out the per-row word is the packed (head << 16 | tail) sum, else the plain row sum
  const int rs_off = kEarlyOut ? n_pad : 0;
  // Image b's column sums for pair X travel by LDS-DMA into the aux buffer, issued by one LATE wave (which has no other
  // copy in flight, so its vmcnt(0) waits for exactly these) behind the first barrier of the pair before X — every
  // thread has read that pair's own sums by then — and are read a whole pair later, after that wave's wait and the
  // barrier that ends the pair in between.
  constexpr int kAuxWave = kWaves / 2;
  const u32 auxw_lds = (u32)__builtin_amdgcn_readfirstlane((int)vc::lds_offset(auxw));
  const u32 auxt_lds = (u32)__builtin_amdgcn_readfirstlane((int)vc::lds_offset(auxt));
  auto stage_aux = [&](const PairInfo& pi) {
    if (wave == kAuxWave && pi.p < hi) {
      int ln = lane;   // (laundered: lane-derived addresses are computed here, not carried across the tile loop)
      asm volatile("" : "+v"(ln));
      const uint8_t* sums = pi.b_frags + frag_bytes_img + (size_t)rs_off * 4;
      const int pieces = ceil_div(pi.n_ct * kTile, 256);            // 1 KiB = 256 column words per piece
      for (int i = 0; i < pieces; ++i)
        glds16(sums + (size_t)i * 1024 + ln * 16, auxw_lds + (u32)(i * 1024));
      if (kEarlyOut && ln < pi.n_ct)
        glds4(pi.b_frags + frag_bytes_img + (size_t)2 * n_pad * 4 + ln * 4, auxt_lds);
    }
  };
  stage_aux(cur);
  if (wave == kAuxWave) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  // The two waves of a SIMD (w and w + 4) run half a tile apart, see pair_kernel.  (On the final kernel: without it the
  // dense path loses 6 % and the sparse one gains 1.5-3 %; switching it per pair — on only behind a pair with relevant
  // similarities — was slower on both, 17.7 vs 18.1 M and 7.58 vs 7.71 M pairs/s: `late` is better a per-wave constant.)
  const bool late = wave >= kWaves / 2;
  v4i afrag[RT][KS];
  int cur_a = -1, cur_tile0 = -1;
  int tna = 0;   // the larger tail norm bound of this wave's two row tiles (wave-uniform)
  int early_score = 0, early_probe = 0;   // gate of the early-out (wave-uniform, kept across pairs)
  bool pairs_dense = false;               // the previous pair held relevant similarities (workgroup-uniform)
  v16i acc[RT];   // (the late half's first epilogue of a pass looks at stale accumulators behind an unreachable threshold)
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[rt][r] = 0;

  while (true) {
    const int p = cur.p;
    const int n1 = cur.n1, n2 = cur.n2, n_ct = cur.n_ct, n_pass = cur.n_pass;
    const uint8_t* a_frags = prepared + (size_t)cur.a * img_stride;
    const int32_t* a_rowsum = (const int32_t*)(a_frags + frag_bytes_img);

    // ---- per-pair LDS state (the previous pair's finalisation ended with a barrier) ---------------------------
    // (columns 0..511 come from the register fetched during the previous pair: the load's latency was 2 k cycles
    // of every pair when it sat here)
    auto init_column = [&](int j, int word) {
      const int head = kEarlyOut ? packed_head(word) : 0, total = kEarlyOut ? head + packed_tail(word) : word;
      if (kEarlyOut) cterm_h[j] = 128 * head + 32640 * d_head;
      cterm[j] = 128 * total + 32640 * d;
      col[j].best = 0ull;
      col[j].second = 0u;
    };
    // Per-pair code indexes through a laundered copy of the thread id: with `tid` itself the compiler keeps a dozen
    // LDS / global addresses alive across the tile loop, spills them, and every reload costs an s_waitcnt vmcnt that
    // drains the LDS-DMA ring (the compiler cannot see the copies in flight).  A few more VALU instructions per pair.
    int tidp = tid;
    asm volatile("" : "+v"(tidp));
    for (int j = tidp; j < n_ct * kTile; j += kThreads) init_column(j, auxw[j]);
    if (kEarlyOut && tidp < n_ct) tnb[tidp] = auxt[tidp];
    for (int i = tidp; i < n1; i += kThreads) { rbest_s[i] = 0; rsecond_s[i] = 0; ridx_s[i] = -1; }
    if (tidp == 0) { *pair_flag = 0; cursor_chk[0] = (int)0x80000000; cursor_chk[1] = 0x7fffffff; }
    bool pair_hit = false;   // some tile of this wave held a relevant similarity

    for (int pass = 0; pass < n_pass; ++pass) {
      const int tile0 = (pass * kWaves + wave) * RT;  // first 32-row tile of a owned by this wave
      if (cur.a != cur_a || tile0 != cur_tile0) {     // wave-uniform: a new image a or a new row pass
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
          for (int kk = 0; kk < KS; ++kk)
            afrag[rt][kk] = *(const v4i*)(a_frags + ((size_t)(tile0 + rt) * KS + kk) * kFragBytes + lane * 16);
        // row term of this lane's row (lane <-> row tile0*32 + lane of the wave's RT*32 rows); the slice is
        // wave-private and its LDS operations execute in order
        {
          const int word = a_rowsum[rs_off + tile0 * kTile + lane];
          const int head = kEarlyOut ? packed_head(word) : 0, total = kEarlyOut ? head + packed_tail(word) : word;
          crow6_wave[lane] = 128 * total - 49024 * d;
          if (kEarlyOut) {
            crow6h_wave[lane] = 128 * head - 49024 * d_head;
            crow6d_wave[lane] = (128 * total - 49024 * d) - (128 * head - 49024 * d_head);
            tna = __builtin_amdgcn_readfirstlane(max(a_rowsum[2 * n_pad + tile0], a_rowsum[2 * n_pad + tile0 + 1]));
          }
        }
        cur_a = cur.a;
        cur_tile0 = tile0;
        // The fragments must have landed before the tile loop: left pending, the compiler's own wait counts for
        // their first use land INSIDE the loop (vmcnt(0) after the last MFMA) and drain the LDS-DMA prefetch of
        // every tile.  vmcnt(0), other counters untouched (gfx9 encoding); a builtin, so the compiler sees it.
        __builtin_amdgcn_s_waitcnt(0x0F70);
      }
      u32 rbest[RT][16], rsec[RT][16];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int r = 0; r < 16; ++r) { rbest[rt][r] = 0; rsec[rt][r] = 0; }
      const u32 row_base = (u32)(tile0 * kTile);

      int ct = 0;   // column term of the tile whose epilogue comes next; always read ahead of an MFMA phase
      int cut = 0;  // row tiles of that tile the early-out cut short (wave-uniform)
      // thresholds of the early-out for column tile jt: acc_head > s_low - cth - TNa TNb  <=>  the tile may still matter
      // When to try it: a saturating score (+2 for a tile cut short, -1 for a failed test, which costs the test and the
      // row-term fix-up but no MFMA) gates it, and while the score is negative one tile in 32 probes whether the data has
      // changed.  It stays on while one test in three succeeds; data on which it never does pays < 1 % for the probes.
      auto mfma_tile = [&](int jt, const uint8_t* slot) -> int {
        if (kEarlyOut && s_low >= 0 && (early_score >= 0 || --early_probe <= 0)) {   // (s_low = -1: nothing may be skipped)
          const int thr = s_low - cterm_h[jt * kTile + c] - __mul24(tna, tnb[jt]);
          const int r = mfma_phase2<KS, true>(afrag, acc, slot, crow6_wave, crow6h_wave, crow6d_wave, lane, h, thr, produce);
          if (r != 0) early_score = min(early_score + 2, 8);
          else { early_score = max(early_score - 1, -8); early_probe = 32; }
          return r;
        }
        return mfma_phase2<KS, false>(afrag, acc, slot, crow6_wave, crow6h_wave, crow6d_wave, lane, h, 0, produce);
      };
      // One barrier per TWO column tiles (with two thirds of the MFMAs gone a tile is ~2400 cycles of which ~590 went into
      // the vmcnt wait, the barrier and the arrival skew).  The barrier publishes both tiles; the ring runs ns - 2 tiles
      // ahead so that the copy issued during the second tile never lands in a slot a slower wave is still reading.
      auto one_tile = [&](int jt, const uint8_t* slot) {
        if (!late) {
          ct = cterm[jt * kTile + c];
          cut = mfma_tile(jt, slot);
        }
        const int ejt = late ? (jt > 0 ? jt - 1 : 0) : jt;
        const int eth = (late && jt == 0) ? 0x7fffffff : s_low;
        pair_hit |= epilogue_phase2(acc, rbest, rsec, ct, col, ejt, c, h, row_base, eth, cut);
        if (late) {
          ct = cterm[jt * kTile + c];
          cut = mfma_tile(jt, slot);
        }
      };
      for (int jt = 0; jt < n_ct;) {
        // (both tiles must be staged already: not so right after the producer idled — tiny images — or with a short ring)
        // Pairs after one that held relevant similarities run one tile per barrier: with the update path in every
        // epilogue the late half's deferred epilogue is the longer part and pairing the tiles loses 3 %.
        const bool two = tpb == 2 && !pairs_dense && jt + 1 < n_ct && prod_seq - cons_seq >= 2;
        // this wave's pieces of the tile(s) of this round have landed once only the younger tiles are pending
        wait_tile<KS, kProd2>(wave, max(prod_seq - cons_seq - (two ? 2 : 1), 0));
        wg_barrier();
        if (jt == 0 && pass == 0) stage_aux(nxt);   // (every thread is past this pair's initialisation)
        const int n_sub = two ? 2 : 1;
        {
          // (Straight-line on purpose.  As a second trip through ONE copy of this body hipcc 7.2.0 gave the SGPR pair that
          // carries produce()'s p_active across the back edge to the early-out gate as well: waves on the variant with the
          // test then saw the producer inactive, the waves of a workgroup disagreed on `two` and barriers paired up wrongly —
          // profiles/r03_matcher_looped_miscompile.md, tools/repro/looped_sub.patch.  The cursor check at the end of every pair
          // (below) turns that class of fault into an error code instead of a wrong match list.)
          const uint8_t* slot = ring + (size_t)cons_slot * KS * kFragBytes;
          if (++cons_slot == ns) cons_slot = 0;
          ++cons_seq;
          one_tile(jt, slot);
          if (two) {
            const uint8_t* slot2 = ring + (size_t)cons_slot * KS * kFragBytes;
            if (++cons_slot == ns) cons_slot = 0;
            ++cons_seq;
            one_tile(jt + 1, slot2);
          }
        }
        jt += n_sub;
      }
      if (late) pair_hit |= epilogue_phase2(acc, rbest, rsec, ct, col, n_ct - 1, c, h, row_base, s_low, cut);

      // ---- row results of this pass ----------------------------------------------------------------------------
      reduce_rows<RT, true>(rbest, rsec, rscratch, lane, c, h, tile0, n1, [&](int row, int best, int second, int idx) {
        rbest_s[row] = best; rsecond_s[row] = second; ridx_s[row] = idx;
      });
    }  // passes

    int tidf = tid;   // (as tidp: the finalisation's addresses are computed here, not carried through the tile loop)
    asm volatile("" : "+v"(tidf));
    if (pair_hit && lane == 0) atomicOr(pair_flag, 1);
    if (lane == 0) {
      const int cursors = (cons_seq & 0xffff) | ((prod_seq & 0x7fff) << 16);
      atomicMax(&cursor_chk[0], cursors);
      atomicMin(&cursor_chk[1], cursors);
    }
    __syncthreads();
    const int pair_was_hit = __builtin_amdgcn_readfirstlane(*pair_flag);
    const bool cursors_agree = __builtin_amdgcn_readfirstlane(cursor_chk[0]) == __builtin_amdgcn_readfirstlane(cursor_chk[1]);
    pairs_dense = pair_was_hit != 0;   // (workgroup-uniform: every wave reads the same word behind the barrier)
    if (pair_was_hit == 0) {
      // No tile of the pair held a similarity above the relevance threshold: every row's best stays below what the
      // angle test accepts, the match list is empty and nothing of the finalisation has to run.
      if (tidf == 0) out_counts[p] = cursors_agree ? 0 : VC_COUNT_SELFCHECK_FAILED;
    } else {
    // ---- angle + ratio tests, cross check, ordered compaction ---------------------------------------------------
    // (finalise_pair's steps written out: through the shared function this kernel's 2048 x 256 sparse rate fell 0.5 % below
    // what it is with its own copy, whichever way lane / wave reached append_ordered)
    if (cross_check) {
      for (int j = tidf; j < n2; j += kThreads) {
        const unsigned long long kb = col[j].best;
        const int row = (int)(0xFFFFFFFFu - (u32)kb);
        m21[j] = accept_tab((int)(kb >> 32), (int)col[j].second, max_ratio, max_distance, s_low) ? row : -1;
      }
      __syncthreads();
    }
    uint32_t* out = out_matches + (size_t)p * n_max * 2;
    int base = 0;
    for (int i0 = 0; i0 < n1; i0 += kThreads) {
      const int i = i0 + tidf;
      bool ok = false;
      int j = -1;
      if (i < n1) {
        j = ridx_s[i];
        ok = accept_tab(rbest_s[i], rsecond_s[i], max_ratio, max_distance, s_low);
        if (ok && cross_check) ok = (m21[j] == i);
      }
      const unsigned long long mask = __ballot(ok);
      if (lane == 0) wave_count[wave] = __popcll(mask);
      __syncthreads();
      int before = base, chunk_total = 0;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) {
        const int wc = wave_count[w];
        before += w < wave ? wc : 0;
        chunk_total += wc;
      }
      if (ok) {
        const int pos = before + __popcll(mask & ((1ull << lane) - 1ull));
        out[2 * pos] = (uint32_t)i;
        out[2 * pos + 1] = (uint32_t)j;
      }
      base += chunk_total;
      __syncthreads();
    }
    if (tidf == 0) out_counts[p] = cursors_agree ? base : VC_COUNT_SELFCHECK_FAILED;
    }
    // the next pair's column sums (copied in during this pair) have landed before the barrier that lets it start
    if (wave == kAuxWave) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();   // the flag and the per-pair state are rewritten by the next pair's initialisation

    // ---- on to the next pair with work ---------------------------------------------------------------------------
    if (nxt.p >= hi) break;
    cur = nxt;
    nxt = fetch();
    if (p_on_next) {
      p_on_next = false;               // the producer's pair is the consumer's pair again
    }
    if (!p_active && nxt.p < hi) {     // the producer had run out of described work: resume on the new next pair
      p_active = true; p_on_next = true;
      p_src = p_base = nxt.b_frags; p_left = p_nct = nxt.n_ct; p_sweeps = nxt.n_pass;
    }
  }  // pairs
}

// ---------------------------------------------------------------------------------------
// small kernels
// ---------------------------------------------------------------------------------------
__global__ void mutual_ratio_kernel(const int32_t* idx12, const int32_t* best12, const int32_t* second12,
                                    int n1, const int32_t* idx21, const int32_t* best21,
                                    const int32_t* second21, int n2, float max_ratio,
                                    float max_distance, int cross_check, uint32_t* out_pairs,
                                    int32_t* out_count) {
  // single workgroup of kThreads: ordered compaction over i
  __shared__ int wave_count[kWaves];
  const int tid = threadIdx.x;
  int base = 0;
  for (int i0 = 0; i0 < n1; i0 += kThreads) {
    const int i = i0 + tid;
    bool ok = false;
    int j = -1;
    if (i < n1) {
      j = idx12[i];
      ok = j >= 0 && j < n2 && accept_dev(best12[i], second12[i], max_ratio, max_distance);
      if (ok && cross_check)
        ok = idx21[j] == i && accept_dev(best21[j], second21[j], max_ratio, max_distance);
    }
    base = append_ordered(ok, i, j, base, wave_count, out_pairs, tid & 63, tid >> 6);
  }
  if (tid == 0) *out_count = base;
}

__global__ void knn_setup_kernel(int32_t* meta, int n1, int n2) {
  meta[0] = n1; meta[1] = n2;   // counts
  meta[2] = 0;  meta[3] = 1;    // the pair
}

__global__ void theta_table_kernel(float* out, int n, int from_table) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s < n) out[s] = from_table ? theta_tab(s) : theta(s);
}

// ---------------------------------------------------------------------------------------
// relevance threshold (host side launch parameter)
// ---------------------------------------------------------------------------------------
// Largest similarity that can be ignored by the searches without changing the match list.
//   S_T   = smallest s with theta(s) <= max_distance: a best below it is always rejected.
//   S_low = largest s (< S_T) with max_ratio * theta(s) > theta(S_T).
// Take a row (or column) with top-2 (b, s2) and drop any elements <= S_low from its scan:
//   b <  S_T : rejected before and after (the best can only shrink).
//   b >= S_T : b > S_low, so the best and its index are untouched.  If s2 > S_low it is untouched
//              too.  If s2 <= S_low, then max_ratio*theta(s2) >= max_ratio*theta(S_low) >
//              theta(S_T) >= theta(b): the ratio test passes, and it passes just the same with
//              whatever smaller runner-up is found instead.
// theta is non-increasing in s and multiplication by a non-negative float is monotone, so both
// thresholds are found by bisection.  A margin of 4 absorbs a last-bit difference between the
// host's and the device's acos (one ulp of theta moves a threshold by < 0.01).
// Returns -1 ("nothing can be ignored") for parameters outside the monotone regime.
inline int relevance_threshold(float max_ratio, float max_distance) {
  if (!(max_ratio >= 0.0f) || !(max_distance == max_distance)) return -1;
  constexpr int kSat = 512 * 512;
  if (theta(kSat) > max_distance) return kSat;  // nothing is ever accepted (max_distance < 0)
  int lo = 0, hi = kSat;  // smallest s with theta(s) <= max_distance
  while (lo < hi) {
    const int mid = (lo + hi) / 2;
    if (theta(mid) <= max_distance) hi = mid; else lo = mid + 1;
  }
  const int s_t = lo;
  const float t_t = theta(s_t);
  if (!(max_ratio * theta(0) > t_t)) return -1;
  lo = 0; hi = s_t > 0 ? s_t - 1 : 0;  // largest s with max_ratio*theta(s) > t_t
  while (lo < hi) {
    const int mid = (lo + hi + 1) / 2;
    if (max_ratio * theta(mid) > t_t) lo = mid; else hi = mid - 1;
  }
  int s_low = lo < s_t - 1 ? lo : s_t - 1;
  s_low -= 4;
  return s_low < -1 ? -1 : s_low;
}

inline int pick_ks(int d) {
  const int need = ksteps_of(d);
  for (int ks : kKsList)
    if (ks >= need) return ks;
  return -1;
}

void launch_prepare(const uint8_t* desc, const int32_t* counts, int n_images, int n_max, int d, int n_tiles, void* prepared,
                    hipStream_t stream) {
  hipLaunchKernelGGL(prepare_kernel, dim3(n_tiles, n_images), dim3(256), 0, stream, desc, counts, n_max, d, n_tiles,
                     pick_ks(d), (uint8_t*)prepared);
}

// what every pair launch is given
struct MatchJob {
  const void* prepared;
  const int32_t* counts;
  int n_tiles, d;
  const int32_t* pairs;
  int n_pairs;
  float max_ratio, max_distance;
  int cross_check, n_max;
  uint32_t* out_matches;
  int32_t* out_counts;
  hipStream_t stream;
};

// the pair kernels may use the whole LDS: set once per kernel and device
template <auto Kernel>
int allow_full_lds() {
  static vc::PerDeviceOnce configured;
  return vc::allow_dynamic_lds(configured, kLdsBytes, Kernel);
}

// pair_kernel: one workgroup per pair.  !FUSED: the one-way outputs instead of the match list; GUIDED: see GuidedArgs.
template <int KS, int RT, bool FUSED, bool GUIDED = false>
int launch_pair(const MatchJob& m, int32_t* o_idx, int32_t* o_best, int32_t* o_second,
                const GuidedArgs<GUIDED>& ga = GuidedArgs<GUIDED>()) {
  // The one-way API reports every row's best / second, so nothing may be skipped there.  The relevance shortcut holds for
  // the masked similarities of guided matching as it does for the plain ones: the rule is the same.
  const int s_low = FUSED ? relevance_threshold(m.max_ratio, m.max_distance) : -1;
  const int n_pad = m.n_tiles * kTile;
  const int ns = plan_slots(KS, n_pad, RT, GUIDED);
  if (ns == 0) return VC_ERR_UNSUPPORTED;
  if (int st = allow_full_lds<pair_kernel<KS, RT, FUSED, GUIDED>>()) return st;
  hipLaunchKernelGGL((pair_kernel<KS, RT, FUSED, GUIDED>), dim3(m.n_pairs), dim3(kThreads),
                     pair_lds(ns * KS * kFragBytes, n_pad, RT, GUIDED).end, m.stream, (const uint8_t*)m.prepared, m.counts,
                     m.n_tiles, m.d, m.pairs, m.max_ratio, m.max_distance, m.cross_check, m.n_max, ns, s_low, m.out_matches,
                     m.out_counts, o_idx, o_best, o_second, ga);
  return vc::check_launch();
}

// The persistent kernel: one workgroup per CU, each walking a contiguous range of the pair list.
template <int KS>
int launch_pair2(const MatchJob& m) {
  const int s_low = relevance_threshold(m.max_ratio, m.max_distance);
  const int n_pad = m.n_tiles * kTile;
  const int ns = plan_slots2(KS, n_pad);
  if (ns == 0) return VC_ERR_UNSUPPORTED;
  if (int st = allow_full_lds<pair2_kernel<KS>>()) return st;
  int cus = 0;
  if (int st = vc::cu_count(&cus)) return st;
  const int grid = m.n_pairs < cus ? m.n_pairs : cus;
  hipLaunchKernelGGL((pair2_kernel<KS>), dim3(grid), dim3(kThreads), pair2_lds(ns * KS * kFragBytes, n_pad).end, m.stream,
                     (const uint8_t*)m.prepared, m.counts, m.n_tiles, m.d, m.pairs, m.n_pairs, m.max_ratio, m.max_distance,
                     m.cross_check, m.n_max, ns, s_low, m.out_matches, m.out_counts);
  return vc::check_launch();
}

int launch_theta(float* out, int n, int from_table, vc_stream_t stream) {
  if (!out || n < 0) return VC_ERR_INVALID_ARG;
  if (n == 0) return VC_OK;
  hipLaunchKernelGGL(theta_table_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, out, n, from_table);
  return vc::check_launch();
}

}  // namespace

// ---------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------
extern "C" {

size_t vc_prepared_bytes(int n_images, int n_max, int d) {
  if (n_images <= 0 || n_max <= 0 || d <= 0) return 0;
  const int ks = pick_ks(d);
  if (ks < 0) return 0;
  return (size_t)n_images * image_bytes(tiles_of(n_max), ks);
}

int vc_prepare_descriptors(const uint8_t* desc, const int32_t* counts, int n_images, int n_max, int d,
                           void* prepared, vc_stream_t stream) {
  if (!desc || !prepared || n_images < 0 || n_max <= 0 || d <= 0) return VC_ERR_INVALID_ARG;
  if (n_max > VC_MAX_KEYPOINTS || d > VC_MAX_DESC_DIM) return VC_ERR_UNSUPPORTED;
  if (((uintptr_t)prepared) % 16 != 0) return VC_ERR_INVALID_ARG;
  if (n_images == 0) return VC_OK;
  launch_prepare(desc, counts, n_images, n_max, d, tiles_of(n_max), prepared, (hipStream_t)stream);
  return vc::check_launch();
}

int vc_match_pairs_u8(const void* prepared, const int32_t* counts, int n_images, int n_max, int d,
                      const int32_t* pairs, int n_pairs, float max_ratio, float max_distance,
                      int cross_check, uint32_t* out_matches, int32_t* out_counts, vc_stream_t stream) {
  if (!prepared || !counts || !pairs || !out_matches || !out_counts) return VC_ERR_INVALID_ARG;
  if (n_images <= 0 || n_max <= 0 || d <= 0 || n_pairs < 0) return VC_ERR_INVALID_ARG;
  if (n_max > VC_MAX_KEYPOINTS || d > VC_MAX_DESC_DIM) return VC_ERR_UNSUPPORTED;
  if (n_pairs == 0) return VC_OK;
  const MatchJob job = {prepared, counts, tiles_of(n_max), d, pairs, n_pairs, max_ratio, max_distance, cross_check, n_max,
                        out_matches, out_counts, (hipStream_t)stream};
  return vc::dispatch<VC_KS_LIST>(pick_ks(d), [&](auto k) {
    // descriptors up to 384 bytes: the persistent kernel (two row tiles per wave)
    if constexpr (persistent_always_fits(k)) {
      return launch_pair2<k>(job);
    } else {
      if constexpr (k <= kMaxKs2) {   // (blocks too large for its LDS plan: the kernel with one workgroup per pair)
        const int st2 = launch_pair2<k>(job);
        if (st2 != VC_ERR_UNSUPPORTED) return st2;
      }
      return launch_pair<k, row_tiles_of(k), true>(job, nullptr, nullptr, nullptr);
    }
  });
}

int vc_match_pairs_guided_u8(const void* prepared, const int32_t* counts, int n_images, int n_max, int d,
                             const float* keypoints_xy, const int32_t* pairs, int n_pairs, const float* models,
                             const int32_t* model_kind, float max_error, float max_ratio, float max_distance,
                             int cross_check, uint32_t* out_matches, int32_t* out_counts, vc_stream_t stream) {
  if (!prepared || !counts || !keypoints_xy || !pairs || !models || !model_kind || !out_matches || !out_counts)
    return VC_ERR_INVALID_ARG;
  if (n_images <= 0 || n_max <= 0 || d <= 0 || n_pairs < 0) return VC_ERR_INVALID_ARG;
  if (((uintptr_t)keypoints_xy) % 8 != 0 || !(max_error >= 0.f)) return VC_ERR_INVALID_ARG;
  if (n_max > VC_MAX_KEYPOINTS || d > VC_MAX_DESC_DIM) return VC_ERR_UNSUPPORTED;
  if (n_pairs == 0) return VC_OK;
  GuidedArgs<true> ga;
  ga.keypoints = keypoints_xy;
  ga.models = models;
  ga.kind = model_kind;
  ga.t2 = max_error * max_error;
  const MatchJob job = {prepared, counts, tiles_of(n_max), d, pairs, n_pairs, max_ratio, max_distance, cross_check, n_max,
                        out_matches, out_counts, (hipStream_t)stream};
  return vc::dispatch<VC_KS_LIST>(pick_ks(d), [&](auto k) {
    // one row tile per wave for every length: the geometric test needs the registers a second one would take
    return launch_pair<k, 1, true, true>(job, nullptr, nullptr, nullptr, ga);
  });
}

// workspace: prepared copies of d1 and d2 (each as a 1-image set, same n_max), a 2-entry counts
// array and one (0,1) pair record.
size_t vc_knn_workspace_bytes(int n1, int n2, int d) {
  const int n_max = n1 > n2 ? n1 : n2;
  if (n_max <= 0 || d <= 0 || pick_ks(d) < 0) return 0;
  return 2 * image_bytes(tiles_of(n_max), pick_ks(d)) + 64;
}

int vc_knn_top2_u8(const uint8_t* d1, int n1, const uint8_t* d2, int n2, int d, int32_t* out_idx,
                   int32_t* out_best, int32_t* out_second, void* workspace, size_t workspace_bytes,
                   vc_stream_t stream) {
  if (n1 < 0 || n2 < 0 || d <= 0) return VC_ERR_INVALID_ARG;
  if (n1 == 0) return VC_OK;
  if (!d1 || !out_idx || !out_best || !out_second || !workspace) return VC_ERR_INVALID_ARG;
  if (n2 > 0 && !d2) return VC_ERR_INVALID_ARG;
  const int n_max = n1 > n2 ? n1 : n2;
  if (n_max > VC_MAX_KEYPOINTS || d > VC_MAX_DESC_DIM) return VC_ERR_UNSUPPORTED;
  if (((uintptr_t)workspace) % 16 != 0) return VC_ERR_INVALID_ARG;
  if (workspace_bytes < vc_knn_workspace_bytes(n1, n2, d)) return VC_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const int ks = pick_ks(d), n_tiles = tiles_of(n_max);
  const size_t img = image_bytes(n_tiles, ks);
  uint8_t* ws = (uint8_t*)workspace;
  int32_t* meta = (int32_t*)(ws + 2 * img);
  hipLaunchKernelGGL(knn_setup_kernel, dim3(1), dim3(1), 0, s, meta, n1, n2);
  // each set is prepared as image 0 of its own 1-image block, with its own row count
  launch_prepare(d1, meta + 0, 1, n1, d, n_tiles, ws, s);
  if (n2 > 0) launch_prepare(d2, meta + 1, 1, n2, d, n_tiles, ws + img, s);
  int st = vc::check_launch();
  if (st != VC_OK) return st;
  const MatchJob job = {ws, meta, n_tiles, d, meta + 2, 1, 0.f, 0.f, 0, n_max, nullptr, nullptr, s};
  return vc::dispatch<VC_KS_LIST>(ks, [&](auto k) {
    return launch_pair<k, row_tiles_of(k), false>(job, out_idx, out_best, out_second);
  });
}

int vc_mutual_ratio(const int32_t* idx12, const int32_t* best12, const int32_t* second12, int n1,
                    const int32_t* idx21, const int32_t* best21, const int32_t* second21, int n2,
                    float max_ratio, float max_distance, int cross_check, uint32_t* out_pairs,
                    int32_t* out_count, vc_stream_t stream) {
  if (n1 < 0 || n2 < 0 || !out_count) return VC_ERR_INVALID_ARG;
  if (n1 > 0 && (!idx12 || !best12 || !second12 || !out_pairs)) return VC_ERR_INVALID_ARG;
  if (cross_check && n1 > 0 && n2 > 0 && (!idx21 || !best21 || !second21)) return VC_ERR_INVALID_ARG;
  // (one workgroup of exactly kThreads: append_ordered counts kWaves waves)
  hipLaunchKernelGGL(mutual_ratio_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, idx12, best12,
                     second12, n1, idx21, best21, second21, n2, max_ratio, max_distance, cross_check,
                     out_pairs, out_count);
  return vc::check_launch();
}

int vc_theta_table(float* out, int n, vc_stream_t stream) { return launch_theta(out, n, 1, stream); }
int vc_theta_eval(float* out, int n, vc_stream_t stream) { return launch_theta(out, n, 0, stream); }

}  // extern "C"
