// bf16 linear layers with fused epilogues for the DINOv2 blocks (the model behind reference
// vit_colmap/features/vit_extractor.py:135-146):  out = epi(x W^T + b)  with
//   epi = identity (qkv), exact-erf GELU (fc1), "+ residual" (attn.proj / fc2 — the residual
//   stream update), or the SwiGLU gate of ViT-g (w12: silu(gate half) * value half, out half as wide),
//   so the activation and the residual add never make their own pass over HBM.
// x [M][K] bf16 (token rows), W [N][K] bf16 (torch Linear layout: one output feature per row), out [M][N] bf16.
//
// Four kernel families, in this order (each has its own comment):
//   1. gemm_kernel<EPI>           128 x 128 staged tile, any K % 64 == 0, N % 128 == 0 (vc_linear_bf16, vc_patch_embed_bf16);
//   2. gemm256_kernel<EPI, CONV>  256 x 256 persistent tile for the wide layers of ViT-B / L / g, also as an implicit-GEMM
//                                 convolution (vc_linear_bf16, vc_conv_taps_bf16);
//   -- shared section of the two K = 384 kernels: x-row load + LayerNorm, table GELU, the steps by which a 32 x 32 block
//      leaves through the wave's transposer, bias as initial value, the 24-MFMA stage loop, the fc1 weight fold; the same
//      load, store and residual steps for tensors kept in fragment order ("FM"), which need no transposer --
//   3. xs_kernel<EPI, LN, GT, XF, RF, OF>  x-stationary GEMM for K = 384: qkv, proj, fc1 of ViT-S (vc_linear_xs_bf16,
//                                 vc_linear_xs_bf16_l: x / residual / out in fragment order) + its prepare kernel;
//   4. mlp2_kernel<XF, OF>        the whole MLP of a 384-wide block in one kernel (vc_mlp_bf16, vc_mlp_bf16_l) + its prepare kernel.
// 3 and 4 take their LDS layout from one constexpr plan each (xs_lds, mlp_lds), which the host entry points read too.
// Vector types, bf16 pair conversions, the GELU forms, the XCD-aware tile order and the swizzled fragment offset of the two
// staged kernels come first; the host helpers and the C entry points are at the end.
//
// 1. gemm_kernel.  M is arbitrary (76 550 at 50 images x 1531 tokens), N % 128 == 0, K % 64 == 0.
// One workgroup = 4 waves = one 128 (tokens) x 128 (features) output tile; two workgroups per CU
// (64 KiB of LDS, <= 128 VGPRs each) so that one tile's epilogue VALU work runs under the other's
// MFMAs.  Per 64-deep K step both operand tiles (128 rows x 128 B) go global -> LDS by LDS-DMA
// (1 KiB per wave instruction, destination lane-linear), double buffered one step ahead; the bank
// swizzle (16-byte chunk ^ (row & 7), conflict-free for the ds_read_b128 column slices) is applied
// to the per-lane SOURCE address.  The product is computed transposed,
//   D^T[feature][token] = W_tile (A operand) x x_tile^T (B operand),  v_mfma_f32_16x16x32_bf16,
// so a lane ends up with 4 CONSECUTIVE FEATURES of one token: bias, GELU and residual are applied
// to 4-vectors and the bf16 result leaves as 8-byte stores.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vitcolmap_hip.h"
#include "common.h"
#include "device.h"

namespace {

typedef __bf16 v8bf __attribute__((ext_vector_type(8)));
typedef __bf16 v4bf __attribute__((ext_vector_type(4)));
typedef __bf16 v2bf __attribute__((ext_vector_type(2)));
typedef float v16f __attribute__((ext_vector_type(16)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef float v2f __attribute__((ext_vector_type(2)));
typedef uint32_t v4u __attribute__((ext_vector_type(4)));
typedef uint32_t v2u __attribute__((ext_vector_type(2)));

// Two floats -> one register of two bf16 (round to nearest even, lo in the low half) and back.
__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
  const v2bf p = {(__bf16)lo, (__bf16)hi};
  return *(const uint32_t*)&p;
}
__device__ __forceinline__ v2f unpack_bf16x2(uint32_t u) { return (v2f){__uint_as_float(u << 16), __uint_as_float(u & 0xffff0000u)}; }

constexpr int BM = 128;              // token rows per tile
constexpr int BN = 128;              // output features per tile
constexpr int BK = 64;               // K step: 64 bf16 = one 128-byte LDS row
constexpr int kImg = 128 * 128;      // bytes of one operand image (128 rows x 128 B)
constexpr int kStage = 2 * kImg;     // [x image | W image]

// EPI_PATCH is internal (vc_patch_embed_bf16); the others are the public VC_EPI_* codes of vc_linear_bf16.
enum { EPI_BIAS = 0, EPI_GELU = 1, EPI_RESIDUAL = 2, EPI_PATCH = 3, EPI_SWIGLU = 4 };
static_assert(EPI_BIAS == VC_EPI_BIAS && EPI_GELU == VC_EPI_GELU && EPI_RESIDUAL == VC_EPI_RESIDUAL && EPI_SWIGLU == VC_EPI_SWIGLU,
              "epilogue codes of the ABI");

// exact GELU, 0.5 x (1 + erf(x / sqrt 2)), erf by Abramowitz-Stegun 7.1.26 (|error| <= 1.5e-7):
// with q = (1 - erf|z|) = poly(t) t exp(-z^2), t = 1 / (1 + p|z|):  gelu = max(x, 0) - 0.5 |x| q.
__device__ __forceinline__ float gelu_erf(float x) {
  const float ax = __builtin_fabsf(x);
  const float t = __builtin_amdgcn_rcpf(__builtin_fmaf(ax, 0.3275911f * 0.70710678118654752f, 1.0f));
  float p = __builtin_fmaf(t, 1.061405429f, -1.453152027f);
  p = __builtin_fmaf(p, t, 1.421413741f);
  p = __builtin_fmaf(p, t, -0.284496736f);
  p = __builtin_fmaf(p, t, 0.254829592f);
  const float zl = x * 0.84932180028801907f;   // x sqrt(log2(e) / 2):  exp(-x^2/2) = exp2(-zl^2)
  const float e = __builtin_amdgcn_exp2f(-(zl * zl));
  const float q = p * t * e;
  return __builtin_fmaf(-0.5f * ax, q, __builtin_fmaxf(x, 0.0f));
}

// The same on a pair of values with 2-wide packed float32 operations (v_pk_fma_f32 / v_pk_mul_f32):
// beside a partner wave that owns the matrix pipe, a lone wave's VALU stream is issue-bound, and a packed
// instruction does twice the work per issue slot.  Only rcp / exp2 / abs / max stay one value at a time.
__device__ __forceinline__ v2f gelu_erf2(v2f x) {
  const v2f ax = {__builtin_fabsf(x[0]), __builtin_fabsf(x[1])};
  const v2f one = {1.0f, 1.0f};
  const v2f den = __builtin_elementwise_fma(ax, (v2f){0.3275911f * 0.70710678118654752f, 0.3275911f * 0.70710678118654752f}, one);
  const v2f t = {__builtin_amdgcn_rcpf(den[0]), __builtin_amdgcn_rcpf(den[1])};
  v2f p = __builtin_elementwise_fma(t, (v2f){1.061405429f, 1.061405429f}, (v2f){-1.453152027f, -1.453152027f});
  p = __builtin_elementwise_fma(p, t, (v2f){1.421413741f, 1.421413741f});
  p = __builtin_elementwise_fma(p, t, (v2f){-0.284496736f, -0.284496736f});
  p = __builtin_elementwise_fma(p, t, (v2f){0.254829592f, 0.254829592f});
  const v2f zl = x * (v2f){0.84932180028801907f, 0.84932180028801907f};
  const v2f z2 = zl * zl;
  const v2f e = {__builtin_amdgcn_exp2f(-z2[0]), __builtin_amdgcn_exp2f(-z2[1])};
  const v2f q = p * t * e;
  const v2f pos = {__builtin_fmaxf(x[0], 0.0f), __builtin_fmaxf(x[1], 0.0f)};
  return __builtin_elementwise_fma(ax * (v2f){-0.5f, -0.5f}, q, pos);
}

// EPI_SWIGLU: silu(a) b = a b / (1 + exp(-a)) on the two float32 pre-activations.  exp(-a) overflows to +inf below
// a ~ -88.7 and v_rcp_f32(+inf) = 0: the gate saturates to (-)0 there and to a itself above, never to NaN.
__device__ __forceinline__ float swiglu_f32(float a, float b) {
  const float e = __builtin_amdgcn_exp2f(a * -1.4426950408889634f);
  return a * __builtin_amdgcn_rcpf(1.0f + e) * b;
}

// Fragment addressing of the two staged kernels in an image of 128-byte rows (64 k): for k-substep ks a lane reads row
// row0 + (l & 15) of a 16-row block, 16-byte chunk 4 ks + (l >> 4), stored at chunk ^ (row & 7).  row0 % 8 == 0, so the rows
// of all 16-row blocks below it share the swizzle: one offset per k-substep, the blocks are 2048 bytes apart.
__device__ __forceinline__ uint32_t frag_off(int row0, int lane, int ks) {
  const int fr = lane & 15, ch = ks * 4 + (lane >> 4);
  return (uint32_t)(row0 + fr) * 128u + (uint32_t)((ch ^ (fr & 7)) << 4);
}

// EPI_SWIGLU (both tile forms): N is the width of the PRODUCT (2 H, DINOv2's w12: rows [0, H) of W make the gate, rows
// [H, 2H) the value) and `out` is [M][H].  A tile's W operand comes from two row ranges — the first half of every wave's
// feature rows from the gate rows of the tile's output columns, the second half from the matching value rows — so a lane's
// accumulators [a] and [a + half] are the gate and the value of the SAME output elements: the tile loop, the staging ring and
// the accumulation order over K are those of the other epilogues, only the W source rows and the store side differ.
template <int EPI>
__global__ __launch_bounds__(256, 2) void gemm_kernel(const __bf16* __restrict__ X, const __bf16* __restrict__ W,
                                                      const __bf16* __restrict__ bias,
                                                      const __bf16* __restrict__ res, __bf16* __restrict__ out,
                                                      int M, int N, int K, int n_tiles_n, int n_tiles,
                                                      int group) {
  // EPI_PATCH: row m = (image b, token t) with b = m / group; the result goes to row m + b + 1 of `out`
  // (one class-token row per image is skipped) and `res` is the position embedding, indexed by 1 + t.
  __shared__ __attribute__((aligned(1024))) uint8_t lds[2][kStage];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave & 1, wn = wave >> 1;

  // XCD-aware tile order of the two staged kernels (vc::xcd_tile), feature tiles fastest: the tiles an XCD works on at one
  // time share x rows in its L2
  const int tile = vc::xcd_tile(blockIdx.x, n_tiles);
  const int tm = tile / n_tiles_n, tn = tile - tm * n_tiles_n;
  const int m0 = tm * BM, n0 = tn * BN;
  // EPI_SWIGLU: the tile makes output columns j0 .. j0 + 63; W image rows [64 wn, 64 wn + 32) are gate rows
  // j0 + 32 wn .. + 31, rows [64 wn + 32, 64 wn + 64) the value rows H + the same
  const int H = N >> 1, j0 = tn * (BN / 2);

  // ---- LDS-DMA staging: a stage is 32 pieces of 1 KiB (8 rows x 128 B); wave w issues x pieces
  // 4w..4w+3 and W pieces 4w..4w+3.  Lane l fills LDS row (l >> 3), chunk (l & 7) of its piece with
  // source chunk (l & 7) ^ (l >> 3)  [row & 7 == l >> 3 because pieces start at multiples of 8 rows].
  const uint32_t lds0 = vc::lds_addr(&lds[0][0]);
  const int prow = lane >> 3, pchunk = (lane & 7) ^ prow;
  const __bf16* xsrc[4];
  const __bf16* wsrc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = (wave * 4 + i) * 8 + prow;
    xsrc[i] = X + (size_t)min(m0 + row, M - 1) * K + pchunk * 8;
    const int wrow = EPI == EPI_SWIGLU ? ((row & 32) ? H : 0) + j0 + (row >> 6) * 32 + (row & 31) : n0 + row;
    wsrc[i] = W + (size_t)wrow * K + pchunk * 8;
  }
  auto issue = [&](int kt, int buf) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const __bf16* src = (i < 4 ? xsrc[i] : wsrc[i - 4]) + kt * BK;
      const uint32_t dst = lds0 + (uint32_t)buf * kStage + (uint32_t)(i >> 2) * kImg + (uint32_t)(wave * 4 + (i & 3)) * 1024u;
      vc::lds_dma16(src, dst);
    }
  };

  v4f acc[4][4];   // [feature block][token block]
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = (v4f){0.f, 0.f, 0.f, 0.f};

  const int fr = lane & 15, fq = lane >> 4;
  uint32_t xoff[2], woff[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    xoff[ks] = frag_off(wm * 64, lane, ks);
    woff[ks] = (uint32_t)kImg + frag_off(wn * 64, lane, ks);
  }

  const int nk = K / BK;
  issue(0, 0);
  for (int kt = 0; kt < nk; ++kt) {
    // this wave's pieces of step kt have landed; after the barrier everyone's have, and everyone
    // has finished reading the other buffer (step kt-1)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    if (kt + 1 < nk) issue(kt + 1, (kt + 1) & 1);
    const uint8_t* st = lds[kt & 1];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      v8bf wf[4], xf[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) wf[a] = *(const v8bf*)(st + woff[ks] + a * (16 * 128));
#pragma unroll
      for (int b = 0; b < 4; ++b) xf[b] = *(const v8bf*)(st + xoff[ks] + b * (16 * 128));
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
          acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[a], xf[b], acc[a][b], 0, 0, 0);
    }
  }

  // ---- epilogue: lane (token = l & 15 of block b, features 4 (l >> 4) .. +3 of block a) -------------
  if (EPI == EPI_SWIGLU) {
    // blocks a = 0, 1 hold the gate and a + 2 the value of output columns j0 + 32 wn + 16 a + 4 fq .. + 3
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const int n = j0 + wn * 32 + a * 16 + fq * 4;
      const v4bf bg = *(const v4bf*)(bias + n), bv = *(const v4bf*)(bias + H + n);
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int m = m0 + wm * 64 + b * 16 + fr;
        if (m < M) {
          v4bf ov;
#pragma unroll
          for (int j = 0; j < 4; ++j)
            ov[j] = (__bf16)swiglu_f32(acc[a][b][j] + (float)bg[j], acc[a + 2][b][j] + (float)bv[j]);
          *(v4bf*)(out + (size_t)m * H + n) = ov;
        }
      }
    }
    return;
  }
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int n = n0 + wn * 64 + a * 16 + fq * 4;
    const v4bf bv = *(const v4bf*)(bias + n);
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int m = m0 + wm * 64 + b * 16 + fr;
      if (m < M) {
        size_t o = (size_t)m * N + n;
        size_t ro = o;
        if (EPI == EPI_PATCH) {
          const int b_img = m / group;
          o = (size_t)(m + b_img + 1) * N + n;
          ro = (size_t)(m - b_img * group + 1) * N + n;
        }
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = acc[a][b][j] + (float)bv[j];
        if (EPI == EPI_GELU) {
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = gelu_erf(v[j]);
        }
        if (EPI == EPI_RESIDUAL || EPI == EPI_PATCH) {
          const v4bf rv = *(const v4bf*)(res + ro);
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] += (float)rv[j];
        }
        v4bf ov;
#pragma unroll
        for (int j = 0; j < 4; ++j) ov[j] = (__bf16)v[j];
        *(v4bf*)(out + o) = ov;
      }
    }
  }
}


// =====================================================================================================
// 256 x 256 tile for the wide layers (ViT-B / ViT-L: n_out % 256 == 0).  The 128 x 128 kernel above moves (128 + 128) x 64 x 2
// bytes through L2 -> LDS per 128 x 128 x 64 MACs, two workgroups per CU do so independently, and every K step ends in a
// vmcnt(0) + barrier: measured bound by that at ~28 % of the matrix peak (the library reaches 35-50 % on the
// ViT-B shapes).  This kernel follows the guide's 256^2 eight-phase structure (cdna_hip_programming.md §5):
//   * ONE workgroup of 8 waves per CU owns a 256 x 256 tile: waves 2 (token halves, `wr`) x 4 (feature quarters, `wc`); per
//     wave D^T[64 features][128 tokens] = 4 x 8 accumulator tiles of v_mfma_f32_16x16x32_bf16 (128 VGPRs);
//   * a 64-deep K tile is computed in FOUR PHASES, one 32-feature x 64-token quadrant (16 MFMAs) each, in the order
//     (f0,t0) (f1,t0) (f1,t1) (f0,t1): a phase re-reads from LDS only the operand half that changes (W half: 4 ds_read_b128,
//     x half: 8), the W0 fragments stay in registers for the fourth;
//   * the two waves of a SIMD (w and w + 4) run half a phase apart: between two barriers one of them is in its MFMA cluster,
//     the other in its memory cluster (fragment reads + its LDS-DMA pieces) — the matrix pipe always has a wave that does
//     nothing but feed it (two barriers per phase, waves 4-7 one barrier late);
//   * staging is cut into UNITS of 16 KiB = the rows one phase starts to need: X0 (token rows [0,64) of both wave rows), W0
//     (feature rows [0,32) of all four wave columns), W1, X1, in that order, one unit (2 pieces of 1 KiB per wave) issued
//     per phase, SIX units ahead, into 2 buffers x 4 units = 128 KiB; one counted wait per K tile (vmcnt(4): two units
//     stay in flight across the barriers) in the fourth phase retires the next K tile.  Hazards, with the half-phase lag
//     counted in: a unit is first read two barriers after every wave's wait for it, and restaged at least TWO phases after
//     its last fragment read was issued (X0: read in phase 0, restaged in phase 2; W0 0 / 3; W1 1 / 0 of the next K tile;
//     X1 2 / 1), so the lgkmcnt(0) for a phase's reads can sit behind the barrier, at the head of the MFMA cluster, where
//     the read latency overlaps the partner's last MFMAs instead of lengthening the memory cluster.
constexpr int G2M = 256, G2N = 256;
constexpr int kUnit2 = 128 * 128;         // 16 KiB: 128 rows x 64 k
constexpr int kBuf2 = 4 * kUnit2;         // X0 | W0 | W1 | X1
constexpr int G256_LDS = 2 * kBuf2;       // 128 KiB
constexpr int kAhead2 = 6;                // units issued ahead of the phase that runs

// CONV: the same kernel as an implicit GEMM over a channels-last image batch x [batch][cH][cW][cC] (+ one trailing row of cC
// zeros, row M): output row m = (b, y, x) gathers kh x ckw taps, K = taps * cC, k = (tap, channel); tap t reads the row of
// pixel (y + cdy0 + t / ckw, x + cdx0 + t % ckw) of the same image, or the zero row when that pixel is outside it.  A K tile
// (64 channels of one tap) is the same 1 KiB pieces as before — the tap only moves the scalar base, and a lane whose pixel
// is outside points at the zero row instead (one v_cndmask per piece).  W [N][K] with k in the same (tap, channel) order.
// cpar >= 0: the result is one parity class of a stride-2 transposed convolution — row (b, y, x) goes to pixel
// (2y + (cpar >> 1), 2x + (cpar & 1)) of a [batch][2 cH][2 cW][N] output (the four classes interleave there, no copy).
template <int EPI, bool CONV>
__global__ __launch_bounds__(512, 2) void gemm256_kernel(const __bf16* __restrict__ X, const __bf16* __restrict__ W,
                                                         const __bf16* __restrict__ bias, const __bf16* __restrict__ res,
                                                         __bf16* __restrict__ out, int M, int N, int K, int n_tiles_n,
                                                         int n_tiles, int cH, int cW, int cC, int ckw, int cdy0, int cdx0,
                                                         int cpar) {
  extern __shared__ __attribute__((aligned(1024))) uint8_t lds2[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 2, wc = wave & 3;
  const int nk = K / BK;
  const int n_units = 4 * nk;
  // Persistent workgroups (one per CU) walk the tile list.  (Measured and dropped: starting them up to one tile-time apart so
  // that epilogues do not coincide — the output writes are not a shared-HBM burst problem; every start delay came back as
  // added time, 1268 -> 1344 us per ViT-B layer.)
  for (int slot = blockIdx.x; slot < n_tiles; slot += gridDim.x) {
  const int tile = vc::xcd_tile(slot, n_tiles);
  const int tm = tile / n_tiles_n, tn = tile - tm * n_tiles_n;
  const int m0 = tm * G2M, n0 = tn * G2N;

  // ---- staging: unit u = 4 t + j of K tile t; j = 0: X0, 1: W0, 2: W1, 3: X1.  Wave w issues pieces 2w, 2w+1 (8 unit rows each).
  // unit row rho -> tile row:  X_h: rho < 64 ? rho + 64 h : 128 + (rho - 64) + 64 h;   W_h: (rho >> 5) * 64 + 32 h + (rho & 31)
  const uint32_t lds0 = vc::lds_addr(&lds2[0]);
  const int prow = lane >> 3, pchunk = (lane & 7) ^ prow;
  uint32_t voffx[2][2], voffw[2];          // per-lane byte offsets from X / W (+ k offset of the K tile added as a scalar)
  uint32_t vtaps[2][2];                    // CONV: bit t set = tap t of this lane's pixel lies inside the image
  const int n_taps = CONV ? K / cC : 1, tiles_per_tap = CONV ? cC / BK : 1;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int rho = (wave * 2 + i) * 8 + prow;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int xr = (rho < 64 ? rho : 128 + (rho - 64)) + 64 * h;
      if (CONV) {
        const int m = m0 + xr, hw = cH * cW;
        const int bimg = m / hw, rem = m - bimg * hw, py = rem / cW, px = rem - py * cW;
        uint32_t bits = 0;
        for (int t = 0; t < n_taps; ++t) {
          const int yy = py + cdy0 + t / ckw, xx = px + cdx0 + t % ckw;
          if (m < M && yy >= 0 && yy < cH && xx >= 0 && xx < cW) bits |= 1u << t;
        }
        vtaps[h][i] = bits;
        voffx[h][i] = (uint32_t)(((size_t)min(m, M - 1) * cC + pchunk * 8) * 2);
      } else {
        voffx[h][i] = (uint32_t)(((size_t)min(m0 + xr, M - 1) * K + pchunk * 8) * 2 - (size_t)min(m0, M - 1) * K * 2);
      }
    }
    // EPI_SWIGLU: unit W0 is gate rows j0 .. j0 + 127 of W (wave column wc takes 32 wc .. + 31), unit W1 the value rows H + the same
    const int wrow = EPI == EPI_SWIGLU ? rho : (rho >> 5) * 64 + (rho & 31);
    voffw[i] = (uint32_t)(((size_t)wrow * K + pchunk * 8) * 2);
  }
  const int H = N >> 1, j0 = tn * (G2N / 2);   // EPI_SWIGLU: width of `out`, first output column of the tile
  const char* const xbase = CONV ? (const char*)X : (const char*)(X + (size_t)min(m0, M - 1) * K);
  const char* const wbase = (const char*)(W + (size_t)(EPI == EPI_SWIGLU ? j0 : n0) * K);
  const size_t whalf = (size_t)(EPI == EPI_SWIGLU ? H : 32) * K * 2;
  auto issue = [&](int u) {
    if (u >= n_units) return;
    const int t = u >> 2, j = u & 3;
    const bool is_x = j == 0 || j == 3;
    const char* sb = is_x ? xbase + (size_t)t * (BK * 2) : wbase + (size_t)t * (BK * 2) + (j == 2 ? whalf : 0);
    int tap = 0;
    uint32_t zoff = 0, spos = 0;           // CONV: offset (from sb) of this lane's 16 bytes in the zero row; forward part of the tap shift
    if (CONV && is_x) {
      tap = t / tiles_per_tap;
      const long long shift = ((long long)(cdy0 + tap / ckw) * cW + (cdx0 + tap % ckw)) * cC * 2;   // bytes, may be negative
      // a backward shift moves the scalar base (the per-lane offsets are unsigned), a forward one is added per lane: the
      // zero row (behind the batch) stays reachable from the base however small the batch is
      const long long sneg = shift < 0 ? shift : 0;
      spos = (uint32_t)(shift - sneg);
      sb = xbase + sneg + (long long)(t - tap * tiles_per_tap) * (BK * 2);
      zoff = (uint32_t)((long long)M * cC * 2 - sneg) + (uint32_t)pchunk * 16u;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      uint32_t vo = j == 0 ? voffx[0][i] : (j == 3 ? voffx[1][i] : voffw[i]);
      if (CONV && is_x) vo = ((j == 0 ? vtaps[0][i] : vtaps[1][i]) >> tap) & 1u ? vo + spos : zoff;
      const uint32_t dst = lds0 + (uint32_t)(t & 1) * kBuf2 + (uint32_t)j * kUnit2 + (uint32_t)(wave * 2 + i) * 1024u;
      vc::lds_dma16(sb, vo, dst);
    }
  };

  v4f acc[4][8];   // [feature block of 16][token block of 16]
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 8; ++b) acc[a][b] = (v4f){0.f, 0.f, 0.f, 0.f};

  // fragment addressing inside a unit (frag_off)
  const int fr = lane & 15, fq = lane >> 4;
  uint32_t xoff[2], woff[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    xoff[ks] = frag_off(wr * 64, lane, ks);
    woff[ks] = frag_off(wc * 32, lane, ks);
  }
  v8bf xf[2][4], wf[2][2][2];   // x fragments of the current token half [ks][block]; W fragments [feature half][ks][block]

  auto read_x = [&](const uint8_t* buf, int th) {
    const uint8_t* u = buf + (th == 0 ? 0 : 3) * kUnit2;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int b = 0; b < 4; ++b) xf[ks][b] = *(const v8bf*)(u + xoff[ks] + b * 2048);
  };
  auto read_w = [&](const uint8_t* buf, int fh) {
    const uint8_t* u = buf + (1 + fh) * kUnit2;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int a = 0; a < 2; ++a) wf[fh][ks][a] = *(const v8bf*)(u + woff[ks] + a * 2048);
  };
  auto barrier = []() { asm volatile("s_barrier" ::: "memory"); };
#define G2_MFMA(FH, TH)                                                                                      \
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                         \
  __builtin_amdgcn_sched_barrier(0);                                                                         \
  __builtin_amdgcn_s_setprio(1);                                                                             \
  _Pragma("unroll") for (int ks = 0; ks < 2; ++ks)                                                           \
  _Pragma("unroll") for (int a = 0; a < 2; ++a)                                                              \
  _Pragma("unroll") for (int b = 0; b < 4; ++b)                                                              \
    acc[2 * (FH) + a][4 * (TH) + b] =                                                                        \
        __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[FH][ks][a], xf[ks][b], acc[2 * (FH) + a][4 * (TH) + b], 0, 0, 0); \
  __builtin_amdgcn_s_setprio(0);

  // ---- prologue: K tile 0 and three units of K tile 1 in flight, K tile 0 landed -----------------------------------
#pragma unroll
  for (int u = 0; u < kAhead2; ++u) issue(u);
  if (nk > 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  barrier();
  if (wr == 1) barrier();   // waves 4-7 run one barrier (half a phase) behind their SIMD partners

  for (int t = 0; t < nk; ++t) {
    const uint8_t* buf = lds2 + (size_t)(t & 1) * kBuf2;
    const int g = 4 * t;
    // phase 0: quadrant (f0, t0)
    read_w(buf, 0);
    __builtin_amdgcn_sched_barrier(0);
    read_x(buf, 0);
    issue(g + kAhead2);
    barrier();
    G2_MFMA(0, 0)
    barrier();
    // phase 1: quadrant (f1, t0)
    read_w(buf, 1);
    issue(g + 1 + kAhead2);
    barrier();
    G2_MFMA(1, 0)
    barrier();
    // phase 2: quadrant (f1, t1)
    read_x(buf, 1);
    issue(g + 2 + kAhead2);
    barrier();
    G2_MFMA(1, 1)
    barrier();
    // phase 3: quadrant (f0, t1); the one wait of the K tile: everything but the two youngest units has landed, i.e. all of
    // K tile t + 1 (its first reads come two barriers later, behind every wave's wait)
    issue(g + 3 + kAhead2);
    if (t + 2 < nk) asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    barrier();
    G2_MFMA(0, 1)
    barrier();
  }
  if (wr == 0) barrier();   // (same number of barriers in both halves)
#undef G2_MFMA

  // ---- epilogue ------------------------------------------------------------------------------------------------------------
  // A lane holds, per (feature block a, token block b), 4 consecutive features of token 16 b + fr: 8 bytes of an output row.
  // Stored from that layout, a store instruction touches 16 to 64 rows with 8 to 16 bytes each, and the epilogue cost 40-65 %
  // of a K = 768 tile's main loop (stores are bound by the lines they touch: same bytes in contiguous KiB ran 100 us per
  // ViT-B layer faster).  Every wave therefore turns its 128 x 64 block through its own 16 KiB of the (now idle) staging
  // buffers — all fragment reads of the tile are behind the last barrier: 8-byte writes from the accumulator layout, 16-byte
  // reads of [8 rows][128 B] per instruction, so each store instruction writes 8 whole 128-byte lines.  The residual takes the
  // same way in: whole-line loads, 16-byte LDS writes, and each lane picks up its own 8 bytes in the accumulator layout, adds
  // in float32 and overwrites them with the rounded result (nothing is rounded before the residual add).  16-byte slots are
  // XORed with (row >> 1) & 7: the 16-byte reads are conflict-free in the hardware's lane groups ({0-3, 12-15, 20-27}, ...:
  // 16 distinct slots of the 256-byte bank row each); the 8-byte writes keep a 2-way conflict (rows 2k and 2k + 1 of a
  // 16-lane group share a slot), which a ds_write_b64's own issue time nearly covers.
  uint8_t* const ep = lds2 + (size_t)wave * 16384;
  const int lrow = lane >> 3, lslot = lane & 7;          // whole-line view: row 8 i + lrow, 16-byte slot lslot
  auto ep_at = [&](int row, int byte) { return ep + row * 128 + (byte ^ (((row >> 1) & 7) << 4)); };
  if (EPI == EPI_SWIGLU) {
    // The wave's block is 128 tokens x 32 output columns: feature blocks a = 0, 1 are the gate, a + 2 the value of columns
    // j0 + 32 wc + 16 a + 4 fq .. + 3, and a row of the block is 64 bytes, half a line.  Two consecutive token rows share one
    // 128-byte row of the transposer (row r -> transposer row r >> 1, bytes 64 (r & 1) ..), which keeps the slot swizzle and
    // both access patterns of the full-width epilogue: 8-byte writes from the accumulator layout (the same 2-way conflict),
    // conflict-free 16-byte reads of 8 transposer rows per instruction — now 16 token rows x 64 contiguous bytes per store
    // instruction, lane -> (row 16 i + (l >> 2), 16-byte slot l & 3).  The wave columns 2c and 2c + 1 complete each other's lines.
    const size_t colh = (size_t)j0 + wc * 32;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const v4bf bg = *(const v4bf*)(bias + colh + a * 16 + fq * 4), bv = *(const v4bf*)(bias + H + colh + a * 16 + fq * 4);
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        const int row = 16 * b + fr;
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = swiglu_f32(acc[a][b][j] + (float)bg[j], acc[a + 2][b][j] + (float)bv[j]);
        *(v2u*)ep_at(row >> 1, 64 * (row & 1) + 32 * a + 8 * fq) = (v2u){pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int m = m0 + wr * 128 + 16 * i + (lane >> 2);
      const v4u o = *(const v4u*)ep_at(8 * i + lrow, lslot * 16);
      if (m < M) *(v4u*)(out + (size_t)m * H + colh + (lane & 3) * 8) = o;
    }
    asm volatile("s_barrier" ::: "memory");   // as below: the next tile's copies land in this buffer
    continue;
  }
  const size_t col0 = (size_t)n0 + wc * 64;
  if (EPI == EPI_RESIDUAL) {
    v4u rr[16];
#pragma unroll
    for (int i = 0; i < 16; ++i)
      rr[i] = *(const v4u*)(res + (size_t)min(m0 + wr * 128 + 8 * i + lrow, M - 1) * N + col0 + lslot * 8);
#pragma unroll
    for (int i = 0; i < 16; ++i) *(v4u*)ep_at(8 * i + lrow, lslot * 16) = rr[i];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const v4bf bv = *(const v4bf*)(bias + col0 + a * 16 + fq * 4);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      uint8_t* const pp = ep_at(16 * b + fr, 32 * a + 8 * fq);
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = acc[a][b][j] + (float)bv[j];
      if (EPI == EPI_GELU) {
#pragma unroll
        for (int j = 0; j < 4; j += 2) {
          const v2f g = gelu_erf2((v2f){v[j], v[j + 1]});
          v[j] = g[0];
          v[j + 1] = g[1];
        }
      }
      if (EPI == EPI_RESIDUAL) {
        const v2u r8 = *(const v2u*)pp;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const v2f rf = unpack_bf16x2(r8[j]);
          v[2 * j] += rf[0];
          v[2 * j + 1] += rf[1];
        }
      }
      *(v2u*)pp = (v2u){pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  if (CONV && cpar >= 0) {
    // a lane's 16 rows are 8 pixels apart: one division for the first, then carries
    int mm = m0 + wr * 128 + lrow;
    int pb = mm / (cH * cW), py = (mm - pb * cH * cW) / cW, px = mm - pb * cH * cW - py * cW;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = 8 * i + lrow;
      const v4u o = *(const v4u*)ep_at(row, lslot * 16);
      const size_t orow = ((size_t)pb * 2 * cH + 2 * py + (cpar >> 1)) * (2 * cW) + 2 * px + (cpar & 1);
      if (mm < M) *(v4u*)(out + orow * N + col0 + lslot * 8) = o;
      mm += 8;
      px += 8;
      while (px >= cW) { px -= cW; if (++py == cH) { py = 0; ++pb; } }
    }
  } else {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = 8 * i + lrow, m = m0 + wr * 128 + row;
      const v4u o = *(const v4u*)ep_at(row, lslot * 16);
      if (m < M) *(v4u*)(out + (size_t)m * N + col0 + lslot * 8) = o;
    }
  }
  asm volatile("s_barrier" ::: "memory");   // every wave is past its last fragment read of this tile before the next tile's copies land
  }  // tiles of this workgroup
}

// =====================================================================================================
// x-stationary kernel for K = 384 (every Linear of ViT-S that reads the 384-wide residual stream or the
// attention output: qkv, proj, fc1).  The staged kernel above moves (128 + 128) x K bytes through
// L2 -> LDS per 128 x 128 tile and is bound by that traffic (measured ~10 TB/s aggregate at 30 % MFMA
// utilisation).  Here a wave keeps ITS 32 token rows resident in registers as MFMA B fragments for the
// whole launch (24 k-steps x 4 VGPRs = 96 VGPRs) and only W streams, once per 256-row workgroup:
//   * W is pre-tiled on the host into fragment order (vc_linear_xs_prepare): piece (nb, ks) is the 1 KiB
//     A operand of v_mfma_f32_32x32x16_bf16 for features 32 nb .. +32, k 16 ks .. +16, so a stage
//     (one 32-feature block, 24 pieces) is 24 perfectly coalesced LDS-DMA instructions and a fragment
//     read is ds_read_b128 at lane x 16 (conflict free, no swizzle);
//   * 8 waves x 32 rows = 256 token rows per workgroup, one persistent workgroup per CU; the
//     (row tile, feature block) stages are split evenly over the grid in row-tile-major order, so a
//     workgroup reloads its x rows at most a few times and the grid finishes together (no tile-count
//     quantisation: 14 400 stages over 256 CUs at fc1);
//   * ring of 3 stages (72 KiB), filled 2 stages ahead, one barrier per stage (24 MFMAs per wave);
//   * all 8 waves run the same stream: the epilogue of block i-1 (exact GELU, residual, bf16 pack,
//     transpose, store) is cut into slices issued between the 24 MFMAs of block i (see the epilogue
//     comment for why the alternative — partner waves in anti-phase — serialises on this hardware);
//   * LayerNorm is fused into the x load: a lane and its partner (l ^ 32) hold one whole row, the
//     statistics are two-pass float32 in registers, gamma is folded into W and beta into the bias by
//     the prepare step, so the normalised activations never exist in memory; the bias is the
//     accumulator's initial value;
//   * D^T orientation (features on registers, token on the lane); v_permlane32_swap + a wave-private
//     LDS transposer turn a block into 16 rows x 64 contiguous bytes per store instruction.
// Measured (76 550 rows, 1x MI355X): qkv+LN 100 us, proj+residual 46 us, fc1+LN+GELU 156 us; ablation
// builds: MFMA + ring alone 64 / 32 / 80 us, the x reloads ~10 us, stores ~10-20 us.
constexpr int XK = 384;
constexpr int XKS = XK / 16;                 // 24 k-steps of v_mfma_f32_32x32x16_bf16
constexpr int XStage = XKS * 1024;           // 24 KiB: one 32-feature block of W in fragment order
constexpr int XNS = 3;                       // ring slots
constexpr int XPF = XNS - 1;                 // stages in flight
constexpr int XRows = 256;                   // token rows per workgroup (8 waves x 32)
constexpr int XChunk = 32 * 128;             // x staging: 32 rows x 64 k (128-byte rows), per wave, double buffered

// GELU by table (EPI_GELU with a table pointer).  float32 VALU work does not overlap with the matrix pipe on
// this part, integer VALU work and LDS reads do (tools/overlap_probe.hip), and the exact GELU is ~150 float
// instructions per block and wave.  The standard bf16 pipeline evaluates gelu on the bf16-ROUNDED pre-activation
// and rounds the result to bf16, i.e. it is a function from 16 bits to 16 bits: for 2^-14 <= |x| < 8 it is looked
// up in LDS (17 exponents x 128 mantissas x 2 signs = 4352 entries of 2 bytes, entry [k][sign] with
// k = (bits & 0x7fff) - kGtLo), the index arithmetic is integer work.  A wave that holds a value outside that
// range (|x| >= 8, |x| < 2^-14, NaN) takes the float path for the block (rare).  Table values: 0.5 x (1 + erff(x / sqrt 2))
// in float32, rounded to nearest-even — what torch's bf16 gelu computes.
constexpr uint32_t kGtLo = (127 - 14) << 7;                 // bf16 bits of 2^-14
constexpr uint32_t kGtN = 17 * 128;                         // magnitudes covered: [2^-14, 8)
constexpr int kGtBytes = (int)kGtN * 2 * 2;                 // 8704

__device__ __forceinline__ uint32_t f32_to_bf16_rne(float v) {
  uint32_t u = __float_as_uint(v);
  u += 0x7fffu + ((u >> 16) & 1u);
  return u >> 16;
}
__global__ void gelu_table_kernel(uint16_t* __restrict__ tab) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= kGtN * 2) return;
  const uint32_t k = i >> 1, sign = i & 1;
  const float x = __uint_as_float(((sign << 15) | (kGtLo + k)) << 16);
  const float y = 0.5f * x * (1.0f + erff(x * 0.70710678118654752f));
  tab[i] = (uint16_t)f32_to_bf16_rne(y);
}

// =====================================================================================================
// What xs_kernel and mlp2_kernel (below) share.  Everything is __forceinline__ and takes its register arrays by
// reference; the step index `sl` / `ks` of a sliced function is a constant after unrolling, so a call leaves only the
// instructions of that step.
//
// ---- LDS plans: one constexpr function per kernel, read by the kernel for its pointers and by the host for its limits.
constexpr int kCuLds = 160 * 1024;                 // LDS of a CU
constexpr int MStage = 2 * XStage;                 // fused MLP, 48 KiB: [W1 chunk | W2 chunk]
constexpr int MNS = 2;                             // ... its ring slots

// xs_kernel: [ring of XNS stages][bias area: float32 bias of the N features, behind it (GT) the GELU table]
//            [per wave 8 KiB: the x transposer, later the out (+0) and residual (+2048) transposers of the epilogue]
// Second form (x in fragment order, below): no x transposer; 4 KiB per wave where a row-major residual or output still
// takes the epilogue's transposers, nothing where both are in fragment order.
struct XsLds {
  uint32_t ring, bias, bias_bytes, tr, end;
  __host__ __device__ constexpr bool bias_fits(int n_out) const { return (uint32_t)n_out * 4 <= bias_bytes; }
  __host__ __device__ constexpr uint32_t table(int n_out) const { return bias + (uint32_t)((n_out * 4 + 15) & ~15); }
  __host__ __device__ constexpr bool table_fits(int n_out) const { return table(n_out) + kGtBytes <= bias + bias_bytes; }
};
__host__ __device__ constexpr XsLds xs_lds(bool x_fm = false, bool epi_row_major = true) {
  vc::LdsCursor c{0};
  XsLds l{};
  l.ring = c.take(XNS * XStage, 1024);
  l.bias_bytes = 16 * 1024;
  l.bias = c.take(l.bias_bytes, 16);
  l.tr = c.take(!x_fm ? 8 * 2 * XChunk : epi_row_major ? 8 * XChunk : 0, 16);
  l.end = c.at;
  return l;
}
static_assert(xs_lds().end == 152 * 1024, "xs_kernel: 72 + 16 + 64 KiB");
static_assert(xs_lds(true, true).end == 120 * 1024 && xs_lds(true, false).end == 88 * 1024,
              "xs_kernel, x in fragment order: 72 + 16 + 32 KiB with a row-major residual or output, 72 + 16 KiB without");
static_assert(xs_lds().ring % 1024 == 0 && XStage % 1024 == 0, "xs_kernel: every LDS-DMA piece lands on a 1 KiB boundary");
static_assert(xs_lds().bias % 16 == 0 && xs_lds().tr % 16 == 0 && XChunk % 16 == 0, "xs_kernel: table and transposers take 16-byte accesses");
static_assert(xs_lds().table_fits(1920) && !xs_lds().table_fits(1952) && xs_lds().table_fits(1536) && xs_lds().bias_fits(4096),
              "xs_kernel: ViT-S's fc1 has its table; bias and table share the area up to 1920 features, the bias alone fills it at 4096");

// mlp2_kernel: [ring of MNS stages][fc1 bias][GELU table][fc2 bias][x transposers of the A waves, 4 x 4 KiB]
//              [out (+0) / residual (+2048) transposers of the B waves, 4 x 4 KiB][activation hand-off: 2 parities x 4 pairs x 2 KiB]
// The fc1 bias gets what the fixed regions leave of the CU's LDS: that is the limit on the hidden width.
struct MlpLds {
  uint32_t ring, b1, b1_bytes, gt, b2, tr_a, tr_b, hand, end;
  __host__ __device__ constexpr int max_hidden() const { return (int)(b1_bytes / 4 / 32 * 32); }
};
__host__ __device__ constexpr MlpLds mlp_lds() {
  constexpr uint32_t fixed = MNS * MStage + kGtBytes + XK * 4 + 2 * 4 * XChunk + 2 * 4 * 2048;
  vc::LdsCursor c{0};
  MlpLds l{};
  l.ring = c.take(MNS * MStage, 1024);
  l.b1_bytes = kCuLds - fixed;
  l.b1 = c.take(l.b1_bytes, 16);
  l.gt = c.take(kGtBytes, 16);
  l.b2 = c.take(XK * 4, 16);
  l.tr_a = c.take(4 * XChunk, 16);
  l.tr_b = c.take(4 * XChunk, 16);
  l.hand = c.take(2 * 4 * 2048, 16);
  l.end = c.at;
  return l;
}
static_assert(mlp_lds().end == kCuLds, "mlp2_kernel: 96 + 6 + 8.5 + 1.5 + 16 + 16 + 16 KiB, no padding between the regions");
static_assert(mlp_lds().ring % 1024 == 0 && MStage % 1024 == 0 && XStage % 1024 == 0, "mlp2_kernel: every LDS-DMA piece lands on a 1 KiB boundary");
static_assert(mlp_lds().gt % 16 == 0 && mlp_lds().tr_a % 16 == 0 && mlp_lds().tr_b % 16 == 0 && mlp_lds().hand % 16 == 0,
              "mlp2_kernel: table, transposers and hand-off take 16-byte accesses");
static_assert(mlp_lds().max_hidden() == 1536, "mlp2_kernel: the hidden width include/vitcolmap_hip.h documents");

// ---- x rows of a wave as MFMA B fragments (+ LayerNorm) -----------------------------------------------------------
// Fragment-shaped global loads (32 rows x 32 B per instruction) run at ~5 B/clk/CU, and a staged copy
// through LDS-DMA is limited by the bytes the staging area lets a wave keep in flight.  So the 32 rows
// are fetched in whole 128-byte lines straight into registers — 24 loads of 8 rows x 128 B, all in
// flight at once (the registers that will hold the fragments are the landing zone) — and then turned
// into fragments 64 k at a time through a 4 KiB wave-private LDS transposer `tp` ([32 rows][128 B], 16-byte
// chunk ^ ((row >> 1) & 7): conflict free for the 8-row writes and the 32-row column-slice reads).
// DS operations of one wave execute in order, so the transposer needs no waits between chunks.
// Two halves, because xs_kernel runs the pending block's epilogue while the loads are in flight.
__device__ __forceinline__ void x_rows_issue(v8bf (&xf)[XKS], const __bf16* X, int row0, int M, int lane) {
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int m = min(row0 + 8 * p + (lane >> 3), M - 1);
    const uint8_t* src = (const uint8_t*)X + (size_t)m * (XK * 2) + (lane & 7) * 16;
#pragma unroll
    for (int c = 0; c < XK / 64; ++c) *(v4u*)&xf[4 * c + p] = *(const v4u*)(src + c * 128);   // raw lines land in xf itself
  }
}
__device__ __forceinline__ void x_layernorm(v8bf (&xf)[XKS], float eps);
template <bool LN>
__device__ __forceinline__ void x_rows_finish(v8bf (&xf)[XKS], uint8_t* tp, int lane, float eps) {
  const int r = lane & 31, h = lane >> 5, prow = lane >> 3;
  const int fsw = (r >> 1) & 7;
#pragma unroll
  for (int c = 0; c < XK / 64; ++c) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int row = 8 * p + prow;
      *(v4u*)(tp + row * 128 + (((lane & 7) ^ ((row >> 1) & 7)) << 4)) = *(const v4u*)&xf[4 * c + p];
    }
#pragma unroll
    for (int k4 = 0; k4 < 4; ++k4)
      xf[4 * c + k4] = *(const v8bf*)(tp + r * 128 + (((2 * k4 + h) ^ fsw) << 4));
  }
  if (LN) x_layernorm(xf, eps);
}
// LayerNorm of the rows in xf (without gamma / beta: the prepare step folds them into W and the bias).
__device__ __forceinline__ void x_layernorm(v8bf (&xf)[XKS], float eps) {
  {
    // a lane and its partner (l ^ 32) hold one whole row: two-pass float32 statistics with packed (2-wide) VALU ops;
    // the passes re-expand the bf16 pairs (shift / mask) instead of keeping 192 floats live
    v2f s2 = {0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < XKS; ++ks) {
      const v4u u = *(const v4u*)&xf[ks];
#pragma unroll
      for (int j = 0; j < 4; ++j) s2 += unpack_bf16x2(u[j]);
    }
    float sum = s2[0] + s2[1];
    sum += __shfl_xor(sum, 32);
    const float mean = sum * (1.0f / XK);
    const v2f mean2 = {mean, mean};
#pragma unroll
    for (int ks = 0; ks < XKS; ++ks) asm volatile("" : "+v"(xf[ks]));
    v2f q2 = {0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < XKS; ++ks) {
      const v4u u = *(const v4u*)&xf[ks];
#pragma unroll
      for (int j = 0; j < 4; ++j) { const v2f d = unpack_bf16x2(u[j]) - mean2; q2 = __builtin_elementwise_fma(d, d, q2); }
    }
    float q = q2[0] + q2[1];
    q += __shfl_xor(q, 32);
    const float rstd = __builtin_amdgcn_rsqf(q * (1.0f / XK) + eps);
    const v2f rstd2 = {rstd, rstd};
#pragma unroll
    for (int ks = 0; ks < XKS; ++ks) asm volatile("" : "+v"(xf[ks]));
#pragma unroll
    for (int ks = 0; ks < XKS; ++ks) {
      const v4u u = *(const v4u*)&xf[ks];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const v2f y = (unpack_bf16x2(u[j]) - mean2) * rstd2;
        xf[ks][2 * j] = (__bf16)y[0];
        xf[ks][2 * j + 1] = (__bf16)y[1];
      }
    }
  }
}

// ---- fragment order ("FM") of an [M][384] bf16 tensor in HBM ------------------------------------------------------------
// ceil(M / 32) blocks of 24 KiB; piece ks of block m >> 5 is xf[ks] of the wave that owns rows 32 (m >> 5) .. + 31:
// element (m, k) at byte ((m >> 5) * 24 + (k >> 4)) * 1024 + (((k >> 3) & 1) * 32 + (m & 31)) * 16 + (k & 7) * 2.
// What the K = 384 kernels hold in registers is what lies in memory, so x needs no transposer (24 loads of 1 KiB
// contiguous) and a 32 x 32 block enters and leaves without LDS: behind half_swap a lane holds the two 16-byte chunks
// k = col0 + 16 h + 8 c .. + 7 (c = 0, 1) of its token, slot 32 c + r of piece col0 / 16 + h — per instruction two runs of
// 512 B.  The buffer has the padded row count; a lane whose row is >= M reads row M - 1's slot, as the row-major loaders
// do, so the padding's content never matters, and stores into it are harmless.  row0 is a multiple of 32 everywhere.
constexpr int FmBlock = XKS * 1024;
__device__ __forceinline__ void half_swap(uint32_t (&ep)[8]);   // (with the block-leaving steps below)
__device__ __forceinline__ size_t fm_row_byte(int m, int h) { return (size_t)(m >> 5) * FmBlock + (size_t)((h * 32 + (m & 31)) * 16); }
__device__ __forceinline__ void x_frags_load(v8bf (&xf)[XKS], const __bf16* X, int row0, int M, int lane) {
  const uint8_t* src = (const uint8_t*)X + fm_row_byte(min(row0 + (lane & 31), M - 1), lane >> 5);
#pragma unroll
  for (int ks = 0; ks < XKS; ++ks) xf[ks] = *(const v8bf*)(src + ks * 1024);
}
// chunk c of the block's results behind half_swap; rows past the padded M fall outside num_records and are dropped
__device__ __forceinline__ void block_store_fm(const uint32_t (&ep)[8], __amdgpu_buffer_rsrc_t out_rs, int row0, int nb, int lane, int c) {
  const v4u v = c == 0 ? (v4u){ep[0], ep[1], ep[4], ep[5]} : (v4u){ep[2], ep[3], ep[6], ep[7]};
  __builtin_amdgcn_raw_buffer_store_b128(v, out_rs, (row0 >> 5) * FmBlock + (2 * nb + (lane >> 5)) * 1024 + (c * 32 + (lane & 31)) * 16, 0, 0);
}
__host__ __device__ constexpr size_t fm_bytes(long long rows) { return (size_t)((rows + 31) / 32) * FmBlock; }
// The residual of a block: the same two chunks, loaded (2 loads of 16 bytes per lane, as many as the row-major form issues:
// xs_kernel's counted vmcnt(7) / vmcnt(5) stay what they are) ...
__device__ __forceinline__ v4u res_load_fm(const __bf16* res, int row0, int M, int nb, int lane, int c) {
  const int m = min(row0 + (lane & 31), M - 1);
  return *(const v4u*)((const uint8_t*)res + (size_t)(m >> 5) * FmBlock + (2 * nb + (lane >> 5)) * 1024 + (c * 32 + (m & 31)) * 16);
}
// ... and taken back into the accumulator layout by half_swap, which is its own inverse: rp[2g], rp[2g + 1] = features
// 8g + 4h .. + 3 of token r as bf16 pairs
__device__ __forceinline__ void res_unswap_fm(uint32_t (&rp)[8], const v4u (&resq)[2]) {
  rp[0] = resq[0][0]; rp[1] = resq[0][1]; rp[4] = resq[0][2]; rp[5] = resq[0][3];
  rp[2] = resq[1][0]; rp[3] = resq[1][1]; rp[6] = resq[1][2]; rp[7] = resq[1][3];
  half_swap(rp);
}
__device__ __forceinline__ v4bf res_group_fm(const uint32_t (&rp)[8], int g) {
  return __builtin_bit_cast(v4bf, (v2u){rp[2 * g], rp[2 * g + 1]});
}

// ---- table GELU of one 32 x 32 block, cut into slices 0-15 that ride between the MFMAs of the next block ---------------
// MFMA layout: lane = token r, half h, accumulator register 4g + j = feature 8g + 4h + j; packed register 2g (2g + 1)
// holds the bf16 pair j = 0, 1 (2, 3) of group g.
struct BlockState {
  uint32_t pb[8];    // pre-activations as bf16 pairs
  uint32_t gq[8];    // looked-up halves in flight (ring of 4 packed registers)
  uint32_t ep[8];    // the block's results as bf16 pairs
  uint32_t gbad;     // largest table index seen (out-of-range detector)
};
__device__ __forceinline__ void pack_group(uint32_t (&dst)[8], int g, float v0, float v1, float v2, float v3) {
  dst[2 * g] = pack_bf16x2(v0, v1);
  dst[2 * g + 1] = pack_bf16x2(v2, v3);
}
// slices 0-3: pre-activations -> bf16 pairs (pb), the only float work; 4-11: table index + LDS gather of packed register
// sl - 4; 7-14: results packed back (three slices, ~100+ cycles, after the gather was issued); 15: range check — a value
// outside the table's range somewhere in the wave sends the block through the float path.  s.ep is complete after slice 15.
__device__ __forceinline__ void gelu_table_slice(int sl, const v16f& pre, BlockState& s, const uint8_t* gt_l) {
  if (sl < 4) {
    pack_group(s.pb, sl, pre[4 * sl], pre[4 * sl + 1], pre[4 * sl + 2], pre[4 * sl + 3]);
    if (sl == 0) s.gbad = 0;
  }
  if (sl >= 4 && sl < 12) {
    const int qd = sl - 4;
    const uint32_t b0 = s.pb[qd] & 0xffffu, b1 = s.pb[qd] >> 16;
    const uint32_t k0 = (b0 & 0x7fffu) - kGtLo, k1 = (b1 & 0x7fffu) - kGtLo;   // wraps to a huge value below the range
    s.gbad = max(s.gbad, max(k0, k1));
    s.gq[2 * (qd & 3)] = *(const uint16_t*)(gt_l + min(k0, kGtN - 1) * 4 + ((b0 >> 15) << 1));
    s.gq[2 * (qd & 3) + 1] = *(const uint16_t*)(gt_l + min(k1, kGtN - 1) * 4 + ((b1 >> 15) << 1));
  }
  if (sl >= 7 && sl < 15) {
    const int qd = sl - 7;
    s.ep[qd] = s.gq[2 * (qd & 3)] | (s.gq[2 * (qd & 3) + 1] << 16);
  }
  if (sl == 15) {
    if (__any(s.gbad >= kGtN)) {
#pragma unroll
      for (int qd = 0; qd < 8; ++qd) {
        const v2f y = gelu_erf2(unpack_bf16x2(s.pb[qd]));
        s.ep[qd] = pack_bf16x2(y[0], y[1]);
      }
    }
  }
}

// ---- a 32 (features) x 32 (tokens) D^T block leaves --------------------------------------------------------------------
// A row-per-lane global access (32 rows per instruction) is issue-bound in the texture path, so both the residual read
// and the result write go through wave-private transposers — [32 tokens][64 B], 16-byte chunk ^ ((token >> 2) & 3),
// conflict free both ways — and touch memory as lane -> (token l >> 2 (+16 q), 16-byte chunk l & 3): 16 rows x 64
// contiguous bytes per instruction.  DS operations of one wave execute in order, so no wait separates write and read.
// Results leave through a raw buffer store: rows past M fall outside num_records and are dropped by the hardware, so
// every block issues exactly two store instructions (xs_kernel's vmcnt bookkeeping counts them).
// The steps, in order: pack_group x 4; half_swap; tr_write; tr_read x 2; block_store x 2.  Residual side: res_load x 2
// (whole lines), res_write x 2, res_read per group (the lane's own 8 bytes back in the accumulator layout).
__device__ __forceinline__ uint8_t* tr_line(uint8_t* tr, int lane, int q) {   // the lane's 16 bytes in the whole-line view
  const int row = (lane >> 2) + 16 * q;
  return tr + row * 64 + (((lane & 3) ^ ((row >> 2) & 3)) << 4);
}
// exchange with the partner lane (l ^ 32): h = 0 ends with features 0..15, h = 1 with 16..31
__device__ __forceinline__ void half_swap(uint32_t (&ep)[8]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {     // i = 0,1: group 0 <-> group 2;  i = 2,3: group 1 <-> group 3
    const auto sw = __builtin_amdgcn_permlane32_swap(ep[i], ep[i + 4], false, false);
    ep[i] = sw[0];
    ep[i + 4] = sw[1];
  }
}
__device__ __forceinline__ void tr_write(uint8_t* tr_out, const uint32_t (&ep)[8], int lane) {
  const int r = lane & 31, h = lane >> 5, rsw = (r >> 2) & 3;
  *(v4u*)(tr_out + r * 64 + (((2 * h) ^ rsw) << 4)) = (v4u){ep[0], ep[1], ep[4], ep[5]};
  *(v4u*)(tr_out + r * 64 + (((2 * h + 1) ^ rsw) << 4)) = (v4u){ep[2], ep[3], ep[6], ep[7]};
}
__device__ __forceinline__ v4u tr_read(uint8_t* tr_out, int lane, int q) { return *(const v4u*)tr_line(tr_out, lane, q); }
// rows row0 .. row0 + 31 of an [M][n_cols] output, columns col0 .. col0 + 31
__device__ __forceinline__ void block_store(v4u v, __amdgpu_buffer_rsrc_t out_rs, int row0, int n_cols, int col0, int lane, int q) {
  const int row = (lane >> 2) + 16 * q;
  __builtin_amdgcn_raw_buffer_store_b128(v, out_rs, (int)(((size_t)(row0 + row) * n_cols + col0 + (lane & 3) * 8) * 2), 0, 0);
}
__device__ __forceinline__ v4u res_load(const __bf16* res, int row0, int M, int n_cols, int col0, int lane, int q) {
  return *(const v4u*)(res + (size_t)min(row0 + (lane >> 2) + 16 * q, M - 1) * n_cols + col0 + (lane & 3) * 8);
}
__device__ __forceinline__ void res_write(uint8_t* tr_res, v4u v, int lane, int q) { *(v4u*)tr_line(tr_res, lane, q) = v; }
__device__ __forceinline__ v4bf res_read(const uint8_t* tr_res, int lane, int g) {   // features 8g + 4h .. + 3 of token r
  const int r = lane & 31, h = lane >> 5;
  return *(const v4bf*)(tr_res + r * 64 + ((g ^ ((r >> 2) & 3)) << 4) + 8 * h);
}

// ---- one 32 x 32 x 384 product ----------------------------------------------------------------------------------------
// The bias is the accumulator's initial value: register 4g + j <- bias32[8g + 4h + j] (bias32: the block's 32 floats in LDS).
__device__ __forceinline__ void acc_from_bias(v16f& acc, const float* bias32, int lane) {
  const float* bl = bias32 + 4 * (lane >> 5);
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const v4f bv = *(const v4f*)(bl + 8 * g);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[4 * g + j] = bv[j];
  }
}
// The 24 MFMAs of a stage (`st`: the lane's 16 bytes of piece 0; pieces are 1 KiB apart).  W fragments are read RD
// k-steps ahead of the MFMA that consumes them (LDS latency ~ 4 MFMAs); then [MFMA, fragment read, behind(ks)] per
// k-step — `behind` is the caller's epilogue slice and / or LDS-DMA piece — with a sched_barrier pinning each group; the
// compiler places the waits.  (The fragment array lives in here: handed in by reference from a caller with two loops,
// xs_kernel's LayerNorm instantiations gained 32-52 bytes of scratch.)
template <int RD, typename F>
__device__ __forceinline__ void stage_mfmas(v16f& acc, const uint8_t* st, const v8bf (&xf)[XKS], F&& behind) {
  v8bf wf[XKS];
#pragma unroll
  for (int ks = 0; ks < RD; ++ks) wf[ks] = *(const v8bf*)(st + ks * 1024);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int ks = 0; ks < XKS; ++ks) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[ks], xf[ks], acc, 0, 0, 0);
    if (ks + RD < XKS) wf[ks + RD] = *(const v8bf*)(st + (ks + RD) * 1024);
    behind(ks);
    __builtin_amdgcn_sched_barrier(0);
  }
}

// ---- prepare side: one fc1-type weight row into fragment order ------------------------------------------------------------
// Row `rr` of a 32-feature block `blk` (XStage / 2 elements): piece ks = k >> 4 is the 1 KiB A operand of k-step ks, lane
// 32 hh + rr holds k = 16 ks + 8 hh .. + 7.  LayerNorm's gamma is folded into the weights; returns the wave's sum of
// w[k] beta[k], the row's share of the folded bias.  One wave per row.
__device__ __forceinline__ float fc1_row_to_fragments(const float* __restrict__ w, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, __bf16* __restrict__ blk, int rr, int lane) {
  float dot = 0.f;
  for (int k = lane; k < XK; k += 64) {
    const float wk = w[k];
    if (beta) dot += wk * beta[k];
    const int ks = k >> 4, hh = (k >> 3) & 1, j = k & 7;
    blk[((size_t)ks * 64 + hh * 32 + rr) * 8 + j] = (__bf16)(gamma ? wk * gamma[k] : wk);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) dot += __shfl_xor(dot, o);
  return dot;
}

// =====================================================================================================
// xs_kernel (described above the K = 384 constants).
constexpr int XReadAhead = 8;  // W fragments read ahead of the MFMA that uses them
constexpr int XIssue0 = 1;      // MFMA behind which the first piece of stage i + 2 is issued ...
constexpr int XIssueStep = 8;   // ... and the distance to the next (the last one stays ahead of the result stores at slice 19)
// XF / RF / OF: x, the residual, the output in fragment order (FM, shared section) instead of row-major; OF needs N == 384.
template <int EPI, bool LN, bool GT, bool XF = false, bool RF = false, bool OF = false>
__global__ __launch_bounds__(512, 1) void xs_kernel(const __bf16* __restrict__ X, const uint8_t* __restrict__ Wp,
                                                    const float* __restrict__ biasf, const __bf16* res,
                                                    __bf16* out, int M, int N, int n_nb, int n_stages, float eps,
                                                    const uint16_t* __restrict__ gelu_tab) {
  constexpr bool RES_RM = EPI == EPI_RESIDUAL && !RF;      // the epilogue's transposers are in use
  constexpr XsLds L = xs_lds(XF, RES_RM || !OF);
  constexpr int TrWave = XF ? XChunk : 2 * XChunk;
  __shared__ __attribute__((aligned(1024))) uint8_t lds[L.end];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  const int G = gridDim.x, bid = blockIdx.x;
  const int s0 = (int)((long long)n_stages * bid / G), s1 = (int)((long long)n_stages * (bid + 1) / G);
  const int n = s1 - s0;
  if (n <= 0) return;

  float* bias_l = (float*)(lds + L.bias);
  for (int i = tid; i < N; i += 512) bias_l[i] = biasf[i];   // visible after the first stage barrier
  uint8_t* const gt_l = lds + L.table(N);   // (the host passes GT only where L.table_fits(N))
  if (GT)
    for (int i = tid; i < kGtBytes / 4; i += 512) ((uint32_t*)gt_l)[i] = ((const uint32_t*)gelu_tab)[i];

  const uint32_t lds0 = vc::lds_addr(&lds[0]);
  // ---- producer: wave w issues pieces 3w..3w+2 of every stage ------------------------------------
  int inb = s0 % n_nb, islot = 0, ileft = n;   // feature block / ring slot / stages left to issue
  // One piece: wave-uniform base in SGPRs + one per-lane offset (with per-piece 64-bit VGPR addresses the compiler keeps
  // three pairs alive across the stage loop).  The last piece of a stage advances the stream.
  const uint32_t lane_off16 = (uint32_t)lane * 16u;
  auto issue_piece = [&](int i) {
    const uint8_t* sbase = Wp + (size_t)inb * XStage + (size_t)(wave * 3 + i) * 1024;
    const uint32_t dst = lds0 + (uint32_t)islot * XStage + (uint32_t)(wave * 3 + i) * 1024u;
    vc::lds_dma16(sbase, lane_off16, dst);
    if (i == 2) {
      // past the end the last stage is staged again into a slot nobody reads (keeps the vmcnt counts uniform)
      if (ileft > 1) { --ileft; inb = inb + 1 == n_nb ? 0 : inb + 1; }
      islot = islot + 1 == XNS ? 0 : islot + 1;
    }
  };
  auto issue = [&]() {
#pragma unroll
    for (int i = 0; i < 3; ++i) issue_piece(i);
  };
#pragma unroll
  for (int j = 0; j < XPF; ++j) issue();

  // ---- x rows of this wave as B fragments (x_rows_issue / x_rows_finish) ----------------------------------------
  v8bf xf[XKS];
  uint8_t* const tr_out = lds + L.tr + wave * TrWave;   // x transposer, then out / residual transposers (idle x staging)
  uint8_t* const tr_res = tr_out + 2048;

  // ---- epilogue of one 32 (features) x 32 (tokens) block (the block-leaving steps above).
  // The epilogue of block i-1 is cut into 24 slices that are issued BETWEEN the 24 MFMAs of block i, in the
  // same wave (all 8 waves run the same stream, no wave roles).  tools/overlap_probe.hip: float32 VALU work does
  // not overlap with the matrix pipe on this part however it is arranged (integer VALU work does), so this
  // costs the same as running the epilogue as a cluster — time = MFMA time + float VALU time — and is kept
  // for its simplicity; the lever for this kernel is fewer float instructions per output.
  const __amdgpu_buffer_rsrc_t out_rs = __builtin_amdgcn_make_buffer_rsrc(out, 0, OF ? (int)fm_bytes(M) : (int)((size_t)M * N * 2), 0x00020000);
  constexpr bool TABLE = EPI == EPI_GELU && GT;
  // the slices at which a finished block (s.ep) is exchanged, written to the transposer, read back and stored: behind the
  // table's 16 slices, or behind 8 slices of float work (values 2 sl, 2 sl + 1) and 4 of packing
  struct Leave { int swap, write, read, store; };
  constexpr Leave at = TABLE ? Leave{16, 17, 19, 22} : Leave{12, 13, 15, 19};
  // state that flows from slice to slice
  v4u resq[2];      // the next block's residual lines
  uint32_t rp[8];   // (RF) the pending block's residual in the accumulator layout
  v16f pa;          // the pending block's accumulators
  float ev[16];     // ... after GELU / residual
  BlockState s;     // ... packed to bf16 pairs
  v4u eo[2];        // ... transposed for the store
  int pm_base = 0, pnb = 0;
  auto load_res = [&](int m_base, int nb) {
    if (EPI == EPI_RESIDUAL) {
#pragma unroll
      for (int q = 0; q < 2; ++q) resq[q] = RF ? res_load_fm(res, m_base, M, nb, lane, q) : res_load(res, m_base, M, N, nb * 32, lane, q);
    }
  };
  auto res_to_lds = [&]() {   // the pending block's residual (loaded an iteration ago) enters the transposer (RF: rp)
    if (EPI == EPI_RESIDUAL) {
      if (RF) {
        res_unswap_fm(rp, resq);
      } else {
#pragma unroll
        for (int q = 0; q < 2; ++q) res_write(tr_res, resq[q], lane, q);
      }
    }
  };
  auto slice = [&](int sl) {
    if (TABLE) {
      gelu_table_slice(sl, pa, s, gt_l);
    } else if (sl < 8) {
      const int j0 = 2 * sl;
      if (EPI == EPI_GELU) {
        const v2f y = gelu_erf2((v2f){pa[j0], pa[j0 + 1]});
        ev[j0] = y[0];
        ev[j0 + 1] = y[1];
      } else if (EPI == EPI_RESIDUAL) {
        if ((sl & 1) == 0) {            // one 8-byte read serves values 4g .. 4g + 3
          const int g = sl >> 1;
          const v4bf rv = RF ? res_group_fm(rp, g) : res_read(tr_res, lane, g);
#pragma unroll
          for (int j = 0; j < 4; ++j) ev[4 * g + j] = pa[4 * g + j] + (float)rv[j];
        }
      } else {
        ev[j0] = pa[j0];
        ev[j0 + 1] = pa[j0 + 1];
      }
    } else if (sl < 12) {
      const int g = sl - 8;
      pack_group(s.ep, g, ev[4 * g], ev[4 * g + 1], ev[4 * g + 2], ev[4 * g + 3]);
    }
    if (sl == at.swap) half_swap(s.ep);
    if (!OF && sl == at.write) tr_write(tr_out, s.ep, lane);
    if (!OF && sl == at.read) {
#pragma unroll
      for (int q = 0; q < 2; ++q) eo[q] = tr_read(tr_out, lane, q);
    }
    if (sl == at.store) {   // (OF: at the same slice, behind the stage's last LDS-DMA piece, which the vmcnt counts rely on)
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        if (OF) block_store_fm(s.ep, out_rs, pm_base, pnb, lane, q);
        else block_store(eo[q], out_rs, pm_base, N, pnb * 32, lane, q);
      }
    }
  };

  v16f acc;
  int mt_cur = -1, slot = 0;
  int mt = s0 / n_nb, nb = s0 - mt * n_nb;
  for (int i = 0; i < n; ++i) {
    // This wave's pieces of stage i (issued BETWEEN the MFMAs of iteration i-2) have landed once only operations issued
    // after them are pending.  Per iteration a wave issues (residual epilogue) 2 loads, then inside the MFMA loop its 3
    // pieces and the 2 result stores of the pending block: iteration i-1 alone accounts for 5 (+2) younger operations in
    // every case — steady state, behind a row-tile switch (whose x loads drain everything older anyway) and while the
    // pipeline fills from iteration 2 on; the stores of iteration i-2 that follow its last piece are not counted, so the
    // wait is never too weak.  Counting keeps a wave from stalling on the write acknowledgement of its latest stores.
    if (i >= 2) {
      if (EPI == EPI_RESIDUAL) asm volatile("s_waitcnt vmcnt(7)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    const bool pending = i > 0;
    if (pending) res_to_lds();
    const bool reload = mt != mt_cur;
    // (stage i + 2 goes into the slot read during iteration i - 1: its three pieces are issued between this
    // iteration's MFMAs — in a block behind the barrier they held every wave for 150-300 cycles with the matrix pipe idle)
    const int m_base = mt * XRows + wave * 32;
    if (reload) {
      // new row tile: the pending block cannot ride under this block's MFMAs (its x loads come first)
      if (XF) x_frags_load(xf, X, m_base, M, lane);
      else x_rows_issue(xf, X, m_base, M, lane);
      if (pending) {
#pragma unroll
        for (int sl = 0; sl < XKS; ++sl) slice(sl);
      }
      if (!XF) x_rows_finish<LN>(xf, tr_out, lane, eps);
      else if (LN) x_layernorm(xf, eps);
      mt_cur = mt;
    }
    load_res(m_base, nb);
    const uint8_t* st = lds + slot * XStage + lane * 16;
    acc_from_bias(acc, bias_l + nb * 32, lane);
    {
      constexpr int XRD = TABLE ? 6 : XReadAhead;   // the table epilogue needs the registers
      auto piece_behind = [&](int ks) {
        if (ks == XIssue0 || ks == XIssue0 + XIssueStep || ks == XIssue0 + 2 * XIssueStep)
          issue_piece((ks - XIssue0) / XIssueStep);
      };
      if (pending && !reload)
        stage_mfmas<XRD>(acc, st, xf, [&](int ks) { slice(ks); piece_behind(ks); });
      else
        stage_mfmas<XRD>(acc, st, xf, piece_behind);
    }
    pa = acc;
    pm_base = m_base;
    pnb = nb;
    slot = slot + 1 == XNS ? 0 : slot + 1;
    if (++nb == n_nb) { nb = 0; ++mt; }
  }
  // the last block's epilogue has no MFMAs to ride under
  res_to_lds();
#pragma unroll
  for (int sl = 0; sl < XKS; ++sl) slice(sl);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // drain the clamped refills before the LDS is released
}

// W [N][K] float32 (+ optional LayerNorm gamma / beta [K] folded in) -> fragment-ordered bf16 + float32 bias.
__global__ __launch_bounds__(256) void xs_prepare_kernel(const float* __restrict__ W, const float* __restrict__ b,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         int N, __bf16* __restrict__ Wp, float* __restrict__ biasf) {
  // one wave per output feature n
  const int lane = threadIdx.x & 63;
  const int nfeat = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (nfeat >= N) return;
  const float dot = fc1_row_to_fragments(W + (size_t)nfeat * XK, gamma, beta, Wp + (size_t)(nfeat >> 5) * (XStage / 2), nfeat & 31, lane);
  if (lane == 0) biasf[nfeat] = (b ? b[nfeat] : 0.f) + dot;
}


// =====================================================================================================
// Fused MLP for 384-wide models:  x += fc2(gelu(fc1(LayerNorm(x))))  in ONE kernel, so the hidden tensor
// (76 550 x 1536 bf16 = 235 MB, written by fc1 and read back by fc2: a third of a block's HBM traffic) never
// exists and fc2 no longer stages both operands through L2 -> LDS.  Structure = the x-stationary kernel with a
// second product per stage:
//   * a stage is one 32-wide chunk of the hidden layer: 24 pieces of W1 (as in xs_kernel) + 24 pieces of W2
//     (12 output blocks x 2 k-steps), 48 KiB, ring of 2;
//   * per stage: H^T(32 hidden x 32 tokens) = W1c X^T (24 MFMAs, bias as initial value) -> GELU by the LDS table
//     (integer work) -> the bf16 pairs ARE the B operand of Out^T += W2c^T-tile x G^T (24 MFMAs; accumulator tile as
//     the next MFMA's operand: W2's k order is permuted by the prepare step to match the register order);
//   * after the last chunk of a row tile: + fc2 bias + residual (the tile's own x rows, read back), stored in place.
// Row tiles are dealt round-robin to one persistent workgroup per CU.

// mlp2_kernel splits the work by role: 8 waves, two per SIMD.  Waves 0-3 ("A") keep the
// normalised x rows and compute H^T chunk by chunk + the GELU; waves 4-7 ("B") keep the 384 x 32 output accumulators
// and run fc2 one stage behind, taking the 32 x 32 bf16 activation tile of their partner (same SIMD, same 32 token rows)
// through a 2 KiB LDS buffer.  Compared with one wave doing both (the single-role kernel of DESIGN.md §4.3): both register
// sets fit 256 VGPRs, so a SIMD holds an fc1 wave and an fc2 wave whose MFMA streams share the matrix pipe, the GELU's
// integer work runs beside the partner's MFMAs, and the LDS-DMA pieces of a stage are issued by 8 waves instead of 4
// (a piece occupies its wave for ~180 cycles: with 12 pieces per wave the staging alone took 2170 cycles per stage).
// Stage i in the ring = [W1 chunk c_i | W2 chunk c_{i-1}] so both halves are consumed in iteration i.
// The LDS layout is mlp_lds (shared section above).

constexpr int M2ReadAhead = 6;    // weight fragments read ahead of the MFMA that uses them
constexpr int M2PiecesA = 3;      // LDS-DMA pieces of a stage issued by each fc1 wave (each fc2 wave issues the other 9): the fc1 role is the longer one
constexpr int M2Issue0 = 1;       // first MFMA behind which a piece of the next stage is issued ...
constexpr int M2IssueStep = 3;    // ... and the distance to the next one (sweep: 1+3k 228 us, 1+2k 229, 0+k 233, 1+4k 235)
constexpr int M2IssueStepB = 2;   // the distance on an fc2 wave with more than six pieces per stage
// XF: x (read by the fc1 waves, and again as the residual) in fragment order (FM, shared section); OF: the result too, in
// place.  XF without OF writes row-major rows into Out, a buffer of its own; otherwise Out is not looked at.
template <bool XF = false, bool OF = false>
__global__ __launch_bounds__(512, 2) void mlp2_kernel(__bf16* __restrict__ X, const uint8_t* __restrict__ Wm,
                                                      const float* __restrict__ b1f, const float* __restrict__ b2f,
                                                      int M, int n_chunks, int n_tiles, float eps,
                                                      const uint16_t* __restrict__ gelu_tab, __bf16* Out) {
  static_assert(XF || !OF, "mlp2_kernel: a row-major x is updated in place");
  constexpr MlpLds L = mlp_lds();
  __shared__ __attribute__((aligned(1024))) uint8_t lds[L.end];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool roleB = wave >= 4;
  const int pairw = wave & 3;                       // row block of the pair inside the 128-row tile
  const int G = gridDim.x, bid = blockIdx.x;
  const int my_tiles = bid < n_tiles ? (n_tiles - bid + G - 1) / G : 0;
  const int n = my_tiles * n_chunks;                // fc1 stages; fc2 runs one iteration behind
  if (n <= 0) return;

  float* const b1_l = (float*)(lds + L.b1);
  float* const b2_l = (float*)(lds + L.b2);
  uint8_t* const gt_l = lds + L.gt;
  for (int i = tid; i < n_chunks * 32; i += 512) b1_l[i] = b1f[i];
  for (int i = tid; i < XK; i += 512) b2_l[i] = b2f[i];
  for (int i = tid; i < kGtBytes / 4; i += 512) ((uint32_t*)gt_l)[i] = ((const uint32_t*)gelu_tab)[i];

  const uint32_t lds0 = vc::lds_addr(&lds[0]);
  // producer: waves 0-3 issue the W1 half of a stage (chunk c1), waves 4-7 the W2 half (chunk c2), six pieces each.
  // One piece: wave-uniform base in SGPRs + one per-lane offset
  // shared by all pieces — with a 64-bit address per piece in VGPRs the compiler kept six pairs alive, spilled them,
  // and every reload in the stage loop waited for vmcnt(0), i.e. for the copy just issued
  const uint32_t lane_off = (uint32_t)lane * 16u;
  constexpr int NA = M2PiecesA, NB = 12 - NA;       // pieces per fc1 / fc2 wave and stage (48 pieces: 24 of W1, then 24 of W2)
  auto issue_piece = [&](int c1, int c2, int slot, int i) {
    const int role = wave >> 2, q = wave & 3;
    if (i >= (role ? NB : NA)) return;
    const int id = role ? 4 * NA + q * NB + i : q * NA + i;
    const int half = id >= 24, idx = id - 24 * half;
    const int c = half ? c2 : c1;
    const uint8_t* sbase = Wm + (size_t)c * MStage + (size_t)half * XStage + (size_t)idx * 1024;
    const uint32_t dst = lds0 + (uint32_t)slot * MStage + (uint32_t)half * XStage + (uint32_t)idx * 1024u;
    vc::lds_dma16(sbase, lane_off, dst);
  };
  auto issue = [&](int c1, int c2, int slot) {
#pragma unroll
    for (int i = 0; i < (NA > NB ? NA : NB); ++i) issue_piece(c1, c2, slot, i);
  };

  // Iteration i (0 .. n+1) works on ring stage i = [W1 chunk of fc1 stage i | W2 chunk of fc1 stage i-2]:
  //   A waves: MFMAs of fc1 stage i, with the GELU of stage i-1 (integer work + LDS gathers, which overlap with MFMAs
  //            in the same wave) issued in slices between them; the activation tile of stage i-1 is handed over at the end;
  //   B waves: fc2 partial product with the activation tile of stage i-2.
  int chunk = 0, slot = 0, tile = bid;
  auto chunk_of = [&](int j) { return j % n_chunks; };
  auto issue_stage = [&](int j, int slot_) {        // stage j; clamped chunks stage data nobody reads
    const int c1 = chunk_of(min(max(j, 0), n - 1)), c2 = chunk_of(min(max(j - 2, 0), n - 1));
    issue(c1, c2, slot_);
  };
  issue_stage(0, 0);
  if (!roleB) {
    // =========================== A: x rows, fc1, GELU ======================================================
    v8bf xf[XKS];
    uint8_t* const tp = lds + L.tr_a + pairw * XChunk;
    v16f hprev;                                      // pre-activations of stage i-1
    BlockState s;                                    // ... their GELU, flowing from slice to slice
    auto gelu_slice = [&](int sl, int parity) {
      gelu_table_slice(sl, hprev, s, gt_l);
      if (sl == 16) {                                // hand the activation tile to the partner (k-step 0, k-step 1)
        uint8_t* const gb = lds + L.hand + (parity * 4 + pairw) * 2048 + lane * 16;
        *(v4u*)gb = (v4u){s.ep[0], s.ep[1], s.ep[2], s.ep[3]};
        *(v4u*)(gb + 1024) = (v4u){s.ep[4], s.ep[5], s.ep[6], s.ep[7]};
      }
    };
    for (int i = 0; i <= n + 1; ++i) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      // The six pieces of the next stage are issued BETWEEN this stage's MFMAs, one every four (round 2: issued in a
      // block they held the wave for 300-650 cycles with its matrix pipe idle; in the fc2 waves, where the block sat
      // behind the MFMAs, the copies' whole L2 latency was then waited for at the top of the next stage — ~750 cycles
      // of every stage).  Stages without MFMAs issue them at once.
      const bool do_issue = i <= n;
      const int nc1 = chunk_of(min(max(i + 1, 0), n - 1)), nc2 = chunk_of(min(max(i - 1, 0), n - 1));
      if (do_issue && !(i < n && i > 0)) issue_stage(i + 1, slot ^ 1);
      if (i < n) {
        if (chunk == 0) {
          if (XF) {
            x_frags_load(xf, X, tile * 128 + pairw * 32, M, lane);
            x_layernorm(xf, eps);
          } else {
            x_rows_issue(xf, X, tile * 128 + pairw * 32, M, lane);
            x_rows_finish<true>(xf, tp, lane, eps);
          }
        }
        const uint8_t* st = lds + slot * MStage + lane * 16;
        v16f hacc;
        acc_from_bias(hacc, b1_l + chunk * 32, lane);
        // the fc1 role is the longer one (its GELU slices and x load ride in this phase): it gets the issue priority on
        // its SIMD — 238 -> 230 us per layer; raising the fc2 role instead loses
        __builtin_amdgcn_s_setprio(1);
        if (i > 0)
          stage_mfmas<M2ReadAhead>(hacc, st, xf, [&](int ks) {
            gelu_slice(ks, (i - 1) & 1);
            if (ks >= M2Issue0 && ks < M2Issue0 + NA * M2IssueStep && (ks - M2Issue0) % M2IssueStep == 0 && do_issue)
              issue_piece(nc1, nc2, slot ^ 1, (ks - M2Issue0) / M2IssueStep);
          });
        else
          stage_mfmas<M2ReadAhead>(hacc, st, xf, [](int) {});
        __builtin_amdgcn_s_setprio(0);
        hprev = hacc;
        if (++chunk == n_chunks) { chunk = 0; tile += G; }
      } else if (i == n) {
        // the last stage's GELU has no MFMAs to ride under
#pragma unroll
        for (int sl = 0; sl < XKS; ++sl) gelu_slice(sl, (i - 1) & 1);
      }
      slot ^= 1;
    }
  } else {
    // =========================== B: fc2 accumulators, two stages behind, tile epilogue ==========================
    v16f oacc[12];
    const __amdgpu_buffer_rsrc_t out_rs =
        __builtin_amdgcn_make_buffer_rsrc(XF && !OF ? Out : X, 0, OF ? (int)fm_bytes(M) : (int)((size_t)M * XK * 2), 0x00020000);
    uint8_t* const tr_out = lds + L.tr_b + pairw * XChunk;
    uint8_t* const tr_res = tr_out + 2048;
    int pchunk = 0;                                  // chunk consumed in this iteration (that of fc1 stage i-2)
    for (int i = 0; i <= n + 1; ++i) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      const bool do_issue = i <= n;
      const int nc1 = chunk_of(min(max(i + 1, 0), n - 1)), nc2 = chunk_of(min(max(i - 1, 0), n - 1));
      if (i >= 2) {
        if (pchunk == 0) {
#pragma unroll
          for (int ob = 0; ob < 12; ++ob)
#pragma unroll
            for (int j = 0; j < 16; ++j) oacc[ob][j] = 0.f;
        }
        const uint8_t* gb = lds + L.hand + ((i & 1) * 4 + pairw) * 2048 + lane * 16;   // parity of stage i-2
        const v8bf g_s0 = *(const v8bf*)gb, g_s1 = *(const v8bf*)(gb + 1024);
        const uint8_t* st2 = lds + slot * MStage + XStage + lane * 16;
        {
          constexpr int RD = M2ReadAhead;
          v8bf wf[24];
#pragma unroll
          for (int q = 0; q < RD; ++q) wf[q] = *(const v8bf*)(st2 + q * 1024);
#pragma unroll
          for (int q = 0; q < 24; ++q) {
            oacc[q >> 1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[q], (q & 1) ? g_s1 : g_s0, oacc[q >> 1], 0, 0, 0);
            if (q + RD < 24) wf[q + RD] = *(const v8bf*)(st2 + (q + RD) * 1024);
            constexpr int BSTEP = NB <= 6 ? M2IssueStep : M2IssueStepB;
            if (q >= M2Issue0 && q < M2Issue0 + NB * BSTEP && (q - M2Issue0) % BSTEP == 0 && do_issue)
              issue_piece(nc1, nc2, slot ^ 1, (q - M2Issue0) / BSTEP);   // (see the A waves)
          }
        }
        if (pchunk == n_chunks - 1) {
          const int m0w = tile * 128 + pairw * 32;
#pragma unroll 1
          for (int ob = 0; ob < 12; ++ob) {
            // the block-leaving steps of the shared section, as one cluster
            v4u resq[2];
#pragma unroll
            for (int q = 0; q < 2; ++q) resq[q] = XF ? res_load_fm(X, m0w, M, ob, lane, q) : res_load(X, m0w, M, XK, ob * 32, lane, q);
            uint32_t rp[8];
            if (XF) {
              res_unswap_fm(rp, resq);
            } else {
#pragma unroll
              for (int q = 0; q < 2; ++q) res_write(tr_res, resq[q], lane, q);
            }
            v16f oa;
            switch (ob) {   // dynamic index into the register tiles
#define VC_OB(k) case k: oa = oacc[k]; break;
              VC_OB(0) VC_OB(1) VC_OB(2) VC_OB(3) VC_OB(4) VC_OB(5) VC_OB(6) VC_OB(7) VC_OB(8) VC_OB(9) VC_OB(10)
              default: oa = oacc[11]; break;
#undef VC_OB
            }
            uint32_t ep[8];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
              const v4bf rv = XF ? res_group_fm(rp, g) : res_read(tr_res, lane, g);
              const v4f bv = *(const v4f*)(b2_l + ob * 32 + 8 * g + 4 * (lane >> 5));
              float v[4];
#pragma unroll
              for (int j = 0; j < 4; ++j) v[j] = oa[4 * g + j] + bv[j] + (float)rv[j];
              pack_group(ep, g, v[0], v[1], v[2], v[3]);
            }
            half_swap(ep);
            if (OF) {
#pragma unroll
              for (int q = 0; q < 2; ++q) block_store_fm(ep, out_rs, m0w, ob, lane, q);
            } else {
              tr_write(tr_out, ep, lane);
#pragma unroll
              for (int q = 0; q < 2; ++q) block_store(tr_read(tr_out, lane, q), out_rs, m0w, XK, ob * 32, lane, q);
            }
          }
          tile += G;
        }
        if (++pchunk == n_chunks) pchunk = 0;
      }
      if (do_issue && i < 2) issue_stage(i + 1, slot ^ 1);   // (no MFMAs to issue them between)
      slot ^= 1;
    }
  }
}

// MLP weights -> stage order: chunk c = [24 pieces of W1' (features 32c..+32, LayerNorm gamma folded) | 24 pieces of W2
// (piece 2 ob + s: output features 32 ob..+32, hidden 32c + 16s + 8(j>>2) + 4h + (j&3) in element j of lane 32h + r)].
__global__ __launch_bounds__(256) void mlp_prepare_kernel(const float* __restrict__ W1, const float* __restrict__ b1,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta,
                                                          const float* __restrict__ W2, const float* __restrict__ b2,
                                                          int n_hid, __bf16* __restrict__ Wm, float* __restrict__ b1f,
                                                          float* __restrict__ b2f) {
  const int lane = threadIdx.x & 63;
  const int unit = blockIdx.x * 4 + (threadIdx.x >> 6);   // hidden feature (fc1 part), then output feature (fc2 part)
  if (unit < n_hid) {
    const float dot = fc1_row_to_fragments(W1 + (size_t)unit * XK, gamma, beta, Wm + (size_t)(unit >> 5) * (MStage / 2), unit & 31, lane);
    if (lane == 0) b1f[unit] = (b1 ? b1[unit] : 0.f) + dot;
  } else if (unit < n_hid + XK) {
    const int f = unit - n_hid, ob = f >> 5, rr = f & 31;
    for (int hd = lane; hd < n_hid; hd += 64) {
      const int c = hd >> 5, e = hd & 31, s = e >> 4, e16 = e & 15;
      // e16 = 8 (j >> 2) + 4 h + (j & 3)
      const int hh = (e16 >> 2) & 1, j = ((e16 >> 3) << 2) | (e16 & 3);
      Wm[(size_t)c * (MStage / 2) + (XStage / 2) + ((size_t)(2 * ob + s) * 64 + hh * 32 + rr) * 8 + j] = (__bf16)W2[(size_t)f * n_hid + hd];
    }
    if (lane == 0) b2f[f] = b2 ? b2[f] : 0.f;
  }
}

}  // namespace

// ---- host helpers of the entry points -----------------------------------------------------------------------------------
// Every pointer a kernel reads or writes with 16-byte accesses (a null optional pointer passes).
template <typename... P>
static bool aligned16(const P*... p) {
  return ((uintptr_t)0 | ... | (uintptr_t)p) % 16 == 0;
}

static bool valid_layout(int layout) { return layout == VC_ACT_ROW_MAJOR || layout == VC_ACT_FRAGMENT; }

// Grid of a persistent kernel: one workgroup per CU, fewer when there is less work.
static unsigned persistent_grid(long long work_items, int cus) { return (unsigned)(work_items < cus ? work_items : cus); }

// xs_kernel and mlp2_kernel store their results through a buffer resource with a 32-bit record count and 32-bit byte
// offsets: one launch writes less than 2 GiB of output, so a call is split into launches over consecutive row ranges, each
// the largest multiple of `tile_rows` whose [rows][n_cols] bf16 output stays below 2 GiB.  launch(first row, rows) -> status.
template <typename F>
static int for_row_ranges(long long rows, int n_cols, int tile_rows, F&& launch) {
  const int chunk = (int)(((1LL << 31) - 1) / ((long long)n_cols * 2) / tile_rows * tile_rows);
  for (long long r0 = 0; r0 < rows; r0 += chunk) {
    if (int st = launch(r0, (int)(rows - r0 < chunk ? rows - r0 : chunk))) return st;
  }
  return VC_OK;
}

// The tile form of vc_linear_bf16: the 256 x 256 tile for wide layers with enough of those tiles to occupy at least half the
// CUs (one workgroup per CU); below that the 128 x 128 tile, two workgroups per CU, fills the chip better (a single image of
// ViT-B is 18-72 large tiles).
static bool linear_takes_large_tile(int rows, int n_out, int cus) {
  return n_out % G2N == 0 && (long long)((rows + G2M - 1) / G2M) * (n_out / G2N) * 2 >= (long long)cus;
}

extern "C" {

int vc_linear_tile_rows(int rows, int n_out) {
  if (rows < 0 || n_out <= 0) return VC_ERR_INVALID_ARG;
  if (n_out % BN != 0) return VC_ERR_UNSUPPORTED;
  int cus = 0;
  if (int st = vc::cu_count(&cus)) return st;
  return linear_takes_large_tile(rows, n_out, cus) ? G2M : BM;
}

int vc_linear_bf16(const void* x, const void* weight, const void* bias, const void* residual_or_null, void* out,
                   int rows, int n_out, int k_in, int epilogue, vc_stream_t stream) {
  if (!x || !weight || !bias || !out || rows < 0 || n_out <= 0 || k_in <= 0) return VC_ERR_INVALID_ARG;
  if (epilogue != EPI_BIAS && epilogue != EPI_GELU && epilogue != EPI_RESIDUAL && epilogue != EPI_SWIGLU)
    return VC_ERR_INVALID_ARG;   // (EPI_PATCH is vc_patch_embed_bf16's alone)
  if ((epilogue == EPI_RESIDUAL) != (residual_or_null != nullptr)) return VC_ERR_INVALID_ARG;
  // EPI_SWIGLU: a tile of either form holds the gate and the value half of its output columns, 128 product columns at least
  if (n_out % (epilogue == EPI_SWIGLU ? 2 * BN : BN) != 0 || k_in % BK != 0) return VC_ERR_UNSUPPORTED;
  if (!aligned16(x, weight, bias, residual_or_null, out)) return VC_ERR_INVALID_ARG;
  if (rows == 0) return VC_OK;
  hipStream_t s = (hipStream_t)stream;
  const __bf16 *px = (const __bf16*)x, *pw = (const __bf16*)weight, *pb = (const __bf16*)bias,
               *pr = (const __bf16*)residual_or_null;
  __bf16* po = (__bf16*)out;
  int cus = 0;
  if (int st = vc::cu_count(&cus)) return st;
  if (linear_takes_large_tile(rows, n_out, cus)) {
    const int tiles_m = (rows + G2M - 1) / G2M, tiles_n = n_out / G2N;
    const long long nt = (long long)tiles_m * tiles_n;
    if (nt > 0x7fffffffLL) return VC_ERR_UNSUPPORTED;
    static vc::PerDeviceOnce configured;
    if (int st = vc::allow_dynamic_lds(configured, G256_LDS, gemm256_kernel<EPI_BIAS, false>, gemm256_kernel<EPI_GELU, false>,
                                       gemm256_kernel<EPI_RESIDUAL, false>, gemm256_kernel<EPI_SWIGLU, false>))
      return st;
    const dim3 grid(persistent_grid(nt, cus)), block(512);
    return vc::dispatch<EPI_BIAS, EPI_GELU, EPI_RESIDUAL, EPI_SWIGLU>(epilogue, [&](auto epi) {
      hipLaunchKernelGGL((gemm256_kernel<epi, false>), grid, block, (size_t)G256_LDS, s, px, pw, pb, pr, po, rows, n_out, k_in,
                         tiles_n, (int)nt, 0, 0, 0, 1, 0, 0, -1);
      return vc::check_launch();
    });
  }
  const int tiles_m = (rows + BM - 1) / BM, tiles_n = n_out / BN;
  const long long nt = (long long)tiles_m * tiles_n;
  if (nt > 0x7fffffffLL) return VC_ERR_UNSUPPORTED;
  return vc::dispatch<EPI_BIAS, EPI_GELU, EPI_RESIDUAL, EPI_SWIGLU>(epilogue, [&](auto epi) {
    hipLaunchKernelGGL(gemm_kernel<epi>, dim3((unsigned)nt), dim3(256), 0, s, px, pw, pb, pr, po, rows, n_out, k_in, tiles_n, (int)nt, 1);
    return vc::check_launch();
  });
}


int vc_conv_taps_bf16(void* x, const void* weight, const void* bias, void* out, int batch, int height, int width, int c_in,
                      int n_out, int kh, int kw, int dy0, int dx0, int out_parity, int epilogue, vc_stream_t stream) {
  if (!x || !weight || !bias || !out || batch < 0 || height <= 0 || width <= 0 || c_in <= 0 || n_out <= 0) return VC_ERR_INVALID_ARG;
  if (epilogue != EPI_BIAS && epilogue != EPI_GELU) return VC_ERR_INVALID_ARG;
  if (kh <= 0 || kw <= 0 || kh * kw > 16 || dy0 < -8 || dy0 > 8 || dx0 < -8 || dx0 > 8) return VC_ERR_INVALID_ARG;
  if (out_parity < -1 || out_parity > 3) return VC_ERR_INVALID_ARG;
  if (n_out % G2N != 0 || c_in % BK != 0) return VC_ERR_UNSUPPORTED;
  if (!aligned16(x, weight, bias, out)) return VC_ERR_INVALID_ARG;
  const long long rows = (long long)batch * height * width;
  if (rows == 0) return VC_OK;
  // per-lane offsets are 32-bit: the image batch, its zero row and the largest tap shift must stay below 4 GiB
  if ((rows + 1 + (long long)(kh + 8) * width) * c_in * 2 >= (1LL << 32) || rows > 0x7fffffffLL) return VC_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync((char*)x + (size_t)rows * c_in * 2, 0, (size_t)c_in * 2, s) != hipSuccess) return vc::fail(hipGetLastError());
  const int k_total = kh * kw * c_in;
  const int tiles_m = (int)((rows + G2M - 1) / G2M), tiles_n = n_out / G2N;
  const long long nt = (long long)tiles_m * tiles_n;
  if (nt > 0x7fffffffLL) return VC_ERR_UNSUPPORTED;
  static vc::PerDeviceOnce configured;
  if (int st = vc::allow_dynamic_lds(configured, G256_LDS, gemm256_kernel<EPI_BIAS, true>, gemm256_kernel<EPI_GELU, true>))
    return st;
  int cus = 0;
  if (int st = vc::cu_count(&cus)) return st;
  const dim3 grid(persistent_grid(nt, cus)), block(512);
  const __bf16 *px = (const __bf16*)x, *pw = (const __bf16*)weight, *pb = (const __bf16*)bias;
  __bf16* po = (__bf16*)out;
  return vc::dispatch<EPI_BIAS, EPI_GELU>(epilogue, [&](auto epi) {
    hipLaunchKernelGGL((gemm256_kernel<epi, true>), grid, block, (size_t)G256_LDS, s, px, pw, pb, (const __bf16*)nullptr, po,
                       (int)rows, n_out, k_total, tiles_n, (int)nt, height, width, c_in, kw, dy0, dx0, out_parity);
    return vc::check_launch();
  });
}


size_t vc_linear_xs_weight_bytes(int n_out, int k_in) {
  if (n_out <= 0 || k_in != XK || n_out % 32 != 0) return 0;
  return (size_t)n_out * XK * 2;
}

int vc_linear_xs_prepare(const float* weight, const float* bias_or_null, const float* ln_gamma_or_null,
                         const float* ln_beta_or_null, int n_out, int k_in, void* weight_tiled, float* bias_folded,
                         vc_stream_t stream) {
  if (!weight || !weight_tiled || !bias_folded || n_out <= 0) return VC_ERR_INVALID_ARG;
  if (k_in != XK || n_out % 32 != 0 || !xs_lds().bias_fits(n_out)) return VC_ERR_UNSUPPORTED;
  if ((ln_gamma_or_null == nullptr) != (ln_beta_or_null == nullptr)) return VC_ERR_INVALID_ARG;
  hipLaunchKernelGGL(xs_prepare_kernel, dim3((n_out + 3) / 4), dim3(256), 0, (hipStream_t)stream, weight, bias_or_null,
                     ln_gamma_or_null, ln_beta_or_null, n_out, (__bf16*)weight_tiled, bias_folded);
  return vc::check_launch();
}

size_t vc_gelu_table_bytes(void) { return (size_t)kGtBytes; }

size_t vc_act_fragment_bytes(long long rows) { return rows > 0 ? fm_bytes(rows) : 0; }

int vc_gelu_table_bf16(void* table, vc_stream_t stream) {
  if (!table || !aligned16(table)) return VC_ERR_INVALID_ARG;
  hipLaunchKernelGGL(gelu_table_kernel, dim3((kGtN * 2 + 255) / 256), dim3(256), 0, (hipStream_t)stream, (uint16_t*)table);
  return vc::check_launch();
}

int vc_linear_xs_bf16(const void* x, const void* weight_tiled, const float* bias_folded, const void* residual_or_null,
                      void* out, int rows, int n_out, int k_in, int epilogue, int fuse_layernorm, float ln_eps,
                      const void* gelu_table_or_null, vc_stream_t stream) {
  return vc_linear_xs_bf16_l(x, weight_tiled, bias_folded, residual_or_null, out, rows, n_out, k_in, epilogue, fuse_layernorm, ln_eps,
                             gelu_table_or_null, VC_ACT_ROW_MAJOR, VC_ACT_ROW_MAJOR, VC_ACT_ROW_MAJOR, stream);
}

int vc_linear_xs_bf16_l(const void* x, const void* weight_tiled, const float* bias_folded, const void* residual_or_null,
                        void* out, int rows, int n_out, int k_in, int epilogue, int fuse_layernorm, float ln_eps,
                        const void* gelu_table_or_null, int x_layout, int residual_layout, int out_layout, vc_stream_t stream) {
  if (!valid_layout(x_layout) || !valid_layout(residual_layout) || !valid_layout(out_layout)) return VC_ERR_INVALID_ARG;
  if (!residual_or_null && residual_layout != VC_ACT_ROW_MAJOR) return VC_ERR_INVALID_ARG;
  // fragment order: what the 384-wide block loop runs — LayerNorm + bias from FM x to row-major rows (qkv), and the
  // residual epilogue from FM x to an FM [rows][384] output, the residual in either layout (proj)
  const bool fm = x_layout != VC_ACT_ROW_MAJOR || residual_layout != VC_ACT_ROW_MAJOR || out_layout != VC_ACT_ROW_MAJOR;
  const bool fm_qkv = x_layout == VC_ACT_FRAGMENT && out_layout == VC_ACT_ROW_MAJOR && epilogue == EPI_BIAS && fuse_layernorm;
  const bool fm_proj = x_layout == VC_ACT_FRAGMENT && out_layout == VC_ACT_FRAGMENT && epilogue == EPI_RESIDUAL &&
                       !fuse_layernorm && n_out == XK;
  if (fm && !fm_qkv && !fm_proj) return VC_ERR_UNSUPPORTED;
  if (!x || !weight_tiled || !bias_folded || !out || rows < 0 || n_out <= 0) return VC_ERR_INVALID_ARG;
  if (epilogue < EPI_BIAS || epilogue > EPI_RESIDUAL) return VC_ERR_INVALID_ARG;
  if ((epilogue == EPI_RESIDUAL) != (residual_or_null != nullptr)) return VC_ERR_INVALID_ARG;
  if (k_in != XK || n_out % 32 != 0 || !xs_lds().bias_fits(n_out)) return VC_ERR_UNSUPPORTED;
  if (!aligned16(x, weight_tiled, bias_folded, residual_or_null, out)) return VC_ERR_INVALID_ARG;
  if (rows == 0) return VC_OK;
  int cus = 0;
  if (int st = vc::cu_count(&cus)) return st;
  const int n_nb = n_out / 32;
  hipStream_t s = (hipStream_t)stream;
  const uint8_t* pw = (const uint8_t*)weight_tiled;
  const uint16_t* gt = (const uint16_t*)gelu_table_or_null;
  if (!aligned16(gt)) return VC_ERR_INVALID_ARG;
  const bool use_gt = gt && epilogue == EPI_GELU && xs_lds().table_fits(n_out);   // (the table shares an LDS area with the bias)
  return for_row_ranges(rows, n_out, XRows, [&](long long r0, int m) {
    const int stages = (m + XRows - 1) / XRows * n_nb;
    const dim3 grid(persistent_grid(stages, cus)), block(512);
    const __bf16* px = (const __bf16*)x + (size_t)r0 * XK;
    const __bf16* pr = residual_or_null ? (const __bf16*)residual_or_null + (size_t)r0 * n_out : nullptr;
    __bf16* po = (__bf16*)out + (size_t)r0 * n_out;
    auto launch = [&](auto epi, auto ln, auto gt_on) {
      hipLaunchKernelGGL((xs_kernel<epi, ln, gt_on>), grid, block, 0, s, px, pw, bias_folded, pr, po, m, n_out, n_nb, stages,
                         ln_eps, gt);
      return vc::check_launch();
    };
    // (a row range starts at a multiple of 256 rows: the same byte offset in both layouts)
    if (fm_qkv) {
      hipLaunchKernelGGL((xs_kernel<EPI_BIAS, true, false, true, false, false>), grid, block, 0, s, px, pw, bias_folded, pr, po, m,
                         n_out, n_nb, stages, ln_eps, gt);
      return vc::check_launch();
    }
    if (fm_proj) {
      if (residual_layout == VC_ACT_FRAGMENT)
        hipLaunchKernelGGL((xs_kernel<EPI_RESIDUAL, false, false, true, true, true>), grid, block, 0, s, px, pw, bias_folded, pr, po,
                           m, n_out, n_nb, stages, ln_eps, gt);
      else
        hipLaunchKernelGGL((xs_kernel<EPI_RESIDUAL, false, false, true, false, true>), grid, block, 0, s, px, pw, bias_folded, pr, po,
                           m, n_out, n_nb, stages, ln_eps, gt);
      return vc::check_launch();
    }
    return vc::dispatch<EPI_BIAS, EPI_GELU, EPI_RESIDUAL>(epilogue, [&](auto epi) {
      return vc::dispatch<true, false>(fuse_layernorm != 0, [&](auto ln) {
        if constexpr (epi == EPI_GELU) {   // only the GELU epilogue has a table variant
          if (use_gt) return launch(epi, ln, std::true_type{});
        }
        return launch(epi, ln, std::false_type{});
      });
    });
  });
}


int vc_patch_embed_bf16(const void* patches, const void* weight, const void* bias, const void* pos_embed, void* out,
                        int n_images, int tokens, int n_out, int k_in, vc_stream_t stream) {
  if (!patches || !weight || !bias || !pos_embed || !out || n_images < 0 || tokens <= 0 || n_out <= 0 || k_in <= 0)
    return VC_ERR_INVALID_ARG;
  if (n_out % BN != 0 || k_in % BK != 0) return VC_ERR_UNSUPPORTED;
  if (!aligned16(patches, weight, bias, pos_embed, out)) return VC_ERR_INVALID_ARG;
  if (n_images == 0) return VC_OK;
  const long long rows = (long long)n_images * tokens;
  const long long nt = ((rows + BM - 1) / BM) * (n_out / BN);
  if (rows > 0x7fffffffLL || nt > 0x7fffffffLL) return VC_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(gemm_kernel<EPI_PATCH>, dim3((unsigned)nt), dim3(256), 0, (hipStream_t)stream, (const __bf16*)patches,
                     (const __bf16*)weight, (const __bf16*)bias, (const __bf16*)pos_embed, (__bf16*)out, (int)rows, n_out,
                     k_in, n_out / BN, (int)nt, tokens);
  return vc::check_launch();
}


size_t vc_mlp_weight_bytes(int n_hidden, int dim) {
  if (dim != XK || n_hidden <= 0 || n_hidden % 32 != 0 || n_hidden > mlp_lds().max_hidden()) return 0;
  return (size_t)(n_hidden / 32) * MStage;
}

int vc_mlp_prepare(const float* w1, const float* b1_or_null, const float* ln_gamma_or_null, const float* ln_beta_or_null,
                   const float* w2, const float* b2_or_null, int n_hidden, int dim, void* weights_tiled, float* b1_folded,
                   float* b2_out, vc_stream_t stream) {
  if (!w1 || !w2 || !weights_tiled || !b1_folded || !b2_out) return VC_ERR_INVALID_ARG;
  if (vc_mlp_weight_bytes(n_hidden, dim) == 0) return VC_ERR_UNSUPPORTED;
  if ((ln_gamma_or_null == nullptr) != (ln_beta_or_null == nullptr)) return VC_ERR_INVALID_ARG;
  hipLaunchKernelGGL(mlp_prepare_kernel, dim3((n_hidden + XK + 3) / 4), dim3(256), 0, (hipStream_t)stream, w1, b1_or_null,
                     ln_gamma_or_null, ln_beta_or_null, w2, b2_or_null, n_hidden, (__bf16*)weights_tiled, b1_folded, b2_out);
  return vc::check_launch();
}

int vc_mlp_bf16_l(void* x_inout, void* out_or_null, const void* weights_tiled, const float* b1_folded, const float* b2,
                  const void* gelu_table, int rows, int n_hidden, int dim, float ln_eps, int x_layout, int out_layout,
                  vc_stream_t stream) {
  if (!x_inout || !weights_tiled || !b1_folded || !b2 || !gelu_table || rows < 0) return VC_ERR_INVALID_ARG;
  if (!valid_layout(x_layout) || !valid_layout(out_layout)) return VC_ERR_INVALID_ARG;
  // in place in either layout, or fragment order in and row-major rows out into a buffer of their own
  const bool separate = x_layout != out_layout;
  if (separate && (x_layout != VC_ACT_FRAGMENT || !out_or_null || out_or_null == x_inout)) return VC_ERR_INVALID_ARG;
  if (!separate && out_or_null && out_or_null != x_inout) return VC_ERR_INVALID_ARG;
  if (vc_mlp_weight_bytes(n_hidden, dim) == 0) return VC_ERR_UNSUPPORTED;
  if (!aligned16(x_inout, out_or_null, weights_tiled, b1_folded, b2, gelu_table)) return VC_ERR_INVALID_ARG;
  if (rows == 0) return VC_OK;
  int cus = 0;
  if (int st = vc::cu_count(&cus)) return st;
  // (a row range starts at a multiple of 128 rows: the same byte offset in both layouts)
  return for_row_ranges(rows, XK, 128, [&](long long r0, int m) {
    const int n_tiles = (m + 127) / 128;
    __bf16* po = separate ? (__bf16*)out_or_null + (size_t)r0 * XK : nullptr;
    auto launch = [&](auto xf, auto of) {
      hipLaunchKernelGGL((mlp2_kernel<xf, of>), dim3(persistent_grid(n_tiles, cus)), dim3(512), 0, (hipStream_t)stream,
                         (__bf16*)x_inout + (size_t)r0 * XK, (const uint8_t*)weights_tiled, b1_folded, b2, m, n_hidden / 32, n_tiles,
                         ln_eps, (const uint16_t*)gelu_table, po);
      return vc::check_launch();
    };
    if (x_layout == VC_ACT_ROW_MAJOR) return launch(std::false_type{}, std::false_type{});
    if (separate) return launch(std::true_type{}, std::false_type{});
    return launch(std::true_type{}, std::true_type{});
  });
}

int vc_mlp_bf16(void* x_inout, const void* weights_tiled, const float* b1_folded, const float* b2, const void* gelu_table,
                int rows, int n_hidden, int dim, float ln_eps, vc_stream_t stream) {
  return vc_mlp_bf16_l(x_inout, nullptr, weights_tiled, b1_folded, b2, gelu_table, rows, n_hidden, dim, ln_eps, VC_ACT_ROW_MAJOR,
                       VC_ACT_ROW_MAJOR, stream);
}

}  // extern "C"
