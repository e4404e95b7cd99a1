// Classical keypoint detectors for the hybrid extractor: FAST-9/16 and Shi-Tomasi "good features to track" (GFTT),
// batched over same-size BGR images.  Specification: tests/util_detect.py (a numpy restatement of OpenCV's algorithms;
// parity with OpenCV itself is unpinned).  Everything up to GFTT's eigenvalue is integer arithmetic, the
// eigenvalue is float32 in a fixed order of operations (the library is built with -ffp-contract=off), so both detectors
// equal the specification exactly.
#include "common.h"
#include "device.h"

namespace {

constexpr int kTileW = 64, kTileH = 16, kThreads = 256;   // output pixels of one workgroup of the stencil kernels
constexpr int kSelThreads = 1024;                          // one workgroup per image in the selection kernels

// OpenCV's fixed-point BGR2GRAY
__device__ __forceinline__ int grey_u8(const uint8_t* px) {
  return (1868 * (int)px[0] + 9617 * (int)px[1] + 4899 * (int)px[2] + 8192) >> 14;
}

__device__ __forceinline__ int reflect101(int v, int n) { return v < 0 ? -v : (v >= n ? 2 * n - 2 - v : v); }

// Exclusive prefix sum of `v` over the workgroup (kSelThreads threads, every thread calls); `total` = the sum.
// `part` is LDS scratch of kSelThreads / 64 + 1 ints.  Ends with a barrier, so `part` may be reused at once.
__device__ __forceinline__ int block_exclusive_scan(int v, int* part, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(inc, d, 64);
    if (lane >= d) inc += o;
  }
  if (lane == 63) part[wave] = inc;
  __syncthreads();
  int before = 0, all = 0;
  for (int i = 0; i < kSelThreads / 64; ++i) {
    const int p = part[i];
    before += i < wave ? p : 0;
    all += p;
  }
  total = all;
  __syncthreads();
  return before + inc - v;
}

// ---- FAST ---------------------------------------------------------------------------------------------------------
// circle of radius 3, (dx, dy) in the order of the specification
constexpr int kCircleX[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
constexpr int kCircleY[16] = {3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3};

// max over the 16 arcs of 9 contiguous circle pixels of max(min(c - p), min(p - c)); min / max over 9 by doubling
__device__ __forceinline__ int fast_arc_score(const int (&d)[16]) {
  int lo2[16], hi2[16], lo4[16], hi4[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    lo2[k] = min(d[k], d[(k + 1) & 15]);
    hi2[k] = max(d[k], d[(k + 1) & 15]);
  }
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    lo4[k] = min(lo2[k], lo2[(k + 2) & 15]);
    hi4[k] = max(hi2[k], hi2[(k + 2) & 15]);
  }
  int best = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int lo9 = min(min(lo4[k], lo4[(k + 4) & 15]), d[(k + 8) & 15]);
    const int hi9 = max(max(hi4[k], hi4[(k + 4) & 15]), d[(k + 8) & 15]);
    best = max(best, max(lo9, -hi9));
  }
  return best;
}

// grid (ceil(w / 64), ceil(h / 16), n).  Grey tile with a halo of 4 in LDS, scores with a halo of 1 in LDS, then the
// 8-neighbour suppression: nms [n][stride] uint8 = the score of a kept corner, else 0; hist [n][256] += kept scores.
__global__ __launch_bounds__(kThreads) void fast_score_kernel(const uint8_t* __restrict__ bgr, int h, int w, int threshold,
                                                              size_t stride, uint8_t* __restrict__ nms,
                                                              int32_t* __restrict__ hist) {
  constexpr int GW = kTileW + 8, GH = kTileH + 8, SW = kTileW + 2, SH = kTileH + 2;
  __shared__ uint8_t g[GH][GW];
  __shared__ uint8_t s[SH][SW];
  __shared__ int32_t lhist[256];
  const int b = blockIdx.z, x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;
  const uint8_t* img = bgr + (size_t)b * h * w * 3;
  lhist[threadIdx.x] = 0;
  for (int i = threadIdx.x; i < GH * GW; i += kThreads) {
    const int ty = i / GW, tx = i % GW, y = y0 - 4 + ty, x = x0 - 4 + tx;
    g[ty][tx] = (y >= 0 && y < h && x >= 0 && x < w) ? (uint8_t)grey_u8(img + ((size_t)y * w + x) * 3) : (uint8_t)0;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < SH * SW; i += kThreads) {
    const int ty = i / SW, tx = i % SW, y = y0 - 1 + ty, x = x0 - 1 + tx;
    int score = 0;
    if (y >= 3 && y < h - 3 && x >= 3 && x < w - 3) {     // closer than 3 to the edge: never a corner
      const int p = g[ty + 3][tx + 3];
      int d[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) d[k] = (int)g[ty + 3 + kCircleY[k]][tx + 3 + kCircleX[k]] - p;
      score = fast_arc_score(d);
      if (score <= threshold) score = 0;
    }
    s[ty][tx] = (uint8_t)score;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kTileH * kTileW; i += kThreads) {
    const int ty = i / kTileW, tx = i % kTileW, y = y0 + ty, x = x0 + tx;
    if (y >= h || x >= w) continue;
    const int c = s[ty + 1][tx + 1];
    const int nb = max(max(max(s[ty][tx], s[ty][tx + 1]), max(s[ty][tx + 2], s[ty + 1][tx])),
                       max(max(s[ty + 1][tx + 2], s[ty + 2][tx]), max(s[ty + 2][tx + 1], s[ty + 2][tx + 2])));
    const int keep = (c > 0 && c > nb) ? c : 0;
    nms[(size_t)b * stride + (size_t)y * w + x] = (uint8_t)keep;
    if (keep) atomicAdd(&lhist[keep], 1);
  }
  __syncthreads();
  if (lhist[threadIdx.x]) atomicAdd(&hist[(size_t)b * 256 + threadIdx.x], lhist[threadIdx.x]);
}

// grid (n), 1024 threads.  The cut: the largest score c with #(S >= c) > max_keypoints keeps every S > c and the first
// max_keypoints - #(S > c) of S == c in raster order; then an ordered compaction of the map, 16 pixels per thread and step.
__global__ __launch_bounds__(kSelThreads) void fast_select_kernel(const uint8_t* __restrict__ nms, int h, int w, size_t stride,
                                                                  const int32_t* __restrict__ hist, int max_keypoints,
                                                                  float* __restrict__ out_xy, int32_t* __restrict__ out_count,
                                                                  int32_t* __restrict__ out_total) {
  __shared__ int part[kSelThreads / 64 + 1];
  __shared__ int cut_s, eq_allow_s, total_s;
  const int b = blockIdx.x, t = threadIdx.x;
  const uint8_t* m = nms + (size_t)b * stride;
  if (t == 0) {
    int above = 0, cut = 0, allow = 0;    // cut 0: everything is kept (scores of kept corners are >= 1)
    for (int v = 255; v >= 1; --v) {
      const int c = hist[(size_t)b * 256 + v];
      if (cut == 0 && above + c > max_keypoints) {
        cut = v;
        allow = max_keypoints - above;
      }
      above += c;
    }
    cut_s = cut;
    eq_allow_s = allow;
    total_s = above;
  }
  __syncthreads();
  const int cut = cut_s, eq_allow = eq_allow_s;
  const size_t npix = (size_t)h * w;
  float* out = out_xy + (size_t)b * max_keypoints * 2;
  int base = 0, eq_base = 0;              // kept points / points equal to the cut before this step, in raster order
  for (size_t start = 0; start < npix; start += (size_t)kSelThreads * 16) {
    const size_t i0 = start + (size_t)t * 16;
    uint8_t v[16];
    if (i0 + 16 <= npix) {
      const uint4 q = *reinterpret_cast<const uint4*>(m + i0);     // stride and i0 are multiples of 16
      const uint32_t qq[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int k = 0; k < 16; ++k) v[k] = (uint8_t)(qq[k >> 2] >> (8 * (k & 3)));
    } else {
#pragma unroll
      for (int k = 0; k < 16; ++k) v[k] = i0 + k < npix ? m[i0 + k] : (uint8_t)0;
    }
    int n_gt = 0, n_eq = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      n_gt += (v[k] > cut) ? 1 : 0;
      n_eq += (cut > 0 && v[k] == cut) ? 1 : 0;
    }
    int tot;
    const int packed = block_exclusive_scan(n_gt | (n_eq << 16), part, tot);   // both counts stay below 2^15 per step
    int gt_before = base + (packed & 0xffff), eq_before = eq_base + (packed >> 16);
    if (n_gt | n_eq) {
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const bool gt = v[k] > cut, eq = cut > 0 && v[k] == cut;
        if (gt || (eq && eq_before < eq_allow)) {
          const int pos = gt_before + min(eq_before, eq_allow);
          const size_t i = i0 + k;
          out[(size_t)pos * 2] = (float)(int)(i % w);
          out[(size_t)pos * 2 + 1] = (float)(int)(i / w);
        }
        gt_before += gt ? 1 : 0;
        eq_before += eq ? 1 : 0;
      }
    }
    base += tot & 0xffff;
    eq_base += tot >> 16;
  }
  const int kept = base + min(eq_base, eq_allow);
  for (int i = kept + t; i < max_keypoints; i += kSelThreads) {
    out[(size_t)i * 2] = 0.f;
    out[(size_t)i * 2 + 1] = 0.f;
  }
  if (t == 0) {
    out_count[b] = kept;
    out_total[b] = total_s;
  }
}

// ---- GFTT ---------------------------------------------------------------------------------------------------------
// order-preserving map float -> uint32 (for an integer atomicMax over floats of either sign)
__device__ __forceinline__ uint32_t float_key(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_float(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// grid (ceil(w / 64), ceil(h / 16), n).  Grey tile with a halo of 4 (reflect-101) in LDS; Sobel products gx^2, gx gy,
// gy^2 at the reflected positions with a halo of 3; 7x7 box sums, rows then columns, int32; lambda [n][h][w] float32 =
// the smaller eigenvalue; max_key [n] = atomicMax of float_key(lambda).
template <int R>
__global__ __launch_bounds__(kThreads) void gftt_lambda_kernel(const uint8_t* __restrict__ bgr, int h, int w,
                                                               float* __restrict__ lambda, uint32_t* __restrict__ max_key) {
  constexpr int HALO = R + 1, GW = kTileW + 2 * HALO, GH = kTileH + 2 * HALO, PW = kTileW + 2 * R, PH = kTileH + 2 * R;
  __shared__ uint8_t g[GH][GW];
  __shared__ int32_t pa[PH][PW], pb[PH][PW], pc[PH][PW];
  __shared__ int32_t ra[PH][kTileW], rb[PH][kTileW], rc[PH][kTileW];
  __shared__ uint32_t wmax[kThreads / 64];
  const int b = blockIdx.z, x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;
  const uint8_t* img = bgr + (size_t)b * h * w * 3;
  // virtual coordinates [x0 - HALO, x0 + 64 + HALO): inside [-HALO, w + HALO) they reflect once (w, h >= 8 > HALO);
  // beyond (a tile that overhangs the image) they are clamped and never used
  for (int i = threadIdx.x; i < GH * GW; i += kThreads) {
    const int ty = i / GW, tx = i % GW;
    const int y = min(max(reflect101(y0 - HALO + ty, h), 0), h - 1), x = min(max(reflect101(x0 - HALO + tx, w), 0), w - 1);
    g[ty][tx] = (uint8_t)grey_u8(img + ((size_t)y * w + x) * 3);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < PH * PW; i += kThreads) {
    const int ty = i / PW, tx = i % PW, vy = y0 - R + ty, vx = x0 - R + tx;
    int a = 0, bb = 0, c = 0;
    if (vy < h + R && vx < w + R) {
      // the product image is extended by reflect-101: the gradient is taken at the reflected position
      const int ry = reflect101(vy, h), rx = reflect101(vx, w);
      const int ym = reflect101(ry - 1, h) - (y0 - HALO), yc = ry - (y0 - HALO), yp = reflect101(ry + 1, h) - (y0 - HALO);
      const int xm = reflect101(rx - 1, w) - (x0 - HALO), xc = rx - (x0 - HALO), xp = reflect101(rx + 1, w) - (x0 - HALO);
      const int gx = ((int)g[ym][xp] + 2 * (int)g[yc][xp] + (int)g[yp][xp]) - ((int)g[ym][xm] + 2 * (int)g[yc][xm] + (int)g[yp][xm]);
      const int gy = ((int)g[yp][xm] + 2 * (int)g[yp][xc] + (int)g[yp][xp]) - ((int)g[ym][xm] + 2 * (int)g[ym][xc] + (int)g[ym][xp]);
      a = gx * gx;
      bb = gx * gy;
      c = gy * gy;
    }
    pa[ty][tx] = a;
    pb[ty][tx] = bb;
    pc[ty][tx] = c;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < PH * kTileW; i += kThreads) {
    const int ty = i / kTileW, tx = i % kTileW;
    int a = 0, bb = 0, c = 0;
#pragma unroll
    for (int k = 0; k <= 2 * R; ++k) {
      a += pa[ty][tx + k];
      bb += pb[ty][tx + k];
      c += pc[ty][tx + k];
    }
    ra[ty][tx] = a;
    rb[ty][tx] = bb;
    rc[ty][tx] = c;
  }
  __syncthreads();
  uint32_t best = 0;   // below the key of every float
  for (int i = threadIdx.x; i < kTileH * kTileW; i += kThreads) {
    const int ty = i / kTileW, tx = i % kTileW, y = y0 + ty, x = x0 + tx;
    if (y >= h || x >= w) continue;
    int a = 0, bb = 0, c = 0;
#pragma unroll
    for (int k = 0; k <= 2 * R; ++k) {
      a += ra[ty + k][tx];
      bb += rb[ty + k][tx];
      c += rc[ty + k][tx];
    }
    const float fa = (float)a, fb = (float)bb, fc = (float)c;
    const float ha = 0.5f * fa, hc = 0.5f * fc, dm = ha - hc;
    const float lam = (ha + hc) - sqrtf(dm * dm + fb * fb);
    lambda[((size_t)b * h + y) * w + x] = lam;
    best = max(best, float_key(lam));
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) best = max(best, (uint32_t)__shfl_xor((int)best, d, 64));
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0) atomicMax(&max_key[b], max(max(wmax[0], wmax[1]), max(wmax[2], wmax[3])));
}

// grid (ceil(h * w / 256), n).  Thresholded lambda v = lambda < quality * max ? 0 : lambda; a candidate has v != 0 and
// v >= the v of its 8 neighbours, outermost rows and columns excluded.  slot [n][h][w] int32 = 0 everywhere (the
// selection kernel writes the ranks of the candidates into it); candidates appended as (lambda bits, y * w + x) in no
// particular order, out_candidates [n] counts all of them, only the first cand_cap are stored.
__global__ __launch_bounds__(kThreads) void gftt_candidates_kernel(const float* __restrict__ lambda, int h, int w,
                                                                   const uint32_t* __restrict__ max_key, float quality,
                                                                   int32_t* __restrict__ slot, uint2* __restrict__ cand,
                                                                   int cand_cap, int32_t* __restrict__ out_candidates) {
  const int b = blockIdx.y;
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= (size_t)h * w) return;
  slot[(size_t)b * h * w + i] = 0;
  const int y = (int)(i / w), x = (int)(i % w);
  const float mx = key_float(max_key[b]);
  if (!(mx > 0.f) || y < 1 || y > h - 2 || x < 1 || x > w - 2) return;
  const float thr = quality * mx;
  const float* L = lambda + (size_t)b * h * w;
  const float c = L[i];
  if (c < thr || c == 0.f) return;
  bool is_max = true;
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      float v = L[(size_t)(y + dy) * w + (x + dx)];
      v = v < thr ? 0.f : v;
      is_max = is_max && c >= v;
    }
  if (!is_max) return;
  const int pos = atomicAdd(&out_candidates[b], 1);
  if (pos < cand_cap) cand[(size_t)b * cand_cap + pos] = make_uint2(__float_as_uint(c), (uint32_t)i);
}

// grid (n), 1024 threads, dynamic LDS: P keys of 8 bytes + P state bytes, P = the power of two >= cand_cap.
// Rank: bitonic sort, lambda descending, the later raster position first among equals.  Greedy minimum-distance pass
// in parallel rounds with the result of the sequential pass: an undecided candidate is rejected when an accepted one
// lies at squared distance < min_dist^2, and accepted when no higher-ranked undecided one does; the candidate of the
// highest rank among the undecided is decided in every round.  Neighbours are found through slot (rank + 1 at the
// pixel of a candidate).  The first max_corners accepted in rank order are written.
__global__ __launch_bounds__(kSelThreads) void gftt_select_kernel(const uint2* __restrict__ cand, int cand_cap, int P,
                                                                  const int32_t* __restrict__ n_candidates, int h, int w,
                                                                  int min_dist, int max_corners, int32_t* __restrict__ slot,
                                                                  float* __restrict__ out_xy, int32_t* __restrict__ out_count) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  __shared__ int part[kSelThreads / 64 + 1];
  __shared__ int undecided_s;
  unsigned long long* key = reinterpret_cast<unsigned long long*>(lds);
  uint8_t* state = lds + (size_t)P * 8;     // bits 0-1: this round, bits 2-3: next round; 0 undecided, 1 accepted, 2 rejected
  const int b = blockIdx.x, t = threadIdx.x;
  float* out = out_xy + (size_t)b * max_corners * 2;
  const int found = n_candidates[b];
  const int n = found > cand_cap ? 0 : found;     // overflow: the caller sees n_candidates > cand_cap and calls again
  for (int i = t; i < P; i += kSelThreads) {
    unsigned long long k = 0;                      // padding sorts behind every candidate (lambda > 0)
    if (i < n) {
      const uint2 c = cand[(size_t)b * cand_cap + i];
      k = ((unsigned long long)c.x << 32) | c.y;
    }
    key[i] = k;
    state[i] = 0;
  }
  __syncthreads();
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = t; i < P / 2; i += kSelThreads) {
        const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
        const unsigned long long a = key[lo], c = key[hi];
        const bool descending = (lo & size) == 0;
        if (descending ? a < c : a > c) {
          key[lo] = c;
          key[hi] = a;
        }
      }
      __syncthreads();
    }
  }
  int32_t* S = slot + (size_t)b * h * w;
  for (int i = t; i < n; i += kSelThreads) S[(uint32_t)key[i]] = i + 1;
  __syncthreads();   // one workgroup: its own global stores are visible to it after the barrier
  const int r = min_dist - 1, d2 = min_dist * min_dist;   // squared distance < min_dist^2 needs |dx|, |dy| <= min_dist - 1
  for (;;) {
    if (t == 0) undecided_s = 0;
    __syncthreads();
    bool any = false;
    for (int i = t; i < n; i += kSelThreads) {
      if ((state[i] & 3) != 0) continue;
      const int idx = (int)(uint32_t)key[i], y = idx / w, x = idx % w;
      bool accepted_near = false, undecided_near = false;
      for (int yy = max(y - r, 0); yy <= min(y + r, h - 1); ++yy)
        for (int xx = max(x - r, 0); xx <= min(x + r, w - 1); ++xx) {
          const int j = S[(size_t)yy * w + xx] - 1;
          if (j < 0 || j >= i || (yy - y) * (yy - y) + (xx - x) * (xx - x) >= d2) continue;
          const int sj = state[j] & 3;
          accepted_near = accepted_near || sj == 1;
          undecided_near = undecided_near || sj == 0;
        }
      const int next = accepted_near ? 2 : (undecided_near ? 0 : 1);
      state[i] = (uint8_t)(next << 2);      // own byte only; the others read bits 0-1, which stay 0 until the barrier
      any = any || next == 0;
    }
    if (any) undecided_s = 1;
    __syncthreads();
    for (int i = t; i < n; i += kSelThreads) {
      const int s = state[i];
      if ((s & 3) == 0) state[i] = (uint8_t)((s >> 2) | (s & 12));
    }
    const bool more = undecided_s != 0;
    __syncthreads();
    if (!more) break;
  }
  int base = 0;
  for (int start = 0; start < n && base < max_corners; start += kSelThreads) {
    const int i = start + t;
    const int acc = (i < n && (state[i] & 3) == 1) ? 1 : 0;
    int tot;
    const int pos = base + block_exclusive_scan(acc, part, tot);
    if (acc && pos < max_corners) {
      const int idx = (int)(uint32_t)key[i];
      out[(size_t)pos * 2] = (float)(idx % w);
      out[(size_t)pos * 2 + 1] = (float)(idx / w);
    }
    base += tot;
  }
  const int kept = min(base, max_corners);
  for (int i = kept + t; i < max_corners; i += kSelThreads) {
    out[(size_t)i * 2] = 0.f;
    out[(size_t)i * 2 + 1] = 0.f;
  }
  if (t == 0) out_count[b] = kept;
}

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
inline size_t fast_stride(int h, int w) { return ((size_t)h * w + 15) & ~(size_t)15; }
inline int pow2_at_least(int v) {
  int p = 2;
  while (p < v) p <<= 1;
  return p;
}
inline bool size_ok(int n, int h, int w) { return n <= 65535 && (long long)h * w <= 0x7fffffff / 4; }

}  // namespace

extern "C" {

size_t vc_detect_fast_workspace_bytes(int n_images, int h, int w) {
  if (n_images <= 0 || h < VC_DETECT_MIN_SIZE || w < VC_DETECT_MIN_SIZE || !size_ok(n_images, h, w)) return 0;
  return align256((size_t)n_images * 256 * sizeof(int32_t)) + (size_t)n_images * fast_stride(h, w);
}

int vc_detect_fast(const uint8_t* images_bgr, int n_images, int h, int w, int threshold, int max_keypoints, void* workspace,
                   size_t workspace_bytes, float* out_xy, int32_t* out_count, int32_t* out_total, vc_stream_t stream) {
  if (!images_bgr || !workspace || !out_xy || !out_count || !out_total || n_images <= 0 || h <= 0 || w <= 0 ||
      threshold < 0 || threshold > 254 || max_keypoints <= 0 || ((uintptr_t)workspace & 15))
    return VC_ERR_INVALID_ARG;
  if (h < VC_DETECT_MIN_SIZE || w < VC_DETECT_MIN_SIZE || !size_ok(n_images, h, w) || (h + kTileH - 1) / kTileH > 65535)
    return VC_ERR_UNSUPPORTED;
  if (workspace_bytes < vc_detect_fast_workspace_bytes(n_images, h, w)) return VC_ERR_WORKSPACE;
  const size_t hist_bytes = (size_t)n_images * 256 * sizeof(int32_t), stride = fast_stride(h, w);
  int32_t* hist = (int32_t*)workspace;
  uint8_t* nms = (uint8_t*)workspace + align256(hist_bytes);
  const hipError_t e = hipMemsetAsync(hist, 0, hist_bytes, (hipStream_t)stream);
  if (e != hipSuccess) return vc::fail(e);
  hipLaunchKernelGGL(fast_score_kernel, dim3((w + kTileW - 1) / kTileW, (h + kTileH - 1) / kTileH, n_images), dim3(kThreads), 0,
                     (hipStream_t)stream, images_bgr, h, w, threshold, stride, nms, hist);
  if (int st = vc::check_launch()) return st;
  hipLaunchKernelGGL(fast_select_kernel, dim3(n_images), dim3(kSelThreads), 0, (hipStream_t)stream, (const uint8_t*)nms, h, w,
                     stride, (const int32_t*)hist, max_keypoints, out_xy, out_count, out_total);
  return vc::check_launch();
}

size_t vc_detect_gftt_workspace_bytes(int n_images, int h, int w, int cand_cap) {
  if (n_images <= 0 || h < VC_DETECT_MIN_SIZE || w < VC_DETECT_MIN_SIZE || !size_ok(n_images, h, w) || cand_cap <= 0 ||
      cand_cap > VC_DETECT_GFTT_MAX_CANDIDATES)
    return 0;
  const size_t px = (size_t)n_images * h * w;
  return align256((size_t)n_images * sizeof(uint32_t)) + align256(px * sizeof(float)) + align256(px * sizeof(int32_t)) +
         (size_t)n_images * cand_cap * sizeof(uint2);
}

int vc_detect_gftt(const uint8_t* images_bgr, int n_images, int h, int w, float quality_level, int min_distance,
                   int block_size, int max_corners, int cand_cap, void* workspace, size_t workspace_bytes, float* out_xy,
                   int32_t* out_count, int32_t* out_candidates, vc_stream_t stream) {
  if (!images_bgr || !workspace || !out_xy || !out_count || !out_candidates || n_images <= 0 || h <= 0 || w <= 0 ||
      !(quality_level > 0.f && quality_level <= 1.f) || min_distance < 1 || max_corners <= 0 || cand_cap <= 0 ||
      ((uintptr_t)workspace & 15))
    return VC_ERR_INVALID_ARG;
  if (h < VC_DETECT_MIN_SIZE || w < VC_DETECT_MIN_SIZE || !size_ok(n_images, h, w) || (h + kTileH - 1) / kTileH > 65535 ||
      cand_cap > VC_DETECT_GFTT_MAX_CANDIDATES || min_distance > 64)
    return VC_ERR_UNSUPPORTED;
  if (workspace_bytes < vc_detect_gftt_workspace_bytes(n_images, h, w, cand_cap)) return VC_ERR_WORKSPACE;
  const size_t px = (size_t)n_images * h * w;
  uint8_t* p = (uint8_t*)workspace;
  uint32_t* max_key = (uint32_t*)p;
  p += align256((size_t)n_images * sizeof(uint32_t));
  float* lambda = (float*)p;
  p += align256(px * sizeof(float));
  int32_t* slot = (int32_t*)p;
  p += align256(px * sizeof(int32_t));
  uint2* cand = (uint2*)p;
  hipError_t e = hipMemsetAsync(max_key, 0, (size_t)n_images * sizeof(uint32_t), (hipStream_t)stream);
  if (e == hipSuccess) e = hipMemsetAsync(out_candidates, 0, (size_t)n_images * sizeof(int32_t), (hipStream_t)stream);
  if (e != hipSuccess) return vc::fail(e);
  const dim3 tiles((w + kTileW - 1) / kTileW, (h + kTileH - 1) / kTileH, n_images);
  // the window (block_size) is a template argument: only 3, 5 and 7 (OpenCV's usual values) are built
  const int st = vc::dispatch<1, 2, 3>(block_size % 2 == 1 ? block_size / 2 : -1, [&](auto R) {
    hipLaunchKernelGGL(gftt_lambda_kernel<decltype(R)::value>, tiles, dim3(kThreads), 0, (hipStream_t)stream, images_bgr, h, w, lambda,
                       max_key);
    return vc::check_launch();
  });
  if (st) return st;
  hipLaunchKernelGGL(gftt_candidates_kernel, dim3((unsigned)(((size_t)h * w + kThreads - 1) / kThreads), n_images),
                     dim3(kThreads), 0, (hipStream_t)stream, (const float*)lambda, h, w, (const uint32_t*)max_key,
                     quality_level, slot, cand, cand_cap, out_candidates);
  if (int st2 = vc::check_launch()) return st2;
  const int P = pow2_at_least(cand_cap);
  static vc::PerDeviceOnce configured;
  if (int st3 = vc::allow_dynamic_lds(configured, VC_DETECT_GFTT_MAX_CANDIDATES * 9, gftt_select_kernel)) return st3;
  hipLaunchKernelGGL(gftt_select_kernel, dim3(n_images), dim3(kSelThreads), (size_t)P * 9, (hipStream_t)stream,
                     (const uint2*)cand, cand_cap, P, (const int32_t*)out_candidates, h, w, min_distance, max_corners, slot,
                     out_xy, out_count);
  return vc::check_launch();
}

}  // extern "C"
