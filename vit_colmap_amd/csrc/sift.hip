// SIFT with COLMAP's default extraction options, computed as VLFeat's vl_sift does (gfx950): grey conversion and
// 2x upsampling, separable Gaussian levels, DoG, 26-neighbour extrema with Newton refinement, 36-bin orientation
// histograms and the 4x4x8 descriptor with COLMAP's normalisation and quantiser.  Replaces the pycolmap call of the
// reference's ColmapSiftExtractor (vit_colmap/features/colmap_sift_extractor.py).  Specification: tests/util_sift.py.
//
// Pyramid, DoG and detection are float32 in exactly the oracle's operation order (fixed tap order, the library is
// built with -ffp-contract=off) and agree with it bit for bit.  Orientation and descriptor call expf / atan2f /
// sqrtf / cosf / sinf and sum in another order than numpy; they agree within tolerance.  Nothing here uses float
// atomics: keypoints are compacted by a counted two-pass scan, histograms are per-lane in LDS and reduced in a
// fixed order, so results are bit-identical run to run and for an image alone or inside a batch.
//
// Layouts: images [B][h][w]; the levels of one octave [L][B][h][w] (level-major, so one level of the whole batch is
// one contiguous block); keypoint records [B][cap][8] = x, y, s, sigma (octave units), DoG level j, y0, x0 (the
// unrefined extremum), 0.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "../../include/vitcolmap_hip.h"
#include "common.h"

namespace {

constexpr int kMaxRadius = VC_SIFT_MAX_RADIUS;
constexpr int kRowTile = 256;     // outputs per block of the row pass
constexpr int kColTile = 64;      // output rows per block of the column pass (64 columns wide)
constexpr float kTwoPi = 6.28318530717958647692f;
constexpr float kEps = 1.1920928955078125e-07f;   // FLT_EPSILON: VLFeat's guard in the descriptor normalisation
constexpr float kTiny = 1.17549435e-38f;          // FLT_MIN

struct Taps {
  float t[2 * kMaxRadius + 1];
};

// ---- grey, resize, upsample --------------------------------------------------------------------------------------
__device__ inline float grey_u8(const uint8_t* img, int w, int y, int x) {
  const uint8_t* p = img + ((size_t)y * w + x) * 3;
  const float b = p[0], g = p[1], r = p[2];
  return floorf(0.2126f * r + 0.7152f * g + 0.0722f * b + 0.5f);
}

struct Lin {
  int i0, i1;
  float a;
};
__device__ inline Lin lin_coef(int d, int n_out, int n_in) {
  float f = (float)(((double)d + 0.5) * ((double)n_in / (double)n_out) - 0.5);
  f = fminf(fmaxf(f, 0.f), (float)(n_in - 1));
  Lin c;
  c.i0 = (int)floorf(f);
  c.i1 = min(c.i0 + 1, n_in - 1);
  c.a = f - (float)c.i0;
  return c;
}

// working-size grey value at (y, x): bilinear on the uint8 grey image when resized, / 255
__device__ inline float base_at(const uint8_t* img, int h, int w, int oh, int ow, int y, int x) {
  if (oh == h && ow == w) return grey_u8(img, w, y, x) / 255.f;
  const Lin cx = lin_coef(x, ow, w), cy = lin_coef(y, oh, h);
  const float top = grey_u8(img, w, cy.i0, cx.i0) * (1.f - cx.a) + grey_u8(img, w, cy.i0, cx.i1) * cx.a;
  const float bot = grey_u8(img, w, cy.i1, cx.i0) * (1.f - cx.a) + grey_u8(img, w, cy.i1, cx.i1) * cx.a;
  return (top * (1.f - cy.a) + bot * cy.a) / 255.f;
}

// VLFeat's upsampling along x of row y at output column X
__device__ inline float up_row(const uint8_t* img, int h, int w, int oh, int ow, int y, int X) {
  const int x = X >> 1;
  if ((X & 1) == 0 || x == ow - 1) return base_at(img, h, w, oh, ow, y, x);
  return 0.5f * (base_at(img, h, w, oh, ow, y, x) + base_at(img, h, w, oh, ow, y, x + 1));
}

__global__ __launch_bounds__(256) void grey_kernel(const uint8_t* __restrict__ bgr, int h, int w, int oh, int ow,
                                                   int upsample, float* __restrict__ out) {
  const int b = blockIdx.z, Y = blockIdx.y;
  const int X = blockIdx.x * blockDim.x + threadIdx.x;
  const int W = upsample ? 2 * ow : ow, H = upsample ? 2 * oh : oh;
  if (X >= W) return;
  const uint8_t* img = bgr + (size_t)b * h * w * 3;
  float v;
  if (!upsample) {
    v = base_at(img, h, w, oh, ow, Y, X);
  } else {
    const int y = Y >> 1;
    if ((Y & 1) == 0 || y == oh - 1) v = up_row(img, h, w, oh, ow, y, X);
    else v = 0.5f * (up_row(img, h, w, oh, ow, y, X) + up_row(img, h, w, oh, ow, y + 1, X));
  }
  out[((size_t)b * H + Y) * W + X] = v;
}

// ---- separable Gaussian: rows, then columns; acc = acc + t[k] * x[i + k - r], edge replicate ----------------------
__global__ __launch_bounds__(256) void blur_rows_kernel(const float* __restrict__ src, float* __restrict__ dst, int h,
                                                        int w, Taps taps, int r) {
  __shared__ float tile[kRowTile + 2 * kMaxRadius];
  const int b = blockIdx.z, y = blockIdx.y, x0 = blockIdx.x * kRowTile;
  const float* row = src + ((size_t)b * h + y) * w;
  for (int i = threadIdx.x; i < kRowTile + 2 * r; i += blockDim.x) tile[i] = row[min(max(x0 + i - r, 0), w - 1)];
  __syncthreads();
  const int x = x0 + threadIdx.x;
  if (x >= w) return;
  float acc = 0.f;
  for (int k = 0; k <= 2 * r; ++k) acc = acc + taps.t[k] * tile[threadIdx.x + k];
  dst[((size_t)b * h + y) * w + x] = acc;
}

// block = 64 columns x 4 row groups; dynamic LDS (kColTile + 2r) x 64 floats
__global__ __launch_bounds__(256) void blur_cols_kernel(const float* __restrict__ src, float* __restrict__ dst, int h,
                                                        int w, Taps taps, int r) {
  extern __shared__ float ctile[];
  const int b = blockIdx.z, x0 = blockIdx.x * 64, y0 = blockIdx.y * kColTile;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int x = min(x0 + tx, w - 1);
  const float* img = src + (size_t)b * h * w;
  for (int i = ty; i < kColTile + 2 * r; i += 4) ctile[i * 64 + tx] = img[(size_t)min(max(y0 + i - r, 0), h - 1) * w + x];
  __syncthreads();
  if (x0 + tx >= w) return;
  for (int i = ty; i < kColTile && y0 + i < h; i += 4) {
    float acc = 0.f;
    for (int k = 0; k <= 2 * r; ++k) acc = acc + taps.t[k] * ctile[(i + k) * 64 + tx];
    dst[((size_t)b * h + y0 + i) * w + x0 + tx] = acc;
  }
}

__global__ __launch_bounds__(256) void downsample_kernel(const float* __restrict__ src, int h, int w,
                                                         float* __restrict__ dst) {
  const int b = blockIdx.z, y = blockIdx.y, oh = h >> 1, ow = w >> 1;
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= ow) return;
  dst[((size_t)b * oh + y) * ow + x] = src[((size_t)b * h + 2 * y) * w + 2 * x];
}

__global__ __launch_bounds__(256) void dog_kernel(const float* __restrict__ levels, size_t level_elems, size_t n,
                                                  float* __restrict__ dog) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    dog[i] = levels[i + level_elems] - levels[i];
}

// ---- detection ---------------------------------------------------------------------------------------------------
struct Dog {
  const float* p;   // DoG of this image, level 0
  size_t ls;        // elements between levels (B * h * w)
  int h, w;
  __device__ float at(int j, int y, int x) const { return p[(size_t)j * ls + (size_t)y * w + x]; }
};

__device__ inline bool is_extremum(const Dog& d, int j, int y, int x, float pre) {
  const float c = d.at(j, y, x);
  const bool up = c >= pre, down = c <= -pre;
  if (!up && !down) return false;
  bool mx = up, mn = down;
  for (int dj = -1; dj <= 1; ++dj)
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx) {
        if (dj == 0 && dy == 0 && dx == 0) continue;
        const float v = d.at(j + dj, y + dy, x + dx);
        mx = mx && c > v;
        mn = mn && c < v;
      }
  return mx || mn;
}

// VLFeat's Newton refinement, acceptance tests included.  rec: x, y, s, sigma, j, y0, x0, 0.
__device__ bool refine(const Dog& d, int j, int y0, int x0, int S, float peak, float edge_lim, float sigma0,
                       float (&rec)[8]) {
  const int h = d.h, w = d.w;
  int x = x0, y = y0, dx = 0, dy = 0;
  float g[3], H[3][3], b[3];
  for (int iter = 0; iter < 5; ++iter) {
    x += dx;
    y += dy;
    const float c = d.at(j, y, x);
    g[0] = 0.5f * (d.at(j, y, x + 1) - d.at(j, y, x - 1));
    g[1] = 0.5f * (d.at(j, y + 1, x) - d.at(j, y - 1, x));
    g[2] = 0.5f * (d.at(j + 1, y, x) - d.at(j - 1, y, x));
    H[0][0] = d.at(j, y, x + 1) + d.at(j, y, x - 1) - 2.f * c;
    H[1][1] = d.at(j, y + 1, x) + d.at(j, y - 1, x) - 2.f * c;
    H[2][2] = d.at(j + 1, y, x) + d.at(j - 1, y, x) - 2.f * c;
    H[0][1] = H[1][0] = 0.25f * (d.at(j, y + 1, x + 1) + d.at(j, y - 1, x - 1) - d.at(j, y + 1, x - 1) - d.at(j, y - 1, x + 1));
    H[0][2] = H[2][0] = 0.25f * (d.at(j + 1, y, x + 1) + d.at(j - 1, y, x - 1) - d.at(j + 1, y, x - 1) - d.at(j - 1, y, x + 1));
    H[1][2] = H[2][1] = 0.25f * (d.at(j + 1, y + 1, x) + d.at(j - 1, y - 1, x) - d.at(j + 1, y - 1, x) - d.at(j - 1, y + 1, x));
    float A[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      b[r] = -g[r];
#pragma unroll
      for (int c2 = 0; c2 < 3; ++c2) A[r][c2] = H[r][c2];
    }
    // Gaussian elimination with partial pivoting (first maximum of |a|), singular -> b = 0
#pragma unroll
    for (int jj = 0; jj < 3; ++jj) {
      int piv = jj;
      float maxa = A[jj][jj], maxabs = fabsf(A[jj][jj]);
#pragma unroll
      for (int i = jj + 1; i < 3; ++i)
        if (fabsf(A[i][jj]) > maxabs) { maxabs = fabsf(A[i][jj]); maxa = A[i][jj]; piv = i; }
      if (maxabs < 1e-10f) { b[0] = b[1] = b[2] = 0.f; break; }
#pragma unroll
      for (int i = jj + 1; i < 3; ++i)
        if (piv == i) {
#pragma unroll
          for (int c2 = 0; c2 < 3; ++c2) { const float t = A[i][c2]; A[i][c2] = A[jj][c2]; A[jj][c2] = t; }
          const float t = b[i]; b[i] = b[jj]; b[jj] = t;
        }
#pragma unroll
      for (int c2 = jj; c2 < 3; ++c2) A[jj][c2] = A[jj][c2] / maxa;
      b[jj] = b[jj] / maxa;
#pragma unroll
      for (int i = jj + 1; i < 3; ++i) {
        const float f = A[i][jj];
#pragma unroll
        for (int c2 = jj; c2 < 3; ++c2) A[i][c2] = A[i][c2] - f * A[jj][c2];
        b[i] = b[i] - f * b[jj];
      }
    }
#pragma unroll
    for (int i = 2; i > 0; --i) {
      const float f = b[i];
#pragma unroll
      for (int ii = i - 1; ii >= 0; --ii) b[ii] = b[ii] - f * A[ii][i];
    }
    dx = ((b[0] > 0.6f && x < w - 2) ? 1 : 0) + ((b[0] < -0.6f && x > 1) ? -1 : 0);
    dy = ((b[1] > 0.6f && y < h - 2) ? 1 : 0) + ((b[1] < -0.6f && y > 1) ? -1 : 0);
    if (dx == 0 && dy == 0) break;
  }
  const float val = d.at(j, y, x) + 0.5f * (g[0] * b[0] + g[1] * b[1] + g[2] * b[2]);
  const float tr = H[0][0] + H[1][1];
  const float det = H[0][0] * H[1][1] - H[0][1] * H[0][1];
  const float score = tr * tr / det;
  const float xn = (float)x + b[0], yn = (float)y + b[1], sn = (float)(j - 1) + b[2];
  const bool good = fabsf(val) >= peak && det > 0.f && score < edge_lim && fabsf(b[0]) < 1.5f && fabsf(b[1]) < 1.5f &&
                    fabsf(b[2]) < 1.5f && xn >= 0.f && xn <= (float)(w - 1) && yn >= 0.f && yn <= (float)(h - 1) &&
                    sn >= -1.f && sn <= (float)(S + 1);
  rec[0] = xn; rec[1] = yn; rec[2] = sn;
  rec[3] = sigma0 * exp2f(sn / (float)S);
  rec[4] = (float)j; rec[5] = (float)y0; rec[6] = (float)x0; rec[7] = 0.f;
  return good;
}

struct DetectArgs {
  const float* dog;
  int B, h, w, S;
  float pre, peak, edge_lim, sigma0;
  int do_refine;
};

__device__ inline bool candidate(const DetectArgs& a, int b, int j, int y, int x, float (&rec)[8]) {
  const Dog d{a.dog + (size_t)b * a.h * a.w, (size_t)a.B * a.h * a.w, a.h, a.w};
  if (!is_extremum(d, j, y, x, a.pre)) return false;
  if (a.do_refine) return refine(d, j, y, x, a.S, a.peak, a.edge_lim, a.sigma0, rec);
  rec[0] = (float)x; rec[1] = (float)y; rec[2] = (float)(j - 1);
  rec[3] = a.sigma0 * exp2f((float)(j - 1) / (float)a.S);
  rec[4] = (float)j; rec[5] = (float)y; rec[6] = (float)x; rec[7] = 0.f;
  return true;
}

__device__ inline int block_sum_256(int v, int* red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const int t = red[0] + red[1] + red[2] + red[3];
  __syncthreads();
  return t;
}

// grid (S * h, B): one block per (DoG level j = 1 .. S, row y); counts the accepted candidates of the row
__global__ __launch_bounds__(256) void detect_count_kernel(DetectArgs a, int32_t* __restrict__ row_counts) {
  __shared__ int red[4];
  const int b = blockIdx.y, j = 1 + blockIdx.x / a.h, y = blockIdx.x % a.h;
  int n = 0;
  if (y >= 1 && y <= a.h - 2)
    for (int x = 1 + threadIdx.x; x <= a.w - 2; x += 256) {
      float rec[8];
      n += candidate(a, b, j, y, x, rec) ? 1 : 0;
    }
  n = block_sum_256(n, red);
  if (threadIdx.x == 0) row_counts[(size_t)b * a.S * a.h + blockIdx.x] = n;
}

// one block per image: in-place exclusive scan of n entries (n = n_fixed, or min(n_dev[b], n_fixed)), total -> total[b]
__global__ __launch_bounds__(256) void scan_kernel(const int32_t* __restrict__ in, int32_t* __restrict__ out, int n_fixed,
                                                   const int32_t* __restrict__ n_dev, int32_t* __restrict__ total) {
  __shared__ int part[257];
  const int b = blockIdx.x;
  const int n = n_dev ? min(max(n_dev[b], 0), n_fixed) : n_fixed;
  const int32_t* src = in + (size_t)b * n_fixed;
  int32_t* dst = out + (size_t)b * n_fixed;
  const int per = (n + 255) / 256, lo = min(threadIdx.x * per, n), hi = min(lo + per, n);
  int s = 0;
  for (int i = lo; i < hi; ++i) s += src[i];
  part[threadIdx.x + 1] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    part[0] = 0;
    for (int i = 1; i <= 256; ++i) part[i] += part[i - 1];
    total[b] = part[256];
  }
  __syncthreads();
  int run = part[threadIdx.x];
  for (int i = lo; i < hi; ++i) {
    const int v = src[i];
    dst[i] = run;
    run += v;
  }
}

// same grid as detect_count_kernel: writes the row's candidates in x order at their scanned offset (slots < cap)
__global__ __launch_bounds__(256) void detect_write_kernel(DetectArgs a, const int32_t* __restrict__ row_offsets, int cap,
                                                           float* __restrict__ out) {
  __shared__ int red[4];
  const int b = blockIdx.y, j = 1 + blockIdx.x / a.h, y = blockIdx.x % a.h;
  if (y < 1 || y > a.h - 2) return;   // whole block: no barrier below is skipped by part of it
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int base = row_offsets[(size_t)b * a.S * a.h + blockIdx.x];
  for (int x0 = 1; x0 <= a.w - 2; x0 += 256) {
    const int x = x0 + threadIdx.x;
    float rec[8];
    const bool hit = x <= a.w - 2 && candidate(a, b, j, y, x, rec);
    const unsigned long long m = __ballot(hit);
    if (lane == 0) red[wave] = __popcll(m);
    __syncthreads();
    int before = 0;
    for (int i = 0; i < wave; ++i) before += red[i];
    const int chunk = red[0] + red[1] + red[2] + red[3];
    const int pos = base + before + __popcll(m & ((1ull << lane) - 1ull));
    if (hit && pos < cap) {
      float* o = out + ((size_t)b * cap + pos) * 8;
#pragma unroll
      for (int i = 0; i < 8; ++i) o[i] = rec[i];
    }
    base += chunk;
    __syncthreads();
  }
}

// ---- gradients, orientation, descriptor --------------------------------------------------------------------------
__device__ inline void grad_at(const float* L, int h, int w, int y, int x, float& mod, float& ang) {
  const float* r = L + (size_t)y * w;
  const float gx = 0.5f * (r[min(x + 1, w - 1)] - r[max(x - 1, 0)]);
  const float gy = 0.5f * (L[(size_t)min(y + 1, h - 1) * w + x] - L[(size_t)max(y - 1, 0) * w + x]);
  mod = sqrtf(gx * gx + gy * gy);
  float a = atan2f(gy, gx);
  if (a < 0.f) a = a + kTwoPi;
  ang = a >= kTwoPi ? 0.f : a;
}

struct Levels {
  const float* p;
  int B, h, w;
  __device__ const float* level(int j, int b) const { return p + ((size_t)j * B + b) * h * w; }
};

// grid (ceil(cap / 4), B), 4 waves: one keypoint per wave, per-lane histograms in LDS reduced in lane order
__global__ __launch_bounds__(256) void orient_kernel(Levels lv, const float* __restrict__ kp, const int32_t* __restrict__ count,
                                                     int cap, int max_ori, int upright, float* __restrict__ angles,
                                                     int32_t* __restrict__ n_angles) {
  __shared__ float hist[4][36][64];
  __shared__ float sum[4][36];
  __shared__ float smooth[4][36];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.y;
  const int k = blockIdx.x * 4 + wave;
  const bool active = k < min(count[b], cap);
  for (int i = 0; i < 36; ++i) hist[wave][i][lane] = 0.f;
  if (active && !upright) {
    const float* rec = kp + ((size_t)b * cap + k) * 8;
    const float xk = rec[0], yk = rec[1], sigma = rec[3];
    const int j = (int)rec[4];
    const float* L = lv.level(j, b);
    const int h = lv.h, w = lv.w;
    const int xi = (int)floorf(xk + 0.5f), yi = (int)floorf(yk + 0.5f);
    const float sw = 1.5f * sigma;
    const int W = max((int)floorf(3.f * sw), 1);
    const float r2max = (float)((double)(W * W) + 0.6);
    const int y_lo = max(-W, -yi), y_hi = min(W, h - 1 - yi), x_lo = max(-W, -xi), x_hi = min(W, w - 1 - xi);
    const int nx = x_hi - x_lo + 1, total = nx * (y_hi - y_lo + 1);
    for (int p = lane; p < total; p += 64) {
      const int ys = y_lo + p / nx, xs = x_lo + p % nx;
      const float ddx = (float)(xi + xs) - xk, ddy = (float)(yi + ys) - yk;
      const float r2 = ddx * ddx + ddy * ddy;
      if (!(r2 < r2max)) continue;
      const float wgt = expf(-r2 / (2.f * sw * sw));
      float mod, ang;
      grad_at(L, h, w, yi + ys, xi + xs, mod, ang);
      const float md = mod * wgt;
      const float fbin = 36.f * ang / kTwoPi;
      const int bin = (int)floorf(fbin - 0.5f);
      const float rb = fbin - (float)bin - 0.5f;
      hist[wave][(bin + 36) % 36][lane] += (1.f - rb) * md;
      hist[wave][(bin + 1) % 36][lane] += rb * md;
    }
  }
  __syncthreads();
  if (lane < 36) {
    float s = 0.f;
    for (int l = 0; l < 64; ++l) s += hist[wave][lane][l];
    sum[wave][lane] = s;
  }
  __syncthreads();
  if (!active || lane != 0) return;
  float* out = angles + ((size_t)b * cap + k) * 4;
  if (upright) {
    out[0] = 0.f;
    n_angles[(size_t)b * cap + k] = 1;
    return;
  }
  float* hs = sum[wave];             // lane 0 alone from here on: the smoothing ping-pongs through LDS, not scratch
  float* tmp = smooth[wave];
  for (int it = 0; it < 6; ++it) {
    for (int i = 0; i < 36; ++i) tmp[i] = (hs[(i + 35) % 36] + hs[i] + hs[(i + 1) % 36]) / 3.f;
    for (int i = 0; i < 36; ++i) hs[i] = tmp[i];
  }
  float maxh = hs[0];
  for (int i = 1; i < 36; ++i) maxh = fmaxf(maxh, hs[i]);
  int n = 0;
  for (int i = 0; i < 36 && n < 4; ++i) {
    const float h0 = hs[i], hm = hs[(i + 35) % 36], hp = hs[(i + 1) % 36];
    if (h0 > 0.8f * maxh && h0 > hm && h0 > hp) {
      const float di = -0.5f * (hp - hm) / (hp + hm - 2.f * h0);
      out[n++] = kTwoPi * ((float)i + di + 0.5f) / 36.f;
    }
  }
  n_angles[(size_t)b * cap + k] = min(n, max_ori);
}

// grid (cap * n_ori, B), one wave per (keypoint, orientation): 128 per-lane bins in LDS, reduced in lane order, then
// L2 / clamp 0.2 / L2 (/ L1 + sqrt), quantised, UBC bin order
__global__ __launch_bounds__(64) void describe_kernel(Levels lv, const float* __restrict__ kp, const int32_t* __restrict__ count,
                                                      int cap, const float* __restrict__ angles,
                                                      const int32_t* __restrict__ n_angles, int n_ori, int l1_root,
                                                      float oct_scale, float sx, float sy,
                                                      const int32_t* __restrict__ row_offsets, int row_cap,
                                                      float* __restrict__ out_rows, uint8_t* __restrict__ out_desc) {
  __shared__ float hist[128][64];
  __shared__ float vec[128];
  const int lane = threadIdx.x, b = blockIdx.y;
  const int k = blockIdx.x / n_ori, o = blockIdx.x % n_ori;
  if (k >= min(count[b], cap) || o >= n_angles[(size_t)b * cap + k]) return;   // whole wave
  const int row = row_offsets[(size_t)b * cap + k] + o;
  if (row >= row_cap) return;
  const float* rec = kp + ((size_t)b * cap + k) * 8;
  const float xk = rec[0], yk = rec[1], sigma = rec[3];
  const int j = (int)rec[4];
  const float angle0 = angles[((size_t)b * cap + k) * 4 + o];
  const float* L = lv.level(j, b);
  const int h = lv.h, w = lv.w;
  for (int i = 0; i < 128; ++i) hist[i][lane] = 0.f;
  const int xi = (int)floorf(xk + 0.5f), yi = (int)floorf(yk + 0.5f);
  const float sbp = 3.f * sigma;
  const int W = (int)floorf(1.41421354f * sbp * 2.5f + 0.5f);
  const float ct0 = cosf(angle0), st0 = sinf(angle0);
  const int y_lo = max(-W, 1 - yi), y_hi = min(W, h - yi - 2), x_lo = max(-W, 1 - xi), x_hi = min(W, w - xi - 2);
  const int nx = x_hi - x_lo + 1, total = (x_hi >= x_lo && y_hi >= y_lo) ? nx * (y_hi - y_lo + 1) : 0;
  for (int p = lane; p < total; p += 64) {
    const int ys = y_lo + p / nx, xs = x_lo + p % nx;
    float mod, ang;
    grad_at(L, h, w, yi + ys, xi + xs, mod, ang);
    float th = ang - angle0;
    if (th < 0.f) th = th + kTwoPi;
    if (th >= kTwoPi) th = th - kTwoPi;
    const float dx = (float)(xi + xs) - xk, dy = (float)(yi + ys) - yk;
    const float nxf = (ct0 * dx + st0 * dy) / sbp;
    const float nyf = (-st0 * dx + ct0 * dy) / sbp;
    const float nt = 8.f * th / kTwoPi;
    const float win = expf(-(nxf * nxf + nyf * nyf) / 8.f);
    const int bx = (int)floorf(nxf - 0.5f), by = (int)floorf(nyf - 0.5f), bt = (int)floorf(nt);
    const float rx = nxf - ((float)bx + 0.5f), ry = nyf - ((float)by + 0.5f), rt = nt - (float)bt;
    const float wm = win * mod;
#pragma unroll
    for (int ix = 0; ix < 2; ++ix)
#pragma unroll
      for (int iy = 0; iy < 2; ++iy) {
        const int cx = bx + ix, cy = by + iy;
        if (cx < -2 || cx >= 2 || cy < -2 || cy >= 2) continue;
#pragma unroll
        for (int it = 0; it < 2; ++it) {
          const float wt = wm * fabsf((float)(1 - ix) - rx) * fabsf((float)(1 - iy) - ry) * fabsf((float)(1 - it) - rt);
          hist[(cy + 2) * 32 + (cx + 2) * 8 + ((bt + it) & 7)][lane] += wt;
        }
      }
  }
  __syncthreads();
  float v[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    float s = 0.f;
    for (int l = 0; l < 64; ++l) s += hist[lane + 64 * q][l];
    v[q] = s;
    vec[lane + 64 * q] = s;
  }
  __syncthreads();
  float ss = 0.f;
  for (int i = 0; i < 128; ++i) ss += vec[i] * vec[i];
  float nrm = sqrtf(ss) + kEps;
#pragma unroll
  for (int q = 0; q < 2; ++q) v[q] = fminf(v[q] / nrm, 0.2f);
  __syncthreads();
  vec[lane] = v[0];
  vec[lane + 64] = v[1];
  __syncthreads();
  ss = 0.f;
  for (int i = 0; i < 128; ++i) ss += vec[i] * vec[i];
  nrm = sqrtf(ss) + kEps;
  v[0] = v[0] / nrm;
  v[1] = v[1] / nrm;
  if (l1_root) {
    __syncthreads();
    vec[lane] = v[0];
    vec[lane + 64] = v[1];
    __syncthreads();
    float s1 = 0.f;
    for (int i = 0; i < 128; ++i) s1 += vec[i];
    s1 = fmaxf(s1, kTiny);
    v[0] = sqrtf(v[0] / s1);
    v[1] = sqrtf(v[1] / s1);
  }
  uint8_t* d = out_desc + ((size_t)b * row_cap + row) * 128;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int bin = lane + 64 * q;
    const int ubc = (bin & ~7) | ((8 - (bin & 7)) & 7);
    d[ubc] = (uint8_t)fminf(255.f, floorf(512.f * v[q] + 0.5f));
  }
  if (lane == 0) {
    float* r = out_rows + ((size_t)b * row_cap + row) * 6;
    const float s = sigma * oct_scale, c = cosf(angle0), sn = sinf(angle0);
    r[0] = (xk * oct_scale + 0.5f) * sx;
    r[1] = (yk * oct_scale + 0.5f) * sy;
    r[2] = (s * c) * sx;
    r[3] = (-s * sn) * sx;
    r[4] = (s * sn) * sy;
    r[5] = (s * c) * sy;
  }
}

bool taps_ok(const float* taps, int r) { return taps && r >= 1 && r <= kMaxRadius; }

}  // namespace

extern "C" {

int vc_sift_grey(const uint8_t* images_bgr, int n_images, int h, int w, int out_h, int out_w, int upsample, float* out,
                 vc_stream_t stream) {
  if (!images_bgr || !out || n_images <= 0 || h <= 0 || w <= 0 || out_h <= 0 || out_w <= 0 || out_h > h || out_w > w ||
      (upsample != 0 && upsample != 1))
    return VC_ERR_INVALID_ARG;
  const int H = upsample ? 2 * out_h : out_h, W = upsample ? 2 * out_w : out_w;
  if (H > 65535 || n_images > 65535) return VC_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(grey_kernel, dim3((W + 255) / 256, H, n_images), dim3(256), 0, (hipStream_t)stream, images_bgr, h, w,
                     out_h, out_w, upsample, out);
  return vc::check_launch();
}

int vc_sift_blur(const float* src, float* tmp, float* dst, int n_images, int h, int w, const float* taps, int radius,
                 vc_stream_t stream) {
  if (!src || !tmp || !dst || n_images <= 0 || h <= 0 || w <= 0 || tmp == src || tmp == dst) return VC_ERR_INVALID_ARG;
  if (!taps_ok(taps, radius)) return VC_ERR_UNSUPPORTED;
  if (h > 65535 || n_images > 65535) return VC_ERR_UNSUPPORTED;
  Taps t{};
  for (int i = 0; i <= 2 * radius; ++i) t.t[i] = taps[i];
  hipLaunchKernelGGL(blur_rows_kernel, dim3((w + kRowTile - 1) / kRowTile, h, n_images), dim3(256), 0, (hipStream_t)stream,
                     src, tmp, h, w, t, radius);
  if (int st = vc::check_launch()) return st;
  const size_t lds = (size_t)(kColTile + 2 * radius) * 64 * sizeof(float);
  hipLaunchKernelGGL(blur_cols_kernel, dim3((w + 63) / 64, (h + kColTile - 1) / kColTile, n_images), dim3(256), lds,
                     (hipStream_t)stream, tmp, dst, h, w, t, radius);
  return vc::check_launch();
}

int vc_sift_downsample(const float* src, int n_images, int h, int w, float* dst, vc_stream_t stream) {
  if (!src || !dst || n_images <= 0 || h < 2 || w < 2) return VC_ERR_INVALID_ARG;
  if (n_images > 65535) return VC_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(downsample_kernel, dim3(((w >> 1) + 255) / 256, h >> 1, n_images), dim3(256), 0, (hipStream_t)stream,
                     src, h, w, dst);
  return vc::check_launch();
}

int vc_sift_dog(const float* levels, int n_levels, int n_images, int h, int w, float* dog, vc_stream_t stream) {
  if (!levels || !dog || n_levels < 2 || n_images <= 0 || h <= 0 || w <= 0) return VC_ERR_INVALID_ARG;
  const size_t le = (size_t)n_images * h * w, n = le * (n_levels - 1);
  const size_t blocks = (n + 255) / 256;
  hipLaunchKernelGGL(dog_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, (hipStream_t)stream,
                     levels, le, n, dog);
  return vc::check_launch();
}

int vc_sift_detect(const float* dog, int n_images, int h, int w, int n_dog_levels, float peak_threshold,
                   float edge_threshold, int refine, int32_t* row_counts, int cap, float* out_keypoints,
                   int32_t* out_count, vc_stream_t stream) {
  if (!dog || !row_counts || !out_keypoints || !out_count || n_images <= 0 || h < 3 || w < 3 || n_dog_levels < 3 ||
      cap <= 0 || !(peak_threshold >= 0.f) || !(edge_threshold > 0.f) || (refine != 0 && refine != 1))
    return VC_ERR_INVALID_ARG;
  const int S = n_dog_levels - 2;
  if ((long long)S * h > 0x7fffffff || n_images > 65535) return VC_ERR_UNSUPPORTED;
  DetectArgs a;
  a.dog = dog; a.B = n_images; a.h = h; a.w = w; a.S = S;
  a.pre = (float)(0.8 * (double)peak_threshold);
  a.peak = peak_threshold;
  const double r = edge_threshold;
  a.edge_lim = (float)((r + 1.0) * (r + 1.0) / r);
  a.sigma0 = (float)(1.6 * std::pow(2.0, 1.0 / S));
  a.do_refine = refine;
  hipLaunchKernelGGL(detect_count_kernel, dim3(S * h, n_images), dim3(256), 0, (hipStream_t)stream, a, row_counts);
  if (int st = vc::check_launch()) return st;
  hipLaunchKernelGGL(scan_kernel, dim3(n_images), dim3(256), 0, (hipStream_t)stream, row_counts, row_counts, S * h,
                     (const int32_t*)nullptr, out_count);
  if (int st = vc::check_launch()) return st;
  hipLaunchKernelGGL(detect_write_kernel, dim3(S * h, n_images), dim3(256), 0, (hipStream_t)stream, a,
                     (const int32_t*)row_counts, cap, out_keypoints);
  return vc::check_launch();
}

int vc_sift_orient(const float* levels, int n_levels, int n_images, int h, int w, const float* keypoints,
                   const int32_t* count, int cap, int max_orientations, int upright, float* out_angles,
                   int32_t* out_n_angles, vc_stream_t stream) {
  if (!levels || !keypoints || !count || !out_angles || !out_n_angles || n_levels < 4 || n_images <= 0 || h <= 0 ||
      w <= 0 || cap <= 0 || max_orientations < 1 || max_orientations > 4 || (upright != 0 && upright != 1))
    return VC_ERR_INVALID_ARG;
  if (n_images > 65535) return VC_ERR_UNSUPPORTED;
  Levels lv{levels, n_images, h, w};
  hipLaunchKernelGGL(orient_kernel, dim3((cap + 3) / 4, n_images), dim3(256), 0, (hipStream_t)stream, lv, keypoints, count,
                     cap, max_orientations, upright, out_angles, out_n_angles);
  return vc::check_launch();
}

int vc_sift_describe(const float* levels, int n_levels, int n_images, int h, int w, const float* keypoints,
                     const int32_t* count, int cap, const float* angles, const int32_t* n_angles, int max_orientations,
                     int normalization, float octave_scale, float scale_x, float scale_y, int32_t* row_offsets,
                     int row_cap, float* out_rows, uint8_t* out_desc, int32_t* out_row_count, vc_stream_t stream) {
  if (!levels || !keypoints || !count || !angles || !n_angles || !row_offsets || !out_rows || !out_desc ||
      !out_row_count || n_levels < 4 || n_images <= 0 || h <= 0 || w <= 0 || cap <= 0 || max_orientations < 1 ||
      max_orientations > 4 || row_cap <= 0 || (normalization != VC_SIFT_NORM_L2 && normalization != VC_SIFT_NORM_L1_ROOT) ||
      !(octave_scale > 0.f) || !(scale_x > 0.f) || !(scale_y > 0.f))
    return VC_ERR_INVALID_ARG;
  if (row_cap < cap * max_orientations) return VC_ERR_WORKSPACE;
  if (n_images > 65535 || (long long)cap * max_orientations > 0x7fffffff) return VC_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(scan_kernel, dim3(n_images), dim3(256), 0, (hipStream_t)stream, n_angles, row_offsets, cap, count,
                     out_row_count);
  if (int st = vc::check_launch()) return st;
  Levels lv{levels, n_images, h, w};
  hipLaunchKernelGGL(describe_kernel, dim3(cap * max_orientations, n_images), dim3(64), 0, (hipStream_t)stream, lv,
                     keypoints, count, cap, angles, n_angles, max_orientations, normalization == VC_SIFT_NORM_L1_ROOT ? 1 : 0,
                     octave_scale, scale_x, scale_y, (const int32_t*)row_offsets, row_cap, out_rows, out_desc);
  return vc::check_launch();
}

}  // extern "C"
