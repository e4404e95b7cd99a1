// Image registration (gfx950): absolute pose from 2D-3D correspondences.  vc_p3p solves the minimal
// problem (three points) for many samples of many registration problems at once; vc_absolute_pose_score and
// vc_absolute_pose_inliers count and mark the correspondences a pixel projection matrix explains.  Sampling, the choice of the
// best hypothesis, the refit and the acceptance rule stay above the ABI (vit_colmap_amd/mapping/absolute_pose.py).
// Specification: tests/util_absolute_pose.py.
//
// vc_p3p — float64, one hypothesis per lane, one wave per workgroup, no barrier, no LDS.  With unit rays f1, f2, f3, depths
// s1, s2, s3 along them and d_ij the squared distances of the world points, the law of cosines gives
//     s_i^2 + s_j^2 - 2 s_i s_j (f_i . f_j) = d_ij.
// Substituting s2 = u s1, s3 = v s1 and eliminating s1^2 leaves two conics in (u, v) (A = d13 / d12, B = d23 / d12):
//     A (1 + u^2 - 2 u c12) = 1 + v^2 - 2 v c13            B (1 + u^2 - 2 u c12) = u^2 + v^2 - 2 u v c23
// whose difference is linear in v: v = N(u) / D(u), N quadratic, D linear.  Put into the first conic it is a quartic in u:
//     N^2 - 2 c13 N D + D^2 - A (1 + u^2 - 2 u c12) D^2 = 0.
// The specification eliminates u instead (a resultant, a quartic in v) and takes the roots from numpy's eigensolver, so that
// the two agree is a test of both.  Per lane:
//   1. the quartic's coefficients, scaled to unit maximum
//   2. real roots   u in [0, 1] of the quartic and, for u > 1, w = 1 / u in (0, 1) of its reversal: the roots of the k-th
//                   derivative bracket those of the (k-1)-th, each bracket is bisected at most kBisections times.  A root list
//                   is positional (slot s: the root between breakpoints s-1 and s, NaN for none), every loop fully unrolled,
//                   so no array has a run-time index
//   3. depths       v = N / D, s1 from d12; at most kPolish Newton steps on the three distance equations themselves take out
//                   the rounding of the quartic's coefficients and of the division by D
//   4. pose         an orthonormal frame on the world triangle and one on the camera-frame triangle: R = Fc Fw', t from the
//                   centroids
// Every loop has a constant trip count but the bisection and the polish, which are capped.  The kernel around solve_p3p and
// the pieces of the root bracketing are those of minimal_solver.h, shared with the five-point solver.  The solver functions are
// __host__ __device__: tools/p3p_host.cpp includes this file and calls solve_p3p on one problem after another.
//
// Scoring — float32 in exactly the specification's order of single operations (the library is built with -ffp-contract=off),
// no division: p = P (X, 1); inlier iff p_w > 0 and |p_xy - obs p_w|^2 <= e^2 p_w^2.  The kernels are those of inlier_count.h.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/vitcolmap_hip.h"
#include "inlier_count.h"
#include "minimal_solver.h"

namespace {

constexpr int kMaxPoses = 4;
constexpr int kPolish = 3;
constexpr double kParallelTol = 1e-20;      // squared sine below which two rays, or two sides of the world triangle, are parallel
constexpr double kProperTol = 1e-9;         // |det R - 1| of a returned rotation

// One level of the bracketing: the (4 - DEG)-th derivative of sum a[i] t^i over (4 - DEG)!, of degree DEG, on [0, 1].  prev:
// the roots of its derivative in positional slots 0 .. DEG - 2 (NaN: none), ascending among the slots that are set; with 0
// and 1 they cut the interval into pieces on which this polynomial is monotone, so a sign change over a piece brackets one
// root.  cur[s]: the root of the piece that ends at breakpoint s (s = DEG - 1: at 1), or NaN.
template <int DEG>
__host__ __device__ __forceinline__ void roots_level(const double (&a)[5], const double (&prev)[4], double (&cur)[4]) {
  constexpr int K = 4 - DEG;
  double coef[DEG + 1];
  vc::derivative_coefficients(coef, DEG, K, a);
  double lo = 0.0, f_lo = vc::horner(coef, DEG, 0.0);
#pragma unroll
  for (int s = 0; s < DEG; ++s) {
    const double hi = s < DEG - 1 ? prev[s] : 1.0;
    double root = NAN;
    if (hi == hi) {                                          // a breakpoint that is set
      const double f_hi = vc::horner(coef, DEG, hi);
      root = vc::root_of_piece(coef, DEG, lo, hi, f_lo, f_hi);
      lo = hi, f_lo = f_hi;
    }
    cur[s] = root;
  }
#pragma unroll
  for (int s = DEG; s < 4; ++s) cur[s] = NAN;
}

// The real roots in [0, 1] of sum a[i] t^i, ascending over the slots that are set.
__host__ __device__ __forceinline__ void real_roots_unit(const double (&a)[5], double (&roots)[4]) {
  double none[4] = {NAN, NAN, NAN, NAN}, r1[4], r2[4], r3[4];
  roots_level<1>(a, none, r1);
  roots_level<2>(a, r1, r2);
  roots_level<3>(a, r2, r3);
  roots_level<4>(a, r3, roots);
}

struct Triangle {
  double f[3][3];                  // unit rays
  double X[3][3];                  // world points
  double c12, c13, c23;            // cosines between the rays
  double d12, d13, d23;            // squared distances between the world points
};

__host__ __device__ __forceinline__ void cross3(const double (&a)[3], const double (&b)[3], double (&c)[3]) {
  c[0] = a[1] * b[2] - a[2] * b[1], c[1] = a[2] * b[0] - a[0] * b[2], c[2] = a[0] * b[1] - a[1] * b[0];
}

__host__ __device__ __forceinline__ double dot3(const double (&a)[3], const double (&b)[3]) {
  return a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
}

// Rays and points -> the triangle's numbers; false for non-finite input, two coincident points or rays, collinear points.
__host__ __device__ __forceinline__ bool make_triangle(const double (&x)[3], const double (&y)[3], Triangle& g) {
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double inv = 1.0 / sqrt(x[i] * x[i] + y[i] * y[i] + 1.0);
    g.f[i][0] = x[i] * inv, g.f[i][1] = y[i] * inv, g.f[i][2] = inv;
    ok = ok && fabs(x[i]) < INFINITY && fabs(y[i]) < INFINITY && inv > 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) ok = ok && fabs(g.X[i][k]) < INFINITY;
  }
  double c[3], e1[3], e2[3], e3[3];
  cross3(g.f[0], g.f[1], c), ok = ok && dot3(c, c) > kParallelTol;
  cross3(g.f[0], g.f[2], c), ok = ok && dot3(c, c) > kParallelTol;
  cross3(g.f[1], g.f[2], c), ok = ok && dot3(c, c) > kParallelTol;
#pragma unroll
  for (int k = 0; k < 3; ++k) e1[k] = g.X[1][k] - g.X[0][k], e2[k] = g.X[2][k] - g.X[0][k], e3[k] = g.X[2][k] - g.X[1][k];
  g.d12 = dot3(e1, e1), g.d13 = dot3(e2, e2), g.d23 = dot3(e3, e3);
  ok = ok && g.d12 > 0.0 && g.d13 > 0.0 && g.d23 > 0.0 && g.d12 < INFINITY && g.d13 < INFINITY && g.d23 < INFINITY;
  cross3(e1, e2, c);
  ok = ok && dot3(c, c) > kParallelTol * g.d12 * g.d13;
  g.c12 = dot3(g.f[0], g.f[1]), g.c13 = dot3(g.f[0], g.f[2]), g.c23 = dot3(g.f[1], g.f[2]);
  return ok;                                                 // every comparison is false for NaN
}

// |residual|^2 of the three distance equations at the depths s.
__host__ __device__ __forceinline__ double distance_residual(const Triangle& g, const double (&s)[3], double (&r)[3]) {
  r[0] = s[0] * s[0] + s[1] * s[1] - 2.0 * s[0] * s[1] * g.c12 - g.d12;
  r[1] = s[0] * s[0] + s[2] * s[2] - 2.0 * s[0] * s[2] * g.c13 - g.d13;
  r[2] = s[1] * s[1] + s[2] * s[2] - 2.0 * s[1] * s[2] * g.c23 - g.d23;
  return r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
}

// Newton on the three distance equations: at most kPolish steps, each kept only if it lowers the residual.
__host__ __device__ __forceinline__ void polish_depths(const Triangle& g, double (&s)[3]) {
  double r[3];
  double res = distance_residual(g, s, r);
  for (int it = 0; it < kPolish; ++it) {
    // J = [a b 0; c 0 d; 0 e f]
    const double a = 2.0 * s[0] - 2.0 * s[1] * g.c12, b = 2.0 * s[1] - 2.0 * s[0] * g.c12;
    const double c = 2.0 * s[0] - 2.0 * s[2] * g.c13, d = 2.0 * s[2] - 2.0 * s[0] * g.c13;
    const double e = 2.0 * s[1] - 2.0 * s[2] * g.c23, f = 2.0 * s[2] - 2.0 * s[1] * g.c23;
    const double inv = -1.0 / (-a * d * e - b * c * f);      // det J
    // adj(J) r
    const double q0 = (-d * e) * r[0] + (-b * f) * r[1] + (b * d) * r[2];
    const double q1 = (-c * f) * r[0] + (a * f) * r[1] + (-a * d) * r[2];
    const double q2 = (c * e) * r[0] + (-a * e) * r[1] + (-b * c) * r[2];
    const double sn[3] = {s[0] + inv * q0, s[1] + inv * q1, s[2] + inv * q2};
    double rn[3];
    const double resn = distance_residual(g, sn, rn);
    if (!(resn < res)) break;                                // also for a NaN step
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k] = sn[k], r[k] = rn[k];
    res = resn;
  }
}

// A right-handed orthonormal frame on the triangle p0 p1 p2: columns e1 along p1 - p0, e2 in the plane, e3 the normal.
__host__ __device__ __forceinline__ void frame_of(const double (&p)[3][3], double (&e)[3][3]) {
  double a[3], b[3], n[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) a[k] = p[1][k] - p[0][k], b[k] = p[2][k] - p[0][k];
  const double ia = 1.0 / sqrt(dot3(a, a));
#pragma unroll
  for (int k = 0; k < 3; ++k) e[0][k] = a[k] * ia;
  cross3(e[0], b, n);
  const double in = 1.0 / sqrt(dot3(n, n));
#pragma unroll
  for (int k = 0; k < 3; ++k) e[2][k] = n[k] * in;
  cross3(e[2], e[0], e[1]);
}

// One pose from a root: u = s2 / s1 (reversed: the root is w = 1 / u).  out: R row-major, then t.  -> false when a depth is
// not positive or the pose is not finite and proper.
__host__ __device__ __forceinline__ bool pose_from_root(const Triangle& g, const double (&fw)[3][3], const double (&n)[3],
                                                        const double (&dd)[2], double root, bool reversed, double* out) {
  const double u = reversed ? 1.0 / root : root;
  if (!(u > 0.0 && u < INFINITY)) return false;
  const double v = ((n[2] * u + n[1]) * u + n[0]) / (dd[1] * u + dd[0]);
  if (!(v > 0.0 && v < INFINITY)) return false;
  const double s1 = sqrt(g.d12 / ((u - 2.0 * g.c12) * u + 1.0));
  double s[3] = {s1, u * s1, v * s1};
  polish_depths(g, s);
  if (!(s[0] > 0.0 && s[1] > 0.0 && s[2] > 0.0 && s[0] < INFINITY && s[1] < INFINITY && s[2] < INFINITY)) return false;
  double pc[3][3], fc[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int k = 0; k < 3; ++k) pc[i][k] = s[i] * g.f[i][k];
  frame_of(pc, fc);
  double r[9], t[3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) r[3 * i + j] = fc[0][i] * fw[0][j] + fc[1][i] * fw[1][j] + fc[2][i] * fw[2][j];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double mc = (pc[0][i] + pc[1][i] + pc[2][i]) / 3.0;
    double rm = 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) rm += r[3 * i + j] * ((g.X[0][j] + g.X[1][j] + g.X[2][j]) / 3.0);
    t[i] = mc - rm;
  }
  const double det = r[0] * (r[4] * r[8] - r[5] * r[7]) + r[1] * (r[5] * r[6] - r[3] * r[8]) + r[2] * (r[3] * r[7] - r[4] * r[6]);
  bool ok = fabs(det - 1.0) < kProperTol;                    // false for NaN
#pragma unroll
  for (int k = 0; k < 9; ++k) ok = ok && fabs(r[k]) <= 2.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) ok = ok && fabs(t[k]) < INFINITY;
  if (!ok) return false;
#pragma unroll
  for (int k = 0; k < 9; ++k) out[k] = r[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) out[9 + k] = t[k];
  return true;
}

// Three 2D-3D correspondences (normalised image points (x, y), world points g.X filled by the caller) -> up to four poses at
// `out` (12 doubles each), ascending in u; -> their number.
__host__ __device__ __forceinline__ int solve_p3p(const double (&x)[3], const double (&y)[3], Triangle& g, double* out) {
  if (!make_triangle(x, y, g)) return 0;
  const double A = g.d13 / g.d12, B = g.d23 / g.d12;
  const double n[3] = {A - B - 1.0, -2.0 * (A - B) * g.c12, A - B + 1.0};      // N(u), from the constant up
  const double dd[2] = {-2.0 * g.c13, 2.0 * g.c23};                              // D(u)
  const double q[3] = {1.0, -2.0 * g.c12, 1.0};                                  // 1 + u^2 - 2 u c12
  const double d2[3] = {dd[0] * dd[0], 2.0 * dd[0] * dd[1], dd[1] * dd[1]};
  const double nn[5] = {n[0] * n[0], 2.0 * n[0] * n[1], n[1] * n[1] + 2.0 * n[0] * n[2], 2.0 * n[1] * n[2], n[2] * n[2]};
  const double nd[5] = {n[0] * dd[0], n[0] * dd[1] + n[1] * dd[0], n[1] * dd[1] + n[2] * dd[0], n[2] * dd[1], 0.0};
  const double qd[5] = {q[0] * d2[0], q[0] * d2[1] + q[1] * d2[0], q[0] * d2[2] + q[1] * d2[1] + q[2] * d2[0],
                        q[1] * d2[2] + q[2] * d2[1], q[2] * d2[2]};
  double p[5], rev[5], big = 0.0;
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    p[i] = nn[i] - 2.0 * g.c13 * nd[i] + (i < 3 ? d2[i] : 0.0) - A * qd[i];
    big = fmax(big, fabs(p[i]));
  }
  if (!(big > 0.0 && big < INFINITY)) return 0;              // no equation left (or not finite): nothing this route can solve
  bool finite = true;
#pragma unroll
  for (int i = 0; i < 5; ++i) p[i] /= big, finite = finite && fabs(p[i]) <= 1.0;
  if (!finite) return 0;
#pragma unroll
  for (int i = 0; i < 5; ++i) rev[i] = p[4 - i];
  double fw[3][3];
  frame_of(g.X, fw);
  double direct[4], inverse[4];
  real_roots_unit(p, direct);
  real_roots_unit(rev, inverse);
  // ascending u: the roots in [0, 1], then those above 1 (w in (0, 1), descending)
  int count = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (direct[i] == direct[i] && count < kMaxPoses && pose_from_root(g, fw, n, dd, direct[i], false, out + 12 * count)) ++count;
#pragma unroll
  for (int i = 3; i >= 0; --i) {
    const double w = inverse[i];
    if (w > 0.0 && w < 1.0 && count < kMaxPoses && pose_from_root(g, fw, n, dd, w, true, out + 12 * count)) ++count;
  }
  return count;
}

struct Correspondences { const double* __restrict__ rays_n; const double* __restrict__ xyz; };   // normalised (x, y); world points

struct P3P {
  static constexpr int kSample = 3, kMaxSolutions = kMaxPoses, kWidth = 12, kWorkDoubles = 0;
  using Data = Correspondences;
  static bool usable(Data d) { return d.rays_n && d.xyz; }
  static __device__ __forceinline__ int solve(Data d, long long lo, const int (&s)[3], double*, int, double* out) {
    Triangle g;
    double x[3], y[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const double* r = d.rays_n + (lo + s[i]) * 2;
      const double* w = d.xyz + (lo + s[i]) * 3;
      x[i] = r[0], y[i] = r[1];
      g.X[i][0] = w[0], g.X[i][1] = w[1], g.X[i][2] = w[2];
    }
    return solve_p3p(x, y, g, out);
  }
};

// ---- scoring ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool inlier_p(const float (&m)[12], float x, float y, float z, float ox, float oy, float t2) {
  const float p0 = m[0] * x + m[1] * y + m[2] * z + m[3];
  const float p1 = m[4] * x + m[5] * y + m[6] * z + m[7];
  const float pw = m[8] * x + m[9] * y + m[10] * z + m[11];
  const float dx = p0 - ox * pw;
  const float dy = p1 - oy * pw;
  return pw > 0.f && dx * dx + dy * dy <= t2 * (pw * pw);   // NaN hypotheses compare false
}

struct Points { const float2* __restrict__ obs; const float4* __restrict__ xyz4; };   // pixel observations; world points, w not read

struct RuleP {
  static constexpr int W = 12;
  using Data = Points;
  static bool usable(Data d) { return d.obs && d.xyz4 && ((uintptr_t)d.xyz4) % 16 == 0 && ((uintptr_t)d.obs) % 8 == 0; }
  static __device__ __forceinline__ bool inlier(const float (&m)[12], Data d, int i, float t2) {
    const float4 q = d.xyz4[i];
    const float2 o = d.obs[i];
    return inlier_p(m, q.x, q.y, q.z, o.x, o.y, t2);
  }
};

}  // namespace

extern "C" {

int vc_p3p(const double* rays_n, const double* xyz, const int32_t* offsets, int n_prob, const int32_t* samples, int n_hyp,
           double* out_pose, int32_t* out_count, vc_stream_t stream) {
  return vc::launch_minimal_solver<P3P>({rays_n, xyz}, offsets, n_prob, samples, n_hyp, out_pose, out_count, stream);
}

int vc_absolute_pose_score(const float* obs, const float* xyz4, const int32_t* offsets, int n_prob, const float* hyp, int n_hyp,
                           float max_error, int32_t* out_counts, vc_stream_t stream) {
  return vc::launch_inlier_count<RuleP>({(const float2*)obs, (const float4*)xyz4}, offsets, n_prob, hyp, n_hyp, max_error,
                                        out_counts, stream);
}

int vc_absolute_pose_inliers(const float* obs, const float* xyz4, const int32_t* offsets, int n_prob, const float* models,
                             float max_error, uint8_t* out_mask, vc_stream_t stream) {
  return vc::launch_inlier_mask<RuleP>({(const float2*)obs, (const float4*)xyz4}, offsets, n_prob, models, max_error, out_mask,
                                       stream);
}

}  // extern "C"
