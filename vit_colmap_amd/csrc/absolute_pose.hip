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
//   2. real roots   u in [0, e] of the quartic and, for u > e, w = 1 / u in (0, 1 / e) of its reversal (e just above 1, so
//                   that u = 1, two points equally far from the camera, lies inside the first range: minimal_solver.h
//                   kSeamEnd): the roots of the k-th
//                   derivative bracket those of the (k-1)-th, each bracket is bisected at most kBisections times.  A root list
//                   is positional (slot s: the root between breakpoints s-1 and s, NaN for none), every loop fully unrolled,
//                   so no array has a run-time index
//   3. depths       v = N / D, s1 from d12; at most kPolish Newton steps on the three distance equations themselves take out
//                   the rounding of the quartic's coefficients and of the division by D.  Where D nearly vanishes at a root, v
//                   comes from the first conic; where the quartic has a double root, the points are relabelled and steps 1 to
//                   3 run again (solve_p3p)
//   4. pose         an orthonormal frame on the world triangle and one on the camera-frame triangle, both along the world
//                   triangle's longest side: R = Fc Fw', t from the centroids
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
constexpr double kTouch = 1e-12;            // |p| over the sum of its terms' magnitudes below which p touches zero at a root of p'
constexpr double kSmallD = 1e-4;            // |D(u)| over the sum of its terms' magnitudes below which v is not taken from N / D

// One level of the bracketing: the (4 - DEG)-th derivative of sum a[i] t^i over (4 - DEG)!, of degree DEG, on [0, vc::kSeamEnd].
// prev: the roots of its derivative in positional slots 0 .. DEG - 2 (NaN: none), ascending among the slots that are set; with 0
// and the end they cut the interval into pieces on which this polynomial is monotone, so a sign change over a piece brackets
// one root.  cur[s]: the root of the piece that ends at breakpoint s (s = DEG - 1: at the end), or NaN.
template <int DEG>
__host__ __device__ __forceinline__ void roots_level(const double (&a)[5], const double (&prev)[4], double (&cur)[4]) {
  constexpr int K = 4 - DEG;
  double coef[DEG + 1];
  vc::derivative_coefficients(coef, DEG, K, a);
  double lo = 0.0, f_lo = vc::horner(coef, DEG, 0.0);
#pragma unroll
  for (int s = 0; s < DEG; ++s) {
    const double hi = s < DEG - 1 ? prev[s] : vc::kSeamEnd;
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

// The real roots in [0, vc::kSeamEnd] of sum a[i] t^i, ascending over the slots that are set.  -> true when the polynomial
// comes within kTouch of its terms' sum at a root of its derivative: a double root, or two that rounding may have merged, which
// a sign change does not find reliably.
__host__ __device__ __forceinline__ bool real_roots_unit(const double (&a)[5], double (&roots)[4]) {
  double none[4] = {NAN, NAN, NAN, NAN}, r1[4], r2[4], r3[4];
  roots_level<1>(a, none, r1);
  roots_level<2>(a, r1, r2);
  roots_level<3>(a, r2, r3);
  roots_level<4>(a, r3, roots);
  bool touches = false;
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    const double b = r3[s];                                  // in (0, kSeamEnd) or NaN, for which the comparison is false
    const double terms = (((fabs(a[4]) * b + fabs(a[3])) * b + fabs(a[2])) * b + fabs(a[1])) * b + fabs(a[0]);
    touches = touches || fabs(vc::horner(a, 4, b)) <= kTouch * terms;
  }
  return touches;
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

// A right-handed orthonormal frame on the triangle p0 p1 p2: columns e1 along one side, e2 in the plane, e3 the normal.
// side 0: e1 along p1 - p0, the plane through p2; side 1: along p2 - p0, through p1; side 2: along p2 - p1, through p0.  The
// world frame and the camera frame of a pose take the same side, the longest of the world triangle: the depths along two rays
// that nearly coincide are determined only to rounding over the sine of their angle, and a frame laid along the short side
// between them would turn the third point by that error times the ratio of the sides.
__host__ __device__ __forceinline__ void frame_of(const double (&p)[3][3], int side, double (&e)[3][3]) {
  double a[3], b[3], n[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double from = side == 2 ? p[1][k] : p[0][k], to = side == 0 ? p[1][k] : p[2][k];
    const double third = side == 0 ? p[2][k] : side == 1 ? p[1][k] : p[0][k];
    a[k] = to - from, b[k] = third - from;
  }
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
// not positive or the pose is not finite and proper.  Where D(u) cancels to within kSmallD of its terms, N / D has lost that
// many digits (N vanishes with D), and v is a root of the first conic instead, v^2 - 2 c13 v + 1 - A (1 + u^2 - 2 u c12) = 0:
// the one that leaves the smaller residual in the second conic.  (Both leave none where D = 0 exactly; the quartic then has a
// double root, which solve_p3p handles.)
__host__ __device__ __forceinline__ bool pose_from_root(const Triangle& g, const double (&fw)[3][3], int side, const double (&n)[3],
                                                        const double (&dd)[2], double root, bool reversed, double* out) {
  const double u = reversed ? 1.0 / root : root;
  if (!(u > 0.0 && u < INFINITY)) return false;
  const double d = dd[1] * u + dd[0];
  double v = ((n[2] * u + n[1]) * u + n[0]) / d;
  if (!(fabs(d) > kSmallD * (fabs(dd[1] * u) + fabs(dd[0])))) {
    const double A = g.d13 / g.d12, B = g.d23 / g.d12, q = (u - 2.0 * g.c12) * u + 1.0;
    const double sq = sqrt(fmax(g.c13 * g.c13 - 1.0 + A * q, 0.0));
    const double va = g.c13 - sq, vb = g.c13 + sq;
    const double ra = fabs(B * q - (u * u + va * va - 2.0 * u * va * g.c23)), rb = fabs(B * q - (u * u + vb * vb - 2.0 * u * vb * g.c23));
    v = ra <= rb ? va : vb;
  }
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
  frame_of(pc, side, fc);
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

// Three 2D-3D correspondences (normalised image points (x, y), world points g.X filled by the caller) under the labelling they
// come in -> up to four poses at `out` (12 doubles each), ascending in u; -> their number.  `clean` is cleared where this
// labelling's elimination is not to be trusted: the quartic touches zero (a double root, or two that rounding may merge).
__host__ __device__ __forceinline__ int solve_labelled(const double (&x)[3], const double (&y)[3], Triangle& g, double* out,
                                                       bool& clean) {
  clean = true;
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
  const int side = g.d12 >= g.d13 && g.d12 >= g.d23 ? 0 : g.d13 >= g.d23 ? 1 : 2;
  frame_of(g.X, side, fw);
  double direct[4], inverse[4];
  bool doubtful = real_roots_unit(p, direct);
  doubtful = real_roots_unit(rev, inverse) || doubtful;
  // ascending u: the roots in [0, kSeamEnd], then those above (w in (0, kSeamInv), descending)
  int count = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (direct[i] == direct[i] && count < kMaxPoses && pose_from_root(g, fw, side, n, dd, direct[i], false, out + 12 * count))
      ++count;
#pragma unroll
  for (int i = 3; i >= 0; --i) {
    const double w = inverse[i];
    if (w > 0.0 && w < vc::kSeamInv && count < kMaxPoses && pose_from_root(g, fw, side, n, dd, w, true, out + 12 * count))
      ++count;
  }
  clean = !doubtful;
  return count;
}

// |R X + t|: the depth of the world point X along its unit ray under the pose at `pose`.
__host__ __device__ __forceinline__ double depth_under(const double* pose, const double (&X)[3]) {
  double c[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) c[i] = pose[3 * i] * X[0] + pose[3 * i + 1] * X[1] + pose[3 * i + 2] * X[2] + pose[9 + i];
  return sqrt(dot3(c, c));
}

// Three 2D-3D correspondences (normalised image points (x, y), world points g.X filled by the caller) -> up to four poses at
// `out` (12 doubles each), ascending in u = s2 / s1; -> their number.  The elimination of v fails where two solutions share
// their u: D(u) = 2 (c23 u - c13) vanishes at a solution exactly when the third ray is perpendicular to the side between the
// first two points in the camera frame, N vanishes with it, the line u = const lies in the conics' difference and meets each
// conic twice, so the quartic has a double root there (no sign change) and v = 0 / 0.  Which point is the third is a choice:
// when a labelling's result is not clean the points are rotated (2 3 1, then 3 1 2), under which the same poses have other
// (u, v), until one is clean; the last one stands when none is.  The poses do not depend on the labelling, their order does:
// after a rotation they are sorted by the depth ratio of the points the caller calls second and first.
// `load(turn, x, y, g)` fills x, y and g.X with the problem's points turned `turn` times (0: as the caller labels them; 1:
// 2 3 1; 2: 3 1 2).  One loop that is not unrolled, so the elimination exists once in the kernel and nothing of the problem has
// to stay in registers through it: the kernel's loader reads the points again.
template <typename Load>
__host__ __device__ __forceinline__ int solve_p3p_turning(const Load& load, Triangle& g, double* out) {
  int count = 0, turn = 0;
#pragma unroll 1
  for (;; ++turn) {
    double x[3], y[3];
    load(turn, x, y, g);
    bool clean;
    count = solve_labelled(x, y, g, out, clean);
    if (clean || turn == 2) break;
  }
  if (turn == 0) return count;
  double X0[3], X1[3];                                       // the caller's first and second point: after one turn in slots 2 and 0
#pragma unroll
  for (int k = 0; k < 3; ++k) X0[k] = turn == 1 ? g.X[2][k] : g.X[1][k], X1[k] = turn == 1 ? g.X[0][k] : g.X[2][k];
  // insertion sort of at most four poses by u under the caller's labelling
  for (int i = 1; i < count; ++i)
    for (int j = i; j > 0; --j) {
      double* a = out + 12 * (j - 1);
      double* b = out + 12 * j;
      if (!(depth_under(b, X1) * depth_under(a, X0) < depth_under(a, X1) * depth_under(b, X0))) break;
      for (int k = 0; k < 12; ++k) {
        const double v = a[k];
        a[k] = b[k], b[k] = v;
      }
    }
  return count;
}

// The problem in arrays (the host programs): x, y and world (3, 3).
struct ArrayLoad {
  const double* x;
  const double* y;
  const double* world;
  __host__ __device__ void operator()(int turn, double (&xo)[3], double (&yo)[3], Triangle& g) const {
    for (int i = 0; i < 3; ++i) {
      const int k = (i + turn) % 3;
      xo[i] = x[k], yo[i] = y[k];
      for (int c = 0; c < 3; ++c) g.X[i][c] = world[3 * k + c];
    }
  }
};

// solve_p3p_turning on a problem in arrays, g.X filled by the caller: what the host programs call.
__host__ __device__ __forceinline__ int solve_p3p(const double (&x)[3], const double (&y)[3], Triangle& g, double* out) {
  double world[9];
  for (int i = 0; i < 9; ++i) world[i] = g.X[i / 3][i % 3];
  return solve_p3p_turning(ArrayLoad{x, y, world}, g, out);
}

struct Correspondences { const double* __restrict__ rays_n; const double* __restrict__ xyz; };   // normalised (x, y); world points

struct P3P {
  static constexpr int kSample = 3, kMaxSolutions = kMaxPoses, kWidth = 12, kWorkDoubles = 0;
  using Data = Correspondences;
  static bool usable(Data d) { return d.rays_n && d.xyz; }
  static __device__ __forceinline__ int solve(Data d, long long lo, const int (&s)[3], double*, int, double* out) {
    Triangle g;
    return solve_p3p_turning(SampleLoad{d, lo, s[0], s[1], s[2]}, g, out);
  }
  struct SampleLoad {                                        // reads the sample's points from memory, turned by selects on the indices
    Data d;
    long long lo;
    int s0, s1, s2;
    __device__ __forceinline__ void operator()(int turn, double (&x)[3], double (&y)[3], Triangle& g) const {
      const int idx[3] = {turn == 0 ? s0 : turn == 1 ? s1 : s2, turn == 0 ? s1 : turn == 1 ? s2 : s0, turn == 0 ? s2 : turn == 1 ? s0 : s1};
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const double* r = d.rays_n + (lo + idx[i]) * 2;
        const double* w = d.xyz + (lo + idx[i]) * 3;
        x[i] = r[0], y[i] = r[1];
        g.X[i][0] = w[0], g.X[i][1] = w[1], g.X[i][2] = w[2];
      }
    }
  };
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
