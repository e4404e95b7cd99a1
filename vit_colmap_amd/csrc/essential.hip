// Calibrated two-view geometry, the minimal solver (gfx950): every real essential matrix through five correspondences,
// for many hypotheses of many image pairs at once.  The hypotheses feed vc_two_view_score as pixel
// fundamental matrices; sampling, scoring and the decision rule stay where they are for F and H
// (vit_colmap_amd/matching/essential.py, two_view.py).  Specification: tests/util_essential.py, which solves the same
// problem by the Stewénius action matrix and numpy's eigensolver; this kernel takes Nistér's route, so that the two agree
// is a test of both.  All arithmetic is float64.
//
// One hypothesis per lane, one wave per workgroup, no barrier.  Per lane:
//   1. null space   Householder QR of the 9x5 matrix of epipolar equations; the last four columns of Q are an orthonormal
//                   basis X, Y, Z, W of the E with x2' E x1 = 0, and E = xX + yY + zZ + W
//   2. constraints  det E = 0 and 2 E E' E - tr(E E') E = 0: ten cubics in x, y, z, a 10x20 matrix in Nistér's column order
//   3. elimination  Gauss-Jordan with partial pivoting on the first ten columns; every loop is fully unrolled, every index a
//                   compile-time constant and a row exchange a pair of selects, so the matrix has no run-time index
//   4. polynomial   rows e..j give a 3x3 matrix B(z) of polynomials with B(z) (x, y, 1)' = 0; det B(z) has degree 10
//   5. real roots   in [-e, e] for the polynomial and, for |z| > e, in (-1 / e, 1 / e) for its reversal in w = 1 / z (e just
//                   above 1, so that a root at |z| = 1 lies inside the first range: minimal_solver.h kSeamEnd); the roots of
//                   the k-th derivative bracket those of the (k-1)-th, each bracket is bisected at most 64 times
//   6. back-substitution  (x, y, 1) is the null vector of B(z) (the largest cross product of two rows); at most three
//                   Gauss-Newton steps on the ten constraints themselves, evaluated on the orthonormal basis, take out the
//                   rounding of the elimination and of the polynomial's coefficients; E is scaled to unit Frobenius norm
// The run-time indexed arrays of step 5 (52 doubles per lane) live in LDS, lane-interleaved, 26 KiB per workgroup.
// Every loop has a constant trip count but the bisection and the polish, which are capped (vc::kBisections, kPolish).
// The kernel around solve_five_point and the pieces of the root bracketing are those of minimal_solver.h, shared with P3P.
// The solver functions are __host__ __device__: tools/five_point_host.cpp includes this file and calls solve_five_point on one
// problem after another (stride 1 for the work area); tests/test_solver_host.py compares that program with the specification.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/vitcolmap_hip.h"
#include "minimal_solver.h"

namespace {

constexpr int kMaxSolutions = 10;
constexpr int kPolish = 3;
constexpr int kWorkDoubles = 11 + 11 + 10 + 10 + 10; // polynomial, one derivative's coefficients, three root lists
constexpr double kRankTol = 1e-12;                   // relative: a column of the 9x5 system inside the span of the others
constexpr double kPivotTol = 1e-13;                  // absolute: the constraint matrix is built from an orthonormal basis

// Linear forms are over (x, y, z, 1); quadratics over xx xy xz x yy yz y zz z 1; cubics in Nistér's column order
//   x3 y3 x2y xy2 x2z x2 y2z y2 xyz xy | xz2 xz x yz2 yz y z3 z2 z 1

// out (quadratic) += sign * a * b
__host__ __device__ __forceinline__ void mul_ll(double (&out)[10], const double (&a)[4], const double (&b)[4], double sign) {
  constexpr int ll[4][4] = {{0, 1, 2, 3}, {1, 4, 5, 6}, {2, 5, 7, 8}, {3, 6, 8, 9}};
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) out[ll[i][j]] += sign * (a[i] * b[j]);
}

// out (cubic) += q * a
__host__ __device__ __forceinline__ void mul_ql(double (&out)[20], const double (&q)[10], const double (&a)[4]) {
  constexpr int ql[10][4] = {{0, 2, 4, 5},    {2, 3, 8, 9},    {4, 8, 10, 11},   {5, 9, 11, 12},   {3, 1, 6, 7},
                              {8, 6, 13, 14},  {9, 7, 14, 15},  {10, 13, 16, 17}, {11, 14, 17, 18}, {12, 15, 18, 19}};
#pragma unroll
  for (int i = 0; i < 10; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) out[ql[i][j]] += q[i] * a[j];
}

// Orthonormal basis of the null space of the five epipolar equations -> n[v][k]: entry k of basis matrix v.
__host__ __device__ __forceinline__ bool null_space(const double (&x1)[5], const double (&y1)[5], const double (&x2)[5],
                                                    const double (&y2)[5], double (&n)[4][9]) {
  double a[9][5], beta[5];
  double scale = 0.0;
#pragma unroll
  for (int c = 0; c < 5; ++c) {
    a[0][c] = x2[c] * x1[c], a[1][c] = x2[c] * y1[c], a[2][c] = x2[c];
    a[3][c] = y2[c] * x1[c], a[4][c] = y2[c] * y1[c], a[5][c] = y2[c];
    a[6][c] = x1[c], a[7][c] = y1[c], a[8][c] = 1.0;
    double s = 0.0;
#pragma unroll
    for (int r = 0; r < 9; ++r) s += a[r][c] * a[r][c];
    scale = fmax(scale, s);
  }
  scale = sqrt(scale);
  bool ok = scale < INFINITY;                               // false for NaN too
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    double s = 0.0;
#pragma unroll
    for (int r = k; r < 9; ++r) s += a[r][k] * a[r][k];
    const double nrm = sqrt(s);
    ok = ok && nrm > kRankTol * scale;
    const double alpha = a[k][k] > 0.0 ? -nrm : nrm;
    const double vk = a[k][k] - alpha;
    beta[k] = 2.0 / (s - a[k][k] * a[k][k] + vk * vk);
    a[k][k] = vk;                                           // column k now holds the Householder vector, rows k..8
#pragma unroll
    for (int j = k + 1; j < 5; ++j) {
      double d = 0.0;
#pragma unroll
      for (int r = k; r < 9; ++r) d += a[r][k] * a[r][j];
      d *= beta[k];
#pragma unroll
      for (int r = k; r < 9; ++r) a[r][j] -= d * a[r][k];
    }
  }
#pragma unroll
  for (int v = 0; v < 4; ++v) {                             // Q e_(5 + v) = H0 H1 H2 H3 H4 e_(5 + v)
#pragma unroll
    for (int r = 0; r < 9; ++r) n[v][r] = r == 5 + v ? 1.0 : 0.0;
#pragma unroll
    for (int k = 4; k >= 0; --k) {
      double d = 0.0;
#pragma unroll
      for (int r = k; r < 9; ++r) d += a[r][k] * n[v][r];
      d *= beta[k];
#pragma unroll
      for (int r = k; r < 9; ++r) n[v][r] -= d * a[r][k];
    }
  }
  return ok;
}

// The ten cubic constraints on E = x n[0] + y n[1] + z n[2] + n[3], one per row of m.
__host__ __device__ __forceinline__ void constraints(const double (&n)[4][9], double (&m)[10][20]) {
  double e[9][4];                                           // entry k of E as a linear form
#pragma unroll
  for (int k = 0; k < 9; ++k)
#pragma unroll
    for (int v = 0; v < 4; ++v) e[k][v] = n[v][k];
#pragma unroll
  for (int r = 0; r < 10; ++r)
#pragma unroll
    for (int c = 0; c < 20; ++c) m[r][c] = 0.0;
  // lam = E E' - tr(E E') / 2 I, symmetric: lam[i][j] for i <= j
  double lam[3][3][10];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = i; j < 3; ++j) {
#pragma unroll
      for (int t = 0; t < 10; ++t) lam[i][j][t] = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) mul_ll(lam[i][j], e[3 * i + k], e[3 * j + k], 1.0);
    }
#pragma unroll
  for (int t = 0; t < 10; ++t) {
    const double half_tr = 0.5 * (lam[0][0][t] + lam[1][1][t] + lam[2][2][t]);
    lam[0][0][t] -= half_tr, lam[1][1][t] -= half_tr, lam[2][2][t] -= half_tr;
  }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int k = 0; k < 3; ++k) mul_ql(m[3 * i + j], i <= k ? lam[i][k] : lam[k][i], e[3 * k + j]);
  // det E by the first row's cofactors
  double c0[10], c1[10], c2[10];
#pragma unroll
  for (int t = 0; t < 10; ++t) c0[t] = c1[t] = c2[t] = 0.0;
  mul_ll(c0, e[4], e[8], 1.0), mul_ll(c0, e[5], e[7], -1.0);
  mul_ll(c1, e[5], e[6], 1.0), mul_ll(c1, e[3], e[8], -1.0);
  mul_ll(c2, e[3], e[7], 1.0), mul_ll(c2, e[4], e[6], -1.0);
  mul_ql(m[9], c0, e[0]), mul_ql(m[9], c1, e[1]), mul_ql(m[9], c2, e[2]);
}

// Gauss-Jordan on columns 0..9 with partial pivoting.  Rows 0..3 (x3, y3, x2y, xy2) are only eliminated forwards: the
// polynomial needs rows 4..9 alone.  False for a pivot below kPivotTol.
__host__ __device__ __forceinline__ bool eliminate(double (&m)[10][20]) {
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 10; ++c) {
#pragma unroll
    for (int r = c + 1; r < 10; ++r) {                      // the largest |entry| of column c moves up to row c
      const bool sw = fabs(m[r][c]) > fabs(m[c][c]);
#pragma unroll
      for (int j = c; j < 20; ++j) {
        const double u = m[c][j], w = m[r][j];
        m[c][j] = sw ? w : u;
        m[r][j] = sw ? u : w;
      }
    }
    ok = ok && fabs(m[c][c]) > kPivotTol;
    const double inv = 1.0 / m[c][c];
#pragma unroll
    for (int j = c + 1; j < 20; ++j) m[c][j] *= inv;
#pragma unroll
    for (int r = 4; r < 10; ++r) {
      if (r == c || (c < 4 && r <= c)) continue;
      const double f = m[r][c];
#pragma unroll
      for (int j = c + 1; j < 20; ++j) m[r][j] -= f * m[c][j];
    }
#pragma unroll
    for (int r = c + 1; r < 4; ++r) {
      const double f = m[r][c];
#pragma unroll
      for (int j = c + 1; j < 20; ++j) m[r][j] -= f * m[c][j];
    }
  }
  return ok;
}

// Rows (p, q) of the eliminated matrix, p the row of a monomial u z and q the row of u: <p> - z <q> has no term in u and
// reads  bx(z) x + by(z) y + b1(z) = 0  with deg bx = deg by = 3 and deg b1 = 4 (coefficients from the constant up).
__host__ __device__ __forceinline__ void b_row(const double (&p)[20], const double (&q)[20], double (&bx)[4], double (&by)[4],
                                               double (&b1)[5]) {
  bx[0] = p[12], bx[1] = p[11] - q[12], bx[2] = p[10] - q[11], bx[3] = -q[10];
  by[0] = p[15], by[1] = p[14] - q[15], by[2] = p[13] - q[14], by[3] = -q[13];
  b1[0] = p[19], b1[1] = p[18] - q[19], b1[2] = p[17] - q[18], b1[3] = p[16] - q[17], b1[4] = -q[16];
}

template <int NA, int NB>
__host__ __device__ __forceinline__ void poly_fma(double (&out)[NA + NB - 1], const double (&a)[NA], const double (&b)[NB], double sign) {
#pragma unroll
  for (int i = 0; i < NA; ++i)
#pragma unroll
    for (int j = 0; j < NB; ++j) out[i + j] += sign * (a[i] * b[j]);
}

// Run-time indexed per-lane storage: element i of a list lives at p[i * stride] (stride 64 in LDS, 1 on the host).
struct Strided {
  double* p;
  int stride;
  __host__ __device__ __forceinline__ double& operator[](int i) const { return p[i * stride]; }
};

// The polynomial's coefficients from the constant up, or those of its reversal.
struct Poly10 {
  Strided a;
  bool reversed;
  __host__ __device__ __forceinline__ double operator[](int i) const { return reversed ? a[10 - i] : a[i]; }
};

// The real roots in [-e, e], e = vc::kSeamEnd just above 1 (see there), of sum a[i] t^i (reversed: of sum a[10 - i] t^i),
// ascending, into the list the function returns through `roots`; -> their number.  Level k works on the k-th derivative over k!,
// whose coefficients are a[i + k] binomial(i + k, k); its roots in [-e, e] and the two ends split the interval into pieces on which the
// (k - 1)-th derivative is monotone, so a sign change at the ends of a piece brackets exactly one root.
__host__ __device__ __forceinline__ int real_roots_unit(const Poly10 a, const Strided coef, Strided prev, Strided cur, Strided* roots) {
  int n_prev = 0;
  for (int k = 9; k >= 0; --k) {
    const int degree = 10 - k;
    vc::derivative_coefficients(coef, degree, k, a);
    int n_cur = 0;
    double lo = -vc::kSeamEnd, f_lo = vc::horner(coef, degree, lo);
    for (int s = 0; s <= n_prev; ++s) {
      const double hi = s < n_prev ? prev[s] : vc::kSeamEnd;
      const double f_hi = vc::horner(coef, degree, hi);
      const double root = vc::root_of_piece(coef, degree, lo, hi, f_lo, f_hi);
      if (root == root && n_cur < kMaxSolutions) cur[n_cur++] = root;
      lo = hi, f_lo = f_hi;
    }
    const Strided t = prev;
    prev = cur, cur = t, n_prev = n_cur;
  }
  *roots = prev;
  return n_prev;
}

// B at t, for the direct polynomials (t = z) or the reversed ones (t = w = 1 / z, the columns of B scaled by w^3, w^3, w^4,
// which keeps every quantity bounded for |z| > 1).
__host__ __device__ __forceinline__ void eval_b(const double (&bx)[3][4], const double (&by)[3][4], const double (&b1)[3][5], double t,
                                                bool reversed, double (&b)[3][3]) {
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    double v0 = 0.0, v1 = 0.0, v2 = 0.0;
#pragma unroll
    for (int k = 4; k >= 0; --k) v2 = v2 * t + (reversed ? b1[r][4 - k] : b1[r][k]);
#pragma unroll
    for (int k = 3; k >= 0; --k) {
      v0 = v0 * t + (reversed ? bx[r][3 - k] : bx[r][k]);
      v1 = v1 * t + (reversed ? by[r][3 - k] : by[r][k]);
    }
    b[r][0] = v0, b[r][1] = v1, b[r][2] = v2;
  }
}

// c = op(a) op(b) for row-major 3x3 matrices; TA / TB transpose the operand.
template <bool TA, bool TB>
__host__ __device__ __forceinline__ void mul3(const double (&a)[9], const double (&b)[9], double (&c)[9]) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double v = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) v += (TA ? a[3 * k + i] : a[3 * i + k]) * (TB ? b[3 * j + k] : b[3 * k + j]);
      c[3 * i + j] = v;
    }
}

__host__ __device__ __forceinline__ void cofactors(const double (&e)[9], double (&c)[9]) {
  c[0] = e[4] * e[8] - e[5] * e[7], c[1] = e[5] * e[6] - e[3] * e[8], c[2] = e[3] * e[7] - e[4] * e[6];
  c[3] = e[2] * e[7] - e[1] * e[8], c[4] = e[0] * e[8] - e[2] * e[6], c[5] = e[1] * e[6] - e[0] * e[7];
  c[6] = e[1] * e[5] - e[2] * e[4], c[7] = e[2] * e[3] - e[0] * e[5], c[8] = e[0] * e[4] - e[1] * e[3];
}

// The ten constraints at a numeric E: r[0..8] = E E' E - tr(E E') / 2 E, r[9] = det E; -> |r|^2.
__host__ __device__ __forceinline__ double residual(const double (&e)[9], double (&r)[10]) {
  double eet[9], t[9];
  mul3<false, true>(e, e, eet);
  mul3<false, false>(eet, e, t);
  const double half_tr = 0.5 * (eet[0] + eet[4] + eet[8]);
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < 9; ++k) r[k] = t[k] - half_tr * e[k], s += r[k] * r[k];
  r[9] = e[0] * (e[4] * e[8] - e[5] * e[7]) + e[1] * (e[5] * e[6] - e[3] * e[8]) + e[2] * (e[3] * e[7] - e[4] * e[6]);
  return s + r[9] * r[9];
}

// Gauss-Newton on the ten constraints themselves for E = h0 g0 + h1 g1 + h2 g2 + g3: at most kPolish steps, each kept only
// if it lowers the residual.  The polynomial's roots carry the rounding of the elimination and of three polynomial
// products; the constraints evaluated on the orthonormal basis do not.
__host__ __device__ __forceinline__ void polish(const double (&g)[4][9], double (&h)[3]) {
  double e[9], r[10];
#pragma unroll
  for (int k = 0; k < 9; ++k) e[k] = h[0] * g[0][k] + h[1] * g[1][k] + h[2] * g[2][k] + g[3][k];
  double res = residual(e, r);
  for (int it = 0; it < kPolish; ++it) {
    double ete[9], eet[9], cof[9], jac[3][10];
    mul3<true, false>(e, e, ete);
    mul3<false, true>(e, e, eet);
    cofactors(e, cof);
    const double half_tr = 0.5 * (eet[0] + eet[4] + eet[8]);
#pragma unroll
    for (int v = 0; v < 3; ++v) {                           // d/dh_v: G E'E + E G'E + E E'G - tr(G E') E - tr(E E') / 2 G; tr(adj(E) G)
      double t0[9], t1[9], t2[9], t3[9], dot = 0.0, ddet = 0.0;
      mul3<false, false>(g[v], ete, t0);
      mul3<true, false>(g[v], e, t1);
      mul3<false, false>(e, t1, t2);
      mul3<false, false>(eet, g[v], t3);
#pragma unroll
      for (int k = 0; k < 9; ++k) dot += g[v][k] * e[k], ddet += cof[k] * g[v][k];
#pragma unroll
      for (int k = 0; k < 9; ++k) jac[v][k] = t0[k] + t2[k] + t3[k] - dot * e[k] - half_tr * g[v][k];
      jac[v][9] = ddet;
    }
    double n00 = 0.0, n01 = 0.0, n02 = 0.0, n11 = 0.0, n12 = 0.0, n22 = 0.0, g0 = 0.0, g1 = 0.0, g2 = 0.0;
#pragma unroll
    for (int k = 0; k < 10; ++k) {
      n00 += jac[0][k] * jac[0][k], n01 += jac[0][k] * jac[1][k], n02 += jac[0][k] * jac[2][k];
      n11 += jac[1][k] * jac[1][k], n12 += jac[1][k] * jac[2][k], n22 += jac[2][k] * jac[2][k];
      g0 += jac[0][k] * r[k], g1 += jac[1][k] * r[k], g2 += jac[2][k] * r[k];
    }
    const double a00 = n11 * n22 - n12 * n12, a01 = n02 * n12 - n01 * n22, a02 = n01 * n12 - n02 * n11;
    const double a11 = n00 * n22 - n02 * n02, a12 = n01 * n02 - n00 * n12, a22 = n00 * n11 - n01 * n01;
    const double inv = -1.0 / (n00 * a00 + n01 * a01 + n02 * a02);
    const double q0 = h[0] + inv * (a00 * g0 + a01 * g1 + a02 * g2);
    const double q1 = h[1] + inv * (a01 * g0 + a11 * g1 + a12 * g2);
    const double q2 = h[2] + inv * (a02 * g0 + a12 * g1 + a22 * g2);
    double en[9], rn[10];
#pragma unroll
    for (int k = 0; k < 9; ++k) en[k] = q0 * g[0][k] + q1 * g[1][k] + q2 * g[2][k] + g[3][k];
    const double resn = residual(en, rn);
    if (!(resn < res)) break;                               // also for a NaN step
    h[0] = q0, h[1] = q1, h[2] = q2, res = resn;
#pragma unroll
    for (int k = 0; k < 9; ++k) e[k] = en[k];
#pragma unroll
    for (int k = 0; k < 10; ++k) r[k] = rn[k];
  }
}

// One solution from a root t of det B.  (x, y, 1) ~ u, the null vector of B(t): the largest cross product of two rows.
//   direct:   (x, y, 1) ~ u             -> E ~ u0 X + u1 Y + u2 z Z + u2 W
//   reversed: (x z^3, y z^3, z^4) ~ u   -> E ~ u0 X + u1 Y + u2 Z + u2 w W
// The largest of the four coefficients is fixed to 1 and the other three are polished; E is scaled to unit Frobenius norm.
// -> false when the matrix is not finite.
__host__ __device__ __forceinline__ bool back_substitute(const double (&bx)[3][4], const double (&by)[3][4], const double (&b1)[3][5],
                                                         const double (&n)[4][9], double t, bool reversed, double* out) {
  double b[3][3];
  eval_b(bx, by, b1, t, reversed, b);
  double u[3] = {0.0, 0.0, 0.0}, best = -1.0;
#pragma unroll
  for (int r = 0; r < 3; ++r) {                             // rows (0, 1), (1, 2), (2, 0)
    const int s = (r + 1) % 3;
    const double c0 = b[r][1] * b[s][2] - b[r][2] * b[s][1];
    const double c1 = b[r][2] * b[s][0] - b[r][0] * b[s][2];
    const double c2 = b[r][0] * b[s][1] - b[r][1] * b[s][0];
    const double nn = c0 * c0 + c1 * c1 + c2 * c2;
    const bool take = nn > best;
    u[0] = take ? c0 : u[0], u[1] = take ? c1 : u[1], u[2] = take ? c2 : u[2];
    best = take ? nn : best;
  }
  const double c[4] = {u[0], u[1], reversed ? u[2] : u[2] * t, reversed ? u[2] * t : u[2]};
  int big = 0;
  double cbig = c[0];
#pragma unroll
  for (int v = 1; v < 4; ++v) {
    const bool larger = fabs(c[v]) > fabs(cbig);
    big = larger ? v : big, cbig = larger ? c[v] : cbig;
  }
  // the basis with matrix `big` moved to the end, by selects
  double g[4][9], h[3];
#pragma unroll
  for (int v = 0; v < 3; ++v) h[v] = (v == big ? c[3] : c[v]) / cbig;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
#pragma unroll
    for (int v = 0; v < 3; ++v) g[v][k] = v == big ? n[3][k] : n[v][k];
    g[3][k] = big == 0 ? n[0][k] : big == 1 ? n[1][k] : big == 2 ? n[2][k] : n[3][k];
  }
  const bool usable = fabs(h[0]) <= 1.0 && fabs(h[1]) <= 1.0 && fabs(h[2]) <= 1.0;      // false for NaN
  if (!usable) return false;
  polish(g, h);
  double e[9], s = 0.0;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    e[k] = h[0] * g[0][k] + h[1] * g[1][k] + h[2] * g[2][k] + g[3][k];
    s += e[k] * e[k];
  }
  const double inv = 1.0 / sqrt(s);
  bool finite = s > 0.0 && inv < INFINITY;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    e[k] *= inv;
    finite = finite && fabs(e[k]) <= 2.0;                   // false for NaN
  }
  if (!finite) return false;
#pragma unroll
  for (int k = 0; k < 9; ++k) out[k] = e[k];
  return true;
}

// Five correspondences -> up to ten matrices at out_e (each 9 doubles, row-major), ascending in the root z of the
// polynomial; -> their number.  `work` holds kWorkDoubles strided doubles.
__host__ __device__ __forceinline__ int solve_five_point(const double (&x1)[5], const double (&y1)[5], const double (&x2)[5],
                                                         const double (&y2)[5], double* work, int stride, double* out_e) {
  double n[4][9];
  if (!null_space(x1, y1, x2, y2, n)) return 0;
  double bx[3][4], by[3][4], b1[3][5];
  {
    double m[10][20];
    constraints(n, m);
    if (!eliminate(m)) return 0;
    b_row(m[4], m[5], bx[0], by[0], b1[0]);
    b_row(m[6], m[7], bx[1], by[1], b1[1]);
    b_row(m[8], m[9], bx[2], by[2], b1[2]);
  }
  const Strided poly{work, stride}, coef{work + 11 * stride, stride}, mid{work + 22 * stride, stride};
  const Strided r0{work + 32 * stride, stride}, r1{work + 42 * stride, stride};
  {
    // det B = (bx0 by1 - by0 bx1) b1_2 + (by0 b1_1 - b1_0 by1) bx2 + (b1_0 bx1 - bx0 b1_1) by2
    double p[11], m01[7], m12[8], m20[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) m12[i] = m20[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 7; ++i) m01[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 11; ++i) p[i] = 0.0;
    poly_fma<4, 4>(m01, bx[0], by[1], 1.0), poly_fma<4, 4>(m01, by[0], bx[1], -1.0);
    poly_fma<4, 5>(m12, by[0], b1[1], 1.0), poly_fma<5, 4>(m12, b1[0], by[1], -1.0);
    poly_fma<5, 4>(m20, b1[0], bx[1], 1.0), poly_fma<4, 5>(m20, bx[0], b1[1], -1.0);
    poly_fma<7, 5>(p, m01, b1[2], 1.0), poly_fma<8, 4>(p, m12, bx[2], 1.0), poly_fma<8, 4>(p, m20, by[2], 1.0);
    double big = 0.0;
#pragma unroll
    for (int i = 0; i < 11; ++i) big = fmax(big, fabs(p[i]));
    if (!(big > 0.0 && big < INFINITY)) return 0;
#pragma unroll
    for (int i = 0; i < 11; ++i) poly[i] = p[i] / big;
  }
  Strided roots{nullptr, stride};
  const int n_dir = real_roots_unit({poly, false}, coef, r0, r1, &roots);
  for (int i = 0; i < n_dir; ++i) mid[i] = roots[i];
  const int n_rev = real_roots_unit({poly, true}, coef, r0, r1, &roots);
  // ascending z: the roots below -e (w in (-1 / e, 0), descending), those in [-e, e], those above e (w in (0, 1 / e), descending)
  int count = 0;
  for (int i = n_rev - 1; i >= 0; --i) {
    const double w = roots[i];
    if (w < 0.0 && w > -vc::kSeamInv && count < kMaxSolutions && back_substitute(bx, by, b1, n, w, true, out_e + 9 * count)) ++count;
  }
  for (int i = 0; i < n_dir; ++i)
    if (count < kMaxSolutions && back_substitute(bx, by, b1, n, mid[i], false, out_e + 9 * count)) ++count;
  for (int i = n_rev - 1; i >= 0; --i) {
    const double w = roots[i];
    if (w > 0.0 && w < vc::kSeamInv && count < kMaxSolutions && back_substitute(bx, by, b1, n, w, true, out_e + 9 * count)) ++count;
  }
  return count;
}

struct Matches { const double* __restrict__ pts_n; };       // normalised x1 y1 x2 y2 per correspondence

struct FivePoint {
  static constexpr int kSample = 5, kMaxSolutions = ::kMaxSolutions, kWidth = 9, kWorkDoubles = ::kWorkDoubles;
  using Data = Matches;
  static bool usable(Data d) { return d.pts_n; }
  static __device__ __forceinline__ int solve(Data d, long long lo, const int (&s)[5], double* work, int stride, double* out) {
    double x1[5], y1[5], x2[5], y2[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      const double* q = d.pts_n + (lo + s[i]) * 4;
      x1[i] = q[0], y1[i] = q[1], x2[i] = q[2], y2[i] = q[3];
    }
    return solve_five_point(x1, y1, x2, y2, work, stride, out);
  }
};

}  // namespace

extern "C" {

int vc_essential_5pt(const double* pts_n, const int32_t* offsets, int n_pairs, const int32_t* samples, int n_hyp,
                     double* out_E, int32_t* out_count, vc_stream_t stream) {
  return vc::launch_minimal_solver<FivePoint>({pts_n}, offsets, n_pairs, samples, n_hyp, out_E, out_count, stream);
}

}  // extern "C"
