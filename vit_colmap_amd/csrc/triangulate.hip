// Track triangulation (gfx950): one 3D point per track of observations under known camera poses, every
// track of a call in one launch.  vc_triangulate_tracks is what a mapper repeats after every registration round
// (vit_colmap_amd/mapping/grow.py).  Specification: tests/util_mapper.py (`triangulate_track`).  This build's own published
// rule; parity with COLMAP's triangulator is unpinned.
//
// float64, one track per lane, one wave per workgroup, no LDS, no barrier, no atomics.  Per track of n observations:
//   1. hypotheses   pairs (p, q), p < q, of observation indices: every pair in lexicographic order while n (n - 1) / 2 <= 64,
//                   otherwise 64 pairs drawn by the published hash (lowbias32, the sampler's constants, SALT_T)
//   2. one of them  the midpoint of the two rays (§4.2g between two arbitrary cameras) with positive depths on both and
//                   enough parallax at the point; counted over every usable observation by the division-free pixel test of
//                   §4.2i in float64; it counts only if p and q are inliers themselves; most inliers win, the lowest index on ties
//   3. refit        at most kRefitSteps Gauss-Newton steps on X over the winner's inliers, 3x3 normal equations accumulated in
//                   observation order and solved by the adjugate; a step is kept only if it lowers the cost, the first one
//                   not kept ends it; the refit is taken iff it is finite and has no fewer inliers
//   4. acceptance   at least two inliers, of which some pair passes the parallax test at the final X
// Nothing is kept per observation: an observation and its camera row are read again wherever they are needed (a track is
// short and its rows stay in cache), so a lane holds three observations at most and no array has a run-time index.  Every
// loop but those over observations, hypotheses and refit steps is fully unrolled.  Angles are tested without trigonometry
// and the only library call is sqrt, so the host build of triangulate_track (tools/triangulate_host.cpp includes this file)
// and the device agree; what a lane computes is sequential, so two launches return the same bits.
//
// vc_split_tracks (specification: tests/util_split.py, `split_component`) runs the same steps on a component of
// the match graph that holds more than one scene point: a step counts, in every run of nodes of one camera, only the free inlier
// nearest the point (Selection) where the other two entry points count every inlier (Inliers); the points a component has
// already attach their selection, then one point per empty slot is peeled off the nodes that are still free.  count_set,
// refit_cost, refit and settle (steps 3 and 4) are written once over either set.  The labels live in global memory, which
// slots were occupied is a bit mask, so here too no array of a lane has a run-time index.  tools/split_tracks_host.cpp is the host build.
//
// vc_refine_tracks (specification: tests/util_rounds.py, `refine_track`) is steps 3 and 4 from a point the
// track has already: after a bundle adjustment moved the poses, the inliers of that point over every usable observation
// take the winner's place.  finish_track is the tail it shares with vc_triangulate_tracks; tools/refine_tracks_host.cpp is its host build.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/vitcolmap_hip.h"
#include "common.h"

namespace {

constexpr int kTriWave = 64;
constexpr int kTriMaxHypotheses = 64;
constexpr int kRefitSteps = 10;                 // TRI_REFIT_STEPS
constexpr uint32_t kSaltT = 0xC3C3C3C3u;        // SALT["T"] of matching/_common.py

struct Tracks {
  const double* __restrict__ obs_xy;
  const int32_t* __restrict__ obs_cam;
  const double* __restrict__ cams;
  int n_cams;
};

// One observation with its camera: R row-major, t, fx, fy, cx, cy (X_cam = R X + t), the pixel (u, v).
struct View {
  double R[9], t[3], fx, fy, cx, cy, u, v;
  bool ok;
};

__host__ __device__ __forceinline__ uint32_t lowbias32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7FEB352Du;
  x ^= x >> 15;
  x *= 0x846CA68Bu;
  x ^= x >> 16;
  return x;
}

__host__ __device__ __forceinline__ bool is_finite(double x) { return fabs(x) < INFINITY; }   // false for NaN

// Observation i of the call.  Unusable (ok = false): a slot outside [0, n_cams), a camera row or a pixel that is not finite.
__host__ __device__ __forceinline__ void load_view(const Tracks& d, long long i, View& w) {
  const int slot = d.obs_cam[i];
  w.ok = slot >= 0 && slot < d.n_cams;
  const double* c = d.cams + (long long)(w.ok ? slot : 0) * 16;
  double row[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    row[k] = w.ok ? c[k] : NAN;
    w.ok = w.ok && is_finite(row[k]);
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) w.R[k] = row[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) w.t[k] = row[9 + k];
  w.fx = row[12], w.fy = row[13], w.cx = row[14], w.cy = row[15];
  w.u = d.obs_xy[2 * i], w.v = d.obs_xy[2 * i + 1];
  w.ok = w.ok && is_finite(w.u) && is_finite(w.v);
}

__host__ __device__ __forceinline__ double dot3(const double (&a)[3], const double (&b)[3]) {
  return a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
}

__host__ __device__ __forceinline__ void centre_of(const View& w, double (&c)[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) c[k] = -(w.R[k] * w.t[0] + w.R[3 + k] * w.t[1] + w.R[6 + k] * w.t[2]);
}

// The ray of a view in the world: direction d = R' x with x = ((u - cx) / fx, (v - cy) / fy, 1), centre c = -R' t.
__host__ __device__ __forceinline__ void ray_of(const View& w, double (&d)[3], double (&c)[3]) {
  const double x = (w.u - w.cx) / w.fx, y = (w.v - w.cy) / w.fy;
#pragma unroll
  for (int k = 0; k < 3; ++k) d[k] = w.R[k] * x + w.R[3 + k] * y + w.R[6 + k];
  centre_of(w, c);
}

// The parallax at X between the centres cp and cq: the angle between X - cp and X - cq is obtuse, or tan^2 of it reaches tan2.
__host__ __device__ __forceinline__ bool parallax(const double (&X)[3], const double (&cp)[3], const double (&cq)[3], double tan2) {
  const double g[3] = {X[0] - cp[0], X[1] - cp[1], X[2] - cp[2]}, h[3] = {X[0] - cq[0], X[1] - cq[1], X[2] - cq[2]};
  const double gh = dot3(g, h);
  const double k[3] = {g[1] * h[2] - g[2] * h[1], g[2] * h[0] - g[0] * h[2], g[0] * h[1] - g[1] * h[0]};
  return gh <= 0.0 || dot3(k, k) >= tan2 * (gh * gh);       // false for NaN
}

__host__ __device__ __forceinline__ void to_camera(const View& w, const double (&X)[3], double (&Xc)[3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i) Xc[i] = w.R[3 * i] * X[0] + w.R[3 * i + 1] * X[1] + w.R[3 * i + 2] * X[2] + w.t[i];
}

// The division-free pixel test; sq: the squared pixel error times Xc_z^2.
__host__ __device__ __forceinline__ bool inlier(const View& w, const double (&X)[3], double e2, double& sq, double& z) {
  double Xc[3];
  to_camera(w, X, Xc);
  z = Xc[2];
  const double a = w.fx * Xc[0] + w.cx * z - w.u * z;
  const double b = w.fy * Xc[1] + w.cy * z - w.v * z;
  sq = a * a + b * b;
  return w.ok && z > 0.0 && sq <= e2 * (z * z);              // false for NaN
}

// Which observations of a track count at a point: `set(d, lo, n, i, w, X, sq, z)` says whether observation i, loaded as w,
// counts at X and leaves its sq and Xc_z.  Inliers is the set of vc_triangulate_tracks and vc_refine_tracks, Selection (below)
// that of vc_split_tracks; the refit and the acceptance test are written once over either.
struct Inliers {
  double e2;
  __host__ __device__ __forceinline__ bool operator()(const Tracks&, long long, int, int, const View& w, const double (&X)[3], double& sq,
                                                      double& z) const {
    return inlier(w, X, e2, sq, z);
  }
};

template <class Set>
__host__ __device__ __forceinline__ int count_set(const Tracks& d, long long lo, int n, const Set& set, const double (&X)[3]) {
  int count = 0;
  for (int i = 0; i < n; ++i) {
    View w;
    double sq, z;
    load_view(d, lo + i, w);
    count += set(d, lo, n, i, w, X, sq, z) ? 1 : 0;
  }
  return count;
}

// The midpoint of the rays of p and q -> X; false when a depth is not finite and positive or the parallax is too small.
__host__ __device__ __forceinline__ bool midpoint(const View& p, const View& q, double tan2, double (&X)[3]) {
  double dp[3], cp[3], dq[3], cq[3];
  ray_of(p, dp, cp);
  ray_of(q, dq, cq);
  const double e[3] = {cq[0] - cp[0], cq[1] - cp[1], cq[2] - cp[2]};
  const double aa = dot3(dp, dp), ab = dot3(dp, dq), bb = dot3(dq, dq), ae = dot3(dp, e), be = dot3(dq, e);
  const double det = aa * bb - ab * ab;
  const double s = (bb * ae - ab * be) / det, r = (ab * ae - aa * be) / det;
  if (!(s > 0.0 && r > 0.0 && s < INFINITY && r < INFINITY)) return false;
#pragma unroll
  for (int k = 0; k < 3; ++k) X[k] = 0.5 * (cp[k] + s * dp[k] + cq[k] + r * dq[k]);
  return parallax(X, cp, cq, tan2);
}

// Sum over the observations that count at X0 of the squared pixel error at X (the set does not move with X).
template <class Set>
__host__ __device__ __forceinline__ double refit_cost(const Tracks& d, long long lo, int n, const Set& set, const double (&X0)[3],
                                                      const double (&X)[3]) {
  double cost = 0.0;
  for (int i = 0; i < n; ++i) {
    View w;
    double sq, z, Xc[3];
    load_view(d, lo + i, w);
    if (!set(d, lo, n, i, w, X0, sq, z)) continue;
    to_camera(w, X, Xc);
    const double iz = 1.0 / Xc[2];
    const double ru = w.fx * Xc[0] * iz + w.cx - w.u, rv = w.fy * Xc[1] * iz + w.cy - w.v;
    cost += ru * ru + rv * rv;
  }
  return cost;
}

// Gauss-Newton on X over the observations that count at X0, from X0.
template <class Set>
__host__ __device__ __forceinline__ void refit(const Tracks& d, long long lo, int n, const Set& set, const double (&X0)[3], double (&X)[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) X[k] = X0[k];
  double cost = refit_cost(d, lo, n, set, X0, X);
  for (int it = 0; it < kRefitSteps; ++it) {
    double A00 = 0.0, A01 = 0.0, A02 = 0.0, A11 = 0.0, A12 = 0.0, A22 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
    for (int i = 0; i < n; ++i) {
      View w;
      double sq, z, Xc[3];
      load_view(d, lo + i, w);
      if (!set(d, lo, n, i, w, X0, sq, z)) continue;
      to_camera(w, X, Xc);
      const double iz = 1.0 / Xc[2];
      const double ru = w.fx * Xc[0] * iz + w.cx - w.u, rv = w.fy * Xc[1] * iz + w.cy - w.v;
      const double xu = Xc[0] * iz, xv = Xc[1] * iz, fu = w.fx * iz, fv = w.fy * iz;
      // d ru / d X = fx / z (R row 0 - x / z R row 2), d rv / d X = fy / z (R row 1 - y / z R row 2)
      const double ju[3] = {fu * (w.R[0] - xu * w.R[6]), fu * (w.R[1] - xu * w.R[7]), fu * (w.R[2] - xu * w.R[8])};
      const double jv[3] = {fv * (w.R[3] - xv * w.R[6]), fv * (w.R[4] - xv * w.R[7]), fv * (w.R[5] - xv * w.R[8])};
      A00 += ju[0] * ju[0] + jv[0] * jv[0], A01 += ju[0] * ju[1] + jv[0] * jv[1], A02 += ju[0] * ju[2] + jv[0] * jv[2];
      A11 += ju[1] * ju[1] + jv[1] * jv[1], A12 += ju[1] * ju[2] + jv[1] * jv[2], A22 += ju[2] * ju[2] + jv[2] * jv[2];
      b0 += ju[0] * ru + jv[0] * rv, b1 += ju[1] * ru + jv[1] * rv, b2 += ju[2] * ru + jv[2] * rv;
    }
    // the adjugate of the symmetric A
    const double c00 = A11 * A22 - A12 * A12, c01 = A02 * A12 - A01 * A22, c02 = A01 * A12 - A02 * A11;
    const double c11 = A00 * A22 - A02 * A02, c12 = A01 * A02 - A00 * A12, c22 = A00 * A11 - A01 * A01;
    const double inv = -1.0 / (A00 * c00 + A01 * c01 + A02 * c02);
    const double Xn[3] = {X[0] + inv * (c00 * b0 + c01 * b1 + c02 * b2), X[1] + inv * (c01 * b0 + c11 * b1 + c12 * b2),
                          X[2] + inv * (c02 * b0 + c12 * b1 + c22 * b2)};
    const double costn = refit_cost(d, lo, n, set, X0, Xn);
    if (!(costn < cost)) break;                              // also for a NaN step
#pragma unroll
    for (int k = 0; k < 3; ++k) X[k] = Xn[k];
    cost = costn;
  }
}

// Hypothesis h of a track of n >= 12 observations, which has more than kTriMaxHypotheses pairs -> (p, q), p < q, by the hash.
__host__ __device__ __forceinline__ void sampled_pair(uint32_t seed, int h, int n, int& p, int& q) {
  const uint32_t x = seed * 0x9E3779B1u + (uint32_t)h * 0x85EBCA6Bu + kSaltT;
  const int a = (int)(lowbias32(x) % (uint32_t)n);
  const int b = (int)(((uint32_t)a + 1u + lowbias32(x + 0xC2B2AE35u) % (uint32_t)(n - 1)) % (uint32_t)n);
  p = a < b ? a : b, q = a < b ? b : a;
}

// Hypothesis h after hypothesis h - 1 = (p, q), from p = q = 0: all pairs (0, 1), (0, 2), ... in order, or the sampled one.
__host__ __device__ __forceinline__ void next_pair(bool all_pairs, uint32_t seed, int h, int n, int& p, int& q) {
  if (all_pairs) {
    if (++q >= n) ++p, q = p + 1;
  } else {
    sampled_pair(seed, h, n, p, q);
  }
}

// Steps 3 and 4 over a set, from a point `best` at which best_count observations count (0: there is none): the refit, taken iff
// it is finite and no fewer count at it, then the acceptance.  -> how many count at the final X, 0 when they are fewer than two
// or no pair of them passes the parallax test there.
template <class Set>
__host__ __device__ __forceinline__ int settle(const Tracks& d, long long lo, int n, const Set& set, const double (&best)[3],
                                               int best_count, double tan2, double (&X)[3]) {
  int count = best_count;
#pragma unroll
  for (int k = 0; k < 3; ++k) X[k] = best[k];
  if (best_count > 0) {
    double Xr[3];
    refit(d, lo, n, set, best, Xr);
    if (is_finite(Xr[0]) && is_finite(Xr[1]) && is_finite(Xr[2])) {
      const int rcount = count_set(d, lo, n, set, Xr);
      if (rcount >= best_count) {
        count = rcount;
#pragma unroll
        for (int k = 0; k < 3; ++k) X[k] = Xr[k];
      }
    }
  }
  // acceptance: some pair of them with enough parallax at X
  bool wide = false;
  if (count >= 2) {
    for (int i = 0; i < n && !wide; ++i) {
      View wi;
      double sq, z, ci[3];
      load_view(d, lo + i, wi);
      if (!set(d, lo, n, i, wi, X, sq, z)) continue;
      centre_of(wi, ci);
      for (int j = i + 1; j < n && !wide; ++j) {
        View wj;
        double cj[3];
        load_view(d, lo + j, wj);
        if (!set(d, lo, n, j, wj, X, sq, z)) continue;
        centre_of(wj, cj);
        wide = parallax(X, ci, cj, tan2);
      }
    }
  }
  return wide ? count : 0;
}

// The tail vc_triangulate_tracks and vc_refine_tracks share, from a point `best` with best_count inliers (0: there is none):
// `settle` over the inliers and the outputs as triangulate_track states them.
__host__ __device__ __forceinline__ int finish_track(const Tracks& d, long long lo, int n, const double (&best)[3], int best_count,
                                                     double e2, double tan2, double (&X)[3], uint8_t* mask, double& error) {
  const int count = settle(d, lo, n, Inliers{e2}, best, best_count, tan2, X);
  const bool wide = count > 0;
  double sum = 0.0;
  for (int i = 0; i < n; ++i) {
    View w;
    double sq, z;
    load_view(d, lo + i, w);
    const bool in = wide && inlier(w, X, e2, sq, z);
    mask[i] = in ? 1 : 0;
    if (in) sum += sqrt(sq / (z * z));
  }
  if (!wide) {
    X[0] = X[1] = X[2] = NAN;
    error = NAN;
    return 0;
  }
  error = sum / (double)count;
  return count;
}

// One track: observations lo .. lo + n of the call.  -> the number of inliers (0: rejected); X, the mean pixel error of the
// inliers and mask[0 .. n) (the track's own slots) are written either way, NaN and 0 for a rejected track.
__host__ __device__ __forceinline__ int triangulate_track(const Tracks& d, long long lo, int n, uint32_t seed, double max_error,
                                                          double tan2, double (&X)[3], uint8_t* mask, double& error) {
  const double e2 = max_error * max_error;
  double best[3] = {NAN, NAN, NAN};
  int best_count = 0;
  const bool all_pairs = (long long)n * (n - 1) / 2 <= kTriMaxHypotheses;
  const int n_hyp = n < 2 ? 0 : all_pairs ? n * (n - 1) / 2 : kTriMaxHypotheses;
  int p = 0, q = 0;                                          // all pairs: (0, 1), (0, 2), ...
  for (int h = 0; h < n_hyp; ++h) {
    next_pair(all_pairs, seed, h, n, p, q);
    View vp, vq;
    load_view(d, lo + p, vp);
    load_view(d, lo + q, vq);
    double Xh[3], sq, z;
    if (!(vp.ok && vq.ok && midpoint(vp, vq, tan2, Xh))) continue;
    if (!(inlier(vp, Xh, e2, sq, z) && inlier(vq, Xh, e2, sq, z))) continue;
    const int count = count_set(d, lo, n, Inliers{e2}, Xh);
    if (count > best_count) {                                // the lowest h on ties
      best_count = count;
#pragma unroll
      for (int k = 0; k < 3; ++k) best[k] = Xh[k];
    }
  }
  return finish_track(d, lo, n, best, best_count, e2, tan2, X, mask, error);
}

// One track re-evaluated at a point it has already: X0's inliers over every usable observation, fewer than two
// or a non-finite X0 reject; then the tail of triangulate_track.  Outputs as there.
__host__ __device__ __forceinline__ int refine_track(const Tracks& d, long long lo, int n, const double (&X0)[3], double max_error,
                                                     double tan2, double (&X)[3], uint8_t* mask, double& error) {
  const double e2 = max_error * max_error;
  const bool given = is_finite(X0[0]) && is_finite(X0[1]) && is_finite(X0[2]);
  const int count0 = given ? count_set(d, lo, n, Inliers{e2}, X0) : 0;
  return finish_track(d, lo, n, X0, count0 >= 2 ? count0 : 0, e2, tan2, X, mask, error);
}

// ---- vc_split_tracks ---------------------------------------------------------------------------------------
// The set of vc_split_tracks at a point X, for slot k: in every run (adjacent nodes of one obs_cam) that holds no node of slot
// k, the free (label -1) usable inlier of X with the smallest sq, the lowest index on ties.  The nodes of a run share their
// camera row, so a neighbour is the node's own view with another pixel and comparing sq compares pixel errors.  A node that
// takes label k while the nodes are walked in ascending order closes its run to the nodes after it, and the ones before it
// had lost to it already: labelling in place selects what counting selected.
struct Selection {
  const int32_t* label;                                      // of the component's nodes; read again at every call
  int k;
  double e2;
  __host__ __device__ __forceinline__ bool operator()(const Tracks& d, long long lo, int n, int i, const View& w, const double (&X)[3],
                                                      double& sq, double& z) const {
    if (label[i] != -1 || !inlier(w, X, e2, sq, z)) return false;
    const int32_t cam = d.obs_cam[lo + i];
    bool mine = true;
    for (int j = i - 1; j >= 0 && d.obs_cam[lo + j] == cam; --j) mine = mine && !beats(d, lo + j, label[j], w, X, sq, true);
    for (int j = i + 1; j < n && d.obs_cam[lo + j] == cam; ++j) mine = mine && !beats(d, lo + j, label[j], w, X, sq, false);
    return mine;
  }
  // Node j of the run of w (w is usable, so the run's camera row is) keeps w's node out: it holds slot k, or it is a free
  // inlier of X with a smaller sq than `than`, an equal one if it comes first.
  __host__ __device__ __forceinline__ bool beats(const Tracks& d, long long j, int32_t label_j, const View& w, const double (&X)[3],
                                                 double than, bool first) const {
    if (label_j == k) return true;
    if (label_j != -1) return false;
    View o = w;
    o.u = d.obs_xy[2 * j], o.v = d.obs_xy[2 * j + 1];
    o.ok = is_finite(o.u) && is_finite(o.v);
    double sq, z;
    return inlier(o, X, e2, sq, z) && (sq < than || (first && sq == than));
  }
};

// The nodes selected at X take label k, in ascending order -> how many; sum: their pixel errors added up in that order.
__host__ __device__ __forceinline__ int label_selection(const Tracks& d, long long lo, int n, int32_t* label, int k, double e2,
                                                        const double (&X)[3], double& sum) {
  const Selection set{label, k, e2};
  int count = 0;
  sum = 0.0;
  for (int i = 0; i < n; ++i) {
    View w;
    double sq, z;
    load_view(d, lo + i, w);
    if (!set(d, lo, n, i, w, X, sq, z)) continue;
    label[i] = k;
    sum += sqrt(sq / (z * z));
    ++count;
  }
  return count;
}

// One component: nodes lo .. lo + n of the call, label[0 .. n) their node_point, pts[max_points][3] its points_xyz and
// count / made / error [max_points] its outputs (include/vitcolmap_hip.h states the rule).  A slot is looked up by a run-time
// index in global memory only; which slots were occupied on input is a bit mask, so no array of the lane has one.
__host__ __device__ __forceinline__ void split_component(const Tracks& d, long long lo, int n, uint32_t seed, int max_points,
                                                         double max_error, double tan2, int32_t* label, double* pts, int32_t* count,
                                                         uint8_t* made, double* error) {
  const double e2 = max_error * max_error;
  unsigned occupied = 0;
  for (int k = 0; k < max_points; ++k) {
    made[k] = 0;
    error[k] = NAN;
    if (is_finite(pts[3 * k]) && is_finite(pts[3 * k + 1]) && is_finite(pts[3 * k + 2])) occupied |= 1u << k;
  }
  // attach: the selection under every point the component has already; the point stays
  for (int k = 0; k < max_points; ++k) {
    if (!(occupied >> k & 1u)) continue;
    const double X[3] = {pts[3 * k], pts[3 * k + 1], pts[3 * k + 2]};
    double sum;
    label_selection(d, lo, n, label, k, e2, X, sum);
  }
  // peel: one new point per empty slot out of the nodes that are still free, until a slot finds none
  const bool all_pairs = (long long)n * (n - 1) / 2 <= kTriMaxHypotheses;
  const int n_hyp = n < 2 ? 0 : all_pairs ? n * (n - 1) / 2 : kTriMaxHypotheses;
  for (int k = 0; k < max_points; ++k) {
    if (occupied >> k & 1u) continue;
    const Selection set{label, k, e2};
    const uint32_t seed_k = seed + (uint32_t)k * 0x9E3779B9u;
    double best[3] = {NAN, NAN, NAN};
    int best_count = 0;
    int p = 0, q = 0;
    for (int h = 0; h < n_hyp; ++h) {
      next_pair(all_pairs, seed_k, h, n, p, q);
      if (label[p] != -1 || label[q] != -1 || d.obs_cam[lo + p] == d.obs_cam[lo + q]) continue;
      View vp, vq;
      load_view(d, lo + p, vp);
      load_view(d, lo + q, vq);
      double Xh[3], sq, z;
      if (!(vp.ok && vq.ok && midpoint(vp, vq, tan2, Xh))) continue;
      if (!(set(d, lo, n, p, vp, Xh, sq, z) && set(d, lo, n, q, vq, Xh, sq, z))) continue;
      const int c = count_set(d, lo, n, set, Xh);
      if (c > best_count) {                                  // the lowest h on ties
        best_count = c;
#pragma unroll
        for (int j = 0; j < 3; ++j) best[j] = Xh[j];
      }
    }
    double X[3], sum;
    if (settle(d, lo, n, set, best, best_count, tan2, X) == 0) break;
    const int c = label_selection(d, lo, n, label, k, e2, X, sum);
    pts[3 * k] = X[0], pts[3 * k + 1] = X[1], pts[3 * k + 2] = X[2];
    made[k] = 1;
    error[k] = sum / (double)c;
  }
  for (int k = 0; k < max_points; ++k) {
    int c = 0;
    for (int i = 0; i < n; ++i) c += label[i] == k ? 1 : 0;
    count[k] = c;
  }
}

// Component t of a call, rows lo .. hi of the per-node arrays; offsets that do not delimit a list reject it: nothing of it is
// read, its labels and points stay and its outputs are 0 / NaN.
__host__ __device__ __forceinline__ void split_or_reject(const Tracks& d, long long t, long long lo, long long hi, uint32_t seed,
                                                         int max_points, double max_error, double tan2, int32_t* node_point,
                                                         double* points_xyz, int32_t* out_count, uint8_t* out_new, double* out_error) {
  const long long base = t * max_points;
  if (lo >= 0 && hi >= lo) {
    split_component(d, lo, (int)(hi - lo), seed, max_points, max_error, tan2, node_point + lo, points_xyz + 3 * base, out_count + base,
                    out_new + base, out_error + base);
    return;
  }
  for (int k = 0; k < max_points; ++k) out_count[base + k] = 0, out_new[base + k] = 0, out_error[base + k] = NAN;
}

// vc_split_tracks: the shape of triangulate_tracks_kernel, one component per lane.  node_point and points_xyz are read and
// written by the lane that owns them only.
__global__ __launch_bounds__(kTriWave) void split_tracks_kernel(Tracks d, const int32_t* __restrict__ offsets, int n_comps,
                                                                const int32_t* __restrict__ seeds, int max_points, double max_error,
                                                                double tan2, int32_t* node_point, double* points_xyz,
                                                                int32_t* __restrict__ out_count, uint8_t* __restrict__ out_new,
                                                                double* __restrict__ out_error) {
  const long long t = (long long)blockIdx.x * kTriWave + threadIdx.x;
  if (t >= n_comps) return;
  split_or_reject(d, t, offsets[t], offsets[t + 1], (uint32_t)seeds[t], max_points, max_error, tan2, node_point, points_xyz, out_count,
                  out_new, out_error);
}

__global__ __launch_bounds__(kTriWave) void triangulate_tracks_kernel(Tracks d, const int32_t* __restrict__ offsets, int n_tracks,
                                                                      const int32_t* __restrict__ seeds, double max_error, double tan2,
                                                                      double* __restrict__ out_xyz, uint8_t* __restrict__ out_mask,
                                                                      int32_t* __restrict__ out_count, double* __restrict__ out_error) {
  const long long t = (long long)blockIdx.x * kTriWave + threadIdx.x;
  if (t >= n_tracks) return;
  const long long lo = offsets[t], hi = offsets[t + 1];
  double X[3] = {NAN, NAN, NAN}, error = NAN;
  int count = 0;
  if (lo >= 0 && hi >= lo)                                   // a track whose offsets do not delimit a list is rejected, nothing of it read
    count = triangulate_track(d, lo, (int)(hi - lo), (uint32_t)seeds[t], max_error, tan2, X, out_mask + lo, error);
  out_xyz[3 * t] = X[0], out_xyz[3 * t + 1] = X[1], out_xyz[3 * t + 2] = X[2];
  out_count[t] = count;
  out_error[t] = error;
}

// vc_refine_tracks: the shape of triangulate_tracks_kernel, init_xyz in place of the seeds.
__global__ __launch_bounds__(kTriWave) void refine_tracks_kernel(Tracks d, const int32_t* __restrict__ offsets, int n_tracks,
                                                                 const double* __restrict__ init_xyz, double max_error, double tan2,
                                                                 double* __restrict__ out_xyz, uint8_t* __restrict__ out_mask,
                                                                 int32_t* __restrict__ out_count, double* __restrict__ out_error) {
  const long long t = (long long)blockIdx.x * kTriWave + threadIdx.x;
  if (t >= n_tracks) return;
  const long long lo = offsets[t], hi = offsets[t + 1];
  double X[3] = {NAN, NAN, NAN}, error = NAN;
  int count = 0;
  if (lo >= 0 && hi >= lo) {                                 // as in triangulate_tracks_kernel
    const double X0[3] = {init_xyz[3 * t], init_xyz[3 * t + 1], init_xyz[3 * t + 2]};
    count = refine_track(d, lo, (int)(hi - lo), X0, max_error, tan2, X, out_mask + lo, error);
  }
  out_xyz[3 * t] = X[0], out_xyz[3 * t + 1] = X[1], out_xyz[3 * t + 2] = X[2];
  out_count[t] = count;
  out_error[t] = error;
}

}  // namespace

extern "C" {

int vc_triangulate_tracks(const double* obs_xy, const int32_t* obs_cam, const int32_t* offsets, int n_tracks, const double* cams,
                          int n_cams, const int32_t* seeds, double max_error_px, double min_tri_angle_tan2, double* out_xyz,
                          uint8_t* out_mask, int32_t* out_count, double* out_error, vc_stream_t stream) {
  if (n_tracks < 0 || n_cams < 0) return VC_ERR_INVALID_ARG;
  if (n_tracks == 0) return VC_OK;
  if (!obs_xy || !obs_cam || !offsets || !seeds || !out_xyz || !out_mask || !out_count || !out_error) return VC_ERR_INVALID_ARG;
  if (!cams && n_cams > 0) return VC_ERR_INVALID_ARG;
  if (!(max_error_px >= 0.0 && max_error_px < INFINITY && min_tri_angle_tan2 >= 0.0 && min_tri_angle_tan2 < INFINITY))
    return VC_ERR_INVALID_ARG;
  const int blocks = (n_tracks + kTriWave - 1) / kTriWave;
  hipLaunchKernelGGL(triangulate_tracks_kernel, dim3((unsigned)blocks), dim3(kTriWave), 0, (hipStream_t)stream,
                     Tracks{obs_xy, obs_cam, cams, n_cams}, offsets, n_tracks, seeds, max_error_px, min_tri_angle_tan2, out_xyz, out_mask,
                     out_count, out_error);
  return vc::check_launch();
}

int vc_refine_tracks(const double* obs_xy, const int32_t* obs_cam, const int32_t* offsets, int n_tracks, const double* cams, int n_cams,
                     const double* init_xyz, double max_error_px, double min_tri_angle_tan2, double* out_xyz, uint8_t* out_mask,
                     int32_t* out_count, double* out_error, vc_stream_t stream) {
  if (n_tracks < 0 || n_cams < 0) return VC_ERR_INVALID_ARG;
  if (n_tracks == 0) return VC_OK;
  if (!obs_xy || !obs_cam || !offsets || !init_xyz || !out_xyz || !out_mask || !out_count || !out_error) return VC_ERR_INVALID_ARG;
  if (!cams && n_cams > 0) return VC_ERR_INVALID_ARG;
  if (!(max_error_px >= 0.0 && max_error_px < INFINITY && min_tri_angle_tan2 >= 0.0 && min_tri_angle_tan2 < INFINITY))
    return VC_ERR_INVALID_ARG;
  const int blocks = (n_tracks + kTriWave - 1) / kTriWave;
  hipLaunchKernelGGL(refine_tracks_kernel, dim3((unsigned)blocks), dim3(kTriWave), 0, (hipStream_t)stream,
                     Tracks{obs_xy, obs_cam, cams, n_cams}, offsets, n_tracks, init_xyz, max_error_px, min_tri_angle_tan2, out_xyz, out_mask,
                     out_count, out_error);
  return vc::check_launch();
}

int vc_split_tracks(const double* obs_xy, const int32_t* obs_cam, const int32_t* offsets, int n_comps, const double* cams, int n_cams,
                    const int32_t* seeds, int max_points, double max_error_px, double min_tri_angle_tan2, int32_t* node_point,
                    double* points_xyz, int32_t* out_count, uint8_t* out_new, double* out_error, vc_stream_t stream) {
  if (n_comps < 0 || n_cams < 0) return VC_ERR_INVALID_ARG;
  if (n_comps == 0) return VC_OK;
  if (max_points < 1 || max_points > VC_SPLIT_MAX_POINTS) return VC_ERR_INVALID_ARG;
  if (!obs_xy || !obs_cam || !offsets || !seeds || !node_point || !points_xyz || !out_count || !out_new || !out_error)
    return VC_ERR_INVALID_ARG;
  if (!cams && n_cams > 0) return VC_ERR_INVALID_ARG;
  if (!(max_error_px >= 0.0 && max_error_px < INFINITY && min_tri_angle_tan2 >= 0.0 && min_tri_angle_tan2 < INFINITY))
    return VC_ERR_INVALID_ARG;
  const int blocks = (n_comps + kTriWave - 1) / kTriWave;
  hipLaunchKernelGGL(split_tracks_kernel, dim3((unsigned)blocks), dim3(kTriWave), 0, (hipStream_t)stream,
                     Tracks{obs_xy, obs_cam, cams, n_cams}, offsets, n_comps, seeds, max_points, max_error_px, min_tri_angle_tan2,
                     node_point, points_xyz, out_count, out_new, out_error);
  return vc::check_launch();
}

}  // extern "C"
