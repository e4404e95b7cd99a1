// Bundle adjustment (gfx950): the kernels of one Levenberg-Marquardt iteration over every pose and every point
// of a sparse model and, where groups of cameras are given, over the groups' intrinsics, by the Schur complement of the points.
// The callers (vit_colmap_amd/mapping/bundle.py, mapping/bundle_intr.py) repeat linearize points, reduce cameras, step; with
// groups linearize intrinsics and reduce border follow the reduction: the groups' unknowns theta_g border the reduced system,
// [[S, B], [B', C]] (dc, dtheta) = -(g, h), which the caller solves.  Without the dense S ("The solver" in §4.2k:
// vc_ba_camera_blocks, vc_ba_schur_product) the caller solves S dc = -g by preconditioned conjugate gradients.
//
// Every pass that sees an observation is one template over (kLoss, kDist); four instances exist:
//   (false, kBaDistNone)    vc_ba_linearize_points, vc_ba_linearize_intrinsics, vc_ba_reduce_border: the pinhole, no loss; loss, obs_w
//                           and cam_dist are absent and not read.
//   (true, kBaDistNone)     the _loss entry points: every observation's J_c, J_p, r and J_theta are multiplied by sw = sqrt(w) of its
//                           loss (Huber, soft L1) before anything is formed from them; the points pass writes obs_w [total], the other
//                           two read it.
//   (true, kBaDistRadial)   the _radial entry points (COLMAP's SIMPLE_RADIAL and RADIAL): cam_dist [n_cams][2] = (k1, k2) travels
//                           beside the cameras' rows, theta_g = (fx, fy, cx, cy, k1, k2).
//   (true, kBaDistOpencv)   the _opencv entry points (COLMAP's OPENCV): cam_dist [n_cams][4] = (k1, k2, p1, p2), theta_g has eight
//                           unknowns and bit 7 of a group's mask holds p1 and p2 together.
// Everything a model sets is a constexpr function of kDist (ba_dist_unknowns, ba_dist_params, ba_dist_jt, ba_dist_max_groups); the
// routines that see only a group's unknowns (the terms' rows, C and h, the points' step) take their number N = ba_dist_unknowns(kDist).
// Under a distortion the loss is always on: VC_BA_LOSS_TRIVIAL gives rho = s and sw = 1, and a product with 1.0 is exact.
//
// float64 in single operations in the written order (-ffp-contract=off), the only library call is sqrt, no atomics.
//   points pass  one point per lane, one wave per workgroup, no LDS.  ba_linearize_points_kernel: every observation of the point's
//                track is linearised (ba_observe; residual r, J_c 2x6, W = J_c' J_p 6x3, written per observation: 32 numbers),
//                V = sum J_p' J_p, g_p and the cost are accumulated in track order, V is damped and inverted by the adjugate.
//                ba_linearize_intrinsics_kernel: obs_jt [total][ba_dist_jt] (what J_theta is rebuilt from; the pinhole's (x, y), its
//                entry points' obs_xn), then the groups outside and the track inside, T = sum J_theta' J_p, q, hq (the observation
//                projected again) and the point's products T V^-1 T', T V^-1 g_p; nothing is a register array indexed by a
//                runtime value.
//   ordered sums ba_ordered_sums_kernel, one wave per row of [rows][n], adds the row in ascending order: the total cost is the one
//                row of the points' costs, the border's C and h come from the rows of its terms (ba_border_system_kernel).
//   camera pass  one workgroup of one wave per camera a.  ba_camera_walk: what lanes share is prepared 64 entries of the camera's
//                list at a time, one per lane (the entry resolved, Y = W V^-1), and left in LDS between two barriers; every lane
//                then walks the batch in order, so the chain of dependent loads that resolves an entry is paid once per batch.
//                ba_reduce_cameras_kernel keeps the row block [6][6 n_cams] of sum Y W' in LDS: entry e = 6 r + c of block b
//                belongs to lane (36 b + e) mod 64 for the whole launch; nobody else reads or writes it, so there is no atomic and
//                the order of a lane's additions is the rule's: camera a's observations in ascending order and, inside each, the
//                track of its point in track order (the next element's flag and camera are loaded while the current element's W
//                is on its way).  ba_reduce_border_kernel keeps a lane's entries of B_a [6][N G] in its registers.
//   solver       ba_camera_blocks_kernel, one wave per camera through ba_camera_walk: lane e < 36 keeps entry e of U_a and of
//                (sum Y W')_aa in its registers, six lanes invert D_a by a 6x6 Cholesky factorisation, a column each.
//                ba_product_points_kernel, one point per lane: s_j = V^-1 sum W' p.  ba_product_cameras_kernel, four waves per
//                camera: 256 entries of the list resolved at once, W s left in LDS, six owner lanes add them in list order.
//   step         ba_step_points_kernel, one point per lane: dX = -V^-1 (g_p + sum W' dc + sum T_g' dtheta_g) in track order, then
//                group order, X + dX; ba_step_cameras_kernel, one camera per lane: q = (1, w / 2) normalised, R(q) R, t + dt, its
//                group's dtheta added to its intrinsics and its row of cam_dist, whether the candidate is valid.  vc_ba_step
//                launches both without groups: T, dtheta, cam_group and the valid flags are then absent and not read.
// What a lane computes is sequential and nothing depends on the order in which lanes or workgroups run, so two launches
// return the same bits, and the same routines compiled for the host (tools/bundle_host.cpp includes this file) return the
// device's.  Every index read from an input array is checked against the array it indexes before it is used.  Specification:
// tests/util_bundle.py, util_bundle_intr.py, util_bundle_loss.py, util_bundle_radial.py, util_bundle_opencv.py, util_bundle_pcg.py.
// This build's own published rule; parity with COLMAP / Ceres is unpinned.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/vitcolmap_hip.h"
#include "common.h"

namespace {

constexpr int kBaWave = 64;
constexpr int kBaLin = 32;                     // numbers per observation: J_c row u (6), row v (6), r (2), W row-major (18)
constexpr int kBaLinR = 12, kBaLinW = 14;

struct BaProblem {
  const double* __restrict__ cams;             // [n_cams][16]
  const uint8_t* __restrict__ const_mask;      // [n_cams]
  const double* __restrict__ points;           // [n_points][3]
  const int32_t* __restrict__ offsets;         // [n_points + 1]
  const int32_t* __restrict__ obs_cam;         // [total]
  const double* __restrict__ obs_xy;           // [total][2]
  int n_cams, n_points, total;
  const double* __restrict__ cam_dist;         // [n_cams][ba_dist_params]; null for the pinhole
};

// What the points pass leaves for the other two.
struct BaLinear {
  const double* __restrict__ vinv;             // [n_points][6]: 00 01 02 11 12 22
  const double* __restrict__ gp;               // [n_points][3]
  const uint8_t* __restrict__ obs_ok;          // [total]
  const double* __restrict__ obs_lin;          // [total][32]
};

__host__ __device__ __forceinline__ bool ba_finite(double x) { return fabs(x) < INFINITY; }   // false for NaN

// Point j's rows of the per-observation arrays -> false when its offsets do not delimit a list inside them.
__host__ __device__ __forceinline__ bool ba_track(const int32_t* __restrict__ offsets, int j, int total, int& lo, int& hi) {
  lo = offsets[j], hi = offsets[j + 1];
  return lo >= 0 && hi >= lo && hi <= total;
}

// X in the camera of row c[16]: Y = R X, Xc = Y + t, (xu, xv) = (Xc_x, Xc_y) / Xc_z, (fu, fv) = (fx, fy) / Xc_z and J_p (2x3).
__host__ __device__ __forceinline__ void ba_project(const double* c, const double (&X)[3], double (&Y)[3], double (&Xc)[3], double& fu,
                                                    double& fv, double& xu, double& xv, double (&ju)[3], double (&jv)[3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    Y[i] = c[3 * i] * X[0] + c[3 * i + 1] * X[1] + c[3 * i + 2] * X[2];
    Xc[i] = Y[i] + c[9 + i];
  }
  const double z = Xc[2];
  fu = c[12] / z, fv = c[13] / z, xu = Xc[0] / z, xv = Xc[1] / z;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    ju[k] = fu * (c[k] - xu * c[6 + k]);
    jv[k] = fv * (c[3 + k] - xv * c[6 + k]);
  }
}

// The loss of an observation ("The loss" in DESIGN.md §4.2k): kind VC_BA_LOSS_*, scale c in px.
struct BaLoss {
  int kind;
  double scale;
};

// A loss the entry points accept: a kind of the header's, a finite positive scale (false for NaN).
__host__ __device__ __forceinline__ bool ba_loss_valid(const BaLoss& loss) {
  return loss.kind >= VC_BA_LOSS_TRIVIAL && loss.kind <= VC_BA_LOSS_SOFT_L1 && loss.scale > 0.0 && loss.scale < INFINITY;
}

// What an entry point without loss arguments hands its launcher: not read without a loss, and valid for the two _loss entry
// points whose weights come in obs_w.
constexpr BaLoss kBaNoLoss{VC_BA_LOSS_TRIVIAL, 1.0};

// s = |r|^2 of the unweighted residual -> rho(s) and the weight w = rho'(s).
__host__ __device__ __forceinline__ void ba_loss(const BaLoss& loss, double s, double& rho, double& w) {
  const double c = loss.scale;
  rho = s, w = 1.0;
  if (loss.kind == VC_BA_LOSS_HUBER) {
    if (!(s <= c * c)) {
      const double q = sqrt(s);
      rho = (2.0 * c) * q - c * c, w = c / q;
    }
  } else if (loss.kind == VC_BA_LOSS_SOFT_L1) {
    const double q = sqrt(1.0 + s / (c * c));
    rho = 2.0 * s / (1.0 + q), w = 1.0 / q;
  }
}

// The radial distortion of a camera ("The distortion" in DESIGN.md §4.2k): (xu, xv) -> (xu s, xv s), s = 1 + k1 rho + k2 rho rho,
// rho = xu xu + xv xv.  What an observation needs of it, each in the written order:
//   s = 1 + k1 rho + k2 rho rho, e = 2 (k1 + 2 k2 rho), the symmetric 2x2 Jacobian D of the map: d00 = s + xu xu e, d01 = xu xv e,
//   d11 = s + xv xv e, and the six numbers from which the border rebuilds J_theta (obs_jt of the radial entry points):
//   xd = xu s, yd = xv s, pu = fx xu rho, pv = fy xv rho, qu = pu rho, qv = pv rho.
// With the tangential terms ("The tangential terms" in §4.2k; COLMAP's OPENCV, cam_dist [n_cams][4] = (k1, k2, p1, p2)) the map is
//   xd = xu s + 2 p1 xu xv + p2 (rho + 2 xu xu), yd = xv s + p1 (rho + 2 xv xv) + 2 p2 xu xv, the radial term first as
//   csrc/undistort.hip writes it, D gains d00 += 2 p1 xv + 6 p2 xu, d01 += 2 p1 xu + 2 p2 xv, d11 += 6 p1 xv + 2 p2 xu, and obs_jt
//   has ten numbers: the six above, then the p1 column (fx 2 xu xv, fy (rho + 2 xv xv)) and the p2 column (fx (rho + 2 xu xu),
//   fy 2 xu xv) of J_theta.
// The residual is r = (fx xd + cx - u, fy yd + cy - v); J_p = diag(fx, fy) D (nu; nv) with (nu; nv) the Jacobian of (xu, xv), which
// ba_project gives on the row with fx = fy = 1, and J_c the same map of the pinhole rows at fx = fy = 1; J_theta =
// ((xd, 0, 1, 0, pu, qu, ..); (0, yd, 0, 1, pv, qv, ..)).  Every product and sum left to right as written.
// The model is the template argument kDist; what it sets:
constexpr int kBaDistNone = 0, kBaDistRadial = 1, kBaDistOpencv = 2;
__host__ __device__ constexpr int ba_dist_unknowns(int dist) { return dist == kBaDistOpencv ? 8 : dist == kBaDistRadial ? 6 : 4; }   // per group
__host__ __device__ constexpr int ba_dist_params(int dist) { return ba_dist_unknowns(dist) - 4; }        // numbers per row of cam_dist
__host__ __device__ constexpr int ba_dist_jt(int dist) { return dist == kBaDistOpencv ? 10 : dist == kBaDistRadial ? 6 : 2; }   // per row of obs_jt
__host__ __device__ constexpr int ba_dist_max_groups(int dist) {
  return dist == kBaDistOpencv ? VC_BA_MAX_GROUPS_OPENCV : dist == kBaDistRadial ? VC_BA_MAX_GROUPS_RADIAL : VC_BA_MAX_GROUPS;
}

// What an observation keeps of its projection: D and the numbers of its row of obs_jt; the pinhole has jt = (x, y) and no D.
template <int kDist>
struct BaDistortion {
  double d00, d01, d11, jt[ba_dist_jt(kDist)];
};

// X in the camera of row c[16] under the row k of cam_dist, kDist != kBaDistNone: ba_project on the row with fx = fy = 1, so that
// iu = 1 / Xc_z and (nu, nv) is the Jacobian of (xu, xv); then J_p = diag(fx, fy) D (nu; nv): ju = fx (d00 nu + d01 nv),
// jv = fy (d01 nu + d11 nv).  The radial term first, the tangential terms added after it, left to right.
template <int kDist>
__host__ __device__ __forceinline__ void ba_project_dist(const double* c, const double* k, const double (&X)[3], double (&Y)[3],
                                                         double (&Xc)[3], double& iu, double& xu, double& xv, BaDistortion<kDist>& rd,
                                                         double (&ju)[3], double (&jv)[3]) {
  static_assert(kDist != kBaDistNone, "the pinhole is ba_project's");
  double n[16], iv, nu[3], nv[3];
#pragma unroll
  for (int i = 0; i < 16; ++i) n[i] = i == 12 || i == 13 ? 1.0 : c[i];
  ba_project(n, X, Y, Xc, iu, iv, xu, xv, nu, nv);
  const double fx = c[12], fy = c[13], k1 = k[0], k2 = k[1];
  const double rho = xu * xu + xv * xv;
  const double s = 1.0 + k1 * rho + k2 * rho * rho;
  const double e = 2.0 * (k1 + 2.0 * k2 * rho);
  rd.d00 = s + xu * xu * e, rd.d01 = xu * xv * e, rd.d11 = s + xv * xv * e;
  rd.jt[0] = xu * s, rd.jt[1] = xv * s, rd.jt[2] = fx * xu * rho, rd.jt[3] = fy * xv * rho;
  rd.jt[4] = rd.jt[2] * rho, rd.jt[5] = rd.jt[3] * rho;
  if constexpr (kDist == kBaDistOpencv) {
    const double p1 = k[2], p2 = k[3];
    rd.d00 = rd.d00 + 2.0 * p1 * xv + 6.0 * p2 * xu;
    rd.d01 = rd.d01 + 2.0 * p1 * xu + 2.0 * p2 * xv;
    rd.d11 = rd.d11 + 6.0 * p1 * xv + 2.0 * p2 * xu;
    rd.jt[0] = rd.jt[0] + 2.0 * p1 * xu * xv + p2 * (rho + 2.0 * xu * xu);
    rd.jt[1] = rd.jt[1] + p1 * (rho + 2.0 * xv * xv) + 2.0 * p2 * xu * xv;
    rd.jt[6] = fx * 2.0 * xu * xv, rd.jt[7] = fy * (rho + 2.0 * xv * xv);
    rd.jt[8] = fx * (rho + 2.0 * xu * xu), rd.jt[9] = fy * 2.0 * xu * xv;
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    ju[i] = fx * (rd.d00 * nu[i] + rd.d01 * nv[i]);
    jv[i] = fy * (rd.d01 * nu[i] + rd.d11 * nv[i]);
  }
}

// Observation o of point X: usable -> lin[32] (zeros otherwise) and J_p (2x3).  With a loss the rows of J_c and J_p and r are
// multiplied by sw = sqrt(w) before anything is formed from them, and rho is the loss of the unweighted residual, the
// observation's term of the cost.  Under a distortion the camera's row of cam_dist must be finite too and the projection is
// ba_project_dist's; the pinhole's is ba_project's on the row as it is.
template <bool kLoss, int kDist>
__host__ __device__ __forceinline__ bool ba_observe(const BaProblem& d, const BaLoss& loss, int o, const double (&X)[3],
                                                    double* __restrict__ lin, double (&ju)[3], double (&jv)[3], double& rho, double& sw) {
  const int slot = d.obs_cam[o];
  bool ok = slot >= 0 && slot < d.n_cams;
  const double* c = d.cams + (long long)(ok ? slot : 0) * 16;
  double row[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    row[k] = ok ? c[k] : NAN;
    ok = ok && ba_finite(row[k]);
  }
  const double u = d.obs_xy[2 * (long long)o], v = d.obs_xy[2 * (long long)o + 1];
  ok = ok && ba_finite(u) && ba_finite(v);
  const unsigned held = ok ? d.const_mask[slot] : 0u;
  double Y[3], Xc[3], fu, fv, xu, xv;
  constexpr bool kDistorted = kDist != kBaDistNone;
  BaDistortion<kDist> rd;
  if constexpr (kDistorted) {
    // the row of cam_dist as the projection reads it: the radial pair, then the tangential pair.  Not a loop over kParams: every loop
    // form tried computes the same and compiles the radial points kernel to 130 VGPRs where this form keeps its 128, the last count
    // with four waves per SIMD (profiles/bundle_one_template_resource_usage.md)
    constexpr int kParams = ba_dist_params(kDist);
    const double k1 = ok ? d.cam_dist[kParams * (long long)slot] : NAN, k2 = ok ? d.cam_dist[kParams * (long long)slot + 1] : NAN;
    ok = ok && ba_finite(k1) && ba_finite(k2);
    double k[kParams] = {k1, k2};
    if constexpr (kDist == kBaDistOpencv) {
      k[2] = ok ? d.cam_dist[kParams * (long long)slot + 2] : NAN, k[3] = ok ? d.cam_dist[kParams * (long long)slot + 3] : NAN;
      ok = ok && ba_finite(k[2]) && ba_finite(k[3]);
    }
    ba_project_dist<kDist>(row, k, X, Y, Xc, fu, xu, xv, rd, ju, jv);
    fv = fu;                                                 // 1 / Xc_z: the rows of J_c below are then the pinhole ones at fx = fy = 1
  } else {
    ba_project(row, X, Y, Xc, fu, fv, xu, xv, ju, jv);
  }
  const double z = Xc[2];
  ok = ok && z > 0.0;                                        // false for NaN
  const double fx = row[12], fy = row[13], cx = row[14], cy = row[15];
  double ru = kDistorted ? fx * rd.jt[0] + cx - u : fx * Xc[0] / z + cx - u, rv = kDistorted ? fy * rd.jt[1] + cy - v : fy * Xc[1] / z + cy - v;
  const double au = fu * xu, av = fv * xv;
  // J_c = J_pi [ -[R X]x | I ]: the pose is perturbed on the left, Xc(w, dt) = Rot(w) (R X) + t + dt
  double cu[6] = {-(au * Y[1]), fu * Y[2] + au * Y[0], -(fu * Y[1]), fu, 0.0, -au};
  double cv[6] = {-(fv * Y[2] + av * Y[1]), av * Y[0], fv * Y[0], 0.0, fv, -av};
  if (kDistorted) {
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const double mu = cu[i], mv = cv[i];
      cu[i] = fx * (rd.d00 * mu + rd.d01 * mv);
      cv[i] = fy * (rd.d01 * mu + rd.d11 * mv);
    }
  }
  rho = 0.0, sw = 1.0;                                      // without a loss the caller forms |r|^2 itself
  if (kLoss) {
    double w;
    ba_loss(loss, ru * ru + rv * rv, rho, w);
    sw = sqrt(w);
#pragma unroll
    for (int k = 0; k < 3; ++k) ju[k] = sw * ju[k], jv[k] = sw * jv[k];
#pragma unroll
    for (int i = 0; i < 6; ++i) cu[i] = sw * cu[i], cv[i] = sw * cv[i];
    ru = sw * ru, rv = sw * rv;
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const bool off = !ok || ((held >> i) & 1u);          // after the weight: a held column and an unusable observation are exactly 0
    cu[i] = off ? 0.0 : cu[i];
    cv[i] = off ? 0.0 : cv[i];
    lin[i] = cu[i], lin[6 + i] = cv[i];
  }
  lin[kBaLinR] = ok ? ru : 0.0, lin[kBaLinR + 1] = ok ? rv : 0.0;
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int k = 0; k < 3; ++k) lin[kBaLinW + 3 * i + k] = ok ? cu[i] * ju[k] + cv[i] * jv[k] : 0.0;
  return ok;
}

// One point: its track linearised -> V^-1 (damped, 0 where the point is constant), g_p, cost, the usable count; per
// observation of the track obs_ok and obs_lin and, with a loss, obs_w: sw of a usable observation, 0 of any other.
template <bool kLoss, int kDist>
__host__ __device__ __forceinline__ int ba_linearize_point(const BaProblem& d, const BaLoss& loss, int j, double lambda, double (&vinv)[6],
                                                           double (&gp)[3], double& cost, uint8_t* __restrict__ obs_ok,
                                                           double* __restrict__ obs_lin, double* __restrict__ obs_w) {
#pragma unroll
  for (int k = 0; k < 6; ++k) vinv[k] = 0.0;
  gp[0] = gp[1] = gp[2] = 0.0;
  cost = 0.0;
  int lo, hi, count = 0;
  if (!ba_track(d.offsets, j, d.total, lo, hi)) return 0;   // nothing of the point is read or written
  const double X[3] = {d.points[3 * (long long)j], d.points[3 * (long long)j + 1], d.points[3 * (long long)j + 2]};
  double A00 = 0.0, A01 = 0.0, A02 = 0.0, A11 = 0.0, A12 = 0.0, A22 = 0.0, sq = 0.0;
  for (int o = lo; o < hi; ++o) {
    double* lin = obs_lin + (long long)o * kBaLin;
    double ju[3], jv[3], rho, sw;
    const bool ok = ba_observe<kLoss, kDist>(d, loss, o, X, lin, ju, jv, rho, sw);
    obs_ok[o] = ok ? 1 : 0;
    if (kLoss) obs_w[o] = ok ? sw : 0.0;
    if (!ok) continue;
    const double ru = lin[kBaLinR], rv = lin[kBaLinR + 1];
    A00 += ju[0] * ju[0] + jv[0] * jv[0], A01 += ju[0] * ju[1] + jv[0] * jv[1], A02 += ju[0] * ju[2] + jv[0] * jv[2];
    A11 += ju[1] * ju[1] + jv[1] * jv[1], A12 += ju[1] * ju[2] + jv[1] * jv[2], A22 += ju[2] * ju[2] + jv[2] * jv[2];
    gp[0] += ju[0] * ru + jv[0] * rv, gp[1] += ju[1] * ru + jv[1] * rv, gp[2] += ju[2] * ru + jv[2] * rv;
    sq += kLoss ? rho : ru * ru + rv * rv;
    ++count;
  }
  cost = 0.5 * sq;
  A00 += lambda * A00, A11 += lambda * A11, A22 += lambda * A22;
  // the adjugate of the symmetric V
  const double c00 = A11 * A22 - A12 * A12, c01 = A02 * A12 - A01 * A22, c02 = A01 * A12 - A02 * A11;
  const double c11 = A00 * A22 - A02 * A02, c12 = A01 * A02 - A00 * A12, c22 = A00 * A11 - A01 * A01;
  const double det = A00 * c00 + A01 * c01 + A02 * c02;
  if (count >= 2 && det > 0.0 && det < INFINITY) {          // otherwise the point is constant for this linearisation
    const double inv = 1.0 / det;
    vinv[0] = c00 * inv, vinv[1] = c01 * inv, vinv[2] = c02 * inv, vinv[3] = c11 * inv, vinv[4] = c12 * inv, vinv[5] = c22 * inv;
  }
  return count;
}

// Entry idx of camera a's list -> the observation and its point's track; false where the entry names no usable
// observation of camera a (the point's offsets, the observation's owner and its slot are checked here).
__host__ __device__ __forceinline__ bool ba_camera_obs_at(const BaProblem& d, const BaLinear& l, const int32_t* __restrict__ obs_point, int a,
                                                          int o, int& j, int& lo, int& hi) {
  if (o < 0 || o >= d.total) return false;
  j = obs_point[o];
  if (j < 0 || j >= d.n_points || !ba_track(d.offsets, j, d.total, lo, hi) || o < lo || o >= hi) return false;
  return d.obs_cam[o] == a && l.obs_ok[o] != 0;
}

__host__ __device__ __forceinline__ bool ba_camera_obs(const BaProblem& d, const BaLinear& l, const int32_t* __restrict__ cam_obs,
                                                       const int32_t* __restrict__ obs_point, int a, int idx, int& o, int& j,
                                                       int& lo, int& hi) {
  o = cam_obs[idx];
  return ba_camera_obs_at(d, l, obs_point, a, o, j, lo, hi);
}

// The registers of one lane of the camera pass: its entry of U_a (the lanes that own block a), of sum J_c' r and of sum Y g_p
// (lanes 0 .. 5).
struct BaLane {
  double u, gr, gy;
};

// What one lane prepares for the others: entry base + lane of camera a's list resolved (o < 0: passed over) and, for a usable
// observation, Y = W V^-1 (6x3, 18 numbers).  A batch of 64 entries is prepared at once, then every lane walks it in order.
struct BaBatch {
  int o[kBaWave], j[kBaWave], lo[kBaWave], hi[kBaWave];
  double y[kBaWave][18];
};

__host__ __device__ __forceinline__ void ba_prepare(const BaProblem& d, const BaLinear& l, const int32_t* __restrict__ cam_obs,
                                                    const int32_t* __restrict__ obs_point, int a, int idx, int last, int lane,
                                                    BaBatch& batch) {
  int o = -1, j = 0, lo = 0, hi = 0;
  if (idx >= last || !ba_camera_obs(d, l, cam_obs, obs_point, a, idx, o, j, lo, hi)) o = -1;
  batch.o[lane] = o, batch.j[lane] = j, batch.lo[lane] = lo, batch.hi[lane] = hi;
  if (o < 0) return;
  const double* w = l.obs_lin + (long long)o * kBaLin + kBaLinW;
  const double* v = l.vinv + (long long)j * 6;
  const double v00 = v[0], v01 = v[1], v02 = v[2], v11 = v[3], v12 = v[4], v22 = v[5];
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    const double w0 = w[3 * r], w1 = w[3 * r + 1], w2 = w[3 * r + 2];
    batch.y[lane][3 * r] = w0 * v00 + w1 * v01 + w2 * v02;
    batch.y[lane][3 * r + 1] = w0 * v01 + w1 * v11 + w2 * v12;
    batch.y[lane][3 * r + 2] = w0 * v02 + w1 * v12 + w2 * v22;
  }
}

// Camera a's list of cam_obs -> false where its offsets delimit nothing: the camera is skipped, nothing of it read.
__host__ __device__ __forceinline__ bool ba_camera_list(const int32_t* __restrict__ cam_offsets, int a, int total, int& first, int& last) {
  first = cam_offsets[a], last = cam_offsets[a + 1];
  return first >= 0 && last >= first && last <= total;
}

// The camera pass of one wave: camera a's list 64 entries at a time, one prepared per lane and left in LDS between two barriers
// (at trip counts the whole wave shares), then every lane calls visit(o, j, lo, hi, y) for the batch's usable observations in order.
template <typename Visit>
__device__ __forceinline__ void ba_camera_walk(const BaProblem& d, const BaLinear& l, const int32_t* __restrict__ cam_offsets,
                                               const int32_t* __restrict__ cam_obs, const int32_t* __restrict__ obs_point, int a, int lane,
                                               BaBatch& batch, Visit visit) {
  int first, last;
  if (!ba_camera_list(cam_offsets, a, d.total, first, last)) return;
  for (int base = first; base < last; base += kBaWave) {
    ba_prepare(d, l, cam_obs, obs_point, a, base + lane, last, lane, batch);
    __syncthreads();
    const int m = last - base < kBaWave ? last - base : kBaWave;
    for (int k = 0; k < m; ++k)
      if (batch.o[k] >= 0) visit(batch.o[k], batch.j[k], batch.lo[k], batch.hi[k], batch.y[k]);
    __syncthreads();
  }
}

// One lane's additions for observation o of camera a (point j, track lo .. hi): its entry of U_a, of the two sums of g_a and,
// along the track, of the blocks of sum Y W' it owns.  acc: the row block [n_cams][36]; y: the observation's 18 numbers of ba_prepare.
__host__ __device__ __forceinline__ void ba_lane_update(const BaProblem& d, const BaLinear& l, int a, int o, int j, int lo, int hi,
                                                        int lane, const double* y, double* acc, BaLane& s) {
  const double* lin = l.obs_lin + (long long)o * kBaLin;
  const int ea = ((lane - 36 * a) % kBaWave + kBaWave) % kBaWave;             // the entry of block a this lane owns, if < 36
  if (ea < 36) s.u += lin[ea / 6] * lin[ea % 6] + lin[6 + ea / 6] * lin[6 + ea % 6];
  if (lane < 6) {
    const double* gp = l.gp + (long long)j * 3;
    s.gr += lin[lane] * lin[kBaLinR] + lin[6 + lane] * lin[kBaLinR + 1];
    s.gy += y[3 * lane] * gp[0] + y[3 * lane + 1] * gp[1] + y[3 * lane + 2] * gp[2];
  }
  // the flag and the camera of the next track element are loaded while this one's W is on its way
  bool ok_next = lo < hi && l.obs_ok[lo] != 0;
  int b_next = lo < hi ? d.obs_cam[lo] : 0;
  for (int o2 = lo; o2 < hi; ++o2) {
    const bool ok = ok_next;
    const int b = b_next;
    if (o2 + 1 < hi) ok_next = l.obs_ok[o2 + 1] != 0, b_next = d.obs_cam[o2 + 1];
    if (!ok || b < 0 || b >= d.n_cams) continue;
    const int e = ((lane - 36 * b) % kBaWave + kBaWave) % kBaWave;
    if (e >= 36) continue;
    const double* w = l.obs_lin + (long long)o2 * kBaLin + kBaLinW + 3 * (e % 6);
    const double* yr = y + 3 * (e / 6);
    acc[36 * b + e] += yr[0] * w[0] + yr[1] * w[1] + yr[2] * w[2];
  }
}

// What a lane writes when camera a's list is through: its entries of S's row block and of g.
__host__ __device__ __forceinline__ void ba_lane_finish(int n_cams, unsigned held, double lambda, int a, int lane, const double* acc,
                                                        const BaLane& s, double* __restrict__ S, double* __restrict__ g) {
  for (int idx = lane; idx < 36 * n_cams; idx += kBaWave) {
    const int b = idx / 36, r = idx % 36 / 6, c = idx % 6;
    double u = 0.0;
    if (b == a) {
      u = s.u;
      // a held parameter, or one that no usable observation moves, has the diagonal 1 and zero rows and columns
      if (r == c) u = ((held >> r) & 1u) || u == 0.0 ? 1.0 : u + lambda * u;
    }
    S[(long long)(6 * a + r) * (6 * n_cams) + 6 * b + c] = u - acc[idx];
  }
  if (lane < 6) g[6 * a + lane] = s.gr - s.gy;
}

// ---- the solver without S (vc_ba_camera_blocks, vc_ba_schur_product; "The solver" in DESIGN.md §4.2k) -----------------------------
// Preconditioned conjugate gradients on S dc = -g need, per camera, U_a, the diagonal block D_a = S_aa, its inverse and g_a, and
// per iteration q = S p = U p - sum W V^-1 sum W' p, which two passes over what the points pass left compute without S.
constexpr int kBaProductThreads = 256;         // entries of a camera's list that the product's camera pass resolves between barriers

// The registers of one lane of the blocks pass: entry e = lane = 6 r + c of U_a and of (sum Y W')_aa (lanes 0 .. 35), the two sums
// of g_a (lanes 0 .. 5).
struct BaBlockLane {
  double u, acc, gr, gy;
};

// One lane's additions for observation o of camera a (point j, track lo .. hi): what ba_lane_update adds to its entries of block
// a and of g, in its order, and nothing of any other block.
__host__ __device__ __forceinline__ void ba_block_update(const BaProblem& d, const BaLinear& l, int a, int o, int j, int lo, int hi,
                                                         int lane, const double* y, BaBlockLane& s) {
  const double* lin = l.obs_lin + (long long)o * kBaLin;
  if (lane < 6) {
    const double* gp = l.gp + (long long)j * 3;
    s.gr += lin[lane] * lin[kBaLinR] + lin[6 + lane] * lin[kBaLinR + 1];
    s.gy += y[3 * lane] * gp[0] + y[3 * lane + 1] * gp[1] + y[3 * lane + 2] * gp[2];
  }
  if (lane >= 36) return;
  const int r = lane / 6, c = lane % 6;
  s.u += lin[r] * lin[c] + lin[6 + r] * lin[6 + c];
  const double* yr = y + 3 * r;
  for (int o2 = lo; o2 < hi; ++o2) {
    if (!l.obs_ok[o2] || d.obs_cam[o2] != a) continue;                        // the observation itself and a camera twice in a track included
    const double* w = l.obs_lin + (long long)o2 * kBaLin + kBaLinW + 3 * c;
    s.acc += yr[0] * w[0] + yr[1] * w[1] + yr[2] * w[2];
  }
}

// Entry e of U_a as the system has it: the diagonal damped, or 1 where the parameter is fixed (held, or no usable observation
// moves it) -> fixed, for the diagonal entries.
__host__ __device__ __forceinline__ double ba_block_u(unsigned held, double lambda, int e, double u, bool& fixed) {
  fixed = false;
  if (e / 6 != e % 6) return u;
  fixed = ((held >> (e / 6)) & 1u) || u == 0.0;
  return fixed ? 1.0 : u + lambda * u;
}

// Column k of D^-1 for the symmetric 6x6 D (row-major, its lower triangle is read): D = L L' by rows, L y = e_k, L' x = y, every
// sum subtracted from its first term left to right.  A pivot that is not finite and positive: column k of the identity.
__host__ __device__ __forceinline__ void ba_block_inverse(const double* D, int k, double (&x)[6]) {
  double L[6][6], y[6];
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double s = D[6 * j + j];
#pragma unroll
    for (int m = 0; m < j; ++m) s -= L[j][m] * L[j][m];
    ok = ok && s > 0.0 && s < INFINITY;                                       // false for NaN
    const double piv = sqrt(s);
    L[j][j] = piv;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double t = D[6 * i + j];
#pragma unroll
      for (int m = 0; m < j; ++m) t -= L[i][m] * L[j][m];
      L[i][j] = t / piv;
    }
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double s = i == k ? 1.0 : 0.0;
#pragma unroll
    for (int m = 0; m < i; ++m) s -= L[i][m] * y[m];
    y[i] = s / L[i][i];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double s = y[i];
#pragma unroll
    for (int m = i + 1; m < 6; ++m) s -= L[m][i] * x[m];
    x[i] = s / L[i][i];
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) x[i] = ok ? x[i] : i == k ? 1.0 : 0.0;
}

// Entry i of p as the product reads it: 0 at a fixed parameter.
__host__ __device__ __forceinline__ double ba_product_entry(const uint8_t* __restrict__ fixed, const double* __restrict__ p, long long i) {
  return fixed[i] ? 0.0 : p[i];
}

// The points pass of the product, point j: s_j = V^-1 sum W' p over the usable observations of the track in track order; 0 where
// the point's offsets delimit nothing (nothing of it is read) and where the point is constant.
__host__ __device__ __forceinline__ void ba_product_point(const BaProblem& d, const BaLinear& l, const uint8_t* __restrict__ fixed,
                                                          const double* __restrict__ p, int j, double (&s)[3]) {
  s[0] = s[1] = s[2] = 0.0;
  int lo, hi;
  if (!ba_track(d.offsets, j, d.total, lo, hi)) return;
  double t[3] = {0.0, 0.0, 0.0};
  for (int o = lo; o < hi; ++o) {
    if (!l.obs_ok[o]) continue;
    const int b = d.obs_cam[o];
    if (b < 0 || b >= d.n_cams) continue;
    const double* w = l.obs_lin + (long long)o * kBaLin + kBaLinW;
    double e[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) e[i] = ba_product_entry(fixed, p, 6 * (long long)b + i);
#pragma unroll
    for (int k = 0; k < 3; ++k)
      t[k] += w[k] * e[0] + w[3 + k] * e[1] + w[6 + k] * e[2] + w[9 + k] * e[3] + w[12 + k] * e[4] + w[15 + k] * e[5];
  }
  const double* v = l.vinv + (long long)j * 6;
  s[0] = v[0] * t[0] + v[1] * t[1] + v[2] * t[2];
  s[1] = v[1] * t[0] + v[3] * t[1] + v[4] * t[2];
  s[2] = v[2] * t[0] + v[4] * t[1] + v[5] * t[2];
}

// What the lanes of the product's camera pass leave for the six owners: whether entry base + lane of camera a's list is a usable
// observation and, for one, W s of its point (6 numbers), parameter-major so that the lanes' stores do not collide.
struct BaProductBatch {
  int ok[kBaProductThreads];
  double c[6][kBaProductThreads];
};

// o: the entry of cam_obs that lane `lane` of the batch resolves, -1 past the end of the list.
__host__ __device__ __forceinline__ void ba_product_prepare(const BaProblem& d, const BaLinear& l, const int32_t* __restrict__ obs_point,
                                                            const double* __restrict__ s, int a, int o, int lane, BaProductBatch& batch) {
  int j = 0, lo = 0, hi = 0;
  const bool ok = ba_camera_obs_at(d, l, obs_point, a, o, j, lo, hi);
  batch.ok[lane] = ok ? 1 : 0;
  if (!ok) return;
  const double* w = l.obs_lin + (long long)o * kBaLin + kBaLinW;
  const double s0 = s[3 * (long long)j], s1 = s[3 * (long long)j + 1], s2 = s[3 * (long long)j + 2];
#pragma unroll
  for (int r = 0; r < 6; ++r) batch.c[r][lane] = w[3 * r] * s0 + w[3 * r + 1] * s1 + w[3 * r + 2] * s2;
}

// Owner lane i adds the first m entries of a batch to its sum, in list order.
__host__ __device__ __forceinline__ void ba_product_add(const BaProductBatch& batch, int m, int i, double& sum) {
  for (int k = 0; k < m; ++k)
    if (batch.ok[k]) sum += batch.c[i][k];
}

// Entry i of q_a = U_a p_a - sum W s, the row of U left to right; a fixed parameter returns its entry of p as it is.
__host__ __device__ __forceinline__ double ba_product_finish(const double* __restrict__ U, const uint8_t* __restrict__ fixed,
                                                             const double* __restrict__ p, int a, int i, double sum) {
  const long long at = 6 * (long long)a;
  if (fixed[at + i]) return p[at + i];
  const double* u = U + 36 * (long long)a + 6 * i;
  double e[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) e[k] = ba_product_entry(fixed, p, at + k);
  return (u[0] * e[0] + u[1] * e[1] + u[2] * e[2] + u[3] * e[3] + u[4] * e[4] + u[5] * e[5]) - sum;
}

// One camera's pose update without trigonometry: q = (1, w / 2) / |(1, w / 2)|, R <- R(q) R, t <- t + dt; the intrinsics are copied.
__host__ __device__ __forceinline__ void ba_pose_step(const double* __restrict__ cam, const double* __restrict__ e,
                                                      double* __restrict__ out) {
  const double hx = 0.5 * e[0], hy = 0.5 * e[1], hz = 0.5 * e[2];
  const double n = sqrt(1.0 + hx * hx + hy * hy + hz * hz);
  const double w = 1.0 / n, x = hx / n, y = hy / n, z = hz / n;
  const double Q[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                       2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                       2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)};
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int k = 0; k < 3; ++k) out[3 * i + k] = Q[3 * i] * cam[k] + Q[3 * i + 1] * cam[3 + k] + Q[3 * i + 2] * cam[6 + k];
#pragma unroll
  for (int i = 0; i < 3; ++i) out[9 + i] = cam[9 + i] + e[3 + i];
#pragma unroll
  for (int i = 12; i < 16; ++i) out[i] = cam[i];
}

// ---- the border of the intrinsics (linearize intrinsics, reduce border, the step with groups) -----------------------------------
// The N = ba_dist_unknowns(kDist) unknowns theta_g of every group of cameras, (fx, fy, cx, cy) and the model's row of cam_dist
// after them, join the reduced system as a border [[S, B], [B', C]]; S and g stay vc_ba_reduce_cameras'.  T_{j,g} = sum J_theta' J_p
// is Nx3 row-major.
constexpr int kBaBorderSlots = (24 * VC_BA_MAX_GROUPS + kBaWave - 1) / kBaWave;   // entries of a camera's B row block per lane
static_assert((36 * VC_BA_MAX_GROUPS_RADIAL + kBaWave - 1) / kBaWave <= kBaBorderSlots, "B_a [6][6 G] of the radial limit must fit a lane's slots");
static_assert((48 * VC_BA_MAX_GROUPS_OPENCV + kBaWave - 1) / kBaWave <= kBaBorderSlots, "B_a [6][8 G] of the OPENCV limit must fit a lane's slots");

struct BaGroups {
  const int32_t* __restrict__ cam_group;       // [n_cams]
  const uint8_t* __restrict__ intr_mask;       // [n_groups]: bits 0-3 fx fy cx cy held, bit 4 tied; radial: bits 5, 6 k1, k2 held; OPENCV: bit 7 p1, p2
  int n_groups;
};

// The rows of the per-point terms [ba_term_rows(G)][n_points] (entry-major: a point per lane writes a row and a wave per row
// reads it, both coalesced): q_{j,g} NxN, hq_{j,g}, p_{j,g} = T V^-1 g_p, P_{j,g,g'} = T_g V^-1 T_g'' NxN.
template <int N>
__host__ __device__ constexpr int ba_term_q(int G, int g) { return N * N * g; }
template <int N>
__host__ __device__ constexpr int ba_term_hq(int G, int g) { return N * N * G + N * g; }
template <int N>
__host__ __device__ constexpr int ba_term_p(int G, int g) { return (N * N + N) * G + N * g; }
template <int N>
__host__ __device__ constexpr int ba_term_P(int G, int g, int g2) { return (N * N + 2 * N) * G + N * N * (g * G + g2); }
template <int N>
__host__ __device__ constexpr int ba_term_rows(int G) { return (N * N + 2 * N) * G + N * N * G * G; }

// Camera slot -> its group, -1 where the slot's group is outside [0, n_groups): its intrinsics are held.  Without groups
// cam_group is not read.
__host__ __device__ __forceinline__ int ba_group_of(const BaGroups& gr, int slot) {
  if (gr.n_groups <= 0) return -1;
  const int g = gr.cam_group[slot];
  return g >= 0 && g < gr.n_groups ? g : -1;
}

// Parameter i < N of a group is held: fx fy cx cy by bits 0-3 of its mask, fy of a tied group (bit 4) too; k1 (i = 4) by bit 5,
// k2 (i = 5) by bit 6; p1 (i = 6) and p2 (i = 7) together by bit 7.
template <int N>
__host__ __device__ __forceinline__ bool ba_theta_held(unsigned mask, int i) {
  if (N > 6 && i >= 6) return ((mask >> 7) & 1u) != 0;
  if (N > 4 && i >= 4) return ((mask >> (i + 1)) & 1u) != 0;
  return ((mask >> i) & 1u) || (((mask >> 4) & 1u) && i == 1);
}

// Column i of J_theta = [[xd, 0, 1, 0, pu, qu, ..], [0, yd, 0, 1, pv, qv, ..]] from the observation's row jt of obs_jt: (x, y) for the
// pinhole, (xd, yd, pu, pv, qu, qv) under the radial distortion, then the p1 column (jt[6], jt[7]) and the p2 column (jt[8], jt[9])
// under OPENCV; tied: column 0 is (xd, yd); a held column is 0.  i may be a runtime value: the column is selected, not indexed.
template <int kDist>
__host__ __device__ __forceinline__ void ba_jtheta(unsigned mask, const double* jt, int i, double& tu, double& tv) {
  const bool tied = (mask >> 4) & 1u;
  tu = i == 0 ? jt[0] : i == 2 ? 1.0 : 0.0;
  tv = i == 0 ? (tied ? jt[1] : 0.0) : i == 1 ? jt[1] : i == 3 ? 1.0 : 0.0;
  if constexpr (kDist != kBaDistNone) {
    tu = i == 4 ? jt[2] : i == 5 ? jt[4] : tu;
    tv = i == 4 ? jt[3] : i == 5 ? jt[5] : tv;
  }
  if constexpr (kDist == kBaDistOpencv) {
    tu = i == 6 ? jt[6] : i == 7 ? jt[8] : tu;
    tv = i == 6 ? jt[7] : i == 7 ? jt[9] : tv;
  }
  if (ba_theta_held<ba_dist_unknowns(kDist)>(mask, i)) tu = tv = 0.0;
}

// A usable observation of X in camera slot again: its row of obs_jt and J_p.  The pinhole projects with the row as it is.
template <int kDist>
__host__ __device__ __forceinline__ void ba_observe_point(const BaProblem& d, int slot, const double (&X)[3], BaDistortion<kDist>& rd,
                                                          double (&ju)[3], double (&jv)[3]) {
  const double* c = d.cams + 16 * (long long)slot;
  double Y[3], Xc[3], fu, fv, xu, xv;
  if constexpr (kDist == kBaDistNone) ba_project(c, X, Y, Xc, fu, fv, rd.jt[0], rd.jt[1], ju, jv);
  else ba_project_dist<kDist>(c, d.cam_dist + ba_dist_params(kDist) * (long long)slot, X, Y, Xc, fu, xu, xv, rd, ju, jv);
}

// One point: obs_jt of its track; per group (outside) over the track (inside) T, q, hq; then the point's products with V^-1.
// A point whose offsets delimit nothing has T and its terms 0 and nothing of its track read or written.  With a loss J_p and
// J_theta (its constant columns too) are multiplied by obs_w[o], as the points pass multiplied what it left in obs_lin; obs_jt
// stays unscaled: the row of ba_observe_point of a usable observation, zeros of any other.
template <bool kLoss, int kDist>
__host__ __device__ __forceinline__ void ba_linearize_point_intrinsics(const BaProblem& d, const BaLinear& l, const BaGroups& gr,
                                                                       const double* __restrict__ obs_w, int j, double* __restrict__ obs_jt,
                                                                       double* T, double* __restrict__ terms) {
  constexpr int N = ba_dist_unknowns(kDist), NT = 3 * N, kJt = ba_dist_jt(kDist);
  const int G = gr.n_groups;
  const long long n = d.n_points;
  int lo, hi;
  if (!ba_track(d.offsets, j, d.total, lo, hi)) lo = hi = 0;
  double X[3] = {0.0, 0.0, 0.0};
  if (lo < hi) X[0] = d.points[3 * (long long)j], X[1] = d.points[3 * (long long)j + 1], X[2] = d.points[3 * (long long)j + 2];
  for (int o = lo; o < hi; ++o) {
    const int slot = d.obs_cam[o];
    BaDistortion<kDist> rd;
    double ju[3], jv[3];
#pragma unroll
    for (int k = 0; k < kJt; ++k) rd.jt[k] = 0.0;
    if (l.obs_ok[o] && slot >= 0 && slot < d.n_cams) ba_observe_point<kDist>(d, slot, X, rd, ju, jv);
#pragma unroll
    for (int k = 0; k < kJt; ++k) obs_jt[kJt * (long long)o + k] = rd.jt[k];
  }
  double* Tj = T + (long long)j * G * NT;
  for (int g = 0; g < G; ++g) {
    const unsigned mask = gr.intr_mask[g];
    double t[NT], q[N * N], hq[N];
#pragma unroll
    for (int k = 0; k < NT; ++k) t[k] = 0.0;
#pragma unroll
    for (int k = 0; k < N * N; ++k) q[k] = 0.0;
#pragma unroll
    for (int k = 0; k < N; ++k) hq[k] = 0.0;
    for (int o = lo; o < hi; ++o) {
      const int slot = d.obs_cam[o];
      if (!l.obs_ok[o] || slot < 0 || slot >= d.n_cams || ba_group_of(gr, slot) != g) continue;
      BaDistortion<kDist> rd;
      double ju[3], jv[3], tu[N], tv[N];
      ba_observe_point<kDist>(d, slot, X, rd, ju, jv);
#pragma unroll
      for (int i = 0; i < N; ++i) ba_jtheta<kDist>(mask, rd.jt, i, tu[i], tv[i]);
      if (kLoss) {
        const double sw = obs_w[o];
#pragma unroll
        for (int k = 0; k < 3; ++k) ju[k] = sw * ju[k], jv[k] = sw * jv[k];
#pragma unroll
        for (int i = 0; i < N; ++i) tu[i] = sw * tu[i], tv[i] = sw * tv[i];
      }
      const double ru = l.obs_lin[(long long)o * kBaLin + kBaLinR], rv = l.obs_lin[(long long)o * kBaLin + kBaLinR + 1];
#pragma unroll
      for (int i = 0; i < N; ++i) {
#pragma unroll
        for (int k = 0; k < 3; ++k) t[3 * i + k] += tu[i] * ju[k] + tv[i] * jv[k];
#pragma unroll
        for (int k = 0; k < N; ++k) q[N * i + k] += tu[i] * tu[k] + tv[i] * tv[k];
        hq[i] += tu[i] * ru + tv[i] * rv;
      }
    }
#pragma unroll
    for (int k = 0; k < NT; ++k) Tj[g * NT + k] = t[k];
#pragma unroll
    for (int k = 0; k < N * N; ++k) terms[(ba_term_q<N>(G, g) + k) * n + j] = q[k];
#pragma unroll
    for (int k = 0; k < N; ++k) terms[(ba_term_hq<N>(G, g) + k) * n + j] = hq[k];
  }
  const double* v = l.vinv + (long long)j * 6;
  const double v00 = v[0], v01 = v[1], v02 = v[2], v11 = v[3], v12 = v[4], v22 = v[5];
  const double g0 = l.gp[3 * (long long)j], g1 = l.gp[3 * (long long)j + 1], g2 = l.gp[3 * (long long)j + 2];
  for (int g = 0; g < G; ++g) {
    double tv[NT];                                                            // T_g V^-1, as Y = W V^-1 is formed
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const double t0 = Tj[g * NT + 3 * i], t1 = Tj[g * NT + 3 * i + 1], t2 = Tj[g * NT + 3 * i + 2];
      tv[3 * i] = t0 * v00 + t1 * v01 + t2 * v02;
      tv[3 * i + 1] = t0 * v01 + t1 * v11 + t2 * v12;
      tv[3 * i + 2] = t0 * v02 + t1 * v12 + t2 * v22;
      terms[(ba_term_p<N>(G, g) + i) * n + j] = tv[3 * i] * g0 + tv[3 * i + 1] * g1 + tv[3 * i + 2] * g2;
    }
    for (int h = 0; h < G; ++h) {
      const double* th = Tj + h * NT;
#pragma unroll
      for (int i = 0; i < N; ++i)
#pragma unroll
        for (int k = 0; k < N; ++k)
          terms[(ba_term_P<N>(G, g, h) + N * i + k) * n + j] = tv[3 * i] * th[3 * k] + tv[3 * i + 1] * th[3 * k + 1] + tv[3 * i + 2] * th[3 * k + 2];
    }
  }
}

// Parameter i of group g moves: not held, not parameter 1 of a tied group, and some usable observation moves it (Q_ii != 0).
template <int N>
__host__ __device__ __forceinline__ bool ba_theta_free(const double* __restrict__ sums, const BaGroups& gr, int g, int i) {
  return !ba_theta_held<N>(gr.intr_mask[g], i) && sums[ba_term_q<N>(gr.n_groups, g) + (N + 1) * i] != 0.0;
}

// Entry (row, col) of C from the ordered sums: delta Q (its diagonal damped) - sum P; the identity where a parameter does not move.
template <int N>
__host__ __device__ __forceinline__ double ba_border_c(const double* __restrict__ sums, const BaGroups& gr, double lambda, int row, int col) {
  const int G = gr.n_groups, g = row / N, i = row % N, h = col / N, k = col % N;
  if (!ba_theta_free<N>(sums, gr, g, i) || !ba_theta_free<N>(sums, gr, h, k)) return row == col ? 1.0 : 0.0;
  double q = 0.0;
  if (g == h) {
    q = sums[ba_term_q<N>(G, g) + N * i + k];
    if (i == k) q += lambda * q;
  }
  return q - sums[ba_term_P<N>(G, g, h) + N * i + k];
}

template <int N>
__host__ __device__ __forceinline__ double ba_border_h(const double* __restrict__ sums, const BaGroups& gr, int row) {
  const int G = gr.n_groups, g = row / N, i = row % N;
  return ba_theta_free<N>(sums, gr, g, i) ? sums[ba_term_hq<N>(G, g) + i] - sums[ba_term_p<N>(G, g) + i] : 0.0;
}

// The registers of one lane of the border's camera pass: entry idx = lane + 64 k of the row block B_a [6][N G], as g = idx / (6 N),
// r = idx % (6 N) / N, i = idx % N, and its two sums.
struct BaBorderLane {
  double jt[kBaBorderSlots], yt[kBaBorderSlots];
};

// One lane's additions for the usable observation o of camera a (its group ga or -1, its point j, y as ba_prepare left it).
// With a loss the column of J_theta is multiplied by obs_w[o]; obs_lin and T carry the weight already.
template <bool kLoss, int kDist>
__host__ __device__ __forceinline__ void ba_border_update(const BaLinear& l, const BaGroups& gr, const double* __restrict__ obs_jt,
                                                          const double* __restrict__ obs_w, const double* __restrict__ T, int ga, int o,
                                                          int j, int lane, const double* y, BaBorderLane& s) {
  constexpr int N = ba_dist_unknowns(kDist), kJt = ba_dist_jt(kDist);
  const int G = gr.n_groups;
  const double sw = kLoss ? obs_w[o] : 1.0;
  const double* lin = l.obs_lin + (long long)o * kBaLin;
  const unsigned mask = ga >= 0 ? gr.intr_mask[ga] : 0u;
  double jt[kJt];
#pragma unroll
  for (int k = 0; k < kJt; ++k) jt[k] = obs_jt[kJt * (long long)o + k];
#pragma unroll
  for (int k = 0; k < kBaBorderSlots; ++k) {
    const int idx = lane + kBaWave * k;
    if (idx >= 6 * N * G) continue;
    const int g = idx / (6 * N), r = idx % (6 * N) / N, i = idx % N;
    if (g == ga) {
      double tu, tv;
      ba_jtheta<kDist>(mask, jt, i, tu, tv);
      if (kLoss) tu = sw * tu, tv = sw * tv;
      s.jt[k] += lin[r] * tu + lin[6 + r] * tv;
    }
    const double* t = T + ((long long)j * G + g) * (3 * N) + 3 * i;
    s.yt[k] += y[3 * r] * t[0] + y[3 * r + 1] * t[1] + y[3 * r + 2] * t[2];
  }
}

template <int N>
__host__ __device__ __forceinline__ void ba_border_finish(int G, int a, int lane, const BaBorderLane& s, double* __restrict__ B) {
#pragma unroll
  for (int k = 0; k < kBaBorderSlots; ++k) {
    const int idx = lane + kBaWave * k;
    if (idx < 6 * N * G) B[(long long)(6 * a + idx % (6 * N) / N) * (N * G) + N * (idx / (6 * N)) + idx % N] = s.jt[k] - s.yt[k];
  }
}

// One point's step: dX = -V^-1 (g_p + sum W' dc + sum_g T_g' dtheta_g), the track in track order, then the groups in ascending
// order, a group's N products added left to right onto the first; 0 where the point's offsets delimit nothing.  Without groups T
// and dtheta are not read.
template <int N>
__host__ __device__ __forceinline__ void ba_point_step(const BaProblem& d, const BaLinear& l, const double* __restrict__ T, int G,
                                                       const double* __restrict__ dc, const double* __restrict__ dtheta, int j,
                                                       double (&dX)[3]) {
  dX[0] = dX[1] = dX[2] = 0.0;
  int lo, hi;
  if (!ba_track(d.offsets, j, d.total, lo, hi)) return;
  double s[3] = {l.gp[3 * (long long)j], l.gp[3 * (long long)j + 1], l.gp[3 * (long long)j + 2]};
  for (int o = lo; o < hi; ++o) {
    if (!l.obs_ok[o]) continue;
    const int b = d.obs_cam[o];
    if (b < 0 || b >= d.n_cams) continue;
    const double* w = l.obs_lin + (long long)o * kBaLin + kBaLinW;
    const double* e = dc + 6 * (long long)b;
#pragma unroll
    for (int k = 0; k < 3; ++k)
      s[k] += w[k] * e[0] + w[3 + k] * e[1] + w[6 + k] * e[2] + w[9 + k] * e[3] + w[12 + k] * e[4] + w[15 + k] * e[5];
  }
  for (int g = 0; g < G; ++g) {
    const double* t = T + ((long long)j * G + g) * (3 * N);
    const double* e = dtheta + N * g;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      double sum = t[k] * e[0];
#pragma unroll
      for (int i = 1; i < N; ++i) sum = sum + t[3 * i + k] * e[i];
      s[k] += sum;
    }
  }
  const double* v = l.vinv + (long long)j * 6;
  dX[0] = -(v[0] * s[0] + v[1] * s[1] + v[2] * s[2]);
  dX[1] = -(v[1] * s[0] + v[3] * s[1] + v[4] * s[2]);
  dX[2] = -(v[2] * s[0] + v[4] * s[1] + v[5] * s[2]);
}

// One camera's step: ba_pose_step, then (fx, fy, cx, cy) += dtheta_0 .. dtheta_3 of its group (tied: dtheta_0 to both focal lengths)
// and its row of cam_dist += the dtheta after them into out_dist (copied where the intrinsics are held: no group, or one outside
// the table) -> whether the candidate's focal lengths are finite and positive and its distortion finite (true where held).  The
// pinhole has neither dist nor out_dist.
template <int kDist>
__host__ __device__ __forceinline__ bool ba_camera_step(const double* __restrict__ cam, const double* __restrict__ dist,
                                                        const double* __restrict__ e, const BaGroups& gr, int a,
                                                        const double* __restrict__ dtheta, double* __restrict__ out,
                                                        double* __restrict__ out_dist) {
  constexpr int kParams = ba_dist_params(kDist);
  ba_pose_step(cam, e, out);
#pragma unroll
  for (int i = 0; i < kParams; ++i) out_dist[i] = dist[i];
  const int g = ba_group_of(gr, a);
  if (g < 0) return true;
  const double* th = dtheta + ba_dist_unknowns(kDist) * g;
  const bool tied = (gr.intr_mask[g] >> 4) & 1u;
  const double fx = cam[12] + th[0], fy = cam[13] + (tied ? th[0] : th[1]);
  out[12] = fx, out[13] = fy, out[14] = cam[14] + th[2], out[15] = cam[15] + th[3];
  bool valid = ba_finite(fx) && ba_finite(fy) && fx > 0.0 && fy > 0.0;
#pragma unroll
  for (int i = 0; i < kParams; ++i) {
    const double k = dist[i] + th[4 + i];
    out_dist[i] = k;
    valid = valid && ba_finite(k);
  }
  return valid;
}

// ---- the kernels of the passes.  Without a loss, loss and obs_w are absent and not read; cam_dist travels in the BaProblem ------
template <bool kLoss, int kDist>
__global__ __launch_bounds__(kBaWave) void ba_linearize_points_kernel(BaProblem d, double lambda, BaLoss loss, double* __restrict__ out_vinv,
                                                                      double* __restrict__ out_gp, double* __restrict__ out_cost,
                                                                      int32_t* __restrict__ out_count, uint8_t* __restrict__ out_obs_ok,
                                                                      double* __restrict__ out_obs_lin, double* __restrict__ out_obs_w) {
  const long long j = (long long)blockIdx.x * kBaWave + threadIdx.x;
  if (j >= d.n_points) return;
  double vinv[6], gp[3], cost;
  const int count = ba_linearize_point<kLoss, kDist>(d, loss, (int)j, lambda, vinv, gp, cost, out_obs_ok, out_obs_lin, out_obs_w);
#pragma unroll
  for (int k = 0; k < 6; ++k) out_vinv[6 * j + k] = vinv[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) out_gp[3 * j + k] = gp[k];
  out_cost[j] = cost;
  out_count[j] = count;
}

// Row blockIdx.x of [rows][n] added in ascending order, one wave per row: a lane loads, every lane adds the 64 values in order.
// The total cost is the one row of the points' costs; the border's sums are the rows of its terms.
__global__ __launch_bounds__(kBaWave) void ba_ordered_sums_kernel(const double* __restrict__ terms, int n, double* __restrict__ out_sums) {
  const double* row = terms + (long long)blockIdx.x * n;
  double sum = 0.0;
  for (int base = 0; base < n; base += kBaWave) {
    const double v = base + (int)threadIdx.x < n ? row[base + threadIdx.x] : 0.0;
    const int m = n - base < kBaWave ? n - base : kBaWave;
    for (int k = 0; k < m; ++k) sum += __shfl(v, k, kBaWave);
  }
  if (threadIdx.x == 0) out_sums[blockIdx.x] = sum;
}

__global__ __launch_bounds__(kBaWave) void ba_reduce_cameras_kernel(BaProblem d, BaLinear l, const int32_t* __restrict__ cam_offsets,
                                                                    const int32_t* __restrict__ cam_obs,
                                                                    const int32_t* __restrict__ obs_point, double lambda,
                                                                    double* __restrict__ out_S, double* __restrict__ out_g) {
  extern __shared__ __attribute__((aligned(16))) double ba_lds[];             // the row block [n_cams][36]
  __shared__ BaBatch batch;
  double* acc = ba_lds;
  const int a = blockIdx.x, lane = threadIdx.x;
  for (int idx = lane; idx < 36 * d.n_cams; idx += kBaWave) acc[idx] = 0.0;  // a lane's own entries: no barrier needed
  BaLane s{0.0, 0.0, 0.0};
  ba_camera_walk(d, l, cam_offsets, cam_obs, obs_point, a, lane, batch,
                 [&](int o, int j, int lo, int hi, const double* y) { ba_lane_update(d, l, a, o, j, lo, hi, lane, y, acc, s); });
  ba_lane_finish(d.n_cams, d.const_mask[a], lambda, a, lane, acc, s, out_S, out_g);
}

// U_a, D_a, D_a^-1, g_a and the fixed flags: one wave per camera over its list, a lane's entry of the two blocks in its registers;
// D_a passes through LDS to the six lanes that each invert it for one column.
__global__ __launch_bounds__(kBaWave) void ba_camera_blocks_kernel(BaProblem d, BaLinear l, const int32_t* __restrict__ cam_offsets,
                                                                   const int32_t* __restrict__ cam_obs,
                                                                   const int32_t* __restrict__ obs_point, double lambda,
                                                                   double* __restrict__ out_U, double* __restrict__ out_D,
                                                                   double* __restrict__ out_Minv, double* __restrict__ out_g,
                                                                   uint8_t* __restrict__ out_fixed) {
  __shared__ BaBatch batch;
  __shared__ double block[36];
  __shared__ int fixed_of[6];
  const int a = blockIdx.x, lane = threadIdx.x;
  BaBlockLane s{0.0, 0.0, 0.0, 0.0};
  ba_camera_walk(d, l, cam_offsets, cam_obs, obs_point, a, lane, batch,
                 [&](int o, int j, int lo, int hi, const double* y) { ba_block_update(d, l, a, o, j, lo, hi, lane, y, s); });
  if (lane < 36) {
    bool fixed;
    const double u = ba_block_u(d.const_mask[a], lambda, lane, s.u, fixed);
    const double dd = u - s.acc;
    out_U[36 * (long long)a + lane] = u, out_D[36 * (long long)a + lane] = dd;
    block[lane] = dd;
    if (lane / 6 == lane % 6) fixed_of[lane / 6] = fixed ? 1 : 0, out_fixed[6 * (long long)a + lane / 6] = fixed ? 1 : 0;
  }
  __syncthreads();
  if (lane < 6) {
    out_g[6 * (long long)a + lane] = fixed_of[lane] ? 0.0 : s.gr - s.gy;
    double x[6];
    ba_block_inverse(block, lane, x);
#pragma unroll
    for (int i = 0; i < 6; ++i) out_Minv[36 * (long long)a + 6 * i + lane] = x[i];
  }
}

__global__ __launch_bounds__(kBaWave) void ba_product_points_kernel(BaProblem d, BaLinear l, const uint8_t* __restrict__ fixed,
                                                                    const double* __restrict__ p, double* __restrict__ out_s) {
  const long long j = (long long)blockIdx.x * kBaWave + threadIdx.x;
  if (j >= d.n_points) return;
  double s[3];
  ba_product_point(d, l, fixed, p, (int)j, s);
#pragma unroll
  for (int k = 0; k < 3; ++k) out_s[3 * j + k] = s[k];
}

// q_a: one workgroup of four waves per camera.  Every lane resolves one entry of the list and forms W s for it; lanes 0 .. 5 own
// the six sums and add a batch in list order.  Two batches alternate in LDS and the owners add batch n - 1 after the first load
// of batch n is on its way, so one barrier per batch is enough: a batch is overwritten two barriers after it was written, and
// the owners have added it before the barrier in between.
__global__ __launch_bounds__(kBaProductThreads) void ba_product_cameras_kernel(BaProblem d, BaLinear l, const int32_t* __restrict__ cam_offsets,
                                                                               const int32_t* __restrict__ cam_obs,
                                                                               const int32_t* __restrict__ obs_point,
                                                                               const double* __restrict__ U, const uint8_t* __restrict__ fixed,
                                                                               const double* __restrict__ p, const double* __restrict__ s,
                                                                               double* __restrict__ out_q) {
  __shared__ BaProductBatch batch[2];
  const int a = blockIdx.x, lane = threadIdx.x;
  double sum = 0.0;
  int first, last;
  if (ba_camera_list(cam_offsets, a, d.total, first, last)) {
    int buf = 0, pending = 0;                                                 // entries of the batch the owners have not added yet
    for (long long base = first; base < last; base += kBaProductThreads, buf ^= 1) {
      const int m = last - base < kBaProductThreads ? (int)(last - base) : kBaProductThreads;
      const int o = lane < m ? cam_obs[base + lane] : -1;
      if (lane < 6) ba_product_add(batch[buf ^ 1], pending, lane, sum);
      ba_product_prepare(d, l, obs_point, s, a, o, lane, batch[buf]);
      pending = m;
      __syncthreads();
    }
    if (lane < 6) ba_product_add(batch[buf ^ 1], pending, lane, sum);
  }
  if (lane < 6) out_q[6 * (long long)a + lane] = ba_product_finish(U, fixed, p, a, lane, sum);
}

template <bool kLoss, int kDist>
__global__ __launch_bounds__(kBaWave) void ba_linearize_intrinsics_kernel(BaProblem d, BaLinear l, BaGroups gr, const double* __restrict__ obs_w,
                                                                          double* __restrict__ out_obs_jt, double* out_T,
                                                                          double* __restrict__ out_terms) {
  const long long j = (long long)blockIdx.x * kBaWave + threadIdx.x;
  if (j < d.n_points) ba_linearize_point_intrinsics<kLoss, kDist>(d, l, gr, obs_w, (int)j, out_obs_jt, out_T, out_terms);
}

// C, h and which parameters move, from the ordered sums: one entry per lane.
template <int N>
__global__ __launch_bounds__(kBaWave) void ba_border_system_kernel(const double* __restrict__ sums, BaGroups gr, double lambda,
                                                                   double* __restrict__ out_C, double* __restrict__ out_h,
                                                                   uint8_t* __restrict__ out_free) {
  const int m = N * gr.n_groups;
  for (int idx = threadIdx.x; idx < m * m; idx += kBaWave) out_C[idx] = ba_border_c<N>(sums, gr, lambda, idx / m, idx % m);
  for (int row = threadIdx.x; row < m; row += kBaWave) {
    out_h[row] = ba_border_h<N>(sums, gr, row);
    out_free[row] = ba_theta_free<N>(sums, gr, row / N, row % N) ? 1 : 0;
  }
}

// B_a: one wave per camera over its list, a lane's entries in its registers.
template <bool kLoss, int kDist>
__global__ __launch_bounds__(kBaWave) void ba_reduce_border_kernel(BaProblem d, BaLinear l, BaGroups gr, const int32_t* __restrict__ cam_offsets,
                                                                   const int32_t* __restrict__ cam_obs, const int32_t* __restrict__ obs_point,
                                                                   const double* __restrict__ obs_jt, const double* __restrict__ obs_w,
                                                                   const double* __restrict__ T, double* __restrict__ out_B) {
  __shared__ BaBatch batch;
  const int a = blockIdx.x, lane = threadIdx.x;
  const int ga = ba_group_of(gr, a);
  BaBorderLane s;
#pragma unroll
  for (int k = 0; k < kBaBorderSlots; ++k) s.jt[k] = s.yt[k] = 0.0;
  ba_camera_walk(d, l, cam_offsets, cam_obs, obs_point, a, lane, batch,
                 [&](int o, int j, int, int, const double* y) { ba_border_update<kLoss, kDist>(l, gr, obs_jt, obs_w, T, ga, o, j, lane, y, s); });
  ba_border_finish<ba_dist_unknowns(kDist)>(gr.n_groups, a, lane, s, out_B);
}

template <int N>
__global__ __launch_bounds__(kBaWave) void ba_step_points_kernel(BaProblem d, BaLinear l, const double* __restrict__ T, int n_groups,
                                                                 const double* __restrict__ dc, const double* __restrict__ dtheta,
                                                                 double* __restrict__ out_points, double* __restrict__ out_dx) {
  const long long j = (long long)blockIdx.x * kBaWave + threadIdx.x;
  if (j >= d.n_points) return;
  double dX[3];
  ba_point_step<N>(d, l, T, n_groups, dc, dtheta, (int)j, dX);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    out_dx[3 * j + k] = dX[k];
    out_points[3 * j + k] = d.points[3 * j + k] + dX[k];
  }
}

// out_valid may be absent (vc_ba_step: no intrinsics move, every candidate is valid); the pinhole has no out_dist.
template <int kDist>
__global__ __launch_bounds__(kBaWave) void ba_step_cameras_kernel(BaProblem d, BaGroups gr, const double* __restrict__ dc,
                                                                  const double* __restrict__ dtheta, double* __restrict__ out_cams,
                                                                  double* __restrict__ out_dist, uint8_t* __restrict__ out_valid) {
  constexpr int kParams = ba_dist_params(kDist);
  const long long a = (long long)blockIdx.x * kBaWave + threadIdx.x;
  if (a >= d.n_cams) return;
  const bool valid = ba_camera_step<kDist>(d.cams + 16 * a, d.cam_dist + kParams * a, dc + 6 * a, gr, (int)a, dtheta, out_cams + 16 * a,
                                           out_dist + kParams * a);
  if (out_valid) out_valid[a] = valid ? 1 : 0;
}

// ---- the launchers: the checks and the launches of an entry-point family, once.  cam_dist and out_dist are required exactly under
// a distortion, obs_w and a valid loss exactly with kLoss; what an entry point does not have it passes as null ----------------------
template <bool kLoss, int kDist>
int ba_launch_linearize_points(const double* cams, int n_cams, const double* cam_dist, const uint8_t* const_mask, const double* points,
                               int n_points, const int32_t* offsets, const int32_t* obs_cam, const double* obs_xy, int total, double lambda,
                               BaLoss loss, double* out_vinv, double* out_gp, double* out_cost, int32_t* out_count, uint8_t* out_obs_ok,
                               double* out_obs_lin, double* out_obs_w, double* out_total_cost, vc_stream_t stream) {
  constexpr bool kDistorted = kDist != kBaDistNone;
  if (n_points < 0 || n_cams < 0 || total < 0) return VC_ERR_INVALID_ARG;
  if (kLoss && !ba_loss_valid(loss)) return VC_ERR_INVALID_ARG;
  if (n_points == 0) return VC_OK;
  if (!points || !offsets || !out_vinv || !out_gp || !out_cost || !out_count || !out_total_cost) return VC_ERR_INVALID_ARG;
  if (n_cams > 0 && (!cams || (kDistorted && !cam_dist) || !const_mask)) return VC_ERR_INVALID_ARG;
  if (total > 0 && (!obs_cam || !obs_xy || !out_obs_ok || !out_obs_lin || (kLoss && !out_obs_w))) return VC_ERR_INVALID_ARG;
  if (!(lambda >= 0.0 && lambda < INFINITY)) return VC_ERR_INVALID_ARG;
  const BaProblem d{cams, const_mask, points, offsets, obs_cam, obs_xy, n_cams, n_points, total, cam_dist};
  hipLaunchKernelGGL((ba_linearize_points_kernel<kLoss, kDist>), dim3((unsigned)((n_points + kBaWave - 1) / kBaWave)), dim3(kBaWave), 0,
                     (hipStream_t)stream, d, lambda, loss, out_vinv, out_gp, out_cost, out_count, out_obs_ok, out_obs_lin, out_obs_w);
  hipLaunchKernelGGL(ba_ordered_sums_kernel, dim3(1), dim3(kBaWave), 0, (hipStream_t)stream, out_cost, n_points, out_total_cost);
  return vc::check_launch();
}

template <bool kLoss, int kDist>
int ba_launch_linearize_intrinsics(const double* cams, int n_cams, const double* cam_dist, const int32_t* cam_group, int n_groups,
                                   const uint8_t* intr_mask, const double* points, int n_points, const int32_t* offsets,
                                   const int32_t* obs_cam, int total, BaLoss loss, const double* vinv, const double* gp,
                                   const uint8_t* obs_ok, const double* obs_lin, const double* obs_w, double* out_obs_jt, double* out_T,
                                   double* out_terms, vc_stream_t stream) {
  constexpr bool kDistorted = kDist != kBaDistNone;
  if (n_cams < 0 || n_groups < 0 || n_points < 0 || total < 0) return VC_ERR_INVALID_ARG;
  if (kLoss && !ba_loss_valid(loss)) return VC_ERR_INVALID_ARG;
  if (n_points == 0 || n_groups == 0) return VC_OK;
  if (n_groups > ba_dist_max_groups(kDist)) return VC_ERR_UNSUPPORTED;
  if (!intr_mask || !points || !offsets || !vinv || !gp || !out_T || !out_terms) return VC_ERR_INVALID_ARG;
  if (n_cams > 0 && (!cams || (kDistorted && !cam_dist) || !cam_group)) return VC_ERR_INVALID_ARG;
  if (total > 0 && (!obs_cam || !obs_ok || !obs_lin || (kLoss && !obs_w) || !out_obs_jt)) return VC_ERR_INVALID_ARG;
  const BaProblem d{cams, nullptr, points, offsets, obs_cam, nullptr, n_cams, n_points, total, cam_dist};
  hipLaunchKernelGGL((ba_linearize_intrinsics_kernel<kLoss, kDist>), dim3((unsigned)((n_points + kBaWave - 1) / kBaWave)), dim3(kBaWave), 0,
                     (hipStream_t)stream, d, BaLinear{vinv, gp, obs_ok, obs_lin}, BaGroups{cam_group, intr_mask, n_groups}, obs_w, out_obs_jt,
                     out_T, out_terms);
  return vc::check_launch();
}

template <bool kLoss, int kDist>
int ba_launch_reduce_border(int n_cams, const int32_t* cam_group, int n_groups, const uint8_t* intr_mask, int n_points, const int32_t* offsets,
                            const int32_t* obs_cam, int total, const int32_t* cam_offsets, const int32_t* cam_obs, const int32_t* obs_point,
                            double lambda, BaLoss loss, const double* vinv, const uint8_t* obs_ok, const double* obs_lin, const double* obs_jt,
                            const double* obs_w, const double* T, const double* terms, double* out_sums, double* out_B, double* out_C,
                            double* out_h, uint8_t* out_free, vc_stream_t stream) {
  if (n_cams < 0 || n_groups < 0 || n_points < 0 || total < 0) return VC_ERR_INVALID_ARG;
  if (kLoss && !ba_loss_valid(loss)) return VC_ERR_INVALID_ARG;
  if (n_groups == 0) return VC_OK;
  if (n_groups > ba_dist_max_groups(kDist) || n_cams > VC_BA_MAX_CAMS) return VC_ERR_UNSUPPORTED;
  if (!intr_mask || !out_sums || !out_C || !out_h || !out_free) return VC_ERR_INVALID_ARG;
  if (n_cams > 0 && (!cam_group || !cam_offsets || !out_B)) return VC_ERR_INVALID_ARG;
  if (n_points > 0 && (!offsets || !vinv || !T || !terms)) return VC_ERR_INVALID_ARG;
  if (total > 0 && (!obs_cam || !cam_obs || !obs_point || !obs_ok || !obs_lin || !obs_jt || (kLoss && !obs_w))) return VC_ERR_INVALID_ARG;
  if (!(lambda >= 0.0 && lambda < INFINITY)) return VC_ERR_INVALID_ARG;
  constexpr int N = ba_dist_unknowns(kDist);
  const BaGroups gr{cam_group, intr_mask, n_groups};
  hipLaunchKernelGGL(ba_ordered_sums_kernel, dim3((unsigned)ba_term_rows<N>(n_groups)), dim3(kBaWave), 0, (hipStream_t)stream, terms, n_points,
                     out_sums);
  hipLaunchKernelGGL(ba_border_system_kernel<N>, dim3(1), dim3(kBaWave), 0, (hipStream_t)stream, out_sums, gr, lambda, out_C, out_h, out_free);
  if (n_cams > 0) {
    const BaProblem d{nullptr, nullptr, nullptr, offsets, obs_cam, nullptr, n_cams, n_points, total, nullptr};
    hipLaunchKernelGGL((ba_reduce_border_kernel<kLoss, kDist>), dim3((unsigned)n_cams), dim3(kBaWave), 0, (hipStream_t)stream, d,
                       BaLinear{vinv, nullptr, obs_ok, obs_lin}, gr, cam_offsets, cam_obs, obs_point, obs_jt, obs_w, T, out_B);
  }
  return vc::check_launch();
}

// The two kernels of a step.  grouped = false is vc_ba_step: then cam_group, T, dtheta and out_valid are absent and none is read.
template <int kDist>
int ba_launch_step(bool grouped, const double* cams, int n_cams, const double* cam_dist, const int32_t* cam_group, int n_groups,
                   const uint8_t* intr_mask, const double* points, int n_points, const int32_t* offsets, const int32_t* obs_cam, int total,
                   const double* vinv, const double* gp, const uint8_t* obs_ok, const double* obs_lin, const double* T, const double* dc,
                   const double* dtheta, double* out_cams, double* out_dist, double* out_points, double* out_dx, uint8_t* out_valid,
                   vc_stream_t stream) {
  constexpr bool kDistorted = kDist != kBaDistNone;
  if (n_cams < 0 || n_groups < 0 || n_points < 0 || total < 0) return VC_ERR_INVALID_ARG;
  if (n_cams == 0 && n_points == 0) return VC_OK;
  if (n_groups > ba_dist_max_groups(kDist)) return VC_ERR_UNSUPPORTED;
  if (n_groups > 0 && (!intr_mask || !dtheta)) return VC_ERR_INVALID_ARG;
  if (n_cams > 0 && (!cams || (kDistorted && (!cam_dist || !out_dist)) || (grouped && (!cam_group || !out_valid)) || !dc || !out_cams))
    return VC_ERR_INVALID_ARG;
  if (n_points > 0 && (!points || !offsets || !vinv || !gp || !out_points || !out_dx || (n_groups > 0 && !T))) return VC_ERR_INVALID_ARG;
  if (n_points > 0 && total > 0 && (!obs_cam || !obs_ok || !obs_lin)) return VC_ERR_INVALID_ARG;
  const BaProblem d{cams, nullptr, points, offsets, obs_cam, nullptr, n_cams, n_points, total, cam_dist};
  const BaGroups gr{cam_group, intr_mask, n_groups};
  if (n_points > 0)
    hipLaunchKernelGGL(ba_step_points_kernel<ba_dist_unknowns(kDist)>, dim3((unsigned)((n_points + kBaWave - 1) / kBaWave)), dim3(kBaWave), 0,
                       (hipStream_t)stream, d, BaLinear{vinv, gp, obs_ok, obs_lin}, T, n_groups, dc, dtheta, out_points, out_dx);
  if (n_cams > 0)
    hipLaunchKernelGGL(ba_step_cameras_kernel<kDist>, dim3((unsigned)((n_cams + kBaWave - 1) / kBaWave)), dim3(kBaWave), 0, (hipStream_t)stream,
                       d, gr, dc, dtheta, out_cams, out_dist, out_valid);
  return vc::check_launch();
}

constexpr int ba_reduce_lds_bytes(int n_cams) { return 36 * n_cams * (int)sizeof(double); }
static_assert(ba_reduce_lds_bytes(VC_BA_MAX_CAMS) + (int)sizeof(BaBatch) <= 160 * 1024, "the row block of VC_BA_MAX_CAMS cameras must fit the CU's LDS");

}  // namespace

extern "C" {

int vc_ba_linearize_points(const double* cams, int n_cams, const uint8_t* const_mask, const double* points, int n_points,
                           const int32_t* offsets, const int32_t* obs_cam, const double* obs_xy, int total, double lambda,
                           double* out_vinv, double* out_gp, double* out_cost, int32_t* out_count, uint8_t* out_obs_ok,
                           double* out_obs_lin, double* out_total_cost, vc_stream_t stream) {
  return ba_launch_linearize_points<false, kBaDistNone>(cams, n_cams, nullptr, const_mask, points, n_points, offsets, obs_cam, obs_xy, total, lambda,
                                                        kBaNoLoss, out_vinv, out_gp, out_cost, out_count, out_obs_ok, out_obs_lin, nullptr,
                                                        out_total_cost, stream);
}

int vc_ba_linearize_points_loss(const double* cams, int n_cams, const uint8_t* const_mask, const double* points, int n_points,
                                const int32_t* offsets, const int32_t* obs_cam, const double* obs_xy, int total, double lambda, int loss,
                                double loss_scale, double* out_vinv, double* out_gp, double* out_cost, int32_t* out_count,
                                uint8_t* out_obs_ok, double* out_obs_lin, double* out_obs_w, double* out_total_cost, vc_stream_t stream) {
  return ba_launch_linearize_points<true, kBaDistNone>(cams, n_cams, nullptr, const_mask, points, n_points, offsets, obs_cam, obs_xy, total, lambda,
                                                       BaLoss{loss, loss_scale}, out_vinv, out_gp, out_cost, out_count, out_obs_ok, out_obs_lin,
                                                       out_obs_w, out_total_cost, stream);
}

int vc_ba_reduce_cameras(int n_cams, const uint8_t* const_mask, int n_points, const int32_t* offsets, const int32_t* obs_cam, int total,
                         const int32_t* cam_offsets, const int32_t* cam_obs, const int32_t* obs_point, double lambda,
                         const double* vinv, const double* gp, const uint8_t* obs_ok, const double* obs_lin, double* out_S,
                         double* out_g, vc_stream_t stream) {
  if (n_cams < 0 || n_points < 0 || total < 0) return VC_ERR_INVALID_ARG;
  if (n_cams == 0) return VC_OK;
  if (n_cams > VC_BA_MAX_CAMS) return VC_ERR_UNSUPPORTED;
  if (!const_mask || !cam_offsets || !out_S || !out_g) return VC_ERR_INVALID_ARG;
  if (n_points > 0 && (!offsets || !vinv || !gp)) return VC_ERR_INVALID_ARG;
  if (total > 0 && (!obs_cam || !cam_obs || !obs_point || !obs_ok || !obs_lin)) return VC_ERR_INVALID_ARG;
  if (!(lambda >= 0.0 && lambda < INFINITY)) return VC_ERR_INVALID_ARG;
  static vc::PerDeviceOnce configured;
  if (int st = vc::allow_dynamic_lds(configured, ba_reduce_lds_bytes(VC_BA_MAX_CAMS), ba_reduce_cameras_kernel)) return st;
  const BaProblem d{nullptr, const_mask, nullptr, offsets, obs_cam, nullptr, n_cams, n_points, total};
  hipLaunchKernelGGL(ba_reduce_cameras_kernel, dim3((unsigned)n_cams), dim3(kBaWave), (size_t)ba_reduce_lds_bytes(n_cams),
                     (hipStream_t)stream, d, BaLinear{vinv, gp, obs_ok, obs_lin}, cam_offsets, cam_obs, obs_point, lambda, out_S, out_g);
  return vc::check_launch();
}

int vc_ba_camera_blocks(int n_cams, const uint8_t* const_mask, int n_points, const int32_t* offsets, const int32_t* obs_cam, int total,
                        const int32_t* cam_offsets, const int32_t* cam_obs, const int32_t* obs_point, double lambda, const double* vinv,
                        const double* gp, const uint8_t* obs_ok, const double* obs_lin, double* out_U, double* out_D, double* out_Minv,
                        double* out_g, uint8_t* out_fixed, vc_stream_t stream) {
  if (n_cams < 0 || n_points < 0 || total < 0) return VC_ERR_INVALID_ARG;
  if (n_cams == 0) return VC_OK;
  if (!const_mask || !cam_offsets || !out_U || !out_D || !out_Minv || !out_g || !out_fixed) return VC_ERR_INVALID_ARG;
  if (n_points > 0 && (!offsets || !vinv || !gp)) return VC_ERR_INVALID_ARG;
  if (total > 0 && (!obs_cam || !cam_obs || !obs_point || !obs_ok || !obs_lin)) return VC_ERR_INVALID_ARG;
  if (!(lambda >= 0.0 && lambda < INFINITY)) return VC_ERR_INVALID_ARG;
  const BaProblem d{nullptr, const_mask, nullptr, offsets, obs_cam, nullptr, n_cams, n_points, total};
  hipLaunchKernelGGL(ba_camera_blocks_kernel, dim3((unsigned)n_cams), dim3(kBaWave), 0, (hipStream_t)stream, d,
                     BaLinear{vinv, gp, obs_ok, obs_lin}, cam_offsets, cam_obs, obs_point, lambda, out_U, out_D, out_Minv, out_g, out_fixed);
  return vc::check_launch();
}

int vc_ba_schur_product(int n_cams, int n_points, const int32_t* offsets, const int32_t* obs_cam, int total, const int32_t* cam_offsets,
                        const int32_t* cam_obs, const int32_t* obs_point, const double* vinv, const uint8_t* obs_ok, const double* obs_lin,
                        const double* U, const uint8_t* fixed, const double* p, double* workspace_s, double* out_q, vc_stream_t stream) {
  if (n_cams < 0 || n_points < 0 || total < 0) return VC_ERR_INVALID_ARG;
  if (n_cams == 0) return VC_OK;
  if (!cam_offsets || !U || !fixed || !p || !out_q) return VC_ERR_INVALID_ARG;
  if (n_points > 0 && (!offsets || !vinv || !workspace_s)) return VC_ERR_INVALID_ARG;
  if (total > 0 && (!obs_cam || !cam_obs || !obs_point || !obs_ok || !obs_lin)) return VC_ERR_INVALID_ARG;
  const BaProblem d{nullptr, nullptr, nullptr, offsets, obs_cam, nullptr, n_cams, n_points, total};
  const BaLinear l{vinv, nullptr, obs_ok, obs_lin};
  if (n_points > 0)
    hipLaunchKernelGGL(ba_product_points_kernel, dim3((unsigned)((n_points + kBaWave - 1) / kBaWave)), dim3(kBaWave), 0, (hipStream_t)stream,
                       d, l, fixed, p, workspace_s);
  hipLaunchKernelGGL(ba_product_cameras_kernel, dim3((unsigned)n_cams), dim3(kBaProductThreads), 0, (hipStream_t)stream, d, l, cam_offsets,
                     cam_obs, obs_point, U, fixed, p, workspace_s, out_q);
  return vc::check_launch();
}

int vc_ba_step(const double* cams, int n_cams, const double* points, int n_points, const int32_t* offsets, const int32_t* obs_cam,
               int total, const double* vinv, const double* gp, const uint8_t* obs_ok, const double* obs_lin, const double* dc,
               double* out_cams, double* out_points, double* out_dx, vc_stream_t stream) {
  return ba_launch_step<kBaDistNone>(false, cams, n_cams, nullptr, nullptr, 0, nullptr, points, n_points, offsets, obs_cam, total, vinv, gp, obs_ok,
                                     obs_lin, nullptr, dc, nullptr, out_cams, nullptr, out_points, out_dx, nullptr, stream);
}

int vc_ba_linearize_intrinsics(const double* cams, int n_cams, const int32_t* cam_group, int n_groups, const uint8_t* intr_mask,
                               const double* points, int n_points, const int32_t* offsets, const int32_t* obs_cam, int total,
                               const double* vinv, const double* gp, const uint8_t* obs_ok, const double* obs_lin, double* out_obs_xn,
                               double* out_T, double* out_terms, vc_stream_t stream) {
  return ba_launch_linearize_intrinsics<false, kBaDistNone>(cams, n_cams, nullptr, cam_group, n_groups, intr_mask, points, n_points, offsets, obs_cam,
                                                            total, kBaNoLoss, vinv, gp, obs_ok, obs_lin, nullptr, out_obs_xn, out_T, out_terms, stream);
}

int vc_ba_linearize_intrinsics_loss(const double* cams, int n_cams, const int32_t* cam_group, int n_groups, const uint8_t* intr_mask,
                                    const double* points, int n_points, const int32_t* offsets, const int32_t* obs_cam, int total,
                                    const double* vinv, const double* gp, const uint8_t* obs_ok, const double* obs_lin, const double* obs_w,
                                    double* out_obs_xn, double* out_T, double* out_terms, vc_stream_t stream) {
  return ba_launch_linearize_intrinsics<true, kBaDistNone>(cams, n_cams, nullptr, cam_group, n_groups, intr_mask, points, n_points, offsets, obs_cam,
                                                           total, kBaNoLoss, vinv, gp, obs_ok, obs_lin, obs_w, out_obs_xn, out_T, out_terms, stream);
}

int vc_ba_reduce_border(int n_cams, const int32_t* cam_group, int n_groups, const uint8_t* intr_mask, int n_points, const int32_t* offsets,
                        const int32_t* obs_cam, int total, const int32_t* cam_offsets, const int32_t* cam_obs, const int32_t* obs_point,
                        double lambda, const double* vinv, const uint8_t* obs_ok, const double* obs_lin, const double* obs_xn,
                        const double* T, const double* terms, double* out_sums, double* out_B, double* out_C, double* out_h,
                        uint8_t* out_free, vc_stream_t stream) {
  return ba_launch_reduce_border<false, kBaDistNone>(n_cams, cam_group, n_groups, intr_mask, n_points, offsets, obs_cam, total, cam_offsets, cam_obs,
                                                     obs_point, lambda, kBaNoLoss, vinv, obs_ok, obs_lin, obs_xn, nullptr, T, terms, out_sums, out_B,
                                                     out_C, out_h, out_free, stream);
}

int vc_ba_reduce_border_loss(int n_cams, const int32_t* cam_group, int n_groups, const uint8_t* intr_mask, int n_points, const int32_t* offsets,
                             const int32_t* obs_cam, int total, const int32_t* cam_offsets, const int32_t* cam_obs, const int32_t* obs_point,
                             double lambda, const double* vinv, const uint8_t* obs_ok, const double* obs_lin, const double* obs_xn,
                             const double* obs_w, const double* T, const double* terms, double* out_sums, double* out_B, double* out_C,
                             double* out_h, uint8_t* out_free, vc_stream_t stream) {
  return ba_launch_reduce_border<true, kBaDistNone>(n_cams, cam_group, n_groups, intr_mask, n_points, offsets, obs_cam, total, cam_offsets, cam_obs,
                                                    obs_point, lambda, kBaNoLoss, vinv, obs_ok, obs_lin, obs_xn, obs_w, T, terms, out_sums, out_B,
                                                    out_C, out_h, out_free, stream);
}

int vc_ba_step_intrinsics(const double* cams, int n_cams, const int32_t* cam_group, int n_groups, const uint8_t* intr_mask,
                          const double* points, int n_points, const int32_t* offsets, const int32_t* obs_cam, int total, const double* vinv,
                          const double* gp, const uint8_t* obs_ok, const double* obs_lin, const double* T, const double* dc,
                          const double* dtheta, double* out_cams, double* out_points, double* out_dx, uint8_t* out_valid,
                          vc_stream_t stream) {
  return ba_launch_step<kBaDistNone>(true, cams, n_cams, nullptr, cam_group, n_groups, intr_mask, points, n_points, offsets, obs_cam, total, vinv, gp,
                                     obs_ok, obs_lin, T, dc, dtheta, out_cams, nullptr, out_points, out_dx, out_valid, stream);
}

// ---- the distortion: the _radial and the _opencv entry points -----------------------------------------------------------------------
int vc_ba_linearize_points_radial(const double* cams, int n_cams, const double* cam_dist, const uint8_t* const_mask, const double* points,
                                  int n_points, const int32_t* offsets, const int32_t* obs_cam, const double* obs_xy, int total, double lambda,
                                  int loss, double loss_scale, double* out_vinv, double* out_gp, double* out_cost, int32_t* out_count,
                                  uint8_t* out_obs_ok, double* out_obs_lin, double* out_obs_w, double* out_total_cost, vc_stream_t stream) {
  return ba_launch_linearize_points<true, kBaDistRadial>(cams, n_cams, cam_dist, const_mask, points, n_points, offsets, obs_cam, obs_xy, total,
                                                         lambda, BaLoss{loss, loss_scale}, out_vinv, out_gp, out_cost, out_count, out_obs_ok,
                                                         out_obs_lin, out_obs_w, out_total_cost, stream);
}

int vc_ba_linearize_intrinsics_radial(const double* cams, int n_cams, const double* cam_dist, const int32_t* cam_group, int n_groups,
                                      const uint8_t* intr_mask, const double* points, int n_points, const int32_t* offsets,
                                      const int32_t* obs_cam, int total, int loss, double loss_scale, const double* vinv, const double* gp,
                                      const uint8_t* obs_ok, const double* obs_lin, const double* obs_w, double* out_obs_jt, double* out_T,
                                      double* out_terms, vc_stream_t stream) {
  return ba_launch_linearize_intrinsics<true, kBaDistRadial>(cams, n_cams, cam_dist, cam_group, n_groups, intr_mask, points, n_points, offsets,
                                                             obs_cam, total, BaLoss{loss, loss_scale}, vinv, gp, obs_ok, obs_lin, obs_w, out_obs_jt,
                                                             out_T, out_terms, stream);
}

int vc_ba_reduce_border_radial(int n_cams, const int32_t* cam_group, int n_groups, const uint8_t* intr_mask, int n_points,
                               const int32_t* offsets, const int32_t* obs_cam, int total, const int32_t* cam_offsets, const int32_t* cam_obs,
                               const int32_t* obs_point, double lambda, int loss, double loss_scale, const double* vinv, const uint8_t* obs_ok,
                               const double* obs_lin, const double* obs_jt, const double* obs_w, const double* T, const double* terms,
                               double* out_sums, double* out_B, double* out_C, double* out_h, uint8_t* out_free, vc_stream_t stream) {
  return ba_launch_reduce_border<true, kBaDistRadial>(n_cams, cam_group, n_groups, intr_mask, n_points, offsets, obs_cam, total, cam_offsets, cam_obs,
                                                      obs_point, lambda, BaLoss{loss, loss_scale}, vinv, obs_ok, obs_lin, obs_jt, obs_w, T, terms,
                                                      out_sums, out_B, out_C, out_h, out_free, stream);
}

int vc_ba_step_radial(const double* cams, int n_cams, const double* cam_dist, const int32_t* cam_group, int n_groups, const uint8_t* intr_mask,
                      const double* points, int n_points, const int32_t* offsets, const int32_t* obs_cam, int total, const double* vinv,
                      const double* gp, const uint8_t* obs_ok, const double* obs_lin, const double* T, const double* dc, const double* dtheta,
                      double* out_cams, double* out_dist, double* out_points, double* out_dx, uint8_t* out_valid, vc_stream_t stream) {
  return ba_launch_step<kBaDistRadial>(true, cams, n_cams, cam_dist, cam_group, n_groups, intr_mask, points, n_points, offsets, obs_cam, total, vinv,
                                       gp, obs_ok, obs_lin, T, dc, dtheta, out_cams, out_dist, out_points, out_dx, out_valid, stream);
}

int vc_ba_linearize_points_opencv(const double* cams, int n_cams, const double* cam_dist, const uint8_t* const_mask, const double* points,
                                  int n_points, const int32_t* offsets, const int32_t* obs_cam, const double* obs_xy, int total, double lambda,
                                  int loss, double loss_scale, double* out_vinv, double* out_gp, double* out_cost, int32_t* out_count,
                                  uint8_t* out_obs_ok, double* out_obs_lin, double* out_obs_w, double* out_total_cost, vc_stream_t stream) {
  return ba_launch_linearize_points<true, kBaDistOpencv>(cams, n_cams, cam_dist, const_mask, points, n_points, offsets, obs_cam, obs_xy, total,
                                                         lambda, BaLoss{loss, loss_scale}, out_vinv, out_gp, out_cost, out_count, out_obs_ok,
                                                         out_obs_lin, out_obs_w, out_total_cost, stream);
}

int vc_ba_linearize_intrinsics_opencv(const double* cams, int n_cams, const double* cam_dist, const int32_t* cam_group, int n_groups,
                                      const uint8_t* intr_mask, const double* points, int n_points, const int32_t* offsets,
                                      const int32_t* obs_cam, int total, int loss, double loss_scale, const double* vinv, const double* gp,
                                      const uint8_t* obs_ok, const double* obs_lin, const double* obs_w, double* out_obs_jt, double* out_T,
                                      double* out_terms, vc_stream_t stream) {
  return ba_launch_linearize_intrinsics<true, kBaDistOpencv>(cams, n_cams, cam_dist, cam_group, n_groups, intr_mask, points, n_points, offsets,
                                                             obs_cam, total, BaLoss{loss, loss_scale}, vinv, gp, obs_ok, obs_lin, obs_w, out_obs_jt,
                                                             out_T, out_terms, stream);
}

int vc_ba_reduce_border_opencv(int n_cams, const int32_t* cam_group, int n_groups, const uint8_t* intr_mask, int n_points,
                               const int32_t* offsets, const int32_t* obs_cam, int total, const int32_t* cam_offsets, const int32_t* cam_obs,
                               const int32_t* obs_point, double lambda, int loss, double loss_scale, const double* vinv, const uint8_t* obs_ok,
                               const double* obs_lin, const double* obs_jt, const double* obs_w, const double* T, const double* terms,
                               double* out_sums, double* out_B, double* out_C, double* out_h, uint8_t* out_free, vc_stream_t stream) {
  return ba_launch_reduce_border<true, kBaDistOpencv>(n_cams, cam_group, n_groups, intr_mask, n_points, offsets, obs_cam, total, cam_offsets, cam_obs,
                                                      obs_point, lambda, BaLoss{loss, loss_scale}, vinv, obs_ok, obs_lin, obs_jt, obs_w, T, terms,
                                                      out_sums, out_B, out_C, out_h, out_free, stream);
}

int vc_ba_step_opencv(const double* cams, int n_cams, const double* cam_dist, const int32_t* cam_group, int n_groups, const uint8_t* intr_mask,
                      const double* points, int n_points, const int32_t* offsets, const int32_t* obs_cam, int total, const double* vinv,
                      const double* gp, const uint8_t* obs_ok, const double* obs_lin, const double* T, const double* dc, const double* dtheta,
                      double* out_cams, double* out_dist, double* out_points, double* out_dx, uint8_t* out_valid, vc_stream_t stream) {
  return ba_launch_step<kBaDistOpencv>(true, cams, n_cams, cam_dist, cam_group, n_groups, intr_mask, points, n_points, offsets, obs_cam, total, vinv,
                                       gp, obs_ok, obs_lin, T, dc, dtheta, out_cams, out_dist, out_points, out_dx, out_valid, stream);
}

}  // extern "C"
