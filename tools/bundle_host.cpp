// The kernels of vit_colmap_amd/csrc/bundle.hip on the CPU, the plain adjustment and the border of the intrinsics: its per-point
// and per-entry routines are __host__ __device__, so this program includes the kernel source and calls them point after point,
// row after row and, for the two camera passes, lane after lane between the places where the kernel has its barriers.  It is how
// the kernels' arithmetic is compared with the specification without a GPU (tests/test_bundle_spec.py,
// tests/test_bundle_intr_spec.py; HOST_SPEC_REL of tests/util_bundle.py and tests/util_bundle_intr.py was measured with it), what
// the GPU tests expect the kernels' bytes to equal, how the routines are run under a host sanitizer and where a fault in them is
// looked for with a host debugger.  tools/triangulate_host.cpp is its counterpart for csrc/triangulate.hip.
//
//   hipcc -x hip --offload-arch=gfx950 -O2 -std=c++17 -ffp-contract=off -o bundle_host tools/bundle_host.cpp
//   ./bundle_host problem.bin result.bin
// problem.bin: int32 n_cams, n_points, total, n_groups (>= 0); float64 lambda; int32 offsets (n_points + 1), obs_cam (total),
// cam_offsets (n_cams + 1), cam_obs (total), obs_point (total), const_mask (n_cams), cam_group (n_cams; none without groups),
// intr_mask (n_groups); float64 cams (n_cams, 16), points (n_points, 3), obs_xy (total, 2), dc (n_cams, 6), dtheta (n_groups, 4):
// the steps are taken with the caller's dc and dtheta, no system is solved here.
// result.bin, the plain section: float64 vinv (n_points, 6), gp (n_points, 3), cost (n_points), total_cost (1), S (6 n_cams,
// 6 n_cams), g (6 n_cams), out_cams (n_cams, 16), out_points (n_points, 3), dx (n_points, 3) (the step under dc alone), obs_lin
// (total, 32); int32 count (n_points); uint8 obs_ok (total).  With n_groups = G >= 1 the border's section follows: float64 obs_xn
// (total, 2), T (n_points, G, 12), terms (24 G + 16 G^2, n_points), sums (24 G + 16 G^2), B (6 n_cams, 4 G), C (4 G, 4 G), h (4 G),
// out_cams, out_points, dx (the step under dc and dtheta); uint8 free (4 G), valid (n_cams).
// Offsets of any kind are passed on as they are: the routines check them.
// A loss ("The loss" in DESIGN.md §4.2k) is an optional extension: where problem.bin goes on after dtheta with int32 loss, float64
// loss_scale, every routine that has a loss variant runs it (vc_ba_linearize_points_loss, vc_ba_linearize_intrinsics_loss,
// vc_ba_reduce_border_loss) and result.bin ends with one more array, float64 obs_w (total).  A loss that the entry point refuses
// (ba_loss_valid) is refused here: one line on stderr, exit status 3, no result.  Without the extension nothing changes.
// The distortion ("The distortion" in §4.2k) is a further extension: where problem.bin goes on after loss_scale with int32 1,
// float64 cam_dist (n_cams, 2), dtheta (n_groups, 6), the routines of the _radial entry points run (the file's dtheta (n_groups, 4)
// is then not used; VC_BA_LOSS_TRIVIAL, 1.0 is the plain case) and result.bin has the layout above with six unknowns per group:
// the plain section as it is (its step under dc alone), then with G >= 1 float64 obs_jt (total, 6), T (n_points, G, 18), terms
// (48 G + 36 G^2, n_points), sums (48 G + 36 G^2), B (6 n_cams, 6 G), C (6 G, 6 G), h (6 G), out_cams, out_points, dx, out_dist
// (n_cams, 2); uint8 free (6 G), valid (n_cams); then obs_w.  More than VC_BA_MAX_GROUPS_RADIAL groups: exit status 3.
// The tangential terms ("The tangential terms" in §4.2k) are the same extension under the marker int32 2: float64 cam_dist
// (n_cams, 4), dtheta (n_groups, 8), the routines of the _opencv entry points, and the radial layout with eight unknowns per group:
// obs_jt (total, 10), T (n_points, G, 24), terms and sums (80 G + 64 G^2), B (6 n_cams, 8 G), C (8 G, 8 G), h (8 G), out_dist
// (n_cams, 4), free (8 G).  More than VC_BA_MAX_GROUPS_OPENCV groups: exit status 3.  Files without the marker 2 are read as before.
#include "../vit_colmap_amd/csrc/bundle.hip"
#include "host_io.h"

// The camera pass of one wave (ba_camera_walk) lane after lane: every batch of camera a's list is prepared by all lanes, then
// visit(lane, o, j, lo, hi, y) is called for every lane in turn over the batch's usable observations in order.
template <typename Visit>
static void camera_walk(const BaProblem& d, const BaLinear& l, const int32_t* cam_offsets, const int32_t* cam_obs, const int32_t* obs_point,
                        int a, Visit visit) {
  BaBatch batch;
  int first, last;
  if (!ba_camera_list(cam_offsets, a, d.total, first, last)) return;
  for (int base = first; base < last; base += kBaWave) {
    for (int lane = 0; lane < kBaWave; ++lane) ba_prepare(d, l, cam_obs, obs_point, a, base + lane, last, lane, batch);
    const int m = last - base < kBaWave ? last - base : kBaWave;
    for (int lane = 0; lane < kBaWave; ++lane)
      for (int k = 0; k < m; ++k)
        if (batch.o[k] >= 0) visit(lane, batch.o[k], batch.j[k], batch.lo[k], batch.hi[k], batch.y[k]);
  }
}

// The two step kernels -> out_cams, out_points, dx, valid.
struct Step {
  std::vector<double> cams, points, dx;
  std::vector<uint8_t> valid;
};

static Step take_step(const BaProblem& d, const BaLinear& l, const BaGroups& gr, const double* T, const double* dc, const double* dtheta) {
  Step s{std::vector<double>(16 * (size_t)d.n_cams), std::vector<double>(3 * (size_t)d.n_points), std::vector<double>(3 * (size_t)d.n_points),
         std::vector<uint8_t>(d.n_cams)};
  for (int j = 0; j < d.n_points; ++j) {
    double dX[3];
    ba_point_step(d, l, T, gr.n_groups, dc, dtheta, j, dX);
    for (int k = 0; k < 3; ++k) s.dx[3 * (size_t)j + k] = dX[k], s.points[3 * (size_t)j + k] = d.points[3 * (size_t)j + k] + dX[k];
  }
  for (int a = 0; a < d.n_cams; ++a)
    s.valid[a] = ba_camera_step(d.cams + 16 * (size_t)a, dc + 6 * (size_t)a, gr, a, dtheta, s.cams.data() + 16 * (size_t)a) ? 1 : 0;
  return s;
}

// The distortion's extensions: every routine under kDist and the loss (the kernels of the _radial and the _opencv entry points),
// six or eight unknowns per group.
template <int kDist>
static int run_dist(const char* path, const BaProblem& d, const BaGroups& gr, const BaLoss& loss, double lambda, const int32_t* cam_offsets,
                      const int32_t* cam_obs, const int32_t* obs_point, const double* cam_dist, const double* dc, const double* dtheta) {
  constexpr int N = ba_dist_unknowns(kDist), kParams = ba_dist_params(kDist);
  const int n_cams = d.n_cams, n_points = d.n_points, total = d.total, G = gr.n_groups;
  std::vector<double> vinv(6 * (size_t)n_points), gp(3 * (size_t)n_points), cost(n_points), total_cost(1, 0.0);
  std::vector<double> obs_lin((size_t)kBaLin * total), obs_w(total);
  std::vector<int32_t> count(n_points);
  std::vector<uint8_t> obs_ok(total);
  for (int j = 0; j < n_points; ++j) {
    double v[6], g[3];
    count[j] = ba_linearize_point<true, kDist>(d, loss, j, lambda, v, g, cost[j], obs_ok.data(), obs_lin.data(), obs_w.data(), cam_dist);
    for (int k = 0; k < 6; ++k) vinv[6 * (size_t)j + k] = v[k];
    for (int k = 0; k < 3; ++k) gp[3 * (size_t)j + k] = g[k];
    total_cost[0] += cost[j];
  }
  const BaLinear l{vinv.data(), gp.data(), obs_ok.data(), obs_lin.data()};
  std::vector<double> S(36 * (size_t)n_cams * n_cams), g(6 * (size_t)n_cams), acc(36 * (size_t)n_cams);
  for (int a = 0; a < n_cams; ++a) {
    BaLane lanes[kBaWave];
    for (int lane = 0; lane < kBaWave; ++lane) lanes[lane] = BaLane{0.0, 0.0, 0.0};
    for (double& v : acc) v = 0.0;
    camera_walk(d, l, cam_offsets, cam_obs, obs_point, a, [&](int lane, int o, int j, int lo, int hi, const double* y) {
      ba_lane_update(d, l, a, o, j, lo, hi, lane, y, acc.data(), lanes[lane]);
    });
    for (int lane = 0; lane < kBaWave; ++lane) ba_lane_finish(n_cams, d.const_mask[a], lambda, a, lane, acc.data(), lanes[lane], S.data(), g.data());
  }
  auto take = [&](const BaGroups& groups, const double* T, const double* dth, Step& s, std::vector<double>& dist) {
    s = Step{std::vector<double>(16 * (size_t)n_cams), std::vector<double>(3 * (size_t)n_points), std::vector<double>(3 * (size_t)n_points),
             std::vector<uint8_t>(n_cams)};
    dist.assign(kParams * (size_t)n_cams, 0.0);
    for (int j = 0; j < n_points; ++j) {
      double dX[3];
      ba_point_step<N>(d, l, T, groups.n_groups, dc, dth, j, dX);
      for (int k = 0; k < 3; ++k) s.dx[3 * (size_t)j + k] = dX[k], s.points[3 * (size_t)j + k] = d.points[3 * (size_t)j + k] + dX[k];
    }
    for (int a = 0; a < n_cams; ++a) {
      if constexpr (kDist == kBaDistOpencv)
        s.valid[a] = ba_camera_step_opencv(d.cams + 16 * (size_t)a, cam_dist + 4 * (size_t)a, dc + 6 * (size_t)a, groups, a, dth,
                                           s.cams.data() + 16 * (size_t)a, dist.data() + 4 * (size_t)a) ? 1 : 0;
      else
        s.valid[a] = ba_camera_step_radial(d.cams + 16 * (size_t)a, cam_dist + 2 * (size_t)a, dc + 6 * (size_t)a, groups, a, dth,
                                           s.cams.data() + 16 * (size_t)a, dist.data() + 2 * (size_t)a) ? 1 : 0;
    }
  };
  Step plain, step;
  std::vector<double> plain_dist, out_dist;
  take(BaGroups{nullptr, nullptr, 0}, nullptr, nullptr, plain, plain_dist);

  std::FILE* out = open_output(path);
  if (!out) return 2;
  write_all(out, vinv), write_all(out, gp), write_all(out, cost), write_all(out, total_cost), write_all(out, S), write_all(out, g);
  write_all(out, plain.cams), write_all(out, plain.points), write_all(out, plain.dx), write_all(out, obs_lin), write_all(out, count);
  write_all(out, obs_ok);
  if (G >= 1) {
    const int rows = ba_term_rows<N>(G), m = N * G;
    std::vector<double> obs_jt((size_t)ba_dist_jt(kDist) * total), T((size_t)n_points * G * 3 * N), terms((size_t)rows * n_points), sums(rows);
    for (int j = 0; j < n_points; ++j)
      ba_linearize_point_intrinsics<true, kDist>(d, l, gr, obs_w.data(), j, obs_jt.data(), T.data(), terms.data(), cam_dist);
    for (int r = 0; r < rows; ++r) {
      double sum = 0.0;
      for (int j = 0; j < n_points; ++j) sum += terms[(size_t)r * n_points + j];
      sums[r] = sum;
    }
    std::vector<double> B(6 * (size_t)n_cams * m), C((size_t)m * m), h(m);
    std::vector<uint8_t> free_(m);
    for (int idx = 0; idx < m * m; ++idx) C[idx] = ba_border_c<N>(sums.data(), gr, lambda, idx / m, idx % m);
    for (int row = 0; row < m; ++row)
      h[row] = ba_border_h<N>(sums.data(), gr, row), free_[row] = ba_theta_free<N>(sums.data(), gr, row / N, row % N) ? 1 : 0;
    for (int a = 0; a < n_cams; ++a) {
      BaBorderLane lanes[kBaWave];
      for (int lane = 0; lane < kBaWave; ++lane)
        for (int k = 0; k < kBaBorderSlots; ++k) lanes[lane].jt[k] = lanes[lane].yt[k] = 0.0;
      const int ga = ba_group_of(gr, a);
      camera_walk(d, l, cam_offsets, cam_obs, obs_point, a, [&](int lane, int o, int j, int, int, const double* y) {
        ba_border_update<true, kDist>(l, gr, obs_jt.data(), obs_w.data(), T.data(), ga, o, j, lane, y, lanes[lane]);
      });
      for (int lane = 0; lane < kBaWave; ++lane) ba_border_finish<N>(G, a, lane, lanes[lane], B.data());
    }
    take(gr, T.data(), dtheta, step, out_dist);
    write_all(out, obs_jt), write_all(out, T), write_all(out, terms), write_all(out, sums), write_all(out, B), write_all(out, C);
    write_all(out, h), write_all(out, step.cams), write_all(out, step.points), write_all(out, step.dx), write_all(out, out_dist);
    write_all(out, free_), write_all(out, step.valid);
  }
  write_all(out, obs_w);
  std::fclose(out);
  std::printf("%d cameras, %d points, %d observations, %d groups, %s, cost %.17g\n", n_cams, n_points, total, G,
              kDist == kBaDistOpencv ? "opencv" : "radial", total_cost[0]);
  return 0;
}

int main(int argc, char** argv) {
  std::FILE* in = open_input(argc, argv, "problem.bin result.bin");
  if (!in) return 2;
  int32_t head[4];
  double lambda;
  if (std::fread(head, sizeof(int32_t), 4, in) != 4 || std::fread(&lambda, sizeof(double), 1, in) != 1 || head[0] < 0 || head[1] < 0 ||
      head[2] < 0 || head[3] < 0 || head[0] > VC_BA_MAX_CAMS || head[3] > VC_BA_MAX_GROUPS) {
    std::fprintf(stderr, "%s: no header\n", argv[1]);
    return 2;
  }
  const int n_cams = head[0], n_points = head[1], total = head[2], G = head[3];
  std::vector<int32_t> offsets(n_points + 1), obs_cam(total), cam_offsets(n_cams + 1), cam_obs(total), obs_point(total), mask32(n_cams);
  std::vector<int32_t> cam_group(G > 0 ? n_cams : 0), intr32(G);
  std::vector<double> cams(16 * (size_t)n_cams), points(3 * (size_t)n_points), obs_xy(2 * (size_t)total), dc(6 * (size_t)n_cams);
  std::vector<double> dtheta(4 * (size_t)G);
  const bool ok = read_all(in, offsets) && read_all(in, obs_cam) && read_all(in, cam_offsets) && read_all(in, cam_obs) &&
                  read_all(in, obs_point) && read_all(in, mask32) && read_all(in, cam_group) && read_all(in, intr32) && read_all(in, cams) &&
                  read_all(in, points) && read_all(in, obs_xy) && read_all(in, dc) && read_all(in, dtheta);
  // the optional loss: nothing after dtheta, or both of its numbers
  int32_t loss_kind = 0;
  BaLoss loss{VC_BA_LOSS_TRIVIAL, 1.0};
  const bool with_loss = ok && std::fread(&loss_kind, sizeof(int32_t), 1, in) == 1;
  const bool loss_read = !with_loss || std::fread(&loss.scale, sizeof(double), 1, in) == 1;
  loss.kind = loss_kind;
  // the optional distortion after the loss: nothing, or the marker (1: radial, 2: with the tangential terms) and both of its arrays
  int32_t dist_mark = 0;
  const bool with_dist = with_loss && loss_read && std::fread(&dist_mark, sizeof(int32_t), 1, in) == 1;
  const bool opencv = with_dist && dist_mark == 2;
  std::vector<double> cam_dist(with_dist ? (opencv ? 4 : 2) * (size_t)n_cams : 0), dist_dtheta(with_dist ? (opencv ? 8 : 6) * (size_t)G : 0);
  const bool dist_read = !with_dist || ((dist_mark == 1 || opencv) && read_all(in, cam_dist) && read_all(in, dist_dtheta));
  std::fclose(in);
  if (!ok || !loss_read || !dist_read) {
    std::fprintf(stderr, "%s: shorter than its header says\n", argv[1]);
    return 2;
  }
  if (with_loss && !ba_loss_valid(loss)) {
    std::fprintf(stderr, "%s: loss %d with scale %g is refused\n", argv[1], loss.kind, loss.scale);
    return 3;
  }
  if (opencv && G > VC_BA_MAX_GROUPS_OPENCV) {
    std::fprintf(stderr, "%s: %d groups with the tangential terms are refused (VC_BA_MAX_GROUPS_OPENCV)\n", argv[1], G);
    return 3;
  }
  if (with_dist && !opencv && G > VC_BA_MAX_GROUPS_RADIAL) {
    std::fprintf(stderr, "%s: %d groups with the distortion are refused (VC_BA_MAX_GROUPS_RADIAL)\n", argv[1], G);
    return 3;
  }
  std::vector<uint8_t> const_mask(n_cams), intr_mask(G);
  for (int a = 0; a < n_cams; ++a) const_mask[a] = (uint8_t)mask32[a];
  for (int g = 0; g < G; ++g) intr_mask[g] = (uint8_t)intr32[g];
  if (with_dist) {
    const BaProblem d{cams.data(), const_mask.data(), points.data(), offsets.data(), obs_cam.data(), obs_xy.data(), n_cams, n_points, total};
    const BaGroups gr{cam_group.data(), intr_mask.data(), G};
    return opencv ? run_dist<kBaDistOpencv>(argv[2], d, gr, loss, lambda, cam_offsets.data(), cam_obs.data(), obs_point.data(), cam_dist.data(),
                                            dc.data(), dist_dtheta.data())
                  : run_dist<kBaDistRadial>(argv[2], d, gr, loss, lambda, cam_offsets.data(), cam_obs.data(), obs_point.data(), cam_dist.data(),
                                            dc.data(), dist_dtheta.data());
  }

  // 1. the points pass and the total cost
  std::vector<double> vinv(6 * (size_t)n_points), gp(3 * (size_t)n_points), cost(n_points), total_cost(1, 0.0);
  std::vector<double> obs_lin((size_t)kBaLin * total);
  std::vector<int32_t> count(n_points);
  std::vector<uint8_t> obs_ok(total);
  std::vector<double> obs_w(with_loss ? total : 0);
  const BaProblem d{cams.data(), const_mask.data(), points.data(), offsets.data(), obs_cam.data(), obs_xy.data(), n_cams, n_points, total};
  for (int j = 0; j < n_points; ++j) {
    double v[6], g[3];
    count[j] = with_loss ? ba_linearize_point<true>(d, loss, j, lambda, v, g, cost[j], obs_ok.data(), obs_lin.data(), obs_w.data())
                         : ba_linearize_point<false>(d, loss, j, lambda, v, g, cost[j], obs_ok.data(), obs_lin.data(), nullptr);
    for (int k = 0; k < 6; ++k) vinv[6 * (size_t)j + k] = v[k];
    for (int k = 0; k < 3; ++k) gp[3 * (size_t)j + k] = g[k];
    total_cost[0] += cost[j];
  }

  // 2. the camera pass: one camera after another, the lanes of its workgroup one after another
  const BaLinear l{vinv.data(), gp.data(), obs_ok.data(), obs_lin.data()};
  std::vector<double> S(36 * (size_t)n_cams * n_cams), g(6 * (size_t)n_cams), acc(36 * (size_t)n_cams);
  for (int a = 0; a < n_cams; ++a) {
    BaLane lanes[kBaWave];
    for (int lane = 0; lane < kBaWave; ++lane) lanes[lane] = BaLane{0.0, 0.0, 0.0};
    for (double& v : acc) v = 0.0;
    camera_walk(d, l, cam_offsets.data(), cam_obs.data(), obs_point.data(), a, [&](int lane, int o, int j, int lo, int hi, const double* y) {
      ba_lane_update(d, l, a, o, j, lo, hi, lane, y, acc.data(), lanes[lane]);
    });
    for (int lane = 0; lane < kBaWave; ++lane)
      ba_lane_finish(n_cams, const_mask[a], lambda, a, lane, acc.data(), lanes[lane], S.data(), g.data());
  }

  // 3. the step under the caller's dc
  const Step plain = take_step(d, l, BaGroups{nullptr, nullptr, 0}, nullptr, dc.data(), nullptr);

  std::FILE* out = open_output(argv[2]);
  if (!out) return 2;
  write_all(out, vinv), write_all(out, gp), write_all(out, cost), write_all(out, total_cost), write_all(out, S), write_all(out, g);
  write_all(out, plain.cams), write_all(out, plain.points), write_all(out, plain.dx), write_all(out, obs_lin), write_all(out, count);
  write_all(out, obs_ok);

  if (G >= 1) {
    // 4. the intrinsics' terms of every point, their ordered sums, C and h
    const BaGroups gr{cam_group.data(), intr_mask.data(), G};
    const int rows = ba_term_rows(G), m = 4 * G;
    std::vector<double> obs_xn(2 * (size_t)total), T((size_t)n_points * G * kBaT), terms((size_t)rows * n_points), sums(rows);
    for (int j = 0; j < n_points; ++j) {
      if (with_loss) ba_linearize_point_intrinsics<true>(d, l, gr, obs_w.data(), j, obs_xn.data(), T.data(), terms.data());
      else ba_linearize_point_intrinsics<false>(d, l, gr, nullptr, j, obs_xn.data(), T.data(), terms.data());
    }
    for (int r = 0; r < rows; ++r) {
      double sum = 0.0;
      for (int j = 0; j < n_points; ++j) sum += terms[(size_t)r * n_points + j];
      sums[r] = sum;
    }
    std::vector<double> B(6 * (size_t)n_cams * m), C((size_t)m * m), h(m);
    std::vector<uint8_t> free_(m);
    for (int idx = 0; idx < m * m; ++idx) C[idx] = ba_border_c(sums.data(), gr, lambda, idx / m, idx % m);
    for (int row = 0; row < m; ++row) h[row] = ba_border_h(sums.data(), gr, row), free_[row] = ba_theta_free(sums.data(), gr, row / 4, row % 4) ? 1 : 0;

    // 5. the border's camera pass
    for (int a = 0; a < n_cams; ++a) {
      BaBorderLane lanes[kBaWave];
      for (int lane = 0; lane < kBaWave; ++lane)
        for (int k = 0; k < kBaBorderSlots; ++k) lanes[lane].jt[k] = lanes[lane].yt[k] = 0.0;
      const int ga = ba_group_of(gr, a);
      camera_walk(d, l, cam_offsets.data(), cam_obs.data(), obs_point.data(), a, [&](int lane, int o, int j, int, int, const double* y) {
        if (with_loss) ba_border_update<true>(l, gr, obs_xn.data(), obs_w.data(), T.data(), ga, o, j, lane, y, lanes[lane]);
        else ba_border_update<false>(l, gr, obs_xn.data(), nullptr, T.data(), ga, o, j, lane, y, lanes[lane]);
      });
      for (int lane = 0; lane < kBaWave; ++lane) ba_border_finish(G, a, lane, lanes[lane], B.data());
    }

    // 6. the step under the caller's dc and dtheta
    const Step step = take_step(d, l, gr, T.data(), dc.data(), dtheta.data());
    write_all(out, obs_xn), write_all(out, T), write_all(out, terms), write_all(out, sums), write_all(out, B), write_all(out, C);
    write_all(out, h), write_all(out, step.cams), write_all(out, step.points), write_all(out, step.dx), write_all(out, free_);
    write_all(out, step.valid);
  }
  write_all(out, obs_w);
  std::fclose(out);
  std::printf("%d cameras, %d points, %d observations, %d groups, cost %.17g\n", n_cams, n_points, total, G, total_cost[0]);
  return 0;
}
