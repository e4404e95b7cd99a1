// The kernels of vit_colmap_amd/csrc/bundle.hip on the CPU, the plain adjustment and the border of the intrinsics: its per-point
// and per-entry routines are __host__ __device__, so this program includes the kernel source and calls them point after point,
// row after row and, for the two camera passes, lane after lane between the places where the kernel has its barriers.  It is how
// the kernels' arithmetic is compared with the specification without a GPU (tests/test_bundle*_spec.py; HOST_SPEC_REL of
// tests/util_bundle.py and tests/util_bundle_intr.py was measured with it), what the GPU tests expect the kernels' bytes to equal,
// how the routines are run under a host sanitizer and where a fault in them is looked for with a host debugger.
// tools/triangulate_host.cpp is its counterpart for csrc/triangulate.hip.
//
//   hipcc -x hip --offload-arch=gfx950 -O2 -std=c++17 -ffp-contract=off -o bundle_host tools/bundle_host.cpp
//   ./bundle_host problem.bin result.bin
// problem.bin: int32 n_cams, n_points, total, n_groups (>= 0); float64 lambda; int32 offsets (n_points + 1), obs_cam (total),
// cam_offsets (n_cams + 1), cam_obs (total), obs_point (total), const_mask (n_cams), cam_group (n_cams; none without groups),
// intr_mask (n_groups); float64 cams (n_cams, 16), points (n_points, 3), obs_xy (total, 2), dc (n_cams, 6), dtheta (n_groups, 4):
// the steps are taken with the caller's dc and dtheta, no system is solved here.  Two optional sections follow, and they choose
// the instance run<kLoss, kDist> of the passes, one of bundle.hip's four:
//   nothing                                              (false, kBaDistNone)
//   int32 loss, float64 loss_scale                       (true, kBaDistNone): "The loss" in DESIGN.md §4.2k
//   then int32 1, float64 cam_dist (n_cams, 2),          (true, kBaDistRadial): "The distortion"; VC_BA_LOSS_TRIVIAL, 1.0 is the
//     dtheta (n_groups, 6)                                 plain case; the first dtheta of the file is not used
//   or int32 2, float64 cam_dist (n_cams, 4),            (true, kBaDistOpencv): "The tangential terms"
//     dtheta (n_groups, 8)
// result.bin, with N = 4, 6, 8 unknowns per group, K = 0, 2, 4 numbers per row of cam_dist and J = 2, 6, 10 per row of obs_jt:
// the plain section, float64 vinv (n_points, 6), gp (n_points, 3), cost (n_points), total_cost (1), S (6 n_cams, 6 n_cams), g
// (6 n_cams), out_cams (n_cams, 16), out_points (n_points, 3), dx (n_points, 3) (the step under dc alone), obs_lin (total, 32);
// int32 count (n_points); uint8 obs_ok (total).  With n_groups = G >= 1 the border's section follows: float64 obs_jt (total, J;
// the pinhole's obs_xn), T (n_points, G, 3 N), terms (2 N G + N^2 (G + G^2), n_points), sums (as many), B (6 n_cams, N G), C (N G,
// N G), h (N G), out_cams, out_points, dx (the step under dc and dtheta), out_dist (n_cams, K; none for the pinhole); uint8 free
// (N G), valid (n_cams).  With a loss the file ends with float64 obs_w (total).
// Offsets of any kind are passed on as they are: the routines check them.  Exit status 2: a file that does not open or is shorter
// than its header says; 3, with one line on stderr and no result: a loss that the entry points refuse (ba_loss_valid) or more
// groups than the model's limit (VC_BA_MAX_GROUPS_RADIAL, VC_BA_MAX_GROUPS_OPENCV).
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

// The two step kernels -> out_cams, out_points, dx, out_dist, valid.
struct Step {
  std::vector<double> cams, points, dx, dist;
  std::vector<uint8_t> valid;
};

template <int kDist>
static Step take_step(const BaProblem& d, const BaLinear& l, const BaGroups& gr, const double* T, const double* dc, const double* dtheta) {
  constexpr int kParams = ba_dist_params(kDist);
  Step s{std::vector<double>(16 * (size_t)d.n_cams), std::vector<double>(3 * (size_t)d.n_points), std::vector<double>(3 * (size_t)d.n_points),
         std::vector<double>(kParams * (size_t)d.n_cams), std::vector<uint8_t>(d.n_cams)};
  for (int j = 0; j < d.n_points; ++j) {
    double dX[3];
    ba_point_step<ba_dist_unknowns(kDist)>(d, l, T, gr.n_groups, dc, dtheta, j, dX);
    for (int k = 0; k < 3; ++k) s.dx[3 * (size_t)j + k] = dX[k], s.points[3 * (size_t)j + k] = d.points[3 * (size_t)j + k] + dX[k];
  }
  for (int a = 0; a < d.n_cams; ++a)
    s.valid[a] = ba_camera_step<kDist>(d.cams + 16 * (size_t)a, d.cam_dist + kParams * (size_t)a, dc + 6 * (size_t)a, gr, a, dtheta,
                                       s.cams.data() + 16 * (size_t)a, s.dist.data() + kParams * (size_t)a) ? 1 : 0;
  return s;
}

// Every pass under (kLoss, kDist) -> result.bin at path.
template <bool kLoss, int kDist>
static int run(const char* path, const BaProblem& d, const BaGroups& gr, const BaLoss& loss, double lambda, const int32_t* cam_offsets,
               const int32_t* cam_obs, const int32_t* obs_point, const double* dc, const double* dtheta) {
  constexpr int N = ba_dist_unknowns(kDist);
  const int n_cams = d.n_cams, n_points = d.n_points, total = d.total, G = gr.n_groups;
  // 1. the points pass and the total cost
  std::vector<double> vinv(6 * (size_t)n_points), gp(3 * (size_t)n_points), cost(n_points), total_cost(1, 0.0);
  std::vector<double> obs_lin((size_t)kBaLin * total), obs_w(kLoss ? total : 0);
  std::vector<int32_t> count(n_points);
  std::vector<uint8_t> obs_ok(total);
  for (int j = 0; j < n_points; ++j) {
    double v[6], g[3];
    count[j] = ba_linearize_point<kLoss, kDist>(d, loss, j, lambda, v, g, cost[j], obs_ok.data(), obs_lin.data(), obs_w.data());
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
    camera_walk(d, l, cam_offsets, cam_obs, obs_point, a, [&](int lane, int o, int j, int lo, int hi, const double* y) {
      ba_lane_update(d, l, a, o, j, lo, hi, lane, y, acc.data(), lanes[lane]);
    });
    for (int lane = 0; lane < kBaWave; ++lane) ba_lane_finish(n_cams, d.const_mask[a], lambda, a, lane, acc.data(), lanes[lane], S.data(), g.data());
  }

  // 3. the step under the caller's dc
  const Step plain = take_step<kDist>(d, l, BaGroups{nullptr, nullptr, 0}, nullptr, dc, nullptr);

  std::FILE* out = open_output(path);
  if (!out) return 2;
  write_all(out, vinv), write_all(out, gp), write_all(out, cost), write_all(out, total_cost), write_all(out, S), write_all(out, g);
  write_all(out, plain.cams), write_all(out, plain.points), write_all(out, plain.dx), write_all(out, obs_lin), write_all(out, count);
  write_all(out, obs_ok);
  if (G >= 1) {
    // 4. the intrinsics' terms of every point, their ordered sums, C and h
    const int rows = ba_term_rows<N>(G), m = N * G;
    std::vector<double> obs_jt((size_t)ba_dist_jt(kDist) * total), T((size_t)n_points * G * 3 * N), terms((size_t)rows * n_points), sums(rows);
    for (int j = 0; j < n_points; ++j) ba_linearize_point_intrinsics<kLoss, kDist>(d, l, gr, obs_w.data(), j, obs_jt.data(), T.data(), terms.data());
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

    // 5. the border's camera pass
    for (int a = 0; a < n_cams; ++a) {
      BaBorderLane lanes[kBaWave];
      for (int lane = 0; lane < kBaWave; ++lane)
        for (int k = 0; k < kBaBorderSlots; ++k) lanes[lane].jt[k] = lanes[lane].yt[k] = 0.0;
      const int ga = ba_group_of(gr, a);
      camera_walk(d, l, cam_offsets, cam_obs, obs_point, a, [&](int lane, int o, int j, int, int, const double* y) {
        ba_border_update<kLoss, kDist>(l, gr, obs_jt.data(), obs_w.data(), T.data(), ga, o, j, lane, y, lanes[lane]);
      });
      for (int lane = 0; lane < kBaWave; ++lane) ba_border_finish<N>(G, a, lane, lanes[lane], B.data());
    }

    // 6. the step under the caller's dc and dtheta
    const Step step = take_step<kDist>(d, l, gr, T.data(), dc, dtheta);
    write_all(out, obs_jt), write_all(out, T), write_all(out, terms), write_all(out, sums), write_all(out, B), write_all(out, C);
    write_all(out, h), write_all(out, step.cams), write_all(out, step.points), write_all(out, step.dx), write_all(out, step.dist);
    write_all(out, free_), write_all(out, step.valid);
  }
  write_all(out, obs_w);
  std::fclose(out);
  std::printf("%d cameras, %d points, %d observations, %d groups, %scost %.17g\n", n_cams, n_points, total, G,
              kDist == kBaDistOpencv ? "opencv, " : kDist == kBaDistRadial ? "radial, " : "", total_cost[0]);
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
  const BaProblem d{cams.data(), const_mask.data(), points.data(), offsets.data(), obs_cam.data(), obs_xy.data(), n_cams, n_points, total,
                    with_dist ? cam_dist.data() : nullptr};
  const BaGroups gr{cam_group.data(), intr_mask.data(), G};
  const double* dth = with_dist ? dist_dtheta.data() : dtheta.data();
  auto go = [&](auto run_fn) { return run_fn(argv[2], d, gr, loss, lambda, cam_offsets.data(), cam_obs.data(), obs_point.data(), dc.data(), dth); };
  if (opencv) return go(run<true, kBaDistOpencv>);
  if (with_dist) return go(run<true, kBaDistRadial>);
  return with_loss ? go(run<true, kBaDistNone>) : go(run<false, kBaDistNone>);
}
