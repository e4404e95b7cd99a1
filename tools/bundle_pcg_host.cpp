// The solver's kernels of vit_colmap_amd/csrc/bundle.hip on the CPU (vc_ba_camera_blocks, vc_ba_schur_product; "The solver" in
// DESIGN.md §4.2k): their per-observation and per-entry routines are __host__ __device__, so this program includes the kernel
// source and calls them point after point and, for the two camera passes, lane after lane between the places where the kernels
// have their barriers.  It is how their arithmetic is compared with the specification without a GPU (tests/test_bundle_pcg_spec.py;
// the bounds of tests/util_bundle_pcg.py were measured with it), what the GPU tests expect the kernels' bytes to equal and how the
// routines are run under a host sanitizer.  tools/bundle_host.cpp is its counterpart for the dense route; its file format is not
// this one's.
//
//   hipcc -x hip --offload-arch=gfx950 -O2 -std=c++17 -ffp-contract=off -o bundle_pcg_host tools/bundle_pcg_host.cpp
//   ./bundle_pcg_host problem.bin result.bin
// problem.bin: int32 n_cams, n_points, total, n_vectors (>= 0), loss; float64 lambda, loss_scale; int32 offsets (n_points + 1),
// obs_cam (total), cam_offsets (n_cams + 1), cam_obs (total), obs_point (total), const_mask (n_cams); float64 cams (n_cams, 16),
// points (n_points, 3), obs_xy (total, 2), p (n_vectors, 6 n_cams).  loss VC_BA_LOSS_TRIVIAL runs vc_ba_linearize_points' routine,
// any other vc_ba_linearize_points_loss'; one that the entry point refuses: one line on stderr, exit status 3.  No limit on n_cams.
// result.bin: float64 U (n_cams, 36), D (n_cams, 36), Minv (n_cams, 36), g (6 n_cams), s (n_vectors, n_points, 3), q (n_vectors,
// 6 n_cams), vinv (n_points, 6), total_cost (1); uint8 fixed (6 n_cams), obs_ok (total).
// Offsets of any kind are passed on as they are: the routines check them.
#include "../vit_colmap_amd/csrc/bundle.hip"
#include "host_io.h"

int main(int argc, char** argv) {
  std::FILE* in = open_input(argc, argv, "problem.bin result.bin");
  if (!in) return 2;
  int32_t head[5];
  double scalars[2];
  if (std::fread(head, sizeof(int32_t), 5, in) != 5 || std::fread(scalars, sizeof(double), 2, in) != 2 || head[0] < 0 || head[1] < 0 ||
      head[2] < 0 || head[3] < 0) {
    std::fprintf(stderr, "%s: no header\n", argv[1]);
    return 2;
  }
  const int n_cams = head[0], n_points = head[1], total = head[2], n_vectors = head[3];
  const BaLoss loss{head[4], scalars[1]};
  const double lambda = scalars[0];
  std::vector<int32_t> offsets(n_points + 1), obs_cam(total), cam_offsets(n_cams + 1), cam_obs(total), obs_point(total), mask32(n_cams);
  std::vector<double> cams(16 * (size_t)n_cams), points(3 * (size_t)n_points), obs_xy(2 * (size_t)total), p((size_t)n_vectors * 6 * n_cams);
  const bool ok = read_all(in, offsets) && read_all(in, obs_cam) && read_all(in, cam_offsets) && read_all(in, cam_obs) &&
                  read_all(in, obs_point) && read_all(in, mask32) && read_all(in, cams) && read_all(in, points) && read_all(in, obs_xy) &&
                  read_all(in, p);
  std::fclose(in);
  if (!ok) {
    std::fprintf(stderr, "%s: shorter than its header says\n", argv[1]);
    return 2;
  }
  if (!ba_loss_valid(loss) || !(lambda >= 0.0 && lambda < INFINITY)) {
    std::fprintf(stderr, "%s: loss %d with scale %g or lambda %g is refused\n", argv[1], loss.kind, loss.scale, lambda);
    return 3;
  }
  std::vector<uint8_t> const_mask(n_cams);
  for (int a = 0; a < n_cams; ++a) const_mask[a] = (uint8_t)mask32[a];

  // 1. the points pass of the linearisation
  std::vector<double> vinv(6 * (size_t)n_points), gp(3 * (size_t)n_points), total_cost(1, 0.0), obs_lin((size_t)kBaLin * total), obs_w(total);
  std::vector<uint8_t> obs_ok(total);
  const BaProblem d{cams.data(), const_mask.data(), points.data(), offsets.data(), obs_cam.data(), obs_xy.data(), n_cams, n_points, total};
  for (int j = 0; j < n_points; ++j) {
    double v[6], g[3], cost;
    if (loss.kind == VC_BA_LOSS_TRIVIAL) ba_linearize_point<false, kBaDistNone>(d, loss, j, lambda, v, g, cost, obs_ok.data(), obs_lin.data(), nullptr);
    else ba_linearize_point<true, kBaDistNone>(d, loss, j, lambda, v, g, cost, obs_ok.data(), obs_lin.data(), obs_w.data());
    for (int k = 0; k < 6; ++k) vinv[6 * (size_t)j + k] = v[k];
    for (int k = 0; k < 3; ++k) gp[3 * (size_t)j + k] = g[k];
    total_cost[0] += cost;
  }
  const BaLinear l{vinv.data(), gp.data(), obs_ok.data(), obs_lin.data()};

  // 2. the blocks pass: one camera after another, the lanes of its wave one after another between the barriers of ba_camera_walk
  std::vector<double> U(36 * (size_t)n_cams), D(36 * (size_t)n_cams), Minv(36 * (size_t)n_cams), g(6 * (size_t)n_cams);
  std::vector<uint8_t> fixed(6 * (size_t)n_cams);
  for (int a = 0; a < n_cams; ++a) {
    BaBlockLane lanes[kBaWave];
    for (int lane = 0; lane < kBaWave; ++lane) lanes[lane] = BaBlockLane{0.0, 0.0, 0.0, 0.0};
    BaBatch batch;
    int first, last;
    if (ba_camera_list(cam_offsets.data(), a, total, first, last))
      for (int base = first; base < last; base += kBaWave) {
        for (int lane = 0; lane < kBaWave; ++lane) ba_prepare(d, l, cam_obs.data(), obs_point.data(), a, base + lane, last, lane, batch);
        const int m = last - base < kBaWave ? last - base : kBaWave;
        for (int lane = 0; lane < kBaWave; ++lane)
          for (int k = 0; k < m; ++k)
            if (batch.o[k] >= 0) ba_block_update(d, l, a, batch.o[k], batch.j[k], batch.lo[k], batch.hi[k], lane, batch.y[k], lanes[lane]);
      }
    double* block = D.data() + 36 * (size_t)a;
    for (int lane = 0; lane < 36; ++lane) {
      bool fix;
      const double u = ba_block_u(const_mask[a], lambda, lane, lanes[lane].u, fix);
      U[36 * (size_t)a + lane] = u, block[lane] = u - lanes[lane].acc;
      if (lane / 6 == lane % 6) fixed[6 * (size_t)a + lane / 6] = fix ? 1 : 0;
    }
    for (int lane = 0; lane < 6; ++lane) {
      g[6 * (size_t)a + lane] = fixed[6 * (size_t)a + lane] ? 0.0 : lanes[lane].gr - lanes[lane].gy;
      double x[6];
      ba_block_inverse(block, lane, x);
      for (int i = 0; i < 6; ++i) Minv[36 * (size_t)a + 6 * i + lane] = x[i];
    }
  }

  // 3. the product for every vector: the points pass, then per camera the batches of its list, every lane preparing its entry
  // before the six owners add the batch in order
  std::vector<double> s((size_t)n_vectors * 3 * n_points), q((size_t)n_vectors * 6 * n_cams);
  for (int v = 0; v < n_vectors; ++v) {
    const double* pv = p.data() + (size_t)v * 6 * n_cams;
    double* sv = s.data() + (size_t)v * 3 * n_points;
    for (int j = 0; j < n_points; ++j) {
      double sj[3];
      ba_product_point(d, l, fixed.data(), pv, j, sj);
      for (int k = 0; k < 3; ++k) sv[3 * (size_t)j + k] = sj[k];
    }
    for (int a = 0; a < n_cams; ++a) {
      double sums[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      BaProductBatch batch;
      int first, last;
      if (ba_camera_list(cam_offsets.data(), a, total, first, last))
        for (long long base = first; base < last; base += kBaProductThreads) {
          const int m = last - base < kBaProductThreads ? (int)(last - base) : kBaProductThreads;
          for (int lane = 0; lane < kBaProductThreads; ++lane)
            ba_product_prepare(d, l, obs_point.data(), sv, a, lane < m ? cam_obs[base + lane] : -1, lane, batch);
          for (int i = 0; i < 6; ++i) ba_product_add(batch, m, i, sums[i]);
        }
      for (int i = 0; i < 6; ++i) q[(size_t)v * 6 * n_cams + 6 * (size_t)a + i] = ba_product_finish(U.data(), fixed.data(), pv, a, i, sums[i]);
    }
  }

  std::FILE* out = open_output(argv[2]);
  if (!out) return 2;
  write_all(out, U), write_all(out, D), write_all(out, Minv), write_all(out, g), write_all(out, s), write_all(out, q), write_all(out, vinv);
  write_all(out, total_cost), write_all(out, fixed), write_all(out, obs_ok);
  std::fclose(out);
  std::printf("%d cameras, %d points, %d observations, %d vectors, cost %.17g\n", n_cams, n_points, total, n_vectors, total_cost[0]);
  return 0;
}
