// The border of the intrinsics of vit_colmap_amd/csrc/bundle.hip on the CPU: tools/bundle_host.cpp's
// counterpart for vc_ba_linearize_intrinsics, vc_ba_reduce_border and vc_ba_step_intrinsics.  It includes the kernel source and
// calls its __host__ __device__ routines point after point, row after row and, for the camera pass, lane after lane between the
// places where the kernel has its barriers.  tests/test_bundle_intr_spec.py compares it with the specification
// (tests/util_bundle_intr.py) and runs it under the host sanitizers; tests/test_bundle_intr_gpu.py expects the kernels' bytes to
// equal its output.
//
//   hipcc -x hip --offload-arch=gfx950 -O2 -std=c++17 -ffp-contract=off -o bundle_intr_host tools/bundle_intr_host.cpp
//   ./bundle_intr_host problem.bin result.bin
// problem.bin: int32 n_cams, n_points, total, n_groups; float64 lambda; int32 offsets (n_points + 1), obs_cam (total),
// cam_offsets (n_cams + 1), cam_obs (total), obs_point (total), const_mask (n_cams), cam_group (n_cams), intr_mask (n_groups);
// float64 cams (n_cams, 16), points (n_points, 3), obs_xy (total, 2), dc (n_cams, 6), dtheta (n_groups, 4): the step is taken
// with the caller's dc and dtheta, no system is solved here.
// result.bin: float64 obs_xn (total, 2), T (n_points, n_groups, 12), terms (24 G + 16 G^2, n_points), sums (24 G + 16 G^2),
// B (6 n_cams, 4 G), C (4 G, 4 G), h (4 G), out_cams (n_cams, 16), out_points (n_points, 3), dx (n_points, 3); uint8 free (4 G),
// valid (n_cams).
#include <cstdio>
#include <vector>

#include "../vit_colmap_amd/csrc/bundle.hip"

template <typename T>
static bool read_all(std::FILE* f, std::vector<T>& v) {
  return v.empty() || std::fread(v.data(), sizeof(T), v.size(), f) == v.size();
}

template <typename T>
static void write_all(std::FILE* f, const std::vector<T>& v) {
  if (!v.empty()) std::fwrite(v.data(), sizeof(T), v.size(), f);
}

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s problem.bin result.bin\n", argv[0]);
    return 2;
  }
  std::FILE* in = std::fopen(argv[1], "rb");
  if (!in) {
    std::fprintf(stderr, "cannot open %s\n", argv[1]);
    return 2;
  }
  int32_t head[4];
  double lambda;
  if (std::fread(head, sizeof(int32_t), 4, in) != 4 || std::fread(&lambda, sizeof(double), 1, in) != 1 || head[0] < 0 || head[1] < 0 ||
      head[2] < 0 || head[3] < 1 || head[0] > VC_BA_MAX_CAMS || head[3] > VC_BA_MAX_GROUPS) {
    std::fprintf(stderr, "%s: no header\n", argv[1]);
    return 2;
  }
  const int n_cams = head[0], n_points = head[1], total = head[2], G = head[3];
  std::vector<int32_t> offsets(n_points + 1), obs_cam(total), cam_offsets(n_cams + 1), cam_obs(total), obs_point(total), mask32(n_cams);
  std::vector<int32_t> cam_group(n_cams), intr32(G);
  std::vector<double> cams(16 * (size_t)n_cams), points(3 * (size_t)n_points), obs_xy(2 * (size_t)total), dc(6 * (size_t)n_cams);
  std::vector<double> dtheta(4 * (size_t)G);
  const bool ok = read_all(in, offsets) && read_all(in, obs_cam) && read_all(in, cam_offsets) && read_all(in, cam_obs) &&
                  read_all(in, obs_point) && read_all(in, mask32) && read_all(in, cam_group) && read_all(in, intr32) && read_all(in, cams) &&
                  read_all(in, points) && read_all(in, obs_xy) && read_all(in, dc) && read_all(in, dtheta);
  std::fclose(in);
  if (!ok) {
    std::fprintf(stderr, "%s: shorter than its header says\n", argv[1]);
    return 2;
  }
  std::vector<uint8_t> const_mask(n_cams), intr_mask(G);
  for (int a = 0; a < n_cams; ++a) const_mask[a] = (uint8_t)mask32[a];
  for (int g = 0; g < G; ++g) intr_mask[g] = (uint8_t)intr32[g];

  // 1. the points pass of tools/bundle_host.cpp, then the intrinsics' terms of every point
  std::vector<double> vinv(6 * (size_t)n_points), gp(3 * (size_t)n_points), cost(n_points), obs_lin((size_t)kBaLin * total);
  std::vector<uint8_t> obs_ok(total);
  const BaProblem d{cams.data(), const_mask.data(), points.data(), offsets.data(), obs_cam.data(), obs_xy.data(), n_cams, n_points, total};
  for (int j = 0; j < n_points; ++j) {
    double v[6], g[3];
    ba_linearize_point(d, j, lambda, v, g, cost[j], obs_ok.data(), obs_lin.data());
    for (int k = 0; k < 6; ++k) vinv[6 * (size_t)j + k] = v[k];
    for (int k = 0; k < 3; ++k) gp[3 * (size_t)j + k] = g[k];
  }
  const BaLinear l{vinv.data(), gp.data(), obs_ok.data(), obs_lin.data()};
  const BaGroups gr{cam_group.data(), intr_mask.data(), G};
  const int rows = ba_term_rows(G);
  std::vector<double> obs_xn(2 * (size_t)total), T((size_t)n_points * G * kBaT), terms((size_t)rows * n_points), sums(rows);
  for (int j = 0; j < n_points; ++j) ba_linearize_point_intrinsics(d, l, gr, j, obs_xn.data(), T.data(), terms.data());

  // 2. the ordered sums, C and h, then the camera pass: one camera after another, its lanes one after another
  for (int r = 0; r < rows; ++r) {
    double sum = 0.0;
    for (int j = 0; j < n_points; ++j) sum += terms[(size_t)r * n_points + j];
    sums[r] = sum;
  }
  const int m = 4 * G;
  std::vector<double> B(6 * (size_t)n_cams * m), C((size_t)m * m), h(m);
  std::vector<uint8_t> free_(m), valid(n_cams);
  for (int idx = 0; idx < m * m; ++idx) C[idx] = ba_border_c(sums.data(), gr, lambda, idx / m, idx % m);
  for (int row = 0; row < m; ++row) h[row] = ba_border_h(sums.data(), gr, row), free_[row] = ba_theta_free(sums.data(), gr, row / 4, row % 4) ? 1 : 0;
  for (int a = 0; a < n_cams; ++a) {
    BaBatch batch;
    BaBorderLane lanes[kBaWave];
    for (int lane = 0; lane < kBaWave; ++lane)
      for (int k = 0; k < kBaBorderSlots; ++k) lanes[lane].jt[k] = lanes[lane].yt[k] = 0.0;
    const int ga = ba_group_of(gr, a);
    const int first = cam_offsets[a], last = cam_offsets[a + 1];
    if (first >= 0 && last >= first && last <= total) {
      for (int base = first; base < last; base += kBaWave) {
        for (int lane = 0; lane < kBaWave; ++lane) ba_prepare(d, l, cam_obs.data(), obs_point.data(), a, base + lane, last, lane, batch);
        const int n = last - base < kBaWave ? last - base : kBaWave;
        for (int lane = 0; lane < kBaWave; ++lane)
          for (int k = 0; k < n; ++k)
            if (batch.o[k] >= 0) ba_border_update(l, gr, obs_xn.data(), T.data(), ga, batch.o[k], batch.j[k], lane, batch.y[k], lanes[lane]);
      }
    }
    for (int lane = 0; lane < kBaWave; ++lane) ba_border_finish(G, a, lane, lanes[lane], B.data());
  }

  // 3. the step under the caller's dc and dtheta
  std::vector<double> out_cams(16 * (size_t)n_cams), out_points(3 * (size_t)n_points), dx(3 * (size_t)n_points);
  for (int j = 0; j < n_points; ++j) {
    double dX[3];
    ba_point_step_intrinsics(d, l, T.data(), G, dc.data(), dtheta.data(), j, dX);
    for (int k = 0; k < 3; ++k) dx[3 * (size_t)j + k] = dX[k], out_points[3 * (size_t)j + k] = points[3 * (size_t)j + k] + dX[k];
  }
  for (int a = 0; a < n_cams; ++a)
    valid[a] = ba_camera_step_intrinsics(cams.data() + 16 * (size_t)a, dc.data() + 6 * (size_t)a, gr, a, dtheta.data(),
                                         out_cams.data() + 16 * (size_t)a) ? 1 : 0;

  std::FILE* out = std::fopen(argv[2], "wb");
  if (!out) {
    std::fprintf(stderr, "cannot open %s\n", argv[2]);
    return 2;
  }
  write_all(out, obs_xn), write_all(out, T), write_all(out, terms), write_all(out, sums), write_all(out, B), write_all(out, C);
  write_all(out, h), write_all(out, out_cams), write_all(out, out_points), write_all(out, dx), write_all(out, free_), write_all(out, valid);
  std::fclose(out);
  std::printf("%d cameras, %d points, %d observations, %d groups\n", n_cams, n_points, total, G);
  return 0;
}
