// The three steps of vit_colmap_amd/csrc/bundle.hip on the CPU: its per-point and per-entry routines are __host__ __device__,
// so this program includes the kernel source and calls them point after point and, for the camera pass, lane after lane
// between the places where the kernel has its barriers.  It is how the kernels' arithmetic is compared with the specification
// without a GPU (tests/test_bundle_spec.py; HOST_SPEC_REL of tests/util_bundle.py was measured with it), what the GPU tests
// expect the kernels' bytes to equal, how the routines are run under a host sanitizer and where a fault in them is looked
// for with a host debugger.  tools/triangulate_host.cpp is its counterpart for csrc/triangulate.hip.
//
//   hipcc -x hip --offload-arch=gfx950 -O2 -std=c++17 -ffp-contract=off -o bundle_host tools/bundle_host.cpp
//   ./bundle_host problem.bin result.bin
// problem.bin: int32 n_cams, n_points, total; float64 lambda; int32 offsets (n_points + 1), obs_cam (total), cam_offsets
// (n_cams + 1), cam_obs (total), obs_point (total), const_mask (n_cams, one int32 each); float64 cams (n_cams, 16), points
// (n_points, 3), obs_xy (total, 2), dc (n_cams, 6): the step is taken with the caller's dc, no system is solved here.
// result.bin: float64 vinv (n_points, 6), gp (n_points, 3), cost (n_points), total_cost (1), S (6 n_cams, 6 n_cams), g
// (6 n_cams), out_cams (n_cams, 16), out_points (n_points, 3), dx (n_points, 3), obs_lin (total, 32); int32 count (n_points);
// uint8 obs_ok (total).  Offsets of any kind are passed on as they are: the routines check them.
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
  int32_t head[3];
  double lambda;
  if (std::fread(head, sizeof(int32_t), 3, in) != 3 || std::fread(&lambda, sizeof(double), 1, in) != 1 || head[0] < 0 || head[1] < 0 ||
      head[2] < 0 || head[0] > VC_BA_MAX_CAMS) {
    std::fprintf(stderr, "%s: no header\n", argv[1]);
    return 2;
  }
  const int n_cams = head[0], n_points = head[1], total = head[2];
  std::vector<int32_t> offsets(n_points + 1), obs_cam(total), cam_offsets(n_cams + 1), cam_obs(total), obs_point(total), mask32(n_cams);
  std::vector<double> cams(16 * (size_t)n_cams), points(3 * (size_t)n_points), obs_xy(2 * (size_t)total), dc(6 * (size_t)n_cams);
  const bool ok = read_all(in, offsets) && read_all(in, obs_cam) && read_all(in, cam_offsets) && read_all(in, cam_obs) &&
                  read_all(in, obs_point) && read_all(in, mask32) && read_all(in, cams) && read_all(in, points) && read_all(in, obs_xy) &&
                  read_all(in, dc);
  std::fclose(in);
  if (!ok) {
    std::fprintf(stderr, "%s: shorter than its header says\n", argv[1]);
    return 2;
  }
  std::vector<uint8_t> const_mask(n_cams);
  for (int a = 0; a < n_cams; ++a) const_mask[a] = (uint8_t)mask32[a];

  // 1. the points pass and the total cost
  std::vector<double> vinv(6 * (size_t)n_points), gp(3 * (size_t)n_points), cost(n_points), total_cost(1, 0.0);
  std::vector<double> obs_lin((size_t)kBaLin * total);
  std::vector<int32_t> count(n_points);
  std::vector<uint8_t> obs_ok(total);
  const BaProblem d{cams.data(), const_mask.data(), points.data(), offsets.data(), obs_cam.data(), obs_xy.data(), n_cams, n_points, total};
  for (int j = 0; j < n_points; ++j) {
    double v[6], g[3];
    count[j] = ba_linearize_point(d, j, lambda, v, g, cost[j], obs_ok.data(), obs_lin.data());
    for (int k = 0; k < 6; ++k) vinv[6 * (size_t)j + k] = v[k];
    for (int k = 0; k < 3; ++k) gp[3 * (size_t)j + k] = g[k];
    total_cost[0] += cost[j];
  }

  // 2. the camera pass: one camera after another, the lanes of its workgroup one after another
  const BaLinear l{vinv.data(), gp.data(), obs_ok.data(), obs_lin.data()};
  std::vector<double> S(36 * (size_t)n_cams * n_cams), g(6 * (size_t)n_cams), acc(36 * (size_t)n_cams);
  for (int a = 0; a < n_cams; ++a) {
    BaBatch batch;
    BaLane lanes[kBaWave];
    for (int lane = 0; lane < kBaWave; ++lane) lanes[lane] = BaLane{0.0, 0.0, 0.0};
    for (double& v : acc) v = 0.0;
    const int first = cam_offsets[a], last = cam_offsets[a + 1];
    if (first >= 0 && last >= first && last <= total) {
      for (int base = first; base < last; base += kBaWave) {
        for (int lane = 0; lane < kBaWave; ++lane) ba_prepare(d, l, cam_obs.data(), obs_point.data(), a, base + lane, last, lane, batch);
        const int m = last - base < kBaWave ? last - base : kBaWave;
        for (int lane = 0; lane < kBaWave; ++lane)
          for (int k = 0; k < m; ++k)
            if (batch.o[k] >= 0)
              ba_lane_update(d, l, a, batch.o[k], batch.j[k], batch.lo[k], batch.hi[k], lane, batch.y[k], acc.data(), lanes[lane]);
      }
    }
    for (int lane = 0; lane < kBaWave; ++lane)
      ba_lane_finish(n_cams, const_mask[a], lambda, a, lane, acc.data(), lanes[lane], S.data(), g.data());
  }

  // 3. the step under the caller's dc
  std::vector<double> out_cams(16 * (size_t)n_cams), out_points(3 * (size_t)n_points), dx(3 * (size_t)n_points);
  for (int j = 0; j < n_points; ++j) {
    double dX[3];
    ba_point_step(d, l, dc.data(), j, dX);
    for (int k = 0; k < 3; ++k) dx[3 * (size_t)j + k] = dX[k], out_points[3 * (size_t)j + k] = points[3 * (size_t)j + k] + dX[k];
  }
  for (int a = 0; a < n_cams; ++a) ba_camera_step(cams.data() + 16 * (size_t)a, dc.data() + 6 * (size_t)a, out_cams.data() + 16 * (size_t)a);

  std::FILE* out = std::fopen(argv[2], "wb");
  if (!out) {
    std::fprintf(stderr, "cannot open %s\n", argv[2]);
    return 2;
  }
  write_all(out, vinv), write_all(out, gp), write_all(out, cost), write_all(out, total_cost), write_all(out, S), write_all(out, g);
  write_all(out, out_cams), write_all(out, out_points), write_all(out, dx), write_all(out, obs_lin), write_all(out, count);
  write_all(out, obs_ok);
  std::fclose(out);
  std::printf("%d cameras, %d points, %d observations, cost %.17g\n", n_cams, n_points, total, total_cost[0]);
  return 0;
}
