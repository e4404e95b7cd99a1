// The P3P solver of vit_colmap_amd/csrc/absolute_pose.hip on the CPU: its solver functions are __host__ __device__, so this
// program includes the kernel source and calls solve_p3p on one problem after another.  It is how the solver is compared
// with the specification without a GPU (tests/test_solver_host.py; the tolerance of tests/test_absolute_pose_gpu.py was
// measured with it), how it is run under a host sanitizer and where a fault in it is looked for with a host debugger.
// tools/five_point_host.cpp is its counterpart for csrc/essential.hip.
//
//   hipcc -x hip --offload-arch=gfx950 -O2 -std=c++17 -ffp-contract=off -o p3p_host tools/p3p_host.cpp
//   ./p3p_host problems.bin poses.bin
// problems.bin: n records of 15 float64 (x0 y0 x1 y1 x2 y2, then the three world points); poses.bin: n records of
// 1 + 48 float64 (the count, then four poses of 12, NaN past the count).
#include <cstdio>
#include <vector>

#include "../vit_colmap_amd/csrc/absolute_pose.hip"

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s problems.bin poses.bin\n", argv[0]);
    return 2;
  }
  std::FILE* in = std::fopen(argv[1], "rb");
  std::FILE* out = std::fopen(argv[2], "wb");
  if (!in || !out) {
    std::fprintf(stderr, "cannot open %s or %s\n", argv[1], argv[2]);
    return 2;
  }
  double rec[15];
  long n = 0, solutions = 0;
  while (std::fread(rec, sizeof(double), 15, in) == 15) {
    const double x[3] = {rec[0], rec[2], rec[4]}, y[3] = {rec[1], rec[3], rec[5]};
    Triangle g;
    for (int i = 0; i < 3; ++i)
      for (int k = 0; k < 3; ++k) g.X[i][k] = rec[6 + 3 * i + k];
    std::vector<double> res(1 + kMaxPoses * 12, NAN);
    const int count = solve_p3p(x, y, g, res.data() + 1);
    for (int i = 1 + 12 * count; i < 1 + kMaxPoses * 12; ++i) res[i] = NAN;
    res[0] = count;
    std::fwrite(res.data(), sizeof(double), res.size(), out);
    ++n, solutions += count;
  }
  std::fclose(in);
  std::fclose(out);
  std::printf("%ld problems, %ld solutions\n", n, solutions);
  return 0;
}
