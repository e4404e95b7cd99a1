// The five-point solver of vit_colmap_amd/csrc/essential.hip on the CPU, the counterpart of p3p_host.cpp: its solver functions
// are __host__ __device__, so this program includes the kernel source and calls solve_five_point on one problem after another
// (stride 1 for the work area that the kernel keeps in LDS).  It is how the solver is compared with the specification without
// a GPU (tests/test_solver_host.py), how it is run under a host sanitizer and where a fault in it is looked for with a host
// debugger.
//
//   hipcc -x hip --offload-arch=gfx950 -O2 -std=c++17 -ffp-contract=off -o five_point_host tools/five_point_host.cpp
//   ./five_point_host problems.bin matrices.bin
// problems.bin: n records of 20 float64 (five rows of x1 y1 x2 y2, normalised); matrices.bin: n records of 1 + 90 float64
// (the count, then ten matrices of 9, row-major, NaN past the count).
#include <cstdio>
#include <vector>

#include "../vit_colmap_amd/csrc/essential.hip"

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s problems.bin matrices.bin\n", argv[0]);
    return 2;
  }
  std::FILE* in = std::fopen(argv[1], "rb");
  std::FILE* out = std::fopen(argv[2], "wb");
  if (!in || !out) {
    std::fprintf(stderr, "cannot open %s or %s\n", argv[1], argv[2]);
    return 2;
  }
  double rec[20];
  long n = 0, solutions = 0;
  while (std::fread(rec, sizeof(double), 20, in) == 20) {
    double x1[5], y1[5], x2[5], y2[5];
    for (int i = 0; i < 5; ++i) x1[i] = rec[4 * i], y1[i] = rec[4 * i + 1], x2[i] = rec[4 * i + 2], y2[i] = rec[4 * i + 3];
    std::vector<double> work(kWorkDoubles, 0.0), res(1 + kMaxSolutions * 9, NAN);
    const int count = solve_five_point(x1, y1, x2, y2, work.data(), 1, res.data() + 1);
    for (int i = 1 + 9 * count; i < 1 + kMaxSolutions * 9; ++i) res[i] = NAN;
    res[0] = count;
    std::fwrite(res.data(), sizeof(double), res.size(), out);
    ++n, solutions += count;
  }
  std::fclose(in);
  std::fclose(out);
  std::printf("%ld problems, %ld solutions\n", n, solutions);
  return 0;
}
