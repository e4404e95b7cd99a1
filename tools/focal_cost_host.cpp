// The focal-length cost of vit_colmap_amd/csrc/focal.hip (vc_focal_cost) on the CPU: focal_load_pair,
// focal_pair_cost, focal_ratio_ok and focal_mean are __host__ __device__, so this program includes the kernel source, calls them on one pair
// after another and adds the terms in the kernels' order (chunks of kFocalChunk pairs in pair order, then the chunks in order).
// It is how the kernel's arithmetic is compared with the specification without a GPU (tests/test_focal_spec.py), how it is run
// under a host sanitizer and what the GPU test compares the kernel's bytes with.
//
//   hipcc -x hip --offload-arch=gfx950 -O2 -std=c++17 -ffp-contract=off -o focal_cost_host tools/focal_cost_host.cpp
//   ./focal_cost_host pairs.bin cost.bin
// pairs.bin: int32 n_pairs, n_cams, n_cand; int32 pair_cam (n_pairs); float64 F (n_pairs, 9), w (n_pairs), cams (n_cams, 4),
// ratios (n_cand).  cost.bin: float64 out_cost (n_cams, n_cand), out_weight (n_cams).
#include "../vit_colmap_amd/csrc/focal.hip"
#include "host_io.h"

int main(int argc, char** argv) {
  std::FILE* in = open_input(argc, argv, "pairs.bin cost.bin");
  if (!in) return 2;
  int32_t head[3];
  if (std::fread(head, sizeof(int32_t), 3, in) != 3 || head[0] < 0 || head[1] < 0 || head[2] < 0) {
    std::fprintf(stderr, "%s: no header\n", argv[1]);
    return 2;
  }
  const int n_pairs = head[0], n_cams = head[1], n_cand = head[2];
  std::vector<int32_t> pair_cam(n_pairs);
  std::vector<double> F(9 * (size_t)n_pairs), w(n_pairs), cams(4 * (size_t)n_cams), ratios(n_cand);
  const bool ok = read_all(in, pair_cam) && read_all(in, F) && read_all(in, w) && read_all(in, cams) && read_all(in, ratios);
  std::fclose(in);
  if (!ok) {
    std::fprintf(stderr, "%s: shorter than its header says\n", argv[1]);
    return 2;
  }
  const size_t cells = (size_t)n_cams * (size_t)n_cand;
  std::vector<double> total(cells, 0.0), weight(n_cams, 0.0), part(cells), part_w(n_cams), out_cost(cells);
  long counted = 0;
  for (long long lo = 0; lo < n_pairs; lo += kFocalChunk) {
    std::fill(part.begin(), part.end(), 0.0);
    std::fill(part_w.begin(), part_w.end(), 0.0);
    for (long long p = lo; p < n_pairs && p < lo + kFocalChunk; ++p) {
      double a[9], wp;
      const int slot = focal_load_pair(F.data(), pair_cam.data(), w.data(), cams.data(), n_cams, p, a, wp);
      if (slot < 0) continue;
      ++counted;
      const double fx0 = cams[4 * (size_t)slot], fy0 = cams[4 * (size_t)slot + 1];
      for (int k = 0; k < n_cand; ++k) {
        const double r = ratios[k];
        const double term = focal_ratio_ok(r) ? wp * focal_pair_cost(a, r * fx0, r * fy0) : 0.0;
        part[(size_t)slot * n_cand + k] = part[(size_t)slot * n_cand + k] + term;
      }
      part_w[slot] = part_w[slot] + wp;
    }
    for (size_t i = 0; i < cells; ++i) total[i] = total[i] + part[i];
    for (int c = 0; c < n_cams; ++c) weight[c] = weight[c] + part_w[c];
  }
  for (int c = 0; c < n_cams; ++c)
    for (int k = 0; k < n_cand; ++k)
      out_cost[(size_t)c * n_cand + k] = focal_mean(total[(size_t)c * n_cand + k], weight[c], ratios[k]);
  std::FILE* out = open_output(argv[2]);
  if (!out) return 2;
  write_all(out, out_cost), write_all(out, weight);
  std::fclose(out);
  std::printf("%d pairs, %ld counted, %d cameras, %d candidates\n", n_pairs, counted, n_cams, n_cand);
  return 0;
}
