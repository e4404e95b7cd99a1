// The keypoint undistortion of vit_colmap_amd/csrc/undistort.hip on the CPU: undistort_point is __host__ __device__, so this
// program includes the kernel source and calls it on one keypoint after another.  It is how the kernel's arithmetic is
// compared with the specification without a GPU (tests/test_undistort_spec.py; HOST_SPEC_REL of tests/util_undistort.py was
// measured with it), how it is run under a host sanitizer and where a fault in it is looked for with a host debugger.
// tools/triangulate_host.cpp is its counterpart for csrc/triangulate.hip.
//
//   hipcc -x hip --offload-arch=gfx950 -O2 -std=c++17 -ffp-contract=off -o undistort_host tools/undistort_host.cpp
//   ./undistort_host keypoints.bin undistorted.bin
// keypoints.bin: int32 n, n_cams; int32 cam (n); float32 xy (n, 2); float64 cams (n_cams, 8).  undistorted.bin: float64 xy
// (n, 2); uint8 valid (n).  A slot outside [0, n_cams) is refused, as the entry point refuses it.
#include "../vit_colmap_amd/csrc/undistort.hip"
#include "host_io.h"

int main(int argc, char** argv) {
  std::FILE* in = open_input(argc, argv, "keypoints.bin undistorted.bin");
  if (!in) return 2;
  int32_t head[2];
  if (std::fread(head, sizeof(int32_t), 2, in) != 2 || head[0] < 0 || head[1] < 0) {
    std::fprintf(stderr, "%s: no header\n", argv[1]);
    return 2;
  }
  const int n = head[0], n_cams = head[1];
  std::vector<int32_t> cam(n);
  std::vector<float> xy(2 * (size_t)n);
  std::vector<double> cams(8 * (size_t)n_cams);
  const bool ok = read_all(in, cam) && read_all(in, xy) && read_all(in, cams);
  std::fclose(in);
  if (!ok) {
    std::fprintf(stderr, "%s: shorter than its header says\n", argv[1]);
    return 2;
  }
  for (int i = 0; i < n; ++i) {
    if (cam[i] < 0 || cam[i] >= n_cams) {
      std::fprintf(stderr, "%s: keypoint %d has slot %d, outside [0, %d)\n", argv[1], i, cam[i], n_cams);
      return 2;
    }
  }
  std::vector<double> out(2 * (size_t)n);
  std::vector<uint8_t> valid(n);
  long inverted = 0;
  for (int i = 0; i < n; ++i) {
    valid[i] = undistort_point((double)xy[2 * (size_t)i], (double)xy[2 * (size_t)i + 1], cams.data() + 8 * (size_t)cam[i], out[2 * (size_t)i],
                               out[2 * (size_t)i + 1])
                   ? 1
                   : 0;
    inverted += valid[i];
  }
  std::FILE* f = open_output(argv[2]);
  if (!f) return 2;
  write_all(f, out), write_all(f, valid);
  std::fclose(f);
  std::printf("%d keypoints, %ld undistorted\n", n, inverted);
  return 0;
}
