// The track refinement of vit_colmap_amd/csrc/triangulate.hip (vc_refine_tracks) on the CPU: refine_track is
// __host__ __device__, so this program includes the kernel source and calls it on one track after another, as
// tools/triangulate_host.cpp does for triangulate_track.  It is how the kernel's arithmetic is compared with the
// specification without a GPU (tests/test_rounds_spec.py; HOST_SPEC_REFINE_X of tests/util_rounds.py was measured with it),
// how it is run under a host sanitizer and what the GPU test compares the kernel's bytes with.
//
//   hipcc -x hip --offload-arch=gfx950 -O2 -std=c++17 -ffp-contract=off -o refine_tracks_host tools/refine_tracks_host.cpp
//   ./refine_tracks_host tracks.bin points.bin
// tracks.bin: int32 n_tracks, n_cams, total; float64 max_error_px, min_tri_angle_tan2; int32 offsets (n_tracks + 1); float64
// init_xyz (n_tracks, 3); int32 obs_cam (total); float64 obs_xy (total, 2), cams (n_cams, 16).  points.bin: float64 xyz
// (n_tracks, 3), error (n_tracks); int32 count (n_tracks); uint8 mask (total).  Offsets that do not ascend from 0 to total are
// refused.
#include "../vit_colmap_amd/csrc/triangulate.hip"
#include "host_io.h"

int main(int argc, char** argv) {
  std::FILE* in = open_input(argc, argv, "tracks.bin points.bin");
  if (!in) return 2;
  int32_t head[3];
  double thr[2];
  if (std::fread(head, sizeof(int32_t), 3, in) != 3 || std::fread(thr, sizeof(double), 2, in) != 2 || head[0] < 0 || head[1] < 0 ||
      head[2] < 0) {
    std::fprintf(stderr, "%s: no header\n", argv[1]);
    return 2;
  }
  const int n_tracks = head[0], n_cams = head[1], total = head[2];
  std::vector<int32_t> offsets(n_tracks + 1), obs_cam(total);
  std::vector<double> init_xyz(3 * (size_t)n_tracks), obs_xy(2 * (size_t)total), cams(16 * (size_t)n_cams);
  const bool ok = read_all(in, offsets) && read_all(in, init_xyz) && read_all(in, obs_cam) && read_all(in, obs_xy) && read_all(in, cams);
  std::fclose(in);
  if (!ok) {
    std::fprintf(stderr, "%s: shorter than its header says\n", argv[1]);
    return 2;
  }
  bool ascending = offsets[0] == 0 && offsets[n_tracks] == total;
  for (int t = 0; t < n_tracks; ++t) ascending = ascending && offsets[t] <= offsets[t + 1];
  if (!ascending) {
    std::fprintf(stderr, "%s: the offsets do not ascend from 0 to %d\n", argv[1], total);
    return 2;
  }
  std::vector<double> xyz(3 * (size_t)n_tracks), error(n_tracks);
  std::vector<int32_t> count(n_tracks);
  std::vector<uint8_t> mask(total);
  const Tracks d{obs_xy.data(), obs_cam.data(), cams.data(), n_cams};
  long accepted = 0;
  for (int t = 0; t < n_tracks; ++t) {
    const double X0[3] = {init_xyz[3 * t], init_xyz[3 * t + 1], init_xyz[3 * t + 2]};
    double X[3];
    count[t] = refine_track(d, offsets[t], offsets[t + 1] - offsets[t], X0, thr[0], thr[1], X, mask.data() + offsets[t], error[t]);
    xyz[3 * t] = X[0], xyz[3 * t + 1] = X[1], xyz[3 * t + 2] = X[2];
    accepted += count[t] > 0;
  }
  std::FILE* out = open_output(argv[2]);
  if (!out) return 2;
  write_all(out, xyz), write_all(out, error), write_all(out, count), write_all(out, mask);
  std::fclose(out);
  std::printf("%d tracks, %ld accepted\n", n_tracks, accepted);
  return 0;
}
