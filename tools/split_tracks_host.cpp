// The track splitting of vit_colmap_amd/csrc/triangulate.hip (vc_split_tracks) on the CPU: split_component is
// __host__ __device__, so this program includes the kernel source and calls it on one component after another, as
// tools/triangulate_host.cpp does for triangulate_track.  It is how the kernel's arithmetic is compared with the
// specification without a GPU (tests/test_split_spec.py; HOST_SPEC_SPLIT_X of tests/util_split.py was measured with it), how
// it is run under a host sanitizer and what the GPU test compares the kernel's bytes with.
//
//   hipcc -x hip --offload-arch=gfx950 -O2 -std=c++17 -ffp-contract=off -o split_tracks_host tools/split_tracks_host.cpp
//   ./split_tracks_host components.bin points.bin
// components.bin: int32 n_comps, n_cams, total, max_points; float64 max_error_px, min_tri_angle_tan2; int32 offsets
// (n_comps + 1), seeds (n_comps), obs_cam (total); float64 obs_xy (total, 2), cams (n_cams, 16); int32 node_point (total);
// float64 points_xyz (n_comps, max_points, 3).  points.bin: float64 points_xyz (n_comps, max_points, 3), error (n_comps,
// max_points); int32 count (n_comps, max_points), node_point (total); uint8 new (n_comps, max_points).  A component whose
// offsets are negative or descend is rejected as the kernel rejects it; one whose offsets pass total, which the kernel is not
// told, is rejected here in the same way.
#include "../vit_colmap_amd/csrc/triangulate.hip"
#include "host_io.h"

int main(int argc, char** argv) {
  std::FILE* in = open_input(argc, argv, "components.bin points.bin");
  if (!in) return 2;
  int32_t head[4];
  double thr[2];
  if (std::fread(head, sizeof(int32_t), 4, in) != 4 || std::fread(thr, sizeof(double), 2, in) != 2 || head[0] < 0 || head[1] < 0 ||
      head[2] < 0 || head[3] < 1 || head[3] > VC_SPLIT_MAX_POINTS) {
    std::fprintf(stderr, "%s: no header\n", argv[1]);
    return 2;
  }
  const int n_comps = head[0], n_cams = head[1], total = head[2], max_points = head[3];
  const size_t n_slots = (size_t)n_comps * max_points;
  std::vector<int32_t> offsets(n_comps + 1), seeds(n_comps), obs_cam(total), node_point(total);
  std::vector<double> obs_xy(2 * (size_t)total), cams(16 * (size_t)n_cams), points_xyz(3 * n_slots);
  const bool ok = read_all(in, offsets) && read_all(in, seeds) && read_all(in, obs_cam) && read_all(in, obs_xy) && read_all(in, cams) &&
                  read_all(in, node_point) && read_all(in, points_xyz);
  std::fclose(in);
  if (!ok) {
    std::fprintf(stderr, "%s: shorter than its header says\n", argv[1]);
    return 2;
  }
  std::vector<double> error(n_slots);
  std::vector<int32_t> count(n_slots);
  std::vector<uint8_t> made(n_slots);
  const Tracks d{obs_xy.data(), obs_cam.data(), cams.data(), n_cams};
  long created = 0;
  for (int t = 0; t < n_comps; ++t) {
    const long long lo = offsets[t], hi = offsets[t + 1];
    split_or_reject(d, t, lo <= total && hi <= total ? lo : -1, hi, (uint32_t)seeds[t], max_points, thr[0], thr[1], node_point.data(),
                    points_xyz.data(), count.data(), made.data(), error.data());
    for (int k = 0; k < max_points; ++k) created += made[(size_t)t * max_points + k];
  }
  std::FILE* out = open_output(argv[2]);
  if (!out) return 2;
  write_all(out, points_xyz), write_all(out, error), write_all(out, count), write_all(out, node_point), write_all(out, made);
  std::fclose(out);
  std::printf("%d components, %ld points created\n", n_comps, created);
  return 0;
}
