// Keypoint undistortion (gfx950): the pixel an ideal pinhole camera with the same K would see in place of a
// raw keypoint of a camera with known lens distortion, every keypoint of a call in one launch.  vc_undistort_points is what
// the matcher and the mapper put in front of the solvers when a camera carries a focal-length prior and a non-zero
// distortion (vit_colmap_amd/mapping/undistort.py).  Specification: tests/util_undistort.py.
//
// float64, one keypoint per lane, no LDS, no barrier.  The model is COLMAP's OPENCV one, (fx, fy, cx, cy, k1, k2, p1, p2);
// SIMPLE_RADIAL and RADIAL are its cases p1 = p2 = 0 (and k2 = 0).  Its inverse has no closed form: Newton's method on the
// normalised point from the distorted one, with the 2x2 Jacobian of the forward model solved by the adjugate, at most
// kUndistortSteps steps.  A keypoint beyond the fold of the model (where the Jacobian stops being positive definite: the
// forward map is no longer one to one) is invalid, not clamped.  The kernel is bandwidth-trivial: a few dozen flops per step
// and 28 bytes per keypoint, once per image, so it has no tuning; it exists on the device because its callers' data is there
// and because one rule on one side is what the verifier, P3P and the triangulation can be compared against.
// Every operation is a single float64 one in the order include/vitcolmap_hip.h states (-ffp-contract=off), there is no
// library call, so the host build of undistort_point (tools/undistort_host.cpp includes this file) and the device agree.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/vitcolmap_hip.h"
#include "common.h"

namespace {

constexpr int kUndistortBlock = 256;
constexpr int kUndistortSteps = 20;             // UNDISTORT_MAX_STEPS: a bound, not a tuned figure (12 were the most seen)
constexpr double kUndistortStop = 1e-24;        // UNDISTORT_STOP: the squared length of the last step, normalised units

// One keypoint (u, v) of the camera c = (fx, fy, cx, cy, k1, k2, p1, p2) -> the undistorted pixel; false (and NaN) where the
// iteration meets a Jacobian that is not positive definite or does not stop within kUndistortSteps steps.
__host__ __device__ __forceinline__ bool undistort_point(double u, double v, const double* c, double& out_u, double& out_v) {
  const double fx = c[0], fy = c[1], cx = c[2], cy = c[3], k1 = c[4], k2 = c[5], p1 = c[6], p2 = c[7];
  const double xd = (u - cx) / fx, yd = (v - cy) / fy;
  double x = xd, y = yd;
  bool valid = false;
  for (int it = 0; it < kUndistortSteps; ++it) {
    const double rho = x * x + y * y;
    const double s = 1.0 + k1 * rho + k2 * rho * rho;
    const double e = 2.0 * (k1 + 2.0 * k2 * rho);
    const double gx = x * s + 2.0 * p1 * x * y + p2 * (rho + 2.0 * x * x) - xd;
    const double gy = y * s + p1 * (rho + 2.0 * y * y) + 2.0 * p2 * x * y - yd;
    const double a = s + x * x * e + 2.0 * p1 * y + 6.0 * p2 * x;
    const double b = x * y * e + 2.0 * p1 * x + 2.0 * p2 * y;
    const double d = s + y * y * e + 6.0 * p1 * y + 2.0 * p2 * x;
    const double det = a * d - b * b;
    if (!(det > 0.0)) break;                                 // also for NaN
    const double sx = (d * gx - b * gy) / det, sy = (a * gy - b * gx) / det;
    x = x - sx;
    y = y - sy;
    if (sx * sx + sy * sy <= kUndistortStop) {
      valid = true;
      break;
    }
  }
  out_u = valid ? fx * x + cx : NAN;
  out_v = valid ? fy * y + cy : NAN;
  return valid;
}

// Sets *bad where a slot of the call is outside [0, n_cams); the entry point reads it before anything is written.
__global__ __launch_bounds__(kUndistortBlock) void undistort_check_slots_kernel(const int32_t* __restrict__ cam, int n, int n_cams,
                                                                                int* __restrict__ bad) {
  const long long i = (long long)blockIdx.x * kUndistortBlock + threadIdx.x;
  if (i >= n) return;
  const int slot = cam[i];
  if (slot < 0 || slot >= n_cams) atomicOr(bad, 1);
}

__global__ __launch_bounds__(kUndistortBlock) void undistort_points_kernel(const float* __restrict__ xy, const int32_t* __restrict__ cam,
                                                                           int n, const double* __restrict__ cams, int n_cams,
                                                                           double* __restrict__ out_xy, uint8_t* __restrict__ out_valid) {
  const long long i = (long long)blockIdx.x * kUndistortBlock + threadIdx.x;
  if (i >= n) return;
  const int slot = cam[i];
  double u = NAN, v = NAN;
  bool valid = false;
  if (slot >= 0 && slot < n_cams)                            // the entry point has checked it; nothing is read past the table
    valid = undistort_point((double)xy[2 * i], (double)xy[2 * i + 1], cams + (long long)slot * 8, u, v);
  out_xy[2 * i] = u, out_xy[2 * i + 1] = v;
  out_valid[i] = valid ? 1 : 0;
}

}  // namespace

extern "C" {

int vc_undistort_points(const float* xy, const int32_t* cam, int n, const double* cams, int n_cams, double* out_xy,
                        uint8_t* out_valid, vc_stream_t stream) {
  if (n < 0 || n_cams < 0) return VC_ERR_INVALID_ARG;
  if (n == 0) return VC_OK;
  if (!xy || !cam || !cams || !out_xy || !out_valid || n_cams == 0) return VC_ERR_INVALID_ARG;
  const hipStream_t s = (hipStream_t)stream;
  const int blocks = (n + kUndistortBlock - 1) / kUndistortBlock;
  // the slots are device data: one flag, checked on the host before the launch that writes (the one wait of this entry point)
  int* d_bad = nullptr;
  int bad = 0;
  hipError_t e = hipMallocAsync((void**)&d_bad, sizeof(int), s);
  if (e != hipSuccess) return vc::fail(e);
  e = hipMemsetAsync(d_bad, 0, sizeof(int), s);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(undistort_check_slots_kernel, dim3((unsigned)blocks), dim3(kUndistortBlock), 0, s, cam, n, n_cams, d_bad);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  const hipError_t freed = hipFreeAsync(d_bad, s);
  if (e != hipSuccess) return vc::fail(e);
  if (freed != hipSuccess) return vc::fail(freed);
  if (bad) return VC_ERR_INVALID_ARG;
  hipLaunchKernelGGL(undistort_points_kernel, dim3((unsigned)blocks), dim3(kUndistortBlock), 0, s, xy, cam, n, cams, n_cams, out_xy,
                     out_valid);
  return vc::check_launch();
}

}  // extern "C"
