"""CPU SPECIFICATION (test infrastructure, NOT product code) of keypoint undistortion: the forward model of
COLMAP's OPENCV camera (fx, fy, cx, cy, k1, k2, p1, p2; SIMPLE_RADIAL and RADIAL are its cases p1 = p2 = 0) and its inversion by
Newton's method, the rule of vc_undistort_points as include/vitcolmap_hip.h states it.  numpy only, vectorised over the keypoints:
every keypoint runs the same single float64 operations in the written order, one that has stopped or failed is frozen.

  start     xd = (u - cx) / fx, yd = (v - cy) / fy, (x, y) = (xd, yd)
  iterate   rho = x x + y y, s = 1 + k1 rho + k2 rho rho, e = 2 (k1 + 2 k2 rho)
            gx = x s + 2 p1 x y + p2 (rho + 2 x x) - xd, gy = y s + p1 (rho + 2 y y) + 2 p2 x y - yd
            a = s + x x e + 2 p1 y + 6 p2 x, b = x y e + 2 p1 x + 2 p2 y, d = s + y y e + 6 p1 y + 2 p2 x, det = a d - b b
            not det > 0 (NaN included): invalid
  step      sx = (d gx - b gy) / det, sy = (a gy - b gx) / det, subtracted; valid once sx sx + sy sy <= 1e-24, at most 20 steps
  output    (fx x + cx, fy y + cy), NaN and 0 where invalid
"""
import numpy as np

MAX_STEPS = 20
STOP = 1e-24
# the four parameter sets (k1, k2, p1, p2) of the round-trip tests and the one whose fold lies inside the image
PARAMETER_SETS = [(-0.15, 0.0, 0.0, 0.0), (-0.15, 0.05, 0.0, 0.0), (0.2, -0.05, 0.0, 0.0), (-0.2, 0.05, 1e-3, -2e-3)]
FOLD_K1 = -0.6
WIDTH, HEIGHT, FOCAL = 640, 480, 600.0
# worst relative difference max|host - spec| / max|spec| of the undistorted pixels between this specification and the kernel's
# per-keypoint routine compiled for the host (tools/undistort_host.cpp, -O2 -ffp-contract=off) over the five parameter sets on the
# grid and the random pixels and over 100 random cameras (measured by tests/test_undistort_spec.py, which prints it: 0, every
# coordinate equal to the bit and every `valid` equal, as the same operations in float64 without contraction should be).  The GPU
# test holds the kernel to the same: equal bits.
HOST_SPEC_REL = 0.0


def camera_row(k, f=FOCAL, width=WIDTH, height=HEIGHT):
    """(k1, k2, p1, p2) -> the eight numbers of the probe's camera: f = 600 on a 640 x 480 image, the centre as principal point."""
    return np.array([f, f, width / 2.0, height / 2.0, k[0], k[1], k[2], k[3]], np.float64)


def distort(xy, cam):
    """The forward model: ideal pinhole pixels (n, 2) -> the pixels the distorted camera `cam` (8,) sees."""
    xy, (fx, fy, cx, cy, k1, k2, p1, p2) = np.asarray(xy, np.float64).reshape(-1, 2), np.asarray(cam, np.float64)
    x, y = (xy[:, 0] - cx) / fx, (xy[:, 1] - cy) / fy
    rho = x * x + y * y
    s = 1.0 + k1 * rho + k2 * rho * rho
    xd = x * s + 2.0 * p1 * x * y + p2 * (rho + 2.0 * x * x)
    yd = y * s + p1 * (rho + 2.0 * y * y) + 2.0 * p2 * x * y
    return np.stack([fx * xd + cx, fy * yd + cy], axis=1)


def distort_normalised(x, y, cam):
    """The forward model on normalised points (for the derivative test)."""
    _, _, _, _, k1, k2, p1, p2 = np.asarray(cam, np.float64)
    rho = x * x + y * y
    s = 1.0 + k1 * rho + k2 * rho * rho
    return x * s + 2.0 * p1 * x * y + p2 * (rho + 2.0 * x * x), y * s + p1 * (rho + 2.0 * y * y) + 2.0 * p2 * x * y


def jacobian(x, y, cam):
    """(a, b, d) of the rule at the normalised point(s) (x, y): the symmetric Jacobian ((a, b), (b, d)) of the forward model."""
    _, _, _, _, k1, k2, p1, p2 = np.asarray(cam, np.float64)
    rho = x * x + y * y
    s = 1.0 + k1 * rho + k2 * rho * rho
    e = 2.0 * (k1 + 2.0 * k2 * rho)
    return s + x * x * e + 2.0 * p1 * y + 6.0 * p2 * x, x * y * e + 2.0 * p1 * x + 2.0 * p2 * y, s + y * y * e + 6.0 * p1 * y + 2.0 * p2 * x


def undistort(xy, cam, cams, steps_out=None):
    """The call of vc_undistort_points on numpy arrays: xy (n, 2) raw pixels (read as float32, as the kernel reads them), cam (n,)
    slots, cams (n_cams, 8) -> xy64 (n, 2) (NaN where invalid), valid bool (n,).  A slot out of range raises ValueError.
    `steps_out`: a list that receives the steps every keypoint took."""
    xy = np.asarray(xy, np.float32).reshape(-1, 2).astype(np.float64)
    cam, cams = np.asarray(cam, np.int64).reshape(-1), np.asarray(cams, np.float64).reshape(-1, 8)
    if len(cam) and (cam.min() < 0 or cam.max() >= len(cams)):
        raise ValueError("undistort: a slot outside [0, n_cams)")
    n = len(cam)
    if n == 0:
        return np.zeros((0, 2)), np.zeros(0, bool)
    fx, fy, cx, cy, k1, k2, p1, p2 = (cams[cam, i] for i in range(8))
    with np.errstate(all="ignore"):
        xd, yd = (xy[:, 0] - cx) / fx, (xy[:, 1] - cy) / fy
        x, y = xd.copy(), yd.copy()
        running, valid, steps = np.ones(n, bool), np.zeros(n, bool), np.zeros(n, np.int32)
        for _ in range(MAX_STEPS):
            rho = x * x + y * y
            s = 1.0 + k1 * rho + k2 * rho * rho
            e = 2.0 * (k1 + 2.0 * k2 * rho)
            gx = x * s + 2.0 * p1 * x * y + p2 * (rho + 2.0 * x * x) - xd
            gy = y * s + p1 * (rho + 2.0 * y * y) + 2.0 * p2 * x * y - yd
            a = s + x * x * e + 2.0 * p1 * y + 6.0 * p2 * x
            b = x * y * e + 2.0 * p1 * x + 2.0 * p2 * y
            d = s + y * y * e + 6.0 * p1 * y + 2.0 * p2 * x
            det = a * d - b * b
            running = running & (det > 0)                                           # False for NaN
            sx, sy = (d * gx - b * gy) / det, (a * gy - b * gx) / det
            x, y = np.where(running, x - sx, x), np.where(running, y - sy, y)
            steps = steps + running
            stopped = running & (sx * sx + sy * sy <= STOP)
            valid, running = valid | stopped, running & ~stopped
            if not running.any():
                break
        out = np.stack([fx * x + cx, fy * y + cy], axis=1)
    if steps_out is not None:
        steps_out.append(steps)
    return np.where(valid[:, None], out, np.nan), valid


def spec_undistort(xy, cam, cams, device=None):
    """`undistort` behind the product's `undistort_fn` seams."""
    return undistort(xy, cam, cams)


def probe_pixels(seed=0, n_random=2000, step=16):
    """The pixels of the tests on the 640 x 480 image: a grid every `step` px, the borders included, plus uniform random ones,
    float32 as a database holds keypoints."""
    gx, gy = np.meshgrid(np.arange(0, WIDTH + 1, step), np.arange(0, HEIGHT + 1, step))
    rs = np.random.RandomState(seed)
    rand = np.stack([rs.uniform(0, WIDTH, n_random), rs.uniform(0, HEIGHT, n_random)], axis=1)
    return np.concatenate([np.stack([gx.ravel(), gy.ravel()], axis=1), rand]).astype(np.float32)


def random_camera(i):
    """Camera i of the 100 random ones from RandomState(52000 + i): f in [400, 900] per axis, the principal point within 20 px of the
    centre, |k1| <= 0.2, |k2| <= 0.05, |p| <= 2e-3 -> (8,)."""
    rs = np.random.RandomState(52000 + i)
    return np.array([rs.uniform(400, 900), rs.uniform(400, 900), WIDTH / 2 + rs.uniform(-20, 20), HEIGHT / 2 + rs.uniform(-20, 20),
                     rs.uniform(-0.2, 0.2), rs.uniform(-0.05, 0.05), rs.uniform(-2e-3, 2e-3), rs.uniform(-2e-3, 2e-3)])


def fold_radius(k1):
    """k2 = p = 0, k1 < 0: the distorted radius r (1 + k1 r^2) grows until r^2 = 1 / (3 |k1|) and is there
    (2 / 3) sqrt(1 / (3 |k1|)); no point has a larger one, and the Newton iteration from a larger one meets det <= 0."""
    return (2.0 / 3.0) * np.sqrt(1.0 / (3.0 * abs(k1)))


# ---- the host program's files ------------------------------------------------------------------------------------------------------------
def write_keypoints_file(path, xy, cam, cams):
    """The input of tools/undistort_host.cpp."""
    xy, cam = np.ascontiguousarray(xy, np.float32).reshape(-1, 2), np.ascontiguousarray(cam, np.int32).reshape(-1)
    cams = np.ascontiguousarray(cams, np.float64).reshape(-1, 8)
    with open(path, "wb") as f:
        f.write(np.array([len(cam), len(cams)], np.int32).tobytes() + cam.tobytes() + xy.tobytes() + cams.tobytes())


def read_undistorted_file(path, n):
    raw = open(path, "rb").read()
    assert len(raw) == 17 * n
    return np.frombuffer(raw, np.float64, 2 * n).reshape(n, 2), np.frombuffer(raw, np.uint8, n, 16 * n).astype(bool)


def run_host(program, tmp_path, xy, cam, cams, name="keypoints"):
    import subprocess

    write_keypoints_file(tmp_path / f"{name}.bin", xy, cam, cams)
    done = subprocess.run([program, str(tmp_path / f"{name}.bin"), str(tmp_path / f"{name}_out.bin")], stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, text=True)
    assert done.returncode == 0, done.stderr
    return read_undistorted_file(tmp_path / f"{name}_out.bin", len(np.asarray(cam).reshape(-1))), done.stderr


def host_cases():
    """The calls the host build is compared on -> [(name, xy, cam, cams)]: the four parameter sets in one call over the probe's
    pixels, the fold camera, and the 100 random cameras on 200 random pixels each."""
    px = probe_pixels()
    cams4 = np.stack([camera_row(k) for k in PARAMETER_SETS])
    cases = [("sets", np.tile(px, (4, 1)), np.repeat(np.arange(4, dtype=np.int32), len(px)), cams4),
             ("fold", px, np.zeros(len(px), np.int32), camera_row((FOLD_K1, 0.0, 0.0, 0.0))[None])]
    rs = np.random.RandomState(7)
    xy = np.stack([rs.uniform(0, WIDTH, 100 * 200), rs.uniform(0, HEIGHT, 100 * 200)], axis=1).astype(np.float32)
    cases.append(("random", xy, np.repeat(np.arange(100, dtype=np.int32), 200), np.stack([random_camera(i) for i in range(100)])))
    return cases


def relative_difference(got, want):
    """max|got - want| / max|want| over the finite entries of `want`; NaN must sit where NaN sits."""
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    return float(np.abs(got[ok] - want[ok]).max() / np.abs(want[ok]).max()) if ok.any() else 0.0
