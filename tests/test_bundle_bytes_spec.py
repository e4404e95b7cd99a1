"""CPU test that pins the bytes of the bundle kernels' routines: the host build of csrc/bundle.hip
(tools/bundle_host.cpp) over five committed problems, one per instance of the passes and one more with groups, against the
SHA-256 of every array of result.bin, recorded once.  The routines use IEEE add, multiply, divide and sqrt in the written order
under -ffp-contract=off, so the digests are a property of the source, not of the optimisation level.  The GPU tests hold the
device's bytes to this host build's.  No GPU."""
import hashlib
import json
import os
import subprocess

import numpy as np

from test_bundle_spec import bundle_host  # noqa: F401 - the fixture

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bundle_bytes")
PROBLEMS = ("plain", "groups", "huber_groups", "radial_groups", "opencv_groups")


def problem_header(path):
    """-> n_cams, n_points, total, G, with_loss, marker (0: pinhole, 1: radial, 2: OPENCV) of a problem.bin."""
    raw = open(path, "rb").read()
    n_cams, n_points, total, G = (int(v) for v in np.frombuffer(raw, np.int32, 4))
    ints = (n_points + 1) + total + (n_cams + 1) + 2 * total + n_cams + (n_cams if G else 0) + G
    at = 16 + 8 + 4 * ints + 8 * (16 * n_cams + 3 * n_points + 2 * total + 6 * n_cams + 4 * G)
    with_loss = len(raw) > at
    marker = int(np.frombuffer(raw, np.int32, 1, at + 12)[0]) if len(raw) > at + 12 else 0
    return n_cams, n_points, total, G, with_loss, marker


def result_arrays(path, n_cams, n_points, total, G, with_loss, marker):
    """The named arrays of result.bin in file order, as the head of tools/bundle_host.cpp lists them -> [(name, bytes)]."""
    N, K, J = 4 + 2 * marker, 2 * marker, 2 + 4 * marker
    rows = 2 * N * G + N * N * (G + G * G)
    layout = [("vinv", 8, 6 * n_points), ("gp", 8, 3 * n_points), ("cost", 8, n_points), ("total_cost", 8, 1), ("S", 8, 36 * n_cams * n_cams),
              ("g", 8, 6 * n_cams), ("out_cams", 8, 16 * n_cams), ("out_points", 8, 3 * n_points), ("dx", 8, 3 * n_points),
              ("obs_lin", 8, 32 * total), ("count", 4, n_points), ("obs_ok", 1, total)]
    if G:
        layout += [("obs_jt", 8, J * total), ("T", 8, n_points * G * 3 * N), ("terms", 8, rows * n_points), ("sums", 8, rows),
                   ("B", 8, 6 * n_cams * N * G), ("C", 8, N * G * N * G), ("h", 8, N * G), ("border_out_cams", 8, 16 * n_cams),
                   ("border_out_points", 8, 3 * n_points), ("border_dx", 8, 3 * n_points), ("out_dist", 8, K * n_cams), ("free", 1, N * G),
                   ("valid", 1, n_cams)]
    layout.append(("obs_w", 8, total if with_loss else 0))
    raw = open(path, "rb").read()
    out, at = [], 0
    for name, size, count in layout:
        out.append((name, raw[at:at + size * count]))
        at += size * count
    assert at == len(raw), (at, len(raw))
    return out


def test_problem_files_are_small_and_cover_the_four_instances():
    seen = []
    for name in PROBLEMS:
        n_cams, n_points, total, G, with_loss, marker = problem_header(os.path.join(GOLDEN, name + ".bin"))
        assert 1 <= n_cams <= 6 and 1 <= n_points <= 24 and G <= 2 and total >= 2 * n_points, name
        seen.append((G > 0, with_loss, marker))
    assert seen == [(False, False, 0), (True, False, 0), (True, True, 0), (True, True, 1), (True, True, 2)]


def test_host_build_returns_the_recorded_bytes_of_every_array(bundle_host, tmp_path):  # noqa: F811
    want = json.load(open(os.path.join(GOLDEN, "digests.json")))
    assert sorted(want) == sorted(PROBLEMS)
    wrong = []
    for name in PROBLEMS:
        problem = os.path.join(GOLDEN, name + ".bin")
        done = subprocess.run([bundle_host, problem, str(tmp_path / "result.bin")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert done.returncode == 0, done.stderr
        arrays = result_arrays(tmp_path / "result.bin", *problem_header(problem))
        assert [k for k, _ in arrays] == list(want[name]), name
        # every problem has an unusable observation and a held parameter: an obs_ok of 0 and a zero column of J_c in obs_lin
        ok = np.frombuffer(dict(arrays)["obs_ok"], np.uint8)
        lin = np.frombuffer(dict(arrays)["obs_lin"], np.float64).reshape(-1, 32)
        assert (ok == 0).any() and (ok == 1).any() and ((lin[ok == 1][:, :6] == 0) & (lin[ok == 1][:, 6:12] == 0)).any(), name
        wrong += [f"{name}: {k}" for k, data in arrays if hashlib.sha256(data).hexdigest() != want[name][k]]
    assert not wrong, wrong
