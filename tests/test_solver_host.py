"""The two minimal solvers without a GPU: their solver functions are __host__ __device__, tools/five_point_host.cpp and
tools/p3p_host.cpp include the kernel sources and run them on the CPU, and here both programs are built and compared with
the numpy specifications on the 300 exact minimal problems of each, under the matching rule, the tolerances and the cap of the
GPU tests (test_essential_gpu.py, test_absolute_pose_gpu.py).  The library is built with -ffp-contract=off and the programs
are too, so what they compute is the kernels' arithmetic in the kernels' order."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import test_absolute_pose_gpu as tp
import test_essential_gpu as te
import util_essential as ue

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
PROGRAMS = ("five_point_host", "p3p_host")
_BUILT = {}


@pytest.fixture(scope="session")
def host_programs(tmp_path_factory):
    """Both programs, built side by side with the line their sources give -> {name: path}; built once however many test
    modules import the fixture (test_solver_families_host.py does)."""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc to build the host programs with")
    if _BUILT:
        return _BUILT
    out = tmp_path_factory.mktemp("solver_host")
    builds = {name: subprocess.Popen([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-o",
                                      str(out / name), os.path.join(ROOT, "tools", name + ".cpp")],
                                     stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for name in PROGRAMS}
    for name, proc in builds.items():
        log, _ = proc.communicate()
        assert proc.returncode == 0, f"{name} does not build:\n{log}"
    _BUILT.update({name: str(out / name) for name in PROGRAMS})
    return _BUILT


def run_program(path, records, out_width, tmp_path):
    """records float64 (n, w) -> the program's output float64 (n, 1 + out_width) with the count in front, NaN past it."""
    records = np.ascontiguousarray(records, np.float64)
    records.tofile(tmp_path / "in.bin")
    subprocess.run([path, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True, stdout=subprocess.DEVNULL)
    res = np.fromfile(tmp_path / "out.bin", np.float64).reshape(len(records), 1 + out_width)
    return res[:, 0].astype(int), res[:, 1:]


def test_five_point_host_matches_the_spec_on_the_300_minimal_problems(host_programs, tmp_path):
    pts, sols = te.minimal_problems()
    count, E = run_program(host_programs["five_point_host"], pts.reshape(300, 20), 90, tmp_path)
    assert np.all((count >= 0) & (count <= 10))
    E = E.reshape(300, 10, 3, 3)
    used = np.arange(10)[None, :] < count[:, None]
    assert np.isnan(E[~used]).all() and np.isfinite(E[used]).all()
    got = [E[i, : count[i]] for i in range(300)]
    bad, worst = te.compare_with_spec(got, sols)
    Et = ue.true_essential()
    spec_bad = [i for i in range(300) if min(ue.matrix_distance(Et, e) for e in sols[i]) > te.TOL]
    truth = max(min(ue.matrix_distance(Et, e) for e in got[i]) for i in range(300) if i not in bad)
    print(f"unmatched problems {bad}, worst matched distance {worst:.3g}, worst distance to the true E {truth:.3g}, "
          f"solutions per problem {sorted(set(count.tolist()))}")
    assert len(spec_bad) <= te.MAX_MISMATCHES                         # the specification alone stays within the cap
    assert len(bad) <= te.MAX_MISMATCHES
    assert truth <= te.TOL


def test_p3p_host_matches_the_spec_on_the_300_minimal_problems(host_programs, tmp_path):
    rays, xyz, sols = tp.minimal_problems()
    count, pose = run_program(host_programs["p3p_host"], np.concatenate([rays.reshape(300, 6), xyz.reshape(300, 9)], axis=1), 48,
                              tmp_path)
    assert np.all((count >= 0) & (count <= 4))
    pose = pose.reshape(300, 4, 12)
    used = np.arange(4)[None, :] < count[:, None]
    assert np.isnan(pose[~used]).all() and np.isfinite(pose[used]).all()
    got = [[(pose[i, j, :9].reshape(3, 3), pose[i, j, 9:]) for j in range(count[i])] for i in range(300)]
    bad, worst = tp.compare_with_spec(got, sols)
    spec_bad = [i for i in range(300) if tp.truth_distance(sols[i]) > tp.TOL_POSE]
    truth = max(tp.truth_distance(got[i]) for i in range(300) if i not in bad)
    print(f"unmatched problems {bad}, worst matched distance {worst:.3g}, worst distance to the true pose {truth:.3g}, "
          f"solutions per problem {sorted(set(count.tolist()))}")
    assert len(spec_bad) <= tp.MAX_MISMATCHES                         # the specification alone stays within the cap
    assert len(bad) <= tp.MAX_MISMATCHES
    assert truth <= tp.TOL_POSE
