"""The two minimal solvers on the named families of tests/util_solver_families.py, without a GPU: the kernels' solver functions
compiled for the host (test_solver_host.py's programs, -O2 -ffp-contract=off: the kernels' arithmetic in the kernels' order).
A forward family is matched with the numpy specification under util_solver.compare_with_spec and has to hold the true motion;
every family's solutions are checked backwards against the equations they solve.  The bounds are multiples of what the
SPECIFICATION's own solutions show (the constants of util_solver_families.py), never of the solver's."""
import numpy as np
import pytest

import test_essential_gpu as te
import util_absolute_pose as ua
import util_essential as ue
import util_solver
import util_solver_families as uf
from test_solver_host import host_programs, run_program  # noqa: F401  (host_programs is a fixture)

DISTINCT = 1e-9               # two solutions of one problem closer than this are one solution returned twice


def check_five_point_family(fam, got):
    """got: one (count, 3, 3) array per problem.  The assertions the host test and the GPU test share -> a line for the log."""
    spec = uf.five_point_spec(fam.name)
    assert all(np.isfinite(S).all() for S in got)
    if not fam.t.any():                                                # pure rotation: E = 0, any count, finite solutions only
        return f"{fam.name}: solutions per problem {sorted(set(len(S) for S in got))}"
    bound = uf.MARGIN * np.array(uf.FIVE_POINT_SPEC_RESIDUALS[fam.name])
    spec_res, res = uf.worst_essential_residuals(fam, spec), uf.worst_essential_residuals(fam, got)
    line = f"{fam.name}: residuals {res} (specification {spec_res}, bound {bound})"
    assert (spec_res <= bound).all(), line                             # the recorded constants still describe the specification
    assert (res <= bound).all(), line
    for i, S in enumerate(got):
        for a in range(len(S)):
            for b in range(a):
                assert ue.matrix_distance(S[a], S[b]) > DISTINCT, f"{fam.name}: problem {i} returns a solution twice"
    if fam.cls != uf.FORWARD:
        return line
    Et = uf.true_essential(fam)
    bad, worst = util_solver.compare_with_spec(got, spec, ue.matrix_distance, te.TOL)
    spec_bad = [i for i, S in enumerate(spec) if min([ue.matrix_distance(Et, e) for e in S] + [9.0]) > te.TOL]
    truth = [min([ue.matrix_distance(Et, e) for e in S] + [9.0]) for S in got]
    lost = [i for i, d in enumerate(truth) if d > te.TOL and i not in bad]
    line += (f"; unmatched {bad}, worst matched distance {worst:.3g}, truth missed in {len([d for d in truth if d > te.TOL])}, worst "
             f"distance to the true E {max([d for d in truth if d <= te.TOL] + [0.0]):.3g}")
    assert len(spec_bad) <= uf.cap(len(got)), line                     # the specification alone stays within the cap
    assert len(bad) <= uf.cap(len(got)), line
    assert not lost, line
    return line


def check_p3p_family(fam, got):
    """got: one list of (R, t) per problem."""
    spec = uf.p3p_spec(fam.name)
    _, _, det_spec, angle_spec = uf.P3P_MEASURED[fam.name]
    spec_res, res = uf.worst_pose_residuals(fam, spec), uf.worst_pose_residuals(fam, got)
    line = f"{fam.name}: |det R - 1|, smallest depth ratio, worst angle {res} (specification {spec_res})"
    for r in (spec_res, res):
        assert r[0] <= uf.MARGIN * det_spec and r[1] > 0 and r[2] <= uf.MARGIN * angle_spec, line
    for i, S in enumerate(got):
        for a in range(len(S)):
            for b in range(a):
                assert ua.pose_distance(*S[a], *S[b]) > DISTINCT, f"{fam.name}: problem {i} returns a pose twice"
    if fam.cls != uf.FORWARD:
        return line
    tol = uf.p3p_tolerance(fam.name)
    bad, worst = util_solver.compare_with_spec(got, spec, lambda a, b: ua.pose_distance(*a, *b), tol)
    spec_bad = [i for i, S in enumerate(spec) if uf.truth_distance(fam, S) > tol]
    truth = [uf.truth_distance(fam, S) for S in got]
    lost = [i for i, d in enumerate(truth) if d > tol and i not in bad]
    line += (f"; tolerance {tol:.3g}, unmatched {bad}, worst matched distance {worst:.3g}, truth missed in "
             f"{len([d for d in truth if d > tol])}, worst distance to the true pose {max([d for d in truth if d <= tol] + [0.0]):.3g}")
    assert len(spec_bad) <= uf.cap(len(got)), line                     # the specification alone stays within the cap
    assert len(bad) <= uf.cap(len(got)), line
    assert not lost, line
    return line


@pytest.mark.parametrize("fam", uf.five_point_families(), ids=repr)
def test_five_point_host_on_the_family(fam, host_programs, tmp_path):
    n = len(fam.pts)
    count, E = run_program(host_programs["five_point_host"], fam.pts.reshape(n, 20), 90, tmp_path)
    assert np.all((count >= 0) & (count <= 10))
    E = E.reshape(n, 10, 3, 3)
    used = np.arange(10)[None, :] < count[:, None]
    assert np.isnan(E[~used]).all() and np.isfinite(E[used]).all()
    print(check_five_point_family(fam, [E[i, : count[i]] for i in range(n)]))


@pytest.mark.parametrize("fam", uf.p3p_families(), ids=repr)
def test_p3p_host_on_the_family(fam, host_programs, tmp_path):
    n = len(fam.rays)
    count, pose = run_program(host_programs["p3p_host"], np.concatenate([fam.rays.reshape(n, 6), fam.xyz.reshape(n, 9)], axis=1), 48,
                              tmp_path)
    assert np.all((count >= 0) & (count <= 4))
    pose = pose.reshape(n, 4, 12)
    used = np.arange(4)[None, :] < count[:, None]
    assert np.isnan(pose[~used]).all() and np.isfinite(pose[used]).all()
    print(check_p3p_family(fam, [[(pose[i, j, :9].reshape(3, 3), pose[i, j, 9:]) for j in range(count[i])] for i in range(n)]))
