"""GPU tests of the two minimal solvers on the named families of tests/util_solver_families.py: vc_essential_5pt and vc_p3p
through the ABI, every family in ONE launch per solver (one hypothesis per minimal problem, the problems' correspondence lists
of different lengths so that `offsets` matters), and one family each again as a single list with n_hyp = 65.  The assertions
are those of test_solver_families_host.py; run_kernel and run_p3p pre-fill the outputs."""
from functools import lru_cache

import numpy as np
import pytest

import test_absolute_pose_gpu as tp
import test_essential_gpu as te
import util_solver_families as uf
from test_solver_families_host import check_five_point_family, check_p3p_family

pytestmark = pytest.mark.gpu

N_HYP_AGAIN = 65              # one more than a wave


def ragged(rows_per_problem, width):
    """Problems of k correspondences each, problem i followed by i % 3 rows nothing samples (NaN) -> offsets, the row of each
    problem's first correspondence, the number of rows.  A problem's list is its k rows and the filler behind them."""
    counts = np.array([rows_per_problem + i % 3 for i in range(width)])
    offsets = np.concatenate([[0], np.cumsum(counts)])
    return offsets, offsets[:-1], int(offsets[-1])


@lru_cache(maxsize=None)
def five_point_launch():
    """-> {family name: list of (count, 3, 3)} from one launch over every family."""
    fams = uf.five_point_families()
    pts = np.concatenate([f.pts for f in fams])                          # (P, 5, 4)
    offsets, first, total = ragged(5, len(pts))
    rows = np.full((total, 4), np.nan)
    for k in range(5):
        rows[first + k] = pts[:, k]
    E, count = te.run_kernel(rows, offsets, np.tile(np.arange(5), (len(pts), 1, 1)))
    out, at = {}, 0
    for f in fams:
        out[f.name] = [E[at + i, 0, : count[at + i, 0]] for i in range(len(f.pts))]
        at += len(f.pts)
    return out


@lru_cache(maxsize=None)
def p3p_launch():
    fams = uf.p3p_families()
    rays, xyz = np.concatenate([f.rays for f in fams]), np.concatenate([f.xyz for f in fams])     # (P, 3, 2), (P, 3, 3)
    offsets, first, total = ragged(3, len(rays))
    r, X = np.full((total, 2), np.nan), np.full((total, 3), np.nan)
    for k in range(3):
        r[first + k], X[first + k] = rays[:, k], xyz[:, k]
    sets, _, _ = tp.run_p3p(r, X, offsets, np.tile(np.arange(3), (len(rays), 1, 1)))
    out, at = {}, 0
    for f in fams:
        out[f.name] = [sets[at + i][0] for i in range(len(f.rays))]
        at += len(f.rays)
    return out


@pytest.mark.parametrize("fam", uf.five_point_families(), ids=repr)
def test_five_point_kernel_on_the_family(fam):
    print(check_five_point_family(fam, five_point_launch()[fam.name]))


@pytest.mark.parametrize("fam", uf.p3p_families(), ids=repr)
def test_p3p_kernel_on_the_family(fam):
    print(check_p3p_family(fam, p3p_launch()[fam.name]))


def test_five_point_kernel_on_one_family_as_65_hypotheses_of_one_pair():
    """The sideways translation (the family the specification used to fail on) as one pair of 500 correspondences: hypothesis k
    samples minimal problem k, in an order of its own."""
    fam = next(f for f in uf.five_point_families() if f.name == "sideways translation")
    rs = np.random.RandomState(65)
    samples = np.stack([5 * k + rs.permutation(5) for k in range(N_HYP_AGAIN)])[None]
    E, count = te.run_kernel(fam.pts.reshape(-1, 4), [0, 5 * len(fam.pts)], samples)
    got = [E[0, k, : count[0, k]] for k in range(N_HYP_AGAIN)]
    truth = [min([te.ue.matrix_distance(uf.true_essential(fam), e) for e in S] + [9.0]) for S in got]
    bad, worst = te.compare_with_spec(got, uf.five_point_spec(fam.name)[:N_HYP_AGAIN])
    print(f"unmatched {bad}, worst matched distance {worst:.3g}, worst distance to the true E {max(truth):.3g}")
    assert len(bad) <= uf.cap(N_HYP_AGAIN)
    assert all(d <= te.TOL for i, d in enumerate(truth) if i not in bad)


def test_p3p_kernel_on_one_family_as_65_hypotheses_of_one_problem():
    """The exactly perpendicular ray (every lane relabels its points) as one problem of 300 correspondences."""
    name = "perpendicular ray eps=0"
    fam = next(f for f in uf.p3p_families() if f.name == name)
    samples = np.stack([3 * k + np.arange(3) for k in range(N_HYP_AGAIN)])[None]
    sets, _, _ = tp.run_p3p(fam.rays.reshape(-1, 2), fam.xyz.reshape(-1, 3), [0, 3 * len(fam.rays)], samples)
    got = sets[0]
    tol = uf.p3p_tolerance(name)
    bad, worst = tp.util_solver.compare_with_spec(got, uf.p3p_spec(name)[:N_HYP_AGAIN], lambda a, b: tp.ua.pose_distance(*a, *b), tol)
    truth = [uf.truth_distance(fam, S) for S in got]
    print(f"unmatched {bad}, worst matched distance {worst:.3g}, worst distance to the true pose {max(truth):.3g}")
    assert len(bad) <= uf.cap(N_HYP_AGAIN)
    assert all(d <= tol for i, d in enumerate(truth) if i not in bad)
