"""What the tests of the two minimal solvers share (test_essential_gpu.py, test_absolute_pose_gpu.py, test_solver_host.py):
the rule by which a solver's solution sets are matched with the specification's."""
import numpy as np


def compare_with_spec(device_sets, spec_sets, distance, tol):
    """One set of solutions per problem from the solver and from the specification; a problem matches when both sets are
    non-empty and every solution of either has one of the other within `tol` under `distance(a, b)`; a problem both leave
    empty is neither.  -> (problems with an unmatched solution, worst matched distance)."""
    bad, worst = [], 0.0
    for i, (D, S) in enumerate(zip(device_sets, spec_sets)):
        d = np.array([[distance(a, b) for b in S] for a in D]).reshape(len(D), len(S))
        ok = len(D) > 0 and len(S) > 0 and d.min(axis=1).max() <= tol and d.min(axis=0).max() <= tol
        if ok:
            worst = max(worst, d.min(axis=1).max(), d.min(axis=0).max())
        elif len(D) or len(S):
            bad.append(i)
    return bad, worst
