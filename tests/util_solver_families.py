"""Named families of exact minimal problems for the two minimal solvers (test infrastructure, NOT product code): the 300
problems of util_essential.py and util_absolute_pose.py share one motion and one point box, and minimal solvers fail at
particular geometries.  Each family is a motion, a generator of camera-frame points, a problem count and a class:
  forward        the solver is matched with the specification and has to hold the true motion
  backward-only  ill-conditioned by construction (both the solver and the specification lose the truth): each returned
                 solution is only checked against the equations it has to satisfy
numpy only, deterministic from the seed.  test_solver_families_host.py runs them through the kernels' solver functions
compiled for the host, test_solver_families_gpu.py through the ABI.

The constants at the end are measured on the CPU from the SPECIFICATION's solutions and from the host build, never from the
GPU (`python tests/util_solver_families.py` prints them again).
"""
import math
from functools import lru_cache

import numpy as np

import util_absolute_pose as ua
import util_essential as ue

FORWARD, BACKWARD_ONLY = "forward", "backward-only"
PER_HUNDRED = 1               # problems per 100 of a family in which a solution may be unmatched, either way (3 in 300 today)


def cap(n):
    """The unmatched problems a family of n may have: 1 per started hundred."""
    return PER_HUNDRED * math.ceil(n / 100)


def rot(axis, angle):
    """Rodrigues: the rotation by `angle` about `axis`."""
    a = np.asarray(axis, np.float64)
    W = ue.skew(a / np.linalg.norm(a))
    return np.eye(3) + np.sin(angle) * W + (1 - np.cos(angle)) * (W @ W)


X_AXIS, Y_AXIS, Z_AXIS = (1.0, 0, 0), (0, 1.0, 0), (0, 0, 1.0)


def box(rs, n, x=3.0, y=2.0, z=(4.0, 9.0)):
    return np.stack([rs.uniform(-x, x, n), rs.uniform(-y, y, n), rs.uniform(z[0], z[1], n)], axis=1)


class Family:
    """name, cls, R, t (the truth; t = 0: none), problems: five-point (n, 5, 4) rows x1 y1 x2 y2, P3P (n, 3, 2) and (n, 3, 3)."""

    def __init__(self, name, cls, R, t, **arrays):
        self.name, self.cls, self.R, self.t = name, cls, np.asarray(R, np.float64), np.asarray(t, np.float64)
        self.__dict__.update(arrays)

    def __repr__(self):
        return self.name


# ---- five-point ---------------------------------------------------------------------------------------------------------------------
def _five(name, cls, R, t, seed, n=100, points=box, surface=None):
    """n problems of five points each; a point whose depth in the second camera is below 0.5 in magnitude is drawn again (its
    image point would be a quotient by almost nothing; the sign of the depth does not matter to E)."""
    rs = np.random.RandomState(seed)
    R, t = np.asarray(R, np.float64), np.asarray(t, np.float64)
    pts = np.zeros((n, 5, 4))
    for i in range(n):
        for k in range(5):
            while True:
                X = points(rs, 1)[0]
                if surface is not None:
                    X[2] = surface(X[0], X[1])
                X2 = R @ X + t
                if abs(X2[2]) >= 0.5:
                    break
            pts[i, k] = [X[0] / X[2], X[1] / X[2], X2[0] / X2[2], X2[1] / X2[2]]
    return Family(name, cls, R, t, pts=pts)


@lru_cache(maxsize=None)
def five_point_families():
    S_R, S_T = ue.SCENE_R, ue.SCENE_T
    fams = [
        _five("forward motion", FORWARD, rot(Y_AXIS, 0.05), (0.02, 0.01, 1.0), 1),
        _five("sideways translation", FORWARD, np.eye(3), (1.0, 0, 0), 2),
        _five("forward translation", FORWARD, np.eye(3), (0, 0, 1.0), 3),
        _five("roll 90", FORWARD, rot(Z_AXIS, np.pi / 2), (0.5, 0.2, 0.1), 4),
        _five("roll 180", FORWARD, rot(Z_AXIS, np.pi), (0.5, 0.2, 0.1), 5),
        _five("yaw 60", FORWARD, rot(Y_AXIS, 1.05), (-3.0, 0, 1.5), 6),
        _five("coplanar", FORWARD, S_R, S_T, 7, surface=lambda x, y: 6.0),
        _five("tilted plane", FORWARD, S_R, S_T, 8, surface=lambda x, y: 6.0 + 0.3 * x - 0.2 * y),
        _five("telephoto", FORWARD, rot(Y_AXIS, 0.002), S_T, 9, points=lambda rs, n: box(rs, n, 1.0, 1.0, (100.0, 140.0))),
        _five("wide angle", FORWARD, S_R, S_T, 10, points=lambda rs, n: box(rs, n, 9.0, 9.0, (3.0, 5.0))),
    ]
    rs = np.random.RandomState(11)
    for k in range(4):
        axis, angle, t = rs.normal(size=3), rs.uniform(0.2, 3.0), rs.normal(size=3)
        fams.append(_five(f"random motion {k}", FORWARD, rot(axis, angle), t, 12 + k, n=60,
                          points=lambda rs, n: box(rs, n, z=(8.0, 14.0))))
    small = rot((1.0, 2, 3), 0.1)
    fams += [
        _five("small baseline 1e-3", BACKWARD_ONLY, small, 1e-3 * np.array([1.0, 0.2, -0.3]), 20),
        _five("small baseline 1e-5", BACKWARD_ONLY, small, 1e-5 * np.array([1.0, 0.2, -0.3]), 21),
        _five("pure rotation", BACKWARD_ONLY, small, np.zeros(3), 22),
    ]
    return fams


def true_essential(fam):
    E = ue.skew(fam.t) @ fam.R
    return E / np.linalg.norm(E)


def essential_residuals(E, pts):
    """One solution against its problem (5, 4) -> (| |E|_F - 1 |, max |x2' E x1|, max |2 E E' E - tr(E E') E| and |det E|)."""
    h1 = np.concatenate([pts[:, :2], np.ones((5, 1))], axis=1)
    h2 = np.concatenate([pts[:, 2:], np.ones((5, 1))], axis=1)
    EEt = E @ E.T
    cubic = 2 * EEt @ E - np.trace(EEt) * E
    return (abs(np.linalg.norm(E) - 1), float(np.abs(np.einsum("ki,ij,kj->k", h2, E, h1)).max()),
            float(max(np.abs(cubic).max(), abs(np.linalg.det(E)))))


# ---- P3P ---------------------------------------------------------------------------------------------------------------------------
P3P_R, P3P_T = rot((1.0, 2, 3), 0.7), np.array([0.3, -0.2, 0.5])


def p3p_box(rs, n):
    return box(rs, n, 1.5, 1.0, (2.0, 6.0))


def _p3p(name, cls, Xc, R=P3P_R, t=P3P_T):
    """Camera-frame triangles Xc (n, 3, 3) under the pose (R, t): X_cam = R X + t."""
    Xc = np.asarray(Xc, np.float64)
    return Family(name, cls, R, t, rays=Xc[:, :, :2] / Xc[:, :, 2:], xyz=(Xc - t) @ R)       # rows R' (Xc - t)


def _perpendicular(rs, eps):
    """Third viewing ray perpendicular to the side Xc2 - Xc1, plus eps times the side's direction."""
    while True:
        a, b, c = p3p_box(rs, 3)
        e = (b - a) / np.linalg.norm(b - a)
        ray = c - (c @ e) * e
        ray = ray / np.linalg.norm(ray) + eps * e
        if ray[2] > 0.5 and abs(np.linalg.norm(a) - np.linalg.norm(b)) >= 0.3:
            return np.stack([a, b, ray * (rs.uniform(2, 6) / ray[2])])


def _seam(rs):
    """The first two points equally far from the camera centre: u = s2 / s1 = 1."""
    a, b, c = p3p_box(rs, 3)
    return np.stack([a, b * (np.linalg.norm(a) / np.linalg.norm(b)), c])


def _isosceles(rs, eps):
    """An isosceles triangle seen from (eps off) its symmetry plane."""
    w, z, h, z2 = rs.uniform(0.5, 1.5), rs.uniform(2, 6), rs.uniform(0.3, 1.0) * rs.choice([-1.0, 1.0]), rs.uniform(2, 6)
    return np.array([[-w, 0, z], [w, 0, z], [eps, h, z2]])


def _depth_ratio(rs):
    a, b, c = p3p_box(rs, 3)
    return np.stack([a, b * (50.0 * a[2] / b[2]), c])


def _small_triangle(rs):
    centre = np.array([rs.uniform(-1.5, 1.5), rs.uniform(-1, 1), 4.0])
    d = rs.normal(size=(3, 3))
    return centre + 1e-3 * d / np.linalg.norm(d, axis=1, keepdims=True)


def _draw(seed, n, one):
    rs = np.random.RandomState(seed)
    return np.stack([one(rs) for _ in range(n)])


@lru_cache(maxsize=None)
def p3p_families():
    fams = [
        _p3p("default pose", FORWARD, _draw(100, 100, lambda rs: p3p_box(rs, 3))),
        _p3p("identity pose", FORWARD, _draw(101, 100, lambda rs: p3p_box(rs, 3)), np.eye(3), np.zeros(3)),
        _p3p("170 about x", FORWARD, _draw(102, 100, lambda rs: p3p_box(rs, 3)), rot(X_AXIS, 2.97), np.array([1.0, 2, 3])),
        _p3p("depth ratio 50", FORWARD, _draw(103, 100, _depth_ratio)),
        _p3p("far points", FORWARD, _draw(104, 100, lambda rs: box(rs, 3, 300.0, 200.0, (800.0, 1200.0)))),
    ]
    for k, eps in enumerate((0.0, 1e-9, 1e-6, 1e-4)):
        fams.append(_p3p(f"perpendicular ray eps={eps:g}", FORWARD, _draw(110 + k, 100, lambda rs: _perpendicular(rs, eps))))
    fams.append(_p3p("seam", FORWARD, _draw(120, 400, _seam)))
    for k, eps in enumerate((0.0, 1e-6, 1e-3)):
        fams.append(_p3p(f"isosceles eps={eps:g}", FORWARD, _draw(130 + k, 100, lambda rs: _isosceles(rs, eps))))
    fams.append(_p3p("small triangle", BACKWARD_ONLY, _draw(140, 100, _small_triangle)))
    return fams


def pose_residuals(R, t, rays, xyz):
    """One pose against its problem -> (|det R - 1|, the smallest depth over the largest, the largest angle between R X_i + t
    and ray i)."""
    Xc = xyz @ R.T + t
    f = np.concatenate([rays, np.ones((3, 1))], axis=1)
    f = f / np.linalg.norm(f, axis=1, keepdims=True)
    depth = (Xc * f).sum(axis=1)
    angle = np.arctan2(np.linalg.norm(np.cross(Xc, f), axis=1), depth)
    return abs(np.linalg.det(R) - 1), float(depth.min() / np.abs(depth).max()), float(angle.max())


def truth_distance(fam, sols):
    return min([ua.pose_distance(R, t, fam.R, fam.t) for R, t in sols] + [9.0])


# ---- the specification's solutions, once per session -----------------------------------------------------------------------------
@lru_cache(maxsize=None)
def five_point_spec(name):
    fam = next(f for f in five_point_families() if f.name == name)
    return [ue.five_point(p[:, :2], p[:, 2:]) for p in fam.pts]


@lru_cache(maxsize=None)
def p3p_spec(name):
    fam = next(f for f in p3p_families() if f.name == name)
    return [ua.p3p(x, X) for x, X in zip(fam.rays, fam.xyz)]


def worst_essential_residuals(fam, sets):
    """-> the three worst residuals over every solution of every problem (zeros when there is none)."""
    r = [essential_residuals(E, p) for p, S in zip(fam.pts, sets) for E in S]
    return np.max(np.array(r).reshape(-1, 3), axis=0, initial=0.0)


def worst_pose_residuals(fam, sets):
    """-> (worst |det R - 1|, smallest depth ratio, worst angle) over every pose of every problem."""
    r = np.array([pose_residuals(R, t, x, X) for x, X, S in zip(fam.rays, fam.xyz, sets) for R, t in S]).reshape(-1, 3)
    if not len(r):
        return np.array([0.0, 1.0, 0.0])
    return np.array([r[:, 0].max(), r[:, 1].min(), r[:, 2].max()])


# ---- measured constants -----------------------------------------------------------------------------------------------------------
MARGIN = 4                    # what a solver may exceed a measured constant by: libm, instruction selection, another route
# five-point, per family: the worst (| |E| - 1 |, |x2' E x1|, ten-constraint residual) over the SPECIFICATION's solutions
# (measured on the CPU); a solver's solutions may show MARGIN times as much.
FIVE_POINT_SPEC_RESIDUALS = {
    "forward motion": (2.3e-16, 3.5e-16, 6.7e-16),
    "sideways translation": (3.4e-16, 4.6e-16, 6.7e-16),
    "forward translation": (2.3e-16, 3.2e-16, 6.7e-16),
    "roll 90": (3.4e-16, 4.1e-16, 5.6e-16),
    "roll 180": (2.3e-16, 3.4e-16, 6.7e-16),
    "yaw 60": (2.3e-16, 6.9e-16, 7.8e-16),
    "coplanar": (3.4e-16, 5.0e-16, 6.7e-16),
    "tilted plane": (3.4e-16, 3.4e-16, 6.7e-16),
    "telephoto": (3.4e-16, 4.5e-16, 6.7e-16),
    "wide angle": (2.3e-16, 3.4e-15, 7.8e-16),
    "random motion 0": (2.3e-16, 3.1e-16, 5.6e-16),
    "random motion 1": (2.3e-16, 2.5e-15, 4.5e-16),
    "random motion 2": (2.3e-16, 3.7e-16, 6.7e-16),
    "random motion 3": (2.3e-16, 4.4e-16, 7.8e-16),
    "small baseline 1e-3": (3.4e-16, 4.6e-16, 3.0e-2),      # the polish stalls: the cubics are nearly dependent
    "small baseline 1e-5": (3.4e-16, 3.3e-16, 9.2e-4),
    "pure rotation": (0.0, 0.0, 0.0),                       # the specification returns nothing: finite solutions, any count
}
# P3P, per family: (worst distance of the specification's nearest solution to the true pose; worst matched distance between the
# specification and the kernel's solver functions compiled for the host, tools/p3p_host.cpp; worst |det R - 1| and worst angle
# between R X_i + t and ray i over the SPECIFICATION's solutions), all measured on the CPU.  The match tolerance of a family
# is MARGIN times the larger of the first two, the convention of util_absolute_pose.TOL_POSE.
P3P_MEASURED = {
    "default pose": (6.8e-12, 3.1e-12, 2.3e-15, 1.5e-14),
    "identity pose": (6.4e-12, 1.1e-11, 1.9e-15, 4.2e-15),
    "170 about x": (4.8e-13, 2.6e-12, 1.8e-15, 1.8e-13),
    "depth ratio 50": (6.5e-11, 8.7e-11, 1.6e-15, 3.2e-12),
    "far points": (1.2e-9, 1.5e-9, 1.8e-15, 4.5e-15),
    "perpendicular ray eps=0": (3.0e-11, 1.4e-11, 1.4e-15, 6.8e-14),
    "perpendicular ray eps=1e-09": (2.1e-12, 2.4e-11, 1.6e-15, 1.6e-14),
    "perpendicular ray eps=1e-06": (1.1e-10, 4.2e-11, 1.6e-15, 3.9e-14),
    "perpendicular ray eps=0.0001": (9.9e-12, 5.1e-12, 1.7e-15, 2.6e-14),
    "seam": (1.2e-10, 1.1e-10, 1.7e-15, 9.7e-15),
    "isosceles eps=0": (7.4e-13, 9.6e-13, 1.6e-15, 1.1e-15),
    "isosceles eps=1e-06": (7.2e-13, 1.1e-12, 1.8e-15, 3.1e-15),
    "isosceles eps=0.001": (4.8e-12, 1.8e-11, 1.6e-15, 3.0e-15),
    "small triangle": (None, None, 1.5e-15, 3.0e-4),        # backward-only: nothing is matched
}


def p3p_tolerance(name):
    spec_truth, host_spec, _, _ = P3P_MEASURED[name]
    return MARGIN * max(spec_truth, host_spec)


if __name__ == "__main__":
    print("FIVE_POINT_SPEC_RESIDUALS = {")
    for fam in five_point_families():
        sets = five_point_spec(fam.name)
        w = worst_essential_residuals(fam, sets)
        miss = 0 if fam.cls != FORWARD else sum(min([ue.matrix_distance(true_essential(fam), e) for e in S] + [9.0]) > 1e-6 for S in sets)
        print(f'    "{fam.name}": ({w[0]:.2g}, {w[1]:.2g}, {w[2]:.2g}),    # truth missed in {miss} of {len(sets)}')
    print("}\nP3P (specification only; the host column comes from test_solver_families_host.py -s):")
    for fam in p3p_families():
        sets = p3p_spec(fam.name)
        w = worst_pose_residuals(fam, sets)
        d = [truth_distance(fam, S) for S in sets]
        print(f'    "{fam.name}": ({max(d):.2g}, HOST, {w[0]:.2g}, {w[2]:.2g}),    # min depth ratio {w[1]:.2g}, '
              f"solutions {sorted(set(len(S) for S in sets))}")
