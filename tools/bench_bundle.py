#!/usr/bin/env python3
"""Bundle adjustment (developer tool, bench.py is the judged entry).  Times the three entry points of
csrc/bundle.hip, the solve of the reduced system and the whole loop of mapping/bundle.py on two problems: the grown model of
the 12-view windowed scene (tests/util_mapper.py, truth_pairs rows: 12 cameras, 1161 points, 4283 observations) and a
synthetic arc of --cams cameras (default 200) 0.5 degrees apart with --points points (default 20 000), each seen by 3-8
neighbouring cameras, 0.5 px noise, poses and points moved off the truth.  A kernel's time is the median over --iters launches
after 3 warm-up launches, by device events; the loop's is wall clock around bundle_adjust, synchronised, the median of --loops
runs.  --refine-focal: the same two problems with every focal 3 % off and one tied group of intrinsics refined (§4.2k, "The
border"): also the three entry points of the border and the bordered solve, and the refined loop beside the plain loop of the
same build, the two alternating.  --radial: after every other column the four entry points with radial distortion on the same
problem (one group of six unknowns, k1 free from 0 and, with --refine-focal, the tied focal free too): the points pass, the
border's two passes and the step, beside the plain points pass and the border with four unknowns of the columns before; and
the loop that refines k1, alternating with the others.  --opencv (with --radial): the four entry points with the tangential terms
on the same problem (one group of eight unknowns, k1, k2, p1, p2 free from 0), and one whole pass (linearise, the border's two
passes, the step) of the _opencv entry points beside the same pass of the _radial ones, the two alternating ("The tangential
terms" in §4.2k).  --loss huber|soft_l1 (--loss-scale PX, default 1): after those columns also the points pass
under the loss (vc_ba_linearize_points_loss) and, with --refine-focal, the border's two passes with obs_w, on the same buffers;
and the loop under the loss beside the plain loop, alternating (with --refine-focal the refined loop under the loss too).
--solver pcg ("The solver" in §4.2k): after every other column vc_ba_camera_blocks, vc_ba_schur_product (both launches), one
whole solve by conjugate gradients on the first linearisation (wall clock, its host reads included) beside the Cholesky column,
the same number of iterations without the host read, and the pcg loop alternating with the dense loop; also a third arc of
--big-cams cameras (default 512, --big-points points) and, with pcg alone, a fourth of --above-cams cameras (default 1024), which
the dense route refuses.
Prints one JSON line.  Needs a GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from vit_colmap_amd import _lib  # noqa: E402
from vit_colmap_amd.mapping import bundle  # noqa: E402

K = np.array([[600.0, 0, 320.0], [0, 600.0, 240.0], [0, 0, 1]])


def windowed_problem():
    import util_bundle as ub
    import util_mapper as um
    from test_absolute_pose_spec import scene_images, truth_pairs

    scene = um.windowed_scene()
    images = scene_images(scene)
    grown = um.grow_model(images, truth_pairs(scene))
    ids, cams, points, offsets, obs_cam, obs_xy = ub.model_problem(images, grown)
    a, b = (ids.index(i) for i in grown["initial_pair"])
    return cams, points, offsets, obs_cam, obs_xy, ub.gauge_mask(cams, a, b)


def arc_problem(n_cams, n_points, seed=1, noise=0.5):
    rs = np.random.RandomState(seed)
    rows = []
    for a in np.radians(0.5 * (np.arange(n_cams) - n_cams / 2)):
        c = np.array([8.0 * np.sin(a), 0.2 * np.cos(5 * a), -8.0 * np.cos(a)])
        z = -c / np.linalg.norm(c)
        x = np.cross([0.0, 1.0, 0.0], z)
        x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z])
        rows.append(np.concatenate([R.reshape(9), -R @ c, [K[0, 0], K[1, 1], K[0, 2], K[1, 2]]]))
    cams = np.stack(rows)
    lengths = rs.randint(3, 9, n_points)
    offsets = np.concatenate([[0], np.cumsum(lengths)])
    point_of = np.repeat(np.arange(n_points), lengths)
    # a point's cameras: a random start and every fourth camera after it, so that a track spans up to 14 degrees
    first = rs.randint(0, n_cams - 4 * 8, n_points)
    obs_cam = (first[point_of] + 4 * (np.arange(offsets[-1]) - offsets[:-1][point_of])).astype(np.int32)
    X = np.stack([rs.uniform(-2, 2, n_points), rs.uniform(-1.5, 1.5, n_points), rs.uniform(-1.5, 1.5, n_points)], axis=1)
    Xc = np.einsum("nij,nj->ni", cams[obs_cam, :9].reshape(-1, 3, 3), X[point_of]) + cams[obs_cam, 9:12]
    obs_xy = np.stack([K[0, 0] * Xc[:, 0] / Xc[:, 2] + K[0, 2], K[1, 1] * Xc[:, 1] / Xc[:, 2] + K[1, 2]], axis=1) + rs.normal(0, noise, (len(obs_cam), 2))
    moved = cams.copy()
    moved[1:, 9:12] += rs.normal(0, 5e-3, (n_cams - 1, 3))
    mask = np.zeros(n_cams, np.uint8)
    mask[0], mask[1] = bundle.HELD_ALL, 1 << (3 + int(np.argmax(np.abs(cams[1, 9:12]))))
    return moved, X + rs.normal(0, 1e-2, X.shape), offsets.astype(np.int32), obs_cam, obs_xy, mask


def device_ms(fn, iters):
    for _ in range(3):
        fn()
    times = []
    for _ in range(iters):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop))
    return float(np.median(times))


def measure(problem, iters, loops, refine=False, loss=None, loss_scale=1.0, radial=False, solver=None, opencv=False):
    cams, points, offsets, obs_cam, obs_xy, mask = problem
    if refine:
        cams = cams.copy()
        cams[:, 12:14] *= 1.03
    c, n, t = len(cams), len(points), len(obs_cam)
    lib = _lib.load()
    dev = torch.device("cuda")
    d = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (cams, mask, points, offsets, obs_cam, obs_xy)]
    x = [torch.from_numpy(a).to(dev) for a in bundle.camera_index(obs_cam, offsets, c)]
    b = bundle._Buffers(torch, c, n, t, dev, with_loss=loss is not None)
    S = torch.zeros((6 * c, 6 * c) if c <= _lib.VC_BA_MAX_CAMS else (1, 1), dtype=torch.float64, device=dev)
    g, dc = torch.zeros(6 * c, dtype=torch.float64, device=dev), torch.zeros(6 * c, dtype=torch.float64, device=dev)
    out_cams, out_points, dx = torch.zeros_like(d[0]), torch.zeros_like(d[2]), torch.zeros_like(d[2])
    p, stream, lam = _lib.ptr, _lib.stream_ptr(), bundle.BA_LAMBDA0

    def linearize():
        _lib.check(lib.vc_ba_linearize_points(p(d[0]), c, p(d[1]), p(d[2]), n, p(d[3]), p(d[4]), p(d[5]), t, lam, p(b.vinv), p(b.gp), p(b.cost),
                                              p(b.count), p(b.obs_ok), p(b.obs_lin), p(b.total_cost), stream), "vc_ba_linearize_points")

    def reduce():
        _lib.check(lib.vc_ba_reduce_cameras(c, p(d[1]), n, p(d[3]), p(d[4]), t, p(x[0]), p(x[1]), p(x[2]), lam, p(b.vinv), p(b.gp), p(b.obs_ok),
                                            p(b.obs_lin), p(S), p(g), stream), "vc_ba_reduce_cameras")

    def solve():
        L, _ = torch.linalg.cholesky_ex(S)
        dc.copy_(torch.cholesky_solve(-g[:, None], L)[:, 0])

    def step():
        _lib.check(lib.vc_ba_step(p(d[0]), c, p(d[2]), n, p(d[3]), p(d[4]), t, p(b.vinv), p(b.gp), p(b.obs_ok), p(b.obs_lin), p(dc), p(out_cams),
                                  p(out_points), p(dx), stream), "vc_ba_step")

    out = dict(cameras=c, points=n, observations=t)
    dense = c <= _lib.VC_BA_MAX_CAMS                                  # above the cap only what pcg needs is measured
    stages = [("linearize_ms", linearize), ("reduce_ms", reduce), ("solve_ms", solve), ("step_ms", step)] if dense else [("linearize_ms", linearize)]
    groups = {}
    if refine:                                                        # one tied group, the principal point held
        f64 = dict(dtype=torch.float64, device=dev)
        groups = dict(cam_group=np.zeros(c, np.int32), intr_mask=np.array([16 | 4 | 8], np.uint8))
        dg, di = torch.from_numpy(groups["cam_group"]).to(dev), torch.from_numpy(groups["intr_mask"]).to(dev)
        xn, T, terms, sums = torch.zeros((t, 2), **f64), torch.zeros((n, 1, 12), **f64), torch.zeros((40, n), **f64), torch.zeros(40, **f64)
        B, C, h, free = torch.zeros((6 * c, 4), **f64), torch.zeros((4, 4), **f64), torch.zeros(4, **f64), torch.zeros(4, dtype=torch.uint8, device=dev)
        M, rhs, dtheta = torch.zeros((6 * c + 4, 6 * c + 4), **f64), torch.zeros(6 * c + 4, **f64), torch.zeros(4, **f64)
        valid = torch.zeros(c, dtype=torch.uint8, device=dev)

        def linearize_intrinsics():
            _lib.check(lib.vc_ba_linearize_intrinsics(p(d[0]), c, p(dg), 1, p(di), p(d[2]), n, p(d[3]), p(d[4]), t, p(b.vinv), p(b.gp), p(b.obs_ok),
                                                      p(b.obs_lin), p(xn), p(T), p(terms), stream), "vc_ba_linearize_intrinsics")

        def reduce_border():
            _lib.check(lib.vc_ba_reduce_border(c, p(dg), 1, p(di), n, p(d[3]), p(d[4]), t, p(x[0]), p(x[1]), p(x[2]), lam, p(b.vinv), p(b.obs_ok),
                                               p(b.obs_lin), p(xn), p(T), p(terms), p(sums), p(B), p(C), p(h), p(free), stream), "vc_ba_reduce_border")

        def solve_bordered():
            M[:6 * c, :6 * c], M[:6 * c, 6 * c:], M[6 * c:, :6 * c], M[6 * c:, 6 * c:] = S, B, B.T, C
            rhs[:6 * c], rhs[6 * c:] = g, h
            L, _ = torch.linalg.cholesky_ex(M)
            sol = torch.cholesky_solve(-rhs[:, None], L)[:, 0]
            dc.copy_(sol[:6 * c]), dtheta.copy_(sol[6 * c:])

        def step_intrinsics():
            _lib.check(lib.vc_ba_step_intrinsics(p(d[0]), c, p(dg), 1, p(di), p(d[2]), n, p(d[3]), p(d[4]), t, p(b.vinv), p(b.gp), p(b.obs_ok),
                                                 p(b.obs_lin), p(T), p(dc), p(dtheta), p(out_cams), p(out_points), p(dx), p(valid), stream),
                       "vc_ba_step_intrinsics")

        stages += [("linearize_intrinsics_ms", linearize_intrinsics), ("reduce_border_ms", reduce_border), ("solve_bordered_ms", solve_bordered),
                   ("step_intrinsics_ms", step_intrinsics)]
    if loss is not None:                                              # after the columns without a loss, on the same buffers
        kind = bundle.LOSSES[loss]

        def linearize_loss():
            _lib.check(lib.vc_ba_linearize_points_loss(p(d[0]), c, p(d[1]), p(d[2]), n, p(d[3]), p(d[4]), p(d[5]), t, lam, kind, loss_scale,
                                                       p(b.vinv), p(b.gp), p(b.cost), p(b.count), p(b.obs_ok), p(b.obs_lin), p(b.obs_w),
                                                       p(b.total_cost), stream), "vc_ba_linearize_points_loss")

        stages.append(("linearize_loss_ms", linearize_loss))
        if refine:
            def linearize_intrinsics_loss():
                _lib.check(lib.vc_ba_linearize_intrinsics_loss(p(d[0]), c, p(dg), 1, p(di), p(d[2]), n, p(d[3]), p(d[4]), t, p(b.vinv), p(b.gp),
                                                               p(b.obs_ok), p(b.obs_lin), p(b.obs_w), p(xn), p(T), p(terms), stream),
                           "vc_ba_linearize_intrinsics_loss")

            def reduce_border_loss():
                _lib.check(lib.vc_ba_reduce_border_loss(c, p(dg), 1, p(di), n, p(d[3]), p(d[4]), t, p(x[0]), p(x[1]), p(x[2]), lam, p(b.vinv),
                                                        p(b.obs_ok), p(b.obs_lin), p(xn), p(b.obs_w), p(T), p(terms), p(sums), p(B), p(C), p(h),
                                                        p(free), stream), "vc_ba_reduce_border_loss")

            stages += [("linearize_intrinsics_loss_ms", linearize_intrinsics_loss), ("reduce_border_loss_ms", reduce_border_loss)]
    radial_args = {}
    if radial:                                                        # after every other column: the _radial entry points, one group, k1 free
        f64 = dict(dtype=torch.float64, device=dev)
        rb = bundle._Buffers(torch, c, n, t, dev, with_dist=2)
        radial_args = dict(cam_group=np.zeros(c, np.int32), intr_mask=np.array([(16 | 4 | 8 if refine else 15) | 64], np.uint8),
                           cam_dist=np.zeros((c, 2)))
        rg, ri = torch.from_numpy(radial_args["cam_group"]).to(dev), torch.from_numpy(radial_args["intr_mask"]).to(dev)
        jt, T6, terms6, sums6 = torch.zeros((t, 6), **f64), torch.zeros((n, 1, 18), **f64), torch.zeros((84, n), **f64), torch.zeros(84, **f64)
        B6, C6, h6, free6 = torch.zeros((6 * c, 6), **f64), torch.zeros((6, 6), **f64), torch.zeros(6, **f64), torch.zeros(6, dtype=torch.uint8, device=dev)
        dtheta6, out_dist, valid6 = torch.zeros(6, **f64), torch.zeros((c, 2), **f64), torch.zeros(c, dtype=torch.uint8, device=dev)

        def linearize_radial():
            _lib.check(lib.vc_ba_linearize_points_radial(p(d[0]), c, p(rb.dist), p(d[1]), p(d[2]), n, p(d[3]), p(d[4]), p(d[5]), t, lam, 0, 1.0,
                                                         p(rb.vinv), p(rb.gp), p(rb.cost), p(rb.count), p(rb.obs_ok), p(rb.obs_lin), p(rb.obs_w),
                                                         p(rb.total_cost), stream), "vc_ba_linearize_points_radial")

        def linearize_intrinsics_radial():
            _lib.check(lib.vc_ba_linearize_intrinsics_radial(p(d[0]), c, p(rb.dist), p(rg), 1, p(ri), p(d[2]), n, p(d[3]), p(d[4]), t, 0, 1.0,
                                                             p(rb.vinv), p(rb.gp), p(rb.obs_ok), p(rb.obs_lin), p(rb.obs_w), p(jt), p(T6), p(terms6),
                                                             stream), "vc_ba_linearize_intrinsics_radial")

        def reduce_border_radial():
            _lib.check(lib.vc_ba_reduce_border_radial(c, p(rg), 1, p(ri), n, p(d[3]), p(d[4]), t, p(x[0]), p(x[1]), p(x[2]), lam, 0, 1.0, p(rb.vinv),
                                                      p(rb.obs_ok), p(rb.obs_lin), p(jt), p(rb.obs_w), p(T6), p(terms6), p(sums6), p(B6), p(C6),
                                                      p(h6), p(free6), stream), "vc_ba_reduce_border_radial")

        def step_radial():
            _lib.check(lib.vc_ba_step_radial(p(d[0]), c, p(rb.dist), p(rg), 1, p(ri), p(d[2]), n, p(d[3]), p(d[4]), t, p(rb.vinv), p(rb.gp),
                                             p(rb.obs_ok), p(rb.obs_lin), p(T6), p(dc), p(dtheta6), p(out_cams), p(out_dist), p(out_points), p(dx),
                                             p(valid6), stream), "vc_ba_step_radial")

        stages += [("linearize_radial_ms", linearize_radial), ("linearize_intrinsics_radial_ms", linearize_intrinsics_radial),
                   ("reduce_border_radial_ms", reduce_border_radial), ("step_radial_ms", step_radial)]
    passes = {}
    if radial and opencv:                                             # the same columns with eight unknowns: all four distortion numbers free
        ob = bundle._Buffers(torch, c, n, t, dev, with_dist=4)
        oi = torch.tensor([(16 | 4 | 8 if refine else 15)], dtype=torch.uint8, device=dev)
        jt8, T8, terms8, sums8 = torch.zeros((t, 10), **f64), torch.zeros((n, 1, 24), **f64), torch.zeros((144, n), **f64), torch.zeros(144, **f64)
        B8, C8, h8, free8 = torch.zeros((6 * c, 8), **f64), torch.zeros((8, 8), **f64), torch.zeros(8, **f64), torch.zeros(8, dtype=torch.uint8, device=dev)
        dtheta8, out_dist8 = torch.zeros(8, **f64), torch.zeros((c, 4), **f64)

        def linearize_opencv():
            _lib.check(lib.vc_ba_linearize_points_opencv(p(d[0]), c, p(ob.dist), p(d[1]), p(d[2]), n, p(d[3]), p(d[4]), p(d[5]), t, lam, 0, 1.0,
                                                         p(ob.vinv), p(ob.gp), p(ob.cost), p(ob.count), p(ob.obs_ok), p(ob.obs_lin), p(ob.obs_w),
                                                         p(ob.total_cost), stream), "vc_ba_linearize_points_opencv")

        def linearize_intrinsics_opencv():
            _lib.check(lib.vc_ba_linearize_intrinsics_opencv(p(d[0]), c, p(ob.dist), p(rg), 1, p(oi), p(d[2]), n, p(d[3]), p(d[4]), t, 0, 1.0,
                                                             p(ob.vinv), p(ob.gp), p(ob.obs_ok), p(ob.obs_lin), p(ob.obs_w), p(jt8), p(T8), p(terms8),
                                                             stream), "vc_ba_linearize_intrinsics_opencv")

        def reduce_border_opencv():
            _lib.check(lib.vc_ba_reduce_border_opencv(c, p(rg), 1, p(oi), n, p(d[3]), p(d[4]), t, p(x[0]), p(x[1]), p(x[2]), lam, 0, 1.0, p(ob.vinv),
                                                      p(ob.obs_ok), p(ob.obs_lin), p(jt8), p(ob.obs_w), p(T8), p(terms8), p(sums8), p(B8), p(C8),
                                                      p(h8), p(free8), stream), "vc_ba_reduce_border_opencv")

        def step_opencv():
            _lib.check(lib.vc_ba_step_opencv(p(d[0]), c, p(ob.dist), p(rg), 1, p(oi), p(d[2]), n, p(d[3]), p(d[4]), t, p(ob.vinv), p(ob.gp),
                                             p(ob.obs_ok), p(ob.obs_lin), p(T8), p(dc), p(dtheta8), p(out_cams), p(out_dist8), p(out_points), p(dx),
                                             p(valid6), stream), "vc_ba_step_opencv")

        stages += [("linearize_opencv_ms", linearize_opencv), ("linearize_intrinsics_opencv_ms", linearize_intrinsics_opencv),
                   ("reduce_border_opencv_ms", reduce_border_opencv), ("step_opencv_ms", step_opencv)]
        passes = dict(radial_pass_ms=lambda: (linearize_radial(), linearize_intrinsics_radial(), reduce_border_radial(), step_radial()),
                      opencv_pass_ms=lambda: (linearize_opencv(), linearize_intrinsics_opencv(), reduce_border_opencv(), step_opencv()))
    if solver == "pcg":
        pcg = bundle._Pcg(torch, lib, c, n, dev, bundle.PCG_REL_TOL, bundle.PCG_MAX_ITERATIONS)
        vector = torch.randn(6 * c, dtype=torch.float64, device=dev)

        def blocks(s=pcg):
            _lib.check(lib.vc_ba_camera_blocks(c, p(d[1]), n, p(d[3]), p(d[4]), t, p(x[0]), p(x[1]), p(x[2]), lam, p(b.vinv), p(b.gp), p(b.obs_ok),
                                               p(b.obs_lin), p(s.U), p(s.D), p(s.Minv), p(s.g), p(s.fixed), stream), "vc_ba_camera_blocks")

        def product(s=pcg, v=vector):
            _lib.check(lib.vc_ba_schur_product(c, n, p(d[3]), p(d[4]), t, p(x[0]), p(x[1]), p(x[2]), p(b.vinv), p(b.obs_ok), p(b.obs_lin), p(s.U),
                                               p(s.fixed), p(v), p(s.s), p(s.q), stream), "vc_ba_schur_product")

        stages += [("blocks_ms", blocks), ("product_ms", product)]
    for name, fn in stages:
        out[name] = round(device_ms(fn, iters), 4)
    if passes:                                                        # one whole pass of either family, the two alternating
        rounds = {name: [] for name in passes}
        for _ in range(loops):
            for name, fn in passes.items():
                rounds[name].append(device_ms(fn, iters))
        out.update({name: round(float(np.median(v)), 4) for name, v in rounds.items()})
    if solver == "pcg":
        # one whole solve on the first linearisation, wall clock with its host reads; then the same number of iterations of the same
        # device work without the read per iteration, which is what the read costs
        linearize()
        solves, blind = [], []
        for _ in range(loops + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, _, k = pcg.solve(blocks, product)
            torch.cuda.synchronize()
            solves.append(1e3 * (time.perf_counter() - t0))
            Minv, free = pcg.Minv.view(-1, 6, 6), pcg.fixed == 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            blocks()
            r = torch.where(free, -pcg.g, torch.zeros_like(pcg.g))
            z = (Minv * r.view(-1, 1, 6)).sum(dim=2).reshape(-1)
            q_, rz, xs = z.clone(), torch.dot(r, z), torch.zeros_like(r)
            for _ in range(k):
                product(pcg, q_)
                pq = torch.dot(q_, pcg.q)
                alpha = rz / pq
                xs, r = xs + alpha * q_, r - alpha * pcg.q
                torch.where(torch.isfinite(pq) & (pq > 0), torch.dot(r, r), pcg.nan)
                z = (Minv * r.view(-1, 1, 6)).sum(dim=2).reshape(-1)
                rz_new = torch.dot(r, z)
                q_, rz = z + (rz_new / rz) * q_, rz_new
            torch.cuda.synchronize()
            blind.append(1e3 * (time.perf_counter() - t0))
        out.update(pcg_solve_ms=round(float(np.median(solves[1:])), 3), pcg_solve_iterations=k,
                   pcg_solve_without_reads_ms=round(float(np.median(blind[1:])), 3))

    def loop(**kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cams_out, _, report = bundle.bundle_adjust(cams, points, offsets, obs_cam, obs_xy, mask, "cuda", **kw)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), report, cams_out

    walls, refined_walls, loss_walls, refined_loss_walls, radial_walls, pcg_walls = [], [], [], [], [], []
    loss_args = {} if loss is None else dict(loss=loss, loss_scale=loss_scale)
    for _ in range(loops + 1):                                        # the first run warms up; the loops alternate
        if solver == "pcg":
            wall, with_pcg, _ = loop(solver="pcg")
            pcg_walls.append(wall)
        if not dense:
            continue
        wall, report, _ = loop()
        walls.append(wall)
        if refine:
            wall, refined, cams_out = loop(**groups)
            refined_walls.append(wall)
        if loss is not None:
            wall, robust, _ = loop(**loss_args)
            loss_walls.append(wall)
            if refine:
                wall, refined_robust, robust_cams = loop(**groups, **loss_args)
                refined_loss_walls.append(wall)
        if radial:
            wall, with_k, _ = loop(**radial_args)
            radial_walls.append(wall)
    if dense:
        out.update(loop_ms=round(float(np.median(walls[1:])), 3), iterations=report["iterations"], accepted_steps=report["accepted_steps"],
                   initial_cost=report["initial_cost"], final_cost=report["final_cost"])
    if solver == "pcg":
        out.update(pcg_loop_ms=round(float(np.median(pcg_walls[1:])), 3), pcg_loop_iterations=with_pcg["iterations"],
                   pcg_accepted_steps=with_pcg["accepted_steps"], pcg_initial_cost=with_pcg["initial_cost"],
                   pcg_final_cost=with_pcg["final_cost"], pcg_iterations=with_pcg["pcg_iterations"])
    if refine:
        out.update(refined_loop_ms=round(float(np.median(refined_walls[1:])), 3), refined_iterations=refined["iterations"],
                   refined_accepted_steps=refined["accepted_steps"], refined_final_cost=refined["final_cost"], refined_focal=float(cams_out[0, 12]))
    if loss is not None:
        out.update(loss_loop_ms=round(float(np.median(loss_walls[1:])), 3), loss_iterations=robust["iterations"],
                   loss_accepted_steps=robust["accepted_steps"], loss_initial_cost=robust["initial_cost"], loss_final_cost=robust["final_cost"])
        if refine:
            out.update(refined_loss_loop_ms=round(float(np.median(refined_loss_walls[1:])), 3), refined_loss_iterations=refined_robust["iterations"],
                       refined_loss_final_cost=refined_robust["final_cost"], refined_loss_focal=float(robust_cams[0, 12]))
    if radial:
        out.update(radial_loop_ms=round(float(np.median(radial_walls[1:])), 3), radial_iterations=with_k["iterations"],
                   radial_final_cost=with_k["final_cost"], radial_k1=float(with_k["cam_dist"][0, 0]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cams", type=int, default=200)
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--loops", type=int, default=5)
    ap.add_argument("--refine-focal", dest="refine_focal", action="store_true",
                    help="every focal 3 %% off; also time the border's entry points and the loop that refines one tied focal")
    ap.add_argument("--loss", choices=[k for k in bundle.LOSSES if k != "trivial"], default=None,
                    help="also time the entry points that take a loss and the loop under it (DESIGN.md §4.2k, \"The loss\")")
    ap.add_argument("--loss-scale", dest="loss_scale", type=float, default=1.0, metavar="PX")
    ap.add_argument("--radial", action="store_true",
                    help="also time the entry points with radial distortion (six unknowns in one group, k1 free from 0) and the loop that "
                         "refines k1 (DESIGN.md §4.2k, \"The distortion\")")
    ap.add_argument("--opencv", action="store_true",
                    help="with --radial: also time the entry points with the tangential terms (eight unknowns in one group) and one whole pass "
                         "of them beside the same pass of the radial ones, alternating")
    ap.add_argument("--solver", choices=["pcg"], default=None,
                    help="also time the two entry points of the matrix-free solver, one solve and the pcg loop beside the dense one, on a "
                         "third arc of --big-cams cameras too and on a fourth of --above-cams with pcg alone (DESIGN.md §4.2k, \"The solver\")")
    ap.add_argument("--big-cams", dest="big_cams", type=int, default=512)
    ap.add_argument("--big-points", dest="big_points", type=int, default=51200)
    ap.add_argument("--above-cams", dest="above_cams", type=int, default=1024)
    ap.add_argument("--above-points", dest="above_points", type=int, default=102400)
    args = ap.parse_args()
    if args.opencv and not args.radial:
        ap.error("--opencv times its columns beside the radial ones: it needs --radial")
    extra = (args.refine_focal, args.loss, args.loss_scale, args.radial, args.solver, args.opencv)
    out = dict(tool="bench_bundle", iters=args.iters, loops=args.loops, refine_focal=args.refine_focal, loss=args.loss,
               loss_scale=args.loss_scale, radial=args.radial, solver=args.solver, windowed=measure(windowed_problem(), args.iters, args.loops, *extra),
               arc=measure(arc_problem(args.cams, args.points), args.iters, args.loops, *extra))
    if args.solver == "pcg":
        out.update(big_arc=measure(arc_problem(args.big_cams, args.big_points), args.iters, args.loops, *extra),
                   above_arc=measure(arc_problem(args.above_cams, args.above_points), args.iters, args.loops, False, None, 1.0, False, "pcg"))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
