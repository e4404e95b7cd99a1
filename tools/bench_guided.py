#!/usr/bin/env python3
"""Guided matching against the unguided matcher on the same prepared blocks (developer tool; bench.py is the judged
entry): vc_match_pairs_guided_u8 over every pair of the 50 x 512 x 384 workload, once with F models and once with H
models, and vc_match_pairs_u8 on the same pairs as the baseline.  Prints one JSON line.

Every image shows the same 512 scene points from its own camera (a rotation about the vertical axis and a side step per
image), so each pair has an exact fundamental matrix (about 3 % of a pair's candidates are admissible at 4 px); the H
models are the pairs' infinite homographies (under 0.2 %).  The descriptors are those of the judged matcher workload
(tests/util_data.image_set): they decide which tiles reach the masked update at all, the models only what it keeps."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from util_data import image_set  # noqa: E402
from vit_colmap_amd.matching import exhaustive_pairs, match_pairs, match_pairs_guided, prepare_descriptors  # noqa: E402

INT8_PEAK_OPS = 5.0e15   # dense int8 MFMA peak of the card, operations per second (multiply and add counted separately)


def cameras_and_keypoints(n_images, n, seed=0, width=640, height=480):
    """-> keypoints float32 (n_images, n, 2), per image (R, t), K: n scene points seen by n_images pinhole cameras."""
    rs = np.random.RandomState(seed)
    K = np.array([[600.0, 0, width / 2], [0, 600.0, height / 2], [0, 0, 1]])
    X = np.stack([rs.uniform(-3, 3, n), rs.uniform(-2, 2, n), rs.uniform(4, 9, n)], axis=1)
    kps, poses = [], []
    for k in range(n_images):
        a = 0.004 * k
        R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        t = np.array([-0.03 * k, 0.002 * k, 0.0])
        p = (K @ (R @ X.T + t[:, None])).T
        kps.append(p[:, :2] / p[:, 2:] + rs.normal(0, 0.5, (n, 2)))
        poses.append((R, t))
    return np.stack(kps).astype(np.float32), poses, K


def pair_models(pairs, poses, K):
    """Exact F (x2' F x1 = 0) and the infinite homography K R K^-1 of every pair, float32 (P, 9) each."""
    Ki = np.linalg.inv(K)
    Fs, Hs = [], []
    for a, b in pairs:
        (Ra, ta), (Rb, tb) = poses[a], poses[b]
        R = Rb @ Ra.T
        t = tb - R @ ta
        tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
        F = Ki.T @ tx @ R @ Ki
        Fs.append((F / np.linalg.norm(F)).reshape(9))
        H = K @ R @ Ki
        Hs.append((H / H[2, 2]).reshape(9))
    return np.stack(Fs).astype(np.float32), np.stack(Hs).astype(np.float32)


def timed(fns, iters):
    """{name: launch} -> {name: (median, min, max) ms}: device events around each launch, the versions alternating inside
    every repetition so that whatever else the machine does falls on all of them alike."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(iters):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=50)
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--d", type=int, default=384)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--kind", default="vit", help="descriptor statistics of tests/util_data.image_set")
    ap.add_argument("--max-error", dest="max_error", type=float, default=4.0)
    a = ap.parse_args()
    desc, counts = image_set(1, a.images, a.n, a.d, kind=a.kind)
    kps, poses, K = cameras_and_keypoints(a.images, a.n)
    pairs = exhaustive_pairs(a.images).numpy()
    f9, h9 = pair_models(pairs, poses, K)
    P = len(pairs)
    dd, dc, dk, dp = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (desc, counts, kps, pairs))
    prepared = prepare_descriptors(dd, dc)
    m = torch.empty((P, a.n, 2), dtype=torch.int32, device="cuda")
    c = torch.empty((P,), dtype=torch.int32, device="cuda")
    out = dict(images=a.images, n=a.n, d=a.d, pairs=P, iters=a.iters, descriptors=a.kind, max_error=a.max_error)
    dev_models = {"F": torch.from_numpy(f9).cuda(), "H": torch.from_numpy(h9).cuda()}
    dev_kind = {"F": torch.full((P,), 0, dtype=torch.int32, device="cuda"), "H": torch.full((P,), 1, dtype=torch.int32, device="cuda")}

    def unguided():
        match_pairs(prepared, dc, a.images, a.n, a.d, dp, out_matches=m, out_counts=c)

    def guided(name):
        return lambda: match_pairs_guided(prepared, dc, a.images, a.n, a.d, dk, dp, dev_models[name], dev_kind[name], a.max_error,
                                          out_matches=m, out_counts=c)

    launches = {"unguided": unguided, "guided_F": guided("F"), "guided_H": guided("H")}
    ms = timed(launches, a.iters)
    ops = 2.0 * a.n * a.n * a.d * P          # every multiply-add of the similarity matrices, as two operations
    for name, fn in launches.items():
        fn()
        torch.cuda.synchronize()
        out[name + "_ms"] = dict(median=ms[name][0], min=ms[name][1], max=ms[name][2])
        out[name + "_matches"] = int(c.sum().item())
        out[name + "_int8_mfma_fraction"] = ops / (ms[name][0] * 1e-3) / INT8_PEAK_OPS
        if name != "unguided":
            out[name + "_over_unguided"] = ms[name][0] / ms["unguided"][0]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
