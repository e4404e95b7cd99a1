#!/usr/bin/env python3
"""Developer tool: DINOv2 ViT-g/14 (SwiGLU) token path, 8 frames of 640 x 480 in bf16, on the hand-written kernels
(`_blocks_gemm`, SwiGLU epilogue) against the library path the model took before (`model._hip = False`: `_blocks_fused`, i.e.
F.linear / SDPA / chunk + silu + mul, under TunableOp as `ViTExtractor` sets it up), same weights, same process.  The legs
alternate and repeat (`--rounds`), each reported as the median over rounds with its min-max spread; then the two MLP GEMMs
alone at the same row count.  Prints one JSON line at the end.  `--no-tunableop` runs the library leg on the default heuristic."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vit_colmap_amd.features.vit_extractor import ViTExtractor  # noqa: E402
from vit_colmap_amd.vit import hip_ops as ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=8)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--no-tunableop", action="store_true")
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_vitg.py measures on the GPU; there is no fallback"

PEAK = 2.5e15                      # bf16 dense MFMA peak, FLOP/s
N_TOK, D, HID, DEPTH = 1531, 1536, 4096, 40
# SURVEY §8 with the SwiGLU term in place of the MLP's: per block qkv + proj (8 N D^2), attention (4 N^2 D), w12 + w3 (3 * 2 N D HID)
FLOP_IMAGE = DEPTH * (8 * N_TOK * D * D + 4 * N_TOK * N_TOK * D + 3 * 2 * N_TOK * D * HID) + 2 * (N_TOK - 1) * 588 * D


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def alternate(legs, rounds, iters, warm=2):
    """legs {name: fn} -> {name: [ms per call, one per round]}, the legs interleaved round by round."""
    for fn in legs.values():
        for _ in range(warm):
            fn()
    out = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            out[k].append(timed(fn, iters))
    return out


def summary(ts):
    return dict(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts))


ex = ViTExtractor(model_name="dinov2_vitg14", num_keypoints=2048, descriptor_dim=128)
model = ex.model
hip = model._hip
assert hip and hip[0]["kind"] == "gemm" and ex.tune_gemm is False
frames = torch.randint(0, 255, (args.frames, 480, 640, 3), dtype=torch.uint8, device="cuda")
if not args.no_tunableop:          # what the constructor does for a model the hand-written GEMMs do not cover
    import torch.cuda.tunable as tunable

    tunable.set_max_tuning_duration(200)
    tunable.set_max_tuning_iterations(20)
    tunable.set_filename(os.devnull, False)


def new_path():
    model._hip, ex.tune_gemm = hip, False
    return ex._tokens(frames)[0]


def library_path():
    model._hip, ex.tune_gemm = False, not args.no_tunableop
    try:
        return ex._tokens(frames)[0]
    finally:
        model._hip, ex.tune_gemm = hip, False


a, b = new_path().float(), library_path().float()
rel = float((a - b).norm() / b.norm())
print(f"tokens, hand-written vs library path: rel L2 {rel:.3e} (both bf16)", flush=True)
del a, b
res = {k: summary(v) for k, v in alternate({"hand_written": new_path, "library": library_path}, args.rounds, args.iters).items()}
for k, s in res.items():
    tf = FLOP_IMAGE * args.frames / (s["median_ms"] * 1e-3)
    s["tflops"], s["share_of_bf16_peak"] = tf / 1e12, tf / PEAK
    print(f"{k:13s} {args.frames} frames: median {s['median_ms']:.2f} ms (min {s['min_ms']:.2f}, max {s['max_ms']:.2f}) = "
          f"{tf / 1e12:.0f} TFLOP/s = {100 * tf / PEAK:.1f} % of the bf16 peak", flush=True)
spread = res["library"]["max_ms"] - res["library"]["min_ms"]
gain = res["library"]["median_ms"] - res["hand_written"]["median_ms"]
print(f"gain {gain:.2f} ms against a library-path spread of {spread:.2f} ms: "
      f"{'faster by more than the spread' if gain > spread else 'NOT faster by more than the spread'}", flush=True)

# ---- the two MLP GEMMs alone, at the rows of the token path ------------------------------------------------------------
M = args.frames * N_TOK
g = torch.Generator(device="cuda").manual_seed(0)
rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)
x = rnd(M, D).to(torch.bfloat16)
w12, b12 = (rnd(2 * HID, D) / D ** 0.5).to(torch.bfloat16), rnd(2 * HID).to(torch.bfloat16)
hdn = rnd(M, HID).to(torch.bfloat16)
w3, b3 = (rnd(D, HID) / HID ** 0.5).to(torch.bfloat16), rnd(D).to(torch.bfloat16)
resid = rnd(M, D).to(torch.bfloat16)
out3 = torch.empty_like(resid)


def lib_w12():
    x1, x2 = F.linear(x, w12, b12).chunk(2, dim=-1)
    return F.silu(x1) * x2


legs = {
    "w12_swiglu_hand_written": lambda: ops.linear(x, w12, b12, ops.EPI_SWIGLU),
    "w12_swiglu_library": lib_w12,
    "w12_library_gemm_alone": lambda: F.linear(x, w12, b12),
    "w3_residual_hand_written": lambda: ops.linear(hdn, w3, b3, ops.EPI_RESIDUAL, residual=resid, out=out3),
    "w3_residual_library": lambda: torch.add(F.linear(hdn, w3, b3), resid, out=out3),
}
flops = {k: 2.0 * M * D * (2 * HID if k.startswith("w12") else HID) for k in legs}
if not args.no_tunableop:          # the library legs as the model's forward would run them
    tunable.enable(True)
gem = {k: summary(v) for k, v in alternate(legs, args.rounds, 20, warm=3).items()}
if not args.no_tunableop:
    tunable.enable(False)
for k, s in gem.items():
    s["tflops"] = flops[k] / (s["median_ms"] * 1e-3) / 1e12
    print(f"{k:26s} {M} rows: median {s['median_ms'] * 1e3:7.1f} us (min {s['min_ms'] * 1e3:.1f}, max {s['max_ms'] * 1e3:.1f}) "
          f"{s['tflops']:5.0f} TFLOP/s", flush=True)
print(json.dumps(dict(tool="bench_vitg", frames=args.frames, rounds=args.rounds, tunableop=not args.no_tunableop,
                      flop_per_image=FLOP_IMAGE, tokens_rel_l2=rel, token_path=res, gemms=gem)))
