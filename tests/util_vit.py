"""Shared helpers of the model-level ViT tests: localised token error reports and float32 references (torch only)."""
import torch

TAIL_ROWS = 256   # the last rows of an image: where ragged row tiles and the last attention query block sit


def token_errors(got: torch.Tensor, ref: torch.Tensor) -> dict:
    """got / ref (B, T, C) float tensors on one device -> localised relative errors (python floats / lists):
      per_image   rel L2 of every image (||g - r|| / ||r|| over its T x C values)
      row_median  median over all rows of the per-row error ||g_t - r_t|| / ||r_t||
      row_max     the worst row of the batch, row_argmax its (image, row)
      tail_max    the worst row among the last TAIL_ROWS rows of any image."""
    assert got.shape == ref.shape and got.dim() == 3, (tuple(got.shape), tuple(ref.shape))
    g, r = got.float(), ref.float()
    diff = g - r
    per_image = diff.flatten(1).norm(dim=1) / r.flatten(1).norm(dim=1)
    row = diff.norm(dim=2) / r.norm(dim=2).clamp_min(1e-30)          # (B, T)
    B, T = row.shape
    flat = int(row.argmax())
    tail = row[:, max(0, T - TAIL_ROWS):]
    return dict(per_image=per_image.tolist(), row_median=float(row.median()), row_max=float(row.max()),
                row_argmax=(flat // T, flat % T), tail_max=float(tail.max()))


def format_errors(e: dict) -> str:
    pi = e["per_image"]
    return (f"per-image rel L2 max {max(pi):.3e} (min {min(pi):.3e}, {len(pi)} images), per-row median {e['row_median']:.3e}, "
            f"max {e['row_max']:.3e} at {e['row_argmax']}, tail max {e['tail_max']:.3e}")


def assert_token_errors(e: dict, image_bound: float, row_bound: float, tail_factor: float = 2.0):
    """Every image under `image_bound`, the worst row under `row_bound`, the tail rows no worse than `tail_factor` x the
    median row (measured 1.1-1.3 x on every variant): an error confined to one image or to the last row tile cannot hide
    behind the batch aggregate."""
    worst = max(e["per_image"])
    assert worst < image_bound, (f"image {e['per_image'].index(worst)}: rel L2 {worst:.3e} >= {image_bound}", format_errors(e))
    assert e["row_max"] < row_bound, (f"row {e['row_argmax']}: rel {e['row_max']:.3e} >= {row_bound}", format_errors(e))
    assert e["tail_max"] <= tail_factor * e["row_median"], (f"tail rows {e['tail_max']:.3e} > {tail_factor} x median", format_errors(e))


def attention_reference(qkv: torch.Tensor, n_heads: int, scale: float, chunk: int = 2048) -> torch.Tensor:
    """softmax(scale Q K^T) V in float32 from (B, N, 3 * H * 64) data, one (image, head) and `chunk` queries at a time, so that
    no more than chunk x N scores exist at once -> (B, N, H * 64) float32."""
    B, N, _ = qkv.shape
    q, k, v = qkv.float().reshape(B, N, 3, n_heads, 64).permute(2, 0, 3, 1, 4)
    out = torch.empty((B, N, n_heads, 64), dtype=torch.float32, device=qkv.device)
    for b in range(B):
        for h in range(n_heads):
            kt, vh = k[b, h].t().contiguous(), v[b, h].contiguous()
            for s in range(0, N, chunk):
                att = torch.softmax((q[b, h, s:s + chunk] @ kt) * scale, dim=-1)
                out[b, s:s + chunk, h] = att @ vh
    return out.reshape(B, N, n_heads * 64)
