"""GPU tests of the multi-stream ViT paths: batch shards inside the block stack (`DinoV2._run_sharded`), shards of the whole
device path (`ViTExtractor.extract_device`), and consecutive pipelined calls as bench.py enqueues them.  The ViT kernels use
no float atomics and a shard computes exactly what the same images compute alone (vit/dinov2.py, "batch shards on HIP
streams"), so every comparison between stream layouts is bit-exact."""
import numpy as np
import pytest
import torch

from oracle import c_oracle
from test_e2e_gpu import synthetic_image
from util_vit import assert_token_errors, format_errors, token_errors

pytestmark = pytest.mark.gpu

K, D = 512, 384      # bench.py's configuration (C2): ViT-S tokens are the descriptors, no projection


def _frames(first, n, w=640, h=480):
    return np.stack([synthetic_image(first + k, w, h) for k in range(n)])


def _patches(imgs):
    from vit_colmap_amd.features import hip_preprocess

    d = torch.from_numpy(imgs).cuda()
    return hip_preprocess.preprocess(d, out_dtype=torch.bfloat16, layout="patches_pad")


def _sharded_vs_alone(model, patches, hp, wp, shards):
    """Tokens of the batch with `shards` block-stack shards; each shard's rows must equal the shard's images run alone on one
    stream.  -> the sharded tokens."""
    B = patches.shape[0]
    model.batch_shards = shards
    assert model._shard_plan(torch.empty((B, 1, 1), device="cuda")) is not None, "the sharded path must engage"
    with torch.inference_mode():
        tokens = model.forward_patch_tokens(patches, hp, wp)
        model.batch_shards = 1
        bounds = [B * i // shards for i in range(shards + 1)]
        for i in range(shards):
            alone = model.forward_patch_tokens(patches[bounds[i]:bounds[i + 1]].contiguous(), hp, wp)
            assert torch.equal(tokens[bounds[i]:bounds[i + 1]], alone), f"shard {i} ({bounds[i]}..{bounds[i + 1]}) of {B}"
    model.batch_shards = None
    return tokens


@pytest.mark.parametrize("B,shards", [(17, 2), (50, 3)])
def test_vits_block_stack_shards_equal_the_shards_alone(B, shards, capsys):
    from vit_colmap_amd.features.vit_extractor import ViTExtractor

    ex = ViTExtractor(model_name="dinov2_vits14", num_keypoints=K, descriptor_dim=D, precision="bf16", seed=0)
    assert ex.model._hip and ex.model._hip[0].get("kind") != "gemm"
    imgs = _frames(0, B)
    tokens = _sharded_vs_alone(ex.model, _patches(imgs), 34, 45, shards)
    if B < 50:
        return
    # every image of the sharded batch against the float32 module path on the same seeded weights
    del ex
    torch.cuda.empty_cache()
    assert not torch.backends.cuda.matmul.allow_tf32
    ref_ex = ViTExtractor(model_name="dinov2_vits14", num_keypoints=K, descriptor_dim=D, precision="fp32", seed=0)
    d = torch.from_numpy(imgs).cuda()
    ref = torch.cat([ref_ex._tokens(d[i:i + 10])[0] for i in range(0, B, 10)])
    e = token_errors(tokens.float(), ref)
    with capsys.disabled():
        print(f"\n[ViT-S, {B} images in {shards} block-stack shards vs float32 module path] {format_errors(e)}")
    assert_token_errors(e, 2.0e-2, 2.5e-2)        # measured 9.74e-3 per image, 1.26e-2 worst row


def test_vitb_block_stack_shards_equal_the_shards_alone():
    from vit_colmap_amd.features.vit_extractor import ViTExtractor

    ex = ViTExtractor(model_name="dinov2_vitb14", num_keypoints=256, descriptor_dim=128, precision="bf16", seed=1)
    assert ex.model._hip and ex.model._hip[0]["kind"] == "gemm"
    imgs = _frames(3, 16, 280, 224)
    _sharded_vs_alone(ex.model, _patches(imgs), 16, 20, 2)


def _serial(ex, d):
    """`_extract_one` on the caller's stream, one shard of the block stack: the reference layout."""
    h, w = d.shape[1:3]
    inner = ex.model.batch_shards
    ex.model.batch_shards = 1
    try:
        with torch.inference_mode():
            return ex._extract_one(d, (h, w, (h // 14) * 14, (w // 14) * 14))
    finally:
        ex.model.batch_shards = inner


def _assert_results_equal(got, ref, what):
    assert set(got) == set(ref), (what, sorted(got), sorted(ref))
    for k in ref:
        assert got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype, (what, k)
        if not torch.equal(got[k], ref[k]):                    # padding behind the counts included
            differ = [i for i in range(ref[k].shape[0]) if not torch.equal(got[k][i], ref[k][i])]
            raise AssertionError(f"{what}: '{k}' differs in images {differ} of {ref[k].shape[0]}")


def test_extract_device_shards_equal_serial_extraction():
    """B = 20, standalone call: two shards, the second on a side stream.  Every output tensor equals `_extract_one` run per
    shard on the caller's stream."""
    from vit_colmap_amd.features.vit_extractor import ViTExtractor

    ex = ViTExtractor(model_name="dinov2_vits14", num_keypoints=K, descriptor_dim=D, precision="bf16", seed=0)
    d = torch.from_numpy(_frames(7, 20)).cuda()
    bounds = ex._shard_bounds(20)
    assert bounds == [0, 10, 20]
    res = ex.extract_device(d)
    parts = [_serial(ex, d[bounds[i]:bounds[i + 1]]) for i in range(2)]
    ref = {k: torch.cat([p[k] for p in parts]) for k in parts[0]}
    torch.cuda.synchronize()
    assert int(ref["count"].min()) > 50
    _assert_results_equal(res, ref, "extract_device(B=20)")


def test_pipelined_calls_as_bench_runs_them():
    """Four frame sets (16-50 images) through a FRESH extractor, `extract_device(frames, input_ready=ev)` enqueued back to back
    with no host synchronisation, each followed on the caller's stream by bench.py's tail (prepare + match into reused output
    buffers); one call's frames are freed and their memory reused on the caller's stream while the pipeline is in flight.
    Each result must equal a serial single-stream run on the same frames, each match list the C oracle on the returned
    descriptors."""
    from vit_colmap_amd.features.vit_extractor import ViTExtractor
    from vit_colmap_amd.matching import exhaustive_pairs, match_pairs, prepare_descriptors

    ex = ViTExtractor(model_name="dinov2_vits14", num_keypoints=K, descriptor_dim=D, precision="bf16", seed=0)
    assert not ex.model._pos_cache                       # the per-grid state is built inside the first pipelined call
    sizes = (50, 16, 33, 24)
    host = [_frames(100 * i, n) for i, n in enumerate(sizes)]
    frames, ready = [], []
    for h in host:
        frames.append(torch.from_numpy(h).cuda())
        ev = torch.cuda.Event()
        ev.record()
        ready.append(ev)
    pairs = [exhaustive_pairs(n, "cuda") for n in sizes]
    p_max = max(p.shape[0] for p in pairs)
    out_m = torch.empty((p_max, K, 2), dtype=torch.int32, device="cuda")
    out_c = torch.empty((p_max,), dtype=torch.int32, device="cuda")
    results, matches = [], []
    for i, n in enumerate(sizes):
        res = ex.extract_device(frames[i], input_ready=ready[i])
        P = pairs[i].shape[0]
        prepared = prepare_descriptors(res["desc_u8"], res["count"])
        match_pairs(prepared, res["count"], n, K, D, pairs[i], out_matches=out_m[:P], out_counts=out_c[:P])
        matches.append((out_m[:P].clone(), out_c[:P].clone()))      # the buffers are reused by the next call
        results.append(res)
        if i == 1:
            # the caller drops these frames while the pipeline is in flight; a same-size block is handed out at once on the
            # caller's stream and overwritten
            shape = frames[1].shape
            frames[1] = None
            junk = torch.empty(shape, dtype=torch.uint8, device="cuda")
            junk.fill_(0xA5)
            del junk
    torch.cuda.synchronize()
    for i, n in enumerate(sizes):
        ref = _serial(ex, torch.from_numpy(host[i]).cuda())
        _assert_results_equal(results[i], ref, f"pipelined call {i} ({n} images)")
        desc = results[i]["desc_u8"].cpu().numpy()
        counts = results[i]["count"].cpu().numpy()
        assert int(counts.min()) > 50
        om, oc, _ = c_oracle.match_pairs(desc, counts, pairs[i].cpu().numpy())
        gm, gc = matches[i][0].cpu().numpy().view(np.uint32), matches[i][1].cpu().numpy()
        assert np.array_equal(gc, oc), f"call {i}: match counts"
        for p in range(len(oc)):
            assert np.array_equal(gm[p, :gc[p]], om[p, :oc[p]]), f"call {i}, pair {p}"
