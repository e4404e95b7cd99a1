"""Model-level GPU tests of every DINOv2 variant the extractors accept: `ViTExtractor._tokens` in bf16 (the product path,
hand-written kernels for every MLP variant) against float32 on the same seeded weights, judged per image and per row
(tests/util_vit.py) rather than by one rel-L2 over the batch.  Plus the `_reg` variants through the trainable and the hybrid
extractor, which share the token path."""
import numpy as np
import pytest
import torch

from oracle import preprocess_oracle as po
from oracle import vit_oracle
from test_e2e_gpu import synthetic_image
from util_vit import assert_token_errors, format_errors, token_errors

pytestmark = pytest.mark.gpu

SEED = 3

# (per-image rel L2 bound, worst-row bound), each about twice the worst value measured on the MI355X (2 frames of 640 x 480,
# seed 3; per-image rel L2 max / worst row / tail-row max over the median row):
#   vits14      9.45e-3 / 1.18e-2 / 1.18       vits14_reg  9.72e-3 / 1.28e-2 / 1.20
#   vitb14      9.52e-3 / 1.12e-2 / 1.18       vitb14_reg  9.78e-3 / 1.12e-2 / 1.13
#   vitl14      1.17e-2 / 1.34e-2 / 1.10       vitl14_reg  1.18e-2 / 1.33e-2 / 1.11
#   vitg14      1.88e-2 / 2.17e-2 / 1.15       (library GEMMs in bf16: the SwiGLU model has no hand-written path)
BOUNDS = {
    "dinov2_vits14": (2.0e-2, 2.5e-2),
    "dinov2_vits14_reg": (2.0e-2, 2.6e-2),
    "dinov2_vitb14": (2.0e-2, 2.5e-2),
    "dinov2_vitb14_reg": (2.0e-2, 2.5e-2),
    "dinov2_vitl14": (2.4e-2, 2.8e-2),
    "dinov2_vitl14_reg": (2.4e-2, 2.8e-2),
    "dinov2_vitg14": (3.8e-2, 4.4e-2),
}


def _frames():
    return np.stack([synthetic_image(k) for k in (0, 5)])


def _oracle_tokens(name, imgs):
    """float32 CPU oracle (oracle/vit_oracle.py) on the seeded weights `ViTExtractor(seed=SEED)` starts from."""
    from vit_colmap_amd.vit import build_dinov2

    model = build_dinov2(name).init_random(SEED)
    sd = {k: v.detach().clone().float() for k, v in model.state_dict().items()}
    x = torch.stack([torch.from_numpy(po.preprocess(im)[0]) for im in imgs])
    with torch.no_grad():
        return vit_oracle.forward_patch_tokens(sd, x, model.arch.heads)


@pytest.mark.parametrize("name", list(BOUNDS))
def test_variant_tokens_against_float32(name, capsys):
    from vit_colmap_amd.features.vit_extractor import ViTExtractor
    from vit_colmap_amd.vit import DINOV2_ARCHS

    arch = DINOV2_ARCHS[name]
    giant = arch.ffn == "swiglu"
    ex = ViTExtractor(model_name=name, precision="bf16", seed=SEED, num_keypoints=256, descriptor_dim=128,
                      tune_gemm=not giant)
    if not giant:
        assert bool(ex.model._hip), f"{name}: the bf16 forward must run on the hand-written kernels"
    assert ex.tune_gemm is False
    imgs = _frames()
    d = torch.from_numpy(imgs).cuda()
    tokens, hp, wp = ex._tokens(d)
    assert (hp, wp) == (34, 45) and tuple(tokens.shape) == (2, hp * wp, arch.dim) and tokens.dtype == torch.bfloat16
    got = tokens.float()
    del ex, tokens
    torch.cuda.empty_cache()
    if arch.dim == 384:
        ref = _oracle_tokens(name, imgs)
        got, what = got.cpu(), "CPU float32 oracle"
    else:
        # float32 module path on the GPU (library GEMMs and SDPA, none of the hand-written kernels), the same seeded weights
        assert not torch.backends.cuda.matmul.allow_tf32
        ref_ex = ViTExtractor(model_name=name, precision="fp32", seed=SEED, num_keypoints=256, descriptor_dim=128)
        assert ref_ex.dtype == torch.float32 and not getattr(ref_ex.model, "_hip", None)
        ref = ref_ex._tokens(d)[0].float()
        del ref_ex
        what = "float32 module path"
    e = token_errors(got, ref)
    with capsys.disabled():
        print(f"\n[{name} bf16 tokens vs {what}] {format_errors(e)}")
    assert_token_errors(e, *BOUNDS[name])
    del got, ref
    torch.cuda.empty_cache()


def test_trainable_extractor_with_register_backbone():
    from vit_colmap_amd.features.trainable_vit_extractor import TrainableViTExtractor

    ex = TrainableViTExtractor(model_name="dinov2_vits14_reg", num_keypoints=300, descriptor_dim=128, device="cuda",
                               precision="bf16", seed=SEED)
    assert bool(ex.model.backbone._hip)
    kp, desc = ex._run_inference(synthetic_image(2))
    assert 50 < len(kp) <= 300 and desc.shape == (len(kp), 128) and desc.dtype == np.uint8
    assert np.isfinite(kp).all()


def test_hybrid_extractor_with_register_backbone():
    from vit_colmap_amd.features.hybrid_extractor import HybridViTExtractor

    ys, xs = np.mgrid[20:460:40, 30:610:40]
    pts = np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.float32) + 0.25
    ex = HybridViTExtractor(model_name="dinov2_vits14_reg", num_keypoints=400, descriptor_dim=128, device="cuda",
                            keypoint_fn=lambda img: pts, seed=SEED)
    assert bool(ex._vit.model._hip)
    kp, desc = ex._run_inference(synthetic_image(3))
    assert len(kp) == len(pts) and desc.shape == (len(pts), 128) and desc.dtype == np.uint8
    assert int((desc.astype(np.int32).sum(axis=1) > 0).sum()) == len(pts)
