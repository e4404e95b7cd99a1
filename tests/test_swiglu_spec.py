"""CPU-side checks of the SwiGLU epilogue of vc_linear_bf16 (DINOv2 ViT-g/14): the header and the Python front end agree on
the code, the shape logic of `hip_ops.linear`, the entry's argument checks (which run before anything touches a device), and
what `prepare_hip` does with a SwiGLU model.  No kernel is launched."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vitcolmap_hip.h")
GEMM = os.path.join(ROOT, "vit_colmap_amd", "csrc", "gemm.hip")


def _defines(path, prefix):
    return {k: int(v) for k, v in re.findall(rf"^#define ({prefix}\w+) \(?(-?\d+)\)?", open(path).read(), flags=re.M)}


def test_header_and_python_agree_on_the_epilogue_codes():
    from vit_colmap_amd.vit import hip_ops

    codes = _defines(HEADER, "VC_EPI_")
    assert codes == {"VC_EPI_BIAS": hip_ops.EPI_BIAS, "VC_EPI_GELU": hip_ops.EPI_GELU,
                     "VC_EPI_RESIDUAL": hip_ops.EPI_RESIDUAL, "VC_EPI_SWIGLU": hip_ops.EPI_SWIGLU}
    assert len(set(codes.values())) == 4
    # the kernel-internal patch-embedding code is none of the public ones
    internal = re.search(r"enum \{([^}]*EPI_PATCH[^}]*)\}", open(GEMM).read()).group(1)
    patch = int(re.search(r"EPI_PATCH = (\d+)", internal).group(1))
    assert patch not in codes.values()
    assert int(re.search(r"EPI_SWIGLU = (\d+)", internal).group(1)) == codes["VC_EPI_SWIGLU"]


def test_linear_supported_and_output_shape():
    from vit_colmap_amd.vit.hip_ops import EPI_BIAS, EPI_GELU, EPI_RESIDUAL, EPI_SWIGLU, linear_out_shape, linear_supported

    w12 = torch.empty(8192, 1536, device="meta")                     # the giant's fused gate / value projection
    assert linear_supported(w12) and linear_supported(w12, EPI_SWIGLU)
    assert linear_out_shape((2, 1531, 1536), w12.shape, EPI_SWIGLU) == (2, 1531, 4096)
    for epi in (EPI_BIAS, EPI_GELU, EPI_RESIDUAL):
        assert linear_out_shape((2, 1531, 1536), w12.shape, epi) == (2, 1531, 8192)
    assert linear_out_shape((37, 64), (256, 64), EPI_SWIGLU) == (37, 128)
    # both halves must fill whole tiles: n_out % 256, where the other epilogues take n_out % 128
    w = torch.empty(384, 64, device="meta")
    assert linear_supported(w) and not linear_supported(w, EPI_SWIGLU)
    assert not linear_supported(torch.empty(256, 100, device="meta"), EPI_SWIGLU)
    assert linear_supported(torch.empty(256, 64, device="meta"), EPI_SWIGLU)
    with pytest.raises(ValueError):
        linear_out_shape((4, 100), (256, 64), EPI_SWIGLU)            # x does not fit the weight
    with pytest.raises(ValueError):
        linear_out_shape((4, 64), (255, 64), EPI_SWIGLU)             # no two halves


def test_entry_checks_its_arguments_before_touching_a_device():
    """rows == 0 returns behind the argument checks and in front of the first device call: the statuses of the contract in
    the header, with made-up (16-byte aligned) addresses that are never dereferenced."""
    from vit_colmap_amd import _lib
    from vit_colmap_amd.vit.hip_ops import EPI_BIAS, EPI_RESIDUAL, EPI_SWIGLU

    lib = _lib.load()
    x, w, b, r, o = (0x1000 * (i + 1) for i in range(5))
    call = lambda res, n, k, epi: lib.vc_linear_bf16(x, w, b, res, o, 0, n, k, epi, None)
    assert call(None, 8192, 1536, EPI_SWIGLU) == _lib.VC_OK
    assert call(None, 256, 64, EPI_SWIGLU) == _lib.VC_OK
    assert call(r, 8192, 1536, EPI_SWIGLU) == -1                     # a residual: VC_ERR_INVALID_ARG
    assert call(None, 384, 64, EPI_SWIGLU) == -2                     # n_out % 256: VC_ERR_UNSUPPORTED
    assert call(None, 256, 100, EPI_SWIGLU) == -2                    # k_in % 64
    assert call(None, 384, 64, EPI_BIAS) == _lib.VC_OK               # (the other epilogues keep n_out % 128)
    assert call(r, 384, 64, EPI_RESIDUAL) == _lib.VC_OK
    assert call(None, 256, 64, 3) == -1 and call(r, 256, 64, 3) == -1   # the internal patch-embedding code stays internal
    assert call(None, 256, 64, 5) == -1 and call(None, 256, 64, -1) == -1
    assert lib.vc_linear_bf16(x + 8, w, b, None, o, 0, 256, 64, EPI_SWIGLU, None) == -1   # misaligned x


def test_prepare_hip_covers_the_swiglu_architecture():
    """A folded SwiGLU model is no longer turned away by `prepare_hip` (`_hip = False` without a word): it builds GEMM
    operands, which needs the parameters on the GPU."""
    from vit_colmap_amd.vit.dinov2 import Arch, DinoV2

    m = DinoV2(Arch(128, 1, 2, ffn="swiglu", img_size=28)).init_random(1).eval().fold_layerscale()
    with pytest.raises(RuntimeError, match="on the GPU"):
        m.prepare_hip()
    # unfolded LayerScale: not prepared, `_blocks_fused` stays the path
    m2 = DinoV2(Arch(128, 1, 2, ffn="swiglu", img_size=28)).init_random(1).eval()
    assert m2.prepare_hip()._hip is False and m2.accepts_padded_patches is False
