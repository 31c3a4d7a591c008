"""FoldedTrunk (fcmf_framework/resnet_eval.py): an eval-mode ResNet trunk with BatchNorm folded into the convolutions, against
oracle/resnet_oracle.py in eval mode.

float32: max error <= 1e-4 max|ref|.  bf16: the oracle is evaluated in float64 on the same float32 parameters and crops, and with
    e_fold  = max |FoldedTrunk - oracle|        e_plain = max |today's eval trunk_nhwc - oracle|
the test asserts e_fold <= 2 e_plain: folding drops one bf16 rounding of every activation before the affine and adds one bf16
rounding of every scaled weight -- errors of the same order, accumulated through the same depth.  Both figures are printed.
"""
import functools

import pytest
import torch

from helpers import _recorded
from oracle import resnet_oracle as RO
import synthetic_data as synth

pytestmark = pytest.mark.gpu

TINY = synth.RESNET_TINY_LAYERS


def _set(dtype):
    from fcmf_framework import ops
    ops.set_compute_dtype(dtype)
    ops.shadows.clear()


@functools.lru_cache(maxsize=None)
def _params(layers):
    return synth.synth_resnet_params(synth.resnet_param_shapes(layers), 0)


@functools.lru_cache(maxsize=None)
def _oracle(layers, n):
    """float64 NHWC output of the oracle's eval trunk on n seeded 64 x 64 crops (computed once, never modified)"""
    P = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in _params(layers).items()}
    y = RO.resnet_trunk(P, synth.synth_crops(n, 64, seed=1).double(), layers, training=False)
    return y.permute(0, 2, 3, 1).contiguous()


def _build(layers, dev):
    from fcmf_framework.resnet import ResNet
    m = ResNet(layers)
    missing, unexpected = m.load_state_dict(_params(layers), strict=False)
    assert not unexpected and all(k.startswith("fc.") for k in missing)
    return m.to(dev).eval()


def _err(y, ref):
    assert tuple(y.shape) == tuple(ref.shape)
    return float((y.detach().double().cpu() - ref).abs().max())


def test_folded_tiny_trunk_fp32(dev):
    from fcmf_framework.resnet_eval import FoldedTrunk
    _set(torch.float32)
    m, ref = _build(TINY, dev), _oracle(TINY, 3)
    y = FoldedTrunk(m)(synth.synth_crops(3, 64, seed=1).to(dev))
    assert y.dtype == torch.float32 and not y.requires_grad
    e, scale = _err(y, ref), float(ref.abs().max())
    print(f"MEASURED folded fp32 tiny: max error {e:.3e}, max|ref| {scale:.3e}, ratio {e / scale:.3e}")
    assert e <= 1e-4 * scale


def test_folded_width_not_a_multiple_of_32_fp32(dev):
    """base = 24: the 1 x 1 convolutions over 24 / 48 input channels cannot be read in place (the GEMM contracts over a multiple of
    32 columns) and take the patch-matrix path with its zero tail; same bound as the 64-wide trunk"""
    from fcmf_framework.resnet import ResNet
    from fcmf_framework.resnet_eval import FoldedTrunk
    _set(torch.float32)
    layers = (1, 1, 1, 1)
    P = synth.synth_resnet_params(synth.resnet_param_shapes(layers, base=24), 0)
    m = ResNet(layers, base=24)
    missing, unexpected = m.load_state_dict(P, strict=False)
    assert not unexpected and all(k.startswith("fc.") for k in missing)
    x = synth.synth_crops(2, 64, seed=1)
    ref = RO.resnet_trunk({k: (v.double() if v.is_floating_point() else v) for k, v in P.items()}, x.double(), layers).permute(0, 2, 3, 1)
    y = FoldedTrunk(m.to(dev).eval())(x.to(dev))
    e, scale = _err(y, ref.contiguous()), float(ref.abs().max())
    print(f"MEASURED folded fp32 base 24: max error {e:.3e}, max|ref| {scale:.3e}")
    assert e <= 1e-4 * scale


@pytest.mark.parametrize("layers,n", [(TINY, 3), (synth.RESNET152_LAYERS, 2)], ids=["tiny", "resnet152"])
def test_folded_trunk_bf16_no_worse_than_plain(dev, layers, n):
    from fcmf_framework.resnet_eval import FoldedTrunk
    _set(torch.bfloat16)
    try:
        m, ref = _build(layers, dev), _oracle(layers, n)
        x = synth.synth_crops(n, 64, seed=1).to(dev)
        with torch.no_grad():
            plain = m.trunk_nhwc(x)
        folded = FoldedTrunk(m)(x)
        assert folded.dtype == torch.bfloat16 and not folded.requires_grad
        e_plain, e_fold = _err(plain, ref), _err(folded, ref)
        print(f"MEASURED bf16 {layers}: e_fold {e_fold:.4e}, e_plain {e_plain:.4e}, max|ref| {float(ref.abs().max()):.4e}")
        assert e_fold <= 2.0 * e_plain
    finally:
        _set(torch.float32)


def test_refresh_is_explicit(dev):
    from fcmf_framework.resnet_eval import FoldedTrunk
    _set(torch.float32)
    m = _build(TINY, dev)
    x = synth.synth_crops(2, 64, seed=1).to(dev)
    f = FoldedTrunk(m)
    y0 = f(x).clone()
    with torch.no_grad():
        m.layer1[0].bn1.running_mean += 0.5
    assert torch.equal(f(x), y0)                     # the snapshot still holds the old statistics
    f.refresh()
    y1 = f(x)
    assert not torch.equal(y1, y0)
    assert torch.equal(y1, FoldedTrunk(m)(x))


def test_train_mode_is_refused(dev):
    from fcmf_framework import _hip as H
    from fcmf_framework.resnet_eval import FoldedTrunk
    _set(torch.float32)
    m = _build(TINY, dev)
    m.train()
    with pytest.raises(H.HipLibraryError):
        FoldedTrunk(m)
    m.eval()
    f = FoldedTrunk(m)
    m.layer2[0].bn2.train()                          # one BatchNorm back in train mode: refresh() refuses too
    with pytest.raises(H.HipLibraryError):
        f.refresh()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_folded_launch_sequence(dev, dtype):
    """no statistics launch, at most one apply-type launch per bottleneck plus the stem's, conv3 of every block one launch"""
    from fcmf_framework import _hip as H
    from fcmf_framework import resnet as R
    from fcmf_framework.resnet_eval import FoldedTrunk
    _set(dtype)
    try:
        m = _build(TINY, dev)
        x = synth.synth_crops(4, 64, seed=1).to(dev)
        f = FoldedTrunk(m)
        f(x)                                         # (the stem's weight shadow and the padded buffers exist after this)
        calls = _recorded(lambda: f(x))
    finally:
        _set(torch.float32)
    names = [c[0] for c in calls]
    print("MEASURED", dtype, len(names), " ".join(names))
    assert all(c[2] == 0 for c in calls)
    assert not [n for n in names if n.startswith("fcmf_bn_stats") or n.startswith("fcmf_bn_finalize")]
    blocks = [b for layer in (m.layer1, m.layer2, m.layer3, m.layer4) for b in layer]
    applies = [n for n in names if n in ("fcmf_bn_apply", "fcmf_bn_apply_pad")]
    assert 1 <= len(applies) <= len(blocks) + 1 and applies[0] == "fcmf_bn_apply"
    assert names.count("fcmf_bn_apply") == 1         # the stem's
    # conv3 + bn3 + identity + relu: ONE fcmf_gemm with FCMF_EPI_ADD_RELU per block, in block order, and nothing but the next
    # block's first GEMM (or the end of the pass) follows it
    EPI = 10                                         # position of `epilogue` among fcmf_gemm's scalar arguments
    conv3 = [i for i, c in enumerate(calls) if c[0] == "fcmf_gemm" and c[1][EPI] == H.EPI_ADD_RELU]
    assert len(conv3) == len(blocks)
    for i, b in zip(conv3, blocks):
        assert calls[i][1][1] == b.conv3.out_channels and calls[i][1][2] == b.conv3.in_channels
        assert i + 1 == len(calls) or calls[i + 1][0] == "fcmf_gemm"
    if dtype == torch.bfloat16:
        assert "fcmf_conv_im2col" not in names
        # every 3x3 convolution is one fcmf_conv_gemm_epi launch with FCMF_EPI_RELU (epilogue: its first scalar argument)
        relu3x3 = [c for c in calls if c[0] == "fcmf_conv_gemm_epi" and c[1][0] == H.EPI_RELU]
        assert len(relu3x3) == len(blocks) and all(c[1][7] == 3 for c in relu3x3)
