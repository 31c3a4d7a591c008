"""ResNet-152 trunk backward (--fine_tune_cnn), op by op, against float64 CPU autograd.

Every case hands the reference exactly what the kernel saw: in bf16 mode the bf16-rounded activations, gradients and
weights, upcast to float64, so the error measured is the kernel's own.  Errors are max |kernel - reference| / max |reference|.

Tolerances are 2-3x the worst error measured on an MI355X over the cases of each test (the "measured" figure next to each):
  * fp32: the GEMMs accumulate in fp32, col2im / the pooling gathers sum at most 9 / 4 / 4 terms in fp32;
  * bf16-stored outputs (dX, BatchNorm dy, pooling dx): one rounding to bf16 (2^-9 relative) on top of that;
  * float32 outputs computed from bf16 operands (dW, dgamma, dbeta): fp32 accumulation only.
"""
import pytest
import torch
import torch.nn.functional as F

import synthetic_data as synth
from oracle import resnet_oracle as RO

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16


def _set(dtype):
    from fcmf_framework import ops
    ops.set_compute_dtype(dtype)
    ops.shadows.clear()


@pytest.fixture(params=[F32, BF16], ids=["fp32", "bf16"])
def dtype(request):
    _set(request.param)
    try:
        yield request.param
    finally:
        _set(F32)


def _rand(shape, seed, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float64) * scale + shift


def _q(t, dtype):
    """what a kernel of compute dtype `dtype` reads of t, as float64"""
    return t.to(dtype).double()


def _rel(got, ref):
    return ((got.detach().double().cpu() - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


def _nchw(v):
    return v.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def _report(name, **errs):
    print(f"MEASURED {name} " + " ".join(f"{k}={v:.3e}" for k, v in errs.items()))


# ------------------------------------------------------------------------------------------------------------------------
# 1. convolution backward: conv2d_bwd_nhwc (dX through the direct GEMM or GEMM + col2im, dW = dY^T A added into grads)
# ------------------------------------------------------------------------------------------------------------------------
# fp32 measured: dX 1.7e-6, dW 4.8e-7 (bound 5e-6 / 1.5e-6).  bf16 measured: dX 3.7e-3 (bf16 roundings of dA, then of the
# col2im sum), dW 2.4e-7 (bound 8e-3 / 1e-6).
CONV_TOL = {F32: (5e-6, 1.5e-6), BF16: (8e-3, 1e-6)}

CONV_CASES = [       # name, Cin, Cout, k, stride, pad, N, H, W
    ("stem_37x40", 3, 64, 7, 2, 3, 2, 37, 40),          # generic im2col from the strided NCHW float32 crops, Kpad 160 != K 147
    ("stem_224", 3, 64, 7, 2, 3, 2, 224, 224),
    ("1x1_64_256", 64, 256, 1, 1, 0, 2, 56, 56),        # direct path (A = the activation itself)
    ("1x1_64_256_add", 64, 256, 1, 1, 0, 2, 56, 56),    # ... with the EPI_ADD epilogue (layer1.0's two branches)
    ("1x1s2_256_15", 256, 512, 1, 2, 0, 2, 15, 15),     # col2im with kh = 1: odd rows / columns of dX are exactly 0
    ("1x1s2_256_14", 256, 512, 1, 2, 0, 2, 14, 14),
    ("1x1s2_1024_14", 1024, 2048, 1, 2, 0, 2, 14, 14),
    ("3x3_64_56", 64, 64, 3, 1, 1, 2, 56, 56),          # col2im, 9 overlapping windows
    ("3x3_512_7", 512, 512, 3, 1, 1, 2, 7, 7),
    ("3x3s2_128_56", 128, 128, 3, 2, 1, 2, 56, 56),     # strided col2im, borders
    ("3x3s2_256_15", 256, 256, 3, 2, 1, 2, 15, 15),
    ("3x3s2_512_14", 512, 512, 3, 2, 1, 2, 14, 14),
    ("3x3_c12", 12, 16, 3, 1, 1, 2, 9, 11),             # generic im2col (C % 8 != 0), Kpad 128 != K 108, col2im through Kpad
]


@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv2d_bwd_matches_float64_autograd(dev, dtype, case):
    from fcmf_framework import resnet as R
    name, cin, cout, k, st, pad, N, Hh, Ww = case
    stem, add = name.startswith("stem"), name.endswith("_add")
    conv = R.Conv2d(cin, cout, k, stride=st, padding=pad, bias=False)
    conv.weight.data = _rand(conv.weight.shape, 1, (2.0 / (cout * k * k)) ** 0.5).float()
    conv = conv.to(dev)
    Ho, Wo = (Hh + 2 * pad - k) // st + 1, (Ww + 2 * pad - k) // st + 1
    x = _rand((N, cin, Hh, Ww), 2)
    dy = _rand((N, cout, Ho, Wo), 3)
    extra = _rand((N, cin, Hh, Ww), 4) if add else None
    # reference on exactly the kernel's operands
    xr = _q(x, dtype).requires_grad_(True)
    wr = _q(conv.weight.detach().cpu(), dtype).requires_grad_(True)
    dyr = _q(dy, dtype)
    F.conv2d(xr, wr, stride=st, padding=pad).backward(dyr)
    dw_ref = wr.grad
    pre = 0.5 * dw_ref.abs().max() * _rand(dw_ref.shape, 5)            # dW is ADDED into an existing gradient
    grads = {conv.weight: pre.float().to(dev)}
    pre_used = grads[conv.weight].double().cpu()
    dyd = _nhwc(dy).contiguous().to(dtype).to(dev)
    if stem:       # as _trunk_backward calls it: the float32 NCHW crops through a strided NHWC view, no dX
        xs = x.float().to(dev)
        v = xs.permute(0, 2, 3, 1)
        assert R.conv2d_bwd_nhwc(conv, v, dyd, grads, need_dx=False, src_strides=v.stride()) is None
        dx = None
    else:
        xd = _nhwc(x).contiguous().to(dtype).to(dev)
        addd = _nhwc(extra).contiguous().to(dtype).to(dev) if add else None
        dx = R.conv2d_bwd_nhwc(conv, xd, dyd, grads, add=addd)
    tol_x, tol_w = CONV_TOL[dtype]
    errs = {"dW": _rel(grads[conv.weight].double().cpu() - pre_used, dw_ref)}
    if dx is not None:
        assert dx.shape == (N, Hh, Ww, cin) and dx.dtype == dtype
        dx_ref = xr.grad + (_q(extra, dtype) if add else 0)
        errs["dX"] = _rel(_nchw(dx), dx_ref)
        if st == 2 and k == 1 and Hh % 2 == 1:
            # a strided 1x1 convolution never reads the odd rows / columns: their gradient is exactly zero
            assert (dx[:, 1::2] == 0).all() and (dx[:, :, 1::2] == 0).all()
    _report(f"conv {name} {dtype}", **errs)
    assert errs["dW"] < tol_w, errs
    if dx is not None:
        assert errs["dX"] < tol_x, errs


# ------------------------------------------------------------------------------------------------------------------------
# 2. BatchNorm(+ReLU) backward: batchnorm_nhwc_(..., save=rec) then batchnorm_bwd_nhwc_
# ------------------------------------------------------------------------------------------------------------------------
def _bn_chunking(rpg, groups, C):
    """bn_chunking of csrc/conv.hip restated: -> (chunks per group, rows per chunk)"""
    slabs = (C + 255) // 256
    chunks = -(-1024 // (slabs * groups))
    chunk = min(max(-(-rpg // chunks), 16), 4096)
    return -(-rpg // chunk), chunk


# fp32 measured: dy 1.6e-7, dgamma / dbeta 1.5e-7 (bound 5e-7 / 5e-7).  bf16 measured: dy 3.7e-3 (one bf16 rounding),
# dgamma / dbeta 1.8e-7 (bound 8e-3 / 5e-7).
BN_TOL = {F32: (5e-7, 5e-7), BF16: (8e-3, 5e-7)}

BN_CASES = [        # name, C, groups, crops per group, H, W, chunking
    ("c64_g1_one_chunk", 64, 1, 1, 3, 4, "one"),
    ("c128_g3_one_chunk", 128, 3, 2, 2, 3, "one"),
    ("c64_g1_ragged", 64, 1, 2, 25, 20, "ragged"),
    ("c256_g3_ragged", 256, 3, 2, 15, 15, "ragged"),
    ("c1024_g3_ragged", 1024, 3, 1, 14, 14, "ragged"),
    ("c2048_g3_ragged_chunk37", 2048, 3, 2, 28, 28, "ragged"),
    ("c2048_g2_layer4", 2048, 2, 2, 7, 7, "ragged"),           # layer4: 49 rows per crop
    ("c2048_g1_layer4", 2048, 1, 3, 7, 7, "ragged"),
    ("c512_g2_layer4_one_crop", 512, 2, 1, 7, 7, "ragged"),  # layer4 bn1 / bn2 with one crop per group: 49 rows
]
BN_MODES = ["relu", "plain_gres", "residual_gres"]    # bn1/bn2; the downsample BN (no ReLU); bn3: relu(bn(y) + identity)


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("mode", BN_MODES)
@pytest.mark.parametrize("case", BN_CASES, ids=[c[0] for c in BN_CASES])
def test_batchnorm_bwd_matches_float64_autograd(dev, dtype, case, mode, training):
    from fcmf_framework import resnet as R
    name, C, groups, B, Hh, Ww, chunking = case
    N, rpg = groups * B, B * Hh * Ww
    chunks, chunk = _bn_chunking(rpg, groups, C)
    if chunking == "one":
        assert chunks == 1
    else:
        assert chunks > 1 and rpg % chunk != 0, (chunks, chunk)
    relu, res, want_gres = mode != "plain_gres", mode == "residual_gres", mode != "relu"
    bn = R.BatchNorm2d(C)
    bn.weight.data = (1 + 0.2 * _rand((C,), 10)).float()
    bn.bias.data = (0.2 * _rand((C,), 11)).float()
    bn.running_mean.data = (0.3 * _rand((C,), 12)).float()
    bn.running_var.data = (0.5 + torch.rand(C, generator=torch.Generator().manual_seed(13))).float()
    rm0, rv0 = bn.running_mean.double().clone(), bn.running_var.double().clone()
    bn = bn.to(dev).train(training)
    y = _rand((N, Hh, Ww, C), 14, 1.3, 0.4).to(dtype).to(dev)
    r = _rand((N, Hh, Ww, C), 15).to(dtype).to(dev) if res else None
    rec = {}
    z = R.batchnorm_nhwc_(y, bn, groups, res=r, relu=relu, out=torch.empty_like(y), save=rec)
    g = _rand((N, Hh, Ww, C), 16, 1.0, 0.3).to(dtype).to(dev)       # (non-zero mean: the mean-gradient term matters)
    g0 = g.double().cpu()
    pw, pb = _rand((C,), 17).float(), _rand((C,), 18).float()
    grads = {bn.weight: pw.to(dev), bn.bias: pb.to(dev)}
    dy, gres = R.batchnorm_bwd_nhwc_(bn, rec, g, y, z if relu else None, grads, want_gres=want_gres)
    assert dy.data_ptr() == g.data_ptr()                              # written in place over g
    # reference: the ReLU mask is the kernel's own z (this compares the BatchNorm backward, not signs of near-zero values)
    mask = (z.double().cpu() > 0).double() if relu else torch.ones_like(g0)
    yr = _nchw(y.double().cpu()).clone().requires_grad_(True)
    wr, br = bn.weight.detach().double().cpu().requires_grad_(True), bn.bias.detach().double().cpu().requires_grad_(True)
    if training:
        out = torch.cat([F.batch_norm(yg, None, None, wr, br, True, 0.0, bn.eps) for yg in yr.chunk(groups, 0)], 0)
    else:
        out = F.batch_norm(yr, rm0, rv0, wr, br, False, 0.0, bn.eps)
    (out * _nchw(g0 * mask)).sum().backward()          # (+ residual: it shifts z, i.e. the mask, not d out / d y)
    tol_y, tol_p = BN_TOL[dtype]
    errs = {"dy": _rel(_nchw(dy), yr.grad),
            "dgamma": _rel(grads[bn.weight].cpu().double() - pw.double(), wr.grad),
            "dbeta": _rel(grads[bn.bias].cpu().double() - pb.double(), br.grad)}
    _report(f"bn {name} {mode} {'train' if training else 'eval'} {dtype}", **errs)
    assert errs["dy"] < tol_y and errs["dgamma"] < tol_p and errs["dbeta"] < tol_p, errs
    if want_gres:       # the gradient on into the identity branch: g masked by the ReLU, bit-exact
        assert gres.data_ptr() != dy.data_ptr()
        assert torch.equal(gres.double().cpu(), g0 * mask)
    else:
        assert gres is None


# ------------------------------------------------------------------------------------------------------------------------
# 3. max-pool 3x3 / stride 2 / pad 1 backward (first-maximum tie rule)
# ------------------------------------------------------------------------------------------------------------------------
def _maxpool_bwd_ref(x, dy, last=False):
    """float64 NCHW reference: every window's gradient to its first (last=True: last) maximum in scan order r, then s"""
    N, C, Hh, Ww = x.shape
    Ho, Wo = dy.shape[2], dy.shape[3]
    cols = F.unfold(F.pad(x, (1, 1, 1, 1), value=float("-inf")), 3, stride=2).view(N, C, 9, Ho * Wo)
    k = (8 - cols.flip(2).argmax(2)) if last else cols.argmax(2)          # argmax returns the first maximum
    ho = torch.arange(Ho).repeat_interleave(Wo).expand_as(k)
    wo = torch.arange(Wo).repeat(Ho).expand_as(k)
    h, w = 2 * ho + k // 3 - 1, 2 * wo + k % 3 - 1
    dx = torch.zeros(N, C, Hh * Ww, dtype=torch.float64)
    dx.scatter_add_(2, h * Ww + w, dy.reshape(N, C, -1))
    return dx.view(N, C, Hh, Ww)


# fp32 measured 8.7e-8 (<= 4 fp32 additions); bf16 measured 2.8e-3 (one rounding of the sum to bf16).
POOL_TOL = {F32: 3e-7, BF16: 8e-3}


@pytest.mark.parametrize("C", [4, 64])
@pytest.mark.parametrize("hw", [(112, 112), (13, 16), (3, 5), (2, 2), (1, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", ["continuous", "ties"])
def test_maxpool_bwd_first_maximum(dev, dtype, kind, hw, C):
    from fcmf_framework import resnet as R
    Hh, Ww = hw
    N = 2
    Ho, Wo = (Hh - 1) // 2 + 1, (Ww - 1) // 2 + 1
    if kind == "ties":       # post-ReLU integers in {0, 1, 2}: many ties, all-zero windows
        x = torch.randint(0, 3, (N, C, Hh, Ww), generator=torch.Generator().manual_seed(20)).double()
    else:
        x = _rand((N, C, Hh, Ww), 21)
    x = _q(x, dtype)
    dy = _q(_rand((N, C, Ho, Wo), 22), dtype)
    ref = _maxpool_bwd_ref(x, dy)
    # the reference is torch's max_pool2d backward (first maximum on CPU, both memory formats)
    for fmt in (torch.contiguous_format, torch.channels_last):
        xa = x.clone(memory_format=fmt).requires_grad_(True)
        F.max_pool2d(xa, 3, 2, 1).backward(dy.contiguous(memory_format=fmt))
        assert torch.equal(xa.grad, ref)
    tol = POOL_TOL[dtype]
    if kind == "ties" and Hh * Ww > 4:
        # teeth: a last-maximum kernel would be far outside the tolerance
        assert _rel(_maxpool_bwd_ref(x, dy, last=True), ref) > 100 * tol
    xd = _nhwc(x).contiguous().to(dtype).to(dev)
    dx = R.maxpool3x3s2_bwd_nhwc(xd, _nhwc(dy).contiguous().to(dtype).to(dev))
    assert dx.shape == xd.shape and dx.dtype == dtype
    e = _rel(_nchw(dx), ref)
    _report(f"maxpool {kind} {Hh}x{Ww} C{C} {dtype}", dx=e)
    assert e < tol


# ------------------------------------------------------------------------------------------------------------------------
# 4. adaptive average-pool backward (AvgPoolFn: both output layouts, overlapping windows)
# ------------------------------------------------------------------------------------------------------------------------
# fp32 measured 7.5e-8 (<= 4 fp32 terms per input pixel); bf16 measured 3.5e-3 (one rounding to bf16).
AVG_TOL = {F32: 3e-7, BF16: 8e-3}


@pytest.mark.parametrize("tokens", [False, True], ids=["nchw", "tokens"])
@pytest.mark.parametrize("geom", [(7, 7, 7, 7), (7, 7, 1, 1), (7, 7, 2, 2), (13, 16, 3, 5)], ids=lambda g: "%dx%d_to_%dx%d" % g)
def test_adaptive_avgpool_bwd(dev, dtype, geom, tokens):
    from fcmf_framework import resnet as R
    Hh, Ww, oh, ow = geom
    N, C = 2, 64
    x = _q(_rand((N, C, Hh, Ww), 30), dtype)
    xd = _nhwc(x).contiguous().to(dtype).to(dev).requires_grad_(True)
    y = R.AvgPoolFn.apply(xd, oh, ow, tokens)
    xr = x.clone().requires_grad_(True)
    yr = F.adaptive_avg_pool2d(xr, (oh, ow))
    if tokens:
        yr = yr.flatten(2).transpose(1, 2)
    assert y.shape == yr.shape and y.dtype == torch.float32
    assert _rel(y, yr.detach()) < 1e-5
    dy = _rand(tuple(yr.shape), 31).float()
    y.backward(dy.to(dev))
    yr.backward(dy.double())
    e = _rel(_nchw(xd.grad), xr.grad)
    _report(f"avgpool {geom} tokens={tokens} {dtype}", dx=e)
    assert xd.grad.dtype == dtype and e < AVG_TOL[dtype]


# 5. one bottleneck: forward_rec + backward_rec against float64 autograd of the oracle's _bottleneck
# ------------------------------------------------------------------------------------------------------------------------
# Worst relative error over the input gradient and every parameter gradient of the block, with the reference's three ReLUs
# masked by the kernel's own z1 / z2 / z3 (as in section 2): with float64 ReLUs, the few outputs that round across zero send a
# full gradient value down the other branch, and the input-gradient error of a bf16 block is then 0.16 - 0.59.
# fp32 measured 1.6e-6 (bound 5e-6); bf16 measured 8.0e-3 over the three blocks, train and eval (bound 2.5e-2).
BLOCK_TOL = {F32: 5e-6, BF16: 2.5e-2}
BLOCKS = [         # name, block, stride, H = W of its input
    ("layer1.0_downsample_s1", "layer1.0", 1, 56),     # stride-1 downsample: conv1's dX GEMM adds the downsample's (EPI_ADD)
    ("layer2.0_downsample_s2", "layer2.0", 2, 56),     # strided: col2im output added by conv1's GEMM
    ("layer2.1_identity", "layer2.1", 1, 28),
]


def _bn_mean_detached(x, w, b, groups, eps=1e-5):
    """wrong twin of a train-mode BatchNorm: the mean-gradient term of its backward dropped"""
    outs = []
    for xg in x.chunk(groups, 0):
        mu = xg.mean((0, 2, 3), keepdim=True)
        var = xg.var((0, 2, 3), unbiased=False, keepdim=True)
        outs.append((xg - mu.detach()) * (var + eps).rsqrt() * w.view(1, -1, 1, 1) + b.view(1, -1, 1, 1))
    return torch.cat(outs, 0)


def _bottleneck_ref(P, p, x, stride, training, groups, masks=None, twin=None):
    """RO._bottleneck with its ReLUs optionally replaced by fixed masks (the kernel's), and optionally one deliberate defect:
    twin='mean': BatchNorm's mean-gradient term dropped (training); twin='gres': the gradient into the identity branch not
    masked by the final ReLU"""
    relu = [F.relu] * 3 if masks is None else [(lambda t, m=m: t * m) for m in masks]

    def bn(prefix, t):
        if twin == "mean":
            return _bn_mean_detached(t, P[prefix + ".weight"], P[prefix + ".bias"], groups)
        return RO._bn(P, prefix, t, training, groups)
    out = relu[0](bn(p + ".bn1", F.conv2d(x, P[p + ".conv1.weight"])))
    out = relu[1](bn(p + ".bn2", F.conv2d(out, P[p + ".conv2.weight"], stride=stride, padding=1)))
    out = bn(p + ".bn3", F.conv2d(out, P[p + ".conv3.weight"]))
    if (p + ".downsample.0.weight") in P:
        x = bn(p + ".downsample.1", F.conv2d(x, P[p + ".downsample.0.weight"], stride=stride))
    if twin == "gres":
        return relu[2](out + x.detach()) + (x - x.detach())
    return relu[2](out + x)


def _block_grads(fn, P, p, x, g):
    """-> {name: gradient} of sum(fn(P, x) * g) for the block's parameters and its input"""
    Pg = {k: (v.clone().requires_grad_(True) if k.startswith(p + ".") and "running" not in k and "num_batches" not in k else v.clone())
          for k, v in P.items()}
    xr = x.clone().requires_grad_(True)
    (fn(Pg, xr) * g).sum().backward()
    out = {k[len(p) + 1:]: v.grad for k, v in Pg.items() if v.requires_grad}
    out["input"] = xr.grad
    return out


def _worst(got, ref):
    return max((_rel(got[k], ref[k]), k) for k in ref)


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("block", BLOCKS, ids=[b[0] for b in BLOCKS])
def test_bottleneck_bwd_matches_oracle_autograd(dev, dtype, block, training):
    """bf16: the worst-gradient error of one block is 8e-3 (measured above), against 0.77 and more for either wrong twin.
    So the 0.963 cosine of test_resnet_gpu.test_fine_tune_cnn_bf16_runs_and_is_close is bf16 rounding compounded through its
    blocks (and ReLU / max-pool decisions that flip with it), not a defect of the backward."""
    from fcmf_framework.resnet import ResNet
    name, p, stride, hw = block
    groups, B = 2, 2
    layers = (1, 2, 1, 1)
    P = synth.synth_resnet_params(synth.resnet_param_shapes(layers), 0)
    m = ResNet(layers)
    m.load_state_dict(P, strict=False)
    m = m.to(dev).train(training)
    blk = m.get_submodule(p)
    cin = blk.conv1.in_channels
    # the kernel's operands: bf16 convolution weights (float32 BatchNorm parameters), bf16 input and output gradient
    Pr = {k: (_q(v, dtype) if v.dim() == 4 else v.double()) for k, v in P.items()}
    x = _q(_rand((groups * B, cin, hw, hw), 40).clamp_min(0), dtype)      # a post-ReLU activation
    ho = (hw - 1) // stride + 1
    g = _q(_rand((groups * B, blk.conv3.out_channels, ho, ho), 41, 1.0, 0.2), dtype)
    tape = []
    with torch.no_grad():
        blk.forward_rec(_nhwc(x).contiguous().to(dtype).to(dev), groups, tape)
    masks = [(_nchw(tape[0][z]).double().cpu() > 0).double() for z in ("z1", "z2", "z3")]
    grads = {}
    dx = blk.backward_rec(tape[0], _nhwc(g).contiguous().to(dtype).to(dev), grads)
    got = {n: grads[q] for n, q in blk.named_parameters()}
    got["input"] = _nchw(dx)
    # the restatement IS the oracle's block when nothing is substituted
    Pc = {k: v.clone() for k, v in Pr.items()}
    assert torch.equal(_bottleneck_ref(Pc, p, x, stride, training, groups), RO._bottleneck({k: v.clone() for k, v in Pr.items()}, p, x, stride,
                                                                                          training, groups))

    def ref_fn(twin=None):
        return lambda Pg, xr: _bottleneck_ref(Pg, p, xr, stride, training, groups, masks, twin)
    ref = _block_grads(ref_fn(), Pr, p, x, g)
    assert set(ref) == set(got)
    err, where = _worst(got, ref)
    tol = BLOCK_TOL[dtype]
    twins = {t: _worst(_block_grads(ref_fn(t), Pr, p, x, g), ref)[0] for t in (("mean", "gres") if training else ("gres",))}
    _report(f"block {name} {'train' if training else 'eval'} {dtype}", worst=err, **{f"twin_{t}": e for t, e in twins.items()})
    assert err < tol, (err, where)
    for t, e in twins.items():       # teeth: a backward with either defect would be far outside the bound
        assert e > 10 * BLOCK_TOL[BF16], (t, e)


# ------------------------------------------------------------------------------------------------------------------------
# 6. full depth, fp32: ResNet-152 on 224 x 224 crops through myResNetImg(..., if_fine_tune=True)
# ------------------------------------------------------------------------------------------------------------------------
def _grad_errors(got, ref):
    """-> (global relative L2 error over all gradients, worst per-parameter relative L2 error, worst per-parameter max error)"""
    a = torch.cat([got[k].detach().double().cpu().flatten() for k in ref])
    b = torch.cat([ref[k].flatten() for k in ref])
    per = [((got[k].detach().double().cpu() - ref[k]).norm() / ref[k].norm()).item() for k in ref]
    return ((a - b).norm() / b.norm()).item(), max(per), max(_rel(got[k], ref[k]) for k in ref)


def test_resnet152_224_fine_tune_gradients_fp32(dev):
    """The real geometry: 112 -> 56 max-pool, 56 / 28 / 14 / 7 maps, layer4's 49-row BatchNorm groups (1 crop per group).

    At this depth the train-mode gradient is ill-conditioned: torch's own float32 CPU autograd of the oracle lands 0.23 (worst
    parameter, max-norm) / 1.4e-2 (global L2) from float64, so no fp32 implementation can meet a 2e-3 worst-parameter bound
    against float64.  The test therefore computes that float32 CPU baseline too (the reference ~3 s, the baseline ~1 s of CPU)
    and requires the kernels to be no worse than 2x it, and within ~3x of their own measured errors: global L2 measured
    1.6e-2 (bound 5e-2; float32 CPU 1.4e-2), worst per-parameter L2 2.0e-2 (bound 6e-2; float32 CPU 2.2e-2), worst
    per-parameter max-norm 0.24 (float32 CPU 0.23)."""
    from fcmf_framework.resnet import ResNet
    from fcmf_framework.resnet_utils import myResNetImg
    _set(F32)
    layers, groups = synth.RESNET152_LAYERS, 2
    P = synth.synth_resnet_params(synth.resnet_param_shapes(layers), 0)
    m = ResNet(layers)
    m.load_state_dict(P, strict=False)
    m = m.to(dev).train()
    x = synth.synth_crops(groups, 224, seed=50)
    w = _rand((groups, 2048, 7, 7), 51)
    names = [k for k in P if "running" not in k and "num_batches" not in k]

    def oracle_grads(dt):
        Po = {k: (v.to(dt).clone().requires_grad_(k in names) if v.dtype.is_floating_point else v.clone()) for k, v in P.items()}
        (RO.my_resnet_img(Po, x.to(dt), layers, 7, training=True, groups=groups) * w.to(dt)).sum().backward()
        return {k: Po[k].grad for k in names}
    ref, f32 = oracle_grads(torch.float64), oracle_grads(torch.float32)
    img = myResNetImg(m, True, dev).train()
    y = img.forward_groups(x.to(dev), groups, att_size=7)
    (y * w.float().to(dev)).sum().backward()
    got = {n: p.grad for n, p in img.resnet.named_parameters() if not n.startswith("fc.")}
    assert set(got) == set(names) and all(g is not None for g in got.values())
    e_l2, e_par, e_max = _grad_errors(got, ref)
    b_l2, b_par, b_max = _grad_errors(f32, ref)
    _report("resnet152 224 fp32", global_l2=e_l2, param_l2=e_par, param_max=e_max, cpu32_global_l2=b_l2, cpu32_param_l2=b_par,
            cpu32_param_max=b_max)
    assert e_l2 < 5e-2 and e_par < 6e-2, (e_l2, e_par)
    assert e_l2 < 2 * b_l2 and e_par < 2 * b_par and e_max < 2 * b_max, ((e_l2, e_par, e_max), (b_l2, b_par, b_max))
