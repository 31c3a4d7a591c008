"""The category classifiers' training pieces on the GPU: the BCE-with-logits kernel, one full training step of a small ResNet
with the 5-way head (image mode: BCE, ROI mode: cross entropy) against a float64 restatement built from oracle/resnet_oracle.py,
FusedAdamW(weight_decay=0) against torch.optim.Adam, eval mode on the running statistics, and ResNet-152 memorising a batch."""
import pytest
import torch
import torch.nn.functional as F

import synthetic_data as synth
from oracle import resnet_oracle as RO

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
SMALL = (1, 1, 1, 1)


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


def _rel(got, ref):
    return ((got.detach().double().cpu() - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


# ---- 1. the BCE kernel ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 64, 256])
@pytest.mark.parametrize("ldt", ["dense", "strided"])
def test_bce_with_logits_matches_float64(dev, n, ldt):
    from fcmf_framework import ops
    g = torch.Generator().manual_seed(n)
    C = 5
    x = torch.randn(n, C, generator=g, dtype=torch.float64) * 6
    x[0, 0], x[-1, 1] = 100.0, -100.0                       # saturated logits: the stable form, no inf / nan
    y = (torch.rand(n, C, generator=g) < 0.4).double()
    xd = x.float().to(dev)
    if ldt == "strided":                                    # logits with a leading dimension (a slice of a wider matrix)
        xd = torch.cat([xd, torch.zeros(n, 3, device=dev)], 1)[:, :C]
    xd.requires_grad_(True)
    loss = ops.bce_with_logits(xd, y.float().to(dev))
    (2.5 * loss).backward()
    xr = x.float().double().requires_grad_(True)
    lr = F.binary_cross_entropy_with_logits(xr, y)
    (2.5 * lr).backward()
    assert abs(loss.item() - lr.item()) <= 1e-6 * max(1.0, abs(lr.item()))
    assert _rel(xd.grad, xr.grad) < 1e-5
    assert torch.isfinite(xd.grad).all()
    p = ops.sigmoid(xd.detach())
    assert (p.double().cpu() - torch.sigmoid(x.float().double())).abs().max().item() < 1e-6


def test_bce_with_logits_bf16_logits(dev):
    from fcmf_framework import ops
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(64, 5, generator=g) * 4).to(BF16)
    y = (torch.rand(64, 5, generator=g) < 0.5).float()
    xd = x.to(dev).requires_grad_(True)
    loss = ops.bce_with_logits(xd, y.to(dev))
    loss.backward()
    xr = x.double().requires_grad_(True)
    F.binary_cross_entropy_with_logits(xr, y.double()).backward()
    assert abs(loss.item() - F.binary_cross_entropy_with_logits(x.double(), y.double()).item()) < 1e-6
    assert xd.grad.dtype == BF16 and _rel(xd.grad, xr.grad) < 8e-3


# ---- 2. one training step of a small ResNet classifier against float64 ---------------------------------------------------
def _small_model(cls_name, dev):
    from fcmf_framework import categories as CAT
    from fcmf_framework.resnet import ResNet
    P = synth.synth_resnet_params(synth.resnet_param_shapes(SMALL), 0)
    m = getattr(CAT, cls_name)(5, ResNet(SMALL))
    m.feature_extractor.load_state_dict(P, strict=False)
    g = torch.Generator().manual_seed(9)
    m.linear.weight.data = torch.randn(5, 2048, generator=g) * 0.05
    m.linear.bias.data = torch.randn(5, generator=g) * 0.1
    return m.to(dev), P


def _oracle(P, head_w, head_b, x, target, mode, training, q):
    Pd = {k: (q(v) if v.dim() == 4 else v.double()).requires_grad_(v.dtype.is_floating_point and "running" not in k)
          if v.dtype.is_floating_point else v.clone() for k, v in P.items()}
    W, b = q(head_w).requires_grad_(True), head_b.double().requires_grad_(True)
    feat = RO.resnet_trunk(Pd, q(x), SMALL, training=training).mean(3).mean(2)
    logits = q(feat) @ W.t() + b
    loss = F.binary_cross_entropy_with_logits(logits, target.double()) if mode == "image" else F.cross_entropy(logits, target)
    loss.backward()
    grads = {"feature_extractor." + k: v.grad for k, v in Pd.items() if torch.is_tensor(v) and v.requires_grad}
    grads["linear.weight"], grads["linear.bias"] = W.grad, b.grad
    return logits.detach(), loss.detach(), grads


# fp32: every quantity within 1e-3 relative (max |err| / max |ref|; measured 1.3e-6 logits, 5.4e-6 worst parameter).
# bf16: logits, loss and the head's gradients within 3e-2 (measured 2.2e-2 logits); the trunk's gradients by their global
# relative L2 error within 0.35 (measured 0.19).  test_resnet_bwd_gpu.py measures 8e-3 per bottleneck block with the ReLU
# decisions pinned to the kernel's; unpinned float64 ReLUs send full gradient values down the other branch wherever a bf16
# value rounds across zero, 0.16 - 0.59 for one block there -- the fp32 case is the exact check of the same code.
@pytest.mark.parametrize("mode", ["image", "roi"])
def test_one_training_step_matches_float64(dev, dtype, mode):
    from fcmf_framework import ops
    m, P = _small_model("MyImgModel" if mode == "image" else "MyRoIModel", dev)
    m.train()
    g = torch.Generator().manual_seed(11)
    x = torch.randn(4, 3, 64, 64, generator=g)
    target = (torch.rand(4, 5, generator=g) < 0.4).float() if mode == "image" else torch.tensor([0, 3, 4, 3])
    q = (lambda t: t.to(BF16).double()) if dtype == BF16 else (lambda t: t.double())
    xin = x.to(dtype).to(dev)
    logits = m(xin)
    loss = ops.bce_with_logits(logits, target.to(dev)) if mode == "image" else ops.cross_entropy(logits, target.to(dev))
    loss.backward()
    r_logits, r_loss, r_grads = _oracle(P, m.linear.weight.detach().cpu(), m.linear.bias.detach().cpu(), x, target, mode, True, q)
    got = {n: p.grad for n, p in m.named_parameters()}
    assert set(r_grads) <= set(got) and all(got[k] is not None for k in r_grads)
    assert got["feature_extractor.fc.weight"] is None
    e_log, e_loss = _rel(logits.float(), r_logits), abs(loss.item() - r_loss.item()) / max(1e-3, abs(r_loss.item()))
    a = torch.cat([got[k].double().cpu().flatten() for k in r_grads])
    b = torch.cat([r_grads[k].flatten() for k in r_grads])
    e_l2 = ((a - b).norm() / b.norm()).item()
    e_max, where = max((_rel(got[k], r_grads[k]), k) for k in r_grads)
    print(f"MEASURED step {mode} {dtype}: logits {e_log:.3e} loss {e_loss:.3e} grad global L2 {e_l2:.3e} worst param {e_max:.3e} ({where})")
    if dtype == F32:
        assert e_log < 1e-3 and e_loss < 1e-3 and e_max < 1e-3, (e_log, e_loss, e_max, where)
    else:
        e_head = max(_rel(got[k], r_grads[k]) for k in ("linear.weight", "linear.bias"))
        assert e_log < 3e-2 and e_loss < 3e-2 and e_head < 3e-2 and e_l2 < 0.35, (e_log, e_loss, e_head, e_l2)


def test_eval_mode_uses_running_statistics(dev):
    m, P = _small_model("MyImgModel", dev)
    m.eval()
    x = torch.randn(3, 3, 64, 64, generator=torch.Generator().manual_seed(12))
    with torch.no_grad():
        got = m(x.to(dev))
    q = lambda t: t.double()
    ref = RO.resnet_trunk({k: v.double() if v.dtype.is_floating_point else v for k, v in P.items()}, x.double(), SMALL,
                          training=False).mean(3).mean(2) @ q(m.linear.weight.detach().cpu()).t() + m.linear.bias.detach().cpu().double()
    assert _rel(got, ref) < 1e-4
    rm = m.feature_extractor.bn1.running_mean.detach().cpu().clone()
    with torch.no_grad():
        m(x.to(dev))
    assert torch.equal(rm, m.feature_extractor.bn1.running_mean.detach().cpu())       # eval never moves the statistics
    # and train mode does: the batch statistics, not the running ones
    m.train()
    with torch.no_grad():
        t = m(x.to(dev))
    assert _rel(t, ref) > 1e-2


# ---- 3. the optimizer ----------------------------------------------------------------------------------------------------
def test_fused_adamw_without_decay_is_adam(dev):
    from fcmf_framework.optimization import FusedAdamW
    g = torch.Generator().manual_seed(13)
    shapes = [(5, 2048), (5,), (64, 3, 7, 7), (70000,)]
    init = [torch.randn(s, generator=g) for s in shapes]
    grads = [[torch.randn(s, generator=g) for s in shapes] for _ in range(3)]
    pd = [p.clone().to(dev).requires_grad_(True) for p in init]
    pc = [p.clone().requires_grad_(True) for p in init]
    od = FusedAdamW(pd, lr=3e-4, weight_decay=0.0)
    oc = torch.optim.Adam(pc, lr=3e-4)
    for step in range(3):
        for p, q, gr in zip(pd, pc, grads[step]):
            p.grad, q.grad = gr.to(dev), gr.clone()
        od.step()
        oc.step()
    for p, q in zip(pd, pc):
        assert (p.detach().cpu() - q.detach()).abs().max().item() < 1e-6


# ---- 4. ResNet-152 memorises a fixed batch -------------------------------------------------------------------------------
MEMO_STEPS = 30


def test_resnet152_classifier_memorises_a_batch(dev, dtype):
    """8 crops, 5 multi-label targets, Adam lr 1e-4: the loss falls from 0.71 to below 0.05 within 30 steps"""
    from fcmf_framework import categories as CAT
    from fcmf_framework import ops
    from fcmf_framework.optimization import FusedAdamW
    from fcmf_framework.resnet import ResNet
    torch.manual_seed(0)
    m = CAT.MyImgModel(5, ResNet(synth.RESNET152_LAYERS))
    m.feature_extractor.load_state_dict(synth.synth_resnet_params(synth.resnet_param_shapes(synth.RESNET152_LAYERS), 0), strict=False)
    m = m.to(dev).train()
    x = synth.synth_crops(8, 224, seed=3).to(dtype).to(dev)
    y = (torch.rand(8, 5, generator=torch.Generator().manual_seed(4)) < 0.4).float().to(dev)
    opt = FusedAdamW(m.parameters(), lr=1e-4, weight_decay=0.0)
    losses = []
    for _ in range(MEMO_STEPS):
        loss = ops.bce_with_logits(m(x), y)
        loss.backward()
        opt.step()
        opt.zero_grad()
        losses.append(loss.item())
    print(f"MEASURED memorise {dtype}: " + " ".join(f"{v:.3f}" for v in losses))
    assert all(v == v for v in losses)
    assert min(losses[-5:]) < 0.05, losses          # measured 0.004 (fp32) / 0.005 (bf16) after 30 steps, from 0.71
