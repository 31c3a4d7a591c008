"""Class weights, label smoothing and the focal factor of the training loss on the GPU (csrc/loss.hip): the kernels through
their C entry points at the smallest shapes that reach every branch, then ops.cross_entropy / ops.vocab_cross_entropy and the
models' loss_aspects, against torch on the CPU in float64 (tests/loss_ref.py).

Tolerances are those of tests/test_ops_gpu.py::test_cross_entropy*: float32 1e-5 relative on the loss and 2e-5 on the gradients,
bf16 logits 2e-2 / 4e-2, wide rows 1e-6 / 4e-3 absolute on a gradient whose entries stay within [-1, 1].  A forward row is a
summand of the loss and is held to the loss's relative bound at the scale of the largest row."""
import pytest
import torch
import torch.nn.functional as F

import loss_ref as R
from helpers import _recorded, max_err, rel_err

pytestmark = pytest.mark.gpu

OPTIONS = [(0.0, 0.0), (0.1, 0.0), (0.0, 2.0), (0.0, 0.5)]      # (label smoothing, focal exponent)
SENTINEL = 7.0
CONFIDENT = 2                                                    # the row whose label holds all but ~3e-7 of the probability


def _H():
    from fcmf_framework import _hip
    return _hip


def _case(n, C, ld, dtype, segments, seed):
    """-> logits buffer [n, ld] of dtype (CPU), labels, weights [C] and [segments, C] in [0.5, 1] (CPU float32).  Row 1's label is
    C - 1, row 3 is ignored, and row CONFIDENT's label sits 15 above the log-sum-exp of the row's other logits: 1 - p_y ~ 3e-7."""
    g = torch.Generator().manual_seed(seed)
    buf = torch.randn(n, ld, generator=g) * 2.0
    lb = torch.randint(0, C, (n,), generator=g)
    lb[1] = C - 1
    lb[3] = -100
    y = int(lb[CONFIDENT])
    others = torch.cat((buf[CONFIDENT, :y], buf[CONFIDENT, y + 1:C])).double()
    buf[CONFIDENT, y] = float(torch.logsumexp(others, 0)) + 15.0
    w1 = torch.rand(C, generator=g) * 0.5 + 0.5
    ws = torch.rand(segments, C, generator=g) * 0.5 + 0.5
    return buf.to(dtype), lb, w1, ws


def _kernels(H, dev, buf, C, lb, weight, segments, eps, gamma, scales, grad, in_place):
    """the three entry points on the buffer's first C columns -> (num, den, dlogits buffer [n, ld])"""
    n, ld = buf.shape
    L = H.lib()
    lbd = lb.to(dev)
    wd = None if weight is None else weight.to(dev).contiguous()
    wstride = 0 if weight is None or weight.dim() == 1 else C
    num = torch.full((n,), SENTINEL, device=dev)
    den = torch.full((n,), SENTINEL, device=dev)
    H.check(L.fcmf_xent_fwd_ex(H.ptr(buf), ld, H.ptr(lbd), H.ptr(wd), wstride, H.ptr(num), H.ptr(den), n, C, segments, -100, eps, gamma,
                               H.dt(buf), H.stream()), "fcmf_xent_fwd_ex")
    d = buf.clone() if in_place else torch.full_like(buf, SENTINEL)
    src = d if in_place else buf
    H.check(L.fcmf_xent_bwd_ex(H.ptr(src), ld, H.ptr(lbd), H.ptr(wd), wstride, H.ptr(d), ld, H.ptr(scales), H.ptr(grad), n, C, segments,
                               -100, eps, gamma, H.dt(buf), H.stream()), "fcmf_xent_bwd_ex")
    return num, den, d


def _reference(buf, C, lb, weight, segments, eps, gamma, scales, grad):
    x = buf[:, :C].detach().cpu().double().requires_grad_(True)
    num, den = R.loss_rows(x, lb, weight, eps, gamma, segments)
    sc = scales.cpu().double()[torch.arange(x.shape[0]) % segments] * float(grad.item())
    g, = torch.autograd.grad((num * sc).sum(), x)
    return num.detach(), den.detach(), g


def _check_shape(dev, n, C, ld, dtype, wide, seed):
    H = _H()
    segments = n                                                 # one row per segment: every weight row and scale is indexed
    cpu_buf, lb, w1, ws = _case(n, C, ld, dtype, segments, seed)
    buf = cpu_buf.to(dev)
    g = torch.Generator().manual_seed(seed + 1)
    f32 = dtype == torch.float32
    tol = 1e-5 if f32 else 2e-2
    for weight, seg in ((None, 1), (w1, 1), (ws, segments)):
        scales = (torch.rand(seg, generator=g) * 0.35 + 0.5).to(dev)     # <= 0.85: a focal row's gradient reaches 1.13 w_y before it
        grad = torch.full((1,), 1.0 if wide else 0.5, device=dev)
        for eps, gamma in OPTIONS:
            what = (C, ld, dtype, None if weight is None else tuple(weight.shape), eps, gamma)
            num, den, d = _kernels(H, dev, buf, C, lb, weight, seg, eps, gamma, scales, grad, False)
            rnum, rden, rg = _reference(buf, C, lb, weight, seg, eps, gamma, scales, grad)
            assert torch.equal(den.cpu().double(), rden), what   # the label's weight itself; 0 for the ignored row
            assert num[3].item() == 0.0 and not d[3, :C].any(), what
            assert max_err(num, rnum) < tol * max(1.0, rnum.abs().max().item()), what
            if wide:
                assert rg.abs().max().item() <= 1.0
                assert max_err(d[:, :C], rg) < (1e-6 if f32 else 4e-3), what
            else:
                assert rel_err(d[:, :C], rg) < 2 * tol, what
            assert (d[:, C:] == SENTINEL).all(), what            # columns at or past C are not written
            # the confident row on its own scale: 1 - p_y ~ 3e-7 carries the focal factor and the label's gradient, and its
            # inputs are exact in both dtypes; float32 arithmetic on it is good to ~1e-5, 1.0f - p_y would be off by ~20 %
            r = CONFIDENT
            assert abs(num[r].item() - rnum[r].item()) < 1e-3 * abs(rnum[r].item()), what
            assert max_err(d[r, :C], rg[r]) < (1e-3 if f32 else 1e-2) * rg[r].abs().max().item(), what
            if wide:
                _, _, dip = _kernels(H, dev, buf, C, lb, weight, seg, eps, gamma, scales, grad, True)
                assert torch.equal(dip[:, :C], d[:, :C]), what   # in place == out of place
                assert torch.equal(dip[:, C:], buf[:, C:]), what # ... and the padding columns keep the logits


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [3, 4, 65, 130, 1023])
def test_narrow_kernels(dev, dtype, C):
    """one wave per row: 37 rows (not a multiple of the 4 rows of a block), fewer classes than lanes up to 16 per lane"""
    _check_shape(dev, 37, C, C + 5, dtype, False, seed=C)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C,ld,n", [(1024, 1024, 9), (1500, 1504, 9), (2049, 2049, 9), (64001, 64032, 5)])
def test_wide_kernels(dev, dtype, C, ld, n):
    """one workgroup per row: the threshold, a ragged tail behind the 16-byte chunks, an odd stride (element accesses), the IAOG
    vocabulary in its padded buffer (whose [segments, C] weight rows are not 16-byte aligned); in place and out of place"""
    _check_shape(dev, n, C, ld, dtype, True, seed=C)


def test_reduce_is_per_segment_and_fixed_order(dev):
    H = _H()
    n, S = 390, 6
    g = torch.Generator().manual_seed(5)
    num, den = torch.rand(n, generator=g) * 3, torch.rand(n, generator=g) + 0.5
    den[4::S] = 0.0
    num[4::S] = 0.0                                              # segment 4 has no live weight
    out = torch.full((1 + S,), SENTINEL, device=dev)
    nd, dd = num.to(dev), den.to(dev)
    H.check(H.lib().fcmf_xent_reduce_ex(H.ptr(nd), H.ptr(dd), n, S, 2.0, H.ptr(out), H.ptr(out[1:]), H.stream()), "reduce")
    assert torch.isnan(out[0]).item() and out[5].item() == 0.0   # 0 / 0 as torch; its rows get a zero scale
    live = [s for s in range(S) if s != 4]
    want = torch.tensor([2.0 / den[s::S].double().sum().item() for s in live])
    assert rel_err(out[1:][live], want) < 1e-6
    den[4::S] = 1.0
    dd = den.to(dev)
    first = None
    for _ in range(3):
        H.check(H.lib().fcmf_xent_reduce_ex(H.ptr(nd), H.ptr(dd), n, S, 2.0, H.ptr(out), H.ptr(out[1:]), H.stream()), "reduce")
        first = out.clone() if first is None else first
        assert torch.equal(out, first)
    want = 2.0 * sum(num[s::S].double().sum() / den[s::S].double().sum() for s in range(S))
    assert abs(out[0].item() - want.item()) < 1e-6 * want.item()


def _ops():
    from fcmf_framework import ops
    return ops


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("eps,gamma", OPTIONS)
def test_cross_entropy_segments_and_weights(dev, dtype, eps, gamma):
    """ops.cross_entropy(segments=6, weight=[6, 4]) over 384 rows = the sum of six criteria, each with its own weight row"""
    ops = _ops()
    n, C, A = 384, 4, 6
    g = torch.Generator().manual_seed(1)
    lg = (torch.randn(n, C, generator=g) * 2).to(dtype).to(dev).requires_grad_(True)
    lb = torch.randint(0, C, (n,), generator=g)
    lb[::7] = -100
    w = torch.rand(A, C, generator=g) + 0.5
    loss = ops.cross_entropy(lg, lb.to(dev), weight=w.to(dev), label_smoothing=eps, focal_gamma=gamma, segments=A)
    (loss * 3.0).backward()
    x = lg.detach().cpu().double().requires_grad_(True)
    if gamma == 0.0:
        ref = sum(F.cross_entropy(x[a::A], lb[a::A], weight=w[a].double(), label_smoothing=eps, ignore_index=-100) for a in range(A))
    else:
        ref = R.loss_ref(x, lb, w, eps, gamma, A)
    (ref * 3.0).backward()
    tol = 1e-5 if dtype == torch.float32 else 2e-2
    assert abs(loss.item() - ref.item()) < tol * abs(ref.item())
    assert rel_err(lg.grad, x.grad) < 2 * tol
    # a shared [C] weight and `mult`
    lg.grad = None
    loss = ops.cross_entropy(lg, lb.to(dev), mult=0.5, weight=w[0].to(dev), label_smoothing=eps, focal_gamma=gamma, segments=A)
    loss.backward()
    x.grad = None
    ref = R.loss_ref(x, lb, w[0], eps, gamma, A, mult=0.5)
    ref.backward()
    assert abs(loss.item() - ref.item()) < tol * abs(ref.item())
    assert rel_err(lg.grad, x.grad) < 2 * tol


def test_cross_entropy_dead_segment(dev):
    """every row of one segment ignored: NaN loss as torch, zero gradient rows there (and finite ones elsewhere)"""
    ops = _ops()
    n, C, A = 48, 4, 6
    g = torch.Generator().manual_seed(2)
    lg = (torch.randn(n, C, generator=g) * 2).to(dev).requires_grad_(True)
    lb = torch.randint(0, C, (n,), generator=g)
    lb[2::A] = -100
    w = (torch.rand(A, C, generator=g) + 0.5).to(dev)
    loss = ops.cross_entropy(lg, lb.to(dev), weight=w, label_smoothing=0.1, segments=A)
    assert torch.isnan(loss).item()
    assert torch.isnan(R.loss_ref(lg.detach().cpu().double(), lb, w.cpu(), 0.1, 0.0, A)).item()
    loss.backward()
    assert not lg.grad[2::A].any()
    rest = torch.ones(n, dtype=torch.bool)
    rest[2::A] = False
    assert torch.isfinite(lg.grad[rest]).all() and lg.grad[rest].abs().sum(1).min().item() > 0
    # a segment whose live rows all carry weight 0
    lb2 = torch.randint(0, C - 1, (n,), generator=g)
    w0 = torch.ones(C, device=dev)
    w0[:C - 1] = 0.0
    lg.grad = None
    dead = ops.cross_entropy(lg, lb2.to(dev), weight=w0)
    assert torch.isnan(dead).item()
    dead.backward()
    assert not lg.grad.any()


def test_defaults_take_the_plain_path(dev):
    """every option at its default: the plain node, the plain launches, the same bits as a call that names none"""
    ops = _ops()
    g = torch.Generator().manual_seed(3)
    lb = torch.randint(0, 4, (384,), generator=g).to(dev)
    base = (torch.randn(384, 4, generator=g) * 2).to(dev)

    def run(**kw):
        lg = base.clone().requires_grad_(True)
        out = {}

        def go():
            out["loss"] = ops.cross_entropy(lg, lb, -100, 6.0, **kw)
            out["loss"].backward()
        names = [c[0] for c in _recorded(go)]
        return out["loss"].detach(), lg.grad, names, type(out["loss"].grad_fn).__name__

    plain = run()
    named = run(weight=None, label_smoothing=0.0, focal_gamma=0.0, segments=1)
    assert plain[2] == named[2] == ["fcmf_xent_fwd", "fcmf_xent_mean", "fcmf_xent_bwd"]
    assert plain[3] == named[3] == "XentFnBackward"
    assert torch.equal(plain[0], named[0]) and torch.equal(plain[1], named[1])
    ex = run(segments=6)
    assert ex[2] == ["fcmf_xent_fwd_ex", "fcmf_xent_reduce_ex", "fcmf_xent_bwd_ex"] and ex[3] == "XentExFnBackward"


def test_weight_is_checked_with_a_reason(dev):
    ops, H = _ops(), _H()
    lg, lb = torch.zeros(12, 4, device=dev), torch.zeros(12, dtype=torch.long, device=dev)
    for w, why in ((torch.ones(4), "cpu"), (torch.ones(5, device=dev), "shape"), (torch.ones(3, 4, device=dev), "shape"),
                   (torch.ones(4, device=dev, dtype=torch.float64), "float32"), ([1.0, 1.0, 1.0, 1.0], "tensor")):
        with pytest.raises(H.HipLibraryError, match=why):
            ops.cross_entropy(lg, lb, weight=w, segments=2)
    with pytest.raises(H.HipLibraryError, match="segments"):
        ops.cross_entropy(lg, lb, segments=5)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_vocab_cross_entropy_label_smoothing(dev, dtype):
    """ops.vocab_cross_entropy(label_smoothing=0.1) at tests/test_ops_gpu.py::test_vocab_cross_entropy_fused_node's geometry ==
    F.cross_entropy(F.linear(...).permute(0, 2, 1), label_smoothing=0.1): value and the gradients of x, W and b; then the same
    with class weights over the vocabulary"""
    ops = _ops()
    ops.set_compute_dtype(dtype)
    ops.shadows.clear()
    try:
        V, K, B, Ld = 1999, 64, 3, 5
        mk = lambda shape, scale, seed: (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale)
        w = mk((V, K), 0.3, 1).to(dev).requires_grad_(True)
        b = mk((V,), 0.1, 2).to(dev).requires_grad_(True)
        x = mk((B, Ld, K), 1.0, 3).to(dtype).to(dev).requires_grad_(True)
        lb = torch.randint(0, V, (B, Ld), generator=torch.Generator().manual_seed(4))
        lb[:, -1] = -100
        cw = torch.rand(V, generator=torch.Generator().manual_seed(5)) + 0.5
        xr, wr, br = (a.detach().float().cpu().requires_grad_(True) for a in (x, w, b))
        wc = wr if dtype == torch.float32 else wr.bfloat16().float()
        tol = 1e-5 if dtype == torch.float32 else 2e-2
        for class_weight in (None, cw):
            for t in (x, w, b, xr, wr, br):
                t.grad = None
            loss = ops.vocab_cross_entropy(x, w, b, lb.to(dev), label_smoothing=0.1,
                                           class_weight=None if class_weight is None else class_weight.to(dev))
            assert type(loss.grad_fn).__name__ == "VocabCrossEntropyExFnBackward"
            loss.backward()
            ref = F.cross_entropy(F.linear(xr, wc, br).permute(0, 2, 1), lb, weight=class_weight, ignore_index=-100, label_smoothing=0.1)
            ref.backward()
            assert abs(loss.item() - ref.item()) < tol * abs(ref.item())
            for got, want in ((x.grad, xr.grad), (w.grad, wr.grad), (b.grad, br.grad)):
                assert rel_err(got, want) < (1e-4 if dtype == torch.float32 else 3e-2)
        plain = ops.vocab_cross_entropy(x, w, b, lb.to(dev), label_smoothing=0.0, class_weight=None)
        assert type(plain.grad_fn).__name__ == "VocabCrossEntropyFnBackward"
        assert torch.equal(plain, ops.vocab_cross_entropy(x, w, b, lb.to(dev)))
    finally:
        ops.set_compute_dtype(torch.float32)
        ops.shadows.clear()


def test_loss_aspects_options(dev):
    """FCMF.loss_aspects and the baselines' loss_aspects with options: the aspects are the segments; without options the plain call"""
    from fcmf_framework.baselines import _Baseline
    from fcmf_framework.fcmf_multimodal import FCMF
    B, A, C = 5, 6, 4
    g = torch.Generator().manual_seed(6)
    base = torch.randn(B, A, C, generator=g) * 2
    lb = torch.randint(0, C, (B, A), generator=g)
    w = torch.rand(A, C, generator=g) + 0.5
    for fn in (FCMF.loss_aspects, _Baseline.loss_aspects):
        for kw in (dict(weight=w.to(dev)), dict(label_smoothing=0.1), dict(weight=w[0].to(dev), focal_gamma=2.0)):
            lg = base.to(dev).requires_grad_(True)
            loss = fn(None, lg, lb.to(dev), **kw)
            loss.backward()
            x = base.double().reshape(B * A, C).requires_grad_(True)
            ref = R.loss_ref(x, lb.reshape(-1), None if "weight" not in kw else kw["weight"].cpu(), kw.get("label_smoothing", 0.0),
                             kw.get("focal_gamma", 0.0), A)
            ref.backward()
            assert abs(loss.item() - ref.item()) < 1e-5 * abs(ref.item())
            assert rel_err(lg.grad.reshape(B * A, C), x.grad) < 2e-5
        lg = base.to(dev)
        assert torch.equal(fn(None, lg, lb.to(dev)), fn(None, lg, lb.to(dev), weight=None, label_smoothing=0.0, focal_gamma=0.0))
