"""The R-Drop consistency term on the GPU (csrc/loss.hip: fcmf_symkl_fwd / fcmf_symkl_bwd): the kernels through their C entry
points at the smallest shapes that reach every branch, then ops.symmetric_kl, ops.vocab_cross_entropy(rdrop_alpha=) and the
models' loss_aspects / IAOGDecoder.loss, against torch on the CPU in float64 (tests/symkl_ref.py).

Tolerances are those of tests/test_loss_options_gpu.py for the same dtype and width: float32 1e-5 relative on a forward row at
the scale of the largest row and 2e-5 on the gradients, bf16 logits 2e-2 / 4e-2, wide rows 1e-6 / 4e-3 absolute on a gradient
whose entries stay within [-1, 1]."""
import pytest
import torch
import torch.nn.functional as F

import symkl_ref as R
import synthetic_data as synth
from helpers import _recorded, batch_to, build_fcmf, max_err, rel_err

pytestmark = pytest.mark.gpu

SENTINEL = 7.0
IGNORED = 3


def _H():
    from fcmf_framework import _hip
    return _hip


def _ops():
    from fcmf_framework import ops
    return ops


def _case(n, C, ld, dtype, seed, scale=2.0):
    """-> two logit buffers [n, ld] of dtype (CPU) and labels with pair IGNORED dead"""
    g = torch.Generator().manual_seed(seed)
    a = (torch.randn(n, ld, generator=g) * scale).to(dtype)
    b = (torch.randn(n, ld, generator=g) * scale).to(dtype)
    lb = torch.zeros(n, dtype=torch.long)
    lb[IGNORED] = -100
    return a, b, lb


def _fwd(H, a, b, C, lb, segments=1):
    n, ld = a.shape
    num = torch.full((n,), SENTINEL, device=a.device)
    den = torch.full((n,), SENTINEL, device=a.device)
    H.check(H.lib().fcmf_symkl_fwd(H.ptr(a), ld, H.ptr(b), ld, H.ptr(lb), H.ptr(num), H.ptr(den), n, C, segments, -100, H.dt(a),
                                   H.stream()), "fcmf_symkl_fwd")
    return num, den


def _bwd(H, a, b, C, lb, scales, grad, da, db, acc):
    n, ld = a.shape
    H.check(H.lib().fcmf_symkl_bwd(H.ptr(a), ld, H.ptr(b), ld, H.ptr(lb), H.ptr(da), da.shape[1], H.ptr(db), db.shape[1], H.ptr(scales),
                                   H.ptr(grad), n, C, scales.numel(), -100, acc, H.dt(a), H.stream()), "fcmf_symkl_bwd")


def _reference(a, b, C, live, scales, grad):
    """float64 rows k [n] (0 where dead) and the gradients of sum_r sc_r k_r, sc_r = scales[r % segments] * grad"""
    x = a[:, :C].detach().cpu().double().requires_grad_(True)
    y = b[:, :C].detach().cpu().double().requires_grad_(True)
    k = R.rows(x, y) * live.double()
    sc = scales.cpu().double()[torch.arange(x.shape[0]) % scales.numel()] * float(grad.item())
    ga, gb = torch.autograd.grad((k * sc).sum(), (x, y))
    return k.detach(), ga, gb


def _check_shape(dev, n, C, ld, dtype, wide, seed, scale=2.0):
    H = _H()
    f32 = dtype == torch.float32
    tol = 1e-5 if f32 else 2e-2
    ca, cb, lb = _case(n, C, ld, dtype, seed, scale)
    a, b = ca.to(dev), cb.to(dev)
    g = torch.Generator().manual_seed(seed + 1)
    for labels in (lb, None):
        live = torch.ones(n, dtype=torch.bool) if labels is None else labels != -100
        lbd = None if labels is None else labels.to(dev)
        for segments in (1, n):
            what = (n, C, ld, dtype, labels is None, segments)
            scales = (torch.rand(segments, generator=g) * 0.35 + 0.5).to(dev)
            grad = torch.full((1,), 1.0 if wide else 0.5, device=dev)
            num, den = _fwd(H, a, b, C, lbd, segments)
            rk, rga, rgb = _reference(a, b, C, live, scales, grad)
            assert torch.equal(den.cpu(), live.float()), what                    # the liveness itself
            assert max_err(num, rk) < tol * max(1.0, rk.abs().max().item()), what
            da, db = torch.full_like(a, SENTINEL), torch.full_like(b, SENTINEL)
            _bwd(H, a, b, C, lbd, scales, grad, da, db, 0)
            if wide:
                assert max(rga.abs().max().item(), rgb.abs().max().item()) <= 1.0
                gtol = 1e-6 if f32 else 4e-3
                assert max_err(da[:, :C], rga) < gtol and max_err(db[:, :C], rgb) < gtol, what
            else:
                assert rel_err(da[:, :C], rga) < 2 * tol and rel_err(db[:, :C], rgb) < 2 * tol, what
            assert (da[:, C:] == SENTINEL).all() and (db[:, C:] == SENTINEL).all(), what      # columns at or past C are not written
            if labels is not None:
                assert num[IGNORED].item() == 0.0 and not da[IGNORED, :C].any() and not db[IGNORED, :C].any(), what
            # acc = 1: prefill + gradient, each element read and written once; a dead pair's destination is left alone
            pa = (torch.rand(n, ld, generator=g) - 0.5).to(dtype).to(dev)
            pb = (torch.rand(n, ld, generator=g) - 0.5).to(dtype).to(dev)
            xa, xb = pa.clone(), pb.clone()
            _bwd(H, a, b, C, lbd, scales, grad, xa, xb, 1)
            wa, wb = pa[:, :C].cpu().double() + rga, pb[:, :C].cpu().double() + rgb
            # the kernel's own bound on the gradient, plus (bf16) the one more rounding of the sum: half an ulp, <= 2^-8 |v|, and
            # 2^-9 for the wide case's |v| < 1 (prefill within +-0.5, gradient far below 0.5)
            if wide:
                assert max(wa.abs().max().item(), wb.abs().max().item()) < 1.0
                atol = 1e-6 if f32 else 4e-3 + 2.0 ** -9
                assert max_err(xa[:, :C], wa) <= atol and max_err(xb[:, :C], wb) <= atol, what
            else:
                for got, want, rg in ((xa, wa, rga), (xb, wb, rgb)):
                    bound = 2 * tol * rg.abs().max().item() + (2.0 ** -23 if f32 else 2.0 ** -8) * want.abs().max().item()
                    assert max_err(got[:, :C], want) <= bound, what
            assert torch.equal(xa[:, C:], pa[:, C:]) and torch.equal(xb[:, C:], pb[:, C:]), what
            if labels is not None:
                assert torch.equal(xa[IGNORED], pa[IGNORED]) and torch.equal(xb[IGNORED], pb[IGNORED]), what


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [1, 3, 4, 65, 130, 1023])
def test_narrow_kernels(dev, dtype, C):
    """one wave per pair: 37 pairs (not a multiple of the 4 pairs of a block), one column up to 16 per lane"""
    _check_shape(dev, 37, C, C + 5, dtype, False, seed=C)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C,ld,n", [(1024, 1024, 9), (1500, 1504, 9), (2049, 2049, 9), (64001, 64032, 5)])
def test_wide_kernels(dev, dtype, C, ld, n):
    """one workgroup per pair: the threshold, a ragged tail behind the 16-byte chunks, an odd stride (element accesses), the IAOG
    vocabulary in its padded buffer.  Logits of scale 1: |dk/da_j| <= 1/2 p_j (|d_j - E_p d| + 1) + 1/2 q_j stays far below 1."""
    _check_shape(dev, n, C, ld, dtype, True, seed=C, scale=1.0)


@pytest.mark.parametrize("C", [4, 64001])
def test_offset_rows_keep_their_digits(dev, C):
    """b = a + 1e-2 noise + 8: k ~ 5e-5 sits 5 decades below the common offset of d = a - b.  Centred on max a - max b the
    float32 sums hold k to ~5e-5 relative; 1/2 (E_p d - E_q d) of the raw d is off by 6e-3 and more."""
    H = _H()
    n = 6
    g = torch.Generator().manual_seed(C)
    a = torch.randn(n, C, generator=g)
    b = a + 1e-2 * torch.randn(n, C, generator=g) + 8.0
    num, den = _fwd(H, a.to(dev), b.to(dev), C, None)
    want = R.rows(a, b)
    assert max_err(num, want) < 1e-3 * want.abs().max().item(), (num.cpu(), want)
    assert (den == 1).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C,ld", [(4, 9), (130, 135), (1500, 1504), (2049, 2049), (64001, 64032)])
def test_equal_rows_give_exact_zeros(dev, dtype, C, ld):
    """b a bitwise copy of a: k == 0 and both gradients all zero, exactly"""
    H = _H()
    n = 5
    a = (torch.randn(n, ld, generator=torch.Generator().manual_seed(C)) * 3).to(dtype).to(dev)
    b = a.clone()
    num, den = _fwd(H, a, b, C, None)
    assert not num.any() and (den == 1).all()
    da, db = torch.full_like(a, SENTINEL), torch.full_like(b, SENTINEL)
    _bwd(H, a, b, C, None, torch.full((1,), 0.75, device=dev), torch.ones(1, device=dev), da, db, 0)
    assert not da[:, :C].any() and not db[:, :C].any()
    assert (da[:, C:] == SENTINEL).all() and (db[:, C:] == SENTINEL).all()


def test_zero_scale_segment(dev):
    """a segment whose scale is 0 (no live pair): zeros with acc = 0, untouched with acc = 1"""
    H = _H()
    n, C = 6, 1500
    a, b, _ = _case(n, C, C, torch.float32, 1)
    a, b = a.to(dev), b.to(dev)
    scales = torch.tensor([0.5, 0.0], device=dev)
    da, db = torch.full_like(a, SENTINEL), torch.full_like(b, SENTINEL)
    _bwd(H, a, b, C, None, scales, None, da, db, 0)
    assert not da[1::2].any() and not db[1::2].any() and da[0::2].any()
    pa, pb = da.clone().fill_(SENTINEL), db.clone().fill_(SENTINEL)
    _bwd(H, a, b, C, None, scales, None, pa, pb, 1)
    assert (pa[1::2] == SENTINEL).all() and (pb[1::2] == SENTINEL).all() and not (pa[0::2] == SENTINEL).all()


def test_bad_arguments_launch_nothing(dev):
    """ld < C, n % segments != 0, an unsupported dtype, da aliasing a: an error code, and the outputs keep their sentinels"""
    H = _H()
    L = H.lib()
    n, C = 6, 5
    a, b = torch.randn(n, C, device=dev), torch.randn(n, C, device=dev)
    num, den = torch.full((n,), SENTINEL, device=dev), torch.full((n,), SENTINEL, device=dev)
    da, db = torch.full((n, C), SENTINEL, device=dev), torch.full((n, C), SENTINEL, device=dev)
    sc = torch.ones(n, device=dev)
    keep = a.clone()

    def fwd(lda=C, seg=1, dt=H.F32):
        return L.fcmf_symkl_fwd(H.ptr(a), lda, H.ptr(b), C, None, H.ptr(num), H.ptr(den), n, C, seg, -100, dt, H.stream())

    def bwd(lda=C, seg=1, dt=H.F32, da_=da, ldda=C):
        return L.fcmf_symkl_bwd(H.ptr(a), lda, H.ptr(b), C, None, H.ptr(da_), ldda, H.ptr(db), C, H.ptr(sc), None, n, C, seg, -100, 0, dt,
                                H.stream())

    for call in (fwd, bwd):
        assert call(lda=C - 1) == H.ERR_ARG and call(seg=4) == H.ERR_ARG and call(dt=H.F64) == H.ERR_UNSUPPORTED
    assert bwd(da_=a) == H.ERR_ARG and bwd(da_=b) == H.ERR_ARG and bwd(ldda=C - 1) == H.ERR_ARG
    torch.cuda.synchronize()
    assert (num == SENTINEL).all() and (den == SENTINEL).all() and (da == SENTINEL).all() and (db == SENTINEL).all()
    assert torch.equal(a, keep)


# ---- ops ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_symmetric_kl_op(dev, dtype):
    """ops.symmetric_kl on [B * A, C] = [10, 4] with segments = 5: value and both .grad; then with one operand detached"""
    ops = _ops()
    g = torch.Generator().manual_seed(11)
    ca, cb = ((torch.randn(10, 4, generator=g) * 2).to(dtype) for _ in range(2))
    lb = torch.zeros(10, dtype=torch.long)
    lb[7] = -100
    tol = 1e-5 if dtype == torch.float32 else 2e-2
    for labels in (None, lb):
        a, b = ca.to(dev).requires_grad_(True), cb.to(dev).requires_grad_(True)
        loss = ops.symmetric_kl(a, b, None if labels is None else labels.to(dev), alpha=0.7, segments=5)
        (loss * 3.0).backward()
        x, y = ca.double().requires_grad_(True), cb.double().requires_grad_(True)
        ref = R.loss(x, y, labels, alpha=0.7, segments=5)
        (ref * 3.0).backward()
        assert abs(loss.item() - ref.item()) < tol * abs(ref.item())
        assert rel_err(a.grad, x.grad) < 2 * tol and rel_err(b.grad, y.grad) < 2 * tol
        if labels is not None:
            assert not a.grad[7].any() and not b.grad[7].any()
        # one operand detached: the other's gradient is the same, the detached one gets none
        a2, b2 = ca.to(dev).requires_grad_(True), cb.to(dev)
        (ops.symmetric_kl(a2, b2, None if labels is None else labels.to(dev), alpha=0.7, segments=5) * 3.0).backward()
        assert torch.equal(a2.grad, a.grad) and b2.grad is None
        a3, b3 = ca.to(dev), cb.to(dev).requires_grad_(True)
        (ops.symmetric_kl(a3, b3, None if labels is None else labels.to(dev), alpha=0.7, segments=5) * 3.0).backward()
        assert torch.equal(b3.grad, b.grad) and a3.grad is None
    # a [B, A, C] view pair, as loss_aspects hands it over
    both = torch.cat((ca, cb)).view(4, 5, 4).to(dev).requires_grad_(True)
    ops.symmetric_kl(both[:2], both[2:], segments=5).backward()
    x = torch.cat((ca, cb)).view(4, 5, 4).double().requires_grad_(True)
    R.loss(x[:2], x[2:], segments=5).backward()
    assert rel_err(both.grad, x.grad) < 2 * tol


def test_symmetric_kl_refuses_with_a_reason(dev):
    ops, H = _ops(), _H()
    a = torch.zeros(10, 4, device=dev)
    for args, kw, why in (((a, torch.zeros(10, 5, device=dev)), {}, "shape"), ((a, torch.zeros(10, 4)), {}, "CPU"),
                          ((a, a.bfloat16()), {}, "float32"), ((a.double(), a.double()), {}, "float32"),
                          ((a, a), dict(segments=3), "segments"),
                          ((a, a, torch.zeros(9, dtype=torch.long, device=dev)), {}, "labels"),
                          ((a, a, torch.zeros(10, dtype=torch.int32, device=dev)), {}, "labels")):
        with pytest.raises(H.HipLibraryError, match=why):
            ops.symmetric_kl(*args, **kw)
    for kw, named in ((dict(alpha=-1.0), "alpha"), (dict(alpha=float("nan")), "alpha"), (dict(segments=0), "segments")):
        with pytest.raises(ValueError, match=named):
            ops.symmetric_kl(a, a, **kw)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_vocab_cross_entropy_rdrop(dev, dtype):
    """ops.vocab_cross_entropy(rdrop_alpha=0.7, label_smoothing=0.1) on the IAOG vocabulary: M = 5 pairs, one ignored position ==
    CE over the 2M rows with the labels repeated + 0.7 x the live pairs' mean symmetric KL, in float64: the loss and the
    gradients of x, W and b within tests/test_loss_options_gpu.py::test_vocab_cross_entropy_label_smoothing's bounds"""
    ops = _ops()
    ops.set_compute_dtype(dtype)
    ops.shadows.clear()
    try:
        V, K, M = 64001, 64, 5
        mk = lambda shape, scale, seed: (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale)
        w = mk((V, K), 0.3, 1).to(dev).requires_grad_(True)
        b = mk((V,), 0.1, 2).to(dev).requires_grad_(True)
        x = mk((2, M, K), 1.0, 3).to(dtype).to(dev).requires_grad_(True)
        lb = torch.randint(0, V, (M,), generator=torch.Generator().manual_seed(4))
        lb[-1] = -100
        loss = ops.vocab_cross_entropy(x, w, b, lb.to(dev), label_smoothing=0.1, rdrop_alpha=0.7)
        assert type(loss.grad_fn).__name__ == "VocabCrossEntropyRDropFnBackward"
        loss.backward()
        xr, wr, br = (t.detach().double().cpu().requires_grad_(True) for t in (x, w, b))
        wc = wr if dtype == torch.float32 else wr.bfloat16().double()
        lg = F.linear(xr.view(2 * M, K), wc, br)
        ref = F.cross_entropy(lg, torch.cat((lb, lb)), ignore_index=-100, label_smoothing=0.1) + R.loss(lg[:M], lg[M:], lb, alpha=0.7)
        ref.backward()
        tol = 1e-5 if dtype == torch.float32 else 2e-2
        assert abs(loss.item() - ref.item()) < tol * abs(ref.item())
        for got, want in ((x.grad, xr.grad.view(2, M, K)), (w.grad, wr.grad), (b.grad, br.grad)):
            assert rel_err(got, want) < (1e-4 if dtype == torch.float32 else 3e-2)
        with pytest.raises(_H().HipLibraryError, match="stacked"):
            ops.vocab_cross_entropy(x[0], w, b, lb.to(dev), rdrop_alpha=0.7)
    finally:
        ops.set_compute_dtype(torch.float32)
        ops.shadows.clear()


# ---- models ---------------------------------------------------------------------------------------------------------------------
NI, NR, B, S = 2, 5, 3, 16


@pytest.fixture(scope="module")
def tiny_fcmf(dev):
    model, _ = build_fcmf(synth.TINY_CFG, NI, NR, dev)
    batch = batch_to(synth.synth_batch(B, synth.TINY_CFG, S=S, num_imgs=NI, num_roi=NR, seed=42), dev)
    return model, batch


def _doubled_logits(model, b):
    two = lambda t: torch.cat((t, t), dim=0)
    return model.forward_aspects(two(b["input_ids"]), two(b["visual_embeds_att"]), two(b["roi_embeds_att"]), two(b["roi_coors"]),
                                 two(b["token_type_ids"]), two(b["attention_mask"]), two(b["added_attention_mask"]))


def _aspects_reference(logits, labels, alpha):
    """float64: sum over aspects of the batch-mean CE over all 2B rows with the labels repeated + alpha x the symmetric KL term"""
    x = logits.detach().cpu().double().requires_grad_(True)
    A, C = x.shape[1:]
    lb2 = torch.cat((labels, labels)).cpu()
    ce = sum(F.cross_entropy(x[:, a], lb2[:, a]) for a in range(A))
    Bh = labels.shape[0]
    kl = R.loss(x[:Bh], x[Bh:], alpha=alpha, segments=A)
    (ce + kl).backward()
    return (ce + kl).detach(), kl.detach(), x.grad


def test_fcmf_loss_aspects_rdrop(dev, tiny_fcmf):
    ops = _ops()
    model, b = tiny_fcmf
    ops.set_compute_dtype(torch.float32)
    model.train()
    try:
        ops.manual_seed(7)
        logits = _doubled_logits(model, b)
        assert logits.shape[0] == 2 * B
        # two copies of a review inside one batch get independent dropout masks: the halves differ for every review
        assert ((logits[:B] - logits[B:]).abs().amax(dim=(1, 2)) > 0).all()
        logits = logits.detach().requires_grad_(True)
        loss = model.loss_aspects(logits, b["labels"], rdrop_alpha=1.3)
        loss.backward()
        ref, kl, g = _aspects_reference(logits, b["labels"], 1.3)
        assert kl.item() > 0
        assert abs(loss.item() - ref.item()) < 1e-5 * abs(ref.item())
        assert rel_err(logits.grad, g) < 2e-5
        # with an option of ops.cross_entropy: the aspects stay the segments of both terms
        lg2 = logits.detach().requires_grad_(True)
        with_ls = model.loss_aspects(lg2, b["labels"], label_smoothing=0.1, rdrop_alpha=1.3)
        x = logits.detach().cpu().double()
        lb2 = torch.cat((b["labels"], b["labels"])).cpu()
        want = sum(F.cross_entropy(x[:, a], lb2[:, a], label_smoothing=0.1) for a in range(x.shape[1])) + kl
        assert abs(with_ls.item() - want.item()) < 1e-5 * abs(want.item())
        with pytest.raises(_H().HipLibraryError, match="two passes"):
            model.loss_aspects(logits[:B], b["labels"], rdrop_alpha=1.3)
    finally:
        model.eval()
    # eval(): no dropout, the two halves agree -- the KL term vanishes and the loss is the plain call's
    with torch.no_grad():
        logits = _doubled_logits(model, b)
        plain = model.loss_aspects(logits[:B], b["labels"])
        kl = ops.symmetric_kl(logits[:B], logits[B:], segments=logits.shape[1], alpha=1.3)
        both = model.loss_aspects(logits, b["labels"], rdrop_alpha=1.3)
    assert abs(kl.item()) <= 1e-6
    assert abs(both.item() - plain.item()) < 1e-5 * abs(plain.item())


def test_baseline_loss_aspects_rdrop(dev):
    from fcmf_framework.baselines import _Baseline
    g = torch.Generator().manual_seed(8)
    base = torch.randn(2 * 5, 6, 4, generator=g) * 2
    lb = torch.randint(0, 4, (5, 6), generator=g)
    lg = base.to(dev).requires_grad_(True)
    loss = _Baseline.loss_aspects(None, lg, lb.to(dev), rdrop_alpha=0.5)
    loss.backward()
    ref, _, gr = _aspects_reference(base, lb, 0.5)
    assert abs(loss.item() - ref.item()) < 1e-5 * abs(ref.item())
    assert rel_err(lg.grad, gr) < 2e-5


# ---- the default path -----------------------------------------------------------------------------------------------------------
def _calls(fn):
    return [c[0] for c in _recorded(fn)]


def test_defaults_never_reach_the_new_entry_points(dev, tiny_fcmf):
    """rdrop_alpha = 0 through loss_aspects and ops.vocab_cross_entropy: the bits of the calls without the argument, the same
    nodes and launches, neither new entry point among them"""
    from fcmf_framework.baselines import _Baseline
    from fcmf_framework.fcmf_multimodal import FCMF
    ops = _ops()
    g = torch.Generator().manual_seed(12)
    base = (torch.randn(5, 6, 4, generator=g) * 2).to(dev)
    lb = torch.randint(0, 4, (5, 6), generator=g).to(dev)
    for fn in (FCMF.loss_aspects, _Baseline.loss_aspects):
        for kw in ({}, dict(label_smoothing=0.1)):
            out = {}

            def run(key, **extra):
                lg = base.clone().requires_grad_(True)
                out[key] = fn(None, lg, lb, **kw, **extra)
                out[key].backward()
                out[key + "_grad"], out[key + "_node"] = lg.grad, type(out[key].grad_fn).__name__
            names0, names1 = _calls(lambda: run("plain")), _calls(lambda: run("zero", rdrop_alpha=0.0))
            assert names0 == names1 and not any("symkl" in n for n in names1)
            assert torch.equal(out["plain"], out["zero"]) and torch.equal(out["plain_grad"], out["zero_grad"])
            assert out["plain_node"] == out["zero_node"]
    V, K, M = 1999, 64, 6
    mk = lambda shape, scale, seed: (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale)
    w, bias = mk((V, K), 0.3, 1).to(dev), mk((V,), 0.1, 2).to(dev)
    x = mk((M, K), 1.0, 3).to(dev)
    vl = torch.randint(0, V, (M,), generator=g).to(dev)
    for kw, node in (({}, "VocabCrossEntropyFnBackward"), (dict(label_smoothing=0.1), "VocabCrossEntropyExFnBackward")):
        out = {}

        def run(key, **extra):
            xx = x.clone().requires_grad_(True)
            out[key] = ops.vocab_cross_entropy(xx, w, bias, vl, **kw, **extra)
            out[key].backward()
            out[key + "_grad"], out[key + "_node"] = xx.grad, type(out[key].grad_fn).__name__
        names0, names1 = _calls(lambda: run("plain")), _calls(lambda: run("zero", rdrop_alpha=0.0))
        assert names0 == names1 and not any("symkl" in n for n in names1)
        assert out["plain_node"] == out["zero_node"] == node
        assert torch.equal(out["plain"], out["zero"]) and torch.equal(out["plain_grad"], out["zero_grad"])
    # ... and the R-Drop node does reach them
    names = _calls(lambda: ops.vocab_cross_entropy(torch.cat((x, x)).requires_grad_(True), w, bias, vl, rdrop_alpha=0.5).backward())
    assert names.count("fcmf_symkl_fwd") == 1 and names.count("fcmf_symkl_bwd") == 1


def test_iaog_decoder_loss_default_and_rdrop(dev):
    """IAOGDecoder.loss / FCMFSeq2Seq.forward_loss: rdrop_alpha = 0 is the call without the argument, bit for bit and launch for
    launch; rdrop_alpha > 0 runs encoder and decoder twice at batch B under different seeds and adds a positive KL term"""
    from helpers import make_hf_dir
    from fcmf_framework.fcmf_pretraining import FCMFSeq2Seq
    ops = _ops()
    ops.set_compute_dtype(torch.float32)
    cfg = synth.TINY_CFG
    V = cfg["vocab_size"]
    model = FCMFSeq2Seq(V, 20, make_hf_dir(cfg), NI, NR, 1.0)
    model.decoder.embedding = torch.nn.Embedding(V, model.decoder.num_hiddens)   # run_pretraining_fcmf.py:189
    shapes = {k: v for k, v in synth.fcmf_param_shapes(cfg).items() if k.startswith("encoder.")}
    shapes.update(synth.iaog_decoder_param_shapes(cfg, V))
    model.load_state_dict(synth.synth_params(shapes), strict=False)
    model = model.to(dev).train()
    bt = batch_to(synth.synth_batch(B, cfg, S=S, num_imgs=NI, num_roi=NR, seed=5, coord_dtype=torch.float32), dev)
    gen = torch.Generator().manual_seed(6)
    dec_X = torch.randint(0, V, (B, 6), generator=gen).to(dev)
    labels = torch.randint(0, V, (B, 6), generator=gen)
    labels[:, -1] = -100
    labels = labels.to(dev)
    enc_X, tt, am, added = (bt[k][:, 0].contiguous() for k in ("input_ids", "token_type_ids", "attention_mask", "added_attention_mask"))

    def run(out, key, **extra):
        ops.manual_seed(21)
        model.zero_grad(set_to_none=True)
        out[key] = model.forward_loss(enc_X, dec_X, labels, bt["visual_embeds_att"], bt["roi_embeds_att"], bt["roi_coors"], tt, am, added,
                                      **extra)
        out[key].backward()
        out[key + "_grad"] = model.decoder.dense.weight.grad.clone()

    out = {}
    names0 = _calls(lambda: run(out, "plain"))
    names1 = _calls(lambda: run(out, "zero", rdrop_alpha=0.0))
    assert names0 == names1 and not any("symkl" in n for n in names1)
    assert torch.equal(out["plain"], out["zero"]) and torch.equal(out["plain_grad"], out["zero_grad"])
    names2 = _calls(lambda: run(out, "rdrop", rdrop_alpha=1.0))
    assert names2.count("fcmf_symkl_fwd") == 1 and names2.count("fcmf_symkl_bwd") == 1
    assert torch.isfinite(out["rdrop"]).item() and torch.isfinite(out["rdrop_grad"]).all()
    # the KL term is what the two differently seeded passes disagree by: positive in train(), and the loss is not the plain one
    assert out["rdrop"].item() != out["plain"].item()
    # the decoder alone, on one encoder state: loss(rdrop_alpha) = CE over both passes + alpha x KL >= the mean CE, and alpha scales it
    with torch.no_grad():
        state, _ = model._decoder_state(enc_X, bt["visual_embeds_att"], bt["roi_embeds_att"], bt["roi_coors"], tt, am, added)
        ops.manual_seed(33)
        plain = model.decoder.loss(dec_X, state, labels)
        ops.manual_seed(33)
        assert torch.equal(plain, model.decoder.loss(dec_X, state, labels, rdrop_alpha=0.0))
        ops.manual_seed(33)
        l0 = model.decoder.loss(dec_X, state, labels, rdrop_alpha=1e-30)      # (both passes' CE, a KL term below float32's reach)
        ops.manual_seed(33)
        l1 = model.decoder.loss(dec_X, state, labels, rdrop_alpha=1.0)
        ops.manual_seed(33)
        l2 = model.decoder.loss(dec_X, state, labels, rdrop_alpha=2.0)
    kl = l1.item() - l0.item()
    assert kl > 0 and abs((l2.item() - l0.item()) - 2 * kl) < 1e-4 * max(kl, abs(l0.item()) * 1e-2)
