"""FusedAdamW (fcmf_multi_sumsq + fcmf_multi_adamw, csrc/misc.hip) against float64 AdamW with the global-norm clip, at tensor
sizes around and beyond the 65536-element chunk, with parameters and gradients that are not 16-byte aligned (the scalar path
for whole chunks), and with the bf16 shadows the update kernel writes in the same pass."""
import math

import numpy as np
import pytest
import torch

import rowwise_ref as R

pytestmark = pytest.mark.gpu

CHUNK = 65536
SIZES = [CHUNK + 5, 3 * CHUNK, CHUNK - 1, 7, 1]      # a chunk + a tail of 5 (4-wide + scalar), whole chunks, one short of a chunk, tiny
GROUP = [0, 1, 0, 1, 0]
LR, WD = (7e-5, 7e-4), (0.01, 0.0)
P_OFF, G_OFF = [1, 2, 3, 1, 2], [0, 3, 1, 0, 3]      # element offsets into the flat buffers of the unaligned layout
SENTINEL = 12345.0


def _f32(x):
    """a hyper-parameter as the kernel receives it: the C ABI takes lr, weight decay, the betas and eps as `float`.  The float64
    reference must start from these, as it starts from the bf16 values a bf16 kernel reads: 1 - beta2 is ill-conditioned in
    beta2 (float32(0.999) = 0.999 + 1.3e-8 makes it 1.3e-5 smaller, relatively), and so is every exp_avg_sq."""
    return float(np.float32(x))


def _randn(n, seed, scale=1.0):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed)) * scale


def max_err(a, b):
    return (a.double() - b.double()).abs().max().item()


def _bits(t):
    return t.detach().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _grads(step, scales):
    return [_randn(n, 100 + 10 * step + i, scales[step]) for i, n in enumerate(SIZES)]


def _place(values, offsets, dev):
    """each tensor as a view `off` elements into its own sentinel-filled flat buffer (off = 0 everywhere: plain aligned tensors)"""
    flats, views = [], []
    for v, off in zip(values, offsets):
        flat = torch.full((v.numel() + 8,), SENTINEL, device=dev)
        flat[off:off + v.numel()] = v.to(dev)
        flats.append(flat)
        views.append(flat[off:off + v.numel()])
    return flats, views


def _frames_intact(flats, offsets):
    for flat, off, n in zip(flats, offsets, SIZES):
        assert bool((flat[:off] == SENTINEL).all()) and bool((flat[off + n:] == SENTINEL).all())


def _trajectory(dev, p_off, g_off, max_norm, scales):
    """len(scales) FusedAdamW steps -> per step (parameters, exp_avg, exp_avg_sq, grad norm) on the CPU; the bf16 shadows
    (taken before the first step) are checked after every step"""
    from fcmf_framework import ops
    from fcmf_framework.optimization import FusedAdamW
    ops.shadows.clear()
    try:
        pflats, pviews = _place([_randn(n, i) for i, n in enumerate(SIZES)], p_off, dev)
        ps = [torch.nn.Parameter(v) for v in pviews]
        assert all(p.data_ptr() % 16 == 4 * off for p, off in zip(ps, p_off))
        opt = FusedAdamW([dict(params=[p for p, g in zip(ps, GROUP) if g == k], lr=LR[k], weight_decay=WD[k]) for k in (0, 1)], lr=1e-3)
        shadows = [ops.shadows.get(p) for p in ps]
        for p, s in zip(ps, shadows):
            assert torch.equal(_bits(s), _bits(p.detach().bfloat16()))
        out = []
        for step in range(len(scales)):
            gflats, gviews = _place(_grads(step, scales), g_off, dev)
            for p, g in zip(ps, gviews):
                p.grad = g
            opt.step(max_grad_norm=max_norm)
            torch.cuda.synchronize()
            _frames_intact(pflats, p_off)
            _frames_intact(gflats, g_off)
            for p, g, gv in zip(ps, _grads(step, scales), gviews):
                assert torch.equal(gv.cpu(), g)                        # gradients are read only (the clip is not materialised)
            for p, s in zip(ps, shadows):
                assert ops.shadows.peek(p) is s                        # written by the update kernel, over every chunk and tail
                assert torch.equal(_bits(s), _bits(p.detach().bfloat16()))
            out.append(([p.detach().cpu().clone() for p in ps], [opt.state[p]["exp_avg"].cpu().clone() for p in ps],
                        [opt.state[p]["exp_avg_sq"].cpu().clone() for p in ps],
                        None if max_norm is None else opt.grad_norm().item()))
        return out
    finally:
        ops.shadows.clear()


def _reference(max_norm, scales):
    ps = [_randn(n, i).double() for i, n in enumerate(SIZES)]
    ms, vs = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
    out = []
    for step in range(len(scales)):
        gs = _grads(step, scales)
        norm = R.global_norm(gs)
        coef = R.clip_coef(norm, max_norm)
        for p, g, m, v, k in zip(ps, gs, ms, vs, GROUP):
            R.adamw_step(p, g, m, v, step + 1, _f32(LR[k]), _f32(WD[k]), coef, betas=(_f32(0.9), _f32(0.999)), eps=_f32(1e-8))
        out.append(([p.clone() for p in ps], [m.clone() for m in ms], [v.clone() for v in vs], norm, coef))
    return out


def _compare(got, ref, max_norm):
    for (p, m, v, norm), (pr, mr, vr, norm_ref, _) in zip(got, ref):
        if max_norm is not None:
            assert abs(norm - norm_ref) <= 1e-6 * norm_ref
        for i in range(len(SIZES)):
            assert max_err(p[i], pr[i]) < 2e-6, f"parameter {i}"
            assert max_err(m[i], mr[i]) < 1e-6 and max_err(v[i], vr[i]) < 1e-6, f"moments of parameter {i}"


SCALES = (0.5, 1.5, 2.5)


@pytest.mark.parametrize("max_norm", [None, 1.0])
def test_fused_adamw_across_chunks_matches_float64(dev, max_norm):
    """three steps over tensors of 65541, 196608, 65535, 7 and 1 elements in two groups: chunk offsets > 0, the 4-wide body and
    the scalar tail of a chunk, parameters and moments against float64"""
    ref = _reference(max_norm, SCALES)
    if max_norm is not None:
        assert all(r[4] < 1.0 for r in ref)                            # the clip is active in every step
    _compare(_trajectory(dev, [0] * 5, [0] * 5, max_norm, SCALES), ref, max_norm)


def test_fused_adamw_clip_inactive_for_small_gradients(dev):
    scales = (1e-4,)
    ref = _reference(1.0, scales)
    assert ref[0][4] == 1.0 and 0.0 < ref[0][3] < 0.1
    _compare(_trajectory(dev, [0] * 5, [0] * 5, 1.0, scales), ref, 1.0)


@pytest.mark.parametrize("max_norm", [None, 1.0])
def test_fused_adamw_unaligned_storage_is_bit_identical(dev, max_norm):
    """parameters 1, 2 and 3 elements into a flat buffer, gradients at other offsets (arena slices can lie so): whole chunks
    take the scalar path.  Same bits as the aligned run, neighbours of every tensor untouched, shadows written as well."""
    aligned = _trajectory(dev, [0] * 5, [0] * 5, max_norm, SCALES)
    shifted = _trajectory(dev, P_OFF, G_OFF, max_norm, SCALES)
    _compare(shifted, _reference(max_norm, SCALES), max_norm)
    for (p, m, v, norm), (p2, m2, v2, norm2) in zip(aligned, shifted):
        assert norm == norm2 or abs(norm - norm2) <= 1e-6 * norm       # (double atomics: the order of the chunks may differ)
        for i in range(len(SIZES)):
            assert torch.equal(_bits(p[i]), _bits(p2[i])), f"parameter {i}"
            assert torch.equal(_bits(m[i]), _bits(m2[i])) and torch.equal(_bits(v[i]), _bits(v2[i])), f"moments of parameter {i}"


@pytest.mark.parametrize("chunk", [CHUNK, 1001])
def test_multi_sumsq_per_tensor_and_total(dev, chunk):
    """accumulates in double: relative 1e-10 against float64.  The second tensor starts one element into its buffer, so every
    chunk of it is unaligned; with a chunk size of 1001 the chunks of the aligned tensors alternate as well."""
    from fcmf_framework import _hip as H
    sizes = [CHUNK + 5, 3 * CHUNK + 3, 7, 1]
    offs = [0, 1, 0, 3]
    vals = [_randn(n, 200 + i, 1.0 + i) for i, n in enumerate(sizes)]
    flats = [torch.full((n + 8,), SENTINEL, device=dev) for n in sizes]
    gs = []
    for f, v, o in zip(flats, vals, offs):
        f[o:o + v.numel()] = v.to(dev)
        gs.append(f[o:o + v.numel()])
    ct = [t for t, n in enumerate(sizes) for _ in range(0, n, chunk)]
    co = [off for n in sizes for off in range(0, n, chunk)]
    i64 = lambda xs: torch.tensor(xs, dtype=torch.int64, device=dev)
    g_ptrs, sz, cod = i64([g.data_ptr() for g in gs]), i64(sizes), i64(co)
    ctd = torch.tensor(ct, dtype=torch.int32, device=dev)
    total = R.guarded((1,), torch.float64, dev)
    per = R.guarded((len(sizes),), torch.float64, dev)
    total.view.zero_()
    per.view.zero_()
    L = H.lib()
    assert L.fcmf_multi_sumsq(H.ptr(g_ptrs), H.ptr(sz), H.ptr(ctd), H.ptr(cod), len(ct), chunk, H.ptr(total.view), H.ptr(per.view),
                              H.stream()) == 0
    torch.cuda.synchronize()
    R.check_all(total, per)
    ref = [float(v.double().pow(2).sum()) for v in vals]
    for got, r in zip(per.view.cpu().tolist(), ref):
        assert abs(got - r) <= 1e-10 * r
    assert abs(total.view.item() - math.fsum(ref)) <= 1e-10 * math.fsum(ref)
    # either output may be left out
    total.view.zero_()
    assert L.fcmf_multi_sumsq(H.ptr(g_ptrs), H.ptr(sz), H.ptr(ctd), H.ptr(cod), len(ct), chunk, H.ptr(total.view), 0, H.stream()) == 0
    torch.cuda.synchronize()
    assert abs(total.view.item() - math.fsum(ref)) <= 1e-10 * math.fsum(ref)
    assert L.fcmf_multi_sumsq(H.ptr(g_ptrs), H.ptr(sz), H.ptr(ctd), H.ptr(cod), len(ct), 0, H.ptr(total.view), 0, H.stream()) == -1
