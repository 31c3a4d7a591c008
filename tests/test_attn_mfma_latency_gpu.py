"""MFMA text-encoder attention after its global loads were gathered into one batch: the additive mask now reaches the
backward's key chunks through registers and lane shuffles, delta takes dO from its LDS image, and the persistent forward
stages the next tile before it stores the current one.  None of that changes a result, so every check here holds for the
kernels before that change as well: a mask value that differs per key and per sequence (any mix-up of key index or
sequence shows), hard masks that are not a suffix, launches whose sequences / tiles must not see each other's state."""
import math

import pytest
import torch

from helpers import mfma_attention, rel_err

pytestmark = pytest.mark.gpu

HEADS, D = 2, 64
HD = HEADS * D
FMIN = torch.finfo(torch.float32).min


def _rand(shape, dev, scale=0.8, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(torch.bfloat16).to(dev)


def _soft_mask(G, Tk, seed=3):
    """finite additive mask, every key of a sequence another value, every sequence another permutation"""
    g = torch.Generator().manual_seed(seed)
    base = torch.linspace(-4.0, 0.0, Tk)
    return torch.stack([base[torch.randperm(Tk, generator=g)] for _ in range(G)])


def _ref64(q, k, v, mask, w, heads):
    """float64 attention on the CPU -> out, dq, dk, dv for the upstream gradient w"""
    c = lambda t: t.detach().double().cpu().requires_grad_(True)
    q, k, v = c(q), c(k), c(v)
    G, Tq, hd = q.shape
    sp = lambda t: t.view(G, -1, heads, hd // heads).transpose(1, 2)
    s = sp(q) @ sp(k).transpose(-1, -2) / math.sqrt(hd // heads) + mask.double().cpu()[:, None, None, :]
    out = (torch.softmax(s, -1) @ sp(v)).transpose(1, 2).reshape(G, Tq, hd)
    (out * w.double().cpu()).sum().backward()
    return out.detach(), q.grad, k.grad, v.grad


def _run(q0, k0, v0, mask, w, p, heads=HEADS, seed=5):
    from fcmf_framework import ops
    q, k, v = (t.clone().requires_grad_(True) for t in (q0, k0, v0))
    ops.manual_seed(seed)
    out = ops.attention(q, k, v, mask=mask, heads=heads, p=p, training=p > 0)
    (out.float() * w.float()).sum().backward()
    return out.detach(), q.grad, k.grad, v.grad


def _check(got, want, floor, tag):
    """rel_err < 3e-2 for out, dq, dk, dv.  A reference that is identically zero (one key: the softmax is constant, dq = dk = 0)
    has no scale of its own: there the error is measured against `floor`, the size of the terms that cancel."""
    for a, b, name in zip(got, want, ("out", "dq", "dk", "dv")):
        if b.abs().max().item() == 0.0:
            e = (a.detach().double().cpu() - b).abs().max().item() / floor
        else:
            e = rel_err(a, b)
        print(f"{tag} {name}: rel_err {e:.3e}")
        assert e < 3e-2, (tag, name, e)


@pytest.mark.parametrize("Tq,Tk", [(128, 128), (77, 128), (33, 17), (1, 1), (128, 97), (200, 256), (130, 129)])
def test_soft_mask_per_key_matches_float64(dev, Tq, Tk):
    G = 3
    q0, k0, v0, w = _rand((G, Tq, HD), dev, seed=1), _rand((G, Tk, HD), dev, seed=2), _rand((G, Tk, HD), dev, seed=3), _rand((G, Tq, HD), dev, seed=9)
    mask = _soft_mask(G, Tk).to(dev)
    got = _run(q0, k0, v0, mask, w, 0.0)
    want = _ref64(q0, k0, v0, mask, w, HEADS)
    # (zero reference: dq = dS K / 8 and dk = dS^T Q / 8 with dS = P (dP - delta), where |dP[q][key]| and |delta[q]| are
    #  at most max over (q, key, head) of sum_d |w[q][d]| |v[key][d]|)
    sp = lambda t: t.float().abs().view(G, -1, HEADS, D).transpose(1, 2)
    floor = (sp(w) @ sp(v0).transpose(-1, -2)).max().item() * max(k0.abs().max().item(), q0.abs().max().item()) / math.sqrt(D)
    _check(got, want, floor, f"soft {Tq}x{Tk}")


def test_soft_mask_fused_layout_matches_float64(dev):
    """q | k | v as column blocks of one [G T, 3 H] buffer (row stride 3 H), the layout the encoder layers use"""
    from fcmf_framework import fused
    G, T = 3, 100
    qkv = _rand((G * T, 3 * HD), dev, seed=1)
    dout = _rand((G * T, HD), dev, 1.0, seed=4)
    mask = _soft_mask(G, T).to(dev)
    out, lse = fused.self_attention_fwd(qkv, mask, G, T, HD, HEADS, 0.0, 11)
    dqkv = fused.self_attention_bwd(qkv, mask, out, lse, dout, G, T, HD, HEADS, 0.0, 11)
    blk = lambda t, i: t[:, i * HD:(i + 1) * HD].reshape(G, T, HD)
    want = _ref64(blk(qkv, 0), blk(qkv, 1), blk(qkv, 2), mask, dout.view(G, T, HD), HEADS)
    got = (out.view(G, T, HD), blk(dqkv, 0), blk(dqkv, 1), blk(dqkv, 2))
    _check(got, want, 1.0, "soft fused 100")


@pytest.mark.parametrize("p", [0.0, 0.2])
def test_hard_mask_in_the_middle_matches_valu_kernel(dev, p):
    """hard-masked keys that are NOT a suffix: a whole leading 32-key chunk, every second key, a fully masked sequence next to
    an unmasked one -- against the VALU kernels with the same dropout seed; masked keys get exactly zero dk / dv"""
    G, T = 4, 128
    q0, k0, v0, w = (_rand((G, T, HD), dev, seed=s) for s in (1, 2, 3, 9))
    m01 = torch.ones(G, T)
    m01[0, :32] = 0
    m01[1, 1::2] = 0
    m01[2] = 0
    mask = ((1 - m01) * FMIN).to(dev)
    res = {}
    for use in (True, False):
        with mfma_attention(use):
            res[use] = _run(q0, k0, v0, mask, w, p)
    for a, b, name in zip(res[True], res[False], ("out", "dq", "dk", "dv")):
        e = rel_err(a, b)
        print(f"hard p={p} {name}: rel_err {e:.3e}")
        assert e < 3e-2, name
    dk, dv = res[True][2], res[True][3]
    for g in (0, 1):          # (sequence 2 has no live key: its softmax is uniform over ALL keys, its gradients are not zero)
        dead = (m01[g] == 0).to(dev)
        assert not dk[g][dead].any() and not dv[g][dead].any(), g
        assert dk[g][~dead].any() and dv[g][~dead].any(), g


def test_backward_sequences_do_not_see_each_other(dev):
    """seven sequences of different lengths in one launch: the gradients of each equal, bit for bit, those of launching it alone"""
    G, T = 7, 128
    lens = [128, 1, 33, 64, 97, 17, 100]
    q0, k0, v0, w = (_rand((G, T, HD), dev, seed=s) for s in (1, 2, 3, 9))
    mask = torch.zeros(G, T)
    for g, l in enumerate(lens):
        mask[g, l:] = FMIN
    mask += _soft_mask(G, T)              # (finfo.min + a few units is still <= -1e30: the padding stays hard)
    mask = mask.to(dev)
    whole = _run(q0, k0, v0, mask, w, 0.0)
    for g in range(G):
        s = slice(g, g + 1)
        alone = _run(q0[s].contiguous(), k0[s].contiguous(), v0[s].contiguous(), mask[s].contiguous(), w[s].contiguous(), 0.0)
        for a, b, name in zip(whole, alone, ("out", "dq", "dk", "dv")):
            assert torch.equal(a[s], b), (g, name)


def test_persistent_forward_tiles_do_not_see_each_other(dev):
    """one launch of 171 x 12 = 2052 tiles (the persistent kernel: every workgroup walks several tiles, each with another length
    and mask): rows of the first, the last and three middle sequences equal, bit for bit, a 3-sequence launch of the same
    inputs (the one-tile kernel, which runs the same tile function)"""
    from fcmf_framework import fused
    G, T, heads = 171, 128, 12
    Hd = heads * D
    gen = torch.Generator(device=dev).manual_seed(1)
    qkv = (torch.randn((G * T, 3 * Hd), device=dev, generator=gen) * 0.8).to(torch.bfloat16)
    mask = _soft_mask(G, T)
    for g in range(G):
        mask[g, 1 + (37 * g) % T:] = FMIN          # lengths 1 .. 128, neighbours far apart
    mask = mask.to(dev)
    out, lse = fused.self_attention_fwd(qkv, mask, G, T, Hd, heads, 0.0, 11)
    for g0 in (0, G // 2 - 1, G - 3):
        o3, l3 = fused.self_attention_fwd(qkv[g0 * T:(g0 + 3) * T], mask[g0:g0 + 3], 3, T, Hd, heads, 0.0, 11)
        assert torch.equal(out[g0 * T:(g0 + 3) * T], o3), g0
        assert torch.equal(lse[g0:g0 + 3], l3), g0


def test_backward_with_dropout_is_deterministic(dev):
    G, Tq, Tk = 3, 128, 128
    q0, k0, v0, w = _rand((G, Tq, HD), dev, seed=1), _rand((G, Tk, HD), dev, seed=2), _rand((G, Tk, HD), dev, seed=3), _rand((G, Tq, HD), dev, seed=9)
    mask = _soft_mask(G, Tk).to(dev)
    a = _run(q0, k0, v0, mask, w, 0.2)
    b = _run(q0, k0, v0, mask, w, 0.2)
    for x, y, name in zip(a, b, ("out", "dq", "dk", "dv")):
        assert torch.equal(x, y), name
    assert a[1].any() and a[2].any() and a[3].any()
