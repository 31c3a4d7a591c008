"""Attention probabilities beyond 256 keys (csrc/attn_long.hip fcmf_attn_mfma_long_probs, ops.shared_kv_attention_probs): per head
and as the head mean formed inside the kernel, against a float64 softmax of the bf16 values the kernel loads, against each
other, against the forward (P V = the attention output) and against themselves (two launches agree bit for bit, every
element of an uninitialised output is written).  heads 2, head dim 64; the shapes of test_attn_long_gpu.py plus a 31-key
and a one-key case: 128-key tile and 32-key chunk boundaries, rows that are not 16-byte aligned (Tk % 4 != 0), a single
key, a single query, one and two query tiles.

Bounds: rel_err < 3e-5 and row sums within 1e-4 of 1 are what test_attn_probs_gpu.py holds the two existing probability
kernels to; P V against the bf16 forward uses test_attn_long_gpu.py's 3e-2; the float32 mode its 1e-4."""
import functools
import math

import pytest
import torch

from helpers import rel_err

pytestmark = pytest.mark.gpu

HEADS, D = 2, 64
HD = HEADS * D
FMIN = torch.finfo(torch.float32).min
BOUND, ROWSUM = 3e-5, 1e-4
#        G  kv_share  Tq   Tk
CASES = [(4, 2, 16, 257), (6, 6, 170, 371), (4, 1, 170, 595), (2, 2, 256, 640), (6, 3, 1, 300), (3, 1, 33, 129), (2, 2, 7, 31),
         (2, 1, 5, 1)]
IDS = ["G%d-share%d-Tq%d-Tk%d" % c for c in CASES]
cases = pytest.mark.parametrize("G,share,Tq,Tk", CASES, ids=IDS)
masks = pytest.mark.parametrize("masked", [False, True], ids=["nomask", "masks"])


def _rand(shape, seed, scale=0.8):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(torch.bfloat16)


def _mask(G, Tk, roles, seed=7):
    """additive float32 key mask [G, Tk]; the role of group g is roles[g]:
       random   25 % of the keys hard-masked, key 0 live
       interior keys 128..383 masked (whole 128-key tiles), 25 % of the rest too, key 0 live
       last     only key Tk-1 live
       full     no live key at all (softmax is uniform over all keys)"""
    gen = torch.Generator().manual_seed(seed)
    dead = torch.rand(G, Tk, generator=gen) < 0.25
    dead[:, 0] = False
    for g, role in enumerate(roles):
        if role == "interior":
            dead[g, 128:384] = True
        elif role == "last":
            dead[g] = True
            dead[g, Tk - 1] = False
        elif role == "full":
            dead[g] = True
    return dead.float() * FMIN


def _roles(G):
    return (["interior", "last", "full"] + ["random"] * G)[:G]


@functools.lru_cache(maxsize=None)
def _case(G, share, Tq, Tk, masked):
    """CPU operands (bf16 q, k, v; float32 mask or None) and the float64 reference [G, heads, Tq, Tk], computed once per case
    and never modified"""
    q, k, v = _rand((G, Tq, HD), 1), _rand((G // share, Tk, HD), 2), _rand((G // share, Tk, HD), 3)
    mask = _mask(G, Tk, _roles(G)) if masked else None
    sp = lambda t: t.double().view(t.shape[0], t.shape[1], HEADS, D).transpose(1, 2)
    sc = sp(q) @ sp(k.repeat_interleave(share, 0)).transpose(-1, -2) / math.sqrt(D)
    if mask is not None:
        sc = sc + mask.double()[:, None, None, :]
    return q, k, v, mask, torch.softmax(sc, -1)


def _on(dev, *ts):
    return [None if t is None else t.to(dev) for t in ts]


def _probs(dev, case, average, **kw):
    from fcmf_framework import ops
    q, k, _, mask, _ = case
    q, k, mask = _on(dev, q, k, mask)
    return ops.shared_kv_attention_probs(q, k, mask=mask, heads=HEADS, kv_share=q.shape[0] // k.shape[0], average_heads=average, **kw)


@masks
@cases
def test_per_head_and_head_mean_match_float64(dev, G, share, Tq, Tk, masked):
    """both modes against the float64 softmax; row sums; hard-masked keys exactly 0; a group without a live key uniform; the
    head mean against the float64 mean of the per-head OUTPUT; two launches of either mode bit-identical"""
    case = _case(G, share, Tq, Tk, masked)
    mask, ref = case[3], case[4]
    per, mean = _probs(dev, case, False), _probs(dev, case, True)
    assert per.shape == (G, HEADS, Tq, Tk) and mean.shape == (G, Tq, Tk)
    assert per.dtype == mean.dtype == torch.float32 and not per.requires_grad and not mean.requires_grad
    errs = {"per_head": rel_err(per, ref), "head_mean": rel_err(mean, ref.mean(1)),
            "mean_vs_per_head": rel_err(mean, per.double().mean(1)),
            "rowsum_per_head": (per.double().sum(-1) - 1).abs().max().item(),
            "rowsum_head_mean": (mean.double().sum(-1) - 1).abs().max().item()}
    print(IDS[CASES.index((G, share, Tq, Tk))], "masked" if masked else "plain", errs)
    for n in ("per_head", "head_mean", "mean_vs_per_head"):
        assert errs[n] < BOUND, (n, errs[n])
    for n in ("rowsum_per_head", "rowsum_head_mean"):
        assert errs[n] < ROWSUM, (n, errs[n])
    assert torch.equal(per, _probs(dev, case, False)) and torch.equal(mean, _probs(dev, case, True))
    if masked:
        dead = mask < -1e30                                             # [G, Tk]
        live_groups = ~dead.all(1)
        hard = dead & live_groups[:, None]
        assert (per.cpu().permute(0, 2, 3, 1)[hard[:, None, :].expand(G, Tq, Tk)] == 0).all()
        assert (mean.cpu()[hard[:, None, :].expand(G, Tq, Tk)] == 0).all()
        for g in (~live_groups).nonzero().flatten().tolist():          # the `full` role
            assert (per[g].cpu() - 1.0 / Tk).abs().max().item() < BOUND / Tk
            assert (mean[g].cpu() - 1.0 / Tk).abs().max().item() < BOUND / Tk


@pytest.mark.parametrize("average", [False, True], ids=["per_head", "head_mean"])
@cases
def test_every_element_is_written(dev, G, share, Tq, Tk, average):
    """masked cases (whole 128-key tiles skipped for the `interior` and `last` groups): an out= tensor full of NaN is finite
    everywhere afterwards and equals a fresh result"""
    case = _case(G, share, Tq, Tk, True)
    shape = (G, Tq, Tk) if average else (G, HEADS, Tq, Tk)
    out = torch.full(shape, float("nan"), dtype=torch.float32, device=dev)
    got = _probs(dev, case, average, out=out)
    assert got is out and torch.isfinite(out).all()
    assert torch.equal(out, _probs(dev, case, average))


@masks
@cases
def test_probabilities_times_v_is_the_forward(dev, G, share, Tq, Tk, masked):
    """float64 P V from the per-head output against ops.shared_kv_attention(p = 0)"""
    from fcmf_framework import ops
    case = _case(G, share, Tq, Tk, masked)
    q, k, v, mask = _on(dev, *case[:4])
    out = ops.shared_kv_attention(q, k, v, mask=mask, heads=HEADS, kv_share=share)
    per = _probs(dev, case, False).double().cpu()
    vh = case[2].double().view(G // share, Tk, HEADS, D).transpose(1, 2).repeat_interleave(share, 0)
    pv = (per @ vh).transpose(1, 2).reshape(G, Tq, HD)
    e = rel_err(out, pv)
    print(IDS[CASES.index((G, share, Tq, Tk))], "masked" if masked else "plain", "P V vs forward", e)
    assert e < 3e-2


@pytest.mark.parametrize("Tk", [285, 371])
def test_float32_parity_mode(dev, Tk):
    """float32 operands: fcmf_attn_probs once per sharing member (kv_share = 3), the head mean a torch reduction; against
    float64 at the 1e-4 of test_attn_long_gpu.py::test_float32_parity_mode"""
    from fcmf_framework import ops
    G, share, Tq = 6, 3, 20
    q, k = _rand((G, Tq, HD), 1), _rand((G // share, Tk, HD), 2)
    mask = _mask(G, Tk, ["interior", "last", "full"] + ["random"] * 3)
    sp = lambda t: t.double().view(t.shape[0], t.shape[1], HEADS, D).transpose(1, 2)
    ref = torch.softmax(sp(q) @ sp(k.repeat_interleave(share, 0)).transpose(-1, -2) / math.sqrt(D) + mask.double()[:, None, None, :], -1)
    qd, kd, md = _on(dev, q.float(), k.float(), mask)
    per = ops.shared_kv_attention_probs(qd, kd, mask=md, heads=HEADS, kv_share=share)
    mean = ops.shared_kv_attention_probs(qd, kd, mask=md, heads=HEADS, kv_share=share, average_heads=True)
    out = torch.full((G, HEADS, Tq, Tk), float("nan"), dtype=torch.float32, device=dev)
    assert ops.shared_kv_attention_probs(qd, kd, mask=md, heads=HEADS, kv_share=share, out=out) is out and torch.equal(out, per)
    e_per, e_mean = rel_err(per, ref), rel_err(mean, ref.mean(1))
    print("float32", Tk, e_per, e_mean)
    assert per.shape == (G, HEADS, Tq, Tk) and mean.shape == (G, Tq, Tk)
    assert e_per < 1e-4 and e_mean < 1e-4


def test_unsupported_configurations_say_so(dev):
    from fcmf_framework import ops
    from fcmf_framework._hip import HipLibraryError
    bf = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device=dev)
    f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
    for q, k, heads in ((bf(2, 257, HD), bf(2, 300, HD), HEADS),        # Tq > 256
                        (bf(2, 16, HD), bf(2, 300, HD), 4),             # bf16 with head dim 32
                        (f32(2, 16, HD), f32(2, 513, HD), HEADS)):      # float32 beyond fcmf_attn_probs' 512 keys
        for average in (False, True):
            with pytest.raises(HipLibraryError, match="unsupported"):
                ops.shared_kv_attention_probs(q, k, heads=heads, average_heads=average)
    with pytest.raises(HipLibraryError, match="query groups per key set"):
        ops.shared_kv_attention_probs(bf(3, 16, HD), bf(2, 300, HD), heads=HEADS, kv_share=2)
    q, k = bf(2, 16, HD), bf(2, 300, HD)
    for bad in (f32(2, 16, 300), f32(2, HEADS, 16, 301), torch.zeros(2, HEADS, 16, 300, dtype=torch.bfloat16, device=dev),
                f32(2, HEADS, 16, 600)[..., ::2]):
        with pytest.raises(HipLibraryError, match="out must be"):
            ops.shared_kv_attention_probs(q, k, heads=HEADS, out=bad)
    with pytest.raises(HipLibraryError, match="out must be"):
        ops.shared_kv_attention_probs(q, k, heads=HEADS, average_heads=True, out=f32(2, HEADS, 16, 300))
