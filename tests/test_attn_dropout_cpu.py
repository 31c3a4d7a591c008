"""What test_attn_dropout_gpu.py relies on, checked on the reference alone (no device): attn_ref.attention_ref at p = 0 is the
row-by-row reference of test_ops_gpu; the selector identities that recover a dropped probability matrix hold; every (case, p,
seed) of the GPU tests drops and keeps at least one live probability; no probe input has a probability that could round to zero;
and the VALU probe configurations go to the kernel families they are meant for (the host plan)."""
import math

import pytest
import torch

import rowwise_ref as RR
import test_attn_dropout_gpu as D
from attn_ref import attention_ref, heads_first, selector, selector_blocks
from test_attn_small_plan_cpu import BF16, OK, _desc
from test_ops_gpu import ATTN_CASES, _attn_ref


def _ref(inp, case, p=0.0, seed=0, share=1, keep=None):
    G, R, heads, d, T1, T2, gd, _, _, causal = case
    e = lambda t: t if t is None or share == 1 else t.repeat_interleave(share, 0)
    return attention_ref(inp["q"], e(inp["k1"]), e(inp["v1"]), inp["k2"], inp["v2"], inp["mask"], inp["bias"], heads, gd,
                         1 / math.sqrt(d), causal, p, seed, keep)


@pytest.mark.parametrize("case", ATTN_CASES)
def test_reference_without_dropout_is_the_row_by_row_reference(case):
    G, R, heads, d, T1, T2, gd, _, _, causal = case
    inp = D.small_inputs(case, torch.float32)
    c = lambda t: None if t is None else t.double()
    want = _attn_ref(c(inp["q"]), c(inp["k1"]), c(inp["v1"]), c(inp["k2"]), c(inp["v2"]), c(inp["mask"]), c(inp["bias"]), heads, gd,
                     1 / math.sqrt(d), causal)
    out, P, Pdrop = _ref(inp, case)
    assert (out - want).abs().max().item() < 1e-12
    assert torch.equal(P, Pdrop) and (P.sum(-1) - 1).abs().max().item() < 1e-12


def test_selectors_recover_the_dropped_probabilities():
    """two segments, groups of 2, p = 0.3: as V the selectors give out[g, r, h*d + c] = Pdrop[g, h, r, j*d + c] exactly; as dO
    over the queries they give dV1[g, t, h*d + c] = Pdrop[g, h, j*d + c, t] (autograd of the reference)"""
    G, R, heads, d, T1, T2, gd = 4, 21, 3, 8, 19, 6, 2
    case = (G, R, heads, d, T1, T2, gd, True, True, False)
    inp = D.small_inputs(case, torch.float32)
    T, HD = T1 + T2, heads * d
    Pdrop = _ref(inp, case, 0.3, RR.SEED_HI)[2]
    assert 0 < (Pdrop == 0).sum() < Pdrop.numel()
    got = torch.zeros_like(Pdrop)
    for j in selector_blocks(T, d):
        S = selector(T, d, heads, j)
        n = min(d, T - j * d)
        probe = dict(inp, v1=S[:T1].expand(G, T1, HD), v2=S[T1:].expand(G // gd, R, T2, HD))
        got[..., j * d:j * d + n] = heads_first(_ref(probe, case, 0.3, RR.SEED_HI)[0], heads)[..., :n]
    assert torch.equal(got, Pdrop)
    got = torch.zeros(G, heads, R, T1, dtype=torch.float64)
    for j in selector_blocks(R, d):
        v1 = inp["v1"].double().requires_grad_(True)
        out = _ref(dict(inp, v1=v1), case, 0.3, RR.SEED_HI)[0]
        dv1, = torch.autograd.grad(out, v1, selector(R, d, heads, j).double().expand(G, R, HD))
        n = min(d, R - j * d)
        got[:, :, j * d:j * d + n] = heads_first(dv1, heads)[..., :n].transpose(-1, -2)
    assert torch.equal(got, Pdrop[..., :T1])


def _check_drops_and_keeps(P, p, seed, tag, keep=None):
    keep = (RR.mask_tensor(seed, tuple(P.shape), p) if keep is None else keep).bool()
    live = P > 1e-6
    assert (live & keep).any() and (live & ~keep).any(), tag
    if int(live.sum()) >= 500:
        assert abs(keep[live].double().mean().item() - (1 - p)) <= 0.08, tag


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_every_case_of_the_gpu_tests_drops_and_keeps_live_probabilities(dtype):
    for case in ATTN_CASES:
        P = _ref(D.small_inputs(case, dtype), case)[1]
        for p, seed in D.dropout_pairs(case):
            _check_drops_and_keeps(P, p, seed, (case, p, seed))
    if dtype == torch.bfloat16:
        G, heads, d = D.MFMA_GEOM
        for Tq, Tk in D.MFMA_A:
            case = (G, Tq, heads, d, Tk, 0, 1, True, False, False)
            P = _ref(D.small_inputs(case, dtype), case)[1]
            for p, seed in D.dropout_pairs(None):
                _check_drops_and_keeps(P, p, seed, ("mfma", Tq, Tk, p, seed))
        for G, share, Tq, Tk in D.LONG_A:
            case = (G, Tq, heads, d, Tk, 0, 1, True, False, False)
            P = _ref(D.shared_inputs(G, share, Tq, Tk, heads, d, dtype), case, share=share)[1]
            for p, seed in D.dropout_pairs(None):
                _check_drops_and_keeps(P, p, seed, ("long", G, share, Tq, Tk, p, seed))
    else:
        from fcmf_framework import ops
        c = D.PARITY
        G, share, Tq, Tk, heads, d, p = (c[n] for n in ("G", "share", "Tq", "Tk", "heads", "d", "p"))
        ops.manual_seed(c["seed"])
        seeds = [ops.next_seed() for _ in range(share)]
        assert len(set(seeds)) == share
        keep = D.parity_keep(seeds, G, share, heads, Tq, Tk, p)
        # (member 0, chunk 1: keys 256.. of groups 0, 2 under seed + 1, counted over a [G/share, heads, Tq, 44] tensor)
        assert torch.equal(keep[0::share, :, :, 256:], RR.mask_tensor(seeds[0] + 1 & (2 ** 64 - 1), (G // share, heads, Tq, Tk - 256), p))
        P = _ref(D.shared_inputs(G, share, Tq, Tk, heads, d, dtype), (G, Tq, heads, d, Tk, 0, 1, True, False, False), share=share)[1]
        _check_drops_and_keeps(P, p, 0, "parity", keep)


def _probe_configs():
    G, heads, d = D.MFMA_GEOM
    for Tq, Tk in D.MFMA_B:
        yield ("mfma", Tq, Tk), D.probe_inputs(G, Tq, heads, d, Tk), heads, 1
    for T in D.FUSED_B:
        yield ("fused", T), D.probe_inputs(G, T, heads, d, T), heads, 1
    for G_, share, Tq, Tk in D.LONG_B:
        yield ("long", G_, share, Tq, Tk), D.probe_inputs(G_, Tq, heads, d, Tk, share=share), heads, share
    for name, (G_, R, h, d_, T1, T2, bias, _, _) in D.VALU_B.items():
        yield ("valu", name), D.probe_inputs(G_, R, h, d_, T1, T2, bias=bias), h, 1


def test_probe_inputs_have_no_probability_near_zero():
    """so that in bf16 and in float32 alike a non-zero recovered entry is a kept one"""
    for tag, inp, heads, share in _probe_configs():
        P = D.probe_reference(inp, heads, share)
        print(tag, "min P", P.min().item())
        assert P.min().item() > 1e-10, tag
        for p in D.B_PS:
            _check_drops_and_keeps(P, p, RR.SEED_HI, tag)


def test_valu_probe_configurations_run_the_kernels_they_name():
    from fcmf_framework import attn
    for name, (G, R, heads, d, T1, T2, bias, kf, kb) in D.VALU_B.items():
        a = _desc(BF16, G, R, heads, d, T1, T2, 1, True, bias, False)
        rf, _, nf = attn.small_plan(a)
        rb, _, nb = attn.small_plan(a, True, T2 > 0, False, True)      # (the probes ask for no dbias)
        assert (rf, rb) == (OK, OK), name
        assert (nf[0], nb[0] + (" + " + nb[1] if nb[1] else "")) == (kf, kb), name
