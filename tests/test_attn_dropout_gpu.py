"""Attention dropout against an independent reference: float64 autograd under the stated mask (attn_ref.attention_ref, whose
mask is rowwise_ref.mask_tensor over the row-major index of the probability tensor) for out, dq, dk1, dv1, dk2, dv2 and dbias
of every VALU kernel family, the MFMA kernels and the long-key kernels (A); the mask itself, bit for bit, as each bf16 kernel's
forward applies it and as its backward regenerates it, recovered with selector matrices (B); and the chunked float32 parity
mode of shared_kv_attention with one seed per member and chunk (C).

Bounds.  A and C: those of test_ops_gpu.test_attention_fwd_bwd for the same cases at p = 0 -- float32 3e-5 (output) and 6e-5
(gradients), bf16 3e-2 and 6e-2, relative to the tensor's maximum.  Dropout multiplies kept probabilities by 1/(1-p) <= 1.43 in
the kernel and in the reference alike, which leaves the error relative to the maximum where it was; one wrongly kept or dropped
entry moves an output by about P |v| / (1-p), 1e-2 and more at these key counts.  B: the kept set must EQUAL the stated mask;
kept values within rtol 2e-2, atol 1e-3 (the bound of test_ops_gpu's *_dropout_consistent tests: bf16 storage).
test_attn_dropout_cpu.py checks on the reference alone what these tests rely on: every (case, p, seed) drops and keeps at
least one live probability, and every probe input has P > 1e-10 everywhere, so that "non-zero" means "kept".

Measured on an MI355X (largest error per kernel family over its cases, output / gradients; all 151 tests pass, 3.5 s):
  A float32  attn_small_fwd_kernel<float, 4, 0 | 64> with attn_small_bwd_kernel<float, *, *> (+ attn_private_grad_kernel<float>)
                                                                              3.8e-7 / 8.0e-7      (bounds 3e-5 / 6e-5)
  A bf16     attn_small_fwd / _bwd_kernel<bf16_t, ...> (+ private_grad)       3.2e-3 / 7.0e-3      (bounds 3e-2 / 6e-2)
             attn_tiny_fwd_kernel<false | true>, attn_tiny_bwd(_blocked)      3.6e-3 / 4.0e-3
             attn_rows_flat_fwd / _bwd_kernel + attn_private_grad_kernel      2.9e-3 / 4.5e-3
             fcmf_attn_mfma_fwd / _bwd                                        3.6e-3 / 3.7e-3
             fcmf_attn_mfma_long_fwd / _bwd                                   3.3e-3 / 5.6e-3
  B          every kept set, forward and backward, equal to the stated mask; kept values within 3.9e-3 relative (one bf16
             rounding) for the MFMA, fused-layout and VALU kernels, 7.5e-3 for the long-key kernels (bound: rtol 2e-2)
  C float32  chunked parity mode                                              3.4e-7 / 5.4e-7      (bounds 3e-5 / 6e-5)
With the group and head swapped in the VALU kernels' counter and two rows swapped in pair_dropout_mult4 (both give a different
but equally well distributed mask), 135 of the 151 tests fail; the 16 that pass are the G = 1 and heads = 1 rows of ATTN_CASES
and the odd-Tk MFMA and long-key cases, which those two changes leave on the stated mask."""
import math

import pytest
import torch

import rowwise_ref as RR
from attn_ref import attention_ref, heads_first, selector, selector_blocks
from helpers import mfma_attention, rel_err
from test_attn_small_plan_cpu import BWD, FLAT_B, FLAT_F, FWD, KERNELS, TINY_B, TINY_BB, TINY_F, TINY_FW
from test_ops_gpu import ATTN_CASES

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
TOL = {F32: 3e-5, BF16: 3e-2}            # the output; gradients twice that (test_attention_fwd_bwd)
FEW = (3, 1, 2, 64, 0, 2, 1, False, False, False)      # 12 probabilities: (0.1, SEED_HI) keeps them all


def dropout_pairs(case):
    """the (p, seed) pairs of part A for a row of ATTN_CASES"""
    few = case is not None and tuple(case) == FEW
    return [(0.3, RR.SEED_LO), (0.5, RR.SEED_HI)] if few else [(0.1, RR.SEED_HI), (0.3, RR.SEED_LO)]


def _randn(shape, dtype, scale, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def hard_mask(G, T, seed=7):
    m01 = (torch.rand(G, T, generator=torch.Generator().manual_seed(seed)) > 0.2).float()
    m01[:, 0] = 1
    return (1 - m01) * -10000.0


def small_inputs(case, dtype):
    """the operands of test_ops_gpu.test_attention_fwd_bwd for a case (same seeds and scales), on the CPU, rounded to dtype"""
    G, R, heads, d, T1, T2, gd, use_mask, use_bias, causal = case
    HD, T = heads * d, T1 + T2
    return dict(q=_randn((G, R, HD), dtype, 0.7, 1),
                k1=_randn((G, T1, HD), dtype, 0.7, 2) if T1 else None, v1=_randn((G, T1, HD), dtype, 0.7, 3) if T1 else None,
                k2=_randn((G // gd, R, T2, HD), dtype, 0.7, 4) if T2 else None,
                v2=_randn((G // gd, R, T2, HD), dtype, 0.7, 5) if T2 else None,
                mask=hard_mask(G, T) if use_mask else None,
                bias=_randn((G // gd, heads, R, T), F32, 1.0, 8) if use_bias else None,
                w=_randn((G, R, HD), dtype, 1.0, 9))


def shared_inputs(G, share, Tq, Tk, heads, d, dtype):
    """q [G,Tq,HD], one key/value set per `share` consecutive groups, a hard key mask per group"""
    HD = heads * d
    return dict(q=_randn((G, Tq, HD), dtype, 0.7, 1), k1=_randn((G // share, Tk, HD), dtype, 0.7, 2),
                v1=_randn((G // share, Tk, HD), dtype, 0.7, 3), k2=None, v2=None, mask=hard_mask(G, Tk), bias=None,
                w=_randn((G, Tq, HD), dtype, 1.0, 9))


# (G, heads, d) of the MFMA cases; part A's (Tq, Tk) and part B's
MFMA_GEOM = (3, 2, 64)
MFMA_A = [(130, 129), (77, 128)]
MFMA_B = [(256, 256), (130, 129), (77, 128), (33, 18)]
#          G  kv_share Tq  Tk
LONG_A = [(6, 3, 77, 300), (2, 1, 64, 515)]
LONG_B = [(6, 3, 77, 300), (2, 1, 64, 515), (4, 2, 40, 1030)]
FUSED_B = [128, 100]
# name: (G, R, heads, d, T1, T2, bias, forward kernel, backward kernel) of part B's VALU bf16 configurations
VALU_B = {
    "tiny": (2, 36, 8, 96, 36, 0, True, TINY_F, TINY_B),
    "wide-blocked": (2, 100, 2, 128, 100, 0, False, TINY_FW, TINY_BB),
    "flat": (2, 7, 3, 64, 128, 36, False, FLAT_F, FLAT_B),
    "general": (2, 129, 2, 64, 64, 0, False, FWD % "bf16_t, 4, 64", BWD % "bf16_t, false, false"),
}
B_PS = [0.25, 0.1]
PARITY = dict(G=4, share=2, Tq=20, Tk=300, heads=2, d=64, p=0.1, seed=2024)     # part C


def probe_inputs(G, R, heads, d, T1, T2=0, share=1, bias=False):
    """part B: bf16 randn * 0.8 operands, a SOFT additive mask (randn * 2: no probability is zero, so zero means dropped)"""
    HD, T = heads * d, T1 + T2
    return dict(q=_randn((G, R, HD), BF16, 0.8, 1), k1=_randn((G // share, T1, HD), BF16, 0.8, 2),
                v1=_randn((G // share, T1, HD), BF16, 0.8, 3),
                k2=_randn((G, R, T2, HD), BF16, 0.8, 4) if T2 else None, v2=_randn((G, R, T2, HD), BF16, 0.8, 5) if T2 else None,
                mask=_randn((G, T), F32, 2.0, 6), bias=_randn((G, heads, R, T), F32, 1.0, 7) if bias else None)


def probe_reference(inp, heads, share=1):
    """-> the float64 probabilities [G, heads, R, T] of probe inputs"""
    k1 = inp["k1"].repeat_interleave(share, 0)
    d = inp["q"].shape[-1] // heads
    return attention_ref(inp["q"], k1, k1, inp["k2"], inp["k2"], inp["mask"], inp["bias"], heads, 1, 1 / math.sqrt(d), False)[1]


def parity_keep(seeds, G, share, heads, Tq, Tk, p, chunk=256):
    """the 0/1 keep tensor [G,heads,Tq,Tk] of the chunked float32 mode: member m (groups m::share) runs chunk i of the keys with
    seed (seeds[m] + i) mod 2^64 on a probability tensor of its own, [G/share, heads, Tq, len_i]"""
    keep = torch.empty(G, heads, Tq, Tk, dtype=torch.float64)
    for m in range(share):
        for i, a in enumerate(range(0, Tk, chunk)):
            b = min(a + chunk, Tk)
            keep[m::share, :, :, a:b] = RR.mask_tensor((seeds[m] + i) & 0xFFFFFFFFFFFFFFFF, (G // share, heads, Tq, b - a), p)
    return keep


# ---- A: float64 autograd under dropout ----------------------------------------------------------------------------------------
NAMES = ("q", "k1", "v1", "k2", "v2", "bias")


def _compare(dev, inp, call, heads, gd, causal, p, seed, tol, tag, share=1, keep=None):
    """call(operands on the device, requiring gradients) -> out; loss sum(out * w); everything against attention_ref's autograd"""
    g = {n: None if inp[n] is None else inp[n].to(dev).requires_grad_(True) for n in NAMES}
    g["mask"] = None if inp["mask"] is None else inp["mask"].to(dev)
    out = call(g)
    (out.float() * inp["w"].to(dev).float()).sum().backward()
    r = {n: None if inp[n] is None else inp[n].double().requires_grad_(True) for n in NAMES}
    expand = lambda t: t if share == 1 else t.repeat_interleave(share, 0)          # (autograd sums dk / dv over the sharers)
    d = inp["q"].shape[-1] // heads
    ref = attention_ref(r["q"], None if r["k1"] is None else expand(r["k1"]), None if r["v1"] is None else expand(r["v1"]),
                        r["k2"], r["v2"], inp["mask"], r["bias"], heads, gd, 1 / math.sqrt(d), causal, p, seed, keep)[0]
    (ref * inp["w"].double()).sum().backward()
    errs = {"out": rel_err(out, ref)}
    errs.update({"d" + n: rel_err(g[n].grad, r[n].grad) for n in NAMES if g[n] is not None})
    print("ERR", tag, " ".join(f"{n}={e:.2e}" for n, e in errs.items()))
    for n, e in errs.items():
        assert e < (tol if n == "out" else 2 * tol), (n, e)


A_PARAMS = [(i, p, s) for i, c in enumerate(ATTN_CASES) for p, s in dropout_pairs(c)]


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("i,p,seed", A_PARAMS, ids=["case%d-p%g-seed%d" % a for a in A_PARAMS])
def test_valu_attention_dropout_matches_float64(dev, dtype, i, p, seed):
    """every row of ATTN_CASES (the kernels of test_attn_small_plan_cpu.KERNELS) at p > 0 with an explicit seed"""
    from fcmf_framework import ops
    case = ATTN_CASES[i]
    G, R, heads, d, T1, T2, gd, use_mask, use_bias, causal = case
    fam = KERNELS[i][:2] if dtype == F32 else KERNELS[i][2:]

    def call(g):
        with mfma_attention(False):
            out = ops.AttentionFn.apply(g["q"], g["k1"], g["v1"], g["k2"], g["v2"], g["mask"], g["bias"], heads, gd,
                                        1 / math.sqrt(d), p, seed, causal)
        assert out.grad_fn.mfma is False
        return out
    _compare(dev, small_inputs(case, dtype), call, heads, gd, causal, p, seed, TOL[dtype], f"[{fam[0]} | {fam[1]}] case{i} p={p}")


@pytest.mark.parametrize("p,seed", dropout_pairs(None), ids=["p0.1-hi", "p0.3-lo"])
@pytest.mark.parametrize("Tq,Tk", MFMA_A)
def test_mfma_attention_dropout_matches_float64(dev, Tq, Tk, p, seed):
    from fcmf_framework import ops
    G, heads, d = MFMA_GEOM

    def call(g):
        with mfma_attention(True):
            out = ops.AttentionFn.apply(g["q"], g["k1"], g["v1"], None, None, g["mask"], None, heads, 1, 1 / math.sqrt(d), p, seed, False)
        assert out.grad_fn.mfma is True
        return out
    _compare(dev, small_inputs((G, Tq, heads, d, Tk, 0, 1, True, False, False), BF16), call, heads, 1, False, p, seed, TOL[BF16],
             f"[fcmf_attn_mfma_fwd | fcmf_attn_mfma_bwd] {Tq}x{Tk} p={p}")


@pytest.mark.parametrize("p,seed", dropout_pairs(None), ids=["p0.1-hi", "p0.3-lo"])
@pytest.mark.parametrize("G,share,Tq,Tk", LONG_A)
def test_long_attention_dropout_matches_float64(dev, G, share, Tq, Tk, p, seed):
    """each member against its key set; dk / dv summed over the sharers.  The counter's group is the QUERY group."""
    from fcmf_framework import ops
    _, heads, d = MFMA_GEOM

    def call(g):
        return ops.SharedKVAttentionFn.apply(g["q"], g["k1"], g["v1"], g["mask"], heads, share, 1 / math.sqrt(d), p, seed)
    _compare(dev, shared_inputs(G, share, Tq, Tk, heads, d, BF16), call, heads, 1, False, p, seed, TOL[BF16],
             f"[fcmf_attn_mfma_long_fwd | fcmf_attn_mfma_long_bwd] G{G} share{share} {Tq}x{Tk} p={p}", share=share)


# ---- B: the mask, bit for bit ---------------------------------------------------------------------------------------------------
def _recover_fwd(fwd, G, heads, R, T, d):
    """fwd(j) -> out [G,R,heads*d] with V = selector j  ->  the dropped probabilities the forward used, [G,heads,R,T]"""
    P = torch.zeros(G, heads, R, T)
    for j in selector_blocks(T, d):
        n = min(d, T - j * d)
        P[..., j * d:j * d + n] = heads_first(fwd(j).detach().float().cpu(), heads)[..., :n]
    return P


def _recover_bwd(bwd, G, heads, R, T, d):
    """bwd(j) -> dV1 [G,T,heads*d] with dO = selector j over the queries  ->  the dropped probabilities the backward regenerated"""
    P = torch.zeros(G, heads, R, T)
    for j in selector_blocks(R, d):
        n = min(d, R - j * d)
        P[:, :, j * d:j * d + n, :] = heads_first(bwd(j).detach().float().cpu(), heads)[..., :n].transpose(-1, -2)
    return P


def _assert_mask(got, P_ref, p, seed, tag, keep=None):
    keep = (RR.mask_tensor(seed, tuple(P_ref.shape), p) if keep is None else keep).bool()
    wrong = (got != 0) != keep
    assert not wrong.any(), f"{tag}: {int(wrong.sum())} of {wrong.numel()} entries kept / dropped against the stated mask, first at " \
                            f"{wrong.nonzero()[0].tolist()}"
    want = (P_ref * RR.inv_keep(p)).float()
    err = ((got - want).abs() / want)[keep].max().item()
    print("MASK", tag, f"exact; kept values rel {err:.2e}")
    assert torch.allclose(got[keep], want[keep], rtol=2e-2, atol=1e-3), tag


def _probe_attention_fn(dev, inp, heads, p, seed, mfma, tag, kernels=None):
    """forward and backward probes through ops.AttentionFn (MFMA or VALU kernels), shared + optional private segment, group_div 1"""
    from fcmf_framework import attn, ops
    G, R, HD = inp["q"].shape
    d, T1 = HD // heads, inp["k1"].shape[1]
    T2 = 0 if inp["k2"] is None else inp["k2"].shape[2]
    T, scale = T1 + T2, 1 / math.sqrt(HD // heads)
    t = {n: None if v is None else v.to(dev) for n, v in inp.items()}
    P_ref = probe_reference(inp, heads)

    def run(v1, v2):
        with mfma_attention(mfma):
            out = ops.AttentionFn.apply(t["q"], t["k1"], v1, t["k2"], v2, t["mask"], t["bias"], heads, 1, scale, p, seed, False)
        assert out.grad_fn is None or out.grad_fn.mfma is mfma
        return out

    if kernels is not None:
        a = attn.desc(t["q"], t["k1"], t["v1"], t["k2"], t["v2"], t["mask"], t["bias"], heads, 1, scale, p, seed, False, 0)
        fwd, bwd = attn.small_plan(a)[2], attn.small_plan(a, True, T2 > 0, False, True)[2]
        assert (fwd[0], bwd[0] + (" + " + bwd[1] if bwd[1] else "")) == kernels

    def fwd(j):
        S = selector(T, d, heads, j).to(BF16).to(dev)
        v2 = S[T1:].expand(G, R, T2, HD).contiguous() if T2 else None
        return run(S[:T1].expand(G, T1, HD).contiguous(), v2)
    _assert_mask(_recover_fwd(fwd, G, heads, R, T, d), P_ref, p, seed, tag + " forward")

    v1 = t["v1"].clone().requires_grad_(True)
    v2 = t["v2"].clone().requires_grad_(True) if T2 else None
    out = run(v1, v2)
    bwd = lambda j: torch.autograd.grad(out, v1, selector(R, d, heads, j).to(BF16).to(dev).expand(G, R, HD).contiguous(),
                                        retain_graph=True)[0]
    got = _recover_bwd(bwd, G, heads, R, T1, d)
    if T2:      # dO = 1: dV2[g, r, t, h*d + c] = Pdrop[g, h, r, T1 + t] for every c
        dv2 = torch.autograd.grad(out, v2, torch.ones_like(out))[0].float().cpu()
        got = torch.cat((got, dv2.view(G, R, T2, heads, d)[..., 0].permute(0, 3, 1, 2)), -1)
    _assert_mask(got, P_ref, p, seed, tag + " backward")


@pytest.mark.parametrize("p", B_PS)
@pytest.mark.parametrize("Tq,Tk", MFMA_B)
def test_mfma_kernels_apply_the_stated_mask(dev, Tq, Tk, p):
    """fcmf_attn_mfma_fwd (dropout_mult4, even and odd bases) and _bwd (the pair form for even Tk, per element for odd Tk)"""
    G, heads, d = MFMA_GEOM
    _probe_attention_fn(dev, probe_inputs(G, Tq, heads, d, Tk), heads, p, RR.SEED_HI, True, f"mfma {Tq}x{Tk} p={p}")


@pytest.mark.parametrize("p", B_PS)
@pytest.mark.parametrize("name", list(VALU_B))
def test_valu_bf16_kernels_apply_the_stated_mask(dev, name, p):
    G, R, heads, d, T1, T2, bias, kf, kb = VALU_B[name]
    _probe_attention_fn(dev, probe_inputs(G, R, heads, d, T1, T2, bias=bias), heads, p, RR.SEED_HI, False, f"valu {name} p={p}",
                        kernels=(kf, kb))


@pytest.mark.parametrize("p", B_PS)
@pytest.mark.parametrize("T", FUSED_B)
def test_fused_layout_applies_the_stated_mask(dev, T, p):
    """fused.self_attention_fwd / _bwd read q | k | v in place from a [G*T, 3*Hd] buffer (row stride 3*Hd) and write dqkv"""
    from fcmf_framework import attn, fused
    G, heads, d = MFMA_GEOM
    Hd, seed = heads * d, RR.SEED_HI
    inp = probe_inputs(G, T, heads, d, T)
    P_ref = probe_reference(inp, heads)
    mask = inp["mask"].to(dev)
    qkv = lambda v: torch.cat((inp["q"], inp["k1"], v), -1).view(G * T, 3 * Hd).to(dev)

    def fwd(j):
        buf = qkv(selector(T, d, heads, j).to(BF16).expand(G, T, Hd))
        return fused.self_attention_fwd(buf, mask, G, T, Hd, heads, p, seed)[0].view(G, T, Hd)
    _assert_mask(_recover_fwd(fwd, G, heads, T, T, d), P_ref, p, seed, f"fused T={T} p={p} forward")

    buf = qkv(inp["v1"])
    assert attn.mfma_eligible(fused._self_desc(buf, mask, G, T, Hd, heads, p, seed))
    out, lse =fused.self_attention_fwd(buf, mask, G, T, Hd, heads, p, seed)

    def bwd(j):
        dout = selector(T, d, heads, j).to(BF16).to(dev).expand(G, T, Hd).reshape(G * T, Hd).contiguous()
        return fused.self_attention_bwd(buf, mask, out, lse, dout, G, T, Hd, heads, p, seed)[:, 2 * Hd:].reshape(G, T, Hd)
    _assert_mask(_recover_bwd(bwd, G, heads, T, T, d), P_ref, p, seed, f"fused T={T} p={p} backward")


@pytest.mark.parametrize("p", B_PS)
@pytest.mark.parametrize("G,share,Tq,Tk", LONG_B)
def test_long_kernels_apply_the_stated_mask(dev, G, share, Tq, Tk, p):
    """fcmf_attn_mfma_long_fwd / _bwd.  The backward probe sets dO for one sharing member at a time: the others add exact zeros
    to the summed dv."""
    from fcmf_framework import ops
    _, heads, d = MFMA_GEOM
    HD, seed, scale = heads * d, RR.SEED_HI, 1 / math.sqrt(d)
    inp = probe_inputs(G, Tq, heads, d, Tk, share=share)
    P_ref = probe_reference(inp, heads, share)
    q, k, mask = inp["q"].to(dev), inp["k1"].to(dev), inp["mask"].to(dev)
    run = lambda v: ops.SharedKVAttentionFn.apply(q, k, v, mask, heads, share, scale, p, seed)
    fwd = lambda j: run(selector(Tk, d, heads, j).to(BF16).to(dev).expand(G // share, Tk, HD).contiguous())
    _assert_mask(_recover_fwd(fwd, G, heads, Tq, Tk, d), P_ref, p, seed, f"long G{G} share{share} {Tq}x{Tk} p={p} forward")

    v = inp["v1"].to(dev).requires_grad_(True)
    out = run(v)
    got = torch.zeros(G, heads, Tq, Tk)
    for m in range(share):
        def bwd(j):
            dout = torch.zeros(G, Tq, HD, dtype=BF16, device=dev)
            dout[m::share] = selector(Tq, d, heads, j).to(BF16).to(dev)
            return torch.autograd.grad(out, v, dout, retain_graph=True)[0]
        got[m::share] = _recover_bwd(bwd, G // share, heads, Tq, Tk, d)
    _assert_mask(got, P_ref, p, seed, f"long G{G} share{share} {Tq}x{Tk} p={p} backward")


# ---- C: the float32 parity mode --------------------------------------------------------------------------------------------------
def test_float32_parity_mode_dropout_matches_float64(dev):
    """ops.shared_kv_attention in float32 beyond the one-piece key limit: chunks of 256 and 44 keys per member, each launch with a
    seed and a probability tensor of its own; the reference applies those masks to the GLOBAL softmax"""
    from fcmf_framework import ops
    c = PARITY
    G, share, Tq, Tk, heads, d, p = (c[n] for n in ("G", "share", "Tq", "Tk", "heads", "d", "p"))
    assert Tk > ops.valu_float32_key_limit(d)
    ops.manual_seed(c["seed"])
    seeds = [ops.next_seed() for _ in range(share)]
    keep = parity_keep(seeds, G, share, heads, Tq, Tk, p)

    def call(g):
        ops.manual_seed(c["seed"])
        return ops.shared_kv_attention(g["q"], g["k1"], g["v1"], mask=g["mask"], heads=heads, kv_share=share, p=p, training=True)
    _compare(dev, shared_inputs(G, share, Tq, Tk, heads, d, F32), call, heads, 1, False, p, 0, TOL[F32],
             "[float32 parity mode, chunked]", share=share, keep=keep)
