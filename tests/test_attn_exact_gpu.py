"""The training attention kernels (csrc/attn_small.hip, attn_mfma.hip, attn_long.hip, attn_probs.hip) on the selected-key operands of
tests/attn_exact_ref.py: probabilities of exactly 0, 1, 1/2, 1/4 (1/T in one fully masked group), every forward sum exact in
float32 and bf16, dS exact as a bf16 MFMA operand.  The operands lie in NaN-poisoned allocations (padded row strides, NaN rows
behind the last row and a NaN frame; mask and bias contiguous with NaN directly behind them), every output in a guarded buffer
that is pre-filled with NaN where the header promises "fully overwritten" and with the sentinel around it.

Each case of test_attn_exact_cpu.CASES calls the one launch path (fcmf_framework.attn) and asserts, in this order: the return
code (H.check) and the route (attn.mfma_eligible, or the plan's kernel names as test_attn_small_plan_cpu.KERNELS lists them);
every output finite; per element |got - ref| <= u |ref| + eps * mag with u derived (attn_exact_ref.u_of) and eps per kernel family
from EPS below, where `out`, attn.probs and attn.long_probs must EQUAL the reference; lse within 4 float32 ulps (at least 2^-22)
of the float64 logsumexp and colsum_part within eps * mag of the float64 column sums; every guard frame, gap column and extra
row still at its sentinel.  Where fcmf_framework.attn allocates a buffer itself (the dq partials of small_backward, the workspace
of long_backward) the same C entry point runs once more with a guarded, NaN-filled one and must give the same bits.

Not reachable at these shapes: attn_mfma_fwd_persist_kernel (2048 tiles or more).

Measured on an MI355X (77 tests, 3.0 s in all; the first case, which loads the library, 0.42 s, every other at most 0.2 s): every
case took the route it is listed under.  Bit-equal to the reference in EVERY family: `out` (attn_small_fwd_kernel<float | bf16_t,
4, 0 | 64>, attn_tiny_fwd_kernel<false | true>, attn_rows_flat_fwd_kernel, fcmf_attn_mfma_fwd, fcmf_attn_mfma_long_fwd, both
layouts), the probabilities of fcmf_attn_probs, fcmf_attn_mfma_probs and fcmf_attn_mfma_long_probs (head mean on and off), dv1 / dv2
and dbias of every backward, colsum_part, and every dq / dk whose reference is a bf16 value (all float32 cases; all of
attn_rows_flat_bwd_kernel, attn_tiny_bwd_kernel, attn_private_grad_kernel<bf16_t> and fcmf_attn_mfma_long_bwd).  lse is the correctly
rounded float32 of the float64 logsumexp everywhere: 0.008 of its tolerance, which is the float32 representation error of log 2.
eps: the largest |got - ref| / mag over the 106 000 elements with ref == 0 and mag > 0 is 0 in every family -- general float32
and bf16 backward (all eight instantiations, with and without attn_private_grad_kernel), tiny, tiny blocked, flat, MFMA (128- and
256-row kernel), long -- because __expf(0 - lse) of the correctly rounded log 2 / log 4 / log T returns exactly 1/2, 1/4, 1/T on
this hardware.  So eps = 4 * 0 = 0 for every family, and the bound is u |ref| alone: the one bf16 rounding of a stored gradient.
Largest error as a fraction of that bound: 0.996 = 255/256 (a tie of round-to-nearest-even) for dq and dk of fcmf_attn_mfma_bwd,
attn_tiny_bwd_blocked_kernel and dk of attn_small_bwd_kernel<bf16_t, false, false>, all in the fully masked group, whose
gradient references are not bf16 values; 0 everywhere else.  Every guard frame, gap
column, extra row, NaN-filled scratch and workspace check passed; a second backward into the test's own guarded dq partials /
workspace gave the same bits.  Bugs found: none.
"""
import math

import pytest
import torch

import attn_exact_ref as AX
import gemm_ref as GR
import rowwise_ref as RR
from test_attn_exact_cpu import BY_ID, IDS, PAD, UNALIGNED, grouped, operands, reference
from test_attn_small_plan_cpu import KERNELS

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
NAN = float("nan")
# eps per kernel family: 4 x the largest |got - ref| / mag over the elements with ref == 0, rounded up to a power of two (the
# measurements are in the docstring: 0 in every family, so there is nothing to round up); never above attn_exact_ref.EPS_CAP =
# 2^-14, at which test_attn_exact_cpu.py evaluates the sensitivity of the reference.  A family that stops being exact at
# ref == 0 is a finding to explain and re-measure, not a reason to raise a figure here.
EPS = {
    "attn_small_bwd_kernel<float": 0.0,
    "attn_small_bwd_kernel<bf16_t": 0.0,
    "attn_tiny_bwd": 0.0,
    "attn_rows_flat_bwd": 0.0,
    "fcmf_attn_mfma_bwd": 0.0,
    "fcmf_attn_mfma_long_bwd": 0.0,
}
VALU_IDS = [i for i in IDS if BY_ID[i]["kind"] == "valu"]
MFMA_IDS = [i for i in IDS if BY_ID[i]["kind"] == "mfma"]
LONG_IDS = [i for i in IDS if BY_ID[i]["kind"] == "long"]


def _mods():
    from fcmf_framework import _hip, attn
    return _hip, attn


def eps_of(family):
    eps = [v for k, v in EPS.items() if family.startswith(k)]
    assert len(eps) == 1 and eps[0] <= AX.EPS_CAP, family
    return eps[0]


# ---- buffers ------------------------------------------------------------------------------------------------------------------------
def operand(t, dt, dev, ld=None, rows_extra=2):
    """a float64 operand [..., cols] in a NaN-poisoned allocation with row stride ld (cols + PAD unless given) -> the strided view"""
    cols = t.shape[-1]
    p = GR.poisoned(t.reshape(-1, cols).to(dt), cols + PAD if ld is None else ld, rows_extra, dev)
    return p.view.unflatten(0, t.shape[:-1]), p


def flat_operand(t, dev):
    """mask / bias: contiguous float32, NaN directly behind the last element and in a frame"""
    p = GR.poisoned(t.reshape(1, -1).float(), t.numel(), 1, dev)
    return p.view.view(t.shape), p


def dense_out(shape, dt, dev, fill=NAN, offset=0):
    """a guarded dense output, pre-filled; offset: elements the view starts behind the 16-byte aligned interior"""
    n = math.prod(shape)
    g = RR.guarded((n + offset,), dt, dev)
    view = g.view[offset:].view(shape)
    view.fill_(fill)
    if offset:
        g.view[:offset].fill_(RR._SENTINEL[dt])
    g.offset = offset
    return view, g


class Blocks:
    """column blocks of a guarded [rows + extra, ld] buffer: live(col0, cols) hands one out (NaN-filled: the kernels overwrite them
    fully); check(): the frames, every column no block owns and the extra rows still hold the sentinel"""

    def __init__(self, rows, ld, dt, dev, extra=3):
        self.g = RR.guarded((rows + extra, ld), dt, dev)
        self.rows, self.s = rows, RR._SENTINEL[dt]
        self.owned = torch.zeros(ld, dtype=torch.bool, device=dev)

    def live(self, col0, cols, shape):
        self.owned[col0:col0 + cols] = True
        v = self.g.view[:self.rows, col0:col0 + cols]
        v.fill_(NAN)
        return v.unflatten(0, shape)

    def check(self):
        self.g.check()
        assert bool((self.g.view[:self.rows][:, ~self.owned] == self.s).all()), "store into the columns between / behind the blocks"
        assert bool((self.g.view[self.rows:] == self.s).all()), "store into the rows below the output"


def check_offset(g):
    g.check()
    if g.offset:
        assert bool((g.view[:g.offset] == RR._SENTINEL[g.buf.dtype]).all()), "write in front of an offset output"


# ---- comparisons ------------------------------------------------------------------------------------------------------------------
def _worst(err, what):
    idx = tuple(int(i) for i in (err == err.max()).nonzero()[0])
    return f"{what}: worst at {idx}"


def finite(got, what):
    assert bool(torch.isfinite(got).all()), f"{what}: {int((~torch.isfinite(got)).sum())} of {got.numel()} elements are not finite"


def equal(cid, fam, name, got, want, dt):
    finite(got, f"{cid} {name}")
    got, want = got.detach().cpu(), want.to(dt)
    same = torch.equal(got, want)
    print(f"EXACT {cid} | {fam} | {name} | equal={same}")
    if not same:
        bad = got != want
        idx = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{cid} {name}: {int(bad.sum())} of {bad.numel()} elements differ, first at {idx}: "
                             f"{got[idx].item()} against {want[idx].item()}")


def bounded(cid, c, fam, name, got, ref, mag, eps=None):
    """per element |got - ref| <= u |ref| + eps mag; prints the largest error / bound and, over the elements with ref == 0, the
    largest error / mag (the measurement eps is set from)"""
    finite(got, f"{cid} {name}")
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    eps = eps_of(fam) if eps is None else eps
    bnd = AX.bound(ref, mag, AX.u_of(c, name), eps)
    err = (got - ref).abs()
    pos = bnd > 0
    ratio = float((err[pos] / bnd[pos]).max()) if bool(pos.any()) else 0.0
    zero = (ref == 0) & (mag > 0)
    e0 = float((err[zero] / mag[zero]).max()) if bool(zero.any()) else 0.0
    same = bool((got == ref).all())
    print(f"EXACT {cid} | {fam} | {name} | equal={same} ratio={ratio:.4f} eps0={e0:.3e} zeros={int(zero.sum())}")
    assert bool((err <= bnd).all()), _worst(err - bnd, f"{cid} {name}: {int((err > bnd).sum())} of {err.numel()} elements above the bound "
                                                          f"(largest error / bound {ratio:.3f}, error {float(err.max()):.3e})")


def lse_close(cid, fam, got, ref):
    finite(got, f"{cid} lse")
    got = got.detach().cpu().double()
    ulp = 2.0 ** (torch.floor(torch.log2(ref.abs().clamp(min=2.0 ** -100))) - 23)
    tol = (4 * ulp).clamp(min=2.0 ** -22)
    err = (got - ref).abs()
    print(f"EXACT {cid} | {fam} | lse | ratio={float((err / tol).max()):.4f}")
    assert bool((err <= tol).all()), _worst(err / tol, f"{cid} lse: {int((err > tol).sum())} elements off by more than 4 ulps")


# ---- the VALU kernels ---------------------------------------------------------------------------------------------------------------
def _valu(dev, cid, unaligned):
    H, attn = _mods()
    c, o, r = BY_ID[cid], operands(cid), reference(cid)
    G, R, heads, d, T1, T2, gd = (c[k] for k in ("G", "R", "heads", "d", "T1", "T2", "gd"))
    T, HD = T1 + T2, heads * d
    dt = F32 if c["dtype"] == "f32" else BF16
    tag = cid + ("-unaligned" if unaligned else "")
    held = []                    # the poisoned allocations stay alive until the kernels have run

    def put(name, flat=False):
        if o[name] is None:
            return None
        view, p = flat_operand(o[name], dev) if flat else operand(o[name], dt, dev)
        held.append(p)
        return view
    q, k1, v1, k2, v2 = (put(n) for n in ("q", "k1", "v1", "k2", "v2"))
    mask, bias = put("mask", True), put("bias", True)
    dout, pd = operand(o["dout"], dt, dev, ld=HD)                        # (dO is read with the output's dense strides)
    a = attn.desc(q, k1, v1, k2, v2, mask, bias, heads, gd, c["scale"], 0.0, 0, c["causal"], 0)
    # route
    want = UNALIGNED[cid] if unaligned else (KERNELS[c["row"]][:2] if dt == F32 else KERNELS[c["row"]][2:])
    has_dbias, is_grouped = bias is not None, grouped(c)
    plans = (attn.small_plan(a, ptrs_aligned=not unaligned), attn.small_plan(a, True, is_grouped, has_dbias, True, not unaligned))
    names = tuple(n[0] + (" + " + n[1] if n[1] else "") for _, _, n in plans)
    assert (plans[0][0], plans[1][0]) == (0, 0) and names == tuple(want), (tag, names)
    ffam, bfam = names
    # forward
    off = 8 // o["q"].to(dt).element_size() if unaligned else 0
    out, og = dense_out((G, R, HD), dt, dev, offset=off)
    lse, lg = dense_out((G, heads, R), F32, dev)
    assert (out.data_ptr() % 16 == 0) != unaligned
    attn.forward(a, out, lse, False)
    pr, pg = dense_out((G, heads, R, T), F32, dev)
    attn.probs(a, pr, heads * R * T, R * T, False)
    torch.cuda.synchronize()
    equal(tag, ffam, "out", out, r["out"], dt)
    equal(tag, "fcmf_attn_probs", "probs", pr, r["P"], F32)
    lse_close(tag, ffam, lse, r["lse"])
    check_offset(og)
    RR.check_all(lg, pg)
    # backward
    G2 = G // gd if is_grouped else G
    new = lambda *shape: dense_out(shape, dt, dev)
    (dk1, g1), (dv1, g2) = (new(G, T1, HD), new(G, T1, HD)) if T1 else ((None, None), (None, None))
    (dk2, g3), (dv2, g4) = (new(G2, R, T2, HD), new(G2, R, T2, HD)) if T2 else ((None, None), (None, None))
    dbias, g5 = dense_out((G, heads, R, T), F32, dev) if has_dbias else (None, None)
    scratch, g6 = dense_out((2 * G * heads * R * T2,), F32, dev) if is_grouped else (None, None)
    dq = attn.small_backward(a, out, dout, lse, out, dk1, dv1, dk2, dv2, dbias, scratch)
    torch.cuda.synchronize()
    per_g = AX.explicit(c, o, r["P"], False, sum_gd=False), AX.explicit(c, o, r["P"], True, sum_gd=False)
    for name, got in (("dq", dq), ("dk1", dk1), ("dv1", dv1), ("dk2", dk2), ("dv2", dv2), ("dbias", dbias)):
        if got is None:
            continue
        if name == "dbias" or (name in ("dk2", "dv2") and not is_grouped):      # written per group: the caller sums
            bounded(tag, c, bfam, name, got, per_g[0][name], per_g[1][name])
        else:
            bounded(tag, c, bfam, name, got, r[name], r["mag"][name])
    RR.check_all(g1, g2, g3, g4, g5, g6)
    check_offset(og)
    # the dq partials in a guarded buffer of the test's own: the same entry point, the same bits
    nch = max(1, (T1 + 127) // 128)
    part, gp = dense_out((nch, G, R, HD), dt, dev)
    ptrs = [H.ptr(t) for t in (out, dout, lse, part, dk1, dv1, dk2, dv2, dbias)]
    if is_grouped:
        H.check(H.lib().fcmf_attn_small_bwd_grouped(a, *ptrs, H.ptr(scratch), scratch.numel() * 4, H.stream()), "fcmf_attn_small_bwd_grouped")
    else:
        H.check(H.lib().fcmf_attn_small_bwd(a, *ptrs, H.stream()), "fcmf_attn_small_bwd")
    dq2 = attn.sum_leading(part)
    torch.cuda.synchronize()
    finite(part, f"{tag} dq partials")
    assert torch.equal(dq2, dq), f"{tag}: dq differs between two runs of the backward"
    RR.check_all(gp, g1, g2, g3, g4, g5, g6)
    del held, pd


@pytest.mark.parametrize("cid", VALU_IDS)
def test_valu_attention_exact(dev, cid):
    _valu(dev, cid, False)


@pytest.mark.parametrize("cid", sorted(UNALIGNED))
def test_valu_attention_unaligned_out_takes_the_general_kernels(dev, cid):
    """`out` 8 bytes off a 16-byte boundary: the tiny / flat kernels give way (test_attn_exact_cpu.UNALIGNED names the general
    kernels that take over), and those meet the same reference under the same bounds"""
    _valu(dev, cid, True)


# ---- the MFMA kernels ---------------------------------------------------------------------------------------------------------------
def _nan_rows(rows, ld, dt, dev, extra=2):
    p = GR.poisoned(torch.zeros(rows, ld, dtype=dt), ld, extra, dev)
    p.view.fill_(NAN)
    return p


@pytest.mark.parametrize("layout", ["separate", "fused"])
@pytest.mark.parametrize("cid", MFMA_IDS)
def test_mfma_attention_exact(dev, cid, layout):
    """separate: q, k, v padded tensors of their own, the gradients laid out like them.  fused: q | k | v as column blocks of a
    [G*T, 3*Hd + 8] buffer whose 8 extra columns are NaN (Tq != Tk: q in a [G*Tq, .] buffer, k | v in a [G*Tk, .] one, the unused
    blocks NaN), dq | dk | dv as the same blocks of guarded dqkv buffers"""
    H, attn = _mods()
    c, o, r = BY_ID[cid], operands(cid), reference(cid)
    G, Tq, Tk, heads = c["G"], c["R"], c["T1"], c["heads"]
    HD = heads * 64
    tag = f"{cid}-{layout}"
    if layout == "separate":
        ld = HD + PAD
        (q, pq), (k, pk), (v, pv) = (operand(o[n], BF16, dev) for n in ("q", "k1", "v1"))
        bq, bk, bv = Blocks(G * Tq, ld, BF16, dev), Blocks(G * Tk, ld, BF16, dev), Blocks(G * Tk, ld, BF16, dev)
        dq, dk, dv = bq.live(0, HD, (G, Tq)), bk.live(0, HD, (G, Tk)), bv.live(0, HD, (G, Tk))
        grads = (bq, bk, bv)
    else:
        ld = 3 * HD + PAD
        pq = _nan_rows(G * Tq, ld, BF16, dev)
        pk = pq if Tq == Tk else _nan_rows(G * Tk, ld, BF16, dev)
        q, k, v = pq.view[:, :HD].unflatten(0, (G, Tq)), pk.view[:, HD:2 * HD].unflatten(0, (G, Tk)), pk.view[:, 2 * HD:3 * HD].unflatten(0, (G, Tk))
        q.copy_(o["q"].to(BF16)), k.copy_(o["k1"].to(BF16)), v.copy_(o["v1"].to(BF16))
        bq = Blocks(G * Tq, ld, BF16, dev)
        bk = bq if Tq == Tk else Blocks(G * Tk, ld, BF16, dev)
        dq, dk, dv = bq.live(0, HD, (G, Tq)), bk.live(HD, HD, (G, Tk)), bk.live(2 * HD, HD, (G, Tk))
        grads = (bq, bk)
    mask, pm = flat_operand(o["mask"], dev)
    dout, pd = operand(o["dout"], BF16, dev, ld=HD)
    a = attn.desc(q, k, v, None, None, mask, None, heads, 1, c["scale"], 0.0, 0, False, 0)
    assert attn.mfma_eligible(a) and attn._ld(a) == (ld, ld) and v.stride() == k.stride()
    out, og = dense_out((G, Tq, HD), BF16, dev)
    lse, lg = dense_out((G, heads, Tq), F32, dev)
    attn.forward(a, out, lse, True)
    pr, pg = dense_out((G, heads, Tq, Tk), F32, dev)
    attn.probs(a, pr, heads * Tq * Tk, Tq * Tk, True)
    torch.cuda.synchronize()
    equal(tag, "fcmf_attn_mfma_fwd", "out", out, r["out"], BF16)
    equal(tag, "fcmf_attn_mfma_probs", "probs", pr, r["P"], F32)
    lse_close(tag, "fcmf_attn_mfma_fwd", lse, r["lse"])
    RR.check_all(og, lg, pg)
    fam = "fcmf_attn_mfma_bwd"
    ref_cs = torch.cat([r["dq"].sum(1), r["dk1"].sum(1), r["dv1"].sum(1)], -1)
    mag_cs = torch.cat([r["mag"]["dq"].sum(1), r["mag"]["dk1"].sum(1), r["mag"]["dv1"].sum(1)], -1)
    first = None
    for with_colsum in (False, True):
        cs, cg = dense_out((G, 3 * HD), F32, dev) if with_colsum else (None, None)
        for t in (dq, dk, dv):
            t.fill_(NAN)
        attn.mfma_backward(a, out, dout, lse, H.ptr(dq), H.ptr(dk), H.ptr(dv), cs)
        torch.cuda.synchronize()
        for name, got in (("dq", dq), ("dk1", dk), ("dv1", dv)):
            bounded(f"{tag}-colsum{int(with_colsum)}", c, fam, name, got, r[name], r["mag"][name])
        if with_colsum:
            bounded(tag, dict(c, dtype="f32"), fam, "colsum_part", cs, ref_cs, mag_cs)
            err = (cs.cpu().double() - ref_cs).abs()
            assert bool((err <= eps_of(fam) * mag_cs).all()), _worst(err, f"{tag} colsum_part beyond eps * mag")
            assert all(torch.equal(x, y) for x, y in zip(first, (dq, dk, dv))), f"{tag}: gradients change with colsum_part"
        first = tuple(t.clone() for t in (dq, dk, dv))
        for b in grads:
            b.check()
        RR.check_all(cg, og, lg)
    del pq, pk, pm, pd


# ---- the long-key kernels -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", LONG_IDS)
def test_long_attention_exact(dev, cid):
    H, attn = _mods()
    c, o, r = BY_ID[cid], operands(cid), reference(cid)
    G, Tq, Tk, heads, kv = c["G"], c["R"], c["T1"], c["heads"], c["kv"]
    HD = heads * 64
    (q, pq), (k, pk), (v, pv), (dout, pd) = (operand(o[n], BF16, dev, ld=HD) for n in ("q", "k1", "v1", "dout"))     # dense: poisoned outside
    mask, pm = flat_operand(o["mask"], dev)
    assert all(t.is_contiguous() for t in (q, k, v, dout, mask))
    out, og = dense_out((G, Tq, HD), BF16, dev)
    lse, lg = dense_out((G, heads, Tq), F32, dev)
    attn.long_forward(q, k, v, mask, out, lse, heads, kv, c["scale"], 0.0, 0)
    pr, pg = dense_out((G, heads, Tq, Tk), F32, dev)
    pmean, pmg = dense_out((G, Tq, Tk), F32, dev)
    attn.long_probs(q, k, mask, pr, heads, kv, c["scale"], False)
    attn.long_probs(q, k, mask, pmean, heads, kv, c["scale"], True)
    torch.cuda.synchronize()
    equal(cid, "fcmf_attn_mfma_long_fwd", "out", out, r["out"], BF16)
    equal(cid, "fcmf_attn_mfma_long_probs", "probs", pr, r["P"], F32)
    equal(cid, "fcmf_attn_mfma_long_probs", "probs, head mean", pmean, r["P"].mean(1), F32)
    lse_close(cid, "fcmf_attn_mfma_long_fwd", lse, r["lse"])
    RR.check_all(og, lg, pg, pmg)
    fam = "fcmf_attn_mfma_long_bwd"
    (dq, g1), (dk, g2), (dv, g3) = (dense_out(s, BF16, dev) for s in ((G, Tq, HD), (G // kv, Tk, HD), (G // kv, Tk, HD)))
    attn.long_backward(q, k, v, mask, out, dout, lse, dq, dk, dv, heads, kv, c["scale"], 0.0, 0)
    torch.cuda.synchronize()
    for name, got in (("dq", dq), ("dk1", dk), ("dv1", dv)):
        bounded(cid, c, fam, name, got, r[name], r["mag"][name])
    RR.check_all(g1, g2, g3, og, lg)
    if kv > 1:      # the workspace in a guarded, NaN-filled buffer of the test's own ("contents need not be initialised")
        first = tuple(t.clone() for t in (dq, dk, dv))
        for t in (dq, dk, dv):
            t.fill_(NAN)
        ws, gw = dense_out((2 * k.numel(),), F32, dev)
        H.check(H.lib().fcmf_attn_mfma_long_bwd(H.ptr(q), H.ptr(k), H.ptr(v), H.ptr(mask), H.ptr(out), H.ptr(dout), H.ptr(lse), H.ptr(dq),
                                                H.ptr(dk), H.ptr(dv), G, heads, Tq, Tk, kv, HD, HD, HD, c["scale"], 0.0, 0, H.ptr(ws),
                                                ws.numel() * 4, H.stream()), "fcmf_attn_mfma_long_bwd")
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(first, (dq, dk, dv))), f"{cid}: gradients depend on the workspace's contents"
        RR.check_all(gw, g1, g2, g3)
    del pq, pk, pv, pd, pm
