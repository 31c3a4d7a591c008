"""What tests/test_attn_exact_gpu.py relies on, checked without a GPU: the case table and the kernels its VALU cases reach (the
host plan, attn.small_plan), the exactness preconditions of the selected-key operands (tests/attn_exact_ref.py), and the
sensitivity of the float64 reference: a lost key, a lost query row, two swapped heads, a V read one row off, or a key mask, bias
or causal fill that is not applied move some element
of the affected outputs by at least 8 times that element's bound, evaluated at the cap eps = 2^-14 of the GPU test.

Which outputs a perturbation must move: a removed key, `out`, dq, dbias and the dk / dv of the key's own segment (a row whose
selected keys are all shared never looks at its private keys, before or after); a removed query row and swapped heads, `out` and
every gradient (a removed row: the key gradients of the segments it has selected keys in); V shifted by one row, everything but dv (dv = P^T dO does not read V).  Heads are swapped where there are two.

One precondition of the issue is narrowed, and asserted as narrowed: `out`, P and dS are representable in the output dtype
(bf16 included), which is what equality of the forward and exactness of the MFMA backward's bf16 operands rest on; the GRADIENT
references are sums of up to 256 such dS terms and are float32 values, not bf16 grid values (dk of a 256-row fully masked group
cannot be), so a bf16 gradient is one rounding away from its reference -- the u |ref| term of the bound, not equality."""
import functools

import pytest
import torch

import attn_exact_ref as AX
from test_attn_small_plan_cpu import BF16, BWD, F32, FWD, KERNELS, OK, PRIV
from test_ops_gpu import ATTN_CASES

SCALES = (0.125, 0.25)
MFMA_SHAPES = [(1, 1), (33, 17), (77, 128), (128, 97), (130, 129), (200, 256), (256, 256)]                # Tq, Tk
LONG_SHAPES = [(6, 3, 77, 300), (2, 1, 64, 515), (4, 2, 40, 1030)]                                        # G, kv_share, Tq, Tk
PAD = 8                  # extra (NaN) columns behind every operand row


def _case(kind, cid, dtype, G, R, heads, d, T1, T2, gd, kv, mask, bias, causal, n):
    return dict(kind=kind, id=cid, dtype=dtype, G=G, R=R, heads=heads, d=d, T1=T1, T2=T2, gd=gd, kv=kv, mask=mask, bias=bias,
                causal=causal, scale=SCALES[n % 2], seed=1000 * (n + 1), row=n)


CASES = []
for _i, (_G, _R, _h, _d, _T1, _T2, _gd, _m, _b, _c) in enumerate(ATTN_CASES):
    for _dt in ("f32", "bf16"):
        CASES.append(_case("valu", f"valu{_i:02d}-{_dt}", _dt, _G, _R, _h, _d, _T1, _T2, _gd, 1, _m, _b, _c, _i))
for _i, (_Tq, _Tk) in enumerate(MFMA_SHAPES):
    CASES.append(_case("mfma", f"mfma-{_Tq}x{_Tk}", "bf16", 3, _Tq, 2, 64, _Tk, 0, 1, 1, True, False, False, 40 + _i))
for _i, (_G, _kv, _Tq, _Tk) in enumerate(LONG_SHAPES):
    CASES.append(_case("long", f"long-{_G}g{_kv}-{_Tq}x{_Tk}", "bf16", _G, _Tq, 2, 64, _Tk, 0, 1, _kv, True, False, False, 50 + _i))
BY_ID = {c["id"]: c for c in CASES}
IDS = list(BY_ID)
# one case per dense family repeats with `out` 8 bytes off a 16-byte boundary: the general kernels must take it over
UNALIGNED = {"valu14-bf16": (FWD % "bf16_t, 4, 0", BWD % "bf16_t, true, false"),                     # tiny
             "valu10-bf16": (FWD % "bf16_t, 4, 64", BWD % "bf16_t, true, true" + PRIV % "bf16_t")}   # flat


@functools.lru_cache(maxsize=None)
def operands(cid):
    return AX.build(BY_ID[cid])


@functools.lru_cache(maxsize=None)
def reference(cid):
    """computed once per process and shared by every test of the case; nobody writes into it"""
    return AX.reference(BY_ID[cid], operands(cid))


def grouped(c):
    """the backward entry point ops.attention takes: grouped whenever there are private keys and group_div <= 8"""
    return c["T2"] > 0 and c["gd"] <= 8 and c["G"] % c["gd"] == 0


def plan_names(c, aligned=True):
    """-> (forward, backward) kernel names of a VALU case with the GPU test's padded row strides (fake addresses: the plan
    reads none)"""
    from fcmf_framework import _hip, attn
    G, R, heads, d, T1, T2 = (c[k] for k in ("G", "R", "heads", "d", "T1", "T2"))
    HD = heads * d
    ld = HD + PAD
    a = _hip.AttnDesc()
    a.dtype, a.G, a.heads, a.d, a.R, a.T1, a.T2, a.group_div = (F32 if c["dtype"] == "f32" else BF16), G, heads, d, R, T1, T2, c["gd"]
    a.q_sg, a.q_sr, a.o_sg, a.o_sr, a.q = R * ld, ld, R * HD, HD, 0x10000000
    if T1:
        a.k1_sg, a.k1_st, a.k1, a.v1 = T1 * ld, ld, 0x20000000, 0x28000000
    if T2:
        a.k2_sg, a.k2_sr, a.k2_st, a.k2, a.v2 = R * T2 * ld, T2 * ld, ld, 0x30000000, 0x38000000
    a.mask = 0x78000000 if c["mask"] else None
    a.bias = 0x80000000 if c["bias"] else None
    a.scale, a.dropout_p, a.seed, a.causal = c["scale"], 0.0, 0, int(c["causal"])
    out = []
    for rc, _, names in (attn.small_plan(a, ptrs_aligned=aligned), attn.small_plan(a, True, grouped(c), c["bias"], True, aligned)):
        assert rc == OK, c["id"]
        out.append(names[0] + (" + " + names[1] if names[1] else ""))
    return tuple(out)


def test_case_table():
    assert len(IDS) == len(CASES) == 2 * len(ATTN_CASES) + len(MFMA_SHAPES) + len(LONG_SHAPES)
    for c in CASES:
        assert c["scale"] in SCALES and 128.0 / c["scale"] in (512.0, 1024.0)
        if c["kind"] != "valu":
            assert c["dtype"] == "bf16" and c["d"] == 64 and c["R"] <= 256 and (c["kind"] == "long" or c["T1"] <= 256)
    assert any(AX.full_group(c) is not None for c in CASES if c["kind"] == "mfma")
    assert any(AX.full_group(c) is not None for c in CASES if c["kind"] == "valu" and c["dtype"] == "bf16")


def test_valu_cases_reach_every_kernel_of_the_plan_table():
    reached = set()
    for c in CASES:
        if c["kind"] == "valu":
            want = KERNELS[c["row"]][:2] if c["dtype"] == "f32" else KERNELS[c["row"]][2:]
            assert plan_names(c) == tuple(want), c["id"]
            reached |= set(want)
    assert reached == {n for row in KERNELS for n in row}
    for cid, general in UNALIGNED.items():
        assert ("tiny" in plan_names(BY_ID[cid])[0]) or ("flat" in plan_names(BY_ID[cid])[0])
        assert plan_names(BY_ID[cid], aligned=False) == general, cid
    assert {("tiny" in plan_names(BY_ID[cid])[0]) for cid in UNALIGNED} == {True, False}


@pytest.mark.parametrize("cid", IDS)
def test_preconditions(cid):
    c, o, r = BY_ID[cid], operands(cid), reference(cid)
    G, R, heads, T = c["G"], c["R"], c["heads"], c["T1"] + c["T2"]
    dt = torch.float32 if c["dtype"] == "f32" else torch.bfloat16
    gfull = o["gfull"]
    # operands exact in the case's dtype
    for name in ("q", "k1", "v1", "k2", "v2", "dout"):
        assert o[name] is None or AX.representable(o[name], torch.bfloat16), name
    # live selected keys per row: 1, 2 or 4 (T in the fully masked group), and the probabilities that follow
    count = o["count"]
    normal = torch.ones(G, dtype=torch.bool)
    if gfull is not None:
        assert bool((count[gfull] == T).all()) and T & (T - 1) == 0
        normal[gfull] = False
    assert bool(((count[normal] == 1) | (count[normal] == 2) | (count[normal] == 4)).all())
    assert len(count[normal].unique()) >= (2 if T > 2 else 1)
    want_P = o["sel"].double() / count[..., None].double()
    assert torch.equal(r["P"], want_P)                                   # exactly 0, 1, 1/2, 1/4 (1/T): float64 sees exp(-128) = 1e-56 ...
    assert set(r["P"].unique().tolist()) <= {0.0, 1.0, 0.5, 0.25, 1.0 / T}
    assert torch.equal(r["lse"][normal], count[normal].double().log())
    # what is asserted EQUAL on the GPU is representable in the output dtype; dS is a bf16 MFMA operand
    assert AX.representable(r["out"], dt) and AX.representable(r["P"], torch.bfloat16)
    assert AX.ds_grid_ok(c, o, r["P"])
    for name in ("dq", "dk1", "dv1", "dk2", "dv2", "dbias"):
        assert r[name] is None or AX.representable(r[name], torch.float32), name
    # every boundary position is a live selected key of some row
    seen = o["sel"][normal].any(0).any(0).any(0) if gfull is not None else o["sel"].any(0).any(0).any(0)
    missing = [t for t in AX.must_positions(c["T1"], c["T2"]) if not seen[t]]
    assert not missing, missing
    if c["mask"]:                                                        # the mask removed a key some row would have selected
        hit = (o["mask"] != 0)[:, None, None, :] & (o["kc"] == o["qc"][..., None])
        assert bool(hit[normal].any()) or T <= 2
    if c["bias"]:                                                        # a knock-out removed a key some row would have selected
        hit = (o["bias"].repeat_interleave(c["gd"], 0) != 0) & (o["kc"] == o["qc"][..., None])
        assert bool(hit.any())
    # no two heads of a group look alike
    for g in range(G):
        for h in range(1, heads):
            assert not torch.equal(o["sel"][g, h], o["sel"][g, 0]) or (R == 1 and T <= 2) or g == gfull
    # the written-out sums (the magnitudes' formulas) are the autograd gradients
    ex = AX.explicit(c, o, r["P"], False)
    for name in ("out", "dq", "dk1", "dv1", "dk2", "dv2", "dbias"):
        assert (r[name] is None) == (ex[name] is None), name
        if r[name] is not None:
            assert torch.equal(ex[name], r[name]) or float((ex[name] - r[name]).abs().max()) <= 1e-12 * float(r["mag"][name].max()), name
            assert bool((r["mag"][name] >= r[name].abs() * (1 - 1e-12)).all()), name
    # all four gradients are non-trivial where the layout says so
    dc, nq, nk = AX.head_split(c["d"])
    qh = AX.heads_first(r["dq"], heads)[normal]
    assert bool((qh[..., :dc + nq] == 0).all()) and bool((qh[..., dc + nq:] != 0).any()) or T == 1
    if r["dk1"] is not None and T > 1 and c["kv"] == 1:
        kh = AX.heads_first(r["dk1"], heads)[normal]
        assert bool((kh[..., :dc] != 0).any()) and bool((kh[..., dc:dc + nq] != 0).any()) and bool((kh[..., dc + nq:] == 0).all())


# ---- sensitivity ------------------------------------------------------------------------------------------------------------------
OUTPUTS = ("out", "dq", "dk1", "dv1", "dk2", "dv2", "dbias")


def _moved(c, base, pert, names):
    """every output in `names` has an element that moved by >= 8 bounds (eps at its cap)"""
    for name in names:
        if base[name] is None:
            continue
        bnd = AX.bound(base[name], base["mag"][name], AX.u_of(c, name), AX.EPS_CAP)
        diff = (pert[name] - base[name]).abs()
        if not bool((diff >= 8 * bnd)[diff > 0].any()):
            return name
    return None


def _with(o, **changed):
    o2 = dict(o)
    o2.update(changed)
    return o2


def _perturbations(c, o):
    """-> [(what, the outputs it must move, perturbed operands, post-processing of the perturbed reference)]"""
    G, R, heads, d, T1, T2 = (c[k] for k in ("G", "R", "heads", "d", "T1", "T2"))
    T = T1 + T2
    gen = torch.Generator().manual_seed(c["seed"])
    gfull = o["gfull"]
    res = []
    # a key some row selects, dropped for its whole group: each boundary position once, and three more
    sel_gt = o["sel"].any(1).any(1)                                      # [G,T]
    if gfull is not None:
        sel_gt[gfull] = False
    picks = []
    for t in AX.must_positions(T1, T2):
        gs = sel_gt[:, t].nonzero().flatten().tolist()
        picks.append((gs[t % len(gs)], t))
    cand = sel_gt.nonzero().tolist()
    picks += [tuple(cand[i]) for i in torch.randint(0, len(cand), (3,), generator=gen).tolist()]
    for g, t in dict.fromkeys(picks):
        if T == 1:
            continue                                                      # (the only key of a row cannot be dropped)
        mask = torch.zeros(G, T, dtype=torch.float64) if o["mask"] is None else o["mask"].clone()
        mask[g, t] = AX.FMIN
        seg = ("dk1", "dv1") if t < T1 else ("dk2", "dv2")
        res.append((f"key {t} of group {g} removed", ("out", "dq", "dbias") + seg, _with(o, mask=mask), None))
    # a query row dropped: its out and dq rows are never written, the key gradients lose its term
    rows = (reference(c["id"])["dq"] != 0).any(-1).nonzero().tolist()     # (a row with ONE selected key has dS = 0, dq = 0)
    every = OUTPUTS if rows else ("out", "dv1", "dv2")                    # (one key in all: no dS at all)
    rows = rows or [[0, 0], [G - 1, R - 1]]
    for g, r in [rows[0], rows[-1]] + [rows[i] for i in torch.randint(0, len(rows), (2,), generator=gen).tolist()]:
        dout = o["dout"].clone()
        dout[g, r] = 0

        def post(ref, g=g, r=r):
            ref["out"] = ref["out"].clone()
            ref["out"][g, r] = 0
        looks = o["sel"][g, :, r]                                         # (a row moves the key gradients of the segments it selects in)
        names = [n for n in every if n not in ("dk1", "dv1", "dk2", "dv2")]
        names += ["dk1", "dv1"] * bool(looks[:, :T1].any()) + ["dk2", "dv2"] * bool(looks[:, T1:].any())
        res.append((f"query row {r} of group {g} removed", tuple(n for n in names if n in every), _with(o, dout=dout), post))
    # two heads of the queries swapped in one group
    for g in range(G if heads >= 2 and T > 1 else 0):
        if g != gfull:
            q = o["q"].clone().view(G, R, heads, d)
            q[g, :, [0, 1]] = q[g, :, [1, 0]]
            res.append((f"heads 0 and 1 of group {g} swapped", every, _with(o, q=q.reshape(G, R, heads * d)), None))
    # the key mask, the bias or the causal fill not applied at all
    seg = ("dk1", "dv1") if T1 else ("dk2", "dv2")
    if o["mask"] is not None and (T1 >= 12 or T2 >= 5):
        res.append(("mask not applied", ("out", "dq", "dbias") + seg, _with(o, mask=None), None))
    if o["bias"] is not None:
        res.append(("bias not applied", ("out", "dq", "dbias") + seg, _with(o, bias=torch.zeros_like(o["bias"])), None))
    if c["causal"]:
        pert_c = dict(c, causal=False)
        res.append(("causal fill not applied", ("out", "dq") + seg, o, lambda ref: ref.update(AX.raw(pert_c, o))))
    # V read one row off
    if T > 1:
        roll = lambda v, dim: None if v is None else torch.roll(v, 1, dim)
        res.append(("v shifted by one row", ("out", "dq", "dk1", "dk2", "dbias"), _with(o, v1=roll(o["v1"], 1), v2=roll(o["v2"], 2)), None))
    return res


@pytest.mark.parametrize("cid", IDS)
def test_reference_is_sensitive_at_the_cap(cid):
    c, o, base = BY_ID[cid], operands(cid), reference(cid)
    perts = _perturbations(c, o)
    assert len(perts) >= (4 if c["T1"] + c["T2"] == 1 else 8)
    swaps = []
    for what, names, o2, post in perts:
        pert = AX.raw(c, o2)
        if post is not None:
            post(pert)
        if "swapped" in what and c["T1"] + c["T2"] <= 2:
            swaps.append(_moved(c, base, pert, names))                   # (two keys, one row: two heads of a group can agree)
            continue
        assert _moved(c, base, pert, names) is None, (what, _moved(c, base, pert, names))
    assert not swaps or None in swaps
