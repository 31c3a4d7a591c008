""""Selected-key" attention operands whose probabilities are exactly 0, 1, 1/2 or 1/4, and their float64 reference with the
per-element magnitudes the error bounds of tests/test_attn_exact_gpu.py are stated in.  Plain module: no fixtures, and nothing
here calls the library.

The d columns of a head are split into code | query-payload | key-payload columns (d/2 | d/4 | rest).  A query row with code c holds
-B in every code column but column c (0 there), dyadic entries ({-1, 0, 1} * 2^-1) in its query-payload columns and zeros in its
key-payload columns.  A coded key with code c' holds the unit vector e_c' in the code columns, zeros in the query-payload columns
and dyadic entries in its key-payload columns; an uncoded ("dead") key holds ones in ALL code columns.  With scale a power of two
and B * scale = 128 the score of (row, key) is the ONE product that survives: exactly 0 where the codes agree, -128 where they
differ, -(dc - 1) * 128 or lower for a dead key.  exp(-128) is 0 in float32, so in any summation order, and through an online
rescaling (whose factors are exp(0) or 0), the probabilities are 1/m on the m "selected" keys of a row and 0 elsewhere; m is 1, 2
or 4 (T for a deliberately fully masked group, T a power of two), so P, every P v product and every partial sum of them is exact
in float32 and in bf16.  A key mask (-1e4 or finfo.min), the causal fill and a bias of -256 each REMOVE keys (exp(-256) = 0 too).

The backward is made exact as well.  dout has at most 8 (d % 8 == 0; else all d / every second) non-zero columns per head and row,
so dP = dO . v is a small integer, delta = sum_t P dP a multiple of 1/m and dS = P (dP - delta) a multiple of 1/m^2 that a bf16
MFMA operand holds exactly (`ds_grid_ok` asserts |n| <= 256).  In a fully masked group the columns of v sum to 0, +-T/2 or +-T/4
over the keys, which keeps delta on a grid of 1/4 and dS = (dP - delta) / T exact.  What is NOT exact is the float32 logsumexp
(log 2, log 4, log T) from which a backward recomputes P, and __expf of it: that is the `eps * mag` term of the bound.

mag: for each output the same sum as the reference, taken over the absolute values of its terms: sum_t P |v| (out),
sum_r P |dO| (dv), scale sum |dS| |k| (dq), scale sum |dS| |q| (dk), |dS| (dbias); sums over sharing groups included."""
import torch

import gemm_ref as GR
from attn_ref import attention_ref

BOUNDARIES = (16, 32, 64, 128, 256, 512, 1024)    # key tile / chunk edges of the kernels: both sides of each are selected somewhere
COUNTS = (1, 2, 4, 2, 1, 4)
KNOCK = -256.0                                    # the bias entry that removes a key
FMIN = float(torch.finfo(torch.float32).min)
EPS_CAP = 2.0 ** -14


def head_split(d):
    """-> (code, query-payload, key-payload) column counts of a head"""
    dc, nq = max(2, d // 2), max(1, d // 4)
    return dc, nq, d - dc - nq


def must_positions(T1, T2):
    """the key positions (shared first, then private) that have to be a selected, live key of some row of a case"""
    T = T1 + T2
    pos = {0, T - 1, max(0, T - 2)}
    pos |= {t for b in BOUNDARIES if b < T for t in (b - 1, b)}
    if T1:
        pos |= {0, T1 - 1}
    if T2:
        pos |= {T1, T - 1}
    return sorted(pos)


def _rot(seq, n):
    seq = list(seq)
    n %= max(1, len(seq))
    return seq[n:] + seq[:n]


def _perm(n, seed):
    return torch.randperm(n, generator=torch.Generator().manual_seed(seed)).tolist()


def _place(codes, counts, first_code, wanted, n_keys, seed, avoid=()):
    """writes first_code, first_code + 1, ... onto counts[i] positions each: the wanted positions first, then seeded filler"""
    order = [t for t in dict.fromkeys(list(wanted) + _perm(n_keys, seed)) if t not in avoid]
    at = 0
    for i, cnt in enumerate(counts):
        for t in order[at:at + cnt]:
            codes[t] = first_code + i
        at += cnt


def _fit(counts, room):
    counts = list(counts)
    while counts and sum(counts) > room:
        counts.pop()
    return counts or ([1] if room >= 1 else [])


def key_codes(c):
    """-> kc1 [G/kv, heads, T1], kc2 [G/gd, heads, R, T2] (int64, -1 = dead key), number of codes.  Shared codes 0 .. ns-1 on 1, 2
    or 4 keys each; with both segments, code ns on shared AND private keys (1 + 1 or 2 + 2: a row's selected keys then straddle
    the segment boundary); then up to three codes on the private keys only, per row.  The placement rotates with (group, head)
    and, for the private keys, with the row."""
    G, R, heads, d, T1, T2, gd, kv = (c[k] for k in ("G", "R", "heads", "d", "T1", "T2", "gd", "kv"))
    dc = head_split(d)[0]
    must = must_positions(T1, T2)
    m1, m2 = [t for t in must if t < T1], [t - T1 for t in must if t >= T1]
    mixed = T2 >= 2 and T1 >= 3
    n_priv = min(3, T2)                                                   # private-only codes per row
    has_victim = any(victims(c, 0))
    ns = 0 if not T1 else min(4, dc - n_priv - int(mixed) - int(has_victim))
    c_mixed, c_victim = ns, ns + int(mixed) + n_priv
    kc1 = torch.full((G // kv, heads, T1), -1, dtype=torch.int64)
    kc2 = torch.full((G // gd, heads, R, T2), -1, dtype=torch.int64)
    for g in range(G // kv if T1 else 0):
        for h in range(heads):
            p = g * heads + h
            cm = (1 + h % 2) if mixed else 0
            v1 = victims(c, g)[0]
            counts = _fit(_rot(COUNTS, p)[:ns], T1 - cm - len(v1))
            n_coded = sum(counts) + cm
            wanted = _rot(m1, p * n_coded)
            if c["causal"]:
                wanted = [0] + [t for t in wanted if t != 0]          # key 0 alone on a code: what row 0 of a causal case can see
                counts = [1] + counts[1:]
            _place(kc1[g, h], counts, 0, wanted, T1, 1000 + p, v1)
            kc1[g, h, v1] = c_victim
            if cm:
                free = [t for t in _rot(m1, p * n_coded + sum(counts)) + _perm(T1, 2000 + p) if kc1[g, h, t] < 0 and t not in v1]
                for t in list(dict.fromkeys(free))[:cm]:
                    kc1[g, h, t] = c_mixed
    for g in range(G // gd if T2 else 0):
        for h in range(heads):
            cm = (1 + h % 2) if mixed else 0
            v2 = victims(c, g)[1]
            for r in range(R):
                p = (g * heads + h) * R + r
                counts = _fit(_rot(COUNTS, p)[:n_priv], T2 - cm - len(v2)) if T2 - cm != 2 else ([1, 1], [2])[p % 3 == 2]
                wanted = _rot(m2, p * (sum(counts) + cm))
                _place(kc2[g, h, r], ([cm] if cm else []) + counts, c_mixed if cm else ns, wanted, T2, 3000 + p, v2)
                kc2[g, h, r, v2] = c_victim
    return kc1, kc2, c_victim + int(has_victim)


def victims(c, key_set):
    """-> (shared positions, private positions) of the "victim" code of a case with a key mask: two keys off the boundary
    positions, the same in every head and row of a key set (they move with the key set), which no other code is placed on.  The
    mask removes the first of the two in every group, so the code has ONE live key, rows select it, and a mask that is not
    applied shows in every head.  Shared keys if there are enough of them, else private ones, else none."""
    T1, T2 = c["T1"], c["T2"]
    if not c["mask"]:
        return [], []
    must = must_positions(T1, T2)
    free1 = [t for t in range(1, T1) if t not in must]
    free2 = [t for t in range(T2) if t + T1 not in must and t + T1 > 0]
    pick = lambda free: [free[(3 * key_set) % len(free)], free[(3 * key_set + 1) % len(free)]]
    if len(free1) >= 4 and T1 >= 12:
        return pick(free1), []
    if len(free2) >= 4:
        return [], pick(free2)
    return [], []


def key_mask(c, kc, gfull):
    """[G, T] additive: -1e4 in the even groups, finfo.min in the odd ones, on every second key that no head and row of the
    group has a code on (key 0 never), and in head g % heads on one key of a two-key code and two keys of a four-key code (they
    become one-key and two-key codes; the boundary positions are spared).  Whatever that does to the other heads' codes, a
    row only ever takes a code with 1, 2 or 4 LIVE keys."""
    G, heads, T1, T = c["G"], c["heads"], c["T1"], c["T1"] + c["T2"]
    must = set(must_positions(c["T1"], c["T2"]))
    mask = torch.zeros(G, T, dtype=torch.float64)
    uses = (kc >= 0).sum((1, 2))                                          # [G,T]
    for g in range(G):
        value = -1e4 if g % 2 == 0 else FMIN
        dead = [t for t in (uses[g] == 0).nonzero().flatten().tolist() if t > 0][g % 2::2]
        if not dead and T > 2:
            dead = [1 + int(uses[g, 1:].argmin())]
        row = kc[g, g % heads, 0, :T1]
        done = set()
        for code in row.unique().tolist():
            at = [t for t in (row == code).nonzero().flatten().tolist() if t not in must and t > 0]
            n = int((row == code).sum())
            if code >= 0 and n in (2, 4) and n not in done and len(at) >= n // 2:
                dead += at[:n // 2]
                done.add(n)
        v1, v2 = victims(c, g // c["kv"])[0], victims(c, g // c["gd"])[1]
        dead += v1[:1] + [T1 + t for t in v2[:1]]
        mask[g, dead] = value
    if gfull is not None:
        mask[gfull] = FMIN
    return mask


def full_group(c):
    """the group whose every key carries the finfo.min mask (uniform 1/T rows), or None: only with a mask, a power-of-two T and
    a second group to put it in"""
    T = c["T1"] + c["T2"]
    return 1 if c["mask"] and c["G"] >= 2 and T & (T - 1) == 0 and not c["causal"] else None


def build(c):
    """the operands of a case as float64 CPU tensors (every entry exact in bf16) and what the tests need to know about them:
    q, k1, v1, k2, v2, mask, bias, dout; kc [G,heads,R,T] the code of every key as row r sees it, qc [G,heads,R] the rows' codes,
    live [G,heads,R,T] (not masked, not causally filled, not knocked out), sel = live & (kc == qc), count = sel.sum(-1)"""
    G, R, heads, d, T1, T2, gd, kv = (c[k] for k in ("G", "R", "heads", "d", "T1", "T2", "gd", "kv"))
    T, HD, seed = T1 + T2, heads * d, c["seed"]
    dc, nq, nk = head_split(d)
    B = 128.0 / c["scale"]
    kc1, kc2, ncodes = key_codes(c)
    gfull = full_group(c)

    def keys(kc, s):
        """[..., heads, T?] codes -> [..., T?, heads, d] keys"""
        kc = kc.movedim(1, -1)                                               # heads last
        k = torch.zeros(kc.shape + (d,), dtype=torch.float64)
        k[..., :dc] = torch.where(kc[..., None] < 0, 1.0, 0.0)
        coded = kc >= 0
        k[..., :dc][coded] = torch.nn.functional.one_hot(kc[coded], dc).double()
        k[..., dc + nq:] = GR.dyadic(kc.shape + (nk,), s, 1)
        return k

    k1 = v1 = k2 = v2 = None
    if T1:
        k1 = keys(kc1, seed + 1).reshape(G // kv, T1, HD)                    # kc1 [G1,heads,T1] -> [G1,T1,heads,d]
        v1 = GR.dyadic((G // kv, T1, HD), seed + 2)
    if T2:
        k2 = keys(kc2, seed + 3).reshape(G // gd, R, T2, HD)                 # kc2 [G2,heads,R,T2] -> [G2,R,T2,heads,d]
        v2 = GR.dyadic((G // gd, R, T2, HD), seed + 4)
    parts = []
    if T1:
        parts.append(kc1.repeat_interleave(kv, 0)[:, :, None, :].expand(G, heads, R, T1))
    if T2:
        parts.append(kc2.repeat_interleave(gd, 0))
    kc = torch.cat(parts, -1)

    t_idx, r_idx = torch.arange(T), torch.arange(R)
    mask = None
    live = torch.ones(G, heads, R, T, dtype=torch.bool)
    if c["mask"]:
        mask = key_mask(c, kc, gfull)
        live &= (mask == 0)[:, None, None, :]
    if c["causal"]:
        live &= (t_idx[None, :] <= r_idx[:, None])[None, None]
    bias = None
    if c["bias"]:
        # one knock-out per (bias group, head, row): the first key of the code the row will look at first, if two keys carry it
        bias = torch.zeros(G // gd, heads, R, T, dtype=torch.float64)
        for g2 in range(G // gd):
            for h in range(heads):
                for r in range(R):
                    want = (r + g2 * heads + h) % ncodes
                    hit = ((kc[g2 * gd, h, r] == want) & live[g2 * gd, h, r]).nonzero().flatten()
                    if len(hit) == 2:
                        bias[g2, h, r, hit[(r + h) % 2]] = KNOCK
        live &= (bias == 0).repeat_interleave(gd, 0)

    n = torch.stack([(live & (kc == code)).sum(-1) for code in range(ncodes)], -1)       # [G,heads,R,ncodes]
    ok = (n == 1) | (n == 2) | (n == 4)
    qc = torch.zeros(G, heads, R, dtype=torch.int64)
    for g in range(G):
        for h in range(heads):
            for r in range(R):
                if g == gfull:
                    continue
                first = r + (g // gd) * heads + h
                pick = [code % ncodes for code in range(first, first + ncodes) if ok[g, h, r, code % ncodes]]
                assert pick, f"{c['id']}: no code with 1, 2 or 4 live keys for row {(g, h, r)}"
                qc[g, h, r] = pick[0]
    sel = live & (kc == qc[..., None])
    if gfull is not None:
        sel[gfull] = True

    qh = torch.zeros(G, R, heads, d, dtype=torch.float64)
    qh[..., :dc] = -B
    qh[..., :dc].scatter_(-1, qc.permute(0, 2, 1)[..., None], 0.0)
    qh[..., dc:dc + nq] = GR.dyadic((G, R, heads, nq), seed + 5, 1)
    q = qh.reshape(G, R, HD)

    col, keep = torch.arange(d), max(1, d // 8)
    sparse = ((col[None, :] - r_idx[:, None]) % keep == 0).double()                      # [R,d]: the non-zero columns of dout
    dout = GR.dyadic((G, R, heads, d), seed + 6)
    dout[dout == 0] = 1.0                                                                # +-1 on the kept columns
    dout = (dout * sparse[None, :, None, :]).reshape(G, R, HD)
    if gfull is not None:
        # columns of v that sum to 0, +-T/2 or +-T/4 over the keys of the fully masked group: entries +-1, (T + sum) / 2 of them +1
        assert T2 == 0
        g1 = gfull // kv
        for j in range(HD):
            s = (0, T // 2, -(T // 2), T // 4, -(T // 4))[j % 5] if T >= 4 else 0
            colv = -torch.ones(T, dtype=torch.float64)
            colv[torch.tensor(_perm(T, seed + 7000 + j)[:(T + s) // 2], dtype=torch.int64)] = 1.0
            v1[g1, :, j] = colv
    return dict(q=q, k1=k1, v1=v1, k2=k2, v2=v2, mask=mask, bias=bias, dout=dout, kc=kc, qc=qc, live=live, sel=sel,
                count=sel.sum(-1), gfull=gfull, ncodes=ncodes)


# ---- the float64 reference ------------------------------------------------------------------------------------------------------
def _scores(c, o):
    """the scores the reference softmax sees, [G,heads,R,T] float64 (for the logsumexp)"""
    G, R, heads, d, gd, kv = (c[k] for k in ("G", "R", "heads", "d", "gd", "kv"))
    qh = o["q"].view(G, R, heads, d).permute(0, 2, 1, 3)
    s = []
    if o["k1"] is not None:
        s.append(qh @ o["k1"].repeat_interleave(kv, 0).view(G, -1, heads, d).permute(0, 2, 3, 1))
    if o["k2"] is not None:
        s.append(torch.einsum("ghrd,grthd->ghrt", qh, o["k2"].repeat_interleave(gd, 0).view(G, R, -1, heads, d)))
    s = torch.cat(s, -1) * c["scale"]
    T = s.shape[-1]
    if o["mask"] is not None:
        s = s + o["mask"][:, None, None, :]
    if o["bias"] is not None:
        s = s + o["bias"].repeat_interleave(gd, 0)
    if c["causal"]:
        s = torch.where(torch.arange(T)[None, :] > torch.arange(R)[:, None], torch.full_like(s, -1e4), s)
    return s


def raw(c, o):
    """attn_ref.attention_ref in float64 on `o` (p = 0) and autograd against `dout`, as they come -> out, P, lse, gradients"""
    G, R, heads, d, gd, kv = (c[k] for k in ("G", "R", "heads", "d", "gd", "kv"))
    leaf = lambda t: None if t is None else t.clone().requires_grad_(True)
    q, k1, v1, k2, v2, bias = (leaf(o[n]) for n in ("q", "k1", "v1", "k2", "v2", "bias"))
    wide = lambda t: None if t is None else t.repeat_interleave(kv, 0)
    out, P, _ = attention_ref(q, wide(k1), wide(v1), k2, v2, o["mask"], bias, heads, gd, c["scale"], c["causal"])
    (out * o["dout"]).sum().backward()
    g = lambda t: None if t is None else t.grad
    return dict(out=out.detach(), P=P.detach(), lse=torch.logsumexp(_scores(c, o), -1), dq=g(q), dk1=g(k1), dv1=g(v1),
                dk2=g(k2), dv2=g(v2), dbias=g(bias))


def reference(c, o):
    """attn_ref.attention_ref in float64 on the operands `o` (p = 0), autograd for the gradients against `dout`, and the
    magnitudes -> dict: out, P, lse, dq, dk1, dv1, dk2, dv2, dbias (None where the case has none; dk1 / dv1 summed over the kv
    sharers, dk2 / dv2 / dbias over the group_div groups) and mag[name] for out and each gradient"""
    ref = raw(c, o)
    # float64 does not flush exp(-128) = 2.6e-56 as float32 does: where float32 arithmetic gives an exact 0, attention_ref leaves
    # 1e-56.  Snap to the written-out sums over P = sel / count (what the preconditions promise), after holding them against autograd.
    P = o["sel"].double() / o["sel"].sum(-1, keepdim=True).double()
    ex = explicit(c, o, P, False)
    assert float((ref["P"] - P).abs().max()) < 1e-50
    for name in ("out", "dq", "dk1", "dv1", "dk2", "dv2", "dbias"):
        assert (ref[name] is None) == (ex[name] is None), name
        if ref[name] is not None:
            assert float((ref[name] - ex[name]).abs().max()) < 1e-45, name
            ref[name] = ex[name]
    ref["P"] = P
    ref["mag"] = magnitudes(c, o, P)
    return ref


def heads_first(x, heads):
    return x.reshape(x.shape[:-1] + (heads, x.shape[-1] // heads)).movedim(-2, 1)


def explicit(c, o, P, absolute, sum_gd=True):
    """the forward and backward sums written out, float64: with absolute the sums of the absolute values of their terms (the
    magnitudes), without it the values themselves (test_attn_exact_cpu.py holds them against autograd) -> dict like reference's,
    plus dS.  sum_gd=False: dk2 / dv2 / dbias per group [G, ...], as fcmf_attn_small_bwd writes them"""
    G, R, heads, d, gd, kv = (c[k] for k in ("G", "R", "heads", "d", "gd", "kv"))
    T1 = 0 if o["k1"] is None else o["k1"].shape[1]
    HD = heads * d
    a = (lambda t: t.abs()) if absolute else (lambda t: t)
    hf = lambda t: t.view(G, -1, heads, d).permute(0, 2, 1, 3)                       # [G,n,HD] -> [G,heads,n,d]
    back = lambda t: t.permute(0, 2, 1, 3).reshape(G, -1, HD)
    share = lambda t, n: t.reshape((G // n, n) + t.shape[1:]).sum(1)
    share_gd = (lambda t: share(t, gd)) if sum_gd else (lambda t: t)
    qh, doh = hf(o["q"]), hf(o["dout"])
    dP = []
    if T1:
        k1h, v1h = hf(o["k1"].repeat_interleave(kv, 0)), hf(o["v1"].repeat_interleave(kv, 0))
        dP.append(doh @ v1h.transpose(-1, -2))
    if o["k2"] is not None:
        k2h, v2h = (t.repeat_interleave(gd, 0).view(G, R, -1, heads, d) for t in (o["k2"], o["v2"]))      # [G,R,T2,heads,d]
        dP.append(torch.einsum("ghrd,grthd->ghrt", doh, v2h))
    dP = torch.cat(dP, -1)
    dS = P * (dP - (P * dP).sum(-1, keepdim=True))
    P1, P2, S1, S2 = P[..., :T1], P[..., T1:], a(dS[..., :T1]), a(dS[..., T1:])
    res = dict(out=0, dq=0, dk1=None, dv1=None, dk2=None, dv2=None, dbias=None, dS=dS)
    if T1:
        res["out"] = res["out"] + P1 @ a(v1h)
        res["dq"] = res["dq"] + c["scale"] * (S1 @ a(k1h))
        res["dk1"] = share(back(c["scale"] * (S1.transpose(-1, -2) @ a(qh))), kv)
        res["dv1"] = share(back(P1.transpose(-1, -2) @ a(doh)), kv)
    if o["k2"] is not None:
        res["out"] = res["out"] + torch.einsum("ghrt,grthd->ghrd", P2, a(v2h))
        res["dq"] = res["dq"] + c["scale"] * torch.einsum("ghrt,grthd->ghrd", S2, a(k2h))
        res["dk2"] = share_gd(c["scale"] * torch.einsum("ghrt,ghrd->grthd", S2, a(qh)).reshape(G, R, -1, HD))
        res["dv2"] = share_gd(torch.einsum("ghrt,ghrd->grthd", P2, a(doh)).reshape(G, R, -1, HD))
    res["out"], res["dq"] = back(res["out"]), back(res["dq"])
    if o["bias"] is not None:
        res["dbias"] = share_gd(a(dS))
    return res


def magnitudes(c, o, P):
    m = explicit(c, o, P, True)
    return {k: v for k, v in m.items() if k != "dS" and v is not None}


def ds_grid_ok(c, o, P):
    """every dS is n * 2^-s with |n| <= 256 for some s: a bf16 operand of an MFMA holds it exactly"""
    dS = explicit(c, o, P, False)["dS"]
    return bool((dS.bfloat16().double() == dS).all())


def representable(t, dtype):
    return bool((t.to(dtype).double() == t).all())


# ---- the bound ------------------------------------------------------------------------------------------------------------------
def u_of(c, name):
    """relative term of the bound for output `name` of a case: 2^-9 per bf16 rounding on the value's path, times the number
    of roundings, times 2; 2^-22 for float32 outputs (dbias always).  One rounding everywhere except the VALU dq, which is
    rounded once per 128-key partial and once more by the sum of the partials (a single partial is returned as it is)."""
    if c["dtype"] == "f32" or name == "dbias":
        return 2.0 ** -22
    nch = max(1, (c["T1"] + 127) // 128)
    roundings = nch + 1 if name == "dq" and c["kind"] == "valu" and nch > 1 else 1
    return 2.0 ** -9 * roundings * 2


def bound(ref, mag, u, eps):
    return u * ref.abs() + eps * mag
