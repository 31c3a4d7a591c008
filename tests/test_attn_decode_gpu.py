"""fcmf_attn_decode (csrc/attn_decode.hip) through ops.decode_attention against float64 torch on random operands: the single-query
attention with indexed keys of the IAOG prefix decode.  Tolerances are those of test_ops_gpu.test_attention_fwd_bwd for
fcmf_attn_small_fwd at the same dtype (relative to the reference's largest entry).  Every case reads its query from the wide
[kx | qx] buffer, reads the cache through an ancestor table in which rows share parents and row order is permuted, keeps NaN
wherever the kernel must not read, and checks the append bit for bit."""
import math

import pytest
import torch

from helpers import rel_err

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 3e-5, torch.bfloat16: 3e-2}


def _ref(q, K, live, scale, heads, exclude=False):
    """float64: q [n, HD], K [n, T, HD] (the keys every row sees, gathered) -> out [n, HD]; scores of positions >= live are -1e4
    (exclude: those keys are left out instead -- what the kernel must NOT compute)"""
    n, T, HD = K.shape
    d = HD // heads
    q4, K4 = q.double().view(n, heads, d), K.double().view(n, T, heads, d)
    s = torch.einsum("nhd,nthd->nht", q4, K4) * scale
    if exclude:
        s, K4 = s[:, :, :live], K4[:, :live]
    else:
        s[:, :, live:] = -1e4
    return torch.einsum("nht,nthd->nhd", torch.softmax(s, dim=-1), K4).reshape(n, HD)


def _bits(x):
    return x.view(torch.int32 if x.dtype == torch.float32 else torch.int16)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("t", [0, 1, 19])
@pytest.mark.parametrize("n", [1, 5, 13])
@pytest.mark.parametrize("heads", [4, 12])
@pytest.mark.parametrize("d", [16, 64])
def test_cache_form_with_append(dev, d, heads, n, t, dtype):
    from fcmf_framework import ops
    HD, Tmax, Rmax = heads * d, t + 3, n + 2
    g = torch.Generator().manual_seed(1000 * d + 100 * heads + 10 * n + t)
    kq = (torch.randn(n, 2 * HD, generator=g) * 0.7).to(dtype)                 # [kx | qx]: the query's row stride is 2 HD
    hist = (torch.randn(Tmax, Rmax, HD, generator=g) * 0.7).to(dtype)
    # ancestors: any row of an earlier round, drawn with replacement (rows share parents) and unrelated to the row's own index
    anc = torch.randint(0, n, (n, t), generator=g)
    if n > 1 and t > 0:
        anc[1, :] = anc[0, :]                                                  # two rows with the same parent at every position
    cache = hist.clone()
    cache[t:] = float("nan")                                                   # the round's own position and everything after it
    cache[:, n:] = float("nan")                                                # rows no ancestor names
    cache, kq_d, anc_d = cache.to(dev), kq.to(dev), anc.to(dev)
    snap = cache.clone()
    out = ops.decode_attention(kq_d[:, HD:], cache, anc_d, heads, t + 1, t + 1, k_new=kq_d[:, :HD], append_at=t)
    torch.cuda.synchronize()
    assert out.shape == (n, HD) and out.dtype == dtype and torch.isfinite(out.float()).all()      # no NaN was read

    K = torch.empty(n, t + 1, HD, dtype=torch.float64)
    for r in range(n):
        for p in range(t):
            K[r, p] = hist[p, anc[r, p]].double()
        K[r, t] = kq[r, :HD].double()
    ref = _ref(kq[:, HD:], K, t + 1, 1 / math.sqrt(d), heads)
    err = rel_err(out, ref)
    print(f"d {d} heads {heads} n {n} t {t} {dtype}: rel err {err:.3e}")
    assert err < TOL[dtype]

    # the append: cache[t, r] = k_new[r] bit for bit, nothing else touched
    assert torch.equal(_bits(cache[t, :n]), _bits(kq_d[:, :HD].contiguous()))
    snap[t, :n] = kq_d[:, :HD]
    assert torch.equal(_bits(cache), _bits(snap))
    # a second launch over the now filled position gives the same bits (fixed-order reductions)
    again = ops.decode_attention(kq_d[:, HD:], cache, anc_d, heads, t + 1, t + 1, k_new=kq_d[:, :HD], append_at=t)
    assert torch.equal(_bits(again), _bits(out))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("t", [1, 4, 7], ids=["live<Tk", "live=Tk", "t>=Tk"])
@pytest.mark.parametrize("n", [1, 5, 13])
def test_cross_form_reads_the_samples_keys_in_place(dev, n, t, dtype):
    """hoisted encoder keys [samples, Tk, HD] read through the sample index (idx_sp = 0), live = min(t + 1, Tk) of Tk = 5 keys"""
    from fcmf_framework import ops
    heads, d, Tk, Bs = 4, 16, 5, 3
    HD, live = heads * d, min(t + 1, 5)
    g = torch.Generator().manual_seed(77 + 10 * n + t)
    q = (torch.randn(n, HD, generator=g) * 0.7).to(dtype)
    keys = (torch.randn(Bs + 1, Tk + 2, HD, generator=g) * 0.7).to(dtype)
    keys[Bs:] = float("nan")                                                   # a sample no row names
    keys[:, Tk:] = float("nan")                                                # positions beyond T
    sample = torch.randint(0, Bs, (n,), generator=g)
    keys_d = keys.to(dev)
    snap = keys_d.clone()
    out = ops.decode_attention(q.to(dev), keys_d, sample.to(dev), heads, Tk, live, pos_dim=1)
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all() and torch.equal(_bits(keys_d), _bits(snap))
    ref = _ref(q, keys[sample, :Tk], live, 1 / math.sqrt(d), heads)
    err = rel_err(out, ref)
    print(f"cross n {n} t {t} live {live} {dtype}: rel err {err:.3e}")
    assert err < TOL[dtype]


def test_masked_keys_are_filled_not_excluded(dev):
    """all live scores near -1e4, so the keys filled with exactly -1e4 carry weight: excluding them gives another answer.  The
    operands are dyadic (multiples of 1/4; component 0 of every head is 1 in every key and -4e4 in q), so scale * <q, k> =
    -1e4 + delta is exact in float32 in any summation order and float64 sees the same scores."""
    from fcmf_framework import ops
    heads, d, Tk, Bs, n, live = 4, 16, 5, 3, 5, 2
    HD = heads * d
    g = torch.Generator().manual_seed(5)
    q = torch.randint(-8, 9, (n, HD), generator=g).float() / 4
    keys = torch.randint(-4, 5, (Bs, Tk, HD), generator=g).float() / 4
    q[:, ::d] = -4e4
    keys[:, :, ::d] = 1.0
    sample = torch.randint(0, Bs, (n,), generator=g)
    K = keys[sample]
    fill = _ref(q, K, live, 0.25, heads)
    excl = _ref(q, K, live, 0.25, heads, exclude=True)
    s = torch.einsum("nhd,nthd->nht", q.double().view(n, heads, d), K.double().view(n, Tk, heads, d))[:, :, :live] * 0.25
    assert (s + 1e4).abs().max() < 8                                            # the live scores ARE near -1e4
    gap = rel_err(excl, fill)
    print(f"float64 exclude vs fill: rel {gap:.3e}")
    assert gap > 10 * TOL[torch.float32]                                        # the test discriminates
    out = ops.decode_attention(q.to(dev), keys.to(dev), sample.to(dev), heads, Tk, live, pos_dim=1)
    err = rel_err(out, fill)
    print(f"kernel vs fill: rel {err:.3e}")
    assert err < TOL[torch.float32]


def test_limits_and_bad_indices(dev):
    from fcmf_framework import _hip as H, ops
    heads, n = 2, 3
    for d, T, want in ((12, 4, H.ERR_UNSUPPORTED), (136, 4, H.ERR_UNSUPPORTED), (16, 513, H.ERR_UNSUPPORTED), (16, 0, H.ERR_UNSUPPORTED)):
        HD = heads * d
        q = torch.zeros(n, HD, device=dev)
        keys = torch.zeros(max(T, 1), n, HD, device=dev)
        idx = torch.zeros(n, max(T, 1), dtype=torch.int64, device=dev)
        out = torch.empty_like(q)
        rc = H.lib().fcmf_attn_decode(H.ptr(q), HD, H.ptr(keys), keys.stride(0), keys.stride(1), H.ptr(idx), idx.stride(0), 1, n, None, 0, 0,
                                      H.ptr(out), HD, n, heads, d, T, T, 0.25, H.F32, H.stream())
        assert rc == want, (d, T, rc)
    d, T = 16, 4
    HD = heads * d
    q = torch.randn(n, HD, device=dev)
    keys = torch.randn(T, n, HD, device=dev)
    with pytest.raises(H.HipLibraryError):                                     # more keys than the cache has positions
        ops.decode_attention(q, keys, torch.zeros(n, T + 1, dtype=torch.int64, device=dev), heads, T + 1, T + 1)
    with pytest.raises(H.HipLibraryError):                                     # a misaligned query view
        ops.decode_attention(torch.randn(n, HD + 1, device=dev)[:, 1:], keys, torch.zeros(n, T, dtype=torch.int64, device=dev), heads, T, T)
    # an index outside the cache's rows reads nothing: that row is NaN, the others are what they were
    idx = torch.zeros(n, T, dtype=torch.int64, device=dev)
    good = ops.decode_attention(q, keys, idx, heads, T, T)
    idx[1, 2] = n
    idx[2, 0] = -1
    out = ops.decode_attention(q, keys, idx, heads, T, T)
    assert torch.equal(out[0], good[0]) and torch.isnan(out[1:]).all()
