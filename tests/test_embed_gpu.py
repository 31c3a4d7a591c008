"""RoBERTa embedding kernels (csrc/norm.hip): fcmf_position_ids across its 64-token chunks, ops.embed_layer_norm forward and
backward against float64 autograd at the pass counts, layouts and with the dropout that the other tests leave out, and the fused
position + type gradient kernel across sequence groups and slots.  Bounds: the 2e-5 / 3e-2 rel_err of test_embedding_layer_norm
(the table gradients sum through float atomics: no bit-equality between runs is asserted)."""
import contextlib

import pytest
import torch
import torch.nn.functional as F

import rowwise_ref as R
from helpers import _CallRecorder, rel_err

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16


def _ops():
    from fcmf_framework import ops, _hip
    return ops, _hip


def _randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


@contextlib.contextmanager
def _recording():
    """the library's entry points recorded as (name, scalars, return code) inside the block"""
    _, H = _ops()
    real = H.lib()
    H._lib = rec = _CallRecorder(real, H.SIGNATURES)
    try:
        yield rec
    finally:
        H._lib = real


# ---- position ids -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [1, 0])
@pytest.mark.parametrize("S", [63, 64, 65, 128, 170, 200])
def test_position_ids_across_64_token_chunks(dev, S, pad):
    """one wave per sequence walks 64-token chunks with a running count; lane 63 takes the whole ballot"""
    _, H = _ops()
    ids = torch.randint(2, 50, (8, S), generator=torch.Generator().manual_seed(S))
    ids[1, 0] = pad                                # a leading pad
    for row, t in ((2, 63), (3, 64)):              # an interior pad on either side of the first chunk boundary
        if t < S - 1:
            ids[row, t] = pad
    for row, t in ((4, 62), (5, 64), (6, 129)):    # trailing pads
        if t < S:
            ids[row, t:] = pad
    ids[7] = pad                                   # nothing but pads
    m = ids.ne(pad).long()
    ref = torch.cumsum(m, 1) * m + pad
    idd = ids.to(dev)
    out = R.guarded((8, S), torch.int64, dev)
    assert H.lib().fcmf_position_ids(H.ptr(idd), H.ptr(out.view), 8, S, pad, H.stream()) == 0
    torch.cuda.synchronize()
    out.check()
    assert torch.equal(out.view.cpu(), ref)


# ---- embedding + LayerNorm (+ dropout) ----------------------------------------------------------------------------------------
def _tables(V, Pn, H_, dev):
    shapes = ((V, H_), (Pn, H_), (2, H_))
    word, ptab, ttab = (_randn(s, i).to(dev).requires_grad_(True) for i, s in enumerate(shapes))
    g = (1 + 0.1 * _randn((H_,), 7)).to(dev).requires_grad_(True)
    b = _randn((H_,), 8).to(dev).requires_grad_(True)
    return word, ptab, ttab, g, b


def _reference(ids, pos, tt, params, w, pad, mask, p):
    """float64 autograd of sum(w * dropout(LN(word[ids] + type[tt] + pos[pos]))) -> y, the five gradients"""
    wr, pr, tr, gr, br = (t.detach().double().cpu().requires_grad_(True) for t in params)
    e = F.embedding(ids, wr, padding_idx=pad) + tr[tt] + F.embedding(pos, pr, padding_idx=pad)
    u = e.mean(-1, keepdim=True)
    s = (e - u).pow(2).mean(-1, keepdim=True)
    y = gr * ((e - u) / torch.sqrt(s + 1e-5)) + br
    if mask is not None:
        y = y * mask.view(y.shape) * R.inv_keep(p)
    (y * w.double()).sum().backward()
    return y.detach(), [t.grad for t in (wr, pr, tr, gr, br)]


def _run(dev, dtype, ids, tt, H_, pad, p, V=50, Pn=24):
    """ops.embed_layer_norm forward + backward on `ids` ([B, S] or [B, A, S]) against the reference; returns the recorded calls"""
    ops, H = _ops()
    S = ids.shape[-1]
    params = _tables(V, Pn, H_, dev)
    idd = ids.to(dev)
    ttd = None if tt is None else tt.to(dev)
    pos = ops.position_ids(idd.view(-1, S), pad).view(ids.shape)
    m2 = ids.ne(pad).long()
    pos_ref = torch.cumsum(m2, -1) * m2 + pad
    assert torch.equal(pos.cpu(), pos_ref)
    mask = None
    if p > 0:
        ops.manual_seed(2024)
    y = ops.embed_layer_norm(idd, pos, ttd, *params, 1e-5, p, p > 0, pad, dtype)
    if p > 0:
        ops.manual_seed(2024)
        assert ops.next_seed() == R.EMBED_SEED                  # the seed the op drew
        mask = R.mask_tensor(R.EMBED_SEED, (ids.numel(), H_), p)
    assert y.dtype == dtype and y.shape == (*ids.shape, H_)
    w = _randn(y.shape, 9).to(dtype).float()                    # (representable in the output type: dy arrives in it)
    with _recording() as rec:
        (y.float() * w.to(dev)).sum().backward()
        torch.cuda.synchronize()
    yr, grads = _reference(ids, pos_ref, torch.zeros_like(ids) if tt is None else tt, params, w, pad, mask, p)
    tol = 2e-5 if dtype == F32 else 3e-2
    assert rel_err(y, yr) < tol
    if mask is not None:
        assert torch.equal(y.detach().cpu().view(-1, H_) != 0, mask.bool() & (yr.view(-1, H_) != 0))
    for name, a, r in zip(("word", "pos", "type", "gamma", "beta"), params, grads):
        assert torch.isfinite(a.grad).all()
        assert rel_err(a.grad, r) < tol * 2, name
    return rec.calls


def _batch(shape, pad, seed=1):
    ids = torch.randint(3, 50, shape, generator=torch.Generator().manual_seed(seed))
    flat = ids.view(-1, shape[-1])
    flat[0, 3:] = pad          # trailing pads
    flat[1, 0] = pad           # a leading pad
    flat[2, 2] = pad           # an interior pad
    tt = torch.zeros_like(ids)
    tt.view(-1, shape[-1])[1] = 1
    tt.view(-1, shape[-1])[2, 3:] = 1
    return ids, tt


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("layout", ["2d", "2d_no_types", "3d"])
@pytest.mark.parametrize("H_", [260, 2048])
def test_embed_layer_norm_pass_counts_layouts_and_dropout(dev, dtype, H_, layout, p):
    """H 260 / 2048: NP 2 and 8.  [B, A, S] ids take the per-token scatter for the position table as well (fcmf_embed_bwd with
    dpos).  p = 0.1 in training mode: y = LN(e) * m / (1 - p) with m from the numpy mask, and every table gradient is that of
    the masked function (fcmf_dropout on dy, then the LayerNorm backward)."""
    pad = 1
    ids, tt = _batch((3, 5) if layout != "3d" else (3, 2, 5), pad)
    calls = _run(dev, dtype, ids, None if layout == "2d_no_types" else tt, H_, pad, p)
    names = [c[0] for c in calls]
    assert ("fcmf_dropout" in names) == (p > 0)
    if layout == "3d":
        assert "fcmf_embed_pos_type_bwd" not in names and "fcmf_embed_pos_bwd" not in names
    else:
        fused = [c for c in calls if c[0] == "fcmf_embed_pos_type_bwd"]
        assert len(fused) == 1
        assert ("fcmf_embed_pos_bwd" in names) == (fused[0][2] != 0)       # the documented fallback when the fused kernel declines


@pytest.mark.parametrize("dtype,H_", [(BF16, 64), (F32, 768), (F32, 64), (BF16, 768)])
def test_fused_position_and_type_gradient_across_groups_and_slots(dev, dtype, H_):
    """130 sequences = three 64-sequence groups (the last with 2); H 64 in bf16: 32 slots per workgroup, H 768 in float32: 1.
    Every other sequence starts with a pad, so the slots of one workgroup see different first position ids: slots with equal
    ids are merged, the rest fall back to per-token atomics.  Both type ids occur."""
    pad, nseq, S = 1, 130, 7
    ids = torch.randint(3, 50, (nseq, S), generator=torch.Generator().manual_seed(4))
    ids[::2, 0] = pad
    ids[5, 4:] = pad
    ids[129, 2] = pad
    tt = torch.randint(0, 2, (nseq, S), generator=torch.Generator().manual_seed(5))
    calls = _run(dev, dtype, ids, tt, H_, pad, 0.0)
    fused = [c for c in calls if c[0] == "fcmf_embed_pos_type_bwd"]
    assert len(fused) == 1 and fused[0][2] == 0                            # the fused kernel ran
    assert "fcmf_embed_pos_bwd" not in [c[0] for c in calls]
