"""Attention probabilities on request (csrc/attn_probs.hip): fcmf_attn_probs (VALU, f32 / bf16) and fcmf_attn_mfma_probs (bf16 MFMA)
against a float64 softmax of the SAME stored inputs, written here from the score formula of include/fcmf_hip.h:
    score = scale * <q, k> + mask[g, t] + bias[g / group_div, h, r, t];   causal: score = -1e4 where t > r;
    head_quirk: output slot h of group g reads head (h * G + g) % heads.
Tolerance: after the load the kernels keep everything in f32, so both dtypes are held to the project's fp32 attention tolerance
(rel_err < 3e-5, test_ops_gpu.test_attention_fwd_bwd); row sums within 1e-4 of 1 (f32 exp and a sum of at most 512 terms).
Every comparison prints its figure before it asserts."""
import math
import os

import numpy as np
import pytest
import torch

from conftest import GOLD
from helpers import mfma_attention, rel_err

pytestmark = pytest.mark.gpu

TOL = 3e-5
FMIN = torch.finfo(torch.float32).min


def _rand(shape, dev, dtype=torch.float32, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype).to(dev)


def _probs_ref(q, k1=None, k2=None, mask=None, bias=None, heads=1, group_div=1, scale=None, causal=False, head_quirk=False):
    """float64 [G, heads, R, T1+T2] from the header's score definition; inputs are the stored (f32 / bf16) values"""
    c = lambda t: None if t is None else t.detach().double().cpu()
    q, k1, k2, mask, bias = c(q), c(k1), c(k2), c(mask), c(bias)
    G, R, HD = q.shape
    d = HD // heads
    scale = 1.0 / math.sqrt(d) if scale is None else scale
    g_idx = torch.arange(G)
    hin = (torch.arange(heads)[None, :] * G + g_idx[:, None]) % heads if head_quirk else torch.arange(heads)[None, :].expand(G, heads)
    pick = lambda x: torch.gather(x, -2, hin.reshape((G,) + (1,) * (x.dim() - 3) + (heads, 1)).expand(x.shape[:-2] + (heads, d)))
    qh = pick(q.reshape(G, R, heads, d))                                         # [G, R, slot, d]
    parts = []
    if k1 is not None:
        parts.append(torch.einsum("grhd,gthd->ghrt", qh, pick(k1.reshape(G, -1, heads, d))))
    if k2 is not None:
        k2g = k2[g_idx // group_div]                                             # [G, R, T2, HD]
        parts.append(torch.einsum("grhd,grthd->ghrt", qh, pick(k2g.reshape(G, R, -1, heads, d))))
    s = torch.cat(parts, -1) * scale
    if mask is not None:
        s = s + mask[:, None, None, :]
    if bias is not None:
        s = s + bias[g_idx // group_div]
    if causal:
        T = s.shape[-1]
        s = torch.where(torch.arange(T)[None, :] > torch.arange(R)[:, None], torch.full_like(s, -1e4), s)
    return torch.softmax(s, -1)


def _check(name, got, ref, tol=TOL):
    err = rel_err(got, ref)
    rows = (got.double().sum(-1) - 1).abs().max().item()
    print(f"{name}: rel_err {err:.3e}  max |row sum - 1| {rows:.3e}")
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(ref.shape), name
    assert err < tol, name
    assert rows < 1e-4, name


def _inputs(case, dev, dtype, mask_value=-10000.0):
    G, R, heads, d, T1, T2, gd, use_mask, use_bias, causal = case
    HD, T = heads * d, T1 + T2
    q = _rand((G, R, HD), dev, dtype, 0.7, seed=1)
    k1 = _rand((G, T1, HD), dev, dtype, 0.7, seed=2) if T1 else None
    k2 = _rand((G // gd, R, T2, HD), dev, dtype, 0.7, seed=4) if T2 else None
    mask = None
    if use_mask:
        m01 = (torch.rand(G, T, generator=torch.Generator().manual_seed(7)) > 0.2).float()
        m01[:, 0] = 1
        mask = ((1 - m01) * mask_value).to(dev)
    bias = _rand((G // gd, heads, R, T), dev, seed=8) if use_bias else None
    return q, k1, k2, mask, bias


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. descriptor kernel
DESC_CASES = [
    # G, R, heads, d, T1, T2, group_div, mask, bias, causal   (from test_ops_gpu.ATTN_CASES: one per branch of the kernel)
    (3, 20, 4, 16, 20, 0, 1, True, False, False),
    (4, 3, 2, 16, 10, 7, 2, True, False, False),
    (4, 3, 2, 16, 0, 9, 2, True, False, False),
    (2, 9, 8, 12, 9, 0, 1, False, True, False),
    (2, 5, 4, 16, 170, 0, 1, True, False, False),
    (3, 6, 4, 16, 6, 0, 1, False, False, True),
    (2, 40, 3, 20, 33, 5, 2, True, True, False),
    (1, 150, 2, 64, 130, 20, 1, True, False, False),
]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", DESC_CASES)
def test_desc_kernel_matches_float64(dev, dtype, case):
    from fcmf_framework import ops
    G, R, heads, d, T1, T2, gd, _, _, causal = case
    q, k1, k2, mask, bias = _inputs(case, dev, dtype)
    with mfma_attention(False):            # (1, 150, 2, 64, ...) has private keys, so no case is MFMA-eligible anyway
        got = ops.attention_probs(q, k1=k1, k2=k2, mask=mask, bias=bias, heads=heads, group_div=gd, causal=causal)
    assert not got.requires_grad
    _check(f"desc {case} {dtype}", got.cpu(), _probs_ref(q, k1, k2, mask, bias, heads, gd, None, causal))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_desc_kernel_query_row_stride_zero(dev, dtype):
    """one query row per group expanded over R rows (the [CLS] query against each image's private keys) is read in place"""
    from fcmf_framework import ops
    G, R, heads, d, T1, T2, gd = 6, 7, 3, 16, 11, 9, 3
    HD = heads * d
    q = _rand((G, HD), dev, dtype, 0.7, seed=1).unsqueeze(1).expand(G, R, HD)
    assert q.stride(1) == 0
    k1 = _rand((G, T1, HD), dev, dtype, 0.7, seed=2)
    k2 = _rand((G // gd, R, T2, HD), dev, dtype, 0.7, seed=3)
    got = ops.attention_probs(q, k1=k1, k2=k2, heads=heads, group_div=gd)
    _check(f"stride-0 query {dtype}", got.cpu(), _probs_ref(q, k1, k2, heads=heads, group_div=gd))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_desc_kernel_reads_column_slices_of_a_wider_buffer(dev, dtype):
    """q and k as column slices of one [G, T, 2*HD + 8] buffer (row strides larger than the head block, k not at offset 0)"""
    from fcmf_framework import ops
    G, T, heads, d = 3, 21, 4, 16
    HD = heads * d
    buf = _rand((G, T, 2 * HD + 8), dev, dtype, 0.7, seed=5)
    k, q = buf[:, :, :HD], buf[:, :, HD + 8:]
    assert not q.is_contiguous() and q.stride(1) == 2 * HD + 8
    got = ops.attention_probs(q, k1=k, heads=heads, causal=True)
    _check(f"column slices {dtype}", got.cpu(), _probs_ref(q, k, heads=heads, causal=True))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("slot_major", [False, True])
@pytest.mark.parametrize("G", [2, 3])
def test_desc_kernel_head_quirk_both_layouts(dev, dtype, G, slot_major):
    """slot h of group g reads head (h*G + g) % 4: G = 2 shares a factor with the 4 heads, G = 3 is coprime to it"""
    from fcmf_framework import ops
    heads, d, R, T = 4, 8, 5, 7
    q = _rand((G, R, heads * d), dev, dtype, 1.2, seed=1)
    k = _rand((G, T, heads * d), dev, dtype, 1.2, seed=2)
    got = ops.attention_probs(q, k1=k, heads=heads, causal=True, head_quirk=True, slot_major=slot_major)
    ref = _probs_ref(q, k, heads=heads, causal=True, head_quirk=True)
    plain = _probs_ref(q, k, heads=heads, causal=True)
    assert rel_err(plain, ref) > 1e-2          # the quirk changes the answer at these sizes
    if slot_major:
        ref = ref.transpose(0, 1).reshape(heads * G, R, T)      # index h*G + g
    _check(f"head_quirk G={G} slot_major={slot_major} {dtype}", got.cpu(), ref)


def test_desc_kernel_limits_are_unsupported(dev):
    from fcmf_framework import ops, _hip as H
    q, k = _rand((1, 2, 16), dev), _rand((1, 513, 16), dev)
    with pytest.raises(H.HipLibraryError, match="unsupported"):
        ops.attention_probs(q, k1=k, heads=1)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. MFMA kernel
MFMA_SHAPES = [(128, 128), (33, 17), (77, 128), (130, 129), (256, 150), (200, 256)]


def _padding_mask(G, Tk, dev, seed):
    """finfo.min on a random number of trailing keys of every sequence (at least one live key)"""
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(1, Tk + 1, (G,), generator=g)
    lens[0] = Tk
    m01 = (torch.arange(Tk)[None, :] < lens[:, None]).float()
    return ((1 - m01) * FMIN).to(dev), lens


def _guarded(shape, dev, margin=1024, sentinel=-777.0):
    """a float32 tensor of `shape` in the middle of a sentinel-filled allocation -> (tensor, check())"""
    n = math.prod(shape)
    raw = torch.full((n + 2 * margin,), sentinel, dtype=torch.float32, device=dev)
    out = raw[margin:margin + n].view(shape)

    def untouched():
        return bool((raw[:margin] == sentinel).all() and (raw[margin + n:] == sentinel).all())
    return out, untouched


@pytest.mark.parametrize("Tq,Tk", MFMA_SHAPES)
def test_mfma_kernel_matches_float64_and_desc_kernel(dev, Tq, Tk):
    from fcmf_framework import ops, _hip as H
    G, heads, d = 3, 2, 64
    HD = heads * d
    q = _rand((G, Tq, HD), dev, torch.bfloat16, 0.8, seed=1)
    k = _rand((G, Tk, HD), dev, torch.bfloat16, 0.8, seed=2)
    mask, lens = _padding_mask(G, Tk, dev, seed=Tq + Tk)
    ref = _probs_ref(q, k, mask=mask, heads=heads)
    # dense q / k through the op, output inside a sentinel margin
    out, untouched = _guarded((G, heads, Tq, Tk), dev)
    got = ops.attention_probs(q, k1=k, mask=mask, heads=heads, out=out)
    assert got is out
    torch.cuda.synchronize()
    assert untouched(), "the MFMA kernel wrote outside its tensor"
    _check(f"mfma dense {Tq}x{Tk}", got.cpu(), ref)
    for g_ in range(G):
        assert not got[g_, :, :, int(lens[g_]):].any(), "a finfo.min-masked key has a non-zero probability"
    # the descriptor kernel on the same inputs
    with mfma_attention(False):
        valu = ops.attention_probs(q, k1=k, mask=mask, heads=heads)
    _check(f"valu dense {Tq}x{Tk}", valu.cpu(), ref)
    err = rel_err(got, valu)
    print(f"mfma vs valu {Tq}x{Tk}: rel_err {err:.3e}")
    assert err < TOL
    # q / k read in place from [rows, 3*HD] buffers (row stride 3*HD, k at column HD), slot-major output
    qb = torch.zeros((G * Tq, 3 * HD), dtype=torch.bfloat16, device=dev)
    kb = torch.zeros((G * Tk, 3 * HD), dtype=torch.bfloat16, device=dev)
    qb[:, :HD] = q.view(G * Tq, HD)
    kb[:, HD:2 * HD] = k.view(G * Tk, HD)
    out2, untouched2 = _guarded((heads * G, Tq, Tk), dev)
    H.check(H.lib().fcmf_attn_mfma_probs(qb.data_ptr(), kb.data_ptr() + HD * 2, mask.data_ptr(), out2.data_ptr(), G, heads, Tq, Tk,
                                         3 * HD, 3 * HD, Tq * Tk, G * Tq * Tk, 1.0 / math.sqrt(d), H.stream()), "fcmf_attn_mfma_probs")
    torch.cuda.synchronize()
    assert untouched2(), "the MFMA kernel wrote outside its tensor (strided inputs)"
    assert torch.equal(out2.view(heads, G, Tq, Tk).transpose(0, 1), got), "strided q / k or the slot-major layout changed the values"


def test_mfma_kernel_limits_are_unsupported(dev):
    from fcmf_framework import _hip as H
    x = torch.zeros((257, 64), dtype=torch.bfloat16, device=dev)
    o = torch.zeros((257, 257), dtype=torch.float32, device=dev)
    L = H.lib()
    assert L.fcmf_attn_mfma_probs(x.data_ptr(), x.data_ptr(), None, o.data_ptr(), 1, 1, 16, 257, 64, 64, 0, 0, 1.0, H.stream()) == H.ERR_UNSUPPORTED
    assert L.fcmf_attn_mfma_probs(x.data_ptr(), x.data_ptr(), None, o.data_ptr(), 1, 1, 257, 16, 64, 64, 0, 0, 1.0, H.stream()) == H.ERR_UNSUPPORTED
    assert L.fcmf_attn_mfma_probs(x.data_ptr(), x.data_ptr(), None, o.data_ptr(), 1, 1, 16, 16, 60, 64, 0, 0, 1.0, H.stream()) == H.ERR_UNSUPPORTED


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. fully masked sequence
@pytest.mark.parametrize("T", [128, 100, 48])
@pytest.mark.parametrize("use_mfma", [True, False])
def test_fully_masked_sequence_is_uniform(dev, T, use_mfma):
    """a sequence whose every key carries finfo.min comes out uniform, 1/T (torch and the forward kernels:
    test_ops_gpu.test_attention_mfma_fully_masked_sequence_is_uniform), next to a normal and a half-padded one"""
    from fcmf_framework import ops
    heads, d = 2, 64
    q = _rand((3, T, heads * d), dev, torch.bfloat16, 0.8, seed=1)
    k = _rand((3, T, heads * d), dev, torch.bfloat16, 0.8, seed=2)
    m01 = torch.ones(3, T)
    m01[1] = 0
    m01[2, T // 2:] = 0
    mask = ((1 - m01) * FMIN).to(dev)
    with mfma_attention(use_mfma):
        got = ops.attention_probs(q, k1=k, mask=mask, heads=heads).cpu()
    _check(f"fully masked T={T} mfma={use_mfma}", got, _probs_ref(q, k, mask=mask, heads=heads))
    dev_u = (got[1] - 1.0 / T).abs().max().item()
    print(f"  uniform row: max |p - 1/T| {dev_u:.3e}")
    assert dev_u < 1e-7
    assert not got[2, :, :, T // 2:].any(), "masked keys of the padded sequence must be exactly 0"


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. consistency with the forward
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", [(3, 20, 4, 16, 20, 0, 1, True, False, False), (4, 3, 2, 16, 10, 7, 2, True, False, False),
                                  (2, 77, 2, 64, 128, 0, 1, True, False, False)])
def test_probs_times_values_is_the_forward_output(dev, dtype, case):
    """P @ V in float64 from the returned P equals ops.attention's output (the last case runs both on the MFMA kernels in bf16)"""
    from fcmf_framework import ops
    G, R, heads, d, T1, T2, gd, _, _, causal = case
    q, k1, k2, mask, bias = _inputs(case, dev, dtype)
    v1 = _rand((G, T1, heads * d), dev, dtype, 0.7, seed=3) if T1 else None
    v2 = _rand((G // gd, R, T2, heads * d), dev, dtype, 0.7, seed=5) if T2 else None
    out = ops.attention(q, k1, v1, k2, v2, mask=mask, bias=bias, heads=heads, group_div=gd, causal=causal)
    P = ops.attention_probs(q, k1=k1, k2=k2, mask=mask, bias=bias, heads=heads, group_div=gd, causal=causal).double().cpu()
    pv = torch.zeros(G, heads, R, d, dtype=torch.float64)
    if T1:
        pv += torch.einsum("ghrt,gthd->ghrd", P[..., :T1], v1.double().cpu().view(G, T1, heads, d))
    if T2:
        v2g = v2.double().cpu()[torch.arange(G) // gd].view(G, R, T2, heads, d)
        pv += torch.einsum("ghrt,grthd->ghrd", P[..., T1:], v2g)
    ref = pv.transpose(1, 2).reshape(G, R, heads * d)
    err = rel_err(out, ref)
    print(f"P @ V vs forward {case} {dtype}: rel_err {err:.3e}")
    assert err < (3e-5 if dtype == torch.float32 else 3e-2)


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. RobertaModel(output_attentions=True)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_roberta_output_attentions(dev, dtype):
    from fcmf_framework import ops
    from fcmf_framework.roberta import RobertaConfig, RobertaModel
    cfg = RobertaConfig(vocab_size=120, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
                        max_position_embeddings=64)
    torch.manual_seed(3)
    model = RobertaModel(cfg).to(dev).eval()
    B, S, heads, d = 3, 48, 2, 64
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(3, 120, (B, S), generator=g)
    am = torch.ones(B, S, dtype=torch.int64)
    am[1, 30:] = 0
    am[2, 7:] = 0
    ids[am == 0] = cfg.pad_token_id
    ids, am = ids.to(dev), am.to(dev)
    captured = []
    hooks = [l.register_forward_pre_hook(lambda m, args: captured.append(args[0].detach().clone())) for l in model.encoder.layer]
    ops.set_compute_dtype(dtype)
    try:
        with torch.no_grad():
            seq1, pooled1, att = model(input_ids=ids, attention_mask=am, output_attentions=True)
            seq0, pooled0, none = model(input_ids=ids, attention_mask=am)
    finally:
        ops.set_compute_dtype(torch.float32)
        for h in hooks:
            h.remove()
    assert none == ()
    assert torch.equal(seq0, seq1) and torch.equal(pooled0, pooled1), "asking for the probabilities changed the model's outputs"
    assert isinstance(att, tuple) and len(att) == 2
    mask = ((1 - am.float()) * FMIN)
    for i, (layer, x) in enumerate(zip(model.encoder.layer, captured[:2])):
        assert x.dtype == dtype
        sa = layer.attention.self
        # q / k as the layer's kernels load them: float64 projection of the stored input with the compute-dtype weights and the
        # float32 bias, rounded to the compute dtype
        proj = lambda lin: (x.double().cpu() @ lin.weight.detach().to(dtype).double().cpu().t() + lin.bias.detach().double().cpu()).to(dtype)
        ref = _probs_ref(proj(sa.query), proj(sa.key), mask=mask, heads=heads)
        assert tuple(att[i].shape) == (B, heads, S, S)
        _check(f"roberta layer {i} {dtype}", att[i].cpu(), ref)
        assert not att[i][2, :, :, 7:].any()


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. IAOG decoder
@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLD, "iaog_attention_weights.npz"))


GOLD_CASES = [(B, kind) for B in (1, 2, 3) for kind in ("self", "cross", "cross_tril")]


@pytest.mark.parametrize("B,kind", GOLD_CASES)
def test_decoder_attention_reproduces_reference_score_and_output(dev, golden, B, kind):
    """Attention with the fixture's weights returns the reference's `score` (in its slot order) and `output`, on both routes: the
    fused self-attention node (k is q) and the head_linear cross attention.  The fixture is the reference's own float32 result (its
    rounding is ~1e-6 relative at these 32- and 8-term sums), held to the same 3e-5 as the float64 comparisons."""
    from fcmf_framework import ops
    from fcmf_framework.iaog_modeling import Attention
    att = Attention(32, 8, 4).to(dev).eval()
    with torch.no_grad():
        att.w_kx.copy_(torch.from_numpy(golden["w_kx"]))
        att.w_qx.copy_(torch.from_numpy(golden["w_qx"]))
        att.proj.weight.copy_(torch.from_numpy(golden["proj_w"]))
        att.proj.bias.copy_(torch.from_numpy(golden["proj_b"]))
    t = lambda key: torch.from_numpy(golden[f"B{B}_{kind}_{key}"]).to(dev)
    k, q = t("k"), t("q")
    if kind == "self":
        k = q
    ml = None if kind == "cross" else torch.ones(B, k.shape[1], dtype=torch.int64, device=dev)
    ops.set_output_attentions(True)
    try:
        with torch.no_grad():
            out, score = att(k, q, ml)
    finally:
        ops.set_output_attentions(False)
    assert score is att.attention_weights and tuple(score.shape) == (4 * B, 5, k.shape[1]) and score.dtype == torch.float32
    _check(f"decoder Attention B={B} {kind} score", score.cpu(), torch.from_numpy(golden[f"B{B}_{kind}_score"]))
    err = rel_err(out, torch.from_numpy(golden[f"B{B}_{kind}_output"]))
    print(f"decoder Attention B={B} {kind} output: rel_err {err:.3e}")
    assert err < TOL
    with torch.no_grad():
        out_off, none = att(k, q, ml)
    assert none is None and att.attention_weights is None
    assert torch.equal(out_off, out)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_decoder_attention_weights_follow_the_switch(dev, dtype):
    from fcmf_framework import ops
    from fcmf_framework.iaog_modeling import IAOGDecoder
    torch.manual_seed(11)
    B, Ld, Le, H, nh, nb = 3, 5, 7, 32, 4, 2
    dec = IAOGDecoder(vocab_size=64, hidden_size=H, num_layers=nb, num_heads=nh).to(dev).eval()
    enc = _rand((B, Le, H), dev, seed=1)
    X = torch.randint(0, 64, (B, Ld), generator=torch.Generator().manual_seed(2)).to(dev)
    emask = torch.ones(B, Le, dtype=torch.int64, device=dev)
    ops.set_compute_dtype(dtype)
    try:
        with torch.no_grad():
            off = dec(X, dec.init_state(enc, emask))
            w_off = dec.attention_weights
            ops.set_output_attentions(True)
            on = dec(X, dec.init_state(enc, emask))
            w_on = dec.attention_weights
    finally:
        ops.set_output_attentions(False)
        ops.set_compute_dtype(torch.float32)
    assert torch.equal(on, off), "asking for the probabilities changed the decoder's output"
    assert all(w is None for row in w_off for w in row)
    assert len(w_on) == 2 and all(len(row) == nb for row in w_on)
    for i in range(nb):
        for w, T in ((w_on[0][i], Ld), (w_on[1][i], Le)):
            assert torch.is_tensor(w) and tuple(w.shape) == (nh * B, Ld, T) and w.dtype == torch.float32
            rows = (w.double().sum(-1) - 1).abs().max().item()
            assert rows < 1e-4
            # the tril rule: key t > r carries -1e4 against scores of order 1 -> exp(-1e4) == 0 in float32
            r, t_ = torch.arange(Ld)[:, None], torch.arange(T)[None, :]
            assert not w.cpu()[:, t_ > r].any()


def test_encoder_carries_enc_attentions(dev):
    """FCMFEncoder / FCMFSeq2Seq hand the text encoder's probabilities on as `enc_attentions` when the switch is on, () when off"""
    import synthetic_data as synth
    from fcmf_framework import ops
    from fcmf_framework.fcmf_pretraining import FCMFSeq2Seq
    from helpers import make_hf_dir
    cfg = synth.TINY_CFG
    NI, NR, B, S = 2, 3, 2, 16
    torch.manual_seed(1)
    model = FCMFSeq2Seq(cfg["vocab_size"], 8, make_hf_dir(cfg), NI, NR, 0.7).to(dev).eval()
    b = {k: v.to(dev) for k, v in synth.synth_batch(B, cfg, S=S, num_imgs=NI, num_roi=NR, seed=1).items()}
    args = (b["input_ids"][:, 0], b["visual_embeds_att"], b["roi_embeds_att"], b["roi_coors"], b["token_type_ids"][:, 0],
            b["attention_mask"][:, 0], b["added_attention_mask"][:, 0])
    dec_X = torch.randint(0, cfg["vocab_size"], (B, 6), generator=torch.Generator().manual_seed(3)).to(dev)
    with torch.no_grad():
        out0, att0 = model.encoder(*args)
        ops.set_output_attentions(True)
        try:
            out1, att1 = model.encoder(*args)
            logits, att2 = model(args[0], dec_X, *args[1:4], token_type_ids=args[4], attention_mask=args[5],
                                 added_attention_mask=args[6], is_train=False)
        finally:
            ops.set_output_attentions(False)
    assert att0 == () and torch.equal(out0, out1)
    heads = cfg["num_attention_heads"]
    for att in (att1, att2):
        assert isinstance(att, tuple) and len(att) == cfg["num_hidden_layers"]
        for p in att:
            assert tuple(p.shape) == (B, heads, S, S) and p.dtype == torch.float32
            assert (p.double().sum(-1) - 1).abs().max().item() < 1e-4
    assert all(torch.equal(a, c) for a, c in zip(att1, att2))
