"""The weight-shadow cache on the GPU: the VALUES of every kind of copy against torch, bit for bit, and the library calls that
three training steps of a live model make with the cache in the loop.
EXPECTED was printed by this file (the MEASURED lines) at the commit before fcmf_framework/shadows.py existed, where it runs
unmodified -- it uses `ops.shadows`' public methods only: profiles/r12_shadow_cache_ab.txt."""
import pytest
import torch

import synthetic_data as synth
from helpers import _calls_digest, _recorded, batch_to, build_fcmf

pytestmark = pytest.mark.gpu

KINDS = ["get", "padded", "get_t", "get_fp8", "get_fp8_t", "head_nk", "derived"]
SHAPE = {"padded": (70, 128), "head_nk": (2, 32, 16)}      # (70 rows pad to 96); every other kind: (64, 128)


def _rand(shape, dev, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dev)


def _ask(kind, p):
    from fcmf_framework import ops
    if kind == "head_nk":
        return ops.shadows.head_nk([p])
    if kind == "derived":
        return ops.shadows.derived(p, "t", lambda src: src.t().contiguous().bfloat16())
    return getattr(ops.shadows, kind)(p)


def _want(kind, p):
    """what torch gives for the CURRENT contents of p's storage"""
    from fcmf_framework import ops
    w = p.detach()
    if kind == "get":
        return w.bfloat16()
    if kind == "padded":
        return torch.cat((w.bfloat16(), torch.zeros((96 - 70, 128), dtype=torch.bfloat16, device=w.device)))
    if kind in ("get_t", "derived"):
        return w.t().contiguous().bfloat16()
    if kind in ("get_fp8", "get_fp8_t"):
        src = w.bfloat16() if kind == "get_fp8" else w.t().contiguous().bfloat16()
        return ops.quant_fp8_rows(src, src.shape[0], src.shape[1], src.shape[1])
    nh, E, d = w.shape
    return w.permute(0, 2, 1).reshape(nh * d, E).bfloat16()      # row h * d + j = w[h, :, j]


def _same(got, want):
    got, want = (got, want) if isinstance(got, tuple) else ((got,), (want,))
    return len(got) == len(want) and all(g.shape == w.shape and g.dtype == w.dtype and torch.equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("kind", KINDS)
def test_every_copy_is_bitwise_what_torch_gives(dev, kind):
    """after the first build; after a raw rewrite of the storage and mark_all_stale(); and for a SECOND Parameter over the same
    storage after a raw rewrite without mark_all_stale() -- what a new model's parameter at a freed model's address is: it must
    get a copy of what lies there now, not the first Parameter's cached one."""
    from fcmf_framework import ops
    ops.shadows.clear()
    try:
        a = torch.nn.Parameter(_rand(SHAPE.get(kind, (64, 128)), dev, 1))
        assert _same(_ask(kind, a), _want(kind, a))
        a.data.copy_(_rand(a.shape, dev, 2))
        ops.shadows.mark_all_stale()
        assert _same(_ask(kind, a), _want(kind, a))
        b = torch.nn.Parameter(a.data)
        assert b.data_ptr() == a.data_ptr() and b._version == a._version
        a.data.copy_(_rand(a.shape, dev, 3))
        assert _same(_ask(kind, b), _want(kind, b))
    finally:
        ops.shadows.clear()


# ------------------------------------------------------------------------------------------------------------------------
# the library calls of three training steps
# ------------------------------------------------------------------------------------------------------------------------
def _steps(params, loss):
    from fcmf_framework.optimization import FusedAdamW
    opt = FusedAdamW(list(params), lr=1e-3)
    for _ in range(3):
        loss().backward()
        opt.step(max_grad_norm=1.0)
        opt.zero_grad(set_to_none=True)


def _fcmf(dev):
    NI, NR, B, S = 2, 5, 3, 16
    model, _ = build_fcmf(synth.TINY_CFG, NI, NR, dev)
    model.train()
    b = batch_to(synth.synth_batch(B, synth.TINY_CFG, S=S, num_imgs=NI, num_roi=NR, seed=1), dev)

    def loss():
        logits = model.forward_aspects(b["input_ids"], b["visual_embeds_att"], b["roi_embeds_att"], b["roi_coors"],
                                       b["token_type_ids"], b["attention_mask"], b["added_attention_mask"])
        return model.loss_aspects(logits, b["labels"])
    return model.parameters(), loss


def _decoder(dev):
    """the decoder of test_head_projection_gpu._decoder_calls: 2 blocks, 4 heads, 256 wide, B = 3 sequences of 8 tokens, 16 encoder rows"""
    from fcmf_framework.iaog_modeling import IAOGDecoder
    torch.manual_seed(0)
    m = IAOGDecoder(vocab_size=96, hidden_size=256, num_layers=2, num_heads=4).to(dev).train()
    g = torch.Generator().manual_seed(1)
    enc = torch.randn((3, 16, 256), generator=g).to(dev).requires_grad_(True)
    ids, labels = (torch.randint(0, 96, (3, 8), generator=g).to(dev) for _ in range(2))
    return m.parameters(), lambda: m.loss(ids, m.init_state(enc, None), labels)


def _roberta_layer_fp8(dev):
    """hidden 128, 2 heads, intermediate 256, T = 48; 6 sequences: 288 rows, so that the e4m3 GEMMs' own gate (M, N >= 256, K a
    multiple of 128) lets the q|k|v and first feed-forward GEMMs (get_fp8) and the second one's dX (get_fp8_t) through"""
    from fcmf_framework.roberta import RobertaConfig, RobertaLayer
    torch.manual_seed(0)
    layer = RobertaLayer(RobertaConfig(vocab_size=120, hidden_size=128, num_hidden_layers=1, num_attention_heads=2,
                                       intermediate_size=256, max_position_embeddings=160)).to(dev).train()
    x = _rand((6, 48, 128), dev, 1).bfloat16().requires_grad_(True)
    mask = torch.zeros((6, 48), device=dev)
    return layer.parameters(), lambda: layer(x, mask).float().sum()


def _packed_in_proj(dev):
    """the baselines' modules (embed 128, 2 heads): a TransformerEncoderLayer (the packed in_proj_weight as the fused q|k|v
    block) and a MultiheadAttention reading 24 memory rows (its three slices through ops.linear)"""
    from fcmf_framework.torch_layers import MultiheadAttention, TransformerEncoderLayer
    torch.manual_seed(0)
    enc = TransformerEncoderLayer(128, 2, dim_feedforward=256, dropout=0.1, activation="gelu", batch_first=True).to(dev).train()
    cross = MultiheadAttention(128, 2, dropout=0.1, batch_first=True).to(dev).train()
    x, mem = (_rand(s, dev, i).bfloat16().requires_grad_(True) for i, s in enumerate([(2, 16, 128), (2, 24, 128)]))
    return list(enc.parameters()) + list(cross.parameters()), lambda: cross(enc(x), mem, mem)[0].float().sum()


CASES = {"fcmf-bf16": (_fcmf, torch.bfloat16, False), "decoder-bf16": (_decoder, torch.bfloat16, False),
         "decoder-f32": (_decoder, torch.float32, False), "roberta-layer-fp8": (_roberta_layer_fp8, torch.bfloat16, True),
         "packed-in-proj-bf16": (_packed_in_proj, torch.bfloat16, False)}
TRANSPOSES = ("fcmf_cast_transpose", "fcmf_multi_cast_transpose")

# case -> (entry points in call order, SHA-256 of [(name, scalar arguments, return code), ...]) at the parent commit
EXPECTED = {
    "fcmf-bf16": ("""
        fcmf_position_ids fcmf_embed_ln_fwd fcmf_additive_mask fcmf_cast fcmf_gemm fcmf_attn_small_fwd fcmf_cast
        fcmf_cast fcmf_cast fcmf_gemm fcmf_add_ln_fwd fcmf_gemm fcmf_gemm fcmf_add_ln_fwd fcmf_cast fcmf_gemm
        fcmf_attn_small_fwd fcmf_cast fcmf_cast fcmf_cast fcmf_gemm fcmf_add_ln_fwd fcmf_gemm fcmf_gemm
        fcmf_add_ln_fwd fcmf_cast fcmf_cast fcmf_gemm fcmf_gemm fcmf_cast fcmf_cast fcmf_gemm fcmf_cast fcmf_gemm
        fcmf_cast fcmf_gemm fcmf_cast fcmf_cast fcmf_gemm fcmf_box_bias_fwd fcmf_cast fcmf_gemm fcmf_cast fcmf_gemm
        fcmf_cast fcmf_gemm fcmf_attn_small_fwd fcmf_cast fcmf_gemm fcmf_gemm fcmf_gemm fcmf_cast fcmf_gemm
        fcmf_additive_mask fcmf_attn_small_fwd fcmf_cast fcmf_cast fcmf_cast fcmf_gemm fcmf_add_ln_fwd fcmf_gemm
        fcmf_gemm fcmf_add_ln_fwd fcmf_cast fcmf_gemm fcmf_cast fcmf_gemm fcmf_additive_mask fcmf_attn_small_fwd
        fcmf_cast fcmf_cast fcmf_cast fcmf_gemm fcmf_add_ln_fwd fcmf_gemm fcmf_gemm fcmf_add_ln_fwd fcmf_cast
        fcmf_gemm fcmf_additive_mask fcmf_cast fcmf_gemm fcmf_attn_small_fwd fcmf_gemm fcmf_add_ln_fwd fcmf_gemm
        fcmf_gemm fcmf_add_ln_fwd fcmf_cast fcmf_gemm fcmf_dropout fcmf_cast fcmf_gemm fcmf_xent_fwd fcmf_xent_mean
        fcmf_xent_bwd fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_colsum fcmf_dropout fcmf_act_bwd
        fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_colsum fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd
        fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_add_ln_bwd_workspace
        fcmf_add_ln_bwd fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_attn_small_bwd fcmf_colsum fcmf_cast_transpose
        fcmf_gemm fcmf_gemm fcmf_act_bwd fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_colsum fcmf_add_ln_bwd_workspace
        fcmf_add_ln_bwd fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_gemm
        fcmf_gemm fcmf_attn_small_bwd_grouped fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_colsum fcmf_act_bwd
        fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_colsum fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd
        fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_add_ln_bwd_workspace
        fcmf_add_ln_bwd fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_attn_small_bwd_grouped fcmf_cast_transpose
        fcmf_gemm fcmf_gemm fcmf_colsum fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_colsum fcmf_cast_transpose
        fcmf_gemm fcmf_gemm fcmf_colsum fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_colsum fcmf_attn_small_bwd
        fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_colsum fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_colsum
        fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_colsum fcmf_box_bias_bwd fcmf_gemm fcmf_colsum
        fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_colsum fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_colsum
        fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm fcmf_colsum
        fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_cast_transpose
        fcmf_gemm fcmf_gemm fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_cast_transpose fcmf_gemm fcmf_gemm
        fcmf_attn_small_bwd fcmf_colsum fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_add_ln_bwd_workspace
        fcmf_add_ln_bwd fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_cast_transpose fcmf_gemm fcmf_gemm
        fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_attn_small_bwd
        fcmf_colsum fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_dropout fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd
        fcmf_embed_pos_type_bwd fcmf_embed_bwd fcmf_multi_sumsq fcmf_multi_adamw fcmf_multi_cast_transpose
        fcmf_position_ids fcmf_embed_ln_fwd fcmf_additive_mask fcmf_cast fcmf_gemm fcmf_attn_small_fwd fcmf_gemm
        fcmf_add_ln_fwd fcmf_gemm fcmf_gemm fcmf_add_ln_fwd fcmf_cast fcmf_gemm fcmf_attn_small_fwd fcmf_gemm
        fcmf_add_ln_fwd fcmf_gemm fcmf_gemm fcmf_add_ln_fwd fcmf_gemm fcmf_gemm fcmf_cast fcmf_gemm fcmf_gemm
        fcmf_gemm fcmf_cast fcmf_gemm fcmf_box_bias_fwd fcmf_gemm fcmf_gemm fcmf_gemm fcmf_attn_small_fwd fcmf_gemm
        fcmf_gemm fcmf_gemm fcmf_gemm fcmf_additive_mask fcmf_attn_small_fwd fcmf_gemm fcmf_add_ln_fwd fcmf_gemm
        fcmf_gemm fcmf_add_ln_fwd fcmf_gemm fcmf_gemm fcmf_additive_mask fcmf_attn_small_fwd fcmf_gemm fcmf_add_ln_fwd
        fcmf_gemm fcmf_gemm fcmf_add_ln_fwd fcmf_gemm fcmf_additive_mask fcmf_cast fcmf_gemm fcmf_attn_small_fwd
        fcmf_gemm fcmf_add_ln_fwd fcmf_gemm fcmf_gemm fcmf_add_ln_fwd fcmf_gemm fcmf_dropout fcmf_gemm fcmf_xent_fwd
        fcmf_xent_mean fcmf_xent_bwd fcmf_gemm fcmf_gemm fcmf_colsum fcmf_dropout fcmf_act_bwd fcmf_gemm fcmf_gemm
        fcmf_colsum fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm
        fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_gemm fcmf_gemm fcmf_attn_small_bwd fcmf_colsum fcmf_gemm
        fcmf_gemm fcmf_act_bwd fcmf_gemm fcmf_gemm fcmf_colsum fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_gemm
        fcmf_gemm fcmf_gemm fcmf_gemm fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_gemm fcmf_gemm
        fcmf_attn_small_bwd_grouped fcmf_gemm fcmf_gemm fcmf_colsum fcmf_act_bwd fcmf_gemm fcmf_gemm fcmf_colsum
        fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_add_ln_bwd_workspace
        fcmf_add_ln_bwd fcmf_gemm fcmf_gemm fcmf_attn_small_bwd_grouped fcmf_gemm fcmf_gemm fcmf_colsum fcmf_gemm
        fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm fcmf_colsum fcmf_attn_small_bwd
        fcmf_gemm fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm fcmf_colsum
        fcmf_box_bias_bwd fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm fcmf_colsum
        fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm fcmf_colsum
        fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_add_ln_bwd_workspace
        fcmf_add_ln_bwd fcmf_gemm fcmf_gemm fcmf_attn_small_bwd fcmf_colsum fcmf_gemm fcmf_gemm
        fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_add_ln_bwd_workspace
        fcmf_add_ln_bwd fcmf_gemm fcmf_gemm fcmf_attn_small_bwd fcmf_colsum fcmf_gemm fcmf_gemm fcmf_dropout
        fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_embed_pos_type_bwd fcmf_embed_bwd fcmf_multi_sumsq
        fcmf_multi_adamw fcmf_multi_cast_transpose fcmf_position_ids fcmf_embed_ln_fwd fcmf_additive_mask fcmf_cast
        fcmf_gemm fcmf_attn_small_fwd fcmf_gemm fcmf_add_ln_fwd fcmf_gemm fcmf_gemm fcmf_add_ln_fwd fcmf_cast
        fcmf_gemm fcmf_attn_small_fwd fcmf_gemm fcmf_add_ln_fwd fcmf_gemm fcmf_gemm fcmf_add_ln_fwd fcmf_gemm
        fcmf_gemm fcmf_cast fcmf_gemm fcmf_gemm fcmf_gemm fcmf_cast fcmf_gemm fcmf_box_bias_fwd fcmf_gemm fcmf_gemm
        fcmf_gemm fcmf_attn_small_fwd fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_additive_mask fcmf_attn_small_fwd
        fcmf_gemm fcmf_add_ln_fwd fcmf_gemm fcmf_gemm fcmf_add_ln_fwd fcmf_gemm fcmf_gemm fcmf_additive_mask
        fcmf_attn_small_fwd fcmf_gemm fcmf_add_ln_fwd fcmf_gemm fcmf_gemm fcmf_add_ln_fwd fcmf_gemm fcmf_additive_mask
        fcmf_cast fcmf_gemm fcmf_attn_small_fwd fcmf_gemm fcmf_add_ln_fwd fcmf_gemm fcmf_gemm fcmf_add_ln_fwd
        fcmf_gemm fcmf_dropout fcmf_gemm fcmf_xent_fwd fcmf_xent_mean fcmf_xent_bwd fcmf_gemm fcmf_gemm fcmf_colsum
        fcmf_dropout fcmf_act_bwd fcmf_gemm fcmf_gemm fcmf_colsum fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_gemm
        fcmf_gemm fcmf_gemm fcmf_gemm fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_gemm fcmf_gemm
        fcmf_attn_small_bwd fcmf_colsum fcmf_gemm fcmf_gemm fcmf_act_bwd fcmf_gemm fcmf_gemm fcmf_colsum
        fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_add_ln_bwd_workspace
        fcmf_add_ln_bwd fcmf_gemm fcmf_gemm fcmf_attn_small_bwd_grouped fcmf_gemm fcmf_gemm fcmf_colsum fcmf_act_bwd
        fcmf_gemm fcmf_gemm fcmf_colsum fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_gemm fcmf_gemm fcmf_gemm
        fcmf_gemm fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_gemm fcmf_gemm fcmf_attn_small_bwd_grouped fcmf_gemm
        fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm
        fcmf_colsum fcmf_attn_small_bwd fcmf_gemm fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm fcmf_colsum fcmf_gemm
        fcmf_gemm fcmf_colsum fcmf_box_bias_bwd fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm fcmf_colsum fcmf_gemm
        fcmf_gemm fcmf_colsum fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm fcmf_colsum
        fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_add_ln_bwd_workspace
        fcmf_add_ln_bwd fcmf_gemm fcmf_gemm fcmf_attn_small_bwd fcmf_colsum fcmf_gemm fcmf_gemm
        fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_add_ln_bwd_workspace
        fcmf_add_ln_bwd fcmf_gemm fcmf_gemm fcmf_attn_small_bwd fcmf_colsum fcmf_gemm fcmf_gemm fcmf_dropout
        fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_embed_pos_type_bwd fcmf_embed_bwd fcmf_multi_sumsq
        fcmf_multi_adamw fcmf_multi_cast_transpose
        """, "d727a50940d2524fe91a7243c26afddeeab09ef9ad99b3ac56c0b6a082609c7d"),
    "decoder-bf16": ("""
        fcmf_embed_scale_fwd fcmf_dropout fcmf_cast fcmf_multi_cast_transpose fcmf_gemm fcmf_multi_cast_transpose
        fcmf_gemm fcmf_attn_small_fwd fcmf_cast fcmf_gemm fcmf_add_ln_fwd fcmf_cast fcmf_multi_cast_transpose
        fcmf_gemm fcmf_attn_small_fwd fcmf_cast fcmf_gemm fcmf_add_ln_fwd fcmf_cast fcmf_cast fcmf_gemm fcmf_gemm
        fcmf_add_ln_fwd fcmf_multi_cast_transpose fcmf_gemm fcmf_attn_small_fwd fcmf_cast fcmf_gemm fcmf_add_ln_fwd
        fcmf_cast fcmf_multi_cast_transpose fcmf_gemm fcmf_attn_small_fwd fcmf_cast fcmf_gemm fcmf_add_ln_fwd
        fcmf_cast fcmf_cast fcmf_gemm fcmf_gemm fcmf_add_ln_fwd fcmf_cast fcmf_gemm fcmf_xent_fwd fcmf_xent_bwd
        fcmf_gemm fcmf_gemm fcmf_colsum fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_cast_transpose fcmf_gemm
        fcmf_gemm fcmf_colsum fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_colsum fcmf_add_ln_bwd_workspace
        fcmf_add_ln_bwd fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_colsum fcmf_attn_small_bwd fcmf_head_gather
        fcmf_head_gather fcmf_gemm fcmf_gemm fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_cast_transpose fcmf_gemm
        fcmf_gemm fcmf_colsum fcmf_attn_small_bwd fcmf_head_gather fcmf_head_gather fcmf_gemm fcmf_gemm
        fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_colsum
        fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_colsum fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd
        fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_colsum fcmf_attn_small_bwd fcmf_head_gather fcmf_head_gather
        fcmf_gemm fcmf_gemm fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_cast_transpose fcmf_gemm fcmf_gemm
        fcmf_colsum fcmf_attn_small_bwd fcmf_head_gather fcmf_head_gather fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm
        fcmf_cast fcmf_dropout fcmf_embed_scale_bwd fcmf_multi_sumsq fcmf_multi_adamw fcmf_multi_cast_transpose
        fcmf_embed_scale_fwd fcmf_dropout fcmf_cast fcmf_gemm fcmf_gemm fcmf_attn_small_fwd fcmf_gemm fcmf_add_ln_fwd
        fcmf_cast fcmf_gemm fcmf_attn_small_fwd fcmf_gemm fcmf_add_ln_fwd fcmf_gemm fcmf_gemm fcmf_add_ln_fwd
        fcmf_gemm fcmf_attn_small_fwd fcmf_gemm fcmf_add_ln_fwd fcmf_cast fcmf_gemm fcmf_attn_small_fwd fcmf_gemm
        fcmf_add_ln_fwd fcmf_gemm fcmf_gemm fcmf_add_ln_fwd fcmf_gemm fcmf_xent_fwd fcmf_xent_bwd fcmf_gemm fcmf_gemm
        fcmf_colsum fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_gemm fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm
        fcmf_colsum fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_gemm fcmf_gemm fcmf_colsum fcmf_attn_small_bwd
        fcmf_head_gather fcmf_head_gather fcmf_gemm fcmf_gemm fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_gemm
        fcmf_gemm fcmf_colsum fcmf_attn_small_bwd fcmf_head_gather fcmf_head_gather fcmf_gemm fcmf_gemm
        fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_gemm fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm fcmf_colsum
        fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_gemm fcmf_gemm fcmf_colsum fcmf_attn_small_bwd fcmf_head_gather
        fcmf_head_gather fcmf_gemm fcmf_gemm fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_gemm fcmf_gemm fcmf_colsum
        fcmf_attn_small_bwd fcmf_head_gather fcmf_head_gather fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_cast
        fcmf_dropout fcmf_embed_scale_bwd fcmf_multi_sumsq fcmf_multi_adamw fcmf_multi_cast_transpose
        fcmf_embed_scale_fwd fcmf_dropout fcmf_cast fcmf_gemm fcmf_gemm fcmf_attn_small_fwd fcmf_gemm fcmf_add_ln_fwd
        fcmf_cast fcmf_gemm fcmf_attn_small_fwd fcmf_gemm fcmf_add_ln_fwd fcmf_gemm fcmf_gemm fcmf_add_ln_fwd
        fcmf_gemm fcmf_attn_small_fwd fcmf_gemm fcmf_add_ln_fwd fcmf_cast fcmf_gemm fcmf_attn_small_fwd fcmf_gemm
        fcmf_add_ln_fwd fcmf_gemm fcmf_gemm fcmf_add_ln_fwd fcmf_gemm fcmf_xent_fwd fcmf_xent_bwd fcmf_gemm fcmf_gemm
        fcmf_colsum fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_gemm fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm
        fcmf_colsum fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_gemm fcmf_gemm fcmf_colsum fcmf_attn_small_bwd
        fcmf_head_gather fcmf_head_gather fcmf_gemm fcmf_gemm fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_gemm
        fcmf_gemm fcmf_colsum fcmf_attn_small_bwd fcmf_head_gather fcmf_head_gather fcmf_gemm fcmf_gemm
        fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_gemm fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm fcmf_colsum
        fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_gemm fcmf_gemm fcmf_colsum fcmf_attn_small_bwd fcmf_head_gather
        fcmf_head_gather fcmf_gemm fcmf_gemm fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_gemm fcmf_gemm fcmf_colsum
        fcmf_attn_small_bwd fcmf_head_gather fcmf_head_gather fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_cast
        fcmf_dropout fcmf_embed_scale_bwd fcmf_multi_sumsq fcmf_multi_adamw fcmf_multi_cast_transpose
        """, "1dadfb3989f59bb2d28ddf9d980c0dbaf4f2a5caf7499121ddf10145032bac8c"),
    "decoder-f32": ("""
        fcmf_embed_scale_fwd fcmf_dropout fcmf_gemm fcmf_gemm fcmf_attn_small_fwd fcmf_gemm fcmf_add_ln_fwd fcmf_gemm
        fcmf_attn_small_fwd fcmf_gemm fcmf_add_ln_fwd fcmf_gemm fcmf_gemm fcmf_add_ln_fwd fcmf_gemm
        fcmf_attn_small_fwd fcmf_gemm fcmf_add_ln_fwd fcmf_gemm fcmf_attn_small_fwd fcmf_gemm fcmf_add_ln_fwd
        fcmf_gemm fcmf_gemm fcmf_add_ln_fwd fcmf_gemm fcmf_xent_fwd fcmf_xent_bwd fcmf_gemm fcmf_gemm fcmf_colsum
        fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_gemm fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm fcmf_colsum
        fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_gemm fcmf_gemm fcmf_colsum fcmf_attn_small_bwd fcmf_head_gather
        fcmf_head_gather fcmf_gemm fcmf_gemm fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_gemm fcmf_gemm fcmf_colsum
        fcmf_attn_small_bwd fcmf_head_gather fcmf_head_gather fcmf_gemm fcmf_gemm fcmf_add_ln_bwd_workspace
        fcmf_add_ln_bwd fcmf_gemm fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm fcmf_colsum fcmf_add_ln_bwd_workspace
        fcmf_add_ln_bwd fcmf_gemm fcmf_gemm fcmf_colsum fcmf_attn_small_bwd fcmf_head_gather fcmf_head_gather
        fcmf_gemm fcmf_gemm fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_gemm fcmf_gemm fcmf_colsum
        fcmf_attn_small_bwd fcmf_head_gather fcmf_head_gather fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_dropout
        fcmf_embed_scale_bwd fcmf_multi_sumsq fcmf_multi_adamw fcmf_embed_scale_fwd fcmf_dropout fcmf_gemm fcmf_gemm
        fcmf_attn_small_fwd fcmf_gemm fcmf_add_ln_fwd fcmf_gemm fcmf_attn_small_fwd fcmf_gemm fcmf_add_ln_fwd
        fcmf_gemm fcmf_gemm fcmf_add_ln_fwd fcmf_gemm fcmf_attn_small_fwd fcmf_gemm fcmf_add_ln_fwd fcmf_gemm
        fcmf_attn_small_fwd fcmf_gemm fcmf_add_ln_fwd fcmf_gemm fcmf_gemm fcmf_add_ln_fwd fcmf_gemm fcmf_xent_fwd
        fcmf_xent_bwd fcmf_gemm fcmf_gemm fcmf_colsum fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_gemm fcmf_gemm
        fcmf_colsum fcmf_gemm fcmf_gemm fcmf_colsum fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_gemm fcmf_gemm
        fcmf_colsum fcmf_attn_small_bwd fcmf_head_gather fcmf_head_gather fcmf_gemm fcmf_gemm
        fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_gemm fcmf_gemm fcmf_colsum fcmf_attn_small_bwd fcmf_head_gather
        fcmf_head_gather fcmf_gemm fcmf_gemm fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_gemm fcmf_gemm fcmf_colsum
        fcmf_gemm fcmf_gemm fcmf_colsum fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_gemm fcmf_gemm fcmf_colsum
        fcmf_attn_small_bwd fcmf_head_gather fcmf_head_gather fcmf_gemm fcmf_gemm fcmf_add_ln_bwd_workspace
        fcmf_add_ln_bwd fcmf_gemm fcmf_gemm fcmf_colsum fcmf_attn_small_bwd fcmf_head_gather fcmf_head_gather
        fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_dropout fcmf_embed_scale_bwd fcmf_multi_sumsq fcmf_multi_adamw
        fcmf_embed_scale_fwd fcmf_dropout fcmf_gemm fcmf_gemm fcmf_attn_small_fwd fcmf_gemm fcmf_add_ln_fwd fcmf_gemm
        fcmf_attn_small_fwd fcmf_gemm fcmf_add_ln_fwd fcmf_gemm fcmf_gemm fcmf_add_ln_fwd fcmf_gemm
        fcmf_attn_small_fwd fcmf_gemm fcmf_add_ln_fwd fcmf_gemm fcmf_attn_small_fwd fcmf_gemm fcmf_add_ln_fwd
        fcmf_gemm fcmf_gemm fcmf_add_ln_fwd fcmf_gemm fcmf_xent_fwd fcmf_xent_bwd fcmf_gemm fcmf_gemm fcmf_colsum
        fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_gemm fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm fcmf_colsum
        fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_gemm fcmf_gemm fcmf_colsum fcmf_attn_small_bwd fcmf_head_gather
        fcmf_head_gather fcmf_gemm fcmf_gemm fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_gemm fcmf_gemm fcmf_colsum
        fcmf_attn_small_bwd fcmf_head_gather fcmf_head_gather fcmf_gemm fcmf_gemm fcmf_add_ln_bwd_workspace
        fcmf_add_ln_bwd fcmf_gemm fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm fcmf_colsum fcmf_add_ln_bwd_workspace
        fcmf_add_ln_bwd fcmf_gemm fcmf_gemm fcmf_colsum fcmf_attn_small_bwd fcmf_head_gather fcmf_head_gather
        fcmf_gemm fcmf_gemm fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_gemm fcmf_gemm fcmf_colsum
        fcmf_attn_small_bwd fcmf_head_gather fcmf_head_gather fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_dropout
        fcmf_embed_scale_bwd fcmf_multi_sumsq fcmf_multi_adamw
        """, "816ba71bea7fb6551a055aa91b9a49c921ab1872a5b1b49aadb8a8d1d5fcc7be"),
    "roberta-layer-fp8": ("""
        fcmf_cast fcmf_quant_fp8_rows fcmf_quant_fp8_rows fcmf_gemm_fp8 fcmf_attn_mfma_fwd fcmf_cast fcmf_cast
        fcmf_cast fcmf_gemm fcmf_add_ln_fwd_fp8 fcmf_quant_fp8_rows fcmf_gemm_fp8 fcmf_gemm fcmf_add_ln_fwd
        fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd_fp8 fcmf_cast_transpose fcmf_quant_fp8_rows fcmf_gemm_fp8 fcmf_gemm
        fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd_fp8 fcmf_cast_transpose
        fcmf_gemm fcmf_gemm fcmf_attn_mfma_bwd fcmf_colsum fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_multi_sumsq
        fcmf_multi_adamw fcmf_multi_cast_transpose fcmf_cast fcmf_quant_fp8_rows fcmf_quant_fp8_rows fcmf_gemm_fp8
        fcmf_attn_mfma_fwd fcmf_gemm fcmf_add_ln_fwd_fp8 fcmf_quant_fp8_rows fcmf_gemm_fp8 fcmf_gemm fcmf_add_ln_fwd
        fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd_fp8 fcmf_quant_fp8_rows fcmf_gemm_fp8 fcmf_gemm fcmf_gemm fcmf_gemm
        fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd_fp8 fcmf_gemm fcmf_gemm fcmf_attn_mfma_bwd fcmf_colsum fcmf_gemm
        fcmf_gemm fcmf_multi_sumsq fcmf_multi_adamw fcmf_multi_cast_transpose fcmf_cast fcmf_quant_fp8_rows
        fcmf_quant_fp8_rows fcmf_gemm_fp8 fcmf_attn_mfma_fwd fcmf_gemm fcmf_add_ln_fwd_fp8 fcmf_quant_fp8_rows
        fcmf_gemm_fp8 fcmf_gemm fcmf_add_ln_fwd fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd_fp8 fcmf_quant_fp8_rows
        fcmf_gemm_fp8 fcmf_gemm fcmf_gemm fcmf_gemm fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd_fp8 fcmf_gemm fcmf_gemm
        fcmf_attn_mfma_bwd fcmf_colsum fcmf_gemm fcmf_gemm fcmf_multi_sumsq fcmf_multi_adamw fcmf_multi_cast_transpose
        """, "e6452280304baef6cec06ae6239bc7b6ddaa48f35a1291d27c9e7935e42c559f"),
    "packed-in-proj-bf16": ("""
        fcmf_cast fcmf_gemm fcmf_attn_mfma_fwd fcmf_cast fcmf_cast fcmf_cast fcmf_gemm fcmf_add_ln_fwd fcmf_gemm
        fcmf_gemm fcmf_add_ln_fwd fcmf_cast fcmf_gemm fcmf_cast fcmf_gemm fcmf_cast fcmf_gemm fcmf_attn_mfma_long_fwd
        fcmf_cast fcmf_gemm fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_colsum fcmf_attn_mfma_long_bwd
        fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_colsum fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_colsum
        fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_colsum fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd
        fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_add_ln_bwd_workspace
        fcmf_add_ln_bwd fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_attn_mfma_bwd fcmf_colsum fcmf_cast_transpose
        fcmf_gemm fcmf_gemm fcmf_multi_sumsq fcmf_multi_adamw fcmf_multi_cast_transpose fcmf_gemm fcmf_attn_mfma_fwd
        fcmf_gemm fcmf_add_ln_fwd fcmf_gemm fcmf_gemm fcmf_add_ln_fwd fcmf_cast fcmf_gemm fcmf_cast fcmf_gemm
        fcmf_cast fcmf_gemm fcmf_attn_mfma_long_fwd fcmf_gemm fcmf_gemm fcmf_gemm fcmf_colsum fcmf_attn_mfma_long_bwd
        fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_colsum fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_colsum
        fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_colsum fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_gemm
        fcmf_gemm fcmf_gemm fcmf_gemm fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_gemm fcmf_gemm fcmf_attn_mfma_bwd
        fcmf_colsum fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_multi_sumsq fcmf_multi_adamw
        fcmf_multi_cast_transpose fcmf_gemm fcmf_attn_mfma_fwd fcmf_gemm fcmf_add_ln_fwd fcmf_gemm fcmf_gemm
        fcmf_add_ln_fwd fcmf_cast fcmf_gemm fcmf_cast fcmf_gemm fcmf_cast fcmf_gemm fcmf_attn_mfma_long_fwd fcmf_gemm
        fcmf_gemm fcmf_gemm fcmf_colsum fcmf_attn_mfma_long_bwd fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_colsum
        fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_colsum fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_colsum
        fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_add_ln_bwd_workspace
        fcmf_add_ln_bwd fcmf_gemm fcmf_gemm fcmf_attn_mfma_bwd fcmf_colsum fcmf_cast_transpose fcmf_gemm fcmf_gemm
        fcmf_multi_sumsq fcmf_multi_adamw fcmf_multi_cast_transpose
        """, "7e25eda0761d6351087f1076bf5cb4d1c4cc27263d5d7fabd33bfd9c90e2beec"),
}
# The one difference: the parent keyed the transposed copies of the packed in_proj_weight's slices on the temporary view objects, so
# every optimizer step pruned them and every backward built them again.  They now belong to the Parameter.
# case -> (positions in the parent's sequence of the fcmf_cast_transpose calls that no longer happen,
#          SHA-256 of the parent's record without the two transpose entry points,
#          what the remaining transpose calls carry: (name, scalar arguments, return code) in order)
DROPPED = {
    "packed-in-proj-bf16": ([77, 81, 85, 101, 126, 130, 134, 150], "95d9c20fa2aa747d5ddfab38becb1833be6c5fd2013c08126a1930d9b6dfb062",
        [('fcmf_cast_transpose', (128, 128), 0), ('fcmf_cast_transpose', (128, 128), 0), ('fcmf_cast_transpose', (128, 128), 0), ('fcmf_cast_transpose', (128, 128), 0)]
        + [('fcmf_cast_transpose', (128, 256), 0), ('fcmf_cast_transpose', (256, 128), 0), ('fcmf_cast_transpose', (128, 128), 0), ('fcmf_cast_transpose', (384, 128), 0)]
        + 3 * [('fcmf_multi_cast_transpose', (24 + 24,), 0)]),     # (the parent's 24 blocks of 64 x 64 + [384, 128]: 12 + 3 x [128, 128]: 4 each)
}


@pytest.mark.parametrize("case", list(CASES))
def test_three_training_steps_make_the_parents_library_calls(dev, case):
    from fcmf_framework import ops
    build, dtype, fp8 = CASES[case]
    ops.set_compute_dtype(dtype)
    ops.set_fp8(fp8)
    ops.manual_seed(0)
    ops.shadows.clear()
    try:
        params, loss = build(dev)
        calls = _recorded(lambda: _steps(params, loss))
    finally:
        ops.set_compute_dtype(torch.float32)
        ops.set_fp8(False)
        ops.shadows.clear()
    names = [c[0] for c in calls]
    rest = [c for c in calls if c[0] not in TRANSPOSES]
    print("MEASURED", repr(case), (" ".join(names), _calls_digest(calls)))
    print("    without the transposes:", _calls_digest(rest))
    for i, c in enumerate(calls):
        if c[0] in TRANSPOSES:
            print("   ", i, c)
    exp_names, exp_digest = EXPECTED[case]
    exp_names = exp_names.split()
    if case not in DROPPED:
        assert names == exp_names
        assert _calls_digest(calls) == exp_digest
    else:
        gone, rest_digest, transposes = DROPPED[case]
        assert all(exp_names[i] == "fcmf_cast_transpose" for i in gone)
        assert names == [n for i, n in enumerate(exp_names) if i not in gone]          # no call gained, these lost
        assert _calls_digest(rest) == rest_digest                                      # every other call: the parent's arguments
        assert [c for c in calls if c[0] in TRANSPOSES] == transposes
