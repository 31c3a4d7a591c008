"""Every library call the public attention entry points make, forward and backward, with the descriptors they pass
(helpers._recorded(desc=True): scalar arguments as the C ABI receives them, every fcmf_attn_desc's non-pointer fields, which of
its pointers are non-null and whether v1 == k1).  The callers build their descriptors, choose MFMA or VALU and launch through
fcmf_framework.attn; what they issue has to be what their own hand-written call sites issued before that module existed.
EXPECTED was printed by this file (the MEASURED lines) at the commit before fcmf_framework/attn.py, with the one line below that
names the module holding the switch reading `from fcmf_framework import ops as switch`: profiles/r11_attention_path_ab.txt."""
import pytest
import torch

from fcmf_framework import attn as switch
from helpers import _calls_digest, _recorded
from test_head_projection_gpu import _decoder_calls, _set

pytestmark = pytest.mark.gpu


def _rand(shape, dev, dtype=torch.float32, seed=0, grad=False):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * 0.7).to(dtype).to(dev).requires_grad_(grad)


def _mask(G, T, dev):
    m01 = (torch.rand(G, T, generator=torch.Generator().manual_seed(7)) > 0.2).float()
    m01[:, 0] = 1
    return ((1 - m01) * -10000.0).to(dev)


def _attention(dev, dtype, G, R, T1, T2, heads, d, gd=1, mask=False, bias=False, p=0.0):
    from fcmf_framework import ops
    HD = heads * d
    q = _rand((G, R, HD), dev, dtype, 1, True)
    k1, v1 = (_rand((G, T1, HD), dev, dtype, s, True) for s in (2, 3))
    k2, v2 = (_rand((G // gd, R, T2, HD), dev, dtype, s, True) for s in (4, 5)) if T2 else (None, None)
    b = _rand((G // gd, heads, R, T1 + T2), dev, seed=8, grad=True) if bias else None
    out = ops.attention(q, k1, v1, k2, v2, mask=_mask(G, T1 + T2, dev) if mask else None, bias=b, heads=heads, group_div=gd, p=p,
                        training=True)
    out.float().sum().backward()
    assert b is None or b.grad is not None


def _probs(dev, dtype, d, slot_major, **kw):
    from fcmf_framework import ops
    G, R, T, heads = 3, 16, 48, 2
    q, k = _rand((G, R, heads * d), dev, dtype, 1), _rand((G, T, heads * d), dev, dtype, 2)
    ops.attention_probs(q, k1=k, mask=_mask(G, T, dev), heads=heads, slot_major=slot_major, **kw)


def _shared_kv(dev, dtype, Tk, p=0.0):
    from fcmf_framework import ops
    G, Tq, heads, d, share = 4, 5, 2, 64, 2
    q = _rand((G, Tq, heads * d), dev, dtype, 1, True)
    k, v = (_rand((G // share, Tk, heads * d), dev, dtype, s, True) for s in (2, 3))
    out = ops.shared_kv_attention(q, k, v, mask=_mask(G, Tk, dev), heads=heads, kv_share=share, p=p, training=True)
    out.float().sum().backward()


def _self_layer(dev, dtype, T):
    """one training pass of a RobertaLayer (hidden 128, 2 heads of 64, attention dropout 0.1) that also returns its probabilities"""
    from fcmf_framework.roberta import RobertaConfig, RobertaLayer
    _set(dtype)
    try:
        torch.manual_seed(0)
        layer = RobertaLayer(RobertaConfig(vocab_size=120, hidden_size=128, num_hidden_layers=1, num_attention_heads=2,
                                           intermediate_size=256, max_position_embeddings=160)).to(dev).train()
        x = _rand((2, T, 128), dev, dtype, 1, True)
        probs = torch.empty((2, 2, T, T), dtype=torch.float32, device=dev)
        layer(x, _mask(2, T, dev), probs=probs).float().sum().backward()
    finally:
        _set(torch.float32)


F32, BF16 = torch.float32, torch.bfloat16
SCENES = {
    "attention-f32-masked-dropout": lambda dev: _attention(dev, F32, 2, 5, 7, 0, 2, 16, mask=True, p=0.1),
    "attention-f32-two-dq-partials": lambda dev: _attention(dev, F32, 2, 5, 130, 0, 2, 16),
    "attention-f32-grouped": lambda dev: _attention(dev, F32, 4, 3, 6, 4, 2, 16, gd=2, bias=True),
    "attention-f32-group-div-1": lambda dev: _attention(dev, F32, 4, 3, 6, 4, 2, 16, gd=1, bias=True),
    "attention-bf16-mfma": lambda dev: _attention(dev, BF16, 2, 16, 48, 0, 2, 64, mask=True),
    "attention-bf16-valu": lambda dev: _attention(dev, BF16, 2, 16, 48, 0, 2, 64, mask=True),
    "probs-mfma": lambda dev: _probs(dev, BF16, 64, False),
    "probs-mfma-slot-major": lambda dev: _probs(dev, BF16, 64, True),
    "probs-valu": lambda dev: _probs(dev, F32, 16, False),
    "probs-valu-slot-major": lambda dev: _probs(dev, F32, 16, True),
    "probs-head-quirk": lambda dev: _probs(dev, BF16, 64, True, causal=True, head_quirk=True),
    "shared-kv-bf16-300": lambda dev: _shared_kv(dev, BF16, 300),
    "shared-kv-f32-100": lambda dev: _shared_kv(dev, F32, 100),
    "shared-kv-f32-300-dropout": lambda dev: _shared_kv(dev, F32, 300, p=0.1),
    "self-layer-bf16-16": lambda dev: _self_layer(dev, BF16, 16),
    "self-layer-f32-16": lambda dev: _self_layer(dev, F32, 16),
    "self-layer-f32-130": lambda dev: _self_layer(dev, F32, 130),
}
DECODER = {"decoder-fp32": "fp32", "decoder-bf16": "bf16"}      # test_head_projection_gpu._decoder_calls, descriptors included
MFMA_OFF = {"attention-bf16-valu"}

EXPECTED = {
    "attention-f32-masked-dropout": ("fcmf_attn_small_fwd fcmf_attn_small_bwd",
        "bc5b1c28b3ed628501b07148765e094507a58d6c6b0abe7a9866bf5a1c0f53c5"),
    "attention-f32-two-dq-partials": ("fcmf_attn_small_fwd fcmf_attn_small_bwd fcmf_sum_axis",
        "5667ab3e97d1fe452bd385188c4c51bb9bc1d2c76cc6c2931caae6dc56793cd6"),
    "attention-f32-grouped": ("fcmf_attn_small_fwd fcmf_attn_small_bwd_grouped fcmf_sum_axis",
        "8aa4a3b5c942efab16a1668496c94509a476f0763c1e267966a10aa19611d3fa"),
    "attention-f32-group-div-1": ("fcmf_attn_small_fwd fcmf_attn_small_bwd_grouped",
        "74a6a840910b489e24a9111ce7e4fca82b0393bf5aac837c7b795ca628974fa6"),
    "attention-bf16-mfma": ("fcmf_attn_mfma_fwd fcmf_attn_mfma_bwd",
        "8550ed9c0807d128fe0c38d770be1f7d16ce709e00e8ab50959e13adce866405"),
    "attention-bf16-valu": ("fcmf_attn_small_fwd fcmf_attn_small_bwd",
        "1b7cd677e3f40b7842ac8ff4ca8d3c6e239b3c30b3efd91d8078c34480125992"),
    "probs-mfma": ("fcmf_attn_mfma_probs",
        "36d8f360923286456dfede77252e159b06387a51ac02d057625b8e133ad4516b"),
    "probs-mfma-slot-major": ("fcmf_attn_mfma_probs",
        "f9435d48af98c845389ca94e1596c90a84c0637d99297cc6171765ac137a403e"),
    "probs-valu": ("fcmf_attn_probs",
        "75cc7e3d511e2bb37319ff9eeb1bf6cd4bb05e0bd799102501f1dde162bc71f6"),
    "probs-valu-slot-major": ("fcmf_attn_probs",
        "bc8cc5d9addf9993f800e5b1480fa0cd4b0fb4872d8a74dbcbb7441ffe0af5dc"),
    "probs-head-quirk": ("fcmf_attn_probs",
        "5d6c05290bb7c3680217cfa533f3931ca21eb3a4ddf2402f62dde4f5fb1e9ea6"),
    "shared-kv-bf16-300": ("fcmf_attn_mfma_long_fwd fcmf_attn_mfma_long_bwd",
        "609aaf98e2d7be92e77d92fe3a4668cb2190b4b5f3d4a2c6f3216b2ab51cb926"),
    "shared-kv-f32-100": ("fcmf_attn_small_fwd fcmf_attn_small_fwd fcmf_attn_small_bwd fcmf_attn_small_bwd",
        "987ee5ec0f79932c18941a90f451f256bcfc10c7b19bbac1563119e4530eb2a4"),
    "shared-kv-f32-300-dropout": ("""
        fcmf_attn_small_fwd fcmf_attn_small_fwd fcmf_attn_small_fwd fcmf_attn_small_fwd fcmf_attn_small_bwd
        fcmf_sum_axis fcmf_attn_small_bwd fcmf_attn_small_bwd fcmf_sum_axis fcmf_attn_small_bwd
        """, "b927239f97fb4c6f6126d2e0413b1b3dbbacc1d1b359a2a57d6d9b9cb3456812"),
    "self-layer-bf16-16": ("""
        fcmf_cast fcmf_gemm fcmf_attn_mfma_fwd fcmf_attn_mfma_probs fcmf_cast fcmf_cast fcmf_cast fcmf_gemm
        fcmf_add_ln_fwd fcmf_gemm fcmf_gemm fcmf_add_ln_fwd fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd
        fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_add_ln_bwd_workspace
        fcmf_add_ln_bwd fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_attn_mfma_bwd fcmf_colsum fcmf_cast_transpose
        fcmf_gemm fcmf_gemm
        """, "da81a4a8b1de757cf0a9e2b07e06d0bca705d8e495f06ed36e48023be80445c9"),
    "self-layer-f32-16": ("""
        fcmf_gemm fcmf_attn_small_fwd fcmf_attn_probs fcmf_gemm fcmf_add_ln_fwd fcmf_gemm fcmf_gemm fcmf_add_ln_fwd
        fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_add_ln_bwd_workspace
        fcmf_add_ln_bwd fcmf_gemm fcmf_gemm fcmf_attn_small_bwd fcmf_colsum fcmf_gemm fcmf_gemm
        """, "4af95ef29467aab95e24e6b4e180c444ab660c4d253d2be93cf3bea6ffd20c29"),
    "self-layer-f32-130": ("""
        fcmf_gemm fcmf_attn_small_fwd fcmf_attn_probs fcmf_gemm fcmf_add_ln_fwd fcmf_gemm fcmf_gemm fcmf_add_ln_fwd
        fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_add_ln_bwd_workspace
        fcmf_add_ln_bwd fcmf_gemm fcmf_gemm fcmf_attn_small_bwd fcmf_sum_axis fcmf_colsum fcmf_gemm fcmf_gemm
        """, "b6ef178d88f8464c377c8cd82e848cd09ce8bd74fa25dc4cbdc4382a3784424e"),
    "decoder-fp32": ("""
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
        fcmf_embed_scale_bwd
        """, "99ef59bdfd68952edf998b338430857516beb287b45b87d472a8fea484caec74"),
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
        fcmf_cast fcmf_dropout fcmf_embed_scale_bwd
        """, "87d2ed1f1cf02a757fe178564e415bd418822b10e895fd44a897ef2472767bda"),
}


@pytest.mark.parametrize("scene", list(SCENES) + list(DECODER))
def test_attention_call_path(dev, scene, monkeypatch):
    from fcmf_framework import ops
    monkeypatch.setattr(switch, "USE_MFMA_ATTENTION", scene not in MFMA_OFF)     # (raises where the module has no such switch)
    ops.manual_seed(0)
    if scene in DECODER:
        calls = _decoder_calls(dev, DECODER[scene], desc=True)
    else:
        calls = _recorded(lambda: SCENES[scene](dev), desc=True)
    names = " ".join(c[0] for c in calls)
    print("MEASURED", repr(scene), (names, _calls_digest(calls)))
    for c in calls:
        if c[3]:
            print("   ", c)
    exp_names, exp_digest = EXPECTED[scene]
    assert names.split() == exp_names.split()
    assert _calls_digest(calls) == exp_digest
