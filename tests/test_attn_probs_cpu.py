"""CPU-side checks of the attention-probability outputs: the golden fixture against a float64 restatement of the reference
Attention's slot -> head rule, the opt-in switch, and the two new C-ABI symbols."""
import ctypes
import math
import os
import re

import numpy as np
import torch

from conftest import GOLD, PKG, ROOT

NH, E, HID = 4, 32, 8


def _score_and_output(g, k, q, causal):
    """float64 restatement of mm_modeling.py:66-132: inputs tiled head-major (row n = slot n // B of batch element n % B), weights
    tiled batch-major (row n uses head n % n_head), i.e. slot s of element b is projected with head (s*B + b) % n_head; values are
    the projected keys; a 2-D memory_len fills -1e4 above the diagonal"""
    wk, wq = (torch.from_numpy(g[n]).double() for n in ("w_kx", "w_qx"))
    pw, pb = torch.from_numpy(g["proj_w"]).double(), torch.from_numpy(g["proj_b"]).double()
    k, q = torch.from_numpy(k).double(), torch.from_numpy(q).double()
    B, R, T = q.shape[0], q.shape[1], k.shape[1]
    score = torch.empty(NH * B, R, T, dtype=torch.float64)
    out = torch.empty(B, R, NH * HID, dtype=torch.float64)
    for s in range(NH):
        for b in range(B):
            h = (s * B + b) % NH
            kx, qx = k[b] @ wk[h], q[b] @ wq[h]
            sc = qx @ kx.t() / math.sqrt(HID)
            if causal:
                sc = torch.where(torch.arange(T)[None, :] > torch.arange(R)[:, None], torch.full_like(sc, -1e4), sc)
            p = torch.softmax(sc, -1)
            score[s * B + b] = p
            out[b, :, s * HID:(s + 1) * HID] = p @ kx
    return score, out @ pw.t() + pb


def test_fixture_agrees_with_the_slot_to_head_rule():
    g = np.load(os.path.join(GOLD, "iaog_attention_weights.npz"))
    assert g["w_kx"].shape == (NH, E, HID) and g["w_qx"].shape == (NH, E, HID)
    n = 0
    for B in (1, 2, 3):
        for kind in ("self", "cross", "cross_tril"):
            k, q = g[f"B{B}_{kind}_k"], g[f"B{B}_{kind}_q"]
            assert k.dtype == np.float32 and k.shape == (B, 5 if kind == "self" else 7, E) and q.shape == (B, 5, E)
            if kind == "self":
                assert np.array_equal(k, q)
            score, out = _score_and_output(g, k, q, causal=kind != "cross")
            for name, ref in (("score", score), ("output", out)):
                got = torch.from_numpy(g[f"B{B}_{kind}_{name}"]).double()
                assert got.shape == ref.shape
                err = ((got - ref).abs().max() / ref.abs().max()).item()
                assert err < 1e-5, (B, kind, name, err)      # the reference ran in float32
            n += 1
    assert n == 9
    assert os.path.getsize(os.path.join(GOLD, "iaog_attention_weights.npz")) < 100 * 1024


def test_output_attentions_switch_round_trips():
    from fcmf_framework import ops
    assert ops.output_attentions() is False      # off by default: the training step never pays for the output
    try:
        ops.set_output_attentions(True)
        assert ops.output_attentions() is True
        ops.set_output_attentions(0)
        assert ops.output_attentions() is False
    finally:
        ops.set_output_attentions(False)


def test_new_symbols_declared_exported_and_bound():
    from fcmf_framework import _hip
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fcmf_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(os.path.join(PKG, "fcmf_framework", "libfcmf_hip.so"))
    for name, nargs in (("fcmf_attn_probs", 5), ("fcmf_attn_mfma_probs", 14)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", src)
        assert m, f"{name} is not declared in include/fcmf_hip.h"
        assert len(m.group(1).split(",")) == nargs == len(_hip.SIGNATURES[name])
        assert hasattr(lib, name), f"{name} is not exported"
        assert getattr(_hip.lib(), name).restype is ctypes.c_int
    assert _hip.lib().fcmf_abi_version() == 4      # additive change


def test_module_surface_accepts_the_probability_arguments():
    """the optional arguments exist with `off` defaults (no GPU needed to see the surface)"""
    import inspect
    from fcmf_framework import fused, iaog_modeling, layers, ops, roberta
    sig = inspect.signature(ops.attention_probs)
    assert [p for p in sig.parameters][:3] == ["q", "k1", "k2"] and sig.parameters["slot_major"].default is False
    assert inspect.signature(layers.transformer_layer).parameters["probs"].default is None
    assert inspect.signature(fused.SelfLayerFn.forward).parameters["probs"].default is None
    assert inspect.signature(roberta.RobertaModel.forward).parameters["output_attentions"].default is False
    assert iaog_modeling.Attention(32, 8, 4).attention_weights is None
