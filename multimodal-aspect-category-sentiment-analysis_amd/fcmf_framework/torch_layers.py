"""torch.nn.MultiheadAttention / TransformerEncoderLayer / TransformerEncoder with torch's parameter names, on the HIP path.

The comparison baselines of the paper (mRoBERTa, TomBERT) are written with these three torch modules; their checkpoints
therefore carry torch's state-dict keys (`in_proj_weight`, `out_proj.*`, `self_attn.*`, `linear1`, `linear2`, `norm1`,
`norm2`, `layers.N.*`).  The modules here keep those keys and shapes and run on what the library has: the packed
`in_proj_weight` [3E, E] is the fused q|k|v block that fused.SelfLayerFn multiplies in one GEMM, cross-attention goes
through ops.shared_kv_attention (any number of keys, one key/value set per `kv_share` consecutive query groups), and a
boolean key-padding mask becomes the hard additive mask (finfo(float32).min: probability exactly 0).
`MultiheadAttention.forward(need_weights=True)` also returns the attention weights, averaged over the heads or per head
(ops.shared_kv_attention_probs: recomputed from the projected q and k by their own kernel).  Two deviations from torch, as
for the text encoder's `output_attentions`: in train() mode they are the softmax BEFORE dropout, and a row without a live
key is uniform where torch gives NaN.  `need_weights` defaults to False here (torch: True).

Only what the baselines use is built -- batch_first=True, post-norm, gelu, biases, no attn_mask; anything else raises
NotImplementedError.  Under training torch drops activations once more between the feed-forward's gelu and its second
Linear, which HF's RobertaLayer (the fused layer's origin) does not: `ops.set_ffn_dropout(True)` (run_baselines.py
--ffn_dropout) turns that dropout on, inside the epilogues of the two feed-forward GEMMs (fcmf_gemm_drop), and the
train()-mode step is then the function torch trains.  It is off by default (a step then regularises slightly less, and is
launch for launch what it was before the switch existed); in eval() mode the two are the same function either way.
"""
import copy

import torch
import torch.nn as nn

from . import ops

_HARD = torch.finfo(torch.float32).min


def padding_to_additive(key_padding_mask):
    """bool [G, T], True = ignore this key -> float32 additive mask [G, T]; a floating mask is additive already, as in
    torch (None stays None)"""
    if key_padding_mask is None or key_padding_mask.dtype.is_floating_point:
        return key_padding_mask
    return key_padding_mask.to(torch.float32) * _HARD


class MultiheadAttention(nn.Module):
    """nn.MultiheadAttention(embed_dim, num_heads, dropout, batch_first=True).  `kv_share` (constructor default, or per call):
    `kv_share` consecutive rows of `query`'s batch read ONE row of `key` / `value`'s batch -- the aspect prompts of a review
    and its visual tokens -- so key / value are projected and stored once per review."""

    def __init__(self, embed_dim, num_heads, dropout=0.0, bias=True, add_bias_kv=False, add_zero_attn=False, kdim=None,
                 vdim=None, batch_first=False, kv_share=1):
        super().__init__()
        if (not batch_first or not bias or add_bias_kv or add_zero_attn or kdim not in (None, embed_dim)
                or vdim not in (None, embed_dim)):
            raise NotImplementedError("MultiheadAttention: only batch_first=True with biases and kdim = vdim = embed_dim")
        if embed_dim % num_heads:
            raise ValueError("embed_dim must be divisible by num_heads")
        self.embed_dim, self.num_heads, self.dropout, self.batch_first, self.kv_share = embed_dim, num_heads, dropout, True, kv_share
        self.head_dim = embed_dim // num_heads
        self.in_proj_weight = nn.Parameter(torch.empty(3 * embed_dim, embed_dim))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * embed_dim))
        self.out_proj = nn.Linear(embed_dim, embed_dim)
        nn.init.xavier_uniform_(self.in_proj_weight)
        nn.init.zeros_(self.out_proj.bias)

    def qkv_params(self):
        """(Wq, bq, Wk, bk, Wv, bv): views of the packed parameters, adjacent in memory (one GEMM in the fused layer)"""
        E, W, b = self.embed_dim, self.in_proj_weight, self.in_proj_bias
        return W[:E], b[:E], W[E:2 * E], b[E:2 * E], W[2 * E:], b[2 * E:]

    def _project(self, query, key, value, key_padding_mask, kv_share):
        """-> q, k, v, additive mask [G, Tk] or None, the sharing factor"""
        share = self.kv_share if kv_share is None else kv_share
        wq, bq, wk, bk, wv, bv = self.qkv_params()
        q = ops.linear(query, wq, bq)
        k = ops.linear(key, wk, bk)
        v = ops.linear(value, wv, bv)
        mask = padding_to_additive(key_padding_mask)
        if mask is not None and mask.shape[0] != q.shape[0]:
            mask = mask.repeat_interleave(share, 0)          # given per key set
        return q, k, v, mask, share

    def _attend(self, q, k, v, mask, share):
        return ops.shared_kv_attention(q, k, v, mask=mask, heads=self.num_heads, kv_share=share, p=self.dropout,
                                       training=self.training)

    def context(self, query, key, value, key_padding_mask=None, kv_share=None):
        """the heads' outputs before out_proj: [G, Tq, E]"""
        return self._attend(*self._project(query, key, value, key_padding_mask, kv_share))

    def forward(self, query, key, value, key_padding_mask=None, need_weights=False, attn_mask=None, average_attn_weights=True,
                kv_share=None):
        """-> (output, weights).  weights is None unless need_weights (torch's default is True; here it is False, the
        baselines throw the weights away): then the float32 softmax of the q and k projected for the output (no second
        projection), [G, Tq, Tk] averaged over the heads or [G, heads, Tq, Tk] -- before dropout also in train() mode, and
        uniform where torch gives NaN (a row without a live key); detached."""
        if attn_mask is not None:
            raise NotImplementedError("MultiheadAttention: attn_mask is not built")
        q, k, v, mask, share = self._project(query, key, value, key_padding_mask, kv_share)
        out = ops.linear(self._attend(q, k, v, mask, share), self.out_proj.weight, self.out_proj.bias)
        if not need_weights:
            return out, None
        return out, ops.shared_kv_attention_probs(q, k, mask=mask, heads=self.num_heads, kv_share=share,
                                                  average_heads=average_attn_weights)


class TransformerEncoderLayer(nn.Module):
    """nn.TransformerEncoderLayer(d_model, nhead, dim_feedforward, dropout, activation="gelu", batch_first=True), post-norm:
    one fused autograd node (fused.SelfLayerFn)"""

    def __init__(self, d_model, nhead, dim_feedforward=2048, dropout=0.1, activation="relu", layer_norm_eps=1e-5,
                 batch_first=False, norm_first=False, bias=True):
        super().__init__()
        if activation != "gelu" or not batch_first or norm_first or not bias:
            raise NotImplementedError('TransformerEncoderLayer: only activation="gelu", batch_first=True, post-norm, with biases')
        self.self_attn = MultiheadAttention(d_model, nhead, dropout=dropout, batch_first=True)
        self.linear1 = nn.Linear(d_model, dim_feedforward)
        self.linear2 = nn.Linear(dim_feedforward, d_model)
        self.norm1 = nn.LayerNorm(d_model, eps=layer_norm_eps)
        self.norm2 = nn.LayerNorm(d_model, eps=layer_norm_eps)
        self.p = float(dropout)

    def forward(self, src, src_mask=None, src_key_padding_mask=None):
        if src_mask is not None:
            raise NotImplementedError("TransformerEncoderLayer: src_mask is not built")
        from .fused import SelfLayerFn
        sa = self.self_attn
        p = self.p if self.training else 0.0
        seed_a = ops.next_seed() if p > 0 else 0
        s0, s1 = (ops.next_seed(), ops.next_seed()) if p > 0 else (0, 0)
        # feed-forward dropout (ops.set_ffn_dropout): probs=None, p_f, seed_f -- the seed drawn last, so the other three masks of
        # the step are those of a run with the switch off; off, the call is argument for argument what it was
        ffn = (None, p, ops.next_seed()) if p > 0 and ops.ffn_dropout() else ()
        return SelfLayerFn.apply(src, padding_to_additive(src_key_padding_mask), *sa.qkv_params(), sa.out_proj.weight,
                                 sa.out_proj.bias, self.norm1.weight, self.norm1.bias, self.linear1.weight, self.linear1.bias,
                                 self.linear2.weight, self.linear2.bias, self.norm2.weight, self.norm2.bias, sa.num_heads,
                                 float(self.norm1.eps), p, p, seed_a, s0, s1, *ffn)


class TransformerEncoder(nn.Module):
    """nn.TransformerEncoder(encoder_layer, num_layers): `layers.N.*`; every layer starts from a copy of `encoder_layer`'s
    parameters, as torch's does"""

    def __init__(self, encoder_layer, num_layers, norm=None):
        super().__init__()
        if norm is not None:
            raise NotImplementedError("TransformerEncoder: a final norm is not built")
        self.layers = nn.ModuleList([copy.deepcopy(encoder_layer) for _ in range(num_layers)])
        self.num_layers = num_layers

    def forward(self, src, mask=None, src_key_padding_mask=None):
        if mask is not None:
            raise NotImplementedError("TransformerEncoder: mask is not built")
        add = padding_to_additive(src_key_padding_mask)      # (converted once for all layers)
        x = src
        for layer in self.layers:
            x = layer(x, src_key_padding_mask=add)
        return x

