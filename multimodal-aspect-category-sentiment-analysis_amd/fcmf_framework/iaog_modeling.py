"""IAOG seq2seq decoder blocks (reference mm_modeling.py:35-132 `Attention`, :558-666 decoder).

Reference quirks reproduced (SURVEY.md Appendix B + oracle/fcmf_oracle.py):
  * values are the projected KEYS (mm_modeling.py:129);
  * any 2-D `memory_len` means a tril(q_len, k_len) mask filled with -1e4, also on the
    decoder->encoder cross attention (:115-124);
  * the per-head weights are tiled batch-major while the inputs are tiled head-major (:79-85), so
    output slot s of batch element b is projected with head (s*B + b) % n_head;
  * the attention `dropout` constructor argument is never used.
The per-head projections are ONE GEMM against the [n_head*d, E] re-layout of w_kx / w_qx instead
of the reference's B-fold `repeat` + bmm.
"""
import math

import torch
import torch.nn as nn

from . import _hip as H
from . import attn, layers, ops


def _quirk_attn_fwd(qx, kx, heads, causal, head_quirk=1):
    """qx [G, R, heads*d], kx [G, T, heads*d] (row strides arbitrary, unit inner stride) -> out [G, R, heads*d] dense, lse.
    head_quirk 0: the plain pairing, slot s reads head s -- what the reference's pairing is at batch size 1 (decode_step)"""
    G, R, HD = qx.shape
    out = torch.empty((G, R, HD), dtype=qx.dtype, device=qx.device)
    lse = torch.empty((G, heads, R), dtype=torch.float32, device=qx.device)
    a = attn.desc(qx, kx, kx, None, None, None, None, heads, 1, 1.0 / math.sqrt(HD // heads), 0.0, 0, causal, head_quirk)
    attn.forward(a, out, lse, False)
    return out, lse


def _quirk_attn_probs(qx, kx, heads, causal, out=None):
    """the softmax of _quirk_attn_fwd, float32 [heads*G, R, T], index slot*G + g (the reference's `score`, mm_modeling.py:126-132)"""
    return ops.attention_probs(qx, k1=kx, heads=heads, causal=causal, head_quirk=True, slot_major=True, out=out)


def _quirk_attn_bwd(qx, kx, out, lse, dout, heads, causal, dq_out, dk_out):
    """gradients per HEAD written into dq_out / dk_out ([G, R|T, heads*d] views with unit inner stride, any row stride): the
    attention backward produces them per output SLOT, fcmf_head_gather sums the slots that read each head
    (slot s of group g reads head (s*G + g) % heads, mm_modeling.py:79-85)"""
    G, R, HD = qx.shape
    T, d = kx.shape[1], HD // heads
    dk_slot = torch.empty((G, T, HD), dtype=qx.dtype, device=qx.device)
    a = attn.desc(qx, kx, kx, None, None, None, None, heads, 1, 1.0 / math.sqrt(d), 0.0, 0, causal, 1)
    dq_slot = attn.small_backward(a, out, dout.contiguous(), lse, out, dk_slot, None)     # values ARE the keys: dk_slot gets both terms
    L, st = H.lib(), H.stream()
    H.check(L.fcmf_head_gather(H.ptr(dq_slot), H.ptr(dq_out), dq_out.stride(1), G, R, heads, d, H.dt(qx), st), "fcmf_head_gather")
    H.check(L.fcmf_head_gather(H.ptr(dk_slot), H.ptr(dk_out), dk_out.stride(1), G, T, heads, d, H.dt(qx), st), "fcmf_head_gather")


class _QuirkAttentionFn(torch.autograd.Function):
    """attention over natural-head-order projections with the reference's slot->head pairing"""

    @staticmethod
    def forward(ctx, qx, kx, heads, causal):
        qx = qx if qx.stride(2) == 1 else qx.contiguous()
        kx = kx if kx.stride(2) == 1 else kx.contiguous()
        out, lse = _quirk_attn_fwd(qx, kx, heads, causal)
        ctx.save_for_backward(qx, kx, out, lse)
        ctx.cfg = (heads, causal)
        return out

    @staticmethod
    def backward(ctx, dout):
        qx, kx, out, lse = ctx.saved_tensors
        heads, causal = ctx.cfg
        dq = torch.empty(qx.shape, dtype=qx.dtype, device=qx.device)
        dk = torch.empty(kx.shape, dtype=kx.dtype, device=kx.device)
        _quirk_attn_bwd(qx, kx, out, lse, dout, heads, causal, dq, dk)
        return dq, dk, None, None


class _SelfQuirkAttentionFn(torch.autograd.Function):
    """decoder self attention `Attention(X, X, causal)` up to (not including) `proj`, as ONE node: the key and query projections
    of the same input are one GEMM against [w_kx | w_qx] (ops.head_project, N = 2 * n_head * d), the attention reads the two halves
    of its output in place, and the backward gathers the per-slot gradients straight into the halves of one [rows, 2*n_head*d]
    buffer that feeds ONE dX and ONE dW GEMM (the reference: 2 x (repeat + bmm) forward, mm_modeling.py:79-92)."""

    @staticmethod
    def forward(ctx, x, wk, wq, heads, causal, probs=None):
        """probs (optional, float32 [heads*G, T, T]): filled with the attention probabilities from the node's own [kx | qx] buffer"""
        G, T, _ = x.shape
        x2 = ops._rows(x)
        kq = ops.head_project(x2, [wk, wq])
        HD = kq.shape[1] // 2
        kq3 = kq.view(G, T, 2 * HD)
        out, lse = _quirk_attn_fwd(kq3[:, :, HD:], kq3[:, :, :HD], heads, causal)
        if probs is not None:
            _quirk_attn_probs(kq3[:, :, HD:], kq3[:, :, :HD], heads, causal, out=probs)
        ctx.save_for_backward(x2, kq, out, lse, wk, wq)
        ctx.cfg = (heads, causal, x.shape)
        return out

    @staticmethod
    def backward(ctx, dout):
        x2, kq, out, lse, wk, wq = ctx.saved_tensors
        heads, causal, xshape = ctx.cfg
        HD = kq.shape[1] // 2
        kq3 = kq.view(xshape[0], xshape[1], 2 * HD)
        dkq = torch.empty_like(kq)
        d3 = dkq.view(kq3.shape)
        _quirk_attn_bwd(kq3[:, :, HD:], kq3[:, :, :HD], out, lse, dout, heads, causal, d3[:, :, HD:], d3[:, :, :HD])
        dx, dws = ops.head_project_bwd(x2, dkq, [wk, wq], ctx.needs_input_grad[0], ctx.needs_input_grad[1] or ctx.needs_input_grad[2])
        return (None if dx is None else dx.view(xshape), *(dws or (None, None)), None, None, None)


_valid_lens_cache = {}


def _dec_valid_lens(B, T, device):
    """arange(1, T+1).repeat(B, 1) (mm_modeling.py:595-597): only its being 2-D matters (-> the tril rule); built once per shape"""
    key = (B, T, str(device))
    v = _valid_lens_cache.get(key)
    if v is None:
        v = _valid_lens_cache[key] = torch.arange(1, T + 1, device=device).repeat(B, 1)
    return v


class Attention(nn.Module):
    def __init__(self, embed_dim, hidden_dim=None, n_head=1, score_function='scaled_dot_product', dropout=0.1):
        super().__init__()
        if hidden_dim is None:
            hidden_dim = embed_dim // n_head
        if score_function != 'scaled_dot_product':
            # the reference raises RuntimeError('invalid score_function') for unknown names; 'mlp' and
            # 'bi_linear' exist there but are never used on the training path
            raise RuntimeError('invalid score_function' if score_function not in ('mlp', 'bi_linear')
                               else f"score_function '{score_function}' is not on the FCMF path")
        self.embed_dim, self.hidden_dim, self.n_head, self.score_function = embed_dim, hidden_dim, n_head, score_function
        self.w_kx = nn.Parameter(torch.empty(n_head, embed_dim, hidden_dim))
        self.w_qx = nn.Parameter(torch.empty(n_head, embed_dim, hidden_dim))
        self.proj = nn.Linear(n_head * hidden_dim, embed_dim)
        self.register_parameter('weight', None)
        nn.init.xavier_uniform_(self.w_kx)
        nn.init.xavier_uniform_(self.w_qx)
        self.attention_weights = None

    def forward(self, k, q, memory_len=None, kx=None):
        """NOTE the argument order: keys first (reference mm_modeling.py:66).  kx: the already projected keys (IAOGDecoder hoists
        the cross-attention key projections of all its blocks into one GEMM)."""
        same = k is q
        if k.dim() == 2:
            k = k.unsqueeze(1)
        if q.dim() == 2:
            q = q.unsqueeze(1)
        k, q = layers.to_compute(k), layers.to_compute(q)
        causal = False
        if memory_len is not None:
            if isinstance(memory_len, (list, tuple)):
                memory_len = torch.tensor(memory_len, device=k.device)
            if memory_len.dim() == 2:
                causal = True
            else:
                raise NotImplementedError("1-D memory_len (key-length fill mask) is only used by the disabled MDE")
        nh = self.n_head
        want = ops.output_attentions()
        if same and kx is None and k.dim() == 3:
            probs = torch.empty((nh * q.shape[0], q.shape[1], q.shape[1]), dtype=torch.float32, device=q.device) if want else None
            out = _SelfQuirkAttentionFn.apply(q, self.w_kx, self.w_qx, nh, causal, probs)    # one GEMM for [kx | qx]
        else:
            if kx is None:
                kx = ops.head_linear(k, self.w_kx)    # [.., nh*hd], natural head order
            qx = ops.head_linear(q, self.w_qx)
            out = _QuirkAttentionFn.apply(qx, kx, nh, causal)
            probs = _quirk_attn_probs(qx, kx, nh, causal) if want else None
        # the reference's `score` (mm_modeling.py:126-132), [n_head*B, q_len, k_len] with index slot*B + b, when
        # ops.set_output_attentions(True); otherwise None: the fused kernel never materialises it
        self.attention_weights = probs
        return ops.linear(out, self.proj.weight, self.proj.bias), probs


class PositionWiseFFN(nn.Module):
    def __init__(self, ffn_num_hiddens, ffn_num_outputs, hidden_size=None):
        super().__init__()
        from . import mm_modeling as mm
        Hd = hidden_size or mm.HIDDEN_SIZE
        self.dense1 = nn.Linear(Hd, ffn_num_hiddens)
        self.act = mm.ACT2FN[mm.HIDDEN_ACT]
        self.dense2 = nn.Linear(ffn_num_hiddens, ffn_num_outputs)

    def forward(self, x):
        return ops.ffn(layers.to_compute(x), self.dense1.weight, self.dense1.bias, self.dense2.weight, self.dense2.bias)


class AddNorm(nn.Module):
    """LN(dropout(Y) + X) (reference mm_modeling.py:566-573)"""

    def __init__(self, norm_shape, dropout):
        super().__init__()
        from .mm_modeling import FCMFLayerNorm
        self.dropout = nn.Dropout(dropout)
        self.ln = FCMFLayerNorm(norm_shape)

    def forward(self, X, Y):
        return ops.add_layer_norm(layers.to_compute(Y), layers.to_compute(X), self.ln.weight, self.ln.bias,
                                  self.ln.variance_epsilon, self.dropout.p, self.training)


class TransformerDecoderBlock(nn.Module):
    def __init__(self, i, hidden_size=None, num_heads=None):
        super().__init__()
        from . import mm_modeling as mm
        Hd, nh = hidden_size or mm.HIDDEN_SIZE, num_heads or mm.NUM_ATTENTION_HEADS
        p = mm.ATTENTION_PROBS_DROPOUT_PROB
        self.i = i
        self.attention1 = Attention(Hd, Hd // nh, nh, 'scaled_dot_product', p)
        self.addnorm1 = AddNorm(Hd, p)
        self.attention2 = Attention(Hd, Hd // nh, nh, 'scaled_dot_product', p)
        self.addnorm2 = AddNorm(Hd, p)
        self.ffn = PositionWiseFFN(Hd, Hd, Hd)
        self.add_norm3 = AddNorm(Hd, p)

    def forward(self, X, state, enc_attention_mask=None, is_train=True, kx=None):
        """kx: this block's cross-attention keys when the decoder has projected them already (IAOGDecoder.project_encoder)"""
        enc_outputs, enc_valid_lens = state[0], state[1]
        if state[2][self.i] is not None:  # the reference concatenates a cache it never reads (:588-601)
            state[2][self.i] = torch.cat((state[2][self.i], X), dim=1)
        if is_train:
            B, T, _ = X.shape
            dec_valid_lens = _dec_valid_lens(B, T, X.device)
        else:
            dec_valid_lens = None
        X2, _ = self.attention1(X, X, dec_valid_lens)
        Y = self.addnorm1(X, X2)
        cross_mask = enc_attention_mask if enc_attention_mask is not None else enc_valid_lens
        Y2, _ = self.attention2(enc_outputs, Y, cross_mask, kx=kx)
        Z = self.addnorm2(Y, Y2)
        return self.add_norm3(Z, self.ffn(Z)), state


class PositionalEncoding(nn.Module):
    def __init__(self, hidden_size=None):
        super().__init__()
        from . import mm_modeling as mm
        Hd = hidden_size or mm.HIDDEN_SIZE
        self.dropout = nn.Dropout(mm.ATTENTION_PROBS_DROPOUT_PROB)
        P = torch.zeros((1, mm.MAX_POSITION_EMBEDDINGS, Hd))
        X = torch.arange(mm.MAX_POSITION_EMBEDDINGS, dtype=torch.float32).reshape(-1, 1) / torch.pow(
            10000, torch.arange(0, Hd, 2, dtype=torch.float32) / Hd)
        P[:, :, 0::2] = torch.sin(X)
        P[:, :, 1::2] = torch.cos(X)
        self.register_buffer('P', P)

    def forward(self, X):
        pe = self.P[:, :X.size(1), :].to(device=X.device).type_as(X)
        return ops.dropout(X + pe, self.dropout.p, self.training)


class _ScaledEmbedding(torch.autograd.Function):
    """emb[ids] * sqrt(H) (+ P[:, :T]): `self.embedding(X) * math.sqrt(self.num_hiddens)` and PositionalEncoding's addition
    (reference mm_modeling.py:650, :633) in one kernel; the embedding gradient is scattered straight into the parameter's
    (arena) gradient slice -- no [V, H] zeros + index_add_ per step"""

    @staticmethod
    def forward(ctx, ids, weight, pos_table, scale, out_dtype):
        idc = ids.contiguous()
        n, Hd = idc.numel(), weight.shape[1]
        T = ids.shape[-1]
        out = torch.empty(tuple(ids.shape) + (Hd,), dtype=out_dtype, device=weight.device)
        P = None if pos_table is None else pos_table.reshape(-1, Hd)[:T].contiguous()
        H.check(H.lib().fcmf_embed_scale_fwd(H.ptr(idc), H.ptr(weight.detach()), H.ptr(P), H.ptr(out), n, Hd, T, weight.shape[0], float(scale),
                                             H.dt(out), H.stream()), "fcmf_embed_scale_fwd")
        ctx.save_for_backward(idc)
        ctx.scale = scale
        ctx.weight = weight
        return out

    @staticmethod
    def backward(ctx, dy):
        (ids,) = ctx.saved_tensors
        d = dy.contiguous()
        V, Hd = ctx.weight.shape
        dw, _ = ops.grad_dest(ctx.weight, (V, Hd), in_place=False, device=dy.device)      # (never in place: a claimed slice gives a temporary that autograd adds)
        H.check(H.lib().fcmf_embed_scale_bwd(H.ptr(d), H.ptr(ids), H.ptr(dw), ids.numel(), Hd, V, None, float(ctx.scale),
                                             H.dt(d), H.stream()), "fcmf_embed_scale_bwd")      # (ids outside the table made the forward's rows NaN: the loss already says so)
        return None, dw, None, None, None


class IAOGDecoder(nn.Module):
    def __init__(self, vocab_size, hidden_size=None, num_layers=None, num_heads=None):
        super().__init__()
        from . import mm_modeling as mm
        self.num_hiddens = hidden_size or mm.HIDDEN_SIZE
        self.num_blks = num_layers or mm.NUM_HIDDEN_LAYERS
        self.embedding = nn.Embedding(vocab_size, self.num_hiddens)
        self.pos_encoding = PositionalEncoding(self.num_hiddens)
        self.blks = nn.Sequential()
        for i in range(self.num_blks):
            self.blks.add_module('block' + str(i), TransformerDecoderBlock(i, self.num_hiddens, num_heads))
        self.dense = nn.Linear(self.num_hiddens, vocab_size)
        self.dense.weight = self.embedding.weight

    def init_state(self, enc_outputs, enc_valid_lens):
        return [enc_outputs, enc_valid_lens, [None] * self.num_blks]

    def project_encoder(self, enc_outputs):
        """every block's cross-attention keys ( = values, mm_modeling.py:129) of an encoder output, one GEMM for all blocks;
        hand the result to forward(..., hoisted=) when the same encoder output is decoded again and again (decoding.py)"""
        return ops.HeadLinearFn.apply(layers.to_compute(enc_outputs), *[blk.attention2.w_kx for blk in self.blks])

    def hidden_states(self, X, state, enc_attention_mask=None, is_train=True, hoisted=None):
        """the decoder stack up to (not including) the vocabulary projection: [B, Ld, H]"""
        # embedding * sqrt(H) + P in one kernel, then PositionalEncoding's dropout (mm_modeling.py:650, :633)
        X = _ScaledEmbedding.apply(X, self.embedding.weight, self.pos_encoding.P, math.sqrt(self.num_hiddens), ops.compute_dtype())
        X = ops.dropout(X, self.pos_encoding.dropout.p, self.training)
        self._attention_weights = [[None] * len(self.blks) for _ in range(2)]
        # every block's cross attention projects the SAME encoder output with its own w_kx: one GEMM for all of them
        enc = layers.to_compute(state[0])
        if hoisted is None:
            hoisted = self.project_encoder(enc) if enc.dim() == 3 else [None] * len(self.blks)
        for i, blk in enumerate(self.blks):
            X, state = blk(X, state, enc_attention_mask=enc_attention_mask, is_train=is_train, kx=hoisted[i])
            self._attention_weights[0][i] = blk.attention1.attention_weights
            self._attention_weights[1][i] = blk.attention2.attention_weights
        return X

    def forward(self, X, state, enc_attention_mask=None, is_train=True, hoisted=None):
        X = self.hidden_states(X, state, enc_attention_mask, is_train, hoisted)
        return ops.vocab_linear(X, self.dense.weight, self.dense.bias)

    def loss(self, X, state, labels, enc_attention_mask=None, ignore_index=-100, label_smoothing=0.0, rdrop_alpha=0.0, state2=None):
        """CrossEntropyLoss(ignore_index, label_smoothing)(forward(X).permute(0, 2, 1), labels) (run_pretraining_fcmf.py:322-324)
        with the vocabulary projection and the loss fused: the [B, Ld, V] logits are never handed out.
        rdrop_alpha > 0 (R-Drop): the stack runs TWICE at batch B -- not once at 2B, the slot -> head pairing of the blocks
        depends on the batch size -- the second time on state2 (a second encoder pass; `state` again when None), each pass under
        its own dropout seeds, and the two [B, Ld, H] hidden states go stacked into ops.vocab_cross_entropy(rdrop_alpha=)."""
        H1 = self.hidden_states(X, state, enc_attention_mask, True)
        if rdrop_alpha == 0.0:
            return ops.vocab_cross_entropy(H1, self.dense.weight, self.dense.bias, labels, ignore_index, label_smoothing=label_smoothing)
        H2 = self.hidden_states(X, state if state2 is None else state2, enc_attention_mask, True)
        return ops.vocab_cross_entropy(torch.cat((H1, H2), dim=0), self.dense.weight, self.dense.bias, labels, ignore_index,
                                       label_smoothing=label_smoothing, rdrop_alpha=rdrop_alpha)

    def _decode_tail(self, X, k, sampler, constraints=None):
        """the end of a decode step on the rows X [n, H] of the last block: the k best tokens (ops.vocab_topk), or -- `sampler` a dict of
        ops.vocab_sample's arguments ctr (int64 [n] on the device), seed, temperature, top_k, top_p -- one sampled token per row,
        as ([n, 1], [n, 1]) in the same order (log-probabilities, ids); k is not read then.  constraints: ops.logits_constrain's
        keyword arguments as a dict (hist int64 [n, L]: every row's whole sequence), applied to the logits before either tail"""
        if sampler is None:
            return ops.vocab_topk(X, self.dense.weight, self.dense.bias, k, constraints=constraints)
        ids, logp = ops.vocab_sample(X, self.dense.weight, self.dense.bias, constraints=constraints, **sampler)
        return logp.view(-1, 1), ids.view(-1, 1)

    @torch.no_grad()
    def decode_step(self, tokens, sample_idx, enc, keys, k, sampler=None, constraints=None):
        """the is_train=False step of n INDEPENDENT rows in one pass: row i is what forward(tensor([[tokens[i]]]),
        init_state(enc[s:s+1], None), is_train=False, hoisted = keys of sample s) computes for s = sample_idx[i] -- position 0, no
        mask on either attention -- followed by log_softmax + topk(k).  At batch size 1 the reference's slot -> head pairing is the
        plain one (slot s reads head (s*1 + 0) % n_head = s), so the n rows share every GEMM and the cross attention runs with
        head_quirk 0 (the one-key self attention needs no launch); stacking them into an ordinary batch would pair slots with other heads (mm_modeling.py:79-85).
        tokens, sample_idx: int64 [n] on the device; enc [Bs, T, H]; keys = project_encoder(enc), formed here when None.
        -> (log-probabilities float32 [n, k], token ids int32 [n, k]) (ops.vocab_topk); no attention weights are kept.  Dropout is
        off whatever the module's mode: this is the evaluation step.  sampler (see _decode_tail): one sampled token per row instead;
        constraints (see there): the step still sees the last token only, the constraints the row's whole sequence."""
        n = tokens.shape[0]
        if keys is None:
            keys = self.project_encoder(enc)
        X = _ScaledEmbedding.apply(tokens.view(n, 1), self.embedding.weight, self.pos_encoding.P, math.sqrt(self.num_hiddens),
                                   ops.compute_dtype())                              # [n, 1, H]: every row at position 0
        def add_norm(an, x, y):                                                      # AddNorm in eval mode, whatever self.training says
            return ops.add_layer_norm(y, x, an.ln.weight, an.ln.bias, an.ln.variance_epsilon, 0.0, False)

        for blk, kx in zip(self.blks, keys):
            a1, a2 = blk.attention1, blk.attention2
            nh = a1.n_head
            # self attention of a one-token row: ONE key, so its softmax is 1 and, values being the keys (mm_modeling.py:129) and the
            # pairing plain, the output IS the token's kx -- bit for bit what the kernel would return (1 * kx).  No w_qx product and
            # no attention launch for it.
            o = ops.head_project(ops._rows(X), [a1.w_kx]).view(n, 1, -1)
            HD = o.shape[2]
            Y = add_norm(blk.addnorm1, X, ops.linear(o, a1.proj.weight, a1.proj.bias))
            qx = ops.head_project(ops._rows(Y), [a2.w_qx]).view(n, 1, HD)
            o, _ = _quirk_attn_fwd(qx, kx.index_select(0, sample_idx), nh, False, head_quirk=0)      # [n, T, HD] gather: T = 1 + 2*num_imgs rows each
            Z = add_norm(blk.addnorm2, Y, ops.linear(o, a2.proj.weight, a2.proj.bias))
            X = add_norm(blk.add_norm3, Z, blk.ffn(Z))
        return self._decode_tail(X.view(n, -1), k, sampler, constraints)

    def init_cache(self, max_len, rows, device=None):
        """the self-attention key cache of a prefix decode (decode_step_prefix): per block [max_len, rows, n_head*d] in the compute
        dtype -- position-major, so a round's appends are one contiguous slab.  Values are the keys: there is no value cache."""
        if not 1 <= max_len <= min(self.pos_encoding.P.shape[1], ops.DECODE_ATTN_MAX_T):
            raise ValueError(f"prefix decode of {max_len} positions: the positional table has {self.pos_encoding.P.shape[1]} rows, "
                             f"the decode-attention kernel reads at most {ops.DECODE_ATTN_MAX_T} keys")
        device = device or self.embedding.weight.device
        return [torch.empty((max_len, rows, blk.attention1.n_head * blk.attention1.hidden_dim), dtype=ops.compute_dtype(), device=device)
                for blk in self.blks]

    @torch.no_grad()
    def decode_step_prefix(self, tokens, sample_idx, anc, t, cache, enc, keys, k, sampler=None, constraints=None):
        """round t of a decode that sees the whole prefix, n rows in one pass.  Row i is the sequence whose token at position t is
        tokens[i], of sample sample_idx[i], whose earlier positions p < t went through this method as row anc[i, p] of round p with
        the same `cache`.  Its result is row t of forward(tensor([seq]), init_state(enc[s:s+1], <2-D mask>), is_train=True) at batch
        size 1 in eval mode: token p embedded at position p, causal self attention, the tril rule on the cross attention (row t
        scores the encoder keys > t as -1e4, mm_modeling.py:115-124), the plain slot -> head pairing.  Causality makes row p of every
        block's input a function of the tokens <= p, so block i needs of the past only the w_kx projection of its input rows: each
        round appends the n rows' keys at cache[i][t, row] (inside the attention launch) and reads positions < t through `anc` --
        beams share and reorder history by index, no block's keys are ever copied.
        tokens, sample_idx int64 [n]; anc int64 [n, >= t] (any strides); cache = init_cache(max_len > t, rows >= n);
        keys = project_encoder(enc), formed here when None.  -> (log-probabilities float32 [n, k], token ids int32 [n, k]).
        Dropout is off whatever the module's mode, as in decode_step; sampler and constraints as there."""
        n = tokens.shape[0]
        if not (0 <= t < cache[0].shape[0] and n <= cache[0].shape[1]):
            raise ValueError(f"decode_step_prefix: round {t} with {n} rows does not fit a cache of {tuple(cache[0].shape[:2])}")
        if keys is None:
            keys = self.project_encoder(enc)
        X = _ScaledEmbedding.apply(tokens.view(n, 1), self.embedding.weight, self.pos_encoding.P[:, t:t + 1], math.sqrt(self.num_hiddens),
                                   ops.compute_dtype()).view(n, -1)                  # every row at position t

        def add_norm(an, x, y):                                                      # AddNorm in eval mode, whatever self.training says
            return ops.add_layer_norm(y, x, an.ln.weight, an.ln.bias, an.ln.variance_epsilon, 0.0, False)

        for blk, kc, kx in zip(self.blks, cache, keys):
            a1, a2 = blk.attention1, blk.attention2
            nh = a1.n_head
            kq = ops.head_project(X, [a1.w_kx, a1.w_qx])                             # [kx | qx] of the n rows, as _SelfQuirkAttentionFn forms it
            HD = kq.shape[1] // 2
            o = ops.decode_attention(kq[:, HD:], kc, anc, nh, t + 1, t + 1, k_new=kq[:, :HD], append_at=t)
            Y = add_norm(blk.addnorm1, X, ops.linear(o, a1.proj.weight, a1.proj.bias))
            qx = ops.head_project(Y, [a2.w_qx])
            Tk = kx.shape[1]
            o = ops.decode_attention(qx, kx, sample_idx, nh, Tk, min(t + 1, Tk), pos_dim=1)      # the sample's keys in place: no gather
            Z = add_norm(blk.addnorm2, Y, ops.linear(o, a2.proj.weight, a2.proj.bias))
            X = add_norm(blk.add_norm3, Z, blk.ffn(Z))
        return self._decode_tail(X, k, sampler, constraints)

    @property
    def attention_weights(self):
        return self._attention_weights
