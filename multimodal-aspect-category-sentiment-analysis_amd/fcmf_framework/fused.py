"""Layer-level fused autograd Functions of the post-LN transformer layer (HF RobertaLayer,
BertLayer mm_modeling.py:331-342, BertCrossAttentionLayer :344-355).

One autograd node per layer instead of ~10, so that the backward can chain the kernels'
fused epilogues: the residual gradients are added by the dX GEMMs (FCMF_EPI_ADD), the bias gradients
of the two dense layers fall out of the LayerNorm backward (dxsum) and of the gelu' epilogue (colsum),
query/key/value run as ONE GEMM against the [3H,H] weight block the three nn.Linear parameters are
views of, and all weight-gradient buffers of a layer come from a single zero fill.
"""
import math

import torch

from . import _hip as H
from . import attn, ops


# --------------------------------------------------------------------------------------
# q/k/v parameters as views of one [3H, H] block
# --------------------------------------------------------------------------------------
class QKVStorageMixin:
    """nn.Module mixin: keeps self.query/key/value (nn.Linear) weights adjacent in one buffer so that
    the three projections are one GEMM.  State-dict keys, Parameter identities and shapes are unchanged."""

    def _fuse_qkv_storage(self):
        q, k, v = self.query, self.key, self.value
        Hh = q.weight.shape[0]
        W = torch.empty((3 * Hh, q.weight.shape[1]), dtype=q.weight.dtype, device=q.weight.device)
        b = torch.empty((3 * Hh,), dtype=q.bias.dtype, device=q.bias.device)
        for i, lin in enumerate((q, k, v)):
            W[i * Hh:(i + 1) * Hh].copy_(lin.weight.data)
            b[i * Hh:(i + 1) * Hh].copy_(lin.bias.data)
            lin.weight.data = W[i * Hh:(i + 1) * Hh]
            lin.bias.data = b[i * Hh:(i + 1) * Hh]
        self._qkv_w, self._qkv_b = W, b

    def _apply(self, fn, *a, **kw):
        out = super()._apply(fn, *a, **kw)
        self._fuse_qkv_storage()      # .to()/.cuda()/.float() re-allocate every parameter separately
        return out

    def qkv_params(self):
        """(W [3H,H], b [3H]) if the storage is still fused, else None"""
        q, k, v = self.query.weight, self.key.weight, self.value.weight
        n = q.numel() * q.element_size()
        if (k.data_ptr() == q.data_ptr() + n and v.data_ptr() == k.data_ptr() + n and q.is_contiguous()
                and self.key.bias.data_ptr() == self.query.bias.data_ptr() + self.query.bias.numel() * 4
                and self.value.bias.data_ptr() == self.key.bias.data_ptr() + self.key.bias.numel() * 4):
            return self._qkv_w, self._qkv_b
        return None


def _fused_weight(ws, dtype):
    """[sum(N_i), K] compute-dtype weight for a list of adjacent (or not) float32 parameters"""
    w0 = ws[0]
    n = w0.numel() * 4
    adjacent = all(ws[i + 1].data_ptr() == ws[i].data_ptr() + n for i in range(len(ws) - 1)) and w0.is_contiguous()
    if adjacent:
        flat = torch.as_strided(w0.detach(), (len(ws) * w0.shape[0],) + tuple(w0.shape[1:]),
                                (w0.stride(0),) + tuple(w0.stride()[1:])) if w0.dim() == 2 else \
            torch.as_strided(w0.detach(), (len(ws) * w0.shape[0],), (1,))
        if dtype == torch.float32:
            return flat
        # `flat` is a temporary: the shadow belongs to w0 (or to the packed parameter w0 is a view of), whose version
        # counter it shares; FusedAdamW marks every shadow it did not refresh itself as stale
        return ops.shadows.get(flat, owner=w0)
    cat = torch.cat([w.detach() for w in ws], 0)
    return cat if dtype == torch.float32 else ops.cast(cat, dtype)


# --------------------------------------------------------------------------------------
# self-attention over a fused [G,T,3H] q|k|v buffer
# --------------------------------------------------------------------------------------
def _self_desc(qkv, mask, G, T, Hd, heads, p, seed):
    """attn.desc over the three column blocks of the [G*T, 3H] buffer, read in place (row stride 3H)"""
    q, k, v = qkv.view(G, T, 3, Hd).unbind(2)
    return attn.desc(q, k, v, None, None, mask, None, heads, 1, 1.0 / math.sqrt(Hd // heads), p, seed, False, 0)


def self_attention_fwd(qkv, mask, G, T, Hd, heads, p, seed):
    out = torch.empty((G * T, Hd), dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty((G, heads, T), dtype=torch.float32, device=qkv.device)
    a = _self_desc(qkv, mask, G, T, Hd, heads, p, seed)
    attn.forward(a, out, lse, attn.mfma_eligible(a))
    return out, lse


def self_attention_probs(qkv, mask, G, T, Hd, heads, probs):
    """fill probs (float32 [G, heads, T, T], contiguous) with the pre-dropout softmax of self_attention_fwd, read from the same
    [G*T, 3H] q|k|v buffer in place, on the kernel family the forward chose"""
    if tuple(probs.shape) != (G, heads, T, T) or probs.dtype != torch.float32 or not probs.is_contiguous():
        raise H.HipLibraryError(f"attention probabilities: need a contiguous float32 {(G, heads, T, T)} tensor")
    a = _self_desc(qkv, mask, G, T, Hd, heads, 0.0, 0)
    attn.probs(a, probs, heads * T * T, T * T, attn.mfma_eligible(a))


def self_attention_bwd(qkv, mask, out, lse, dout, G, T, Hd, heads, p, seed, bias_grad=None):
    """-> dqkv [G*T, 3H].  bias_grad (float32 [3H], accumulated into): the column sums of dqkv = the gradient of the fused
    q|k|v bias; the MFMA kernel produces them per sequence from its f32 accumulators (no extra pass over dqkv)."""
    a = _self_desc(qkv, mask, G, T, Hd, heads, p, seed)
    if attn.mfma_eligible(a):
        dqkv = torch.empty_like(qkv)
        db, col = dqkv.data_ptr(), Hd * qkv.element_size()
        part = None if bias_grad is None else torch.empty((G, 3 * Hd), dtype=torch.float32, device=qkv.device)
        attn.mfma_backward(a, out, dout, lse, db, db + col, db + 2 * col, part)
        rows = part
    else:
        dk, dv = (torch.empty((G, T, Hd), dtype=qkv.dtype, device=qkv.device) for _ in range(2))
        dq = attn.small_backward(a, out, dout, lse, dk, dk, dv)                  # (like_q = dk: dq has the shape and dtype of dk)
        rows = dqkv = torch.cat((dq, dk, dv), dim=-1).view(G * T, 3 * Hd)
    if bias_grad is not None:
        H.check(H.lib().fcmf_colsum(H.ptr(rows), H.ptr(bias_grad), rows.shape[0], 3 * Hd, 3 * Hd, H.dt(rows), 1, H.stream()),
                "fcmf_colsum")
    return dqkv


# --------------------------------------------------------------------------------------
# shared tail: out-proj -> add+LN -> FFN -> add+LN
# --------------------------------------------------------------------------------------
def _want_q(rows, Hd, dtype, bf16_consumer=False):
    """the fp8 mode quantises the LayerNorm output inside the LayerNorm kernel when an fp8 GEMM will consume it
    (bf16_consumer: the GEMM that reads it carries the feed-forward dropout and stays bf16 -- nothing would read the e4m3 copy)"""
    return ops.fp8_enabled() and dtype == torch.bfloat16 and Hd % 128 == 0 and rows >= 256 and not bf16_consumer


def _post_fwd(c, res, res_ld, wo, bo, g1, be1, w1, b1, w2, b2, g2, be2, eps, p, seeds, p_f=0.0, seed_f=0):
    """c [M,H] attention context; res rows at stride res_ld.  Returns y and the tensors the backward needs.
    p_f > 0: nn.TransformerEncoderLayer's dropout between the feed-forward's gelu and its second Linear, applied by the first
    GEMM's epilogue (mask over [M, I] from seed_f); the saved `a` is then the dropped activation."""
    dt = c.dtype
    M, Hd = c.shape
    I = w1.shape[0]
    co, c1, c2 = ops.as_compute(wo, dt), ops.as_compute(w1, dt), ops.as_compute(w2, dt)
    h = torch.empty((M, Hd), dtype=dt, device=c.device)
    ops.gemm_nt(c, wo, co, h, M, Hd, Hd, Hd, bias=bo.detach())
    h1, m1, r1, h1q = ops.ln_fwd(h, res, res_ld, g1, be1, eps, p, seeds[0], h, quant=_want_q(M, Hd, dt, p_f > 0))     # (the pre-LN sum z1 overwrites h)
    u = torch.empty((M, I), dtype=dt, device=c.device)
    a = torch.empty((M, I), dtype=dt, device=c.device)
    if p_f > 0:
        ops.gemm_nt(h1, w1, c1, a, M, I, Hd, Hd, bias=b1.detach(), aux=u, epi=H.EPI_GELU_DROP, drop=(p_f, seed_f))
    else:
        ops.gemm_nt(h1, w1, c1, a, M, I, Hd, Hd, bias=b1.detach(), aux=u, epi=H.EPI_GELU, xq=h1q)
    f = torch.empty((M, Hd), dtype=dt, device=c.device)
    ops.gemm_nt(a, w2, c2, f, M, Hd, I, I, bias=b2.detach())
    y, m2, r2, _ = ops.ln_fwd(f, h1, Hd, g2, be2, eps, p, seeds[1], f)                                       # (z2 overwrites f)
    return y, (h, m1, r1, h1, u, a, f, m2, r2)


def _post_bwd(dy, c, saved, wo, w1, w2, g1, g2, p, seeds, G, p_f=0.0, seed_f=0):
    """-> dc [M,H], dres (= dz1) [M,H]; weight / bias / LN gradients are accumulated into the views in G.
    p_f > 0: the gelu' GEMM regenerates the forward's feed-forward mask (both write [M, I]) and its column sums are masked"""
    z1, m1, r1, h1, u, a, z2, m2, r2 = saved
    dt = c.dtype
    M, Hd = c.shape
    I = w1.shape[0]
    co, c1, c2 = ops.as_compute(wo, dt), ops.as_compute(w1, dt), ops.as_compute(w2, dt)
    dz2, df, dfq = ops.ln_bwd(dy, z2, g2, m2, r2, p, seeds[1], G["g2"], G["be2"], G["b2"], quant=_want_q(M, Hd, dt, p_f > 0))
    du = torch.empty((M, I), dtype=dt, device=c.device)
    if p_f > 0:
        ops.gemm_dx(df, w2, c2, du, M, I, Hd, aux=u, epi=H.EPI_DGELU_DROP, colsum=G["b1"], drop=(p_f, seed_f))      # (df W2) * gelu'(u) * mask; db1
    else:
        ops.gemm_dx(df, w2, c2, du, M, I, Hd, aux=u, epi=H.EPI_DGELU, colsum=G["b1"], dyq=dfq)      # (df W2) * gelu'(u); db1
    ops.gemm(df, a, G["w2"], Hd, I, M, Hd, I, I, 1, 1, acc=True)                   # dW2 = df^T a
    dh1 = torch.empty((M, Hd), dtype=dt, device=c.device)
    ops.gemm_dx(du, w1, c1, dh1, M, Hd, I, aux=dz2, epi=H.EPI_ADD)                             # du W1 + dz2 (residual)
    ops.gemm(du, h1, G["w1"], I, Hd, M, I, Hd, Hd, 1, 1, acc=True)                # dW1 = du^T h1
    dz1, dh, dhq = ops.ln_bwd(dh1, z1, g1, m1, r1, p, seeds[0], G["g1"], G["be1"], G["bo"], quant=_want_q(M, Hd, dt))
    dc = torch.empty((M, Hd), dtype=dt, device=c.device)
    ops.gemm_dx(dh, wo, co, dc, M, Hd, Hd, dyq=dhq)
    ops.gemm(dh, c, G["wo"], Hd, Hd, M, Hd, Hd, Hd, 1, 1, acc=True)
    return dc, dz1


def _layer_grads(device, Hd, I, params):
    """all float32 gradient buffers of one layer.  params: name -> Parameter (or the [q, k, v] list for "wqkv" / "bqkv").
    -> (G: name -> buffer to accumulate into, R: name -> what to hand autograd for it), both from ops.grad_dest: the
    parameters' slices of the step's flat gradient arena when one is active (dp.GradArena: zeroed once per step); the names that
    are not there share ONE zero fill."""
    shapes = dict(wqkv=(3 * Hd, Hd), bqkv=(3 * Hd,), wo=(Hd, Hd), w1=(I, Hd), w2=(Hd, I), bo=(Hd,), b1=(I,), b2=(Hd,),
                  g1=(Hd,), be1=(Hd,), g2=(Hd,), be2=(Hd,))
    G, R = {}, {}
    for n, q in params.items():
        G[n], R[n] = ops.grad_dest(q, shapes[n], temp=False)
    rest = [n for n in params if G[n] is None]
    if rest:
        flat = torch.zeros(sum(math.prod(shapes[n]) for n in rest), dtype=torch.float32, device=device)
        off = 0
        for n in rest:
            k = math.prod(shapes[n])
            G[n] = R[n] = flat[off:off + k].view(shapes[n])
            off += k
    return G, R


def _split3(g, Hd):
    """the fused q|k|v gradient [3H, ...] as the three parameters' gradients (None: accumulated in place)"""
    return (None, None, None) if g is None else (g[:Hd], g[Hd:2 * Hd], g[2 * Hd:])


class PostAttentionFn(torch.autograd.Function):
    """attention.output.dense -> dropout -> +res -> LN -> FFN(GELU) -> dropout -> +res -> LN"""

    @staticmethod
    def forward(ctx, c, res, wo, bo, g1, be1, w1, b1, w2, b2, g2, be2, eps, p, seed0, seed1):
        c2 = ops._rows(c).contiguous()
        r2 = ops._rows(res)
        if r2.stride(1) != 1:
            r2 = r2.contiguous()
        y, saved = _post_fwd(c2, r2, ops._ld(r2), wo, bo, g1, be1, w1, b1, w2, b2, g2, be2, eps, p, (seed0, seed1))
        ctx.save_for_backward(c2, wo, w1, w2, g1, g2, bo, be1, b1, b2, be2, *saved)
        ctx.cfg = (p, seed0, seed1, c.shape, res.shape)
        return y.view(c.shape)

    @staticmethod
    def backward(ctx, dy):
        c2, wo, w1, w2, g1, g2, bo, be1, b1, b2, be2, *saved = ctx.saved_tensors
        p, s0, s1, cshape, rshape = ctx.cfg
        G, R = _layer_grads(c2.device, c2.shape[1], w1.shape[0],
                            dict(wo=wo, w1=w1, w2=w2, bo=bo, b1=b1, b2=b2, g1=g1, be1=be1, g2=g2, be2=be2))
        dc, dres = _post_bwd(dy.reshape(c2.shape).contiguous(), c2, saved, wo, w1, w2, g1, g2, p, (s0, s1), G)
        return (dc.view(cshape), dres.view(rshape), R["wo"], R["bo"], R["g1"], R["be1"], R["w1"], R["b1"], R["w2"], R["b2"],
                R["g2"], R["be2"], None, None, None, None)


class SelfLayerFn(torch.autograd.Function):
    """the whole self-attention layer: fused QKV GEMM -> attention -> PostAttention tail.
    probs (optional, float32 [G, heads, T, T]): filled with the layer's pre-dropout attention probabilities from the node's own
    q|k|v buffer (one more launch; nothing is saved for it and the backward does not know about it).
    p_f, seed_f: the feed-forward dropout of nn.TransformerEncoderLayer (see _post_fwd); 0 = HF's RobertaLayer, which has none."""

    @staticmethod
    def forward(ctx, x, mask, wq, bq, wk, bk, wv, bv, wo, bo, g1, be1, w1, b1, w2, b2, g2, be2, heads, eps, p_h, p_a,
                seed_a, seed0, seed1, probs=None, p_f=0.0, seed_f=0):
        G_, T, Hd = x.shape
        M = G_ * T
        x2 = x.reshape(M, Hd)
        if not x2.is_contiguous():
            x2 = x2.contiguous()
        dt = x2.dtype
        wqkv = _fused_weight([wq, wk, wv], dt)
        bqkv = _fused_weight([bq, bk, bv], torch.float32)
        qkv = torch.empty((M, 3 * Hd), dtype=dt, device=x.device)
        wm = _fused_weight([wq, wk, wv], torch.float32)             # the [3H, H] float32 view when the storage is fused
        ops.gemm_nt(x2, wm if wm.data_ptr() == wq.data_ptr() else None, wqkv, qkv, M, 3 * Hd, Hd, Hd, bias=bqkv, owner=wq)
        mk = None if mask is None else mask.contiguous().float()
        c, lse = self_attention_fwd(qkv, mk, G_, T, Hd, heads, p_a, seed_a)
        if probs is not None:
            self_attention_probs(qkv, mk, G_, T, Hd, heads, probs)
        y, saved = _post_fwd(c, x2, Hd, wo, bo, g1, be1, w1, b1, w2, b2, g2, be2, eps, p_h, (seed0, seed1), p_f, seed_f)
        ctx.save_for_backward(x2, mk, qkv, c, lse, wq, wk, wv, wo, w1, w2, g1, g2, bq, bk, bv, bo, be1, b1, b2, be2, *saved)
        ctx.cfg = (heads, p_h, p_a, seed_a, seed0, seed1, x.shape, p_f, seed_f)
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        x2, mk, qkv, c, lse, wq, wk, wv, wo, w1, w2, g1, g2, bq, bk, bv, bo, be1, b1, b2, be2, *saved = ctx.saved_tensors
        heads, p_h, p_a, seed_a, s0, s1, xshape, p_f, seed_f = ctx.cfg
        G_, T, Hd = xshape
        M, dt = G_ * T, x2.dtype
        G, R = _layer_grads(x2.device, Hd, w1.shape[0],
                            dict(wqkv=[wq, wk, wv], bqkv=[bq, bk, bv], wo=wo, w1=w1, w2=w2, bo=bo, b1=b1, b2=b2, g1=g1, be1=be1,
                                 g2=g2, be2=be2))
        dc, dz1 = _post_bwd(dy.reshape(M, Hd).contiguous(), c, saved, wo, w1, w2, g1, g2, p_h, (s0, s1), G, p_f, seed_f)
        dqkv = self_attention_bwd(qkv, mk, c, lse, dc, G_, T, Hd, heads, p_a, seed_a, bias_grad=G["bqkv"])
        wqkv = _fused_weight([wq, wk, wv], dt)
        dx = torch.empty((M, Hd), dtype=dt, device=x2.device)
        wm = _fused_weight([wq, wk, wv], torch.float32)
        ops.gemm_dx(dqkv, wm if wm.data_ptr() == wq.data_ptr() else None, wqkv, dx, M, Hd, 3 * Hd, aux=dz1, epi=H.EPI_ADD, owner=wq)   # + residual gradient
        ops.gemm(dqkv, x2, G["wqkv"], 3 * Hd, Hd, M, 3 * Hd, Hd, Hd, 1, 1, acc=True)
        Ws, bs = _split3(R["wqkv"], Hd), _split3(R["bqkv"], Hd)
        return (dx.view(xshape), None, Ws[0], bs[0], Ws[1], bs[1], Ws[2], bs[2], R["wo"], R["bo"],
                R["g1"], R["be1"], R["w1"], R["b1"], R["w2"], R["b2"], R["g2"], R["be2"],
                None, None, None, None, None, None, None, None, None, None)
