"""Float64 reference of the attention kernels WITH dropout: a vectorised restatement of fcmf_attn_desc's semantics
(include/fcmf_hip.h) whose dropout mask is rowwise_ref.mask_tensor -- the counter of every attention kernel is the row-major
element index of the probability tensor [G, heads, R, T1+T2] -- and the selector matrices that make a kernel show its dropped
probability matrix.  Plain module: no fixtures, and nothing here calls the library."""
import torch

from rowwise_ref import inv_keep, mask_tensor


def attention_ref(q, k1, v1, k2, v2, mask, bias, heads, group_div, scale, causal, p=0.0, seed=0, keep=None):
    """q [G,R,heads*d]; k1 / v1 [G,T1,heads*d] or None; k2 / v2 [G/group_div,R,T2,heads*d] or None; mask [G,T] additive or None;
    bias [G/group_div,heads,R,T] additive or None (T = T1 + T2, the shared keys first); the causal fill is -1e4 where t > r.
    -> out [G,R,heads*d] (differentiable), P [G,heads,R,T], Pdrop = P * keep * inv_keep(p) with keep the 0/1 tensor
    mask_tensor(seed, (G,heads,R,T), p) unless the caller hands in its own (a mask assembled from several launches)."""
    G, R, HD = q.shape
    d = HD // heads
    dd = lambda t: None if t is None else t.double()
    q, k1, v1, k2, v2, mask, bias = (dd(t) for t in (q, k1, v1, k2, v2, mask, bias))
    qh = q.view(G, R, heads, d).permute(0, 2, 1, 3)                                   # [G,h,R,d]
    shared = lambda t: t.view(G, -1, heads, d).permute(0, 2, 1, 3)                    # [G,h,T1,d]
    private = lambda t: t.repeat_interleave(group_div, 0).view(G, R, -1, heads, d)    # [G,R,T2,h,d]
    s = []
    if k1 is not None:
        s.append(qh @ shared(k1).transpose(-1, -2))
    if k2 is not None:
        s.append(torch.einsum("ghrd,grthd->ghrt", qh, private(k2)))
    s = torch.cat(s, -1) * scale
    T = s.shape[-1]
    if mask is not None:
        s = s + mask[:, None, None, :]
    if bias is not None:
        s = s + bias.repeat_interleave(group_div, 0)
    if causal:
        s = torch.where(torch.arange(T)[None, :] > torch.arange(R)[:, None], torch.full_like(s, -1e4), s)
    P = torch.softmax(s, -1)
    if keep is None:
        keep = mask_tensor(seed, (G, heads, R, T), p) if p > 0 else torch.ones((G, heads, R, T), dtype=torch.float64)
    Pdrop = P * keep * inv_keep(p)
    T1 = 0 if k1 is None else k1.shape[1]
    out = 0
    if k1 is not None:
        out = out + Pdrop[..., :T1] @ shared(v1)
    if k2 is not None:
        out = out + torch.einsum("ghrt,grthd->ghrd", Pdrop[..., T1:], private(v2))
    return out.permute(0, 2, 1, 3).reshape(G, R, HD), P, Pdrop


def selector(T, d, heads, j):
    """[T, heads*d] float32 with S[t, h*d + c] = 1 iff t == j*d + c.  As V it makes out[g, r, h*d + c] = Pdrop[g, h, r, j*d + c]
    (the only term: every other one is a product with an exact zero); as dO over the queries it makes
    dV1[g, t, h*d + c] = Pdrop[g, h, j*d + c, t]."""
    S = torch.zeros(T, heads, d)
    c = torch.arange(min(d, max(0, T - j * d)))
    S[j * d + c, :, c] = 1
    return S.reshape(T, heads * d)


def selector_blocks(T, d):
    """the j of the selectors that cover T columns"""
    return range((T + d - 1) // d)


def heads_first(x, heads):
    """[G, R, heads*d] -> [G, heads, R, d]"""
    G, R, HD = x.shape
    return x.reshape(G, R, heads, HD // heads).permute(0, 2, 1, 3)
