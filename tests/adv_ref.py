"""float64 statement of the FGM adversary on the token embeddings (include/fcmf_hip.h: fcmf_adv_scale, fcmf_embed_ln_adv_fwd;
ops.EmbeddingAdversary), beside tests/rowwise_ref.py whose LayerNorm it reuses.

    scale[s] = epsilon / || g[s, t, :] over the tokens t with ids[s, t] != pad ||_2        (0 where that norm is 0)
    z[s, t]  = ((word[ids] + type[tt]) + pos[pos]) + scale[s] * g[s, t]   at the tokens that are not pad, the plain sum at pads
    y        = LayerNorm(z) * gamma + beta, then the dropout mask

Rows of g at pad tokens are never read: they may hold NaN."""
import torch

import rowwise_ref as R


def live(ids, pad):
    """bool [nseq, S]: the tokens that are not pad (ids of any rank: the last axis is the sequence)"""
    return ids.reshape(-1, ids.shape[-1]).ne(pad)


def norms(g, ids, pad):
    """float64 [nseq]: the L2 norm of every sequence's gradient over its live tokens"""
    S = ids.shape[-1]
    g = g.double().reshape(-1, S, g.shape[-1])
    m = live(ids, pad)
    return torch.where(m[..., None], g, torch.zeros((), dtype=torch.float64)).pow(2).sum((1, 2)).sqrt()


def scale(g, ids, pad, epsilon):
    """float64 [nseq]"""
    n = norms(g, ids, pad)
    return torch.where(n > 0, float(epsilon) / torch.where(n > 0, n, torch.ones_like(n)), torch.zeros_like(n))


def perturbation(g, ids, pad, sc):
    """float64 [nseq, S, H]: sc[s] * g[s, t] at live tokens, exactly 0 at pads (whatever g holds there)"""
    S = ids.shape[-1]
    g = g.double().reshape(-1, S, g.shape[-1])
    return torch.where(live(ids, pad)[..., None], sc.double()[:, None, None] * g, torch.zeros((), dtype=torch.float64))


def embed_ln_adv(ids, pos, tt, word, ptab, ttab, gamma, beta, eps, g, sc, pad, mask=None, p=0.0):
    """-> y, z, mean, rstd in float64, rows = tokens.  tt None: type row 0.  mask: the 0/1 dropout mask [ntok, H]"""
    H_ = word.shape[1]
    idf, pf = ids.reshape(-1), pos.reshape(-1)
    tf = torch.zeros_like(idf) if tt is None else tt.reshape(-1)
    z = (word.double()[idf] + ttab.double()[tf]) + ptab.double()[pf]
    z = z + perturbation(g, ids, pad, sc).reshape(-1, H_)
    y, mean, rstd = R.ln_fwd(z, gamma, beta, eps)
    if mask is not None:
        y = y * mask * R.inv_keep(p)
    return y, z, mean, rstd
