"""float64 numpy restatement of the BERTScore definition in include/fcmf_hip.h, shared by the kernel and the scorer tests"""
import numpy as np


def ref_scores(c, r, lc, lr, wc=None, wr=None):
    """float64 restatement: c [N, Lc, H], r [N, Lr, H] float64 arrays, lengths, optional weights -> [N, 3]"""
    out = np.zeros((c.shape[0], 3))
    for n in range(c.shape[0]):
        a, b = c[n, :lc[n]], r[n, :lr[n]]
        if lc[n] == 0 or lr[n] == 0:
            continue
        u = np.ones(lc[n]) if wc is None else wc[n, :lc[n]].astype(np.float64)
        v = np.ones(lr[n]) if wr is None else wr[n, :lr[n]].astype(np.float64)
        if u.sum() == 0 or v.sum() == 0:
            continue
        s = (a @ b.T) / (np.linalg.norm(a, axis=1)[:, None] * np.linalg.norm(b, axis=1)[None, :])
        p = (u * s.max(1)).sum() / u.sum()
        q = (v * s.max(0)).sum() / v.sum()
        out[n] = (p, q, 2 * p * q / (p + q) if p + q != 0 else 0.0)
    return out
