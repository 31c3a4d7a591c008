"""The symmetric-KL (R-Drop) term of include/fcmf_hip.h as torch states it, in float64 on the CPU: rows by F.kl_div on
log_softmax in both directions, the per-segment mean over the live pairs, gradients by autograd.  `closed_form` and
`closed_form_grads` are the header's own formulas, which tests/test_rdrop_cpu.py holds against this statement."""
import torch
import torch.nn.functional as F


def rows(a, b):
    """k_r = 1/2 [KL(p_r || q_r) + KL(q_r || p_r)], p = softmax(a), q = softmax(b): float64 [n]"""
    la, lb = F.log_softmax(a.double(), -1), F.log_softmax(b.double(), -1)
    kl_pq = F.kl_div(lb, la, reduction="none", log_target=True).sum(-1)       # KL(p || q): input = log q, target = log p
    kl_qp = F.kl_div(la, lb, reduction="none", log_target=True).sum(-1)
    return 0.5 * (kl_pq + kl_qp)


def live_mask(n, labels=None, ignore_index=-100):
    return torch.ones(n, dtype=torch.bool) if labels is None else labels.reshape(-1).cpu() != ignore_index


def loss(a, b, labels=None, ignore_index=-100, alpha=1.0, segments=1):
    """alpha * sum_s [ sum_{r in s, live} k_r / #live pairs of s ], pair r in segment r % segments (0 / 0 = NaN for a dead segment)"""
    C = a.shape[-1]
    k = rows(a.reshape(-1, C), b.reshape(-1, C))
    live = live_mask(k.shape[0], labels, ignore_index)
    k = torch.where(live, k, torch.zeros_like(k))
    return alpha * sum(k[s::segments].sum() / live[s::segments].sum().double() for s in range(segments))


def closed_form(a, b):
    """1/2 sum_c (p_c - q_c) d_c, d = a - b"""
    a, b = a.double(), b.double()
    return 0.5 * ((F.softmax(a, -1) - F.softmax(b, -1)) * (a - b)).sum(-1)


def closed_form_grads(a, b):
    """(dk/da, dk/db) = (1/2 [p (d - E_p d) + p - q], -1/2 [q (d - E_q d) + p - q])"""
    a, b = a.double(), b.double()
    p, q, d = F.softmax(a, -1), F.softmax(b, -1), a - b
    Ep, Eq = (p * d).sum(-1, keepdim=True), (q * d).sum(-1, keepdim=True)
    return 0.5 * (p * (d - Ep) + p - q), -0.5 * (q * (d - Eq) + p - q)
