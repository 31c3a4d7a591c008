"""Float64 CPU reference of the training loss with options (include/fcmf_hip.h, fcmf_xent_*_ex):

    l_n  = (1 - eps) w_y (1 - p_y)^gamma (-log p_y) + (eps / C) sum_c w_c (-log p_c)
    loss = mult * sum_s [ sum_{n in s, live} l_n / sum_{n in s, live} w_{y_n} ]        row r -> segment r % segments

`loss_ref` is what the tests compare against: torch's own F.cross_entropy per segment for gamma = 0, the formula through float64
autograd for gamma > 0.  `loss_rows` states the formula row by row (the forward kernels' two outputs)."""
import torch
import torch.nn.functional as F


def _segment_weight(weight, s):
    if weight is None:
        return None
    w = weight.detach().double().cpu()
    return w if w.dim() == 1 else w[s]


def loss_rows(logits, labels, weight=None, eps=0.0, gamma=0.0, segments=1, ignore_index=-100):
    """-> (num [n], den [n]) in float64, differentiable in `logits` (a float64 CPU tensor): l_n and w_{y_n}, 0 for ignored rows.
    1 - p_y is summed from the other classes' probabilities, so a confident row keeps its digits."""
    n, C = logits.shape
    live = labels != ignore_index
    y = torch.where(live, labels, torch.zeros_like(labels))
    w = torch.ones(n, C, dtype=torch.float64)
    if weight is not None:
        for s in range(segments):
            w[s::segments] = _segment_weight(weight, s)
    logp = F.log_softmax(logits, dim=1)
    hot = F.one_hot(y, C).bool()
    q = logp.exp().masked_fill(hot, 0.0).sum(1)
    lpy = logp.gather(1, y[:, None])[:, 0]
    wy = w.gather(1, y[:, None])[:, 0]
    focal = q.pow(gamma) if gamma > 0 else torch.ones_like(q)
    num = (1.0 - eps) * wy * focal * (-lpy) + (eps / C) * (w * -logp).sum(1)
    zero = torch.zeros_like(num)
    return torch.where(live, num, zero), torch.where(live, wy, zero)


def loss_formula(logits, labels, weight=None, eps=0.0, gamma=0.0, segments=1, ignore_index=-100, mult=1.0):
    num, den = loss_rows(logits, labels, weight, eps, gamma, segments, ignore_index)
    return mult * sum(num[s::segments].sum() / den[s::segments].sum() for s in range(segments))


def loss_ref(logits, labels, weight=None, eps=0.0, gamma=0.0, segments=1, ignore_index=-100, mult=1.0):
    """logits: float64 CPU [n, C] (requires_grad for the gradient), labels int64 CPU [n], weight None / [C] / [segments, C]"""
    assert logits.dtype == torch.float64 and not logits.is_cuda
    if gamma > 0:
        return loss_formula(logits, labels, weight, eps, gamma, segments, ignore_index, mult)
    return mult * sum(F.cross_entropy(logits[s::segments], labels[s::segments], weight=_segment_weight(weight, s), label_smoothing=eps,
                                      ignore_index=ignore_index) for s in range(segments))
