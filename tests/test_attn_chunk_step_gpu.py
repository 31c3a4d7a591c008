"""The two MFMA attention backwards run ONE chunk step (csrc/attn_tiles.h: bwd_chunk_phase1 / bwd_chunk_phase2, called from
attn_mfma_bwd_body and attn_long_bwd_body): on the same operands, mask, seed, output and logsumexp, attn.mfma_backward and
attn.long_backward (kv_share = 1) return the same dq, dk and dv -- value equality, a signed zero is not a difference.  Both
use the same expressions in the same order for delta, the probabilities and the scale products, and the chunks that one of
them skips contribute exact zeros.  heads 2, head dim 64, G = 2.
Shapes (Tq, Tk): the smallest that cross a chunk boundary, a key-tile boundary, a query-tile boundary and the two-tile maximum.
No fully masked sequence: the two forwards define its logsumexp differently (pinned in test_attn_long_gpu.py)."""
import functools
import math

import pytest
import torch

from fcmf_framework import _hip as H
from fcmf_framework import attn

pytestmark = pytest.mark.gpu

HEADS, D, G = 2, 64, 2
HD = HEADS * D
FMIN = torch.finfo(torch.float32).min
SHAPES = [(33, 17), (128, 97), (130, 129), (200, 256)]
SEED = 0x5EED1234ABCD


def _rand(shape, seed, scale=0.8):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def _operands(Tq, Tk):
    dev = torch.device("cuda:0")
    return tuple(t.to(dev) for t in (_rand((G, Tq, HD), 1), _rand((G, Tk, HD), 2), _rand((G, Tk, HD), 3), _rand((G, Tq, HD), 4)))


def _mask(kind, Tk):
    if kind == "none":
        return None
    if kind == "soft":
        return (torch.randn((G, Tk), generator=torch.Generator().manual_seed(7)) * 2.0).cuda()
    m = torch.zeros((G, Tk))
    live = Tk - Tk // 3                 # the trailing third is padding ...
    m[:, live:] = FMIN
    if live > 64:                       # ... and one whole 32-key chunk in the middle is dead, live keys on both sides
        c = 1 if live <= 96 else 2
        m[:, 32 * c:32 * c + 32] = FMIN
    return m.cuda()


@pytest.mark.parametrize("kind", ["none", "soft", "hard"])
@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("Tq,Tk", SHAPES, ids=["Tq%d-Tk%d" % s for s in SHAPES])
def test_short_and_long_backward_agree(Tq, Tk, p, kind):
    q, k, v, dout = _operands(Tq, Tk)
    mask = _mask(kind, Tk)
    scale = 1.0 / math.sqrt(D)
    a = attn.desc(q, k, v, None, None, mask, None, HEADS, 1, scale, p, SEED, False, 0)
    out = torch.empty_like(q)
    lse = torch.empty((G, HEADS, Tq), dtype=torch.float32, device=q.device)
    attn.forward(a, out, lse, mfma=True)
    short = [torch.empty_like(t) for t in (q, k, v)]
    attn.mfma_backward(a, out, dout, lse, *[H.ptr(t) for t in short])
    long = [torch.empty_like(t) for t in (q, k, v)]
    attn.long_backward(q, k, v, mask, out, dout, lse, *long, HEADS, 1, scale, p, SEED)
    torch.cuda.synchronize()
    for name, s, l in zip(("dq", "dk", "dv"), short, long):
        assert torch.isfinite(s.float()).all(), name
        assert torch.equal(s, l), (name, (s != l).nonzero()[:1].tolist())
