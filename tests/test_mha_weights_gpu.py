"""Attention weights of the torch-named layers: torch_layers.MultiheadAttention.forward(need_weights=True) against
torch.nn.MultiheadAttention on the CPU (float64, eval(), the same state dict), averaged over the heads and per head, and the
baselines' `output_attentions`.

Bounds are those tests/test_baselines_gpu.py holds these modules to: float32 within 1e-3; bf16 within 2e-2 x |ref|max."""
import pytest
import torch

from baseline_ref import CFG
from helpers import make_hf_dir

pytestmark = pytest.mark.gpu

E, HEADS = 128, 2
#          G  kv_share Tq   Tk  padding mask
SHAPES = {"Tq16-Tk300-share2-padding": (4, 2, 16, 300, True), "Tq170-Tk371": (2, 1, 170, 371, False)}


def _inputs(G, share, Tq, Tk, padded, seed=3):
    g = torch.Generator().manual_seed(seed)
    query = torch.randn(G, Tq, E, generator=g)
    key = torch.randn(G // share, Tk, E, generator=g)
    kpm = None
    if padded:      # per query group, True = ignore: a padded tail of its own length, holes, a whole 128-key tile; key 0 stays
        kpm = torch.rand(G, Tk, generator=g) < 0.2
        kpm[:, 0] = False
        kpm[0, 128:256] = True
        for i in range(G):
            kpm[i, Tk - 17 * (i + 1):] = True
    return query, key, kpm


def _modules(seed=0):
    from fcmf_framework import torch_layers as T
    torch.manual_seed(seed)
    ours = T.MultiheadAttention(E, HEADS, dropout=0.1, batch_first=True)
    g = torch.Generator().manual_seed(seed + 1)
    ours.in_proj_bias.data = 0.1 * torch.randn(3 * E, generator=g)
    ours.out_proj.bias.data = 0.1 * torch.randn(E, generator=g)
    ref = torch.nn.MultiheadAttention(E, HEADS, dropout=0.1, batch_first=True).double()
    ref.load_state_dict({k: v.detach().double() for k, v in ours.state_dict().items()}, strict=True)
    return ours.eval(), ref.eval()


def _close(tag, dtype, got, ref):
    err = (got.detach().double().cpu() - ref).abs().max().item()
    scale = ref.abs().max().item()
    print(f"{tag}: err {err:.3e} (|ref|max {scale:.4f})")
    assert err < (1e-3 if dtype == torch.float32 else 2e-2 * scale), (tag, err, scale)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_need_weights_matches_torch(dev, shape, dtype):
    from fcmf_framework import ops
    from fcmf_framework.layers import to_compute
    G, share, Tq, Tk, padded = SHAPES[shape]
    query, key, kpm = _inputs(G, share, Tq, Tk, padded)
    ours, ref = _modules()
    ours = ours.to(dev)
    with torch.no_grad():
        ke = key.double().repeat_interleave(share, 0)
        ref_out, ref_mean = ref(query.double(), ke, ke, key_padding_mask=kpm, need_weights=True, average_attn_weights=True)
        _, ref_per = ref(query.double(), ke, ke, key_padding_mask=kpm, need_weights=True, average_attn_weights=False)
    ops.set_compute_dtype(dtype)
    try:
        q, k = to_compute(query.to(dev)), to_compute(key.to(dev))
        m = None if kpm is None else kpm.to(dev)
        plain, none = ours(q, k, k, key_padding_mask=m, kv_share=share)
        out_a, mean = ours(q, k, k, key_padding_mask=m, need_weights=True, kv_share=share)
        out_p, per = ours(q, k, k, key_padding_mask=m, need_weights=True, average_attn_weights=False, kv_share=share)
    finally:
        ops.set_compute_dtype(torch.float32)
    assert none is None
    assert torch.equal(out_a, plain) and torch.equal(out_p, plain)        # asking for the weights does not change the output
    assert mean.shape == (G, Tq, Tk) and per.shape == (G, HEADS, Tq, Tk)
    assert mean.dtype == per.dtype == torch.float32 and not mean.requires_grad and not per.requires_grad
    _close(f"{shape} {dtype} output", dtype, plain.float(), ref_out)
    _close(f"{shape} {dtype} averaged weights", dtype, mean, ref_mean)
    _close(f"{shape} {dtype} per-head weights", dtype, per, ref_per)
    if padded:
        assert (mean.cpu()[kpm[:, None, :].expand(G, Tq, Tk)] == 0).all()      # ignored keys: exactly 0, as in torch


def test_attn_mask_stays_refused(dev):
    ours, _ = _modules()
    x = torch.zeros(2, 4, E, device=dev)
    with pytest.raises(NotImplementedError):
        ours.to(dev)(x, x, x, attn_mask=torch.zeros(4, 4, device=dev), need_weights=True)


@pytest.fixture(scope="module")
def hf_dir():
    return make_hf_dir(CFG)


@pytest.mark.parametrize("geom", ["f32-106keys", "bf16-371keys"])
@pytest.mark.parametrize("name", ["mRoBERTa", "TomBERT"])
def test_baselines_output_attentions(dev, hf_dir, name, geom):
    """forward_aspects(output_attentions=True): head-averaged cross-attention weights, one [Tq, visual tokens] block per
    aspect prompt, rows summing to 1; the logits are those of the plain call; `forward` agrees with it aspect by aspect"""
    from baseline_ref import fixture_batch
    from fcmf_framework import baselines, ops
    dtype, NI, NR = {"f32-106keys": (torch.float32, 2, 4), "bf16-371keys": (torch.bfloat16, 7, 4)}[geom]
    torch.manual_seed(0)
    model = getattr(baselines, name)(hf_dir).to(dev).eval()
    ids, mask, tids, tmask, vis, roi, _ = (t.to(dev) for t in fixture_batch(NI, NR))
    B, A, S = ids.shape
    args = (ids, mask, vis, roi) if name == "mRoBERTa" else (tids, tmask, ids, mask, vis, roi)
    Tq = S if name == "mRoBERTa" else tids.shape[2]
    ops.set_compute_dtype(dtype)
    try:
        with torch.no_grad():
            plain = model.forward_aspects(*args)
            logits, weights = model.forward_aspects(*args, output_attentions=True)
            one = tuple(t[:, 1] if t.dim() == 3 else t for t in args)      # aspect 1 alone
            logits1, weights1 = model(*one, output_attentions=True)
    finally:
        ops.set_compute_dtype(torch.float32)
    assert torch.equal(logits, plain)
    assert weights.shape == (B, A, Tq, NI * (49 + NR)) and weights.dtype == torch.float32
    assert (weights.double().sum(-1) - 1).abs().max().item() < 1e-4
    assert (weights >= 0).all()
    assert weights1.shape == (B, Tq, NI * (49 + NR))
    err = (weights1 - weights[:, 1]).abs().max().item()
    print(name, geom, "aspect 1 alone vs in the batch", err, weights.max().item())
    assert err < (1e-4 if dtype == torch.float32 else 2e-2 * weights.max().item())      # (test_baselines_gpu.py: aspects vs stacked)
