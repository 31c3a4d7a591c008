"""The comparison baselines against fixtures recorded from the REFERENCE's own training scripts
(tools/make_baseline_golden.py -> tests/golden/baseline_*.npz): the scripts' state-dict key lists and shapes, full-model
per-aspect logits, the loss (sum over aspects of the batch-mean cross entropy) and every parameter's gradient -- the text
encoder's included -- from `forward_aspects` on the inputs and weights that tests/baseline_ref.py regenerates from seeds.

Bounds (test_parity_gpu.py's): float32 logits and loss within 1e-3, gradient norms and the fixture's sampled elements within
2e-4 as for fcmf_tiny; bf16 logits within 2e-2 x |ref|max, gradient norms within 3e-2, cosine over the sampled elements
>= 0.999.  float32 at 371 keys runs the chunked VALU route of ops.shared_kv_attention."""
import os

import numpy as np
import pytest
import torch

from baseline_ref import CFG, FIX_A, FIX_B, fixture_batch, seeded_state
from conftest import GOLD
from helpers import make_hf_dir

pytestmark = pytest.mark.gpu

FIXTURES = {"mroberta-371": ("mRoBERTa", "baseline_mroberta_371keys.npz", 7, 4),
            "mroberta-595": ("mRoBERTa", "baseline_mroberta_595keys.npz", 7, 36),
            "tomroberta-371": ("TomBERT", "baseline_tomroberta_371keys.npz", 7, 4),
            "ef_captr": ("EFCapTrRoBERTa", "baseline_ef_captr.npz", 7, 4)}
CASES = [(f, torch.float32) for f in FIXTURES if f != "mroberta-595"] + [(f, torch.bfloat16) for f in FIXTURES]
ZERO_GRAD = (".key.bias",)           # analytically zero (softmax shift invariance): rounding noise only


@pytest.fixture(scope="module")
def hf_dir():
    return make_hf_dir(CFG)


def _cos(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return (a @ b / (a.norm() * b.norm() + 1e-300)).item()


@pytest.mark.parametrize("fix,dtype", CASES, ids=[f"{f}-{'f32' if d == torch.float32 else 'bf16'}" for f, d in CASES])
def test_baseline_matches_reference_fixture(dev, hf_dir, fix, dtype):
    from fcmf_framework import baselines, ops
    cls, file, NI, NR = FIXTURES[fix]
    z = np.load(os.path.join(GOLD, file))
    model = getattr(baselines, cls)(hf_dir, num_labels=4)
    named = dict(model.named_parameters())
    # the reference script's parameter names and shapes are this model's
    assert {str(k): tuple(int(x) for x in str(s).split(",")) for k, s in zip(z["keys"], z["shapes"])} == \
        {n: tuple(p.shape) for n, p in named.items()}
    model.load_state_dict(seeded_state({n: p.shape for n, p in named.items()}), strict=False)
    model = model.to(dev).eval()
    ops.shadows.clear()
    named = dict(model.named_parameters())
    ids, mask, tids, tmask, vis, roi, labels = (t.to(dev) for t in fixture_batch(NI, NR))
    args = {"mRoBERTa": (ids, mask, vis, roi), "TomBERT": (tids, tmask, ids, mask, vis, roi), "EFCapTrRoBERTa": (ids, mask)}[cls]
    ops.set_compute_dtype(dtype)
    try:
        logits = model.forward_aspects(*args)
        loss = model.loss_aspects(logits, labels)
        loss.backward()
    finally:
        ops.set_compute_dtype(torch.float32)
    ref = torch.from_numpy(z["logits"])
    assert logits.shape == (FIX_B, FIX_A, 4)
    e_log, e_loss = (logits.float().cpu() - ref).abs().max().item(), abs(loss.item() - float(z["loss"]))
    worst, e_el, got, want = ("", 0.0), ("", 0.0), [], []
    for n, rn in zip([str(x) for x in z["grad_names"]], z["grad_norms"]):
        if n.endswith(ZERO_GRAD) or n.startswith("roberta.pooler"):
            continue
        g = named[n].grad
        assert g is not None and torch.isfinite(g).all(), n
        worst = max(worst, (n, abs(g.float().norm().item() - rn) / max(rn, 1e-3)), key=lambda t: t[1])
        gs = g.float().flatten().cpu()[torch.from_numpy(z["gidx_" + n])]
        r = torch.from_numpy(z["g_" + n]).float()
        e_el = max(e_el, (n, (gs - r).abs().max().item() / max(r.abs().max().item(), 1e-4)), key=lambda t: t[1])
        got.append(gs / (r.norm() + 1e-30)); want.append(r / (r.norm() + 1e-30))
    c = _cos(torch.cat(got), torch.cat(want))
    print(f"{fix} {dtype}: logit err {e_log:.3e} (|ref|max {ref.abs().max().item():.3f}), loss err {e_loss:.3e}, worst gradient norm err "
          f"{worst}, worst sampled element err {e_el}, cosine over the sampled elements {c:.6f}")
    assert named["roberta.pooler.dense.weight"].grad is None          # unused by these models, in the reference too
    if dtype == torch.float32:
        assert e_log < 1e-3 and e_loss < 1e-3 and worst[1] < 2e-4 and e_el[1] < 2e-4
    else:
        assert e_log < 2e-2 * ref.abs().max().item() and worst[1] < 3e-2 and c > 0.999
