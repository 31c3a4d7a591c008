"""The comparison baselines (fcmf_framework/baselines.py) on the GPU against a float64 restatement built from torch's own
nn.MultiheadAttention / nn.TransformerEncoder on the CPU, loaded from the SAME state dict (so the key names and shapes of
fcmf_framework/torch_layers.py are exercised on the way), and `forward_aspects` against stacked `forward`.

The text encoder is tested elsewhere (test_parity_gpu.py); here both sides start from the same last_hidden_state, so that
what is compared is what this module adds: the two visual projections, the cross-attention over 106 / 371 / 595 visual
tokens, the transformer layers on top and the classifier -- logits, the gradient into the text features and the gradient
of every new parameter.

Bounds (the project's, test_parity_gpu.py): float32 logits within 1e-3; bf16 logits within 2e-2 x |ref|max, gradients per
parameter within 3e-2 of the reference norm and cosine >= 0.999 with every parameter normalised by its reference norm.
float32 runs at 2 photos (106 keys): the float32 VALU attention holds K and V of a head in LDS, about 280 keys at most."""
import pytest
import torch

from baseline_ref import CFG, RefM, RefT
from helpers import make_hf_dir

pytestmark = pytest.mark.gpu

B, A, S, T = 3, 3, 40, 16
GEOMS = {"f32-106keys": (torch.float32, 2, 4), "bf16-371keys": (torch.bfloat16, 7, 4), "bf16-595keys": (torch.bfloat16, 7, 36)}


@pytest.fixture(scope="module")
def hf_dir():
    return make_hf_dir(CFG)


def _seed_params(model, seed=0):
    g = torch.Generator().manual_seed(seed)
    for n, p in model.named_parameters():
        if n.startswith("roberta."):
            continue
        if "norm" in n and n.endswith("weight"):
            p.data = 1 + 0.1 * torch.randn(p.shape, generator=g)
        else:
            p.data = 0.06 * torch.randn(p.shape, generator=g)


def _batch(NI, NR, seed=1):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, CFG["vocab_size"], (B, A, S), generator=g)
    lens = torch.tensor([[40, 33, 21], [17, 40, 9], [28, 12, 40]])[:B, :A]
    mask = (torch.arange(S)[None, None, :] < lens[..., None]).long()
    ids = torch.where(mask.bool(), ids, torch.full_like(ids, CFG["pad_token_id"]))
    tids = torch.randint(3, CFG["vocab_size"], (B, A, T), generator=g)
    tmask = (torch.arange(T)[None, None, :] < torch.randint(2, T + 1, (B, A, 1), generator=g)).long()
    tids = torch.where(tmask.bool(), tids, torch.full_like(tids, CFG["pad_token_id"]))
    vis = torch.randn(B, NI, 49, 2048, generator=g) * 0.5
    roi = torch.randn(B, NI, NR, 2048, generator=g) * 0.5
    return ids, mask, tids, tmask, vis, roi


def _cos(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return (a @ b / (a.norm() * b.norm() + 1e-300)).item()


def _compare(tag, dtype, logits, ref_logits, grads, ref_grads):
    """grads / ref_grads: name -> tensor (parameters of the new modules and the text features)"""
    err = (logits.detach().float().cpu() - ref_logits.detach().float()).abs().max().item()
    scale = ref_logits.abs().max().item()
    worst, got, ref = ("", 0.0), [], []
    for n, r in ref_grads.items():
        g = grads[n].detach().double().cpu()
        rn = r.double().norm().item()
        e = abs(g.norm().item() - rn) / rn
        worst = max(worst, (n, e), key=lambda t: t[1])
        got.append(g.flatten() / rn)
        ref.append(r.double().flatten() / rn)
    c = _cos(torch.cat(got), torch.cat(ref))
    print(f"{tag}: logit err {err:.3e} (|ref|max {scale:.3f}), worst gradient norm err {worst}, cosine {c:.6f}")
    if dtype == torch.float32:
        assert err < 1e-3 and worst[1] < 1e-3 and c > 0.99999
    else:
        assert err < 2e-2 * scale and worst[1] < 3e-2 and c > 0.999


def _load_ref(ref, model):
    sd = {k: v.detach().cpu().double() for k, v in model.state_dict().items() if not k.startswith("roberta.")}
    ref.double().load_state_dict(sd, strict=True)         # torch's own modules accept the product's keys and shapes
    return ref.eval()


def _new_param_grads(model):
    return {n: p.grad for n, p in model.named_parameters() if not n.startswith("roberta.")}


@pytest.mark.parametrize("geom", list(GEOMS))
def test_mroberta_matches_torch_modules(dev, hf_dir, geom):
    from fcmf_framework import ops
    from fcmf_framework.baselines import mRoBERTa
    dtype, NI, NR = GEOMS[geom]
    model = mRoBERTa(hf_dir)
    _seed_params(model)
    ref = _load_ref(RefM(), model)
    model = model.to(dev).eval()
    ids, mask, _, _, vis, roi = _batch(NI, NR)
    ids, mask = ids[:, 0], mask[:, 0]
    w = torch.randn(B, 4, generator=torch.Generator().manual_seed(9))
    ops.set_compute_dtype(dtype)
    try:
        text = model._encode(ids.to(dev), mask.to(dev)).detach().requires_grad_(True)
        logits = model._fuse(text, model._visual_tokens(vis.to(dev), roi.to(dev)), mask.to(dev), 1)
        (logits * w.to(dev)).sum().backward()
    finally:
        ops.set_compute_dtype(torch.float32)
    tr = text.detach().double().cpu().requires_grad_(True)
    ref_logits = ref(tr, mask, vis.double(), roi.double())
    (ref_logits * w.double()).sum().backward()
    grads, ref_grads = _new_param_grads(model), {n: p.grad for n, p in ref.named_parameters()}
    grads["text"], ref_grads["text"] = text.grad, tr.grad
    _compare("mRoBERTa " + geom, dtype, logits, ref_logits, grads, ref_grads)


@pytest.mark.parametrize("geom", ["f32-106keys", "bf16-371keys"])
def test_tombert_matches_torch_modules(dev, hf_dir, geom):
    from fcmf_framework import ops
    from fcmf_framework.baselines import TomBERT
    dtype, NI, NR = GEOMS[geom]
    model = TomBERT(hf_dir)
    _seed_params(model)
    ref = _load_ref(RefT(), model)
    model = model.to(dev).eval()
    ids, mask, tids, tmask, vis, roi = _batch(NI, NR)
    ids, mask, tids, tmask = ids[:, 0], mask[:, 0], tids[:, 0], tmask[:, 0]
    w = torch.randn(B, 4, generator=torch.Generator().manual_seed(9))
    ops.set_compute_dtype(dtype)
    try:
        h_t = model._encode(tids.to(dev), tmask.to(dev)).detach().requires_grad_(True)
        h_s = model._encode(ids.to(dev), mask.to(dev)).detach().requires_grad_(True)
        logits = model._fuse(h_t, h_s, mask.to(dev), model._visual_tokens(vis.to(dev), roi.to(dev)), 1)
        (logits * w.to(dev)).sum().backward()
    finally:
        ops.set_compute_dtype(torch.float32)
    tr, sr = (t.detach().double().cpu().requires_grad_(True) for t in (h_t, h_s))
    ref_logits = ref(tr, sr, mask, vis.double(), roi.double())
    (ref_logits * w.double()).sum().backward()
    grads, ref_grads = _new_param_grads(model), {n: p.grad for n, p in ref.named_parameters()}
    grads.update(h_t=h_t.grad, h_s=h_s.grad)
    ref_grads.update(h_t=tr.grad, h_s=sr.grad)
    _compare("TomBERT " + geom, dtype, logits, ref_logits, grads, ref_grads)


@pytest.mark.parametrize("geom", ["f32-106keys", "bf16-371keys"])
@pytest.mark.parametrize("name", ["mRoBERTa", "TomBERT", "EFCapTrRoBERTa"])
def test_forward_aspects_equals_stacked_forward(dev, hf_dir, name, geom):
    """logits and the loss gradient: all aspects in one pass with the visual tokens projected once per review and read with
    kv_share = A, against one `forward` per aspect"""
    from fcmf_framework import baselines, ops
    dtype, NI, NR = GEOMS[geom]
    model = getattr(baselines, name)(hf_dir)
    _seed_params(model)
    model = model.to(dev).eval()
    ids, mask, tids, tmask, vis, roi = (t.to(dev) for t in _batch(NI, NR))
    labels = torch.randint(0, 4, (B, A), generator=torch.Generator().manual_seed(3)).to(dev)
    if name == "mRoBERTa":
        args = lambda a: (ids[:, a], mask[:, a], vis, roi) if a is not None else (ids, mask, vis, roi)
    elif name == "TomBERT":
        args = lambda a: (tids[:, a], tmask[:, a], ids[:, a], mask[:, a], vis, roi) if a is not None else (tids, tmask, ids, mask, vis, roi)
    else:
        args = lambda a: (ids[:, a], mask[:, a]) if a is not None else (ids, mask)
    ops.set_compute_dtype(dtype)
    try:
        one = model.forward_aspects(*args(None))
        model.loss_aspects(one, labels).backward()
        g_one = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
        model.zero_grad()
        stacked = torch.stack([model(*args(a)) for a in range(A)], 1)
        model.loss_aspects(stacked, labels).backward()
        g_st = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    finally:
        ops.set_compute_dtype(torch.float32)
    assert one.shape == (B, A, 4) and set(g_one) == set(g_st)
    err, scale = (one - stacked).abs().max().item(), stacked.abs().max().item()
    names = [n for n in g_st if not n.endswith(".key.bias")]      # (analytically zero, softmax shift invariance: rounding noise only)
    a = torch.cat([g_one[n].flatten() / g_st[n].norm() for n in names])
    b = torch.cat([g_st[n].flatten() / g_st[n].norm() for n in names])
    print(f"{name} {geom}: aspects-vs-stacked logit err {err:.3e} (|max| {scale:.3f}), gradient cosine {_cos(a, b):.6f}")
    if dtype == torch.float32:
        assert err < 1e-4 and _cos(a, b) > 0.99999
    else:
        assert err < 2e-2 * scale and _cos(a, b) > 0.999


@pytest.mark.parametrize("model,ckpt,tag", [("mroberta", "mroberta", "mroberta"), ("tomroberta", "tombert", "tombert"),
                                            ("ef_captr", "seed_3_ef_captr_model", "ef_captr")])
def test_driver_synthetic_epoch_trains_evaluates_and_checkpoints(tmp_path, dev, hf_dir, model, ckpt, tag):
    """one run_baselines.py epoch of 2 synthetic steps in bf16 at the published geometry (7 photos x 4 ROIs = 371 keys): through the
    gradient arena and FusedAdamW (the packed in_proj parameters reach both as views), finite loss, dev macro-F1, best + last
    checkpoints under the reference scripts' names with the model's key set, the weights have moved, and the test-set pass"""
    import os
    import run_baselines as drv
    from fcmf_framework import baselines, ops
    out = str(tmp_path / model)
    try:
        loss = drv.main(["--model", model, "--output_dir", out, "--pretrained_hf_model", hf_dir, "--do_train", "--do_eval", "--num_imgs", "7",
                         "--num_rois", "4", "--train_batch_size", "3", "--eval_batch_size", "3", "--synthetic_steps", "2", "--max_len", "48",
                         "--num_train_epochs", "1", "--learning_rate", "1e-3", "--seed", "3", "--bf16"])
    finally:
        ops.set_compute_dtype(torch.float32)
    assert loss == loss and abs(loss) < 1e4                       # finite
    torch.manual_seed(3)                                          # (the driver seeds torch with --seed before it builds the model)
    init = getattr(baselines, drv.MODELS[model][0])(hf_dir).state_dict()
    for t in ("best", "last"):
        ck = torch.load(os.path.join(out, f"{ckpt}_{t}.pth"), map_location="cpu", weights_only=True)
        assert set(ck) >= {"epoch", "best_score", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict"}
        assert ck["epoch"] == 0 and set(ck["model_state_dict"]) == set(init)
        assert all(torch.isfinite(v).all() for v in ck["model_state_dict"].values())
    sd = ck["model_state_dict"]
    keys = ["classifier.weight", "roberta.encoder.layer.0.attention.self.query.weight"]
    keys += {"mroberta": ["cross_attention.in_proj_weight", "mm_encoder.layers.0.self_attn.in_proj_weight", "mm_encoder.layers.2.self_attn.in_proj_bias"],
             "tomroberta": ["ti_matching.0.mha.in_proj_weight", "ti_matching.0.mha.in_proj_bias", "mm_encoder.layers.0.self_attn.in_proj_weight"],
             "ef_captr": []}[model]
    for k in keys:                                                # every one of them took optimizer steps
        assert not torch.equal(sd[k], init[k]), k
    assert torch.equal(sd["roberta.pooler.dense.weight"], init["roberta.pooler.dense.weight"])      # unused: frozen, as without a gradient
    log = open(os.path.join(out, f"training_{tag}.log")).read()
    assert "Dev macro-F1 per aspect" in log and "Test macro-F1 per aspect" in log
    assert "Average F1:" in open(os.path.join(out, f"test_results_{tag}.txt")).read()
    assert open(os.path.join(out, "test_predictions_formatted.txt")).read().count("Sentence ") == 3
