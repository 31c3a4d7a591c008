"""Micro-benchmark of the long-key, shared-K/V MFMA attention (ops.shared_kv_attention, csrc/attn_long.hip) at the mRoBERTa
cross-attention shape of a B = 64 step: G = 64 reviews x 6 aspect prompts, 12 heads of 64, 170 text queries, bf16, dropout
0.1, padding masks that keep U{3..7} of a review's 7 photos -- against 371 keys (7 x (49 + 4)) and 595 keys (7 x (49 + 36)),
kv_share = 6.  At 371 keys the same work is also timed on the only route the library had before: ops.attention on the VALU
kernel with K / V expanded six times (the expansion itself and the sum of the six key gradients are NOT timed: they would
only add to that route).  Forward + backward per call, median of per-call device-event times after warm-up, the two routes
alternating.  Usage (GPU box, repo root):  python tools/attn_long_bench.py
Then the step time of a synthetic mRoBERTa training step at B = 64 (FCMF-base sized text encoder with random weights, 7 photos x
4 ROIs, bf16, dropout on, forward_aspects + loss + backward + clip + AdamW as run_baselines.py runs it): median of 10 steps after 3.
Prints one JSON line: times in microseconds / milliseconds and the bytes/s that the operands every call must read and write
imply.  Exits with status 1 if the long-key kernel is slower than the expanded VALU route at 371 keys."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.getcwd(), "multimodal-aspect-category-sentiment-analysis_amd"))
import torch
from fcmf_framework import attn, ops

dev = torch.device("cuda:0")
B, A, heads, Tq, HD, p = 64, 6, 12, 170, 768, 0.1
G = B * A


def operands(Tk, per_photo):
    g = torch.Generator().manual_seed(0)
    mk = lambda *s: (torch.randn(*s, generator=g) * 0.5).to(dev).bfloat16().requires_grad_(True)
    q, k, v = mk(G, Tq, HD), mk(B, Tk, HD), mk(B, Tk, HD)
    w = (torch.randn(G, Tq, HD, generator=g) * 0.5).to(dev).bfloat16()
    photos = torch.randint(3, 8, (B,), generator=g)
    dead = torch.arange(Tk)[None, :] >= (photos * per_photo)[:, None]
    mask = (dead.float() * torch.finfo(torch.float32).min).repeat_interleave(A, 0).to(dev)
    return q, k, v, w, mask


def one_call(fn, q, k, v, w):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    q.grad = k.grad = v.grad = None
    a.record()
    fn(q, k, v).backward(w)
    b.record()
    return a, b


def measure(routes, reps=20, warm=3):
    """routes: name -> (fn, q, k, v, w); alternates them, returns name -> median microseconds"""
    ev = {n: [] for n in routes}
    for i in range(warm + reps):
        for n, r in routes.items():
            pair = one_call(*r)
            if i >= warm:
                ev[n].append(pair)
    torch.cuda.synchronize()
    return {n: statistics.median(a.elapsed_time(b) for a, b in ps) * 1e3 for n, ps in ev.items()}


def min_bytes(Tk):
    """fwd reads q, k, v and writes out; bwd reads q, k, v, out, dout and writes dq, dk, dv (bf16, K / V once per review)"""
    return 2 * (6 * G * Tq * HD + 6 * B * Tk * HD)


res = {"shape": dict(G=G, kv_share=A, heads=heads, Tq=Tq, d=64, dtype="bf16", dropout=p)}
for Tk, per_photo in ((371, 53), (595, 85)):
    q, k, v, w, mask = operands(Tk, per_photo)
    routes = {"long": (lambda q, k, v: ops.shared_kv_attention(q, k, v, mask=mask, heads=heads, kv_share=A, p=p, training=True),
                       q, k, v, w)}
    if Tk <= 512:
        ke = k.detach().repeat_interleave(A, 0).requires_grad_(True)
        ve = v.detach().repeat_interleave(A, 0).requires_grad_(True)

        def valu(q, k, v):
            attn.USE_MFMA_ATTENTION = False
            try:
                return ops.attention(q, k, v, mask=mask, heads=heads, p=p, training=True)
            finally:
                attn.USE_MFMA_ATTENTION = True
        routes["valu_expanded"] = (valu, q, ke, ve, w)
    t = measure(routes)
    res[f"Tk{Tk}"] = {f"{n}_fwd_bwd_us": round(us, 1) for n, us in t.items()}
    res[f"Tk{Tk}"]["long_min_bytes_MB"] = round(min_bytes(Tk) / 1e6, 1)
    res[f"Tk{Tk}"]["long_TBps"] = round(min_bytes(Tk) / (t["long"] * 1e-6) / 1e12, 3)
    del q, k, v, w, mask, routes


def mroberta_step_ms(steps=10, warm=3):
    import tempfile
    import run_baselines as drv
    import synthetic_data as synth
    from fcmf_framework.baselines import mRoBERTa
    from fcmf_framework.dp import GradArena
    from fcmf_framework.optimization import FusedAdamW
    from fcmf_framework.roberta import RobertaConfig, RobertaModel
    d = tempfile.mkdtemp(prefix="hf_")
    RobertaModel(RobertaConfig(**synth.BASE_CFG)).save_pretrained(d)
    model = mRoBERTa(d)
    for q in model.roberta.pooler.parameters():
        q.requires_grad = False
    model = model.to(dev).train()
    ops.shadows.clear()
    ops.set_compute_dtype(torch.bfloat16)
    opt = FusedAdamW(drv.param_groups(model), lr=2e-5)
    arena = GradArena.for_model(model, skip=lambda n: "roberta.pooler" in n)
    batches = [tuple(t.to(dev) if torch.is_tensor(t) else t for t in b)
               for b in drv.SyntheticBatches("mroberta", synth.BASE_CFG, 2, B, 7, 4, A, 256, 11)]
    times = []
    for i in range(warm + steps):
        arena.zero()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        logits, labels, _ = drv.forward_batch("mroberta", model, batches[i % 2], lambda v, r: (v, r))
        model.loss_aspects(logits, labels).backward()
        opt.step(max_grad_norm=1.0)
        b.record()
        torch.cuda.synchronize()
        if i >= warm:
            times.append(a.elapsed_time(b))
    arena.deactivate()
    ops.set_compute_dtype(torch.float32)
    return statistics.median(times)


res["mroberta_step_B64_ms"] = round(mroberta_step_ms(), 2)
print(json.dumps(res))
if res["Tk371"]["long_fwd_bwd_us"] > res["Tk371"]["valu_expanded_fwd_bwd_us"]:
    sys.exit("long-key MFMA attention is slower than the expanded VALU route at 371 keys")
