"""Micro-benchmark of the attention-probabilities kernels at the FCMF-base text-encoder shape (384 sequences x 12 heads x 128 x 128,
head dim 64, bf16, padding masks with lengths U{32..128}), read in place from a [rows, 3*H] q|k|v buffer as the fused layer does,
with the forward attention kernel of the same run for scale.  Usage (GPU box, repo root):  python tools/attn_probs_bench.py
Prints one JSON line: times in microseconds, the HBM write rate the probabilities' time implies (G*heads*T*T*4 bytes out)."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.getcwd(), "multimodal-aspect-category-sentiment-analysis_amd"))
import torch
from fcmf_framework import attn, fused

dev = torch.device("cuda:0")
G, T, Hd, heads = 384, 128, 768, 12
g = torch.Generator().manual_seed(0)
qkv = (torch.randn(G * T, 3 * Hd, generator=g) * 0.5).to(dev).bfloat16()
lens = torch.randint(32, T + 1, (G,), generator=g)
mask = ((torch.arange(T)[None, :] >= lens[:, None]).float() * torch.finfo(torch.float32).min).to(dev)
probs = torch.empty((G, heads, T, T), dtype=torch.float32, device=dev)


def timeit(fn, reps=30):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


res = {"shape": dict(G=G, heads=heads, Tq=T, Tk=T, d=Hd // heads, dtype="bf16")}
res["fwd_mfma_us"] = round(timeit(lambda: fused.self_attention_fwd(qkv, mask, G, T, Hd, heads, 0.0, 0)), 1)
for name, use in (("probs_mfma_us", True), ("probs_valu_us", False)):
    attn.USE_MFMA_ATTENTION = use
    try:
        res[name] = round(timeit(lambda: fused.self_attention_probs(qkv, mask, G, T, Hd, heads, probs)), 1)
    finally:
        attn.USE_MFMA_ATTENTION = True
out_bytes = probs.numel() * 4
res["out_MB"] = round(out_bytes / 1e6, 1)
res["probs_mfma_write_TBps"] = round(out_bytes / (res["probs_mfma_us"] * 1e-6) / 1e12, 3)
res["probs_valu_write_TBps"] = round(out_bytes / (res["probs_valu_us"] * 1e-6) / 1e12, 3)
res["row_sum_err"] = float((probs.double().sum(-1) - 1).abs().max())
print(json.dumps(res))
