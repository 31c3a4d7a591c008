"""Micro-benchmark of the BERTScore matching kernel (fcmf_bertscore through ops.bertscore) at the shape the IAOG evaluation makes:
N = 4096 pairs of 24 x 24 tokens, H = 768, bf16, <s> / </s> weights -- next to the same scores written in eager torch (normalise,
torch.bmm, max, weighted means) on the same tensors, as a yardstick only: the product never takes that path.
Usage (GPU box, repo root):  python tools/bertscore_bench.py
Prints one JSON line: median microseconds of 9 windows of 50 calls each (device events, 5 warm-up calls per path, the two paths
alternating), the input bytes a call has to read, the HBM rate the kernel's time implies, and the largest difference of the scores."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.getcwd(), "multimodal-aspect-category-sentiment-analysis_amd"))
import torch
from fcmf_framework import ops

dev = torch.device("cuda:0")
N, L, Hd = 4096, 24, 768
g = torch.Generator().manual_seed(0)
base = torch.randn(N, 1, Hd, generator=g)
cand = (0.6 * base + torch.randn(N, L, Hd, generator=g)).to(dev).bfloat16()
ref = (0.6 * base + torch.randn(N, L, Hd, generator=g)).to(dev).bfloat16()
lens = torch.full((N,), L, dtype=torch.int32, device=dev)
w = torch.ones(N, L, device=dev)
w[:, 0] = w[:, -1] = 0.0


def kernel():
    return ops.bertscore(cand, ref, lens, lens, w, w)


def eager():
    c = cand.float()
    r = ref.float()
    c = c / c.norm(dim=-1, keepdim=True)
    r = r / r.norm(dim=-1, keepdim=True)
    s = torch.bmm(c, r.transpose(1, 2))
    p = (s.max(2).values * w).sum(1) / w.sum(1)
    q = (s.max(1).values * w).sum(1) / w.sum(1)
    return torch.stack([p, q, 2 * p * q / (p + q)], 1)


def window(fn, reps=50):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


for fn in (kernel, eager):
    for _ in range(5):
        fn()
torch.cuda.synchronize()
times = {"kernel": [], "eager": []}
for _ in range(9):
    times["kernel"].append(window(kernel))
    times["eager"].append(window(eager))
in_bytes = (cand.numel() + ref.numel()) * 2
k_us = statistics.median(times["kernel"])
res = {"shape": dict(N=N, Lc=L, Lr=L, H=Hd, dtype="bf16"),
       "kernel_us": round(k_us, 1), "kernel_us_min_max": [round(min(times["kernel"]), 1), round(max(times["kernel"]), 1)],
       "eager_bmm_max_us": round(statistics.median(times["eager"]), 1),
       "eager_us_min_max": [round(min(times["eager"]), 1), round(max(times["eager"]), 1)],
       "in_MB": round(in_bytes / 1e6, 1), "kernel_read_TBps": round(in_bytes / (k_us * 1e-6) / 1e12, 3),
       "max_abs_diff": float((kernel() - eager()).abs().max())}
print(json.dumps(res))
