"""Micro-benchmark of the feed-forward dropout fused into the FFN GEMMs' epilogues (fcmf_gemm_drop) against the same result
composed from the entry points that existed before it, at the TomBERT shape: M = 8 reviews x 6 aspects x 257 tokens = 12 336
rows, N = 3072, K = 768, bf16, both operands K-contiguous.
  forward   fused:    fcmf_gemm_drop FCMF_EPI_GELU_DROP (+ aux)
            composed: fcmf_gemm FCMF_EPI_GELU (+ aux), fcmf_dropout in place
  backward  fused:    fcmf_gemm_drop FCMF_EPI_DGELU_DROP (+ colsum)
            composed: fcmf_gemm FCMF_EPI_DGELU, fcmf_dropout in place, fcmf_colsum
(the column sums are added into a buffer on both sides: its zero fill belongs to the layer's one fill of all its gradients)
Usage (GPU box, repo root):  python tools/ffn_dropout_bench.py [--out FILE] [--p 0.1] [--rounds 15] [--reps 20]
Prints (and writes to FILE) one JSON object: per path the median microseconds per call over `rounds` windows of `reps` calls
(device events, 5 warm-up calls per path, the four paths alternating round by round), min and max of the windows, the name of the
last GEMM kernel, and how far the fused results are from the composed ones (kept sets must be equal; a kept value differs by the
second bf16 rounding of the composed form at most)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.getcwd(), "multimodal-aspect-category-sentiment-analysis_amd"))
import torch
from fcmf_framework import _hip as H

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--p", type=float, default=0.1)
ap.add_argument("--rounds", type=int, default=15)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--shape", type=int, nargs=3, default=[8 * 6 * 257, 3072, 768], metavar=("M", "N", "K"))
args = ap.parse_args()

assert torch.cuda.is_available(), "this benchmark measures the MI355X: there is nothing to report without one"
dev = torch.device("cuda:0")
M, N, K = args.shape
p, seed = args.p, (5 << 32) | 17
g = torch.Generator().manual_seed(0)
bf = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(dev).bfloat16()
A, W, u = bf(M, K), bf(N, K, scale=0.2), bf(M, N, scale=1.5)
bias = torch.randn(N, generator=g).to(dev)
C1, C2, U1, U2 = (torch.empty((M, N), dtype=torch.bfloat16, device=dev) for _ in range(4))
cs1, cs2 = (torch.zeros(N, dtype=torch.float32, device=dev) for _ in range(2))
L, ctx, P, BF = H.lib(), H.gemm_ctx(), H.ptr, H.BF16
names = {}


def gemm(C, b, aux, cs, epi):
    H.check(L.fcmf_gemm(ctx, P(A), P(W), P(C), P(b), P(aux), P(cs), M, N, K, K, K, N, 0, 0, BF, BF, epi, 0, H.stream()), "fcmf_gemm")


def gemm_drop(C, b, aux, cs, epi):
    H.check(L.fcmf_gemm_drop(ctx, P(A), P(W), P(C), P(b), P(aux), P(cs), M, N, K, K, K, N, 0, 0, BF, BF, epi, p, seed, H.stream()), "fcmf_gemm_drop")


def dropout(C):
    H.check(L.fcmf_dropout(P(C), P(C), M * N, p, seed, BF, H.stream()), "fcmf_dropout")


def fwd_fused():
    gemm_drop(C1, bias, U1, None, H.EPI_GELU_DROP)


def fwd_composed():
    gemm(C2, bias, U2, None, H.EPI_GELU)
    dropout(C2)


def bwd_fused():
    gemm_drop(C1, None, u, cs1, H.EPI_DGELU_DROP)


def bwd_composed():
    gemm(C2, None, u, None, H.EPI_DGELU)
    dropout(C2)
    H.check(L.fcmf_colsum(P(C2), P(cs2), M, N, N, BF, 1, H.stream()), "fcmf_colsum")


PATHS = {"forward_fused": fwd_fused, "forward_composed": fwd_composed, "backward_fused": bwd_fused, "backward_composed": bwd_composed}


def window(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / args.reps * 1e3


def agreement():
    """fused against composed on the same operands: kept sets, largest relative difference of a kept value, column sums"""
    out = {}
    for tag, f, c in (("forward", fwd_fused, fwd_composed), ("backward", bwd_fused, bwd_composed)):
        cs1.zero_(), cs2.zero_()
        f(), c()
        torch.cuda.synchronize()
        x, y = C1.float(), C2.float()
        out[tag] = {"kept_sets_equal": bool(torch.equal(x != 0, y != 0)),
                    "max_rel_diff_of_a_value": float(((x - y).abs() / y.abs().clamp_min(1e-30)).max()),
                    "kept_fraction": float((x != 0).float().mean())}
        if tag == "forward":
            out[tag]["aux_equal"] = bool(torch.equal(U1, U2))
        else:
            out[tag]["colsum_max_rel_diff"] = float((cs1 - cs2).abs().max() / cs2.abs().max())
    return out


for name, fn in PATHS.items():
    for _ in range(5):
        fn()
    names[name] = H.last_gemm_kernel()
torch.cuda.synchronize()
times = {n: [] for n in PATHS}
order = list(PATHS)
for r in range(args.rounds):
    for n in (order if r % 2 == 0 else order[::-1]):
        times[n].append(window(PATHS[n]))
res = {"shape": dict(M=M, N=N, K=K, dtype="bf16", p=p), "rounds": args.rounds, "calls_per_window": args.reps, "unit": "us per call"}
for n in PATHS:
    t = times[n]
    res[n] = {"median": round(statistics.median(t), 1), "min": round(min(t), 1), "max": round(max(t), 1), "last_gemm_kernel": names[n]}
for d in ("forward", "backward"):
    f, c = res[d + "_fused"], res[d + "_composed"]
    res[d + "_fused_minus_composed"] = round(f["median"] - c["median"], 1)
    res[d + "_fused_no_slower"] = bool(f["median"] <= c["median"] + (c["max"] - c["min"]))
res["agreement"] = agreement()
res["activation_MB"] = round(M * N * 2 / 1e6, 1)
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")
