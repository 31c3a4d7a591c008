"""The wide loss kernels with options against the plain ones, on the same buffers in one process:
fcmf_xent_fwd_ex / fcmf_xent_bwd_ex with label smoothing against fcmf_xent_fwd / fcmf_xent_bwd at the IAOG shape
(M rows of V = 64001 classes in a 64032-column bf16 buffer).  Device events, a warm-up of every kernel, the two versions
alternating inside each repetition.  Prints one JSON line (and writes it to --out when given).

    python tools/loss_bench.py [--rows 8192] [--reps 20] [--eps 0.1] [--weighted] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-aspect-category-sentiment-analysis_amd"))

from fcmf_framework import _hip as H  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--classes", type=int, default=64001)
    ap.add_argument("--ld", type=int, default=64032)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--eps", type=float, default=0.1)
    ap.add_argument("--weighted", action="store_true", help="class weights over the vocabulary as well (a float32 [V] vector)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = torch.device("cuda:0")
    M, V, ld = a.rows, a.classes, a.ld
    g = torch.Generator(device=dev).manual_seed(1)
    logits = (torch.randn((M, ld), device=dev, generator=g) * 3).bfloat16()
    d = torch.empty_like(logits)
    lb = torch.randint(0, V, (M,), device=dev, generator=g)
    lb[::9] = -100
    w = (torch.rand(V, device=dev, generator=g) + 0.5) if a.weighted else None
    rows = torch.empty((2, M), dtype=torch.float32, device=dev)
    nvalid = torch.zeros(1, dtype=torch.float32, device=dev)
    out = torch.empty(2, dtype=torch.float32, device=dev)
    one = torch.ones(1, dtype=torch.float32, device=dev)
    L, st, dt = H.lib(), H.stream(), H.dt(logits)
    p = H.ptr
    calls = {
        "fwd_plain": lambda: L.fcmf_xent_fwd(p(logits), ld, p(lb), p(rows[0]), p(nvalid), M, V, -100, dt, st),
        "fwd_ex": lambda: L.fcmf_xent_fwd_ex(p(logits), ld, p(lb), p(w), 0, p(rows[0]), p(rows[1]), M, V, 1, -100, a.eps, 0.0, dt, st),
        "bwd_plain": lambda: L.fcmf_xent_bwd(p(logits), ld, p(lb), p(d), ld, p(one), 1.0, M, V, -100, dt, st),
        "bwd_ex": lambda: L.fcmf_xent_bwd_ex(p(logits), ld, p(lb), p(w), 0, p(d), ld, p(out[1:]), p(one), M, V, 1, -100, a.eps, 0.0, dt, st),
        "reduce_ex": lambda: L.fcmf_xent_reduce_ex(p(rows[0]), p(rows[1]), M, 1, 1.0, p(out), p(out[1:]), st),
    }
    for name, f in calls.items():              # warm-up (fwd_ex and reduce_ex run before bwd_ex: its scale is real)
        for _ in range(3):
            H.check(f(), name)
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(a.reps):
        for name, f in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            H.check(f(), name)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3)
    med = {k: statistics.median(v) for k, v in times.items()}
    live = int((lb != -100).sum().item())
    row_bytes = live * V * 2                    # the bf16 logits of the live rows, once
    res = {"bench": "loss_wide", "rows": M, "live_rows": live, "classes": V, "ld": ld, "dtype": "bf16", "eps": a.eps, "weighted": a.weighted,
           "reps": a.reps, "median_us": {k: round(v, 1) for k, v in med.items()},
           "min_us": {k: round(min(v), 1) for k, v in times.items()}, "max_us": {k: round(max(v), 1) for k, v in times.items()},
           "fwd_ratio_ex_over_plain": round(med["fwd_ex"] / med["fwd_plain"], 3),
           "bwd_ratio_ex_over_plain": round(med["bwd_ex"] / med["bwd_plain"], 3),
           "fwd_ex_read_TBps": round(row_bytes / med["fwd_ex"] * 1e-6, 2), "fwd_plain_read_TBps": round(row_bytes / med["fwd_plain"] * 1e-6, 2),
           "loss": out[0].item()}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
