"""fcmf_multi_adamw_ema against fcmf_multi_adamw on the benchmark model's parameter set, and one FusedAdamW.ema_weights() entry
plus exit.  Both update kernels run on the same tables (parameters, gradients, moments, bf16 shadows of the 2-D
weights as in a bf16 step) in one process, alternating inside each repetition, after a warm-up of each; device events.  Nothing
is flushed between calls: the working set (28 / 36 bytes per parameter, ~3-4 GB) is an order of magnitude beyond the 256 MiB last-level
cache, so every call streams from HBM.  Prints one JSON line (and writes it to --out when given).

    python tools/ema_bench.py [--reps 20] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "multimodal-aspect-category-sentiment-analysis_amd"))

import bench  # noqa: E402
from fcmf_framework import _hip as H  # noqa: E402
from fcmf_framework import ops  # noqa: E402
from fcmf_framework.optimization import FusedAdamW  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = torch.device("cuda:0")
    model = bench.fcmf_initial_model(bench.BASE_CFG, 7, 7).to(dev)
    opt = FusedAdamW(bench.param_groups(model), lr=7e-4)
    opt.set_ema(0.999)
    g = torch.Generator(device=dev).manual_seed(1)
    params = [p for grp in opt.param_groups for p in grp["params"]]
    for p in params:
        p.grad = torch.randn(p.shape, device=dev, generator=g) * 1e-3
        if p.dim() == 2:
            ops.shadows.get(p)              # the bf16 copy a bf16 step keeps: the update kernels refresh it
            if max(p.shape) <= 4096:        # (a linear layer, not an embedding table)
                ops.shadows.get_t(p)        # the transposed copy its dX GEMM reads: rebuilt on leaving ema_weights()
    opt.step(max_grad_norm=1.0)             # builds the tables, the moments and the averages
    T, L, st = opt._tables, H.lib(), H.stream()
    n = int(T["sizes"].sum().item())
    shadowed = sum(p.numel() for p in params if ops.shadows.peek(p) is not None)
    ng = len(opt.param_groups)
    lr = (ctypes.c_float * 8)(*[float(x["lr"]) for x in opt.param_groups] + [0.0] * (8 - ng))
    wd = (ctypes.c_float * 8)(*[float(x["weight_decay"]) for x in opt.param_groups] + [0.0] * (8 - ng))
    p = H.ptr
    common = lambda step: (p(T["p"]), p(T["g_ptrs"]), p(T["m"]), p(T["v"]), p(T["sh_ptrs"]), p(T["sizes"]), p(T["group"]), p(T["ct"]),
                           p(T["co"]), T["nchunks"], opt.CHUNK, lr, wd, ng, 0.9, 0.999, 1e-8, step, p(opt._sumsq), 1.0, st)
    step = [2]

    def plain():
        H.check(L.fcmf_multi_adamw(*common(step[0])), "fcmf_multi_adamw")
        step[0] += 1

    def ema():
        H.check(L.fcmf_multi_adamw_ema(*common(step[0]), p(T["e"]), 0.999), "fcmf_multi_adamw_ema")
        step[0] += 1

    def block():
        with opt.ema_weights():
            pass

    calls = {"adamw": plain, "adamw_ema": ema, "ema_weights_enter_exit": block}
    for f in calls.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(a.reps):
        for name, f in calls.items():
            times[name].append(timed(f))
    med = {k: statistics.median(v) for k, v in times.items()}
    by_plain, by_ema = 28 * n + 2 * shadowed, 36 * n + 2 * shadowed
    res = {"bench": "adamw_ema", "parameters": n, "tensors": len(params), "chunks": T["nchunks"], "bf16_shadowed_parameters": shadowed,
           "reps": a.reps, "median_us": {k: round(v, 1) for k, v in med.items()},
           "min_us": {k: round(min(v), 1) for k, v in times.items()}, "max_us": {k: round(max(v), 1) for k, v in times.items()},
           "ratio_ema_over_plain": round(med["adamw_ema"] / med["adamw"], 3),
           "byte_ratio_expected": round(by_ema / by_plain, 3),
           "adamw_TBps": round(by_plain / med["adamw"] * 1e-6, 2), "adamw_ema_TBps": round(by_ema / med["adamw_ema"] * 1e-6, 2),
           "swap_pair_bytes": 2 * (16 * n + 2 * shadowed)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
