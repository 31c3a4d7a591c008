"""The symmetric-KL (R-Drop) kernels at the two shapes the drivers give them: 384 pairs x 4 columns float32 (FCMF:
64 reviews x 6 aspects) and 2048 pairs x 64001 columns bf16 in 64032-column buffers (the IAOG vocabulary), with
fcmf_xent_fwd_ex / fcmf_xent_bwd_ex over the same 2 x pairs rows beside the wide shape.  Device events, a warm-up of every
kernel, the kernels alternating inside each repetition.  The narrow kernels run for a few microseconds, so each of their samples
is a train of --train launches between two events, divided by its length.  Bytes are counted from the shapes: `needed` = every
operand once (forward 2 rows, backward 2 rows in + 2 out, acc also 2 destinations in), `issued` = what the kernels load and
store (the backward reads the two rows twice).  Prints one JSON line (and writes it to --out when given).

    python tools/symkl_bench.py [--reps 20] [--train 50] [--out FILE]
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


def shape_calls(dev, n, C, ld, dtype, segments, with_xent):
    g = torch.Generator(device=dev).manual_seed(1)
    both = (torch.randn((2 * n, ld), device=dev, generator=g) * 2).to(dtype)      # the two passes stacked, as the vocabulary node holds them
    a, b = both[:n], both[n:]
    d = torch.zeros_like(both)
    da, db = d[:n], d[n:]
    lb = torch.randint(0, C, (2 * n,), device=dev, generator=g)
    rows = torch.empty((2, 2 * n), dtype=torch.float32, device=dev)
    out = torch.empty(1 + segments, dtype=torch.float32, device=dev)
    one = torch.ones(1, dtype=torch.float32, device=dev)
    L, st, dt, p = H.lib(), H.stream(), H.dt(both), H.ptr
    calls = {
        "symkl_fwd": lambda: L.fcmf_symkl_fwd(p(a), ld, p(b), ld, p(lb), p(rows[0]), p(rows[1]), n, C, segments, -100, dt, st),
        "reduce": lambda: L.fcmf_xent_reduce_ex(p(rows[0]), p(rows[1]), n, segments, 1.0, p(out), p(out[1:]), st),
        "symkl_bwd": lambda: L.fcmf_symkl_bwd(p(a), ld, p(b), ld, p(lb), p(da), ld, p(db), ld, p(out[1:]), p(one), n, C, segments, -100, 0, dt, st),
        "symkl_bwd_acc": lambda: L.fcmf_symkl_bwd(p(a), ld, p(b), ld, p(lb), p(da), ld, p(db), ld, p(out[1:]), p(one), n, C, segments, -100, 1, dt, st),
    }
    if with_xent:
        xr = torch.empty((2, 2 * n), dtype=torch.float32, device=dev)
        xo = torch.empty(2, dtype=torch.float32, device=dev)
        calls["xent_fwd_ex"] = lambda: L.fcmf_xent_fwd_ex(p(both), ld, p(lb), None, 0, p(xr[0]), p(xr[1]), 2 * n, C, 1, -100, 0.1, 0.0, dt, st)
        calls["xent_reduce"] = lambda: L.fcmf_xent_reduce_ex(p(xr[0]), p(xr[1]), 2 * n, 1, 1.0, p(xo), p(xo[1:]), st)
        calls["xent_bwd_ex"] = lambda: L.fcmf_xent_bwd_ex(p(both), ld, p(lb), None, 0, p(d), ld, p(xo[1:]), p(one), 2 * n, C, 1, -100, 0.1, 0.0, dt, st)
    return calls, (both, d, lb, rows, out, one)


def measure(calls, reps, train):
    for name, f in calls.items():              # warm-up, in an order that gives the backward a real scale
        for _ in range(3):
            H.check(f(), name)
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(reps):
        for name, f in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(train):
                H.check(f(), name)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / train)
    return times


def report(times, n, C, es, skip=("reduce", "xent_reduce")):
    row = n * C * es                           # one operand: n rows of C elements
    needed = {"symkl_fwd": 2 * row, "symkl_bwd": 4 * row, "symkl_bwd_acc": 6 * row, "xent_fwd_ex": 2 * row, "xent_bwd_ex": 4 * row}
    issued = {"symkl_fwd": 2 * row, "symkl_bwd": 6 * row, "symkl_bwd_acc": 8 * row, "xent_fwd_ex": 2 * row, "xent_bwd_ex": 6 * row}
    res = {}
    for k, v in times.items():
        med = statistics.median(v)
        res[k] = {"median_us": round(med, 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
        if k not in skip:
            res[k].update(needed_MB=round(needed[k] / 1e6, 3), needed_TBps=round(needed[k] / med * 1e-6, 3),
                          issued_TBps=round(issued[k] / med * 1e-6, 3))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--train", type=int, default=50, help="launches per sample of the narrow shape")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = torch.device("cuda:0")
    res = {"bench": "symkl", "reps": a.reps}
    calls, keep = shape_calls(dev, 384, 4, 4, torch.float32, 6, False)
    res["narrow_384x4_f32"] = dict(train=a.train, **report(measure(calls, a.reps, a.train), 384, 4, 4))
    del calls, keep
    calls, keep = shape_calls(dev, 2048, 64001, 64032, torch.bfloat16, 1, True)
    res["wide_2048x64001_bf16"] = dict(train=1, **report(measure(calls, a.reps, 1), 2048, 64001, 2))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
