"""The two kernels of the FGM adversary at the benchmark step's shape, 384 sequences x 170 tokens x 768 columns in
bf16, beside the file's streaming yardsticks over the same element count: fcmf_dropout (one read, one write) and the plain
fcmf_embed_ln_fwd.  Device events, a warm-up of every kernel, the kernels alternating inside each repetition.  Bytes are counted
from the shapes: the activation-sized operands each kernel must move once (the float32 table rows the embedding kernels gather
are left out: 50 distinct ids, resident in cache).  Prints one JSON line (and writes it to --out when given).

    python tools/adv_kernels_bench.py [--reps 20] [--out FILE]
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = torch.device("cuda:0")
    nseq, S, Hd, pad, dtype = 384, 170, 768, 1, torch.bfloat16
    ntok = nseq * S
    gen = torch.Generator(device=dev).manual_seed(1)
    ids = torch.randint(2, 50, (nseq, S), device=dev, generator=gen)
    ids[:, S - 20:] = pad                      # a padded tail, as real reviews have
    m = ids.ne(pad).long()
    pos = torch.cumsum(m, 1) * m + pad
    word, ptab, ttab = (torch.randn(s, device=dev, generator=gen) for s in ((50, Hd), (S + 2, Hd), (2, Hd)))
    gamma, beta = torch.ones(Hd, device=dev), torch.zeros(Hd, device=dev)
    g = torch.randn((ntok, Hd), device=dev, generator=gen).to(dtype)
    y, z, x = torch.empty_like(g), torch.empty_like(g), torch.empty_like(g)
    mean, rstd = torch.empty(ntok, device=dev), torch.empty(ntok, device=dev)
    scale = torch.empty(nseq, device=dev)
    L, st, dt, p = H.lib(), H.stream(), H.dt(g), H.ptr
    emb = (p(ids), p(pos), None, p(word), p(ptab), p(ttab), p(gamma), p(beta), p(y), p(z), p(mean), p(rstd), ntok, Hd, 1e-5, 0.1, 12345,
           dt, st)
    calls = {
        "adv_scale": lambda: L.fcmf_adv_scale(p(g), p(ids), p(scale), nseq, S, Hd, pad, 0.5, dt, st),
        "embed_ln_adv_fwd": lambda: L.fcmf_embed_ln_adv_fwd(*emb, p(g), p(scale), S, pad),
        "embed_ln_fwd": lambda: L.fcmf_embed_ln_fwd(*emb),
        "dropout": lambda: L.fcmf_dropout(p(g), p(x), g.numel(), 0.1, 12345, dt, st),
    }
    act = ntok * Hd * 2                        # one activation-sized bf16 operand
    live = float(m.float().mean())
    needed = {"adv_scale": act * live, "embed_ln_adv_fwd": act * (2 + live), "embed_ln_fwd": act * 2, "dropout": act * 2}
    for name, f in calls.items():
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
    res = {"bench": "adv_kernels", "shape": [nseq, S, Hd], "dtype": "bf16", "live_token_fraction": round(live, 3), "reps": a.reps}
    for k, v in times.items():
        med = statistics.median(v)
        res[k] = {"median_us": round(med, 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2),
                  "needed_MB": round(needed[k] / 1e6, 2), "needed_TBps": round(needed[k] / med * 1e-6, 3)}
    res["adv_scale"]["note"] = "reads every live row twice (maximum, then squares); needed counts it once"
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
