"""Micro-benchmark of the row passes of the flagship step: fcmf_colsum at [49152, 768] and [21952, 768] bf16 and [384, 2304] f32,
fcmf_add_ln_fwd and fcmf_add_ln_bwd (with workspace: the main kernel plus its reduce pass) at [49152, 768] bf16, p = 0.1, with
residual.  30 launches between two HIP events, three alternating runs; prints us per call and GB/s of the bytes a call must move.
Usage (GPU box, repo root):
    python tools/rowpass_bench.py [--lib path/to/libfcmf_hip.so]
An explicit library allows a same-box A/B of two builds with one script."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.getcwd(), "multimodal-aspect-category-sentiment-analysis_amd"))
import torch
from fcmf_framework import _hip as H

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=None)
a = ap.parse_args()
if a.lib:
    H.LIB_PATH = os.path.abspath(a.lib)
L = H.lib()
dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(0)
st = H.stream()


def timeit(fn, reps=30):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


cases = []
for M, N, dt in ((49152, 768, torch.bfloat16), (21952, 768, torch.bfloat16), (384, 2304, torch.float32)):
    x = torch.randn(M, N, generator=g).to(dt).to(dev)
    out = torch.zeros(N, device=dev)
    cases.append(("colsum [%d, %d] %s" % (M, N, "bf16" if dt == torch.bfloat16 else "f32"), x.numel() * x.element_size(),
                  lambda x=x, out=out, M=M, N=N: H.check(L.fcmf_colsum(H.ptr(x), H.ptr(out), M, N, N, H.dt(x), 1, st), "fcmf_colsum")))

rows, Hd, p = 49152, 768, 0.1
x, res, dy = ((torch.randn(rows, Hd, generator=g) * s).bfloat16().to(dev) for s in (1.0, 1.0, 0.1))
gamma, beta = torch.ones(Hd, device=dev), torch.zeros(Hd, device=dev)
y, z, dz, dx = (torch.empty_like(x) for _ in range(4))
mean, rstd = torch.empty(rows, device=dev), torch.empty(rows, device=dev)
dgamma, dbeta, dxsum = (torch.zeros(Hd, device=dev) for _ in range(3))
ws = torch.empty(L.fcmf_add_ln_bwd_workspace(rows, Hd), device=dev)
row_bytes = rows * Hd * 2
cases.append(("add_ln_fwd [%d, %d] bf16" % (rows, Hd), 4 * row_bytes,          # x, res in; y, z out
              lambda: H.check(L.fcmf_add_ln_fwd(H.ptr(x), H.ptr(res), Hd, H.ptr(gamma), H.ptr(beta), H.ptr(y), H.ptr(z), H.ptr(mean),
                                                H.ptr(rstd), rows, Hd, 1e-12, p, 1234, H.BF16, st), "fcmf_add_ln_fwd")))
cases.append(("add_ln_bwd [%d, %d] bf16" % (rows, Hd), 4 * row_bytes,          # dy, z in; dz, dx out
              lambda: H.check(L.fcmf_add_ln_bwd(H.ptr(dy), H.ptr(z), H.ptr(gamma), H.ptr(mean), H.ptr(rstd), H.ptr(dz), H.ptr(dx),
                                                H.ptr(dgamma), H.ptr(dbeta), H.ptr(dxsum), H.ptr(ws), rows, Hd, p, 1234, H.BF16, st),
                              "fcmf_add_ln_bwd")))
cases[3][2]()           # z, mean, rstd for the backward
times = [[timeit(fn) for _, _, fn in cases] for _ in range(3)]
print(os.path.basename(os.path.dirname(H.LIB_PATH)), "(us per call, three runs; GB/s of the best)")
for i, (name, nbytes, _) in enumerate(cases):
    t = [run[i] for run in times]
    print("  %-34s %7.1f %7.1f %7.1f   %7.0f GB/s" % (name, t[0], t[1], t[2], nbytes / min(t) * 1e-3))
