"""Benchmark of the IAOG beam-search decode: the per-sample path (decoding.beam_search_ids, one batch-1 decoder call per new
(sample, last token)) next to the batched path (decoding.beam_search_ids_batch, one IAOGDecoder.decode_step per beam round for the
whole eval batch), on a synthetic FCMFSeq2Seq at the real geometry: H 768, 12 heads, 12 blocks, V 64001, 7 images, bf16,
--beam_size 2, --max_len_decoder 20, at 16 and 64 samples per batch.  Also the kernel alone: fcmf_logsoftmax_topk next to eager
log_softmax + topk on the same [n, 64032] bf16 buffer (V = 64001 columns valid).
"prefix": the batched path in both contexts (decoding.beam_search_ids_batch(context="last" | "prefix"): the memoised last-token
decode next to the decode on the whole prefix, which runs every live beam every round), and one cross-attention step of the prefix
decode fused (ops.decode_attention reading the hoisted keys through the sample index) next to composed (index_select of the rows'
keys + the attention forward the last-token step uses).  --only_prefix skips the other sections.
--strategy sample runs the sampling legs INSTEAD of the sections above: the kernel alone (fcmf_sample_token with top-k 50 + top-p 0.9,
with top-p 0.9 only and unfiltered, next to fcmf_logsoftmax_topk at k = beam_size and to an eager softmax / sort / cumsum / Gumbel
argmax composition, a yardstick only, all alternating on one [n, 64032] bf16 buffer), and in the decode: the prefix beam search
next to prefix sampling with num_chains = beam_size (decoding.sample_ids_batch) -- the same rows through the same blocks per round,
another tail kernel -- alternating, with sampling's median over the beam's.
--constraints runs the constraint legs INSTEAD of the sections above: the kernel alone (fcmf_logits_constrain with repetition penalty
1.3, no-repeat bigrams and a minimum length on sequences of 20 and of 512 tokens, next to fcmf_logsoftmax_topk, alternating on one
[n, 64032] bf16 buffer), and the prefix beam decode with constraints off next to the same decode with no_repeat_ngram_size=2,
repetition_penalty=1.3, min_length=5, alternating: constrained beams run longer by design, so the rounds run (decode_step_prefix
calls) and the time per round are reported beside the time per batch.
--loop runs the decode-loop legs INSTEAD of the sections above: the advance kernels alone (fcmf_beam_advance / fcmf_chain_advance on
the state of samples x beam_size slots, round max_len / 2, between device events), and the prefix decode with loop="host" (the
baseline: one upload and one blocking read per round) next to loop="device" at poll_every 0 and 4, alternating, for beam search and
for sampling (num_chains = beam_size): time per batch, rounds run (decode_step_prefix calls), time per round, and whether the legs
decoded the same sequences.
Usage (GPU box, repo root):  python tools/decode_bench.py [--samples 16 64] [--beam_size 2] [--max_len_decoder 20] [--only_prefix]
                                                          [--strategy sample] [--constraints] [--loop]
Prints one JSON line.  Decode: wall time per eval batch between device synchronisations, median of 5 (min, max beside it), both
paths warmed up once per batch size and alternating, the number of decoder calls of each path, and whether the two paths decoded
the same token sequences.  Kernel: median microseconds of 9 windows of 50 calls between device events, alternating."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.join(os.getcwd(), "multimodal-aspect-category-sentiment-analysis_amd"))
import torch
import torch.nn.functional as F

import synthetic_data as synth
from fcmf_framework import decoding, ops
from fcmf_framework.fcmf_pretraining import FCMFSeq2Seq
from fcmf_framework.roberta import RobertaConfig, RobertaModel

p = argparse.ArgumentParser()
p.add_argument("--samples", type=int, nargs="+", default=[16, 64])
p.add_argument("--beam_size", type=int, default=2)
p.add_argument("--max_len_decoder", type=int, default=20)
p.add_argument("--seq_len", type=int, default=64)
p.add_argument("--num_rois", type=int, default=4)
p.add_argument("--only_prefix", action="store_true")
p.add_argument("--strategy", default="beam", choices=("beam", "sample"))
p.add_argument("--constraints", action="store_true")
p.add_argument("--loop", action="store_true")
args = p.parse_args()

assert torch.cuda.is_available(), "decode_bench.py measures on the MI355X: no GPU, no number"
dev = torch.device("cuda:0")
cfg = synth.BASE_CFG
V, NI, SEP = cfg["vocab_size"], 7, 2
torch.manual_seed(0)
hf = tempfile.mkdtemp(prefix="hf_")
RobertaModel(RobertaConfig(**cfg)).save_pretrained(hf)
model = FCMFSeq2Seq(V, args.max_len_decoder, hf, NI, args.num_rois, 1.0).to(dev).eval()
ops.set_compute_dtype(torch.bfloat16)
dec = model.decoder

calls = {"forward": 0, "decode_step": 0}
_fwd, _step = dec.forward, dec.decode_step


def counted(name, fn):
    def run(*a, **k):
        calls[name] += 1
        return fn(*a, **k)
    return run


dec.forward, dec.decode_step = counted("forward", _fwd), counted("decode_step", _step)


def batch_args(B):
    b = synth.synth_batch(B, cfg, S=args.seq_len, num_imgs=NI, num_roi=args.num_rois, num_aspects=1, seed=B, coord_dtype=torch.float32)
    b = {k: v.to(dev) for k, v in b.items()}
    return (b["input_ids"][:, 0], b["attention_mask"][:, 0], b["token_type_ids"][:, 0], b["added_attention_mask"][:, 0],
            b["visual_embeds_att"], b["roi_embeds_att"], b["roi_coors"])


def per_sample(a):
    return [decoding.beam_search_ids(model, 0, SEP, *(t[i] for t in a), beam_size=args.beam_size, max_len=args.max_len_decoder)[0]
            for i in range(a[0].shape[0])]


def batched(a):
    return [r[0] for r in decoding.beam_search_ids_batch(model, 0, SEP, *a, beam_size=args.beam_size, max_len=args.max_len_decoder)]


def timed(fn, a):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn(a)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def stats(ts):
    return dict(median_ms=round(statistics.median(ts) * 1e3, 1), min_ms=round(min(ts) * 1e3, 1), max_ms=round(max(ts) * 1e3, 1))


res = {"geometry": dict(H=cfg["hidden_size"], heads=cfg["num_attention_heads"], blocks=cfg["num_hidden_layers"], V=V, num_imgs=NI,
                        dtype="bf16", beam_size=args.beam_size, max_len=args.max_len_decoder), "decode": [], "kernel": [], "prefix": []}
sampling = args.strategy == "sample"
if sampling:
    res["sample_kernel"], res["sample_decode"] = [], []
for B in ([] if args.only_prefix or sampling or args.loop else args.samples):
    a = batch_args(B)
    ids_one, ids_many = per_sample(a), batched(a)                         # warm-up of every shape of both paths
    times = {"per_sample": [], "batched": []}
    for _ in range(5):
        for k in calls:
            calls[k] = 0
        times["per_sample"].append(timed(per_sample, a)[0])
        n_one = dict(calls)
        for k in calls:
            calls[k] = 0
        times["batched"].append(timed(batched, a)[0])
        n_many = dict(calls)
    res["decode"].append({"samples_per_batch": B, "per_sample": stats(times["per_sample"]), "batched": stats(times["batched"]),
                          "decoder_calls": {"per_sample": n_one["forward"], "batched": n_many["decode_step"]},
                          "same_sequences": sum(x == y for x, y in zip(ids_one, ids_many)), "mean_len": sum(map(len, ids_many)) / B})

# ---- the kernel alone
Vp = (V + ops.VOCAB_PAD - 1) // ops.VOCAB_PAD * ops.VOCAB_PAD


def window(fn, reps=50):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3


def med(ts):
    return dict(us=round(statistics.median(ts), 1), us_min_max=[round(min(ts), 1), round(max(ts), 1)])


for n in (sorted({B * args.beam_size for B in args.samples}) if sampling else []):
    x = (torch.randn(n, Vp, generator=torch.Generator().manual_seed(n)) * 3).to(dev).bfloat16()
    ctr = torch.arange(n, device=dev)

    def eager_sample():                                   # temperature 1, top-p 0.9, one Gumbel draw: what the kernel replaces
        p_sorted, order = torch.sort(torch.softmax(x[:, :V].float(), dim=-1), dim=-1, descending=True)
        keep = torch.cumsum(p_sorted, dim=-1) - p_sorted < 0.9
        g = -torch.log(-torch.log(torch.rand_like(p_sorted)))
        return order.gather(1, torch.argmax(torch.where(keep, torch.log(p_sorted) + g, float("-inf")), dim=-1, keepdim=True))

    legs = {"sample_k50_p0.9": lambda: ops.sample_token(x, V, ctr, 1, top_k=50, top_p=0.9),
            "sample_p0.9": lambda: ops.sample_token(x, V, ctr, 1, top_p=0.9),
            "sample_unfiltered": lambda: ops.sample_token(x, V, ctr, 1),
            "topk": lambda: ops.logsoftmax_topk(x, V, args.beam_size), "eager": eager_sample}
    for fn in legs.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in legs}
    for _ in range(9):
        for k, fn in legs.items():
            t[k].append(window(fn))
    res["sample_kernel"].append({"rows": n, "ld": Vp, **{k: med(v) for k, v in t.items()}})

for B in (args.samples if sampling else []):
    a = batch_args(B)
    fns = {"beam_prefix": lambda a: [r[0] for r in decoding.beam_search_ids_batch(model, 0, SEP, *a, beam_size=args.beam_size,
                                                                                  max_len=args.max_len_decoder, context="prefix")],
           "sample_prefix": lambda a: [r[0] for r in decoding.sample_ids_batch(model, 0, SEP, *a, num_chains=args.beam_size,
                                                                               max_len=args.max_len_decoder, context="prefix",
                                                                               sampler=dict(seed=1, top_k=50, top_p=0.9))]}
    ids = {c: fn(a) for c, fn in fns.items()}             # warm-up of every shape of both
    times = {c: [] for c in fns}
    for _ in range(5):
        for c, fn in fns.items():
            times[c].append(timed(fn, a)[0])
    st = {c: stats(t) for c, t in times.items()}
    res["sample_decode"].append({"samples_per_batch": B, **st, "mean_len": {c: sum(map(len, v)) / B for c, v in ids.items()},
                                 "sample_over_beam": round(st["sample_prefix"]["median_ms"] / st["beam_prefix"]["median_ms"], 3)})
if sampling:
    print(json.dumps(res))
    sys.exit(0)

if args.constraints:
    res["constrain_kernel"], res["constrain_decode"] = [], []
    CONS = dict(no_repeat_ngram_size=2, repetition_penalty=1.3, min_length=5)
    for n in sorted({B * args.beam_size for B in args.samples}):
        x = (torch.randn(n, Vp, generator=torch.Generator().manual_seed(n)) * 3).to(dev).bfloat16()
        y = x.clone()                                     # the constraint legs edit in place: their own buffer
        hist = {L: torch.randint(0, V, (n, L), generator=torch.Generator().manual_seed(L)).to(dev) for L in (20, 512)}
        legs = {f"constrain_L{L}": (lambda L=L: ops.logits_constrain(y, V, hist[L], repetition_penalty=1.3, no_repeat_ngram_size=2,
                                                                     min_length=L + 1, sep_id=SEP)) for L in (20, 512)}
        legs["topk"] = lambda: ops.logsoftmax_topk(x, V, args.beam_size)
        for fn in legs.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in legs}
        for _ in range(9):
            for k, fn in legs.items():
                t[k].append(window(fn))
        res["constrain_kernel"].append({"rows": n, "ld": Vp, **{k: med(v) for k, v in t.items()}})
    rounds = {"n": 0}
    dec.decode_step_prefix = (lambda *a, _fn=dec.decode_step_prefix, **k: (rounds.__setitem__("n", rounds["n"] + 1), _fn(*a, **k))[1])
    for B in args.samples:
        a = batch_args(B)
        fns = {c: (lambda a, k=k: [r[0] for r in decoding.beam_search_ids_batch(model, 0, SEP, *a, beam_size=args.beam_size,
                                                                                 max_len=args.max_len_decoder, context="prefix", constraints=k)])
               for c, k in (("off", None), ("on", CONS))}
        ids = {c: fn(a) for c, fn in fns.items()}         # warm-up of every shape of both
        times, nr = {c: [] for c in fns}, {}
        for _ in range(5):
            for c, fn in fns.items():
                rounds["n"] = 0
                times[c].append(timed(fn, a)[0])
                nr[c] = rounds["n"]
        st = {c: dict(stats(t), rounds=nr[c], ms_per_round=round(statistics.median(t) * 1e3 / nr[c], 3)) for c, t in times.items()}
        res["constrain_decode"].append({"samples_per_batch": B, **st, "mean_len": {c: sum(map(len, v)) / B for c, v in ids.items()},
                                        "on_over_off_per_round": round(st["on"]["ms_per_round"] / st["off"]["ms_per_round"], 3)})
    print(json.dumps(res))
    sys.exit(0)

if args.loop:
    res["advance_kernel"], res["loop_decode"] = [], []
    W, L = args.beam_size, args.max_len_decoder
    for B in args.samples:
        g = torch.Generator().manual_seed(B)
        t = L // 2
        logp = -torch.rand(B * W, W, generator=g).to(dev)
        ids = torch.randint(SEP + 1, V, (B * W, W), generator=g).int().to(dev)        # never sep: no sample is ever done
        beams, chains = ops.advance_state(B, W, L, 0, dev), ops.advance_state(B, W, L, 0, dev, chains=True)
        beams["state"].fill_(ops.SLOT_LIVE)
        logp1, ids1 = logp[:, 0].contiguous(), ids[:, 0].contiguous()
        legs = {"beam_advance": lambda: ops.beam_advance(logp, ids, beams, t, SEP),
                "chain_advance": lambda: ops.chain_advance(logp1, ids1, chains, t, SEP)}
        for fn in legs.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        tm = {k: [] for k in legs}
        for _ in range(9):
            for k, fn in legs.items():
                tm[k].append(window(fn))
        res["advance_kernel"].append({"samples": B, "rows": B * W, "round": t, **{k: med(v) for k, v in tm.items()}})
    rounds = {"n": 0}
    dec.decode_step_prefix = (lambda *a, _fn=dec.decode_step_prefix, **k: (rounds.__setitem__("n", rounds["n"] + 1), _fn(*a, **k))[1])

    def beam_leg(**kw):
        return lambda a: [r[0] for r in decoding.beam_search_ids_batch(model, 0, SEP, *a, beam_size=W, max_len=L, context="prefix", **kw)]

    def sample_leg(**kw):
        return lambda a: [r[0] for r in decoding.sample_ids_batch(model, 0, SEP, *a, num_chains=W, max_len=L, context="prefix",
                                                                  sampler=dict(seed=1, top_k=50, top_p=0.9), **kw)]

    for B in args.samples:
        a = batch_args(B)
        for strategy, leg in (("beam", beam_leg), ("sample", sample_leg)):
            fns = {"host": leg(loop="host"), "device_poll0": leg(loop="device", poll_every=0), "device_poll4": leg(loop="device", poll_every=4)}
            out = {c: fn(a) for c, fn in fns.items()}     # warm-up of every shape of all three
            times, nr = {c: [] for c in fns}, {}
            for _ in range(5):
                for c, fn in fns.items():
                    rounds["n"] = 0
                    times[c].append(timed(fn, a)[0])
                    nr[c] = rounds["n"]
            st = {c: dict(stats(tt), rounds=nr[c], ms_per_round=round(statistics.median(tt) * 1e3 / nr[c], 3)) for c, tt in times.items()}
            res["loop_decode"].append({"strategy": strategy, "samples_per_batch": B, "rows": B * W, **st,
                                       "same_sequences": {c: sum(x == y for x, y in zip(out["host"], out[c])) for c in fns if c != "host"},
                                       "device_over_host": {c: round(st[c]["median_ms"] / st["host"]["median_ms"], 3) for c in fns if c != "host"}})
    print(json.dumps(res))
    sys.exit(0)

for n in ([] if args.only_prefix else sorted({B * args.beam_size for B in args.samples})):
    x = (torch.randn(n, Vp, generator=torch.Generator().manual_seed(n)) * 3).to(dev).bfloat16()
    kernel = lambda: ops.logsoftmax_topk(x, V, args.beam_size)
    eager = lambda: torch.topk(F.log_softmax(x[:, :V].float(), dim=-1), args.beam_size)
    for fn in (kernel, eager):
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    t = {"kernel": [], "eager": []}
    for _ in range(9):
        t["kernel"].append(window(kernel))
        t["eager"].append(window(eager))
    (kl, ki), (el, ei) = kernel(), eager()
    res["kernel"].append({"rows": n, "ld": Vp, "k": args.beam_size,
                          "kernel_us": round(statistics.median(t["kernel"]), 1), "kernel_us_min_max": [round(min(t["kernel"]), 1), round(max(t["kernel"]), 1)],
                          "eager_us": round(statistics.median(t["eager"]), 1), "eager_us_min_max": [round(min(t["eager"]), 1), round(max(t["eager"]), 1)],
                          "same_ids": bool(torch.equal(ki.long(), ei)), "max_abs_diff": float((kl - el).abs().max())})

# ---- the whole prefix next to the last token
def in_context(context):
    return lambda a: [r[0] for r in decoding.beam_search_ids_batch(model, 0, SEP, *a, beam_size=args.beam_size,
                                                                   max_len=args.max_len_decoder, context=context)]


for B in args.samples:
    a = batch_args(B)
    fns = {c: in_context(c) for c in ("last", "prefix")}
    ids = {c: fn(a) for c, fn in fns.items()}                             # warm-up of every shape of both
    times = {c: [] for c in fns}
    for _ in range(5):
        for c, fn in fns.items():
            times[c].append(timed(fn, a)[0])
    res["prefix"].append({"samples_per_batch": B, **{c: stats(t) for c, t in times.items()},
                          "same_sequences": sum(x == y for x, y in zip(ids["last"], ids["prefix"])),
                          "mean_len": {c: sum(map(len, v)) / B for c, v in ids.items()}})

from fcmf_framework.iaog_modeling import _quirk_attn_fwd
nh, Tk = cfg["num_attention_heads"], 1 + 2 * NI
for B in args.samples:
    n, g = B * args.beam_size, torch.Generator().manual_seed(B)
    kx = torch.randn(B, Tk, cfg["hidden_size"], generator=g).to(dev).bfloat16()
    qx = torch.randn(n, cfg["hidden_size"], generator=g).to(dev).bfloat16()
    sample = torch.arange(n, device=dev) // args.beam_size
    fused = lambda: ops.decode_attention(qx, kx, sample, nh, Tk, Tk, pos_dim=1)
    composed = lambda: _quirk_attn_fwd(qx.view(n, 1, -1), kx.index_select(0, sample), nh, False, head_quirk=0)
    for fn in (fused, composed):
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    t = {"fused": [], "composed": []}
    for _ in range(9):
        t["fused"].append(window(fused))
        t["composed"].append(window(composed))
    res["prefix"].append({"cross_attention_rows": n, "keys": Tk,
                          "fused_us": round(statistics.median(t["fused"]), 1), "fused_us_min_max": [round(min(t["fused"]), 1), round(max(t["fused"]), 1)],
                          "composed_us": round(statistics.median(t["composed"]), 1),
                          "composed_us_min_max": [round(min(t["composed"]), 1), round(max(t["composed"]), 1)],
                          "max_abs_diff": float((fused().float() - composed()[0].view(n, -1).float()).abs().max())})
print(json.dumps(res))
