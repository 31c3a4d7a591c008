"""The constrained IAOG decode on the GPU: decoding.beam_search_ids_batch / sample_ids_batch with `constraints=` in both contexts
(csrc/constrain.hip between the vocabulary GEMM and the tails) against the oracle's loops -- oracle.beam_search_ids /
sampling_ref.sample_chains -- over the ORACLE decoder with the constrained step of tests/constraints_ref.py; one batch of five
against two and three; the off path; the pre-training driver's flags.  Tiny model of test_decode_prefix_gpu.py (H 64, 4 heads, 2
blocks, V 512), float32, a fixed random encoder output per sample.

Ids must be equal and scores within 1e-4.  The encoder seeds and max_len of `SEARCHES` / `CHAINS_AT` were chosen on the CPU with
the oracle so that (a) every pruning decision and every draw of the constrained reference is decided by 1e-2, 100 times the score
bound, (b) the unconstrained reference decode of the same samples gives another id sequence for at least half of them; both are
recomputed and asserted here, and (c) is asserted on the device result: no repeated bigram under no_repeat_ngram_size=2, no
separator before position max_len under min_length=max_len.  Figures are printed before they are asserted."""
import collections
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import constraints_ref as C
import rowwise_ref as R
import sampling_ref as S
import synthetic_data as synth
from oracle import fcmf_oracle as O
from helpers import make_hf_dir
from test_decode_batch_gpu import _args, _iaog_model, _run, _set
from test_decode_prefix_gpu import CFG, _enc, _FixedEncoder, _oracle_params

pytestmark = pytest.mark.gpu

START, SEP = 0, 2
TOL, DECIDED = 1e-4, 1e-2
NGRAM = dict(no_repeat_ngram_size=2, repetition_penalty=1.3)
# a sharp sampler: the tiny model's distributions are flat (the best tokens within a few 1e-2 of each other), and chains drawn from 50
# of 512 near-equal tokens never repeat one within a few rounds, so no constraint would change them
SAMPLER = dict(seed=R.SEED_HI, temperature=0.05, top_k=4, top_p=0.9)
NCHAINS, OFFSET = 2, 7


def minlen(max_len, tokens):
    return dict(min_length=max_len, suppress_tokens=tuple(tokens))


def _logits(P, enc_cpu, s, context):
    """the oracle decoder's step of sample s: seq -> logits [V] (float32 torch), on the whole prefix or on the last token"""
    if context == "prefix":
        return lambda seq: O.iaog_decoder_forward(P, CFG, torch.tensor([seq]), enc_cpu[s:s + 1], training=False, is_train=True)[0, -1].float()
    return lambda seq: O.iaog_decoder_forward(P, CFG, torch.tensor([[seq[-1]]]), enc_cpu[s:s + 1], training=False, is_train=False)[0, -1].float()


def beam_reference(P, enc_cpu, s, beam, max_len, context, cfg):
    """oracle.beam_search_ids over the (constrained, when cfg) oracle step, and the smallest score gap at any of its pruning
    decisions, as test_decode_prefix_gpu._oracle_search computes it -> (ids, score, finished, gap)"""
    raw = _logits(P, enc_cpu, s, context)
    logp = C.constrained_step(raw, SEP, as_logprobs=True, **cfg) if cfg else (lambda seq: F.log_softmax(raw(seq), dim=-1))
    pools, score_of = {}, {(START,): 0.0}

    def step(seq):                                      # called once per live beam and round
        lp = logp(seq)
        mine = score_of[tuple(seq)]
        pools.setdefault(len(seq), []).append(mine + lp.double())
        for tok in torch.topk(lp, beam).indices.tolist():
            score_of[tuple(seq) + (tok,)] = mine + lp[tok].item()
        return lp

    with torch.no_grad():
        ids, score, fin = O.beam_search_ids(step, START, SEP, beam_size=beam, max_len=max_len)
    gap = float("inf")
    for pool in pools.values():
        best = torch.cat(pool).sort(descending=True).values
        gap = min(gap, (best[beam - 1] - best[beam]).item())
    fs = sorted((f[0] for f in fin), reverse=True)
    if len(fs) > 1:
        gap = min(gap, fs[0] - fs[1])
    return ids, score, fin, gap


def chain_reference(P, enc_cpu, s, max_len, context, cfg):
    """sampling_ref.sample_chains over the (constrained) oracle step for sample s of the batch -> (chains, decided, smallest lead)"""
    raw = _logits(P, enc_cpu, s, context)
    step = C.constrained_step(raw, SEP, **cfg) if cfg else (lambda seq: raw(seq).double().numpy())
    with torch.no_grad():
        return S.sample_chains(step, OFFSET + s, NCHAINS, START, SEP, max_len, SAMPLER["seed"], SAMPLER["temperature"], SAMPLER["top_k"],
                               SAMPLER["top_p"])


def frequent_tokens(seqs, k=8):
    """the k tokens that decodes produce most often (the lower id among equals), the most frequent first, the start token aside"""
    count = collections.Counter(t for seq in seqs for t in seq[1:])
    return sorted(count, key=lambda t: (-count[t], t))[:k]


def check_property(setting, seqs, max_len, tokens):
    """(c): what the constraint promises, on sequences the DEVICE returned"""
    for seq in seqs:
        if setting == "ngram":
            assert not C.has_repeated_ngram(seq, 2), seq
        else:
            assert SEP not in seq[1:max_len] and not set(tokens) & set(seq[1:]), (seq, tokens)


# (beam width, context, setting) / (context, setting) -> (the encoder seeds of the five samples, max_len, what "minlen" suppresses).
# The suppressed tokens are the most frequent ones, the model's most frequent first, of the unconstrained reference decodes of the
# encoder seeds 0 .. 63 in that context (`frequent_tokens` of them, computed when the table was made): token 93 in context "last",
# where the decodes of all seeds share it; a few more in context "prefix", where they share less.
SEARCHES = {
    (2, "last", "ngram"): ((17, 1446, 1488, 1731, 2000), 4, None),
    (2, "last", "minlen"): ((37, 102, 113, 130, 164), 4, (93,)),
    (2, "prefix", "ngram"): ((0, 3, 5, 6, 9), 4, None),
    (2, "prefix", "minlen"): ((1686, 5931, 6461, 7829, 8103), 4, (93, 169, 19, 34)),
    (3, "last", "ngram"): ((377, 397, 557, 1156, 2375), 3, None),
    (3, "last", "minlen"): ((1034, 1343, 1942, 2342, 4000), 3, (93,)),
    (3, "prefix", "ngram"): ((15587, 25711, 26527, 37183, 73), 3, None),
    (3, "prefix", "minlen"): ((1252, 1983, 3776, 3816, 4940), 3, (93,)),
}
CHAINS_AT = {
    ("last", "ngram"): ((102, 116, 132, 148, 164), 6, None),
    ("last", "minlen"): ((100, 116, 132, 148, 164), 6, (93, 73, 19, 170, 225, 338, 234, 327)),
    ("prefix", "ngram"): ((100, 116, 132, 148, 164), 6, None),
    ("prefix", "minlen"): ((100, 116, 132, 149, 164), 6, (169, 93, 34, 45, 225, 330)),
}


def _beam_case(model, P, beam, context, setting):
    seeds, max_len, token = SEARCHES[(beam, context, setting)]
    enc_cpu = _enc(seeds)
    free = [beam_reference(P, enc_cpu, s, beam, max_len, context, None) for s in range(len(seeds))]
    cfg = NGRAM if setting == "ngram" else minlen(max_len, token)
    want = [beam_reference(P, enc_cpu, s, beam, max_len, context, cfg) for s in range(len(seeds))]
    return enc_cpu, max_len, cfg, token, free, want


@pytest.mark.parametrize("setting", ["ngram", "minlen"])
@pytest.mark.parametrize("context", ["last", "prefix"])
@pytest.mark.parametrize("beam", [2, 3])
def test_constrained_beam_search_matches_the_oracle(dev, beam, context, setting):
    from fcmf_framework import decoding
    model, batch = _iaog_model(dev, 5)
    enc_cpu, max_len, cfg, token, free, want = _beam_case(model, _oracle_params(model), beam, context, setting)
    gap = min(w[3] for w in want)
    differ = sum(f[0] != w[0] for f, w in zip(free, want))
    print(f"beam {beam} {context} {setting} {cfg}: the constrained oracle's smallest gap at a pruning decision {gap:.3e}; "
          f"{differ} of 5 samples decode differently without the constraint")
    assert gap > DECIDED, "a pruning decision of the oracle's search is not decided: choose other encoder seeds"
    assert 2 * differ >= 5
    _set(torch.float32)
    enc = enc_cpu.to(dev)

    def run(sl):
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(model, "encoder", _FixedEncoder(enc[sl]))
            return decoding.beam_search_ids_batch(model, START, SEP, *_args(batch, sl), beam_size=beam, max_len=max_len, context=context,
                                                  constraints=cfg)

    got = run(slice(0, 5))
    worst = 0.0
    for s in range(5):
        ids, score, fin, _ = want[s]
        assert got[s][0] == ids, (s, got[s][0], ids)
        assert [f[1] for f in got[s][2]] == [f[1] for f in fin], s
        worst = max([worst, abs(got[s][1] - score)] + [abs(a[0] - b[0]) for a, b in zip(got[s][2], fin)])
        check_property(setting, [got[s][0]] + [f[1] for f in got[s][2]], max_len, token)
    print(f"beam {beam} {context} {setting}: scores vs the oracle, max |d| {worst:.3e} (bound {TOL})")
    assert worst < TOL
    assert run(slice(0, 2)) + run(slice(2, 5)) == got                # one batch of 5 equals 2 + 3
    with pytest.MonkeyPatch.context() as mp:                          # the unbatched entry point: the batched path with one sample
        mp.setattr(model, "encoder", _FixedEncoder(enc[:1]))
        one = decoding.beam_search_ids(model, START, SEP, *[a[0] for a in _args(batch, slice(0, 1))], beam_size=beam, max_len=max_len,
                                       context=context, constraints=cfg)
    assert one == got[0]


@pytest.mark.parametrize("setting", ["ngram", "minlen"])
@pytest.mark.parametrize("context", ["last", "prefix"])
def test_constrained_sampling_matches_the_oracle(dev, context, setting):
    from fcmf_framework import decoding
    model, batch = _iaog_model(dev, 5)
    P = _oracle_params(model)
    seeds, max_len, token = CHAINS_AT[(context, setting)]
    enc_cpu = _enc(seeds)
    free = [chain_reference(P, enc_cpu, s, max_len, context, None)[0] for s in range(5)]
    cfg = NGRAM if setting == "ngram" else minlen(max_len, token)
    want = [chain_reference(P, enc_cpu, s, max_len, context, cfg) for s in range(5)]
    ok, lead = all(w[1] for w in want), min(w[2] for w in want)
    differ = sum([c[1] for c in f] != [c[1] for c in w[0]] for f, w in zip(free, want))
    print(f"sample {context} {setting} {cfg}: the constrained oracle's smallest lead {lead:.3e}, every draw decided: {ok}; "
          f"{differ} of 5 samples decode differently without the constraint")
    assert ok and lead >= DECIDED, "a draw of the oracle's run is not decided: choose other encoder seeds"
    assert 2 * differ >= 5
    _set(torch.float32)
    enc = enc_cpu.to(dev)

    def run(sl, offset):
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(model, "encoder", _FixedEncoder(enc[sl]))
            return decoding.sample_ids_batch(model, START, SEP, *_args(batch, sl), num_chains=NCHAINS, max_len=max_len, context=context,
                                             sampler=SAMPLER, sample_offset=offset, constraints=cfg)

    got = run(slice(0, 5), OFFSET)
    worst = 0.0
    for s in range(5):
        ids, score, chains = got[s]
        assert [c[1] for c in chains] == [c[1] for c in want[s][0]], (s, chains, want[s][0])
        worst = max([worst] + [abs(a[0] - b[0]) for a, b in zip(chains, want[s][0])])
        assert (score, ids) == max(chains, key=lambda c: c[0])
        check_property(setting, [c[1] for c in chains], max_len, token)
    print(f"sample {context} {setting}: chain scores vs the oracle, max |d| {worst:.3e} (bound {TOL})")
    assert worst < TOL
    assert run(slice(0, 2), OFFSET) + run(slice(2, 5), OFFSET + 2) == got      # one batch of 5 equals 2 + 3


def test_constraints_off_run_no_new_code(dev, monkeypatch):
    """constraints=None and an all-off dict: ops.logits_constrain is never called, and ids and scores are those of a call without
    the argument; with a constraint on it is called once per round"""
    from fcmf_framework import decoding, ops
    calls = []
    monkeypatch.setattr(ops, "logits_constrain", lambda *a, _fn=ops.logits_constrain, **k: (calls.append(1), _fn(*a, **k))[1])
    model, batch = _iaog_model(dev, 3)
    _set(torch.float32)
    args = _args(batch, slice(0, 3))
    off = dict(repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0, suppress_tokens=())
    for context in ("last", "prefix"):
        beam = lambda **k: decoding.beam_search_ids_batch(model, START, SEP, *args, beam_size=2, max_len=5, context=context, **k)
        chain = lambda **k: decoding.sample_ids_batch(model, START, SEP, *args, num_chains=2, max_len=5, context=context, sampler=SAMPLER, **k)
        for fn in (beam, chain):
            plain = fn()
            assert fn(constraints=None) == plain and fn(constraints=off) == plain and fn(constraints={}) == plain
            assert not calls
            on = fn(constraints=dict(no_repeat_ngram_size=1))
            assert 1 <= len(calls) <= 5 and on != plain
            calls.clear()
    with pytest.raises(ValueError, match="vocabulary"):
        decoding.beam_search_ids_batch(model, START, SEP, *args, beam_size=2, max_len=5, constraints=dict(suppress_tokens=range(505)))
    with pytest.raises(ValueError, match="max_len"):
        decoding.sample_ids_batch(model, START, SEP, *args, max_len=513, constraints=dict(min_length=2))


def _predictions(out):
    return open(os.path.join(out, "iaog_test_predictions_formatted.txt"), "rb").read()


def test_driver_constraint_flags(tmp_path, dev, caplog, monkeypatch):
    """the new flags reach iaog_eval.generate and the kernel; a bad value stops the run before training with the flag named; a run
    with the defaults spelled out writes the predictions file of a run without the flags, byte for byte"""
    import iaog_eval
    import run_pretraining_fcmf as drv
    from fcmf_framework import ops
    seen, calls = [], []
    monkeypatch.setattr(iaog_eval, "generate", lambda *a, _fn=iaog_eval.generate, **k: (seen.append(k.get("constraints")), _fn(*a, **k))[1])
    monkeypatch.setattr(ops, "logits_constrain", lambda *a, _fn=ops.logits_constrain, **k: (calls.append(1), _fn(*a, **k))[1])
    hf = make_hf_dir(synth.TINY_CFG)
    with pytest.raises(ValueError, match="--repetition_penalty"):
        _run(drv, str(tmp_path / "bad"), hf, ["--repetition_penalty", "0"], caplog)
    with pytest.raises(ValueError, match="--min_length_decoder"):
        _run(drv, str(tmp_path / "bad"), hf, ["--min_length_decoder", "7"], caplog)      # ARGS: --max_len_decoder 6
    assert not (tmp_path / "bad").exists() and not seen
    files = {}
    runs = (("plain", ["--batched_decode"]),
            ("spelled", ["--batched_decode", "--repetition_penalty", "1.0", "--no_repeat_ngram_size", "0", "--min_length_decoder", "0"]),
            ("on", ["--repetition_penalty", "1.3", "--no_repeat_ngram_size", "2", "--min_length_decoder", "4", "--suppress_tokens", "5", "9"]))
    for name, extra in runs:
        seen.clear(); calls.clear()
        out = str(tmp_path / name)
        msgs = _run(drv, out, hf, extra, caplog)
        assert any("[Macro-Avg] F1:" in m for m in msgs)
        files[name] = _predictions(out)
        print(name, seen[:1], len(calls))
        if name == "on":
            assert seen and all(c == dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_length=4, suppress_tokens=(5, 9)) for c in seen)
            assert calls
        else:
            assert seen and all(c is None for c in seen) and not calls
    assert files["spelled"] == files["plain"]
    # (the driver's model is freshly initialised and two steps old: its six-token decodes rarely repeat a token, so the constrained
    # run may well write the same text; that constraints change a decode is asserted above, on the synthetic parameters)
