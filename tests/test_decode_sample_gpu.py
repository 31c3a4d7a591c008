"""The sampling IAOG decode on the GPU: decoding.sample_ids_batch in both contexts (IAOGDecoder.decode_step / decode_step_prefix
ending in ops.vocab_sample, csrc/sample.hip) against tests/sampling_ref.sample_chains run over the ORACLE decoder -- per prefix
`oracle.iaog_decoder_forward(..., training=False, is_train=True)[0, -1]`, per last token the is_train=False call; the same samples
decoded as one batch and as two; the pre-training driver with --decode_strategy sample, and its beam output unchanged by the new
flags.  Tiny model of test_decode_prefix_gpu.py (H 64, 4 heads, 2 blocks, V 512), float32, a fixed random encoder output per sample.
Every draw of the oracle's run is asserted DECIDED (sampling_ref's header): the encoder seeds below were chosen on the CPU for
that.  Figures are printed before they are asserted."""
import os

import pytest
import torch

import rowwise_ref as R
import sampling_ref as S
import synthetic_data as synth
from oracle import fcmf_oracle as O
from helpers import make_hf_dir
from test_decode_batch_gpu import _args, _iaog_model, _run, _set
from test_decode_prefix_gpu import CFG, _enc, _FixedEncoder, _oracle_params

pytestmark = pytest.mark.gpu

CHAINS, MAX_LEN, START, SEP = 2, 8, 0, 2
SAMPLER = dict(seed=R.SEED_HI, temperature=0.7, top_k=50, top_p=0.9)
# the encoder seeds of the five samples per context: every draw of the oracle's chains is decided
ENC_SEEDS = {"last": (100, 101, 102, 103, 104), "prefix": (100, 101, 102, 103, 104)}
OFFSET = 7                                              # the batch's first sample is sample 7 of its eval set


def oracle_chains(P, enc_cpu, context):
    """sampling_ref.sample_chains over the oracle decoder for every sample -> ([chains per sample], all decided, smallest lead)"""
    out, all_ok, worst = [], True, float("inf")
    for s in range(enc_cpu.shape[0]):
        if context == "prefix":
            step = lambda seq: O.iaog_decoder_forward(P, CFG, torch.tensor([seq]), enc_cpu[s:s + 1], training=False, is_train=True)[0, -1].double().numpy()
        else:
            step = lambda seq: O.iaog_decoder_forward(P, CFG, torch.tensor([[seq[-1]]]), enc_cpu[s:s + 1], training=False, is_train=False)[0, -1].double().numpy()
        with torch.no_grad():
            chains, ok, lead = S.sample_chains(step, OFFSET + s, CHAINS, START, SEP, MAX_LEN, SAMPLER["seed"], SAMPLER["temperature"],
                                               SAMPLER["top_k"], SAMPLER["top_p"])
        out.append(chains)
        all_ok, worst = all_ok and ok, min(worst, lead)
    return out, all_ok, worst


@pytest.mark.parametrize("context", ["last", "prefix"])
def test_sampled_chains_match_the_oracle_and_do_not_depend_on_the_batch(dev, context):
    from fcmf_framework import decoding
    model, batch = _iaog_model(dev, 5)
    enc_cpu = _enc(ENC_SEEDS[context])
    want, ok, lead = oracle_chains(_oracle_params(model), enc_cpu, context)
    print(f"{context}: the oracle's smallest lead {lead:.3e}, every draw decided: {ok}")
    assert ok, "a draw of the oracle's run is not decided: choose other encoder seeds"
    _set(torch.float32)
    enc = enc_cpu.to(dev)

    def run(sl, offset):
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(model, "encoder", _FixedEncoder(enc[sl]))
            return decoding.sample_ids_batch(model, START, SEP, *_args(batch, sl), num_chains=CHAINS, max_len=MAX_LEN, context=context,
                                             sampler=SAMPLER, sample_offset=offset)

    got = run(slice(0, 5), OFFSET)
    worst = 0.0
    for s in range(5):
        ids, score, chains = got[s]
        assert [c[1] for c in chains] == [c[1] for c in want[s]], (s, chains, want[s])
        for (a, seq), (b, _) in zip(chains, want[s]):
            worst = max(worst, abs(a - b) / (len(seq) - 1))
        best = max(chains, key=lambda c: c[0])
        assert (score, ids) == best
    print(f"{context}: chain scores vs the oracle, max |d| per token {worst:.3e}")
    assert worst < 1e-4
    assert len({tuple(c[1]) for g in got for c in g[2]}) > 5           # the chains differ from each other
    split = run(slice(0, 2), OFFSET) + run(slice(2, 5), OFFSET + 2)
    assert [[c[1] for c in g[2]] for g in split] == [[c[1] for c in g[2]] for g in got]
    assert [g[0] for g in split] == [g[0] for g in got]


def test_length_penalty_on_the_device_paths(dev):
    """the beam search's finished list is the same with and without a penalty, and the choice is the penalised ranking of it"""
    from fcmf_framework import decoding
    model, batch = _iaog_model(dev, 3)
    _set(torch.float32)
    for context in ("last", "prefix"):
        zero = decoding.beam_search_ids_batch(model, 0, 2, *_args(batch, slice(0, 3)), beam_size=2, max_len=6, context=context)
        pen = decoding.beam_search_ids_batch(model, 0, 2, *_args(batch, slice(0, 3)), beam_size=2, max_len=6, context=context, length_penalty=1.0)
        for z, p in zip(zero, pen):
            assert p[2] == z[2]
            assert (p[1], p[0]) == max(p[2], key=lambda c: c[0] / max(len(c[1]) - 1, 1))


def _predictions(out):
    return open(os.path.join(out, "iaog_test_predictions_formatted.txt"), "rb").read()


def test_driver_sample_decode_and_unchanged_beam_output(tmp_path, dev, caplog, monkeypatch):
    """--decode_strategy sample runs one epoch on the tiny configuration, decodes through the sampling tail and writes the predictions
    file; the beam decode's predictions file is byte for byte the same with no new flag, with --decode_strategy beam, and with the
    defaults of every new flag spelled out"""
    import run_pretraining_fcmf as drv
    from fcmf_framework import ops
    calls = {"vocab_sample": 0, "vocab_topk": 0}
    for name in calls:
        def spy(*a, _fn=getattr(ops, name), _name=name, **k):
            calls[_name] += 1
            return _fn(*a, **k)
        monkeypatch.setattr(ops, name, spy)
    hf = make_hf_dir(synth.TINY_CFG)
    files = {}
    runs = (("plain", ["--batched_decode"]), ("beam", ["--batched_decode", "--decode_strategy", "beam"]),
            ("spelled", ["--batched_decode", "--decode_strategy", "beam", "--length_penalty", "0", "--temperature", "1", "--top_k", "0",
                         "--top_p", "1", "--num_chains", "1", "--sample_seed", "0"]),
            ("sample", ["--decode_strategy", "sample", "--top_p", "0.9", "--num_chains", "2", "--length_penalty", "1.0"]))
    for name, extra in runs:
        for k in calls:
            calls[k] = 0
        out = str(tmp_path / name)
        msgs = _run(drv, out, hf, extra, caplog)
        assert any("[Macro-Avg] F1:" in m for m in msgs)
        files[name] = _predictions(out)
        lines = files[name].decode("utf-8").split("\n")
        assert any(l.startswith("MACRO AVERAGE") for l in lines) and any(l.startswith("   predict:") for l in lines)
        print(name, dict(calls), [l for l in lines if l.startswith("   predict:")][:3])
        if name == "sample":
            assert calls["vocab_sample"] > 0 and calls["vocab_topk"] == 0
        else:
            assert calls["vocab_topk"] > 0 and calls["vocab_sample"] == 0
    assert files["beam"] == files["plain"] and files["spelled"] == files["plain"]
