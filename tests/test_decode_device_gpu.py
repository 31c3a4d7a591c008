"""The device decode loop end to end on the real step (tiny model of test_decode_batch_gpu.py / test_decode_prefix_gpu.py, fp32):
loop="device" against loop="host" for beam search in both contexts and with constraints, for sampling (exactly), through
iaog_eval.generate and the pre-training driver; and that a device-loop call makes no host round trip per round.

Beam search compares with a bound, not `==`: the host loop runs fewer rows in the early rounds (and, in context "last", only the
rows its memo lacks), so the step's GEMMs have other shapes.  1e-4 is the project's bound for step rows against the teacher-forced
call (test_decode_prefix_gpu.py).  The searches are SEARCHES of that file, chosen so that every pruning decision of the oracle is
wider than 1e-2 -- re-asserted here -- so that a difference of 1e-4 cannot change a decision.  Figures are printed before they are
asserted."""
import os

import pytest
import torch

import synthetic_data as synth
from helpers import make_hf_dir
from test_decode_batch_gpu import _args, _iaog_model, _run, _set
from test_decode_prefix_gpu import CFG, SEARCHES, V, _batches, _enc, _FixedEncoder, _oracle_params, _oracle_search

pytestmark = pytest.mark.gpu

CONSTRAINTS = dict(no_repeat_ngram_size=2, repetition_penalty=1.3, min_length=3)


def _compare(name, host, device):
    worst = 0.0
    for s, (h, d) in enumerate(zip(host, device)):
        assert d[0] == h[0], (name, s, d[0], h[0])
        assert len(d[2]) == len(h[2]), (name, s)
        worst = max([worst, abs(d[1] - h[1])] + [abs(a - b) for a, b in zip(sorted(f[0] for f in d[2]), sorted(f[0] for f in h[2]))])
    print(f"{name}: device loop vs host loop, scores max |d| {worst:.3e} (exactly 0: {worst == 0.0})")
    assert worst < 1e-4


@pytest.mark.parametrize("beam", [2, 3])
def test_device_beam_search_matches_the_host_loop(dev, beam):
    from fcmf_framework import decoding
    seeds, max_len = SEARCHES[beam]
    model, batch = _iaog_model(dev, 3)
    enc_cpu = _enc(seeds)
    P = _oracle_params(model)
    gap = min(_oracle_search(P, enc_cpu, s, beam, max_len, 2)[3] for s in range(3))
    print(f"beam {beam}: the oracle's smallest gap at a pruning decision {gap:.3e}")
    assert gap > 1e-2
    _set(torch.float32)
    args = _args(batch, slice(0, 3))
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(model, "encoder", _FixedEncoder(enc_cpu.to(dev)))
        for context, cons in (("prefix", None), ("last", None), ("prefix", CONSTRAINTS)):
            kw = dict(beam_size=beam, max_len=max_len, context=context, constraints=cons)
            host = decoding.beam_search_ids_batch(model, 0, 2, *args, loop="host", **kw)
            got = {p: decoding.beam_search_ids_batch(model, 0, 2, *args, loop="device", poll_every=p, **kw) for p in (0, 4)}
            assert got[0] == got[4]
            _compare(f"beam {beam} {context}{' constrained' if cons else ''}", host, got[4])
        one = decoding.beam_search_ids(model, 0, 2, *[a[0] for a in args], beam_size=beam, max_len=max_len, context="prefix", loop="device")
        many = decoding.beam_search_ids_batch(model, 0, 2, *args, beam_size=beam, max_len=max_len, context="prefix", loop="device")
        assert one[0] == many[0][0] and abs(one[1] - many[0][1]) < 1e-4


@pytest.mark.parametrize("context", ["prefix", "last"])
@pytest.mark.parametrize("num_chains", [1, 3])
@pytest.mark.parametrize("seed", [0, 5])
def test_device_sampling_equals_the_host_loop_exactly(dev, seed, num_chains, context):
    """sep is suppressed, so no chain ever ends and the host loop runs the same R rows every round: tokens AND scores are equal"""
    from fcmf_framework import decoding
    model, batch = _iaog_model(dev, 3)
    _set(torch.float32)
    kw = dict(num_chains=num_chains, max_len=6, context=context, sampler=dict(seed=seed, temperature=0.9, top_k=40, top_p=0.95),
              sample_offset=11, constraints=dict(suppress_tokens=[2]))
    args = _args(batch, slice(0, 3))
    host = decoding.sample_ids_batch(model, 0, 2, *args, loop="host", **kw)
    for poll in (0, 4):
        got = decoding.sample_ids_batch(model, 0, 2, *args, loop="device", poll_every=poll, **kw)
        assert got == host
    assert all(len(q) == 7 and 2 not in q for _, _, chains in host for _, q in chains)
    if num_chains == 3:
        assert any(chains[0][1] != chains[1][1] for _, _, chains in host)       # chains are independent draws


def _count_round_trips(mp, fn):
    n = {"n": 0}

    def counted(real):
        def f(*a, **k):
            n["n"] += 1
            return real(*a, **k)
        return f

    for name in ("cpu", "tolist", "item"):
        mp.setattr(torch.Tensor, name, counted(getattr(torch.Tensor, name)))
    real_tensor = torch.tensor

    def tensor(*a, **k):
        if k.get("device") is not None:
            n["n"] += 1
        return real_tensor(*a, **k)

    mp.setattr(torch, "tensor", tensor)
    fn()
    return n["n"]


@pytest.mark.parametrize("strategy", ["beam", "beam_constrained", "sample"])
def test_no_round_trip_per_round(dev, strategy):
    """Tensor.cpu / .tolist / .item and torch.tensor(..., device=) inside a device-loop call with poll_every=0: as many for 6 rounds
    as for 3; the host loop, counted the same way, pays for every round"""
    from fcmf_framework import decoding
    model, batch = _iaog_model(dev, 3)
    _set(torch.float32)
    args = _args(batch, slice(0, 3))

    def call(loop, max_len):
        if strategy == "sample":
            return lambda: decoding.sample_ids_batch(model, 0, 2, *args, num_chains=2, max_len=max_len, context="prefix", loop=loop,
                                                     poll_every=0)
        return lambda: decoding.beam_search_ids_batch(model, 0, 2, *args, beam_size=2, max_len=max_len, context="prefix", loop=loop,
                                                      poll_every=0, constraints=CONSTRAINTS if strategy == "beam_constrained" else None)

    counts = {}
    for loop in ("device", "host"):
        for max_len in (3, 6):
            with pytest.MonkeyPatch.context() as mp:
                counts[(loop, max_len)] = _count_round_trips(mp, call(loop, max_len))
    print(f"{strategy}: host round trips by (loop, max_len): {counts}")
    assert counts[("device", 3)] == counts[("device", 6)]
    assert counts[("host", 6)] >= counts[("host", 3)] + 3                        # the counter does see a per-round trip


def test_generate_device_loop_equals_host_loop(dev):
    from iaog_eval import generate
    model, _ = _iaog_model(dev, 1)
    tok = synth.IdTokenizer(dict(vocab_size=V, pad_token_id=CFG["pad_token_id"]))
    aspects = ["a", "b", "c"]
    _set(torch.float32)
    feats = lambda a, b: (a, b)
    for kw in (dict(context="prefix"), dict(context="last"), dict(context="prefix", strategy="sample", num_chains=2, sampler=dict(seed=3))):
        host = generate(model, tok, _batches(CFG, aspects), feats, 2, 6, aspects, batched=True, loop="host", **kw)
        device = generate(model, tok, _batches(CFG, aspects), feats, 2, 6, aspects, loop="device", poll_every=2, **kw)
        assert sum(len(v) for v in host[0].values()) == 8
        assert device == host, kw


def test_driver_device_loop_writes_the_same_predictions(tmp_path, dev, caplog, monkeypatch):
    import run_pretraining_fcmf as drv
    from fcmf_framework import ops
    calls = {"beam_advance": 0}
    monkeypatch.setattr(ops, "beam_advance", lambda *a, _fn=ops.beam_advance, **k: (calls.__setitem__("beam_advance", calls["beam_advance"] + 1), _fn(*a, **k))[1])
    hf = make_hf_dir(CFG)
    files = {}
    for name, extra in (("host", ["--decode_context", "prefix", "--decode_loop", "host"]),
                        ("device", ["--decode_context", "prefix", "--decode_loop", "device", "--decode_poll_every", "2"])):
        calls["beam_advance"] = 0
        out = str(tmp_path / name)
        msgs = _run(drv, out, hf, extra, caplog)
        assert any("[Macro-Avg] F1:" in m for m in msgs)
        files[name] = open(os.path.join(out, "iaog_test_predictions_formatted.txt"), encoding="utf-8").read()
        assert (calls["beam_advance"] > 0) == (name == "device")
    # the whole file: the metric block and every prediction (both runs train the same two steps from the same seed)
    detail = {k: v[v.index("DETAILED PREDICTIONS (Filtered View):"):] for k, v in files.items()}
    print("prediction lines equal:", detail["device"] == detail["host"], "| whole files equal:", files["device"] == files["host"])
    assert "   predict:" in detail["host"]
    assert files["device"] == files["host"]
