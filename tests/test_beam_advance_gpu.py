"""Beam and chain bookkeeping on the device (csrc/beam.hip: fcmf_beam_advance / fcmf_chain_advance behind
decoding.beam_rounds_device / sample_rounds_device) against the unchanged host loops, EXACTLY: a scripted step reads lookup tables
indexed by (sample, token at position t), all log-probabilities multiples of 2^-6, so every sum is exact, ties are exact and the
comparison is `==` on ids, scores and the whole finished list in its order.

Vocabulary: 7 tokens (start 0, sep 2) for beam sizes up to 3.  A row of `ids` holds distinct tokens and never the start token
(which stands at position 0 only); 7 tokens cannot give 8 beams that, and the sample that never finishes needs 8 distinct tokens
beside start and sep, so beam size 8 runs on 10 tokens, the smallest vocabulary that can.

The tables are built per sample from TABLE_SEED; samples 2 and 3 of a five-sample batch are shaped (done in round 1 / never
emits sep).  `test_tables_exercise_every_rule` needs no GPU: it asserts on the HOST loop's trace that the tables produce every
situation the kernel has a rule for, so that the GPU comparisons cannot pass vacuously."""
import ctypes
import random

import pytest
import torch

gpu = pytest.mark.gpu

START, SEP = 0, 2
TABLE_SEED = 31      # chosen on the CPU: test_tables_exercise_every_rule holds (about one seed in fifteen does)
BS, WS, LENS = (1, 5), (1, 2, 3, 8), (1, 4, 20)


def _vs(W):
    return 7 if W <= 3 else 10


def _tables(B, W, seed=TABLE_SEED):
    """logp float32 [B, Vs, W] (multiples of 2^-6 in [-1, 0], descending along k as a top-k gives them) and ids int32 [B, Vs, W]
    (distinct per row).  Few distinct values: ties are common.  Of five samples, sample 2 never offers sep after the start token
    and then sep first at 0 with everything else 4 below (all beams end in round 1), sample 3 never offers sep."""
    Vs = _vs(W)
    rng = random.Random(1000 * seed + 10 * B + W)
    logp = torch.zeros(B, Vs, W)
    ids = torch.zeros(B, Vs, W, dtype=torch.int32)
    every = [v for v in range(Vs) if v != START]
    no_sep = [v for v in every if v != SEP]
    for b in range(B):
        for v in range(Vs):
            vals = sorted((-rng.randrange(0, 9) / 8.0 - rng.randrange(0, 2) / 64.0 for _ in range(W)), reverse=True)
            toks = rng.sample(every, W)
            if B == 5 and b == 3:
                toks = rng.sample(no_sep, W)
            if B == 5 and b == 2:
                if v == START:
                    toks = rng.sample(no_sep, W)
                else:
                    toks = [SEP] + rng.sample(no_sep, W - 1)
                    vals = [0.0] + [x - 4.0 for x in vals[1:]]
            logp[b, v] = torch.tensor(vals)
            ids[b, v] = torch.tensor(toks, dtype=torch.int32)
    return logp, ids


def _host_step(logp, ids):
    lp, ii = logp.tolist(), ids.tolist()
    return lambda pairs: {p: (lp[p[0]][p[1]], ii[p[0]][p[1]]) for p in pairs}


def _host_beams(B, W, max_len, length_penalty, trace=None):
    """decoding.beam_rounds in memo mode on the tables; trace: a list that receives one record per `_advance` call"""
    from fcmf_framework import decoding
    logp, ids = _tables(B, W)
    if trace is None:
        return decoding.beam_rounds(_host_step(logp, ids), B, START, SEP, W, max_len, length_penalty=length_penalty)
    real = decoding._advance
    finals = []                                               # the samples' `final` lists, by identity, in sample order

    def spy(beams, final, tops, sep_id, beam_size):
        if not any(final is f for f in finals):
            finals.append(final)
        b = next(i for i, f in enumerate(finals) if f is final)
        cands = sorted((score + tops(j, seq)[0][k] for j, (score, seq) in enumerate(beams) if seq[-1] != sep_id for k in range(beam_size)),
                       reverse=True)
        out = real(beams, final, tops, sep_id, beam_size)
        trace.append(dict(b=b, t=len(beams[0][1]) - 1, cands=cands, out=out, final_len=len(final)))
        return out

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(decoding, "_advance", spy)
        return decoding.beam_rounds(_host_step(logp, ids), B, START, SEP, W, max_len, length_penalty=length_penalty)


def test_tables_exercise_every_rule():
    """on the host reference's trace (no GPU): B 5, W 3, max_len 20 meets every situation; the permutation, the repeated parent and
    the tie are also met at W 2 and 8, so that no beam size is compared on trivial rounds only"""
    B, W, max_len = 5, 3, 20
    trace = []
    res = _host_beams(B, W, max_len, 0.0, trace)
    adv = [r for r in trace if r["out"] is not None]
    tie = [r for r in adv if len(r["cands"]) > W and r["cands"][W - 1] == r["cands"][W]]
    perm = [r for r in adv if sorted(r["out"][1]) == list(range(W)) and r["out"][1] != list(range(W))]
    dup = [r for r in adv if len(set(r["out"][1])) < W]
    last_t = {b: max(r["t"] for r in trace if r["b"] == b) for b in range(B)}
    assert tie, "an exact score tie across the pruning boundary"
    assert perm, "surviving beams whose parents are a non-identity permutation"
    assert dup, "one parent filling several slots"
    assert any(len(fin) > W for _, _, fin in res), "a sample with more than W finished hypotheses"
    # a sample that finishes nothing: its result is its beams, all max_len + 1 tokens long and none ended before the last position
    nothing = [b for b, (_, _, fin) in enumerate(res) if all(len(s) == max_len + 1 and SEP not in s[:-1] for _, s in fin) and len(fin) == W]
    assert 3 in nothing
    assert last_t[2] == 1 and max(last_t.values()) >= 3, "a sample done in round 1 while others run on"
    # ended in the last round, but `final` is non-empty: the ended beam is not in the result
    quirk = [r for r in adv if r["t"] == max_len - 1 and r["final_len"] > 0 and any(s[-1] == SEP for _, s in r["out"][0])
             and not all(s[-1] == SEP for _, s in r["out"][0])]
    assert quirk, "a beam that ended in the last round of a sample whose finished list is non-empty"
    for r in quirk:
        ended = [s for _, s in r["out"][0] if s[-1] == SEP]
        assert all(s not in [f[1] for f in res[r["b"]][2]] for s in ended)
    for w in (2, 8):
        trace = []
        _host_beams(5, w, 20, 0.0, trace)
        adv = [r for r in trace if r["out"] is not None]
        assert any(len(r["cands"]) > w and r["cands"][w - 1] == r["cands"][w] for r in adv), w
        assert any(sorted(r["out"][1]) == list(range(w)) and r["out"][1] != list(range(w)) for r in adv), w
        assert any(len(set(r["out"][1])) < w for r in adv), w


_REF = {}


def _ref(B, W, max_len, lp):
    key = (B, W, max_len, lp)
    if key not in _REF:
        _REF[key] = _host_beams(B, W, max_len, lp)
    return _REF[key]


@gpu
@pytest.mark.parametrize("poll_every", [0, 1, 4])
@pytest.mark.parametrize("length_penalty", [0.0, 1.0])
@pytest.mark.parametrize("max_len", LENS)
@pytest.mark.parametrize("W", WS)
@pytest.mark.parametrize("B", BS)
def test_device_beam_rounds_equal_the_host_loop(dev, B, W, max_len, length_penalty, poll_every):
    from fcmf_framework import decoding
    logp, ids = (x.to(dev) for x in _tables(B, W))
    sidx = torch.arange(B * W, device=dev) // W
    fed = []

    def step(tokens, t, anc, hist):
        assert tokens.shape == (B * W,) and tokens.is_contiguous() and anc.shape == (B * W, t) and hist.shape == (B * W, t + 1)
        fed.append(tokens.clone())
        return logp[sidx, tokens], ids[sidx, tokens]

    got, st = decoding.beam_rounds_device(step, B, START, SEP, W, max_len, "last", length_penalty, None, dev, poll_every,
                                          return_state=True)
    want = _ref(B, W, max_len, length_penalty)
    assert len(got) == B
    for b in range(B):
        assert got[b][0] == want[b][0], (b, got[b][0], want[b][0])
        assert got[b][1] == want[b][1], (b, got[b][1], want[b][1])
        assert got[b][2] == want[b][2], (b, got[b][2], want[b][2])           # the whole finished list, scores and order included
    # the ancestor table: position p of slot r was fed to the step in round p as row anc[p, r], of the same sample
    rounds = len(fed)
    assert rounds == max_len if poll_every == 0 else rounds <= max_len
    fed = torch.stack(fed).cpu()
    seq, anc = st["seq"].cpu(), st["anc"].cpu()
    assert ((anc[:rounds] >= 0) & (anc[:rounds] < B * W)).all()
    assert torch.equal(torch.gather(fed, 1, anc[:rounds]), seq[:rounds])
    assert torch.equal(anc[:rounds] // W, (torch.arange(B * W) // W).expand(rounds, -1))
    assert ((seq >= 0) & (seq < _vs(W))).all()                              # every row of every round ran on a valid token


def _sampler_tables(B, C=11):
    """scripted sampler: (log-probability, token) by (sample, token at position t, counter mod C); sep is drawn often enough that
    chains end at different rounds"""
    rng = random.Random(77 + B)
    logp = torch.tensor([[[-rng.randrange(0, 64) / 64.0 for _ in range(C)] for _ in range(7)] for _ in range(B)])
    ids = torch.tensor([[[rng.choice((1, 3, 4, 5, 6, SEP)) for _ in range(C)] for _ in range(7)] for _ in range(B)], dtype=torch.int32)
    return logp, ids, C


@gpu
@pytest.mark.parametrize("poll_every", [0, 1, 4])
@pytest.mark.parametrize("length_penalty", [0.0, 1.0])
@pytest.mark.parametrize("max_len", LENS)
@pytest.mark.parametrize("W", WS)
@pytest.mark.parametrize("B", BS)
def test_device_chains_equal_the_host_loop(dev, B, W, max_len, length_penalty, poll_every):
    from fcmf_framework import decoding
    logp, ids, C = _sampler_tables(B)
    lp, ii = logp.tolist(), ids.tolist()
    offset = 3
    want = decoding.sample_rounds(lambda rows: [(lp[b][tok][n % C], ii[b][tok][n % C]) for b, tok, n in rows], B, START, SEP, W, max_len,
                                  sample_offset=offset, length_penalty=length_penalty)
    if B == 5 and W >= 3 and max_len == 20:
        lens = {len(s) for _, _, chains in want for _, s in chains}
        assert len(lens) >= 3, lens                                          # chains that end at different rounds
    logp, ids = logp.to(dev), ids.to(dev)
    sidx = torch.arange(B * W, device=dev) // W
    fed = []

    def step(tokens, t, anc, hist, ctr):
        assert ctr.dtype == torch.int64 and ctr.shape == (B * W,)
        fed.append(tokens.clone())
        return logp[sidx, tokens, ctr % C], ids[sidx, tokens, ctr % C]

    got, st = decoding.sample_rounds_device(step, B, START, SEP, W, max_len, "last", offset, length_penalty, None, dev, poll_every,
                                            return_state=True)
    assert got == want
    rounds = len(fed)
    assert torch.equal(st["anc"][:rounds].cpu(), torch.arange(B * W).expand(rounds, -1))
    assert torch.equal(torch.stack(fed).cpu(), st["seq"][:rounds].cpu())


@gpu
def test_poll_stops_early_with_the_same_result(dev):
    """sample 2's tables alone (all beams end in round 1): with a poll the loop stops before max_len"""
    from fcmf_framework import decoding
    logp, ids = (x[2:3].contiguous().to(dev) for x in _tables(5, 3))
    W, n = 3, []

    def step(tokens, t, anc, hist):
        n.append(t)
        return logp[0, tokens], ids[0, tokens]

    res = {}
    for poll in (0, 1, 4):
        del n[:]
        res[poll] = decoding.beam_rounds_device(step, 1, START, SEP, W, 20, device=dev, poll_every=poll)
        assert len(n) == {0: 20, 1: 2, 4: 4}[poll]
    assert res[0] == res[1] == res[4] and len(res[0][0][2]) >= W


def test_limits_are_refused_before_any_launch():
    from fcmf_framework import decoding, ops
    step = lambda *a: pytest.fail("the step must not run")
    for kw in (dict(beam_size=9), dict(max_len=512), dict(beam_size=0), dict(max_len=0)):
        with pytest.raises(ValueError):
            decoding.beam_rounds_device(step, 2, START, SEP, **kw)
    for kw in (dict(num_chains=9), dict(max_len=512)):
        with pytest.raises(ValueError):
            decoding.sample_rounds_device(step, 2, START, SEP, **kw)
    with pytest.raises(ValueError):
        ops.advance_state(2, 9, 20, START, "cpu")


def test_c_entry_points_refuse_bad_arguments():
    """the error codes of the header, on host buffers: every refusal comes before a launch, so no GPU is needed"""
    from fcmf_framework import _hip
    lib = _hip.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)

    def beam(B=2, W=3, t=0, max_len=4, ld=3, null=False):
        return lib.fcmf_beam_advance(None if null else p, p, ld, B, W, t, max_len, SEP, p, p, p, p, p, p, p, p, p, None)

    def chain(B=2, W=3, t=0, max_len=4, null=False):
        return lib.fcmf_chain_advance(None if null else p, p, B, W, t, max_len, SEP, p, p, p, p, p, p, None)

    for fn in (beam, chain):
        assert fn(W=9) == _hip.ERR_UNSUPPORTED and fn(W=0) == _hip.ERR_UNSUPPORTED
        assert fn(max_len=512) == _hip.ERR_UNSUPPORTED and fn(max_len=0) == _hip.ERR_UNSUPPORTED
        assert fn(null=True) == _hip.ERR_ARG and fn(B=-1) == _hip.ERR_ARG and fn(t=-1) == _hip.ERR_ARG and fn(t=4) == _hip.ERR_ARG
        assert fn(B=0) == 0                                                  # nothing to do: no launch
    assert beam(ld=2) == _hip.ERR_ARG
