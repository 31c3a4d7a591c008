"""IAOG decode on the whole prefix, on the GPU: IAOGDecoder.decode_step_prefix (key cache + csrc/attn_decode.hip) against the
teacher-forced batch-1 decoder call whose last row defines it; decoding.beam_search_ids_batch(context="prefix") against the
oracle's beam search over the oracle decoder (oracle.beam_search_ids hands the whole sequence to its step function);
iaog_eval.generate and the pre-training driver in prefix mode.  Tiny model of test_decode_batch_gpu.py: H 64, 4 heads, 2 blocks,
V 512; every sample's encoder output is random (seeded per sample), never the synthetic batch's, which differs by 1.4e-4 between
samples only and would hide a mix-up.  Figures are printed before they are asserted."""
import os
import random

import pytest
import torch
import torch.nn.functional as F

import synthetic_data as synth
from oracle import fcmf_oracle as O
from test_decode_batch_gpu import NI, _args, _iaog_model, _run, _set
from helpers import make_hf_dir

pytestmark = pytest.mark.gpu

CFG = synth.TINY_CFG
V, HD = CFG["vocab_size"], CFG["hidden_size"]
TK = 1 + 2 * NI
TWIN_DEPTH = 12


def _enc(seeds):
    return torch.stack([torch.randn(TK, HD, generator=torch.Generator().manual_seed(s)) for s in seeds])


def _rounds(n, t, seed):
    """the rows of rounds 0 .. t of a made-up search over 3 samples, n rows per round: rows[p] = [(sample, seq, ancestors)] in the
    order the step sees them.  A row's parent is drawn with replacement from the round before (rows share parents: branching) and
    every round's rows are shuffled (a row's index says nothing about its parent's).  Two rows, the twins, stay in sample 0
    throughout; in round t they carry the same token 123 after histories that differ in the last TWIN_DEPTH positions (one
    differing position moves the last row of a long sequence too little to tell a mix-up from rounding): the same (sample, last token), told apart by
    history alone.  -> (rows, the twins' indices in round t or [])"""
    rng = random.Random(seed)
    twin = [0, 1] if n >= 2 else []                     # where the twins sit in the current round
    sample = [[0 if i < 2 else i % 3 for i in range(n)]]
    parent, twins = [None], [twin]
    for p in range(1, t + 1):
        par = [rng.randrange(n) for _ in range(n)]      # logical rows: 0 and 1 are the twins
        for i in range(len(twin)):
            par[i] = twin[i] if p > t - TWIN_DEPTH else rng.choice(twin)      # each twin its own line through the last rounds
        order = list(range(n))
        rng.shuffle(order)
        parent.append([par[i] for i in order])
        sample.append([sample[-1][j] for j in parent[-1]])
        twin = [order.index(i) for i in range(len(twin))]
        twins.append(twin)
    tok = [[rng.randrange(3, V) for _ in range(n)] for _ in range(t + 1)]
    if twin and t >= 1:
        for back in range(1, min(t, TWIN_DEPTH) + 1):
            tok[t - back][twins[t - back][0]], tok[t - back][twins[t - back][1]] = 5 + 2 * back, 43 + 2 * back      # (7, 45), (9, 47), ...
        tok[t][twin[0]] = tok[t][twin[1]] = 123
    rows = [[(sample[0][i], [tok[0][i]], []) for i in range(n)]]
    for p in range(1, t + 1):
        prev = rows[-1]
        rows.append([(sample[p][i], prev[j][1] + [tok[p][i]], prev[j][2] + [j]) for i, j in enumerate(parent[p])])
    return rows, (twin if t >= 1 else [])


def _check_rows(rows):
    """the made-up search is consistent: reading the tokens back through a row's ancestors gives its sequence"""
    for p, rs in enumerate(rows):
        for s, seq, anc in rs:
            assert len(seq) == p + 1 and [rows[q][a][1][-1] for q, a in enumerate(anc)] == seq[:-1]
            assert all(rows[q][a][0] == s for q, a in enumerate(anc))


def _play(dec, rows, enc, keys, k, dev):
    """rounds 0 .. t through decode_step_prefix with one cache -> the last round's (log-probabilities, ids)"""
    n = len(rows[0])
    cache = dec.init_cache(len(rows), n + 1, dev)
    for c in cache:
        c.fill_(float("nan"))                           # whatever a round does not write it must not read
    for p, rs in enumerate(rows):
        buf = torch.tensor([[r[0] for r in rs], [r[1][-1] for r in rs]] + [[r[2][q] for r in rs] for q in range(p)], device=dev)
        logp, ids = dec.decode_step_prefix(buf[1], buf[0], buf[2:].t(), p, cache, enc, keys, k)
    return logp.cpu(), ids.cpu()


def _teacher_forced(dec, enc, s, seq, dev):
    """log-softmax of the last row of the teacher-forced batch-1 call: the definition of the prefix step"""
    e = enc[s:s + 1]
    lg = dec(torch.tensor([seq], device=dev), dec.init_state(e, torch.ones(1, TK, device=dev)), is_train=True)
    return F.log_softmax(lg[0, -1].float(), dim=-1).cpu()


@pytest.mark.parametrize("t", [0, 1, 2, 7, 19])
@pytest.mark.parametrize("n", [1, 5, 13])
def test_prefix_step_rows_equal_the_teacher_forced_batch1_call(dev, n, t):
    model, _ = _iaog_model(dev, 1)
    dec = model.decoder
    K = 3
    _set(torch.float32)
    enc = _enc((100, 101, 102)).to(dev)
    rows, twin = _rounds(n, t, 10 * n + t)
    _check_rows(rows)
    with torch.no_grad():
        logp, ids = _play(dec, rows, enc, dec.project_encoder(enc), K, dev)
        ref = [_teacher_forced(dec, enc, s, seq, dev) for s, seq, _ in rows[t]]
    if twin and t >= 1:
        # the test's own discriminating power: same sample, same last token, another history
        (sa, qa, _), (sb, qb, _) = rows[t][twin[0]], rows[t][twin[1]]
        assert sa == sb and qa[-1] == qb[-1] and qa != qb
        gap = (ref[twin[0]] - ref[twin[1]]).abs().max().item()
        print(f"n {n} t {t}: reference rows that differ in history alone: max |d| {gap:.3e}")
        assert gap > 1e-3
    assert logp.shape == (n, K) and logp.dtype == torch.float32 and ids.dtype == torch.int32
    worst = 0.0
    for i in range(n):
        ws, wi = torch.topk(ref[i], K)
        assert ids[i].tolist() == wi.tolist(), (i, rows[t][i])
        worst = max(worst, (logp[i] - ws).abs().max().item())
    print(f"decode_step_prefix n {n} t {t}: top-{K} log-probabilities vs the teacher-forced batch-1 call, max |d| {worst:.3e}")
    assert worst < 1e-4


def _oracle_params(model):
    return {k: v.detach().float().cpu() for k, v in model.state_dict().items()}


def _oracle_logp(P, enc_cpu, s, seq):
    lg = O.iaog_decoder_forward(P, CFG, torch.tensor([seq]), enc_cpu[s:s + 1], training=False, is_train=True)
    return F.log_softmax(lg[0, -1].float(), dim=-1)


@pytest.mark.parametrize("n,t", [(13, 7), (5, 19)])
def test_prefix_step_bf16_is_as_close_to_the_oracle_as_the_teacher_forced_forward(dev, n, t):
    """e_hist = max |log p of the bf16 prefix step - the float32 CPU oracle| over the step's top-16 entries of every row; e_tf = the
    same for the existing bf16 teacher-forced forward's last row, at the same entries.  The two paths round the same tensors at the
    same places; the factor 2 covers the different summation order of the probability-weighted key sum.
    Measured on the MI355X: see DESIGN.md 5d."""
    from fcmf_framework import ops
    model, _ = _iaog_model(dev, 1)
    dec = model.decoder
    K = ops.TOPK_MAX
    P = _oracle_params(model)
    enc_cpu = _enc((100, 101, 102))
    rows, _ = _rounds(n, t, 10 * n + t)
    _set(torch.bfloat16)
    try:
        enc = enc_cpu.to(dev)
        with torch.no_grad():
            logp, ids = _play(dec, rows, enc, dec.project_encoder(enc), K, dev)
            tf = [_teacher_forced(dec, enc, s, seq, dev) for s, seq, _ in rows[t]]
    finally:
        _set(torch.float32)
    e_hist = e_tf = 0.0
    for i, (s, seq, _) in enumerate(rows[t]):
        want = _oracle_logp(P, enc_cpu, s, seq)[ids[i].long()]
        e_hist = max(e_hist, (logp[i] - want).abs().max().item())
        e_tf = max(e_tf, (tf[i][ids[i].long()] - want).abs().max().item())
    print(f"bf16 n {n} t {t}: e_hist {e_hist:.3e}  e_tf {e_tf:.3e}")
    assert torch.isfinite(logp).all()
    assert e_hist <= 2 * e_tf + 1e-4


def _oracle_search(P, enc_cpu, s, beam, max_len, sep):
    """oracle.beam_search_ids over the oracle decoder, and the smallest score gap at any of its pruning decisions: per round the
    beam-th against the (beam+1)-th best of ALL candidates (every live beam x every token: what decides the survivors), and the
    best finished sequence against the runner-up"""
    pools, score_of = {}, {(0,): 0.0}

    def step(seq):                                      # called once per live beam and round
        lp = _oracle_logp(P, enc_cpu, s, seq)
        mine = score_of[tuple(seq)]
        pools.setdefault(len(seq), []).append(mine + lp.double())
        for tok in torch.topk(lp, beam).indices.tolist():
            score_of[tuple(seq) + (tok,)] = mine + lp[tok].item()
        return lp

    ids, score, fin = O.beam_search_ids(step, 0, sep, beam_size=beam, max_len=max_len)
    gap = float("inf")
    for pool in pools.values():
        best = torch.cat(pool).sort(descending=True).values
        gap = min(gap, (best[beam - 1] - best[beam]).item())
    fs = sorted((f[0] for f in fin), reverse=True)
    if len(fs) > 1:
        gap = min(gap, fs[0] - fs[1])
    return ids, score, fin, gap


class _FixedEncoder(torch.nn.Module):
    def __init__(self, enc):
        super().__init__()
        self.enc = enc

    def forward(self, enc_ids, *a, **k):
        return self.enc[:enc_ids.shape[0]]


# per beam size: the encoder seeds of the three samples and max_len, chosen on the CPU so that every pruning decision of the
# oracle's search has a gap > 1e-2.  The tiny model's distributions are flat (log-probabilities of the best tokens within a few
# 1e-2 of each other): of 4400 seeds a handful reach 1e-2 at these lengths, none in a longer search of width 3.
SEARCHES = {2: ((489, 586, 448), 6), 3: ((1112, 1390, 3311), 3)}


@pytest.mark.parametrize("beam", [2, 3])
def test_prefix_beam_search_matches_the_oracle(dev, beam):
    from fcmf_framework import decoding
    seeds, max_len = SEARCHES[beam]
    model, batch = _iaog_model(dev, 3)
    P = _oracle_params(model)
    enc_cpu = _enc(seeds)
    want = [_oracle_search(P, enc_cpu, s, beam, max_len, 2) for s in range(3)]
    gap = min(w[3] for w in want)
    print(f"beam {beam}: the oracle's smallest gap at a pruning decision {gap:.3e}")
    assert gap > 1e-2
    _set(torch.float32)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(model, "encoder", _FixedEncoder(enc_cpu.to(dev)))
        got = decoding.beam_search_ids_batch(model, 0, 2, *_args(batch, slice(0, 3)), beam_size=beam, max_len=max_len, context="prefix")
        one = decoding.beam_search_ids(model, 0, 2, *[a[0] for a in _args(batch, slice(0, 3))], beam_size=beam, max_len=max_len,
                                       context="prefix")
    worst = 0.0
    for s in range(3):
        ids, score, fin, _ = want[s]
        assert got[s][0] == ids, (s, got[s][0], ids)
        worst = max(worst, abs(got[s][1] - score))
        assert len(got[s][2]) == len(fin)
        worst = max([worst] + [abs(a - b) for a, b in zip(sorted(f[0] for f in got[s][2]), sorted(f[0] for f in fin))])
    print(f"beam {beam}: scores vs the oracle, max |d| {worst:.3e}")
    assert worst < 1e-3
    assert one[0] == got[0][0] and one[1] == got[0][1]               # the unbatched entry point: the same path with one sample


def _batches(cfg, aspects):
    s0 = 0
    for B, seed in ((5, 21), (3, 22)):
        b = synth.synth_batch(B, cfg, S=16, num_imgs=NI, num_roi=5, num_aspects=1, seed=seed, coord_dtype=torch.float32)
        dec = torch.randint(3, cfg["vocab_size"], (B, 6), generator=torch.Generator().manual_seed(seed))
        lab = torch.roll(dec, -1, dims=1)
        lab[:, -1] = -100
        yield (b["visual_embeds_att"], b["roi_embeds_att"], b["roi_coors"], lab, dec, b["input_ids"][:, 0], b["token_type_ids"][:, 0],
               b["attention_mask"][:, 0], b["added_attention_mask"][:, 0], [aspects[(s0 + k) % 3] for k in range(B)],
               [f"synthetic review {s0 + k}" for k in range(B)])
        s0 += B


def test_generate_prefix_batched_equals_per_sample_and_differs_from_last(dev):
    from iaog_eval import generate
    model, _ = _iaog_model(dev, 1)
    tok = synth.IdTokenizer(dict(vocab_size=V, pad_token_id=CFG["pad_token_id"]))
    aspects = ["a", "b", "c"]
    _set(torch.float32)
    feats = lambda a, b: (a, b)
    one = generate(model, tok, _batches(CFG, aspects), feats, 2, 6, aspects, context="prefix")
    many = generate(model, tok, _batches(CFG, aspects), feats, 2, 6, aspects, batched=True, context="prefix")
    last = generate(model, tok, _batches(CFG, aspects), feats, 2, 6, aspects, batched=True)
    assert sum(len(v) for v in one[0].values()) == 8
    assert many == one
    assert many[0] != last[0]                                        # the whole prefix is another function than the last token


def test_driver_prefix_decode(tmp_path, dev, caplog, monkeypatch):
    """--decode_context prefix: every decode step of the run is a prefix step, none a batched last-token step, and the
    run writes its result files.  The driver's own model is freshly initialised and two steps old: its next token is decided by the
    current token's scaled embedding, against which positions and history weigh little, so both contexts decode the same text (as
    printed).  That the two contexts decode different text is asserted on `generate` above, with the synthetic parameters."""
    import run_pretraining_fcmf as drv
    from fcmf_framework.iaog_modeling import IAOGDecoder
    calls = {"decode_step_prefix": 0, "decode_step": 0}
    for name in calls:
        def spy(self, *a, _fn=getattr(IAOGDecoder, name), _name=name, **k):
            calls[_name] += 1
            return _fn(self, *a, **k)
        monkeypatch.setattr(IAOGDecoder, name, spy)
    hf = make_hf_dir(CFG)
    texts = {}
    for name, extra in (("last", ["--batched_decode"]), ("prefix", ["--decode_context", "prefix"])):
        for k in calls:
            calls[k] = 0
        out = str(tmp_path / name)
        msgs = _run(drv, out, hf, extra, caplog)
        assert any("[Macro-Avg] F1:" in m for m in msgs)
        path = os.path.join(out, "iaog_test_predictions_formatted.txt")
        assert os.path.exists(path) and os.path.exists(os.path.join(out, "pretraining_iaog.log"))
        lines = open(path, encoding="utf-8").read().split("\n")
        assert any(l.startswith("MACRO AVERAGE") for l in lines)
        texts[name] = [l for l in lines[lines.index("DETAILED PREDICTIONS (Filtered View):"):] if l.startswith("   predict:")]
        print(name, dict(calls), texts[name][:3])
        if name == "prefix":
            assert calls["decode_step_prefix"] > 0 and calls["decode_step"] == 0
        else:
            assert calls["decode_step"] > 0 and calls["decode_step_prefix"] == 0
    assert len(texts["prefix"]) == len(texts["last"]) > 0
