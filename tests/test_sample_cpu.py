"""The sampling decode without a GPU: tests/sampling_ref.py (the float64 statement of fcmf_sample_token's contract) against
hand-worked rows; the contract's hash as a sampler (empirical frequencies); the host loop decoding.sample_rounds on scripted steps
of both contexts against sampling_ref.sample_chains; the length penalty of the beam and sampling loops; the driver's new flags."""
import math

import numpy as np
import pytest
import torch

import rowwise_ref as R
import sampling_ref as S
from oracle import fcmf_oracle as O
from test_decode_batch_cpu import BEAM, MAX_LEN, SEP, START, _tables
from test_surface import PUBLISHED_PRETRAIN, REF_PRETRAIN_FLAGS, _argv

NINF = float("-inf")


def kept(x, T=1.0, top_k=0, top_p=1.0):
    K, _, M = S.filtered(np.array(x, dtype=np.float64), T, top_k, top_p)
    with np.errstate(invalid="ignore"):
        return np.nonzero(K)[0].tolist(), np.nonzero(K & ((M < top_p) | (top_p >= 1.0)))[0].tolist()


# ---- the reference against hand-worked rows ---------------------------------------------------------------------------------
def test_top_k_keeps_every_tie_at_the_kth_value():
    x = [1.0, 3.0, 2.0, 3.0, 2.0, 0.0]                  # descending: 3 3 2 2 1 0 -- the 3rd largest is 2, and both 2s stay
    assert kept(x, top_k=3)[0] == [1, 2, 3, 4]
    assert kept(x, top_k=2)[0] == [1, 3] and kept(x, top_k=1)[0] == [1, 3]      # the tied maxima
    assert kept(x, top_k=4)[0] == [1, 2, 3, 4] and kept(x, top_k=5)[0] == [0, 1, 2, 3, 4]
    assert kept(x, top_k=0)[0] == kept(x, top_k=6)[0] == kept(x, top_k=99)[0] == list(range(6))


def test_nucleus_ties_stand_or_fall_together():
    x = np.log([0.1, 0.4, 0.2, 0.1, 0.2])               # M: 0.4 -> 0, both 0.2 -> 0.4, both 0.1 -> 0.8
    assert kept(x, top_p=0.39)[1] == [1]
    assert kept(x, top_p=0.41)[1] == [1, 2, 4] and kept(x, top_p=0.79)[1] == [1, 2, 4]
    assert kept(x, top_p=0.81)[1] == [0, 1, 2, 3, 4] and kept(x, top_p=1.0)[1] == [0, 1, 2, 3, 4]
    # the temperature enters the masses: at T = 0.5 they are 16 : 4 : 4 : 1 : 1 over 26 -- M(0.2) = 0.615, M(0.1) = 0.923
    assert kept(x, T=0.5, top_p=0.6)[1] == [1] and kept(x, T=0.5, top_p=0.63)[1] == [1, 2, 4] and kept(x, T=0.5, top_p=0.93)[1] == [0, 1, 2, 3, 4]
    # after top-k the masses are those of the kept set: k = 3 keeps 0.4, 0.2, 0.2 -> 0.5, 0.25, 0.25; M(0.2) = 0.5
    assert kept(x, top_k=3, top_p=0.49) == ([1, 2, 4], [1]) and kept(x, top_k=3, top_p=0.51) == ([1, 2, 4], [1, 2, 4])


def test_a_tiny_top_p_leaves_the_tied_maxima():
    assert kept([5.0, 5.0, 1.0, 5.0, 4.0], top_p=1e-6)[1] == [0, 1, 3]
    ids = {S.sample_row([5.0, 5.0, 1.0, 5.0, 4.0], c, 7, top_p=1e-6)[0] for c in range(200)}
    assert ids == {0, 1, 3}                              # and the draw chooses among them


def test_minus_inf_columns_are_never_drawn():
    x = [NINF, 0.0, NINF, 1.0, NINF]
    assert kept(x, top_k=4)[0] == [0, 1, 2, 3, 4]        # the 4th largest value is -inf: every column is >= it
    for T, k, p in ((1.0, 0, 1.0), (3.0, 4, 1.0), (1.0, 0, 0.999999)):
        out = [S.sample_row(x, c, 11, T, k, p) for c in range(300)]
        assert {o[0] for o in out} == {1, 3}
    lp = S.logp_of(x, 3)
    assert abs(lp - (1.0 - math.log(1.0 + math.e))) < 1e-12


def test_the_draw_is_the_gumbel_argmax_and_logp_is_unfiltered():
    x = np.array([0.3, -1.0, 2.0, 1.5, 0.0, 1.9])
    for c in range(50):
        u = S.uniform_row(R.SEED_HI, c, 6)
        assert ((u > 0) & (u < 1)).all() and (u.astype(np.float32).astype(np.float64) == u).all()      # exact in float32
        h = R._hash32(R.SEED_HI, np.uint64(c << 20) | np.arange(6, dtype=np.uint64))
        assert (u == ((h >> np.uint64(9)).astype(np.float64) + 0.5) / 2 ** 23).all()
        v = x / 0.7 - np.log(-np.log(u))
        j, lp, _, _ = S.sample_row(x, c, R.SEED_HI, 0.7, 0, 1.0)
        assert j == int(np.argmax(v)) and abs(lp - (x[j] - np.log(np.exp(x).sum()))) < 1e-12
        j3 = S.sample_row(x, c, R.SEED_HI, 0.7, 3, 1.0)[0]                      # top-3: columns 2, 5, 3
        assert j3 == max((2, 5, 3), key=lambda i: v[i])
    # the counter is taken modulo 2^44, and the column is the low 20 bits
    assert (S.hash_row(5, (1 << 44) + 9, 4) == S.hash_row(5, 9, 4)).all()
    assert S.counter(3, 1, 4, 2, 8) == (3 * 2 + 1) * 8 + 4


def test_undecided_rows_are_reported():
    """a column on the nucleus boundary that would win, and a near tie of the two best, both leave a row undecided"""
    x = np.log([0.5, 0.3, 0.2])
    won = [S.sample_row(x, c, 3, 1.0, 0, 0.8 + 5e-5) for c in range(400)]      # M(0.2) = 0.8: within EPS of top_p
    assert {j for j, _, _, _ in won} == {0, 1, 2}                              # column 2 is in the nucleus by 5e-5: it can be drawn,
    assert all(not ok for j, _, ok, _ in won if j == 2)                        # and a row it wins is not decided
    assert all(ok == (lead >= S.LEAD) for j, _, ok, lead in won if j != 2)
    clear = [S.sample_row(x, c, 3, 1.0, 0, 0.7) for c in range(400)]           # M(0.2) = 0.8, M(0.3) = 0.5: nothing near 0.7
    assert all(ok == (lead >= S.LEAD) for _, _, ok, lead in clear) and {j for j, _, _, _ in clear} == {0, 1}


# ---- the contract's hash as a sampler ---------------------------------------------------------------------------------------
def test_hash_gumbel_draws_follow_the_distribution():
    x = np.array([1.2, -0.5, 0.0, 2.0, 0.7, -2.0, 1.9, 0.3])
    n = 20000
    pair = (np.arange(n, dtype=np.uint64)[:, None] << np.uint64(20)) | np.arange(8, dtype=np.uint64)[None, :]
    for seed, T in ((R.SEED_LO, 1.0), (R.SEED_HI, 0.7)):
        u = ((R._hash32(seed, pair) >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23
        ids = np.argmax(x[None, :] / T - np.log(-np.log(u)), axis=1)
        assert ids[:50].tolist() == [S.sample_row(x, c, seed, T)[0] for c in range(50)]
        p = np.exp(x / T) / np.exp(x / T).sum()
        freq = np.bincount(ids, minlength=8) / n
        z = np.abs(freq - p) / np.sqrt(p * (1 - p) / n)
        print(f"seed {seed} T {T}: worst deviation {z.max():.2f} binomial standard deviations")
        assert z.max() < 4.0


# ---- sample_rounds on scripted steps ----------------------------------------------------------------------------------------
V_S, SEP_S, LEN_S, CHAINS, SEED_S = 6, 3, 7, 3, 99
SAMPLER = dict(temperature=0.8, top_k=4, top_p=0.9)


def _table(n):
    t = torch.randn(n, V_S, V_S, generator=torch.Generator().manual_seed(1), dtype=torch.float64) * 2.0
    t[4, :, SEP_S] = -50.0                                # sample 4 never draws SEP: it runs to max_len
    return t.numpy()


def _logits(tab, b, seq, context):
    """last: a function of (sample, last token); prefix: of the whole sequence"""
    if context == "last":
        return tab[b, seq[-1]]
    return tab[b, seq[-1]] + sum(0.3 * tab[b, tok] / (len(seq) - p) for p, tok in enumerate(seq[:-1]))


def _scripted(tab, offset, context, asked):
    """a step over `tab` for a batch whose first sample is sample `offset` of the set; every row it is asked is recorded"""
    if context == "last":
        def step(rows):
            asked.append([(offset + b, tok, ctr) for b, tok, ctr in rows])
            return [S.sample_row(tab[offset + b, tok], ctr, SEED_S, **SAMPLER)[:2][::-1] for b, tok, ctr in rows]
        return step
    rounds = []                                          # per round: the (token, ancestors) of its rows

    def step(rows, t):
        assert t == len(rounds)
        rounds.append([(tok, anc) for _, tok, anc, _ in rows])
        out = []
        for b, tok, anc, ctr in rows:
            assert len(anc) == t
            seq = [rounds[p][a][0] for p, a in enumerate(anc)] + [tok]      # the history, read back through the ancestors
            asked.append([(offset + b, tuple(seq), ctr)])
            out.append(S.sample_row(_logits(tab, offset + b, seq, "prefix"), ctr, SEED_S, **SAMPLER)[:2][::-1])
        return out
    return step


@pytest.mark.parametrize("context", ["last", "prefix"])
def test_sample_rounds_equals_the_per_chain_statement(context):
    from fcmf_framework.decoding import sample_rounds
    n = 5
    tab = _table(n)
    asked = []
    got = sample_rounds(_scripted(tab, 0, context, asked), n, START, SEP_S, CHAINS, LEN_S, context)
    ends = set()
    for b in range(n):
        want, _, _ = S.sample_chains(lambda seq: _logits(tab, b, seq, context), b, CHAINS, START, SEP_S, LEN_S, SEED_S, **SAMPLER)
        assert got[b][2] == want, b                     # ids and Python-float scores, chain by chain
        best = max(want, key=lambda c: c[0])
        assert (got[b][1], got[b][0]) == best
        for score, seq in want:
            assert seq[0] == START and (seq[-1] == SEP_S or len(seq) == LEN_S + 1) and SEP_S not in seq[1:-1]
            ends.add(len(seq))
    assert all(len(seq) == LEN_S + 1 and seq[-1] != SEP_S for _, seq in got[4][2])      # the max_len path
    assert len(ends) >= 3, ends                         # chains end at different rounds
    rows = [r for call in asked for r in call]
    if context == "last":
        assert len(asked) <= LEN_S and len(asked[0]) == n * CHAINS      # one call per round, every chain a row of the first
    assert len({r[2] for r in rows}) == len(rows)       # no counter is used twice
    # counters as specified: recomputed from (sample, chain, round) of every draw
    want_ctr = {S.counter(b, c, t, CHAINS, LEN_S) for b in range(n) for c in range(CHAINS) for t in range(len(got[b][2][c][1]) - 1)}
    assert {r[2] for r in rows} == want_ctr


@pytest.mark.parametrize("context", ["last", "prefix"])
def test_sample_rounds_does_not_depend_on_the_batch_split(context):
    from fcmf_framework.decoding import sample_rounds
    tab = _table(5)
    run = lambda off, n: sample_rounds(_scripted(tab, off, context, []), n, START, SEP_S, CHAINS, LEN_S, context, sample_offset=off)
    whole = run(0, 5)
    assert run(0, 2) + run(2, 3) == whole and run(0, 1) + run(1, 4) == whole
    assert sample_rounds(_scripted(tab, 0, context, []), 5, START, SEP_S, CHAINS, LEN_S, context, sample_offset=1) != whole


# ---- length penalty ---------------------------------------------------------------------------------------------------------
def _ranked(fin, lp):
    return max(fin, key=lambda c: c[0] / max(len(c[1]) - 1, 1) ** lp)      # (max: the first among equals, as a stable sort's [0])


def test_length_penalty_0_is_the_present_beam_search():
    from fcmf_framework.decoding import beam_rounds
    n = 5
    tab = _tables(n)

    def step_many(pairs):
        return {(b, tok): tuple(x.tolist() for x in torch.topk(tab[b, tok], BEAM)) for b, tok in pairs}

    plain = beam_rounds(step_many, n, START, SEP, beam_size=BEAM, max_len=MAX_LEN)
    zero = beam_rounds(step_many, n, START, SEP, beam_size=BEAM, max_len=MAX_LEN, length_penalty=0.0)
    for b in range(n):
        ids, score, fin = O.beam_search_ids(lambda seq: tab[b, seq[-1]], START, SEP, beam_size=BEAM, max_len=MAX_LEN)
        assert zero[b][0] == ids and zero[b][1] == score and zero[b][2] == fin, b      # equality of ids and of float scores
    assert plain == zero
    for lp in (0.5, 1.0, 2.0):
        pen = beam_rounds(step_many, n, START, SEP, beam_size=BEAM, max_len=MAX_LEN, length_penalty=lp)
        for b in range(n):
            assert pen[b][2] == zero[b][2]               # the search itself is untouched: the same finished list, raw scores
            assert (pen[b][1], pen[b][0]) == _ranked(pen[b][2], lp)
    assert any(pen[b][0] != zero[b][0] for b in range(n))      # (lp = 2 moves the choice of at least one scripted sample)


def _short_or_long():
    """START -> SEP costs 1.0; START -> 1 -> 2 -> SEP costs 0.6 + 0.5 + 0.4 = 1.5 in all but 0.5 per token"""
    low = -9.0
    row = {START: {SEP: -1.0, 1: -0.6}, 1: {2: -0.5, SEP: -3.0}, 2: {SEP: -0.4, 1: -4.0}}

    def step_many(pairs):
        out = {}
        for b, tok in pairs:
            lp = sorted(((row[tok].get(j, low - j), j) for j in range(6)), reverse=True)[:2]
            out[(b, tok)] = ([s for s, _ in lp], [j for _, j in lp])
        return out
    return step_many


@pytest.mark.parametrize("context", ["last", "prefix"])
def test_length_penalty_1_picks_the_longer_hypothesis(context):
    from fcmf_framework.decoding import beam_rounds
    pairs = _short_or_long()
    step = pairs if context == "last" else (lambda rows, t: [pairs([(b, tok)])[(b, tok)] for b, tok, _ in rows])
    res = {lp: beam_rounds(step, 2, START, SEP, beam_size=2, max_len=6, context=context, length_penalty=lp) for lp in (0.0, 1.0)}
    for b in range(2):
        assert res[0.0][b][0] == [START, SEP] and res[0.0][b][1] == -1.0
        assert res[1.0][b][0] == [START, 1, 2, SEP] and res[1.0][b][1] == -0.6 + -0.5 + -0.4      # the returned score stays the raw sum
        assert res[1.0][b][2] == res[0.0][b][2]
        for lp in (0.0, 1.0):
            assert (res[lp][b][1], res[lp][b][0]) == _ranked(res[lp][b][2], lp)


def test_length_penalty_covers_the_fallback_to_the_live_beams_and_the_chains():
    from fcmf_framework.decoding import _best, beam_rounds, sample_rounds
    tab = _tables(5)
    step_many = lambda pairs: {(b, tok): tuple(x.tolist() for x in torch.topk(tab[b, tok], BEAM)) for b, tok in pairs}
    for lp in (0.0, 1.0):
        got = beam_rounds(step_many, 5, START, SEP, beam_size=BEAM, max_len=2, length_penalty=lp)      # too short to finish everywhere
        assert any(all(seq[-1] != SEP for _, seq in g[2]) for g in got)
        assert all((g[1], g[0]) == _ranked(g[2], lp) for g in got)
    fin = [(-1.0, [0, 3]), (-1.5, [0, 1, 2, 3]), (-1.5, [0, 1, 1, 3])]
    assert _best(fin) == fin[0] and _best(fin, 1.0) == fin[1] and _best([(-2.0, [0])], 1.0) == (-2.0, [0])
    stab = _table(5)
    for lp in (0.0, 1.5):
        got = sample_rounds(_scripted(stab, 0, "last", []), 5, START, SEP_S, CHAINS, LEN_S, length_penalty=lp)
        assert all((g[1], g[0]) == _ranked(g[2], lp) for g in got)


# ---- the driver's flags -----------------------------------------------------------------------------------------------------
def test_driver_sampling_flags_defaults_and_validation(tmp_path):
    import run_pretraining_fcmf as drv
    base = ["--output_dir", str(tmp_path / "o"), "--pretrained_hf_model", str(tmp_path), "--synthetic_steps", "2"]
    a = drv.build_parser().parse_args(base)
    assert (a.decode_strategy, a.temperature, a.top_k, a.top_p, a.num_chains, a.sample_seed, a.length_penalty) == ("beam", 1.0, 0, 1.0, 1, 0, 0.0)
    a = drv.build_parser().parse_args(base + "--decode_strategy sample --temperature 0.7 --top_k 50 --top_p 0.9 --num_chains 4 --sample_seed 5 "
                                             "--length_penalty 1.0".split())
    assert (a.decode_strategy, a.temperature, a.top_k, a.top_p, a.num_chains, a.sample_seed, a.length_penalty) == ("sample", 0.7, 50, 0.9, 4, 5, 1.0)
    with pytest.raises(SystemExit):
        drv.build_parser().parse_args(base + ["--decode_strategy", "greedy"])
    sample = base + ["--do_eval", "--decode_strategy", "sample"]
    for extra, match in ((["--temperature", "0"], "temperature"), (["--temperature", "inf"], "temperature"),
                         (["--temperature", "-1"], "temperature"), (["--top_k", "-1"], "top_k"), (["--top_p", "0"], "top_p"),
                         (["--top_p", "1.5"], "top_p"), (["--num_chains", "0"], "--num_chains"), (["--sample_seed", "-3"], "--sample_seed"),
                         (["--length_penalty", "nan"], "--length_penalty"),
                         (["--decode_context", "prefix", "--max_len_decoder", "513"], "--max_len_decoder")):
        with pytest.raises(ValueError, match=match):
            drv.main(sample + extra)
    with pytest.raises(ValueError, match="--length_penalty"):
        drv.main(base + ["--do_eval", "--length_penalty", "inf"])
    assert not (tmp_path / "o").exists()                # refused before anything is trained or written


def test_the_reference_command_lines_still_parse():
    import run_pretraining_fcmf as drv
    a = drv.build_parser().parse_args(PUBLISHED_PRETRAIN)
    assert (a.max_len_decoder, a.beam_size, a.decode_strategy, a.length_penalty, a.decode_context) == (8, 2, "beam", 0.0, "last")
    c = drv.build_parser().parse_args(_argv(REF_PRETRAIN_FLAGS))
    assert c.beam_size == 2 and c.do_eval and c.decode_strategy == "beam" and c.num_chains == 1
