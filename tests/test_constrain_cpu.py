"""Generation constraints without a GPU: tests/constraints_ref.py (the numpy statement of fcmf_logits_constrain) against
hand-worked rows and against transformers' own logits processors; ops.check_constraints / decoding.make_constraints / the
pre-training driver's refusals; decoding.beam_rounds and sample_rounds with constraints on, over scripted steps, against the
oracle's beam search and sampling_ref.sample_chains over the constrained step -- and, with constraints=None, the exact calls the
loops made before constraints existed."""
import numpy as np
import pytest
import torch

import constraints_ref as C
import sampling_ref as S
from oracle import fcmf_oracle as O
from test_decode_batch_cpu import BEAM, MAX_LEN, SEP, START, _tables
from fcmf_framework.decoding import make_constraints      # the feature under test: without it nothing here says anything
from fcmf_framework.ops import CONSTRAIN_MAX_T, check_constraints

INF = float("inf")


# ---- the reference against hand-worked rows ---------------------------------------------------------------------------------
def test_repetition_penalty_once_per_distinct_token():
    x = [4.0, -4.0, 0.0, 2.0, -0.0, -INF, 8.0]
    got = C.constrain_row(x, [0, 1, 0, 0, 5, 4, 1, 0, 0], repetition_penalty=2.0)
    assert got.tolist() == [2.0, -8.0, 0.0, 2.0, -0.0, -INF, 8.0]            # token 0 five times: 4 / 2, not 4 / 32
    assert np.signbit(got[4]) and not np.signbit(got[2])
    half = C.constrain_row(x, [0, 1, 6], repetition_penalty=0.5)
    assert half.tolist() == [8.0, -2.0, 0.0, 2.0, -0.0, -INF, 16.0]
    # float32 arithmetic, one rounding: 1 / 1.3 in float32, then to bf16
    y = C.constrain_row([1.0], [0], repetition_penalty=1.3)
    assert y[0] == np.float32(1.0) / np.float32(1.3)
    yb = C.constrain_row([1.0], [0], repetition_penalty=1.3, bf16=True)
    assert yb[0] == np.float32(0.76953125) and C.to_bf16_bits([yb[0]])[0] == 0x3F45


def test_bf16_rounding_is_to_nearest_even():
    f = lambda bits: np.array([bits], dtype=np.uint32).view(np.float32)[0]
    assert C.to_bf16_bits([f(0x3F808000)])[0] == 0x3F80           # a tie: to the even neighbour below
    assert C.to_bf16_bits([f(0x3F818000)])[0] == 0x3F82           # a tie: to the even neighbour above
    assert C.to_bf16_bits([f(0x3F808001)])[0] == 0x3F81
    assert C.to_bf16_bits([-INF])[0] == 0xFF80
    x = torch.randn(4096, generator=torch.Generator().manual_seed(0)) * 50
    assert np.array_equal(C.from_bf16_bits(C.to_bf16_bits(x.numpy())), x.to(torch.bfloat16).float().numpy())


def test_no_repeat_ngram_hand_worked():
    V = 10
    ban = lambda h, n: sorted(C.banned(h, V, no_repeat_ngram_size=n))
    assert ban([3, 4, 5, 3], 2) == [4]                     # "3" was followed by 4
    assert ban([3, 4, 5, 3, 4, 6, 3], 2) == [4]            # several matches of the suffix, one token
    assert ban([3, 4, 5, 3, 6, 7, 3], 2) == [4, 6]         # several matches, two tokens
    assert ban([7, 7, 7], 2) == [7]                        # a match that overlaps the suffix itself
    assert ban([1, 2, 3], 1) == [1, 2, 3]                  # n = 1 bans every token of the sequence
    assert ban([1, 2], 3) == []                            # L < n bans nothing
    assert ban([1, 2, 9], 3) == []                         # L = n: the one start is the suffix's own tokens 1 2 != 2 9
    assert ban([1, 2, 1, 2], 3) == [1]                     # L = n + 1: starts 0 (1 2 == 1 2 -> bans h[2] = 1) and 1 (2 1 != 1 2)
    assert ban([5, 5, 5, 5], 3) == [5]
    assert ban([1, 2, 3, 4, 1, 2, 3], 4) == [4]
    assert ban([1, 2, 3, 4, 9, 2, 3], 4) == []
    assert ban([3, -1, 5, 3], 2) == [] and ban([3, V, 3], 2) == []      # the followed token is outside [0, V): nothing


def test_min_length_suppressed_ids_and_the_order_of_the_rules():
    x = np.arange(1, 9, dtype=np.float32)
    got = C.constrain_row(x, [0, 1, 2], min_length=4, sep_id=5)
    assert np.isneginf(got[5]) and np.array_equal(np.delete(got, 5), np.delete(x, 5))          # L = m - 1
    assert np.array_equal(C.constrain_row(x, [0, 1, 2, 3], min_length=4, sep_id=5), x)         # L = m
    got = C.constrain_row(x, [0], ban_ids=[7, -1, 8, 13, 2])
    assert np.isneginf(got[[2, 7]]).all() and np.isfinite(np.delete(got, [2, 7])).all()
    assert np.array_equal(C.constrain_row(x, [0], min_length=9, sep_id=8), x)                  # sep outside [0, V)
    # a column both penalised and banned is -inf; columns beyond V keep what they held
    got = C.constrain_row(x, [3, 4, 3], V=6, repetition_penalty=2.0, no_repeat_ngram_size=2, ban_ids=[6, 7])
    assert got.tolist() == [1.0, 2.0, 3.0, 2.0, -INF, 6.0, 7.0, 8.0]
    assert np.array_equal(C.constrain_row(x, [1, 2, 3]), x)                                    # everything off


# ---- the reference against transformers' processors --------------------------------------------------------------------------
def _hf():
    lp = pytest.importorskip("transformers.generation.logits_process")
    return lp


@pytest.mark.parametrize("theta", [0.5, 1.3, 2.0])
def test_reference_equals_transformers_repetition_penalty(theta):
    lp = _hf()
    g = torch.Generator().manual_seed(3)
    V, L, rows = 50, 12, 16
    x = torch.randn(rows, V, generator=g) * 4
    x[:, 7], x[:, 9] = 0.0, -INF
    hist = torch.randint(0, 12, (rows, L), generator=g)        # 12 tokens, 12 positions: repeats in every row
    want = lp.RepetitionPenaltyLogitsProcessor(theta)(hist, x.clone()).numpy()
    got = C.constrain_rows(x.numpy(), hist.numpy(), repetition_penalty=theta)
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_reference_equals_transformers_no_repeat_ngram(n):
    lp = _hf()
    g = torch.Generator().manual_seed(4 + n)
    V, rows = 9, 64
    for L in (n - 1, n, n + 1, 9, 30):
        if L < 1:
            continue
        hist = torch.randint(0, 3, (rows, L), generator=g)     # three tokens: many repeated n-grams
        x = torch.randn(rows, V, generator=g)
        want = lp.NoRepeatNGramLogitsProcessor(n)(hist, x.clone()).numpy()
        got = C.constrain_rows(x.numpy(), hist.numpy(), no_repeat_ngram_size=n)
        assert got.tobytes() == want.tobytes(), (n, L)
        assert L < n or np.isneginf(got).any()


def test_reference_equals_transformers_min_length_and_suppress_tokens():
    lp = _hf()
    x = torch.randn(3, 20, generator=torch.Generator().manual_seed(8))
    for L in (3, 4, 5):
        hist = torch.zeros(3, L, dtype=torch.long)
        want = lp.MinLengthLogitsProcessor(5, 2)(hist, x.clone()).numpy()
        assert C.constrain_rows(x.numpy(), hist.numpy(), min_length=5, sep_id=2).tobytes() == want.tobytes()
    want = lp.SuppressTokensLogitsProcessor([1, 3, 19])(torch.zeros(3, 2, dtype=torch.long), x.clone()).numpy()
    assert C.constrain_rows(x.numpy(), np.zeros((3, 2), dtype=np.int64), ban_ids=[1, 3, 19]).tobytes() == want.tobytes()


def test_reference_equals_the_processors_chained_in_its_order():
    lp = _hf()
    g = torch.Generator().manual_seed(11)
    hist = torch.randint(0, 5, (32, 7), generator=g)
    x = torch.randn(32, 40, generator=g) * 3
    s = x.clone()
    for p in (lp.RepetitionPenaltyLogitsProcessor(1.3), lp.NoRepeatNGramLogitsProcessor(2), lp.MinLengthLogitsProcessor(9, 2),
              lp.SuppressTokensLogitsProcessor([4, 30])):
        s = p(hist, s)
    got = C.constrain_rows(x.numpy(), hist.numpy(), repetition_penalty=1.3, no_repeat_ngram_size=2, min_length=9, sep_id=2, ban_ids=[4, 30])
    assert got.tobytes() == s.numpy().tobytes()


# ---- argument checks --------------------------------------------------------------------------------------------------------
def test_check_constraints_names_the_argument():
    from fcmf_framework import ops
    assert ops.CONSTRAIN_MAX_T == 512 == ops.DECODE_ATTN_MAX_T
    ops.check_constraints()
    ops.check_constraints(1.3, 2, 5, (1, 3))
    for kw, match in ((dict(repetition_penalty=0.0), "repetition_penalty"), (dict(repetition_penalty=-1.0), "repetition_penalty"),
                      (dict(repetition_penalty=INF), "repetition_penalty"), (dict(repetition_penalty=float("nan")), "repetition_penalty"),
                      (dict(no_repeat_ngram_size=-1), "no_repeat_ngram_size"), (dict(no_repeat_ngram_size=1.5), "no_repeat_ngram_size"),
                      (dict(min_length=-2), "min_length"), (dict(min_length=2.0), "min_length"),
                      (dict(suppress_tokens=(3, -1)), "suppress_tokens"), (dict(suppress_tokens=(1.5,)), "suppress_tokens"),
                      (dict(suppress_tokens=range(1025)), "suppress_tokens")):
        with pytest.raises(ValueError, match=match):
            ops.check_constraints(**kw)
    ops.check_constraints(suppress_tokens=range(1024))


def test_make_constraints_checks_and_collapses():
    from fcmf_framework.decoding import make_constraints
    assert make_constraints() is None and make_constraints(None) is None and make_constraints({}) is None
    assert make_constraints(dict(repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0, suppress_tokens=[])) is None
    got = make_constraints(dict(no_repeat_ngram_size=2), suppress_tokens=[5, 1])
    assert got == dict(repetition_penalty=1.0, no_repeat_ngram_size=2, min_length=0, suppress_tokens=(5, 1))
    assert make_constraints(got) == got                    # a checked dict passes through
    assert make_constraints(repetition_penalty=1.3)["repetition_penalty"] == 1.3
    assert make_constraints(min_length=3)["min_length"] == 3
    with pytest.raises(ValueError, match="unknown settings.*bad_words"):
        make_constraints(dict(bad_words=[1]))
    with pytest.raises(ValueError, match="repetition_penalty"):
        make_constraints(repetition_penalty=0)
    with pytest.raises(ValueError, match="suppress_tokens"):
        make_constraints(suppress_tokens=7)


def test_driver_constraint_flags_defaults_and_validation(tmp_path):
    import run_pretraining_fcmf as drv
    base = ["--output_dir", str(tmp_path / "o"), "--pretrained_hf_model", str(tmp_path), "--synthetic_steps", "2"]
    a = drv.build_parser().parse_args(base)
    assert (a.repetition_penalty, a.no_repeat_ngram_size, a.min_length_decoder, a.suppress_tokens) == (1.0, 0, 0, [])
    a = drv.build_parser().parse_args(base + "--repetition_penalty 1.3 --no_repeat_ngram_size 2 --min_length_decoder 5 --suppress_tokens 1 3 4".split())
    assert (a.repetition_penalty, a.no_repeat_ngram_size, a.min_length_decoder, a.suppress_tokens) == (1.3, 2, 5, [1, 3, 4])
    ev = base + ["--do_eval"]
    for extra, match in ((["--repetition_penalty", "0"], "--repetition_penalty"), (["--repetition_penalty", "inf"], "--repetition_penalty"),
                         (["--repetition_penalty", "-2"], "--repetition_penalty"), (["--no_repeat_ngram_size", "-1"], "--no_repeat_ngram_size"),
                         (["--min_length_decoder", "-1"], "--min_length_decoder"), (["--suppress_tokens", "3", "-4"], "--suppress_tokens"),
                         (["--min_length_decoder", "9", "--max_len_decoder", "8"], "--min_length_decoder"),
                         (["--no_repeat_ngram_size", "2", "--max_len_decoder", "513"], "--max_len_decoder"),
                         (["--repetition_penalty", "1.3", "--beam_size", "17"], "--beam_size"),
                         (["--suppress_tokens", "1", "2", "--vocab_size", "12", "--max_len_decoder", "8", "--beam_size", "2"], "--vocab_size")):
        with pytest.raises(ValueError, match=match):
            drv.main(ev + extra)
    assert not (tmp_path / "o").exists()                # refused before anything is trained or written


# ---- the host loops over scripted steps -------------------------------------------------------------------------------------
SETTINGS = [dict(no_repeat_ngram_size=2, repetition_penalty=1.3), dict(min_length=MAX_LEN, suppress_tokens=(1,)),
            dict(no_repeat_ngram_size=3), dict(repetition_penalty=2.0, min_length=3)]


def _logits(tab, b, seq, context):
    """last: a function of (sample, last token); prefix: of the whole sequence"""
    if context == "last":
        return tab[b, seq[-1]]
    return tab[b, seq[-1]] + sum(0.3 * tab[b, tok] / (len(seq) - p) for p, tok in enumerate(seq[:-1]))


def _beam_step(tab, context, cfg, asked):
    """the scripted step of a constrained beam search: the constrained log-softmax of `_logits`, top BEAM; records every row"""
    top = lambda b, seq: tuple(v.tolist() for v in torch.topk(
        C.constrained_step(lambda s: _logits(tab, b, s, context), SEP, as_logprobs=True, **cfg)(seq), BEAM))
    if context == "last":
        def step(rows):
            asked.append(list(rows))
            assert all(len(r) == 3 and r[2][-1] == r[1] for r in rows)
            return [top(b, seq) for b, _, seq in rows]
        return step
    rounds = []

    def step(rows, t):
        assert t == len(rounds)
        rounds.append([tok for _, tok, _, _ in rows])
        asked.append(list(rows))
        for b, tok, anc, seq in rows:                    # the sequence handed over IS the one the ancestors spell
            assert len(anc) == t and [rounds[p][a] for p, a in enumerate(anc)] + [tok] == seq
        return [top(b, seq) for b, _, _, seq in rows]
    return step


@pytest.mark.parametrize("cfg", SETTINGS, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
@pytest.mark.parametrize("context", ["last", "prefix"])
def test_constrained_beam_rounds_equal_the_oracle_over_the_constrained_step(context, cfg):
    from fcmf_framework.decoding import beam_rounds, make_constraints
    n = 5
    tab = _tables(n)
    asked = []
    got = beam_rounds(_beam_step(tab, context, cfg, asked), n, START, SEP, beam_size=BEAM, max_len=MAX_LEN, context=context,
                      constraints=make_constraints(cfg))
    plain = 0
    for b in range(n):
        step = C.constrained_step(lambda s: _logits(tab, b, s, context), SEP, as_logprobs=True, **cfg)
        ids, score, fin = O.beam_search_ids(step, START, SEP, beam_size=BEAM, max_len=MAX_LEN)
        assert got[b][0] == ids and got[b][1] == score and got[b][2] == fin, b      # ids and Python-float scores
        free = O.beam_search_ids(lambda s: torch.log_softmax(_logits(tab, b, s, context), -1), START, SEP, beam_size=BEAM, max_len=MAX_LEN)
        plain += free[0] != ids
        for _, seq in fin:
            if cfg.get("no_repeat_ngram_size"):
                assert not C.has_repeated_ngram(seq, cfg["no_repeat_ngram_size"]), seq
            if cfg.get("min_length"):
                assert SEP not in seq[1:cfg["min_length"]], seq
            assert not set(cfg.get("suppress_tokens", ())) & set(seq[1:])
    assert plain >= 1, plain                              # the constraint changes what is decoded (most samples end within 4 tokens)
    # one call per round, every live beam a row -- no memo: rows with the same (sample, last token) do occur, both are asked
    assert len(asked) <= MAX_LEN and [r[:2] for r in asked[0]] == [(b, START) for b in range(n)]
    assert all(len(r[-1]) == t + 1 for t, rows in enumerate(asked) for r in rows)
    if context == "last" and "suppress_tokens" not in cfg:
        assert any(len({r[:2] for r in rows}) < len(rows) for rows in asked)
    # pruning reorders: somewhere the row at beam position j continues another position's sequence of the round before
    moved = False
    for prev, rows in zip(asked, asked[1:]):
        for b in range(n):
            p, q = [r[-1] for r in prev if r[0] == b], [r[-1] for r in rows if r[0] == b]
            moved |= len(p) == len(q) == BEAM and [s[:-1] for s in q] != p
    assert moved


def _chain_step(tab, offset, context, cfg, asked, sampler, seed):
    draw = lambda b, seq, ctr: S.sample_row(C.constrained_step(lambda s: _logits(tab, offset + b, s, context), S_SEP, **cfg)(seq), ctr, seed,
                                            **sampler)[:2][::-1]
    if context == "last":
        def step(rows):
            asked.append(list(rows))
            assert all(len(r) == 4 and r[3][-1] == r[1] for r in rows)
            return [draw(b, seq, ctr) for b, _, ctr, seq in rows]
        return step
    rounds = []

    def step(rows, t):
        assert t == len(rounds)
        rounds.append([tok for _, tok, _, _, _ in rows])
        asked.append(list(rows))
        for b, tok, anc, ctr, seq in rows:
            assert [rounds[p][a] for p, a in enumerate(anc)] + [tok] == seq
        return [draw(b, seq, ctr) for b, _, _, ctr, seq in rows]
    return step


S_V, S_SEP, S_LEN, S_CHAINS, S_SEED = 12, 2, 6, 3, 77
S_SAMPLER = dict(temperature=0.9, top_k=8, top_p=0.95)
S_SETTINGS = [dict(no_repeat_ngram_size=2, repetition_penalty=1.3), dict(min_length=S_LEN, suppress_tokens=(5,))]


@pytest.mark.parametrize("cfg", S_SETTINGS, ids=["ngram2-rep1.3", "minlen-suppress"])
@pytest.mark.parametrize("context", ["last", "prefix"])
def test_constrained_sample_rounds_equal_the_per_chain_statement(context, cfg):
    from fcmf_framework.decoding import make_constraints, sample_rounds
    n = 4
    tab = (torch.randn(n, S_V, S_V, generator=torch.Generator().manual_seed(2)) * 2.0)
    asked = []
    got = sample_rounds(_chain_step(tab, 0, context, cfg, asked, S_SAMPLER, S_SEED), n, START, S_SEP, S_CHAINS, S_LEN, context,
                        constraints=make_constraints(cfg))
    differs = 0
    for b in range(n):
        step = C.constrained_step(lambda s: _logits(tab, b, s, context), S_SEP, **cfg)
        want, _, _ = S.sample_chains(step, b, S_CHAINS, START, S_SEP, S_LEN, S_SEED, **S_SAMPLER)
        assert got[b][2] == want, b
        free, _, _ = S.sample_chains(lambda s: _logits(tab, b, s, context).double().numpy(), b, S_CHAINS, START, S_SEP, S_LEN, S_SEED, **S_SAMPLER)
        differs += [c[1] for c in free] != [c[1] for c in want]
        for _, seq in want:
            if cfg.get("no_repeat_ngram_size"):
                assert not C.has_repeated_ngram(seq, 2)
            if cfg.get("min_length"):
                assert len(seq) == S_LEN + 1 and S_SEP not in seq[1:S_LEN] and 5 not in seq[1:]
    assert differs >= 2
    assert all(len(r[-1]) == t + 1 for t, rows in enumerate(asked) for r in rows) and len(asked[0]) == n * S_CHAINS
    # the sequences handed over are copies: what the loop appends later does not reach into a recorded call
    assert all(len(r[-1]) == 1 for r in asked[0])


# ---- constraints=None: the loops' calls as they were before constraints existed ---------------------------------------------------
# recorded from the loops of the commit before this feature, over `_tables(5)[:2]` / the table of `_plain_chain_calls`, max_len 3
PLAIN_BEAM_LAST = [[(0, 0), (1, 0)], [(0, 1), (1, 2)], [(0, 5), (1, 5)]]
PLAIN_BEAM_PREFIX = [([(0, 0, []), (1, 0, [])], 0), ([(0, 1, [0]), (1, 2, [1])], 1), ([(0, 5, [0, 0]), (1, 5, [1, 1]), (1, 2, [1, 1])], 2)]
PLAIN_CHAIN_LAST = [[(0, 0, 0), (0, 0, 3), (1, 0, 6), (1, 0, 9)], [(0, 5, 1), (0, 5, 4), (1, 2, 7)], [(0, 4, 2), (0, 5, 5), (1, 1, 8)]]
PLAIN_CHAIN_PREFIX = [([(0, 0, [], 0), (0, 0, [], 3), (1, 0, [], 6), (1, 0, [], 9)], 0), ([(0, 5, [0], 1), (0, 5, [1], 4), (1, 2, [2], 7)], 1),
                      ([(0, 4, [0, 0], 2), (0, 5, [1, 1], 5), (1, 1, [2, 2], 8)], 2)]


def _plain_beam_calls(context, **kw):
    from fcmf_framework.decoding import beam_rounds
    tab = _tables(5)[:2]
    calls = []
    if context == "last":
        def step(pairs):
            calls.append([tuple(p) for p in pairs])
            return {(b, t): tuple(x.tolist() for x in torch.topk(tab[b, t], BEAM)) for b, t in pairs}
    else:
        def step(rows, t):
            calls.append(([(b, tok, list(anc)) for b, tok, anc in rows], t))
            return [tuple(x.tolist() for x in torch.topk(_logits(tab, b, [START] * len(anc) + [tok], "prefix"), BEAM)) for b, tok, anc in rows]
    beam_rounds(step, 2, START, SEP, beam_size=BEAM, max_len=3, context=context, **kw)
    return calls


def _plain_chain_calls(context, **kw):
    from fcmf_framework.decoding import sample_rounds
    tab = (torch.randn(2, 6, 6, generator=torch.Generator().manual_seed(5), dtype=torch.float64) * 2.0).numpy()
    calls = []
    if context == "last":
        def step(rows):
            calls.append([tuple(r) for r in rows])
            return [S.sample_row(tab[b, tok], ctr, 9)[:2][::-1] for b, tok, ctr in rows]
    else:
        def step(rows, t):
            calls.append(([(b, tok, list(anc), ctr) for b, tok, anc, ctr in rows], t))
            return [S.sample_row(tab[b, tok] + 0.1 * len(anc), ctr, 9)[:2][::-1] for b, tok, anc, ctr in rows]
    sample_rounds(step, 2, START, 3, 2, 3, context, **kw)
    return calls


def test_without_constraints_the_steps_receive_what_they_always_did():
    kw = dict(constraints=None)
    assert _plain_beam_calls("last", **kw) == PLAIN_BEAM_LAST
    assert _plain_beam_calls("prefix", **kw) == PLAIN_BEAM_PREFIX
    assert _plain_chain_calls("last", **kw) == PLAIN_CHAIN_LAST
    assert _plain_chain_calls("prefix", **kw) == PLAIN_CHAIN_PREFIX
