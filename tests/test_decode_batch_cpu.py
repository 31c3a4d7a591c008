"""Host loop of the batched IAOG beam search (fcmf_framework.decoding.beam_rounds) against the oracle's restatement of the
reference loop (oracle.fcmf_oracle.beam_search_ids) run per sample: a `step_many` backed by a seeded table of random
log-probabilities per (sample, token), over a tiny vocabulary so that SEP does occur.  No GPU."""
import pytest
import torch

from oracle import fcmf_oracle as O

V, SEP, START, BEAM, MAX_LEN = 6, 3, 0, 2, 7
NEVER = 4          # this sample's table gives SEP the lowest probability after every token: it runs to max_len


def _tables(n):
    g = torch.Generator().manual_seed(0)
    t = torch.log_softmax(torch.randn(n, V, V, generator=g, dtype=torch.float64) * 2.0, dim=-1).float()
    t[NEVER, :, SEP] = -50.0
    return t


def test_beam_rounds_equals_oracle_per_sample():
    from fcmf_framework.decoding import beam_rounds
    n = 5
    tab = _tables(n)
    asked = []

    def step_many(pairs):
        asked.extend(pairs)
        out = {}
        for b, tok in pairs:
            s, i = torch.topk(tab[b, tok], BEAM)
            out[(b, tok)] = (s.tolist(), i.tolist())
        return out

    got = beam_rounds(step_many, n, START, SEP, beam_size=BEAM, max_len=MAX_LEN)
    assert len(asked) == len(set(asked)), "a (sample, token) pair was requested twice"
    ends = set()
    for b in range(n):
        ids, score, fin = O.beam_search_ids(lambda seq: tab[b, seq[-1]], START, SEP, beam_size=BEAM, max_len=MAX_LEN)
        assert got[b][0] == ids and got[b][1] == score and got[b][2] == fin, b
        ends.add(max(len(f[1]) for f in fin) if any(f[1][-1] == SEP for f in fin) else None)
    assert got[NEVER][0][-1] != SEP and len(got[NEVER][0]) == MAX_LEN + 1          # the max_len path
    assert len(ends) >= 4, ends                                                   # samples finish at different rounds (seed 0: lengths 6, 2, 4, 2, never)


def test_beam_rounds_calls_the_step_once_per_round():
    from fcmf_framework.decoding import beam_rounds
    tab = _tables(5)
    calls = []

    def step_many(pairs):
        calls.append(list(pairs))
        return {(b, t): tuple(x.tolist() for x in torch.topk(tab[b, t], BEAM)) for b, t in pairs}

    beam_rounds(step_many, 5, START, SEP, beam_size=BEAM, max_len=MAX_LEN)
    assert len(calls) <= MAX_LEN and calls[0] == [(b, START) for b in range(5)]


def test_driver_flag_default_and_beam_limit(tmp_path):
    """--batched_decode is off by default; a beam wider than the top-k kernel's limit is refused before anything is trained or written"""
    import run_pretraining_fcmf as drv
    base = ["--output_dir", str(tmp_path / "o"), "--pretrained_hf_model", str(tmp_path), "--synthetic_steps", "2"]
    assert not drv.build_parser().parse_args(base).batched_decode
    assert drv.build_parser().parse_args(base + ["--batched_decode"]).batched_decode
    with pytest.raises(ValueError, match="--beam_size 17"):
        drv.main(base + ["--do_eval", "--batched_decode", "--beam_size", "17"])
    assert not (tmp_path / "o").exists()
