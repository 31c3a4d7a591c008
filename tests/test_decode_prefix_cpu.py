"""Host loop of the prefix-mode IAOG beam search (fcmf_framework.decoding.beam_rounds(context="prefix")) against the oracle's
restatement of the reference loop (oracle.fcmf_oracle.beam_search_ids), which already hands the whole sequence to its step function.
The fake step here sees what the device step sees -- (sample, token, ancestors) per row -- and rebuilds every beam's sequence from
its own per-round record of the rows' tokens, read through the ancestor table: that is the cache's addressing.  Its log-probabilities
depend on the WHOLE sequence (seeded by a hash of it), so a wrong ancestor changes the search.  No GPU."""
import hashlib

import pytest
import torch

from oracle import fcmf_oracle as O

V, SEP, START, MAX_LEN = 6, 3, 0, 7
NEVER = 4          # this sample gives SEP the lowest probability after every sequence: it runs to max_len


def _logp(b, seq):
    """float32 [V] log-probabilities of sample b after `seq`: a function of the whole sequence"""
    h = hashlib.sha256(repr((b, tuple(seq))).encode()).digest()
    g = torch.Generator().manual_seed(int.from_bytes(h[:7], "little"))
    x = torch.randn(V, generator=g, dtype=torch.float64) * 2.0
    if b == NEVER:
        x[SEP] = -50.0
    elif len(seq) > 1 + b:            # samples get ready to finish at different rounds
        x[SEP] += 3.0
    else:
        x[SEP] = -50.0
    return torch.log_softmax(x, dim=-1).float()


class _Step:
    """step_many of prefix mode: keeps the token of every (round, row) -- what the key cache keeps of a row -- and checks that reading
    it back through a row's ancestors gives a sequence that the search actually holds"""

    def __init__(self, beam):
        self.beam, self.tok_at, self.calls, self.seqs = beam, [], [], []

    def __call__(self, rows, t):
        assert t == len(self.tok_at), "rounds come in order, one call each"
        self.tok_at.append([tok for _, tok, _ in rows])
        self.calls.append(len(rows))
        out = []
        for b, tok, anc in rows:
            assert len(anc) == t and all(0 <= a < len(self.tok_at[p]) for p, a in enumerate(anc))
            seq = [self.tok_at[p][a] for p, a in enumerate(anc)] + [tok]
            self.seqs.append((t, b, tuple(seq)))
            s, i = torch.topk(_logp(b, seq), self.beam)
            out.append((s.tolist(), i.tolist()))
        return out


@pytest.mark.parametrize("beam", [1, 3])
def test_prefix_rounds_equal_the_oracle_per_sample(beam):
    from fcmf_framework.decoding import beam_rounds
    n = 5
    step = _Step(beam)
    got = beam_rounds(step, n, START, SEP, beam_size=beam, max_len=MAX_LEN, context="prefix")
    assert len(step.calls) <= MAX_LEN and step.calls[0] == n and max(step.calls) <= n * beam
    ends = set()
    for b in range(n):
        asked = []

        def ref_step(seq):
            asked.append(tuple(seq))
            return _logp(b, seq)

        ids, score, fin = O.beam_search_ids(ref_step, START, SEP, beam_size=beam, max_len=MAX_LEN)
        assert got[b][0] == ids and got[b][1] == score and got[b][2] == fin, b
        # the ancestor invariant, in every round and for every row: the sequences rebuilt through the ancestor tables are exactly
        # the live beams the oracle expanded, in its order (a duplicate beam is a row of its own: there is no memo)
        mine = [(t, s) for t, bb, s in step.seqs if bb == b]
        assert [s for _, s in mine] == asked and all(len(s) == t + 1 for t, s in mine), b
        ends.add(len(ids) if ids[-1] == SEP else None)
    assert got[NEVER][0][-1] != SEP and len(got[NEVER][0]) == MAX_LEN + 1          # the max_len path
    assert len(ends) >= 4, ends                                                   # samples finish at different rounds


def test_prefix_rows_branch_and_reorder():
    """the shapes the ancestor table is for do occur: two rows of a round with the same parent, and rows of one sample whose
    parents are not in row order (a beam overtook another)"""
    from fcmf_framework.decoding import beam_rounds
    seen = {"shared": False, "reordered": False}

    def step(rows, t):
        if t >= 1:
            parents = {}
            for b, _, anc in rows:
                parents.setdefault(b, []).append(anc[-1])
            for ps in parents.values():
                seen["shared"] |= len(set(ps)) < len(ps)
                seen["reordered"] |= ps != sorted(ps)
        return [tuple(x.tolist() for x in torch.topk(_logp(NEVER, [tok] + list(anc)), 3)) for b, tok, anc in rows]

    beam_rounds(step, 3, START, SEP, beam_size=3, max_len=MAX_LEN, context="prefix")
    assert seen["shared"] and seen["reordered"], seen


def test_default_context_is_last_and_unknown_contexts_are_refused():
    from fcmf_framework.decoding import beam_rounds
    with pytest.raises(ValueError, match="context"):
        beam_rounds(lambda pairs: {}, 1, START, SEP, context="all")
    calls = []

    def step_many(pairs):                       # the "last" protocol: (sample, token) pairs in, a dict out
        calls.append(pairs)
        return {p: ([-1.0, -2.0], [SEP, 1]) for p in pairs}

    out = beam_rounds(step_many, 2, START, SEP, beam_size=2, max_len=3)
    assert calls[0] == [(0, START), (1, START)] and out[0][0] == [START, SEP]


def test_driver_flag_default_and_limits(tmp_path):
    """--decode_context is `last` by default; prefix mode's beam and length limits are checked before anything is trained or written"""
    import run_pretraining_fcmf as drv
    base = ["--output_dir", str(tmp_path / "o"), "--pretrained_hf_model", str(tmp_path), "--synthetic_steps", "2"]
    assert drv.build_parser().parse_args(base).decode_context == "last"
    assert drv.build_parser().parse_args(base + ["--decode_context", "prefix"]).decode_context == "prefix"
    with pytest.raises(SystemExit):
        drv.build_parser().parse_args(base + ["--decode_context", "all"])
    with pytest.raises(ValueError, match="--beam_size 17"):
        drv.main(base + ["--do_eval", "--decode_context", "prefix", "--beam_size", "17"])
    with pytest.raises(ValueError, match="--max_len_decoder 513"):
        drv.main(base + ["--do_eval", "--decode_context", "prefix", "--max_len_decoder", "513"])
    assert not (tmp_path / "o").exists()
