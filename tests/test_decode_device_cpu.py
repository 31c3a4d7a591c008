"""The host side of the device decode loop, without a GPU: decoding.rebuild_beams / rebuild_chains on hand-written state buffers
(every branch of `fin = final if final else beams`, `_best` with and without a length penalty), the driver's two flags, the
ValueErrors before any launch, and loop="host" handing `beam_rounds` / `sample_rounds` exactly the arguments it always did."""
import inspect

import pytest
import torch

START, SEP = 0, 2


def _state(W, max_len, slots, finished):
    """host lists as beam_rounds_device reads them back.  slots: per sample [(score, state, seq)] (seq padded here); finished: per
    sample [(score, seq)]"""
    S = max_len + 1
    pad = lambda s: list(s) + [9] * (S - len(s))                 # 9: what lies behind a sequence's length must not be read
    score = [x[0] for smp in slots for x in smp]
    state = [x[1] for smp in slots for x in smp]
    rows = [pad(x[2]) for smp in slots for x in smp]
    seq = [[r[p] for r in rows] for p in range(S)]
    n = max(max(len(f) for f in finished), 1)
    fin_count = [len(f) for f in finished]
    fin_score = [[e[0] for e in f] + [0.0] * (n - len(f)) for f in finished]
    fin_len = [[len(e[1]) for e in f] + [0] * (n - len(f)) for f in finished]
    fin_seq = [[pad(e[1]) for e in f] + [[9] * S] * (n - len(f)) for f in finished]
    return score, state, seq, fin_count, fin_score, fin_len, fin_seq


def test_rebuild_beams_every_branch_of_the_fin_rule():
    from fcmf_framework import decoding
    W, max_len = 2, 3
    slots = [
        # sample 0: nothing finished, both beams live: fin = the beams in slot order, full length
        [(-1.0, 1, [0, 5, 6, 7]), (-1.5, 1, [0, 5, 4, 3])],
        # sample 1: nothing finished before, one beam ended in the last round: it IS in fin (fin = beams)
        [(-2.0, 2, [0, 4, 4, SEP]), (-0.5, 1, [0, 4, 4, 6])],
        # sample 2: a finished list, and a beam that ended in the last round: that beam is NOT in fin
        [(-0.25, 2, [0, 3, 3, SEP]), (-3.0, 1, [0, 3, 3, 5])],
        # sample 3: done early; finished entries of different lengths, in append order (not sorted)
        [(-9.0, 2, [0, SEP, SEP, SEP]), (-9.0, 2, [0, 7, SEP, SEP])],
    ]
    finished = [[], [], [(-4.0, [0, SEP])], [(-3.0, [0, 7, SEP]), (-1.0, [0, SEP]), (-1.0, [0, 6, SEP])]]
    got = decoding.rebuild_beams(*_state(W, max_len, slots, finished), W, 0.0)
    assert got[0] == ([0, 5, 6, 7], -1.0, [(-1.0, [0, 5, 6, 7]), (-1.5, [0, 5, 4, 3])])
    assert got[1] == ([0, 4, 4, 6], -0.5, [(-2.0, [0, 4, 4, SEP]), (-0.5, [0, 4, 4, 6])])
    assert got[2] == ([0, SEP], -4.0, [(-4.0, [0, SEP])])
    assert got[3] == ([0, SEP], -1.0, [(-3.0, [0, 7, SEP]), (-1.0, [0, SEP]), (-1.0, [0, 6, SEP])])      # first among equals
    for g in got:
        assert all(isinstance(s, float) for s, _ in g[2]) and all(9 not in q for _, q in g[2])
    # the length penalty changes the choice, never the list or the returned (raw) score
    pen = decoding.rebuild_beams(*_state(W, max_len, slots, finished), W, 1.0)
    assert [p[2] for p in pen] == [g[2] for g in got]
    assert pen[3][:2] == ([0, 6, SEP], -1.0)                     # -1 / 2 beats -1 / 1 and -3 / 2
    assert pen[1][:2] == ([0, 4, 4, 6], -0.5)
    for b in range(4):
        assert pen[b][:2] == decoding._best(got[b][2], 1.0)[::-1]


def test_rebuild_beams_skips_empty_slots():
    """a state that never ran a round (max_len rounds always fill every slot; this is the shape of the initial state)"""
    from fcmf_framework import decoding
    got = decoding.rebuild_beams(*_state(3, 1, [[(0.0, 1, [0]), (0.0, 0, [0]), (0.0, 0, [0])]], [[]]), 3)
    assert got[0][2] == [(0.0, [0, 9])]


def test_rebuild_chains():
    from fcmf_framework import decoding
    score = [-2.0, -1.0, -1.0, -0.5]
    length = [4, 2, 3, 4]
    rows = [[0, 5, 6, 7], [0, SEP, SEP, SEP], [0, 4, SEP, SEP], [0, 3, 3, 3]]
    seq = [[r[p] for r in rows] for p in range(4)]
    got = decoding.rebuild_chains(score, length, seq, 2, 0.0)
    assert got == [([0, SEP], -1.0, [(-2.0, [0, 5, 6, 7]), (-1.0, [0, SEP])]), ([0, 3, 3, 3], -0.5, [(-1.0, [0, 4, SEP]), (-0.5, [0, 3, 3, 3])])]
    pen = decoding.rebuild_chains(score, length, seq, 2, 1.0)
    assert pen[0][:2] == ([0, 5, 6, 7], -2.0) and pen[1][:2] == ([0, 3, 3, 3], -0.5)      # -2 / 3 beats -1 / 1
    one = decoding.rebuild_chains(score, length, seq, 1, 0.0)
    assert len(one) == 4 and one[2] == ([0, 4, SEP], -1.0, [(-1.0, [0, 4, SEP])])


def test_parser_flags_and_defaults():
    import run_pretraining_fcmf as drv
    p = drv.build_parser()
    base = ["--output_dir", "x"] if any(a.dest == "output_dir" and a.required for a in p._actions) else []
    need = [a for a in p._actions if a.required and a.dest != "output_dir"]
    base += [s for a in need for s in (a.option_strings[0], "1")]
    args = p.parse_args(base)
    assert args.decode_loop == "host" and args.decode_poll_every == 4
    args = p.parse_args(base + ["--decode_loop", "device", "--decode_poll_every", "0"])
    assert args.decode_loop == "device" and args.decode_poll_every == 0
    with pytest.raises(SystemExit):
        p.parse_args(base + ["--decode_loop", "graph"])


def test_value_errors_come_before_any_work():
    """the checks are the first thing the entry points do: `model` is never touched (None would raise AttributeError)"""
    from fcmf_framework import decoding
    a = (None, START, SEP) + (None,) * 7
    with pytest.raises(ValueError, match="beam_size"):
        decoding.beam_search_ids_batch(*a, beam_size=9, loop="device")
    with pytest.raises(ValueError, match="beam_size"):
        decoding.beam_search_ids(*a, beam_size=9, loop="device")
    with pytest.raises(ValueError, match="max_len"):
        decoding.beam_search_ids_batch(*a, beam_size=3, max_len=512, loop="device")
    with pytest.raises(ValueError, match="num_chains"):
        decoding.sample_ids_batch(*a, num_chains=9, loop="device")
    with pytest.raises(ValueError, match="loop"):
        decoding.beam_search_ids_batch(*a, loop="graph")
    with pytest.raises(ValueError, match="loop"):
        decoding.sample_ids_batch(*a, loop="graph")
    with pytest.raises(ValueError, match="poll_every"):
        decoding._run_device_rounds(dict(max_len=3), lambda t: None, -1)
    # the host loop has no such limit: beam_size 9 passes the check (and fails later, on the None model)
    with pytest.raises(AttributeError):
        decoding.beam_search_ids_batch(*a, beam_size=9)


class _Dec(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.dense = torch.nn.Linear(4, 64)

    def project_encoder(self, enc):
        return ["keys"]

    def init_cache(self, max_len, rows, device):
        return ["cache", max_len, rows]


class _Model(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.decoder = _Dec()

    def encoder(self, enc_ids, *a):
        return torch.zeros(enc_ids.shape[0], 3, 4)


@pytest.mark.parametrize("context", ["last", "prefix"])
def test_host_loop_hands_beam_rounds_todays_arguments(monkeypatch, context):
    """loop="host", given or defaulted, through every wrapper: `beam_rounds` / `sample_rounds` see the positional and keyword
    arguments of the code before the device loop existed, and the device loops are never entered"""
    from fcmf_framework import decoding
    seen = []
    monkeypatch.setattr(decoding, "beam_rounds", lambda *a, **k: seen.append(("beam", a[1:], k)) or [([0, 5], -1.0, [])] * 2)
    monkeypatch.setattr(decoding, "sample_rounds", lambda *a, **k: seen.append(("sample", a[1:], k)) or [([0, 5], -1.0, [])] * 2)
    boom = lambda *a, **k: pytest.fail("the device loop must not run")
    monkeypatch.setattr(decoding, "beam_rounds_device", boom)
    monkeypatch.setattr(decoding, "sample_rounds_device", boom)
    model = _Model()
    t = torch.zeros(2, 3, dtype=torch.long)
    args = (model, START, SEP, t, t, t, t, t, t, t)
    for kw in ({}, dict(loop="host"), dict(loop="host", poll_every=0)):
        del seen[:]
        decoding.beam_search_ids_batch(*args, beam_size=2, max_len=5, context=context, length_penalty=0.5, **kw)
        decoding.sample_ids_batch(*args, num_chains=2, max_len=5, context=context, sample_offset=7, length_penalty=0.5, **kw)
        if context == "prefix":
            assert seen[0] == ("beam", (2, START, SEP, 2, 5, "prefix", 0.5, None), {})
            assert seen[1] == ("sample", (2, START, SEP, 2, 5, "prefix", 7, 0.5, None), {})
        else:
            assert seen[0] == ("beam", (2, START, SEP, 2, 5), dict(length_penalty=0.5, constraints=None))
            assert seen[1] == ("sample", (2, START, SEP, 2, 5, "last", 7, 0.5, None), {})


def test_wrappers_hand_the_host_loop_no_new_keyword(monkeypatch):
    """beam_search_batch / sample_batch / beam_search / beam_search_ids (batched path): with loop="host" the callee is called with
    exactly the keywords it always got; with loop="device" it also gets loop and poll_every"""
    import synthetic_data as synth
    from fcmf_framework import decoding
    seen = []

    def spy(name, ret):
        def f(*a, **k):
            seen.append((name, sorted(k)))
            return ret
        return f

    monkeypatch.setattr(decoding, "beam_search_ids_batch", spy("beam", [([0, 5], -1.0, [])] * 2))
    monkeypatch.setattr(decoding, "sample_ids_batch", spy("sample", [([0, 5], -1.0, [])] * 2))
    tok = synth.IdTokenizer(dict(vocab_size=64, pad_token_id=1))
    t = torch.zeros(2, 3, dtype=torch.long)
    old_beam = ["beam_size", "constraints", "context", "length_penalty", "max_len"]
    old_sample = ["constraints", "context", "length_penalty", "max_len", "num_chains", "sample_offset", "sampler"]
    decoding.beam_search_batch(_Model(), tok, t, t, t, t, t, t, t)
    decoding.sample_batch(_Model(), tok, t, t, t, t, t, t, t)
    decoding.beam_search(_Model(), tok, t[0], t[0], t[0], t[0], t[0], t[0], t[0], context="prefix")
    assert seen == [("beam", old_beam), ("sample", old_sample), ("beam", old_beam)]
    del seen[:]
    decoding.beam_search_batch(_Model(), tok, t, t, t, t, t, t, t, loop="device", poll_every=2)
    decoding.sample_batch(_Model(), tok, t, t, t, t, t, t, t, loop="device")
    decoding.beam_search(_Model(), tok, t[0], t[0], t[0], t[0], t[0], t[0], t[0], loop="device")      # context "last": the batched path too
    new = ["loop", "poll_every"]
    assert seen == [("beam", sorted(old_beam + new)), ("sample", sorted(old_sample + new)), ("beam", sorted(old_beam + new))]


def test_every_entry_point_takes_loop_and_poll_every():
    import iaog_eval
    from fcmf_framework import decoding
    for fn in (decoding.beam_search_ids_batch, decoding.beam_search_batch, decoding.sample_ids_batch, decoding.sample_batch,
               decoding.beam_search_ids, decoding.beam_search, iaog_eval.generate):
        p = inspect.signature(fn).parameters
        assert p["loop"].default == "host" and p["poll_every"].default == 4, fn.__name__
