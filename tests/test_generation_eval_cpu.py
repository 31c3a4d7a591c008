"""Host logic of the IAOG generation evaluation (iaog_eval.py, synthetic_data.IdTokenizer, the driver's new flag): no GPU."""
import torch

import synthetic_data as synth

ASPECTS = ['Location', 'Food', 'Room', 'Facilities', 'Service', 'Public_area']


def test_strip_rule_and_its_length_edge():
    from iaog_eval import strip_rule
    assert strip_rule("n sạch sẽ") == "sạch sẽ"
    assert strip_rule("n x") == "x"
    assert strip_rule("n ") == "n "                  # len == 2: nothing would remain, kept (reference :423 `len > 2`)
    assert strip_rule("n") == "n"
    assert strip_rule("no n here") == "no n here"
    assert strip_rule("") == ""


def test_label_decoding_drops_ignore_index():
    from iaog_eval import decode_label
    tok = synth.IdTokenizer(synth.TINY_CFG)
    labels = torch.tensor([17, 300, 5, 2, -100, -100])
    assert decode_label(tok, labels) == "17 300 5"                 # -100 dropped, </s> skipped
    assert decode_label(tok, torch.tensor([-100, -100])) == ""
    assert decode_label(tok, [0, 9, 1, 1, -100]) == "9"            # <s> and pad are special too


class StubScorer:
    """P = 0.5 everywhere, R = 0.25, F = number of characters the pair shares in length / 10"""

    def __init__(self):
        self.calls = []

    def __call__(self, cands, refs):
        self.calls.append((list(cands), list(refs)))
        n = len(cands)
        return torch.full((n,), 0.5), torch.full((n,), 0.25), torch.tensor([min(len(c), len(r)) / 10 for c, r in zip(cands, refs)])


def test_macro_bertscore_bookkeeping():
    from iaog_eval import macro_bertscore
    preds = {'Location': ["ab", "abcd"], 'Food': [], 'Room': ["abcdef"]}
    refs = {'Location': ["abc", "ab"], 'Food': [], 'Room': ["abcdefgh"]}
    stub = StubScorer()
    per, macro = macro_bertscore(preds, refs, ['Location', 'Food', 'Room', 'Service'], stub)
    assert list(per) == ['Location', 'Food', 'Room', 'Service']
    assert per['Food'] is None and per['Service'] is None                     # no samples / not even a key
    assert per['Location'] == (0.5, 0.25, torch.tensor([0.2, 0.2]).mean().item())
    assert abs(per['Room'][2] - 0.6) < 1e-7
    assert len(stub.calls) == 2 and stub.calls[0] == (["ab", "abcd"], ["abc", "ab"])      # one call per aspect WITH samples
    assert macro[0] == 0.5 and macro[1] == 0.25 and abs(macro[2] - 0.4) < 1e-7           # mean over the 2 aspects that have samples
    # nothing anywhere: zeros, and the scorer is never called
    stub = StubScorer()
    per, macro = macro_bertscore({}, {}, ASPECTS, stub)
    assert macro == (0.0, 0.0, 0.0) and all(v is None for v in per.values()) and not stub.calls


EXPECTED = (
    "TEST METRICS (BERTScore with /models/visobert):\n"
    "--------------------------------------------------\n"
    "Location        | P: 0.9123 | R: 0.8000 | F1: 0.8525\n"
    "Food            | (No positive samples)\n"
    "Room            | P: 0.5000 | R: 0.2500 | F1: 0.3333\n"
    "Public_area     | (No positive samples)\n"
    "--------------------------------------------------\n"
    "MACRO AVERAGE   | P: 0.7062 | R: 0.5250 | F1: 0.5929\n"
    "==================================================\n"
    "\n"
    "DETAILED PREDICTIONS (Filtered View):\n"
    "{\n"
    "Sentence 0: phòng đẹp , gần biển\n"
    "Location:\n"
    "   predict: location gần biển\n"
    "   label:   location gần\n"
    "Room:\n"
    "   predict: none\n"
    "   label:   room đẹp\n"
    "}\n"
    "{\n"
    "Sentence 2: chỉ có dự đoán\n"
    "Room:\n"
    "   predict: room ổn\n"
    "   label:   \n"
    "}\n"
)


def test_write_predictions_matches_the_reference_format(tmp_path):
    """literal file from the reference's format lines (run_pretraining_fcmf.py:564-626): metrics block, then the blocks of the texts
    that have something to show -- an aspect whose prediction AND label are 'none' / empty is hidden, a text with nothing left too"""
    from iaog_eval import write_predictions
    per = {'Location': (0.91234, 0.8, 0.85249), 'Food': None, 'Room': (0.5, 0.25, 1 / 3), 'Public_area': None}
    macro = (0.70617, 0.525, 0.59291)
    results = [
        {'text': "phòng đẹp , gần biển", 'aspects': {'Location': {'predict': "location gần biển", 'label': "location gần"},
                                                    'Room': {'predict': "none", 'label': "room đẹp"},
                                                    'Food': {'predict': " None ", 'label': ""}}},
        {'text': "không có gì", 'aspects': {'Food': {'predict': "", 'label': "NONE"}}},
        {'text': "chỉ có dự đoán", 'aspects': {'Room': {'predict': "room ổn", 'label': ""}}},
    ]
    path = tmp_path / "iaog_test_predictions_formatted.txt"
    write_predictions(str(path), "/models/visobert", per, macro, results)
    assert path.read_text(encoding="utf-8") == EXPECTED


def test_id_tokenizer_round_trip():
    tok = synth.IdTokenizer(synth.TINY_CFG)
    assert (tok.bos_token_id, tok.cls_token_id, tok.sep_token_id, tok.pad_token_id) == (0, 0, 2, 1) and len(tok) == 512
    ids = [17, 300, 5, 511]
    text = tok.decode(ids)
    assert text == "17 300 5 511"
    assert tok.encode(text, add_special_tokens=False) == ids
    assert tok.encode(text) == [0] + ids + [2]
    assert tok.decode(torch.tensor([0] + ids + [2, 1, 1]), skip_special_tokens=True) == text
    assert tok.encode("") == [0, 2]                                                        # an empty string is <s> </s>
    assert tok.encode(text, truncation=True, max_length=4) == [0, 17, 300, 2]
    enc = tok(text, max_length=8, padding='max_length', truncation=True)
    assert enc["input_ids"] == [0, 17, 300, 5, 511, 2, 1, 1] and enc["attention_mask"] == [1] * 6 + [0] * 2
    try:
        tok.encode("512")
        raise AssertionError("expected ValueError")
    except ValueError:
        pass


def test_new_flag_defaults_and_scorer_directory_rule(tmp_path):
    import pytest
    import run_pretraining_fcmf as drv
    base = ["--output_dir", str(tmp_path / "o"), "--pretrained_hf_model", str(tmp_path)]
    a = drv.build_parser().parse_args(base)
    assert a.synthetic_eval_samples == 0 and not a.do_eval and a.bert_score_model == 'uitnlp/visobert' and a.beam_size == 2
    # real data: the hub name of the default is not a directory -> refused with the reason
    with pytest.raises(ValueError, match="local model directory"):
        drv.scorer_dir(a)
    # synthetic mode: the default falls back to the --pretrained_hf_model directory; an explicit non-directory is still refused
    a = drv.build_parser().parse_args(base + ["--synthetic_steps", "2"])
    assert drv.scorer_dir(a) == str(tmp_path)
    a = drv.build_parser().parse_args(base + ["--synthetic_steps", "2", "--bert_score_model", str(tmp_path / "missing")])
    with pytest.raises(ValueError, match="local model directory"):
        drv.scorer_dir(a)
