"""IAOG generation evaluation on the GPU: the encoder stopped after `num_layers` layers, the BERTScore scorer against sentences
encoded alone, and the pre-training driver's --do_eval path in synthetic mode (beam-search decode -> BERTScore -> best checkpoint ->
formatted test log).  Every comparison prints its figure before it asserts."""
import logging
import os
import re

import numpy as np
import pytest
import torch

import synthetic_data as synth
from bertscore_ref import ref_scores
from helpers import make_hf_dir

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]


def tiny_roberta(dev, layers=2):
    from fcmf_framework.roberta import RobertaConfig, RobertaModel
    cfg = dict(synth.TINY_CFG, num_hidden_layers=layers)
    m = RobertaModel(RobertaConfig(**cfg))
    m.load_state_dict(synth.synth_params(synth.roberta_param_shapes(cfg)))
    return m.to(dev).eval()


def sentences(lengths, seed):
    """token-id lists <s> ... </s> of the given lengths (2 = the two special tokens only)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    return [[0] + [int(t) for t in rng.integers(3, synth.TINY_CFG["vocab_size"], size=l - 2)] + [2] for l in lengths]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_encode_num_layers(dtype, dev):
    from fcmf_framework import ops
    two, one = tiny_roberta(dev, 2), tiny_roberta(dev, 1)       # synthetic weights are keyed by name: layer 0 and the embeddings agree
    for k, v in one.state_dict().items():
        assert torch.equal(v, two.state_dict()[k]), k
    b = synth.synth_batch(3, synth.TINY_CFG, S=24, num_imgs=1, num_roi=1, num_aspects=1, seed=4)
    ids, mask = b["input_ids"][:, 0].to(dev), b["attention_mask"][:, 0].to(dev)
    ops.set_compute_dtype(dtype)
    try:
        with torch.no_grad():
            today = two.encode(ids, None, mask)
            assert torch.equal(two.encode(ids, None, mask, num_layers=None), today)
            assert torch.equal(two.encode(ids, None, mask, num_layers=2), today)
            assert torch.equal(two.encode(ids, None, mask, num_layers=7), today)
            first = two.encode(ids, None, mask, num_layers=1)
            assert torch.equal(first, one.encode(ids, None, mask))
            assert not torch.equal(first, today)
    finally:
        ops.set_compute_dtype(torch.float32)


LENGTHS_C = [2, 5, 38, 17, 3, 24, 9, 31, 12]      # candidate 0 is <s> </s> only
LENGTHS_R = [7, 38, 4, 16, 29, 2, 11, 20, 33]


def _alone(scorer, ids):
    """float64 scores from embeddings of every sentence encoded ALONE (batch of 1, no padding)"""
    def emb(s):
        e, l = scorer.embed([s])
        assert e.shape[:2] == (1, len(s)) and int(l[0]) == len(s)
        return e[0].double().cpu().numpy()
    out = []
    for c, r in zip(*ids):
        w = lambda n: np.array([[0.0] + [1.0] * (n - 2) + [0.0]])
        out.append(ref_scores(emb(c)[None], emb(r)[None], [len(c)], [len(r)], w(len(c)), w(len(r)))[0])
    return np.stack(out)


def test_score_ids_against_sentences_encoded_alone(dev):
    from fcmf_framework import ops
    from fcmf_framework.bertscore import BertScorer
    ops.set_compute_dtype(torch.float32)
    scorer = BertScorer(tiny_roberta(dev), num_layers=12, batch_size=4)      # clamped to the depth; 3 encoder batches a side
    assert scorer.num_layers == 2 and scorer.max_tokens == 38
    cands, refs = sentences(LENGTHS_C, 1), sentences(LENGTHS_R, 2)
    P, R, F = scorer.score_ids(cands, refs)
    got = torch.stack([P, R, F], 1)
    assert got.shape == (9, 3) and got.dtype == torch.float32 and torch.isfinite(got).all()
    want = _alone(scorer, (cands, refs))
    err = np.abs(got.double().cpu().numpy() - want).max()
    print(f"score_ids vs sentences encoded alone (f32): max |d| {err:.3e}; F {got[:, 2].tolist()}")
    assert err <= 1e-4
    assert torch.equal(got[0], torch.zeros(3, device=dev))                   # the <s> </s> candidate: weight sum 0
    assert torch.equal(got[5, :], torch.zeros(3, device=dev))                # and the <s> </s> reference
    # input order: a shuffle of the pairs permutes the scores the same way
    perm = [4, 0, 8, 2, 6, 1, 7, 3, 5]
    Pp, Rp, Fp = scorer.score_ids([cands[i] for i in perm], [refs[i] for i in perm])
    d = (torch.stack([Pp, Rp, Fp], 1) - got[perm]).abs().max().item()
    print(f"shuffled inputs: max |d| {d:.3e}")
    assert d <= 1e-5


def test_score_ids_bf16_against_float64_matching_of_its_own_embeddings(dev):
    from fcmf_framework import ops
    from fcmf_framework.bertscore import BertScorer
    ops.set_compute_dtype(torch.bfloat16)
    try:
        scorer = BertScorer(tiny_roberta(dev), num_layers=2, batch_size=4)
        cands, refs = sentences(LENGTHS_C, 1), sentences(LENGTHS_R, 2)
        P, R, F = scorer.score_ids(cands, refs)
        ce, cl = scorer.embed(cands)
        re_, rl = scorer.embed(refs)
        assert ce.dtype == torch.bfloat16
        cl, rl = cl.tolist(), rl.tolist()
        w = lambda lens, L: np.stack([np.r_[0.0, np.ones(max(l - 2, 0)), 0.0, np.zeros(L - l)] for l in lens])
        want = ref_scores(ce.double().cpu().numpy(), re_.double().cpu().numpy(), cl, rl, w(cl, ce.shape[1]), w(rl, re_.shape[1]))
        err = np.abs(torch.stack([P, R, F], 1).double().cpu().numpy() - want).max()
        print(f"score_ids bf16 vs float64 matching of the same embeddings: max |d| {err:.3e}")
        assert err <= 1e-4
    finally:
        ops.set_compute_dtype(torch.float32)


def test_text_path_through_id_tokenizer(dev):
    """score(texts) = score_ids(ids) when the texts are the ids' decimal spelling; '' is <s> </s>"""
    from fcmf_framework import ops
    from fcmf_framework.bertscore import BertScorer
    ops.set_compute_dtype(torch.float32)
    tok = synth.IdTokenizer(synth.TINY_CFG)
    scorer = BertScorer(tiny_roberta(dev))
    cands, refs = sentences([6, 2, 11], 3), sentences([9, 5, 11], 4)
    text = lambda ss: [" " + tok.decode(s, skip_special_tokens=True) + " " for s in ss]
    assert text(cands)[1].strip() == ""
    a = torch.stack(scorer.score(text(cands), text(refs), tok))
    b = torch.stack(scorer.score_ids(cands, refs))
    assert torch.equal(a, b)


ARGS = ["--do_train", "--synthetic_steps", "3", "--synthetic_eval_samples", "4", "--num_train_epochs", "2", "--beam_size", "2",
        "--max_len_decoder", "6", "--num_imgs", "2", "--num_rois", "2", "--train_batch_size", "2", "--eval_batch_size", "3",
        "--synthetic_dec_len", "6", "--max_seq_length", "16", "--seed", "9"]
LINE = re.compile(r"^(\S+)\s+\| P: (-?\d\.\d{4}) \| R: (-?\d\.\d{4}) \| F1: (-?\d\.\d{4})$")


def _run(drv, out, hf, extra, caplog):
    from fcmf_framework import ops
    caplog.clear()
    try:
        with caplog.at_level(logging.INFO, logger="iaog"):
            drv.main(["--output_dir", out, "--pretrained_hf_model", hf] + ARGS + extra)
    finally:
        ops.set_compute_dtype(torch.float32)
        lg = logging.getLogger("iaog")
        for h in list(lg.handlers):                         # the driver adds its handlers per run
            lg.removeHandler(h)
            h.close()
    return [r.getMessage() for r in caplog.records]


def test_driver_synthetic_eval(tmp_path, dev, caplog):
    import run_pretraining_fcmf as drv
    from review_batches import ASPECTS
    hf = make_hf_dir(synth.TINY_CFG)
    # ---- without --do_eval: exactly the files of the driver as it was, whatever --synthetic_eval_samples says
    plain = str(tmp_path / "plain")
    _run(drv, plain, hf, [], caplog)
    assert sorted(os.listdir(plain)) == ["pretraining_iaog.log", "seed_9_iaog_model_last.pth"]
    assert torch.load(os.path.join(plain, "seed_9_iaog_model_last.pth"), map_location="cpu", weights_only=True)["best_score"] == 0.0
    # ---- a scorer path that is no directory: refused before anything is trained or written
    bad = str(tmp_path / "bad")
    with pytest.raises(ValueError, match="local model directory"):
        drv.main(["--output_dir", bad, "--pretrained_hf_model", hf] + ARGS + ["--do_eval", "--bert_score_model", str(tmp_path / "nope")])
    assert not os.path.exists(bad)
    # ---- --do_eval
    out = str(tmp_path / "eval")
    msgs = _run(drv, out, hf, ["--do_eval"], caplog)
    assert sorted(os.listdir(out)) == ["iaog_test_predictions_formatted.txt", "pretraining_iaog.log", "seed_9_iaog_model_best.pth",
                                       "seed_9_iaog_model_last.pth"]
    f1 = [float(m.rsplit(" ", 1)[1]) for m in msgs if "[Macro-Avg] F1:" in m]
    print("epoch macro F1:", f1)
    assert len(f1) == 2
    last = torch.load(os.path.join(out, "seed_9_iaog_model_last.pth"), map_location="cpu", weights_only=True)
    best = torch.load(os.path.join(out, "seed_9_iaog_model_best.pth"), map_location="cpu", weights_only=True)
    assert last["epoch"] == 1 and -1.0 <= last["best_score"] <= 1.0
    assert abs(last["best_score"] - max(f1)) < 5e-5 and best["best_score"] == last["best_score"]     # (the log rounds to 4 places)
    assert best["epoch"] in (0, 1) and (best["epoch"] == 0 or f1[1] >= f1[0])
    lines = open(os.path.join(out, "iaog_test_predictions_formatted.txt"), encoding="utf-8").read().split("\n")
    assert lines[0] == f"TEST METRICS (BERTScore with {hf}):" and lines[1] == "-" * 50
    metric = lines[2:2 + len(ASPECTS)]
    assert [l.split()[0] for l in metric] == list(ASPECTS)                    # one line per aspect, in order
    scored = [LINE.match(l) for l in metric[:4]]                              # 4 samples -> the first 4 aspects have one each
    assert all(scored) and all(l.endswith("| (No positive samples)") for l in metric[4:])
    macro = LINE.match(lines[3 + len(ASPECTS)].replace("MACRO AVERAGE", "MACRO_AVERAGE"))
    assert lines[2 + len(ASPECTS)] == "-" * 50 and macro
    for k in (2, 3, 4):
        mean = sum(float(m.group(k)) for m in scored) / 4
        assert abs(float(macro.group(k)) - mean) <= 1e-4, (k, macro.group(k), mean)
    assert "DETAILED PREDICTIONS (Filtered View):" in lines and sum(l.startswith("Sentence ") for l in lines) == 4
    # ---- resume carries best_score on
    _run(drv, out, hf, ["--do_eval", "--num_train_epochs", "3", "--resume_from_checkpoint", os.path.join(out, "seed_9_iaog_model_last.pth")], caplog)
    again = torch.load(os.path.join(out, "seed_9_iaog_model_last.pth"), map_location="cpu", weights_only=True)
    assert again["epoch"] == 2 and again["best_score"] >= last["best_score"]


def test_driver_synthetic_eval_with_extractors(tmp_path, dev, caplog):
    """--synthetic_pixels: the trunks run inside the decode too, and their checkpoints sit beside the model's"""
    import run_pretraining_fcmf as drv
    hf = make_hf_dir(synth.TINY_CFG)
    out = str(tmp_path / "px")
    _run(drv, out, hf, ["--do_eval", "--synthetic_pixels", "64", "--num_train_epochs", "1", "--synthetic_steps", "1",
                        "--synthetic_eval_samples", "2", "--bf16"], caplog)
    want = [f"seed_9_{t}_model_{k}.pth" for t in ("iaog", "resimg", "resroi") for k in ("best", "last")]
    assert sorted(os.listdir(out)) == sorted(want + ["iaog_test_predictions_formatted.txt", "pretraining_iaog.log"])
    ck = torch.load(os.path.join(out, "seed_9_resimg_model_best.pth"), map_location="cpu", weights_only=True)
    assert ck["best_score"] == torch.load(os.path.join(out, "seed_9_iaog_model_last.pth"), map_location="cpu", weights_only=True)["best_score"]
