"""Batched IAOG decode on the GPU: IAOGDecoder.decode_step (n independent (sample, last token) rows in one pass, plain head
pairing per row) against the existing batch-1 decoder call per row; decoding.beam_search_ids_batch against the reference fixture
iaog_decode.npz with the bounds of test_parity_gpu.test_iaog_beam_search_matches_reference_fixture; iaog_eval.generate and the
pre-training driver with and without batched decode.  Tiny model: H 64, 4 heads, 2 blocks, V 512.  Figures are printed before
they are asserted."""
import logging
import os
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import synthetic_data as synth
from conftest import GOLD
from helpers import batch_to, make_hf_dir

pytestmark = pytest.mark.gpu

NI, NR, S = 2, 5, 16


def _set(dtype):
    from fcmf_framework import ops
    ops.set_compute_dtype(dtype)


def _iaog_model(dev, B):
    from fcmf_framework.fcmf_pretraining import FCMFSeq2Seq
    cfg = synth.TINY_CFG
    V = cfg["vocab_size"]
    model = FCMFSeq2Seq(V, 20, make_hf_dir(cfg), NI, NR, 1.0)
    model.decoder.embedding = torch.nn.Embedding(V, model.decoder.num_hiddens)   # run_pretraining_fcmf.py:189
    shapes = {k: v for k, v in synth.fcmf_param_shapes(cfg).items() if k.startswith("encoder.")}
    shapes.update(synth.iaog_decoder_param_shapes(cfg, V))
    model.load_state_dict(synth.synth_params(shapes), strict=False)
    model = model.to(dev).eval()
    batch = batch_to(synth.synth_batch(B, cfg, S=S, num_imgs=NI, num_roi=NR, seed=5, coord_dtype=torch.float32), dev)
    return model, batch


def _args(batch, sl):
    return (batch["input_ids"][sl, 0], batch["attention_mask"][sl, 0], batch["token_type_ids"][sl, 0],
            batch["added_attention_mask"][sl, 0], batch["visual_embeds_att"][sl], batch["roi_embeds_att"][sl], batch["roi_coors"][sl])


@pytest.mark.parametrize("n", [1, 5, 13])
def test_decode_step_rows_equal_the_batch1_call(dev, n):
    """n = 5, 13: neither 1 nor a multiple of the 4 heads -- a step that kept the batch-size-dependent pairing, or mixed rows up,
    fails.  enc is random per sample (seeds 100..102), NOT the encoder's output of the synthetic batch: that differs by 1.4e-4
    between samples only and would hide a mix-up."""
    model, _ = _iaog_model(dev, 1)
    dec = model.decoder
    Hd, K = dec.num_hiddens, 3
    _set(torch.float32)
    enc = torch.stack([torch.randn(1 + 2 * NI, Hd, generator=torch.Generator().manual_seed(100 + s)) for s in range(3)]).to(dev)
    toks = (0, 7, 123)
    with torch.no_grad():
        ref = {}
        for s in range(3):
            for t in toks:
                lg = dec(torch.tensor([[t]], device=dev), dec.init_state(enc[s:s + 1], None), is_train=False)
                ref[(s, t)] = F.log_softmax(lg[0, -1].float(), dim=-1).cpu()
        # the test's own discriminating power: two samples at the same token are further apart than the tolerance by 10x
        gap = min((ref[(0, t)] - ref[(s, t)]).abs().max().item() for t in toks for s in (1, 2))
        print(f"batch-1 log-probabilities, sample 0 vs another at the same token: max |d| >= {gap:.3e}")
        assert gap > 1e-3
        rng = random.Random(n)
        pairs = [(s, t) for s in range(3) for t in toks]
        rows = [pairs[rng.randrange(9)] for _ in range(n)] if n != 13 else pairs + [pairs[rng.randrange(9)] for _ in range(4)]
        rng.shuffle(rows)
        idx = torch.tensor(rows, device=dev)
        logp, ids = dec.decode_step(idx[:, 1].contiguous(), idx[:, 0].contiguous(), enc, dec.project_encoder(enc), K)
    assert logp.shape == (n, K) and logp.dtype == torch.float32 and ids.dtype == torch.int32
    worst = 0.0
    for i, p in enumerate(rows):
        ws, wi = torch.topk(ref[p], K)
        assert ids[i].cpu().tolist() == wi.tolist(), (i, p)
        worst = max(worst, (logp[i].cpu() - ws).abs().max().item())
    print(f"decode_step n = {n}: top-{K} log-probabilities vs the batch-1 call, max |d| {worst:.3e}")
    assert worst < 1e-4


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_batched_beam_search_matches_reference_fixture(dev, dtype):
    from fcmf_framework import decoding
    z = np.load(os.path.join(GOLD, "iaog_decode.npz"))
    max_len = int(z["geometry"][3])
    model, batch = _iaog_model(dev, 2)
    args = _args(batch, slice(0, 2))
    _set(dtype)
    try:
        res = decoding.beam_search_ids_batch(model, 0, 2, *args, beam_size=2, max_len=max_len)          # SEP 2 never produced
        assert len(res) == 2
        for b, (ids, score, fin) in enumerate(res):
            assert len(ids) == max_len + 1 and ids[0] == 0 and len(fin) == 2
            if dtype == torch.float32:
                assert ids == z[f"s{b}_a_ids"].tolist() and abs(score - float(z[f"s{b}_a_score"])) < 1e-3
                assert np.allclose([f[0] for f in fin], z[f"s{b}_a_final_scores"], atol=1e-3)
        seps = [int(z[f"s{b}_b_sep"]) for b in range(2)]
        for b in range(2):                       # the fixture's SEP is per sample: the batch is decoded with each, its own sample checked
            ids, score, fin = decoding.beam_search_ids_batch(model, 0, seps[b], *args, beam_size=3, max_len=max_len)[b]
            assert ids[0] == 0 and 2 <= len(ids) <= max_len + 1
            if dtype == torch.float32:
                assert ids[-1] == seps[b]
                assert ids == z[f"s{b}_b_ids"].tolist() and abs(score - float(z[f"s{b}_b_score"])) < 1e-3
                assert [len(f[1]) for f in fin] == z[f"s{b}_b_final_lens"].tolist()
    finally:
        _set(torch.float32)


def test_generate_batched_equals_per_sample(dev):
    from iaog_eval import generate
    cfg = synth.TINY_CFG
    model, _ = _iaog_model(dev, 1)
    tok = synth.IdTokenizer(dict(vocab_size=cfg["vocab_size"], pad_token_id=cfg["pad_token_id"]))
    aspects = ["a", "b", "c"]

    def batches():
        s0 = 0
        for B, seed in ((5, 21), (3, 22)):
            b = synth.synth_batch(B, cfg, S=S, num_imgs=NI, num_roi=NR, num_aspects=1, seed=seed, coord_dtype=torch.float32)
            dec = torch.randint(3, cfg["vocab_size"], (B, 6), generator=torch.Generator().manual_seed(seed))
            lab = torch.roll(dec, -1, dims=1)
            lab[:, -1] = -100
            yield (b["visual_embeds_att"], b["roi_embeds_att"], b["roi_coors"], lab, dec, b["input_ids"][:, 0], b["token_type_ids"][:, 0],
                   b["attention_mask"][:, 0], b["added_attention_mask"][:, 0], [aspects[(s0 + k) % 3] for k in range(B)],
                   [f"synthetic review {s0 + k}" for k in range(B)])
            s0 += B

    _set(torch.float32)
    feats = lambda a, b: (a, b)
    one = generate(model, tok, batches(), feats, 2, 6, aspects)
    many = generate(model, tok, batches(), feats, 2, 6, aspects, batched=True)
    assert sum(len(v) for v in one[0].values()) == 8
    assert many == one


ARGS = ["--do_train", "--synthetic_steps", "2", "--synthetic_eval_samples", "6", "--num_train_epochs", "1", "--beam_size", "2",
        "--max_len_decoder", "6", "--num_imgs", "2", "--num_rois", "2", "--train_batch_size", "2", "--eval_batch_size", "4",
        "--synthetic_dec_len", "6", "--max_seq_length", "16", "--seed", "9", "--do_eval"]


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


def test_driver_batched_decode(tmp_path, dev, caplog):
    import run_pretraining_fcmf as drv
    hf = make_hf_dir(synth.TINY_CFG)
    texts, f1 = {}, {}
    for name, extra in (("per_sample", []), ("batched", ["--batched_decode"])):
        out = str(tmp_path / name)
        msgs = _run(drv, out, hf, extra, caplog)
        f1[name] = [float(m.rsplit(" ", 1)[1]) for m in msgs if "[Macro-Avg] F1:" in m]
        lines = open(os.path.join(out, "iaog_test_predictions_formatted.txt"), encoding="utf-8").read().split("\n")
        texts[name] = lines[lines.index("DETAILED PREDICTIONS (Filtered View):"):]
        f1[name].append(float(next(l for l in lines if l.startswith("MACRO AVERAGE")).rsplit(" ", 1)[1]))
    print("macro F1 per sample / batched:", f1)
    assert texts["batched"] == texts["per_sample"] and any(l.startswith("   predict:") for l in texts["batched"])
    assert len(f1["batched"]) == len(f1["per_sample"]) == 2
    assert all(abs(a - b) <= 1e-4 for a, b in zip(f1["batched"], f1["per_sample"]))
