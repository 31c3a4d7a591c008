"""Attention maps of the fusion layers (ops.set_output_fusion_attentions, FCMFEncoder.fusion_attentions,
BoxMultiHeadedAttention.box_attn) against what the REFERENCE computes in the same places
(tests/golden/fusion_attentions.npz, tools/make_fusion_attention_golden.py: the tiny geometry, the weights and inputs of
fcmf_tiny.npz, eval mode), across aspect batching, with the switch on and off, and through the fine-tuning driver's
--dump_attention_maps.

Bounds.  fp32 against the fixture: 3e-5 absolute (the bound of the probability kernels, test_attn_probs_gpu.py; the values
are probabilities, at most 1) and 1e-3 relative to the largest reference value (the level of the fp32 `inter_*` comparisons
of test_parity_gpu.py) -- both.  bf16: that file's scale-aware bound, 2e-2 x |ref|max.  Aspect batching in fp32 changes only
the row counts of the GEMMs in front of the maps: 1e-5 absolute, two orders above float32 rounding of O(1) scores."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLD
from helpers import batch_to, build_fcmf, make_hf_dir, max_err
import synthetic_data as synth

pytestmark = pytest.mark.gpu

NAMES = ("text2img", "text2roi", "fusion", "box")


@pytest.fixture(scope="module")
def tiny(dev):
    z = np.load(os.path.join(GOLD, "fusion_attentions.npz"))
    B, S, NI, NR = int(z["B"]), int(z["S"]), int(z["NI"]), int(z["NR"])
    model, _ = build_fcmf(synth.TINY_CFG, NI, NR, dev)
    model.eval()
    batch = batch_to(synth.synth_batch(B, synth.TINY_CFG, S=S, num_imgs=NI, num_roi=NR, seed=42), dev)
    assert batch["input_ids"].shape[1] == int(z["A"])
    return z, model, batch


def _set(dtype):
    from fcmf_framework import ops
    ops.set_compute_dtype(dtype)
    ops.shadows.clear()


def _aspects(model, b, sl=slice(None)):
    return model.forward_aspects(b["input_ids"][:, sl], b["visual_embeds_att"], b["roi_embeds_att"], b["roi_coors"],
                                 b["token_type_ids"][:, sl], b["attention_mask"][:, sl], b["added_attention_mask"][:, sl])


def _maps(model, b, sl=slice(None)):
    """forward_aspects with the switch on -> logits, {name: CPU tensor}; the switch is off again afterwards"""
    from fcmf_framework import ops
    ops.set_output_fusion_attentions(True)
    try:
        with torch.no_grad():
            logits = _aspects(model, b, sl)
        fa = model.encoder.fusion_attentions
        assert set(fa) == set(NAMES) and fa["box"] is model.encoder.box_head.box_attn
        assert all(t.dtype == torch.float32 and not t.requires_grad for t in fa.values())
        return logits, {k: v.cpu() for k, v in fa.items()}
    finally:
        ops.set_output_fusion_attentions(False)


def _reference(z):
    """the fixture in the layouts of fusion_attentions: aspects folded into the batch axis, photos into the box batch"""
    B, A, NI = int(z["B"]), int(z["A"]), int(z["NI"])
    r = {k: torch.from_numpy(z[k]) for k in NAMES}
    return {"text2img": r["text2img"].reshape(B * A, *r["text2img"].shape[2:]), "text2roi": r["text2roi"].reshape(B * A, *r["text2roi"].shape[2:]),
            "fusion": r["fusion"].reshape(B * A, *r["fusion"].shape[2:]), "box": r["box"].reshape(B * NI, *r["box"].shape[2:])}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_maps_match_the_reference(tiny, dev, dtype):
    z, model, batch = tiny
    B, A, S, NI, NR = (int(z[k]) for k in ("B", "A", "S", "NI", "NR"))
    heads = synth.TINY_CFG["num_attention_heads"]
    _set(dtype)
    try:
        _, got = _maps(model, batch)
    finally:
        _set(torch.float32)
    ref = _reference(z)
    shapes = {"text2img": (B * A, NI, heads, 49), "text2roi": (B * A, NI, heads, S + NR), "fusion": (B * A, heads, 1 + 2 * NI, 1 + 2 * NI),
              "box": (B * NI, 8, NR, NR)}
    for n in NAMES:
        assert tuple(got[n].shape) == shapes[n] == tuple(ref[n].shape), n
        err, scale = max_err(got[n], ref[n]), ref[n].abs().max().item()
        print(n, dtype, f"err {err:.3e} |ref|max {scale:.4f}")
        assert (got[n].double().sum(-1) - 1).abs().max().item() < 1e-4, n
        if dtype == torch.float32:
            assert err < 3e-5 and err < 1e-3 * scale, (n, err, scale)
        else:
            assert err < 2e-2 * scale, (n, err, scale)


def test_aspect_batching_gives_the_per_aspect_maps(tiny, dev):
    z, model, batch = tiny
    B = int(z["B"])
    _set(torch.float32)
    _, both = _maps(model, batch, slice(0, 2))
    for a in range(2):
        _, one = _maps(model, batch, slice(a, a + 1))
        for n in ("text2img", "text2roi", "fusion"):
            got = both[n].reshape(B, 2, *both[n].shape[1:])[:, a]
            assert got.shape == one[n].shape
            err = max_err(got, one[n])
            print(n, "aspect", a, err)
            assert err < 1e-5, (n, a, err)
        assert max_err(both["box"], one["box"]) < 1e-5         # (does not depend on the aspect)


def test_switch_off_leaves_nothing_and_changes_nothing(tiny, dev):
    from fcmf_framework import ops
    z, model, batch = tiny
    _set(torch.float32)
    assert ops.output_fusion_attentions() is False
    enc = model.encoder
    one = lambda k: batch[k][:, 0]
    args = (one("input_ids"), batch["visual_embeds_att"], batch["roi_embeds_att"], batch["roi_coors"], one("token_type_ids"),
            one("attention_mask"), one("added_attention_mask"))
    ops.set_output_attentions(True)
    try:
        with torch.no_grad():
            off_logits = _aspects(model, batch)
            assert enc.fusion_attentions is None and enc.box_head.box_attn is None
            off_out, off_att = enc(*args)
            assert enc.fusion_attentions is None and enc.box_head.box_attn is None
            on_logits, maps = _maps(model, batch)
            ops.set_output_fusion_attentions(True)
            on_out, on_att = enc(*args)
            ops.set_output_fusion_attentions(False)
            assert enc.fusion_attentions is not None
            _aspects(model, batch)
            assert enc.fusion_attentions is None and enc.box_head.box_attn is None      # cleared by the next forward
    finally:
        ops.set_output_attentions(False)
        ops.set_output_fusion_attentions(False)
    assert torch.equal(on_logits, off_logits) and torch.equal(on_out, off_out)
    assert len(on_att) == len(off_att) == synth.TINY_CFG["num_hidden_layers"]
    assert all(torch.equal(a, b) for a, b in zip(on_att, off_att))


ZERO_GRAD = (".key.bias", "box_head.linears.1.bias")      # analytically zero (softmax shift invariance): rounding noise only


def test_training_step_does_not_change(tiny, dev):
    """train() mode, dropout p = 0, the same seed, the switch off and on.

    The backward of this project is not bit-reproducible from one run to the next: the embedding tables, the LayerNorm and bias
    gradients and the split-K weight gradients are summed with float atomics.  Measured on an MI355X with the switch OFF in
    every run, 61 of the 105 parameter gradients of this very step differed between runs, by up to 3.6e-7 of the gradient's
    largest element (2e-1 for the analytically zero key biases), and a switch-on run differed from a switch-off run by the
    same amounts (at most 3.3e-7) -- `torch.equal` on the gradients fails for the switch-off step against itself.  So what
    "the switch changes nothing" can mean is asserted piece by piece, each as strictly as the step allows:
      * the train()-mode logits are torch.equal (the forward is deterministic);
      * the library calls of forward + backward, in order and with every scalar argument, are identical once the four
        probability launches (box, text2img, text2roi, fusion) are taken out of the switch-on record: nothing else is added,
        nothing in the backward moves;
      * every gradient agrees within 1e-5 of its largest element -- 170 float32 ulps, 30 times the measured reordering noise,
        three orders below what another dropout mask or a changed saved tensor would do; the analytically zero gradients,
        which are rounding noise only, are left out as in test_parity_gpu.py."""
    from fcmf_framework import ops
    from helpers import _recorded
    z, model, batch = tiny
    _set(torch.float32)
    drops = [m for m in model.modules() if isinstance(m, torch.nn.Dropout)]
    saved = [m.p for m in drops]
    grads, logits, calls = {}, {}, {}
    try:
        for m in drops:
            m.p = 0.0
        model.train()
        for on in (False, True):
            ops.set_output_fusion_attentions(on)
            ops.manual_seed(11)
            model.zero_grad(set_to_none=True)

            def step():
                logits[on] = _aspects(model, batch)
                model.loss_aspects(logits[on], batch["labels"]).backward()
            calls[on] = _recorded(step)
            assert (model.encoder.fusion_attentions is not None) == on
            grads[on] = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    finally:
        ops.set_output_fusion_attentions(False)
        for m, p in zip(drops, saved):
            m.p = p
        model.eval()
        model.zero_grad(set_to_none=True)
    assert torch.equal(logits[True], logits[False])
    probs = ("fcmf_attn_probs", "fcmf_attn_mfma_probs", "fcmf_attn_mfma_long_probs")
    assert not [c for c in calls[False] if c[0] in probs]
    assert len([c for c in calls[True] if c[0] in probs]) == 4
    assert [c for c in calls[True] if c[0] not in probs] == calls[False]
    assert set(grads[True]) == set(grads[False]) and len(grads[True]) > 20
    worst = ("", 0.0)
    for n, g in grads[False].items():
        if n.endswith(ZERO_GRAD):
            continue
        e = ((grads[True][n] - g).abs().max() / (g.abs().max() + 1e-30)).item()
        worst = max(worst, (n, e), key=lambda t: t[1])
    print("largest gradient difference, switch on vs off:", worst)
    assert worst[1] < 1e-5, worst


def test_driver_dumps_attention_maps(tmp_path, dev):
    """one synthetic test-set pass of run_multimodal_fcmf.py with --dump_attention_maps"""
    import run_multimodal_fcmf as drv
    from fcmf_framework import ops
    hf = make_hf_dir(synth.TINY_CFG)
    out = str(tmp_path / "maps")
    try:
        drv.main(["--output_dir", out, "--pretrained_hf_model", hf, "--do_eval", "--num_imgs", "2", "--num_rois", "5",
                  "--eval_batch_size", "2", "--synthetic_steps", "4", "--max_seq_length", "16", "--seed", "3", "--dump_attention_maps"])
    finally:
        ops.set_compute_dtype(torch.float32)
    assert ops.output_fusion_attentions() is False
    z = np.load(os.path.join(out, "test_attention_maps.npz"))
    N, A = 4, 6                                                    # 2 test batches of 2 reviews, the 6 default aspects
    assert z["patches"].shape == (N, A, 2, 49) and z["rois"].shape == (N, A, 2, 5) and z["roi_mass"].shape == (N, A, 2)
    for k in ("patches", "rois"):
        assert z[k].dtype == np.float32 and (z[k] >= 0).all()
        assert np.abs(z[k].astype(np.float64).sum(-1) - 1).max() < 1e-4, k
    assert ((z["roi_mass"] > 0) & (z["roi_mass"] < 1)).all()
    assert os.path.exists(os.path.join(out, "test_results_fcmf.txt"))
