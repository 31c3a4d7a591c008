"""Generation evaluation of the IAOG pre-training driver: beam-search decode of every sample, BERTScore of the decoded text against
the label text, macro average over the aspects, and the formatted test log.  The reference keeps this half commented out
(run_pretraining_fcmf.py:376-452 dev leg, :462-632 test leg); file:line citations are into it.  The decode is
`fcmf_framework.decoding.beam_search`, the score `fcmf_framework.bertscore` (the project's encoder + csrc/bertscore.hip)."""
import torch

from fcmf_framework.decoding import beam_search, beam_search_batch, make_constraints, sample_batch


def strip_rule(pred_text):
    """the reference's clean-up of a decoded prediction (:423, :544): a leading "n " goes, unless nothing would remain"""
    if pred_text.startswith("n ") and len(pred_text) > 2:
        return pred_text[2:]
    return pred_text


def decode_label(tokenizer, labels):
    """label ids -> text: ignore_index positions (-100) dropped (:539-541), special tokens skipped"""
    ids = [int(t) for t in (labels.tolist() if hasattr(labels, "tolist") else labels) if int(t) != -100]
    return tokenizer.decode(ids, skip_special_tokens=True)


@torch.no_grad()
def generate(model, tokenizer, batches, features, beam_size, max_len, aspects=(), batched=False, context="last",
             strategy="beam", sampler=None, num_chains=1, length_penalty=0.0, constraints=None, loop="host", poll_every=4):
    """decode every sample of every batch (:385-426, :499-557).  A batch is the dataset's 11-tuple (images, ROI crops, boxes,
    labels, decoder ids, encoder ids / type / mask / added mask, aspect names, texts) on any device; `features` is
    train_harness.make_features' closure, called once per batch; the beam search runs per sample, or -- batched=True -- once per
    batch, every sample advancing one beam round per decoder call (decoding.beam_search_batch: the same beam rules per sample).
    context="prefix": every decode step is conditioned on the beam's whole prefix instead of its last token (decoding.py's header).
    strategy="sample": `num_chains` sampled chains per sample instead of a beam (decoding.sample_batch; always the batched step),
    `sampler` = decoding.make_sampler's settings; the running sample index is carried across the batches, so a sample's text does
    not depend on the batch size.  length_penalty: the final choice among the finished beams / the chains (decoding.py's header).
    constraints: decoding.make_constraints' settings (repetition penalty, n-gram blocking, minimum length, suppressed ids, on the
    step's logits: csrc/constrain.hip); any of them on implies the batched step.
    loop="device": the beam / chain bookkeeping runs on the device (csrc/beam.hip, decoding.py's header: no upload and no read per
    round but a poll of the done flags every `poll_every` rounds); implies the batched step.  "host" (default): the host loops.
    -> (preds, refs, results): {aspect: [text]} twice (every name of `aspects` present, in that order, then any other in order of
    appearance) and the per-text grouping [{'text': ..., 'aspects': {aspect: {'predict', 'label'}}}] in order of first appearance."""
    device = next(model.parameters()).device
    model.eval()
    if strategy not in ("beam", "sample"):
        raise ValueError(f"strategy must be 'beam' or 'sample', got {strategy!r}")
    constraints = make_constraints(constraints)
    batched = batched or constraints is not None or loop == "device"
    loop_kw = {} if loop == "host" else dict(loop=loop, poll_every=poll_every)
    preds, refs = {a: [] for a in aspects}, {a: [] for a in aspects}
    by_text = {}
    seen = 0                                   # samples decoded so far: the sampling counters' sample_offset
    for batch in batches:
        t_img, roi_img, coors, labels, _, enc_ids, enc_type, enc_mask, added, names, texts = batch
        t_img, roi_img, coors, enc_ids, enc_type, enc_mask, added = (
            t.to(device) for t in (t_img, roi_img, coors, enc_ids, enc_type, enc_mask, added))
        vis, roi = features(t_img, roi_img)
        if strategy == "sample":
            texts_b = sample_batch(model, tokenizer, enc_ids, enc_mask, enc_type, added, vis, roi, coors.float(), num_chains=num_chains,
                                   max_len=max_len, context=context, sampler=sampler, sample_offset=seen, length_penalty=length_penalty,
                                   constraints=constraints, **loop_kw)
        else:
            texts_b = beam_search_batch(model, tokenizer, enc_ids, enc_mask, enc_type, added, vis, roi, coors.float(), beam_size=beam_size,
                                        max_len=max_len, context=context, length_penalty=length_penalty,
                                        constraints=constraints, **loop_kw) if batched else None
        seen += enc_ids.shape[0]
        for i in range(enc_ids.shape[0]):
            pred = texts_b[i] if texts_b is not None else beam_search(
                model=model, tokenizer=tokenizer, enc_ids=enc_ids[i], enc_mask=enc_mask[i], enc_type=enc_type[i],
                add_mask=added[i], vis_embeds=vis[i], roi_embeds=roi[i], roi_coors=coors[i].float(),
                beam_size=beam_size, max_len=max_len, device=device, context=context, length_penalty=length_penalty)[0]
            pred = strip_rule(pred)
            label = decode_label(tokenizer, labels[i])
            name, text = names[i], texts[i]
            preds.setdefault(name, []).append(pred)
            refs.setdefault(name, []).append(label)
            by_text.setdefault(text, {'text': text, 'aspects': {}})['aspects'][name] = {"predict": pred, "label": label}
    return preds, refs, list(by_text.values())


def macro_bertscore(preds, refs, aspects, scorer):
    """scorer(cands, refs) -> (P, R, F) tensors, one value per pair.  -> (per_aspect, macro): per_aspect[a] = (mean P, mean R,
    mean F) or None for an aspect without samples, in the order of `aspects`; macro = the mean of those triples over the aspects
    that have samples, zeros when none has (:432-440, :573-592)."""
    per_aspect = {}
    tot, count = [0.0, 0.0, 0.0], 0
    for a in aspects:
        if len(preds.get(a, ())) > 0:
            P, R, F = scorer(preds[a], refs[a])
            m = (P.mean().item(), R.mean().item(), F.mean().item())
            per_aspect[a] = m
            tot = [t + v for t, v in zip(tot, m)]
            count += 1
        else:
            per_aspect[a] = None
    macro = tuple(t / count for t in tot) if count > 0 else (0.0, 0.0, 0.0)
    return per_aspect, macro


def aspect_line(a, m):
    return f"{a:<15} | P: {m[0]:.4f} | R: {m[1]:.4f} | F1: {m[2]:.4f}"


def write_predictions(path, model_name, per_aspect, macro, results):
    """iaog_test_predictions_formatted.txt in the reference's format (:564-626): the metrics block, then one { Sentence i: ... }
    block per text, showing the aspects where the prediction or the label is something other than 'none' / empty"""
    with open(path, "w", encoding="utf-8") as f:
        f.write(f"TEST METRICS (BERTScore with {model_name}):\n")
        f.write("-" * 50 + "\n")
        for a, m in per_aspect.items():
            f.write(aspect_line(a, m) + "\n" if m is not None else f"{a:<15} | (No positive samples)\n")
        f.write("-" * 50 + "\n")
        f.write(f"MACRO AVERAGE   | P: {macro[0]:.4f} | R: {macro[1]:.4f} | F1: {macro[2]:.4f}\n")
        f.write("=" * 50 + "\n\n")
        f.write("DETAILED PREDICTIONS (Filtered View):\n")
        for i, sample in enumerate(results):
            buf = []
            for a in per_aspect:
                res = sample['aspects'].get(a, {'predict': 'none', 'label': 'none'})
                pred, label = str(res['predict']).strip(), str(res['label']).strip()
                if not (pred.lower() in ('none', '') and label.lower() in ('none', '')):
                    buf += [f"{a}:\n", f"   predict: {pred}\n", f"   label:   {label}\n"]
            if buf:
                f.write("{\n")
                f.write(f"Sentence {i}: {sample['text']}\n")
                f.writelines(buf)
                f.write("}\n")
