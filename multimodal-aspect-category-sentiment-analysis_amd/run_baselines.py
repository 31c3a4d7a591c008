#!/usr/bin/env python3
"""Training / evaluation driver of the paper's three comparison baselines on MI355X:
    run_baselines.py --model {mroberta,tomroberta,ef_captr} <the published command line of that baseline>

It accepts the union of the flags of the reference's three scripts (mROBERTa/train_mroberta_vimacsa_full.py:294-316,
tomROBERTa/train_tomroberta_vimacsa_full.py:263-285, EF-CapTrRoBERTa/train_ef_captr_roberta.py:140-158), so each published
command line parses once --model is added, and keeps their step: AdamW with two weight-decay groups (0.01 / none for biases
and LayerNorm), linear warm-up schedule, clip 1.0, dev macro-F1 after every epoch, the best checkpoint under the script's file
name (`mroberta_best.pth`, `tombert_best.pth`, `seed_{seed}_ef_captr_model_best.pth`; `_last` beside it), then the test-set
pass into `test_results_{mroberta,tombert,ef_captr}.txt` and `test_predictions_formatted.txt`.
What changes is how a step runs: the aspect prompts of a batch go through ONE `forward_aspects` call (the visual tokens are
projected once per review and the cross-attention reads them with kv_share = aspects), clip + AdamW are FusedAdamW, the
gradients live in one arena; process set-up, checkpoint dictionary and the loop of an epoch are train_harness.py's.
Extra flags, as in run_multimodal_fcmf.py: --bf16 (--fp16 maps to it), --synthetic_steps N (seeded synthetic batches, no
dataset / tokenizer needed), --precomputed_features (the dataset yields ResNet-152 features: a FeatureCache under
--data_dir/features), --resnet_checkpoint.  Single process: the reference's baseline scripts have no distributed mode."""
import argparse
import json
import logging
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from fcmf_framework import baselines, ops  # noqa: E402
from fcmf_framework.dp import GradArena  # noqa: E402
from fcmf_framework.optimization import FusedAdamW, get_linear_schedule_with_warmup  # noqa: E402
from device_prefetch import DevicePrefetcher  # noqa: E402
from train_harness import (add_adv_arguments, add_ema_arguments, add_loss_arguments, averaged, build_extractors,  # noqa: E402
                           check_adv_arguments, check_ema_arguments, check_loss_arguments, class_weight_tensor, init_run, log_adv,
                           log_rdrop, make_adversary, make_features, save_model, setup_ema, split_decay, train_epoch, train_label_table,
                           twice)
from run_multimodal_fcmf import POLARITY_MAP, macro_f1  # noqa: E402

#            model class, checkpoint name before _best / _last (seed filled in), name in the log and result files
MODELS = {"mroberta": ("mRoBERTa", "mroberta", "mroberta"),
          "tomroberta": ("TomBERT", "tombert", "tombert"),
          "ef_captr": ("EFCapTrRoBERTa", "seed_{seed}_ef_captr_model", "ef_captr")}
TARGET_LEN, SENTENCE_LEN = 16, 170


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--model", required=True, choices=sorted(MODELS))
    # ---- the three reference parsers (a flag they share appears once; defaults are the scripts') ----
    p.add_argument("--data_dir", default='../vimacsa', type=str)
    p.add_argument("--output_dir", default=None, type=str, required=True)
    p.add_argument('--image_dir', default='../vimacsa/image', help='path to images')
    p.add_argument("--pretrained_hf_model", default="xlm-roberta-base", type=str)
    p.add_argument("--list_aspect", default=['Location', 'Food', 'Room', 'Facilities', 'Service', 'Public_area'], nargs='+')
    p.add_argument("--num_polarity", default=4, type=int)
    p.add_argument("--num_imgs", "--num_img", dest="num_imgs", default=3, type=int)       # (EF-CapTr spells it --num_img)
    p.add_argument("--num_rois", default=7, type=int)
    p.add_argument("--caption_file", default='visual_captions_vi.json', type=str)
    p.add_argument("--max_len", default=256, type=int)
    p.add_argument("--do_train", action='store_true')
    p.add_argument("--do_eval", action='store_true')
    p.add_argument("--train_batch_size", default=8, type=int)
    p.add_argument("--eval_batch_size", default=8, type=int)
    p.add_argument("--learning_rate", default=2e-5, type=float)
    p.add_argument("--num_train_epochs", default=10.0, type=float)
    p.add_argument("--warmup_proportion", default=0.1, type=float)
    p.add_argument('--gradient_accumulation_steps', type=int, default=1)
    p.add_argument('--seed', type=int, default=42)
    p.add_argument('--fp16', action='store_true')
    p.add_argument('--fine_tune_cnn', action='store_true')
    p.add_argument("--no_cuda", action='store_true')
    p.add_argument("--resume_from_checkpoint", default=None, type=str)
    # ---- MI355X additions ----
    p.add_argument('--bf16', action='store_true', help="bf16 activations on the MFMA kernels")
    p.add_argument('--synthetic_steps', type=int, default=0, help="train on N seeded synthetic batches per epoch; no dataset needed")
    p.add_argument('--precomputed_features', action='store_true', help="the dataset yields ResNet-152 features instead of pixels")
    p.add_argument('--resnet_checkpoint', default=None, type=str, help="torchvision resnet152 state dict for the HIP trunk")
    p.add_argument('--ffn_dropout', action='store_true',
                   help="nn.TransformerEncoderLayer's dropout between the feed-forward's gelu and its second Linear (ops.set_ffn_dropout)")
    add_loss_arguments(p)
    add_ema_arguments(p)
    add_adv_arguments(p)
    p.set_defaults(ddp=False)
    return p


def param_groups(model):
    """two groups (reference mRoBERTa :362-364): weight decay 0.01, and none for biases / LayerNorm"""
    decay, exempt = split_decay([(n, p) for n, p in model.named_parameters() if p.requires_grad])
    return [{'params': decay, 'weight_decay': 0.01}, {'params': exempt, 'weight_decay': 0.0}]


class SyntheticBatches:
    """seeded stand-in for DataLoader(BaselineDataset): the tuple layouts of baselines_dataset.py with precomputed features"""

    def __init__(self, model, cfg, steps, batch, num_imgs, num_rois, num_aspects, max_len, seed):
        self.model, self.cfg, self.steps, self.batch = model, cfg, steps, batch
        self.ni, self.nr, self.na, self.max_len, self.seed = num_imgs, num_rois, num_aspects, max_len, seed

    def __len__(self):
        return self.steps

    def __iter__(self):
        import synthetic_data as synth
        room = self.cfg["max_position_embeddings"] - 2
        for i in range(self.steps):
            mk = lambda S, s: synth.synth_batch(self.batch, self.cfg, S=min(S, room), num_imgs=self.ni, num_roi=self.nr,
                                                num_aspects=self.na, seed=self.seed + i + s)
            texts = [f"synthetic review {self.seed + i}:{j}" for j in range(self.batch)]
            if self.model == "ef_captr":
                b = mk(self.max_len, 0)
                yield b["input_ids"], b["attention_mask"], b["labels"], texts
                continue
            b = mk(SENTENCE_LEN, 0)
            head = (b["visual_embeds_att"], b["roi_embeds_att"])
            if self.model == "mroberta":
                yield head + (b["input_ids"], b["attention_mask"], b["labels"], texts)
            else:
                t = mk(TARGET_LEN, 500000)
                yield head + (t["input_ids"], t["attention_mask"], b["input_ids"], b["attention_mask"], b["labels"], texts)


def forward_batch(name, model, batch, features, copies=1):
    """one batch of baselines_dataset.py's layout -> (logits [B, aspects, polarities], labels, texts).  copies=2 (an R-Drop
    training step): the model sees every review twice, logits [2B, ...], labels stay [B, ...]; the doubling comes AFTER the
    feature extractor, so under --fine_tune_cnn the trunks still see each crop once"""
    rep = twice if copies == 2 else (lambda *t: t)
    if name == "ef_captr":
        ids, mask, labels, texts = batch
        return model.forward_aspects(*rep(ids, mask)), labels, texts
    vis, roi = features(batch[0], batch[1])
    *text_side, labels, texts = batch[2:]
    return model.forward_aspects(*rep(*text_side, vis, roi)), labels, texts


@torch.no_grad()
def predict(name, model, loader, device, features):
    model.eval()
    for batch in DevicePrefetcher(loader, device, float32_fields=() if name == "ef_captr" else (1,)):
        logits, labels, texts = forward_batch(name, model, batch, features)
        yield logits.argmax(-1).cpu().numpy(), labels.cpu().numpy(), texts


def evaluate(name, model, loader, device, features, aspects, logger, output_dir=None, tag=None):
    """macro-F1 averaged over the aspects (dev set: reference mRoBERTa :420-444).  With output_dir: the test-set pass (:452-520),
    per-aspect precision / recall / F1 into `test_results_{tag}.txt` and every review's predicted and gold polarities into
    `test_predictions_formatted.txt`"""
    true, pred, formatted = [[] for _ in aspects], [[] for _ in aspects], []
    for p, y, texts in predict(name, model, loader, device, features):
        for a in range(len(aspects)):
            true[a] += y[:, a].tolist()
            pred[a] += p[:, a].tolist()
        for j, t in enumerate(texts):
            formatted.append((t, [(POLARITY_MAP.get(int(p[j, a]), "Unknown"), POLARITY_MAP.get(int(y[j, a]), "Unknown"))
                                  for a in range(len(aspects))]))
    prf = [macro_f1(true[a], pred[a]) for a in range(len(aspects))]
    avg = float(np.mean([f for _, _, f in prf]))
    logger.info("%s macro-F1 per aspect: %s  mean %.4f", "Test" if output_dir else "Dev", ["%.4f" % f for _, _, f in prf], avg)
    if output_dir:
        with open(os.path.join(output_dir, f"test_results_{tag}.txt"), "w") as w:
            w.write("***** Test results *****\n")
            for a, (pr, rc, f1) in zip(aspects, prf):
                w.write(f"{a} - P: {pr:.4f}, R: {rc:.4f}, F1: {f1:.4f}\n")
            w.write(f"Average F1: {avg:.4f}\n")
        with open(os.path.join(output_dir, "test_predictions_formatted.txt"), "w", encoding="utf-8") as f:
            f.write(f"TEST DETAILED PREDICTIONS\nAverage Macro F1: {avg:.4f}\n" + "=" * 50 + "\n\n")
            for i, (text, rows) in enumerate(formatted):
                f.write("{\n" + f"Sentence {i}: {text}\n")
                for a, (pp, ll) in zip(aspects, rows):
                    f.write(f"{a}:\n   predict: {pp}\n   label:   {ll}\n")
                f.write("}\n")
    return avg


def real_loaders(args, model):
    """DataLoaders over baselines_dataset.BaselineDataset: tokenizer, frames, ROI table, captions / feature cache from --data_dir"""
    from transformers import AutoTokenizer
    import pandas as pd
    from torch.utils.data import DataLoader, RandomSampler, SequentialSampler
    from baselines_dataset import BaselineDataset
    tokenizer = AutoTokenizer.from_pretrained(args.pretrained_hf_model)
    model.roberta.resize_token_embeddings(len(tokenizer))
    roi_df = captions = None
    if args.model == "ef_captr":
        cap = args.caption_file if os.path.isabs(args.caption_file) else os.path.join(args.data_dir, args.caption_file)
        captions = json.load(open(cap, encoding="utf-8")) if os.path.exists(cap) else {}
    else:
        roi_df = pd.read_csv(f"{args.data_dir}/roi_data.csv")
        roi_df['file_name'] = roi_df['file_name'] + '.png'

    def loader(split, batch, shuffle):
        path = f'{args.data_dir}/{split}.json'
        if not os.path.exists(path):
            return None
        cache = None
        if args.precomputed_features and args.model != "ef_captr":
            from feature_cache import FeatureCache
            cache = FeatureCache(os.path.join(args.data_dir, "features", split))
        ds = BaselineDataset(pd.read_json(path), tokenizer, args.model, args.image_dir, roi_df, args.num_imgs, args.num_rois,
                             feature_cache=cache, caption_dict=captions, max_len=args.max_len)
        return DataLoader(ds, sampler=RandomSampler(ds) if shuffle else SequentialSampler(ds), batch_size=batch, pin_memory=True)
    return (loader("train", args.train_batch_size, True), loader("dev", args.eval_batch_size, False),
            loader("test", args.eval_batch_size, False) if args.do_eval else None)


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.gradient_accumulation_steps < 1:
        raise ValueError("Invalid gradient_accumulation_steps parameter: {}, should be >= 1".format(args.gradient_accumulation_steps))
    weight_request = check_loss_arguments(args)
    check_ema_arguments(args)
    check_adv_arguments(args)
    cls_name, ckpt, tag = MODELS[args.model]
    ckpt = ckpt.format(seed=args.seed)
    fmt = logging.Formatter('%(asctime)s - %(levelname)s - %(name)s - %(message)s', datefmt='%m/%d/%Y %H:%M:%S')
    _, _, _, device, _, logger = init_run(args, "baselines", f"training_{tag}.log", formatter=fmt, script="run_baselines.py")
    args.train_batch_size = int(args.train_batch_size / args.gradient_accumulation_steps)
    logger.info("model: %s device: %s bf16: %s", cls_name, device, args.bf16 or args.fp16)
    ops.set_ffn_dropout(args.ffn_dropout)        # (before the model is built; the encoder layers read it at every forward)
    logger.info("feed-forward dropout of the torch encoder layers: %s", "on" if args.ffn_dropout else "off")

    aspects = args.list_aspect
    model = getattr(baselines, cls_name)(args.pretrained_hf_model, num_labels=args.num_polarity)
    for p in model.roberta.pooler.parameters():
        p.requires_grad = False                  # never used by these models: the reference's optimizer skips it (no gradient)
    cfg = model.roberta.config
    train_loader = dev_loader = test_loader = None
    resnet_img = resnet_roi = None
    if args.synthetic_steps > 0:
        cfgd = dict(vocab_size=cfg.vocab_size, pad_token_id=cfg.pad_token_id, max_position_embeddings=cfg.max_position_embeddings)
        synthetic = lambda steps, batch, seed: SyntheticBatches(args.model, cfgd, steps, batch, args.num_imgs, args.num_rois,
                                                                len(aspects), args.max_len, seed)
        train_loader = synthetic(args.synthetic_steps, args.train_batch_size, args.seed)
        if args.do_eval:
            dev_loader = synthetic(max(1, args.synthetic_steps // 2), args.eval_batch_size, args.seed + 77)
            test_loader = synthetic(max(1, args.synthetic_steps // 2), args.eval_batch_size, args.seed + 99)
    elif args.do_train or args.do_eval:
        train_loader, dev_loader, test_loader = real_loaders(args, model)
        if args.model != "ef_captr" and not args.precomputed_features:
            from fcmf_framework.resnet import resnet152
            weights = torch.load(args.resnet_checkpoint, map_location='cpu', weights_only=True) if args.resnet_checkpoint else None
            if weights is None:
                logger.info("ResNet-152: no --resnet_checkpoint given: random init")
            resnet_img, resnet_roi = build_extractors(lambda: resnet152(weights=weights) if weights is not None else resnet152(),
                                                      args.fine_tune_cnn, device)
    model = model.to(device)
    optimizer = FusedAdamW(param_groups(model), lr=args.learning_rate)
    ema = setup_ema(optimizer, args, logger, True)          # before a checkpoint's optimizer state is loaded: its 'ema' is kept
    steps_per_epoch = len(train_loader) if train_loader is not None else 0
    num_train_steps = int(steps_per_epoch / args.gradient_accumulation_steps * args.num_train_epochs)
    scheduler = get_linear_schedule_with_warmup(optimizer, int(num_train_steps * args.warmup_proportion), num_train_steps)
    arena = GradArena.for_model(model, skip=lambda name: "roberta.pooler" in name)
    start_epoch, max_f1 = 0, 0.0
    if args.resume_from_checkpoint and os.path.isfile(args.resume_from_checkpoint):
        ck = torch.load(args.resume_from_checkpoint, map_location=device, weights_only=True)
        model.load_state_dict(ck['model_state_dict'])
        optimizer.load_state_dict(ck['optimizer_state_dict'])
        scheduler.load_state_dict(ck['scheduler_state_dict'])
        start_epoch, max_f1 = ck['epoch'] + 1, ck.get('best_score', 0.0)
        ops.shadows.clear()
    features = make_features(resnet_img, resnet_roi)
    f32_fields = () if args.model == "ef_captr" else (1,)
    last_loss = [float("nan")]

    class_weight = class_weight_tensor(weight_request, lambda: train_label_table(train_loader, first_wins=args.model != "ef_captr"),
                                       len(aspects), args.num_polarity, device, args.output_dir, logger, True) if args.do_train else None
    if args.do_train:
        logger.info("training loss: label_smoothing %g focal_gamma %g class_weights %s", args.label_smoothing, args.focal_gamma,
                    args.class_weights)
        log_rdrop(args, logger)
        log_adv(args, logger)

    def loss_fn(batch):
        rdrop = args.rdrop_alpha if model.training else 0.0
        logits, labels, _ = forward_batch(args.model, model, batch, features, copies=2 if rdrop > 0 else 1)
        return model.loss_aspects(logits, labels, weight=class_weight, label_smoothing=args.label_smoothing,
                                  focal_gamma=args.focal_gamma, rdrop_alpha=rdrop)

    def log(step, loss):
        last_loss[0] = loss
        logger.info("step %d loss %.4f", step, loss)

    if args.do_train:
        for epoch in range(start_epoch, int(args.num_train_epochs)):
            model.train()
            if resnet_img is not None:
                resnet_img.train(); resnet_roi.train()
            train_epoch(DevicePrefetcher(train_loader, device, float32_fields=f32_fields), loss_fn, arena=arena, reducer=None,
                        optimizer=optimizer, scheduler=scheduler, accum=args.gradient_accumulation_steps, log=log,
                        adversary=make_adversary(args))
            logger.info("--> Epoch %d Completed. LR %.2e last logged loss %.4f", epoch, optimizer.param_groups[0]['lr'], last_loss[0])
            f1 = 0.0
            if dev_loader is not None:
                if resnet_img is not None:
                    resnet_img.eval(); resnet_roi.eval()
                with averaged(optimizer, ema):
                    f1 = evaluate(args.model, model, dev_loader, device, features, aspects, logger)
            tags = ['last'] + (['best'] if f1 > max_f1 or not os.path.exists(f'{args.output_dir}/{ckpt}_best.pth') else [])
            max_f1 = max(max_f1, f1)
            for t in tags:      # with --ema_decay `best` holds the averaged weights that earned the score, `last` the raw ones + the average
                with averaged(optimizer, ema and t == 'best'):
                    save_model(f'{args.output_dir}/{ckpt}_{t}.pth', model, optimizer, scheduler, epoch, max_f1)
    if args.do_eval and test_loader is not None:
        logger.info("===================== STARTING TEST EVALUATION =====================")
        best_path = f'{args.output_dir}/{ckpt}_best.pth'
        if os.path.exists(best_path):
            logger.info("Loading Best Checkpoint from: %s", best_path)
            model.load_state_dict(torch.load(best_path, map_location=device, weights_only=True)['model_state_dict'])
            ops.shadows.clear()
        else:
            logger.warning("No best model found! Using current weights.")
        with averaged(optimizer, ema and not os.path.exists(best_path)):      # (a best checkpoint already holds the averaged weights)
            evaluate(args.model, model, test_loader, device, features, aspects, logger, output_dir=args.output_dir, tag=tag)
    arena.deactivate()
    return last_loss[0]


if __name__ == "__main__":
    main()
