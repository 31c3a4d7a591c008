#!/usr/bin/env python3
"""MACSA fine-tuning driver on MI355X -- drop-in for the reference's run_multimodal_fcmf.py.

Same command-line flags (reference run_multimodal_fcmf.py:65-118), same step order (:427-489), same
checkpoint dictionary and file names (:40-58,557-563), same torchrun environment contract
(RANK / LOCAL_RANK / WORLD_SIZE).  What changes is how a step is executed:
  * the 6 aspect forwards of a batch run as ONE `FCMF.forward_aspects` call on the HIP kernels;
  * clip_grad_norm_(1.0) + AdamW are the two fused multi-tensor kernels of `FusedAdamW`;
  * under --ddp the gradient mean is a bucketed RCCL all-reduce overlapped with backward
    (fcmf_framework.dp.GradReducer); the data is sharded ONCE (the reference shards it twice,
    :208-210 and :421);
  * --bf16 selects the MFMA path (bf16 activations, fp32 master weights, no loss scaler);
    --fp16 is accepted for compatibility and maps to --bf16.
The ResNet-152 extractors are checkpointed next to the model under the reference's names
(`seed_{seed}_resimg_model_{best,last}.pth`, `..._resroi_model_...`, :557-563) and restored on resume / for the test
evaluation through the reference's path rewrites (:334-346, :588-598); after training, --do_eval runs the TEST-set
evaluation of :567-694 and writes `test_results_fcmf.txt` + `test_predictions_formatted.txt` in the reference's format.
Batches reach the GPU through `device_prefetch.DevicePrefetcher` (pinned host memory, copy stream, one batch ahead).
Process set-up, the checkpoint code, the extractors and the loop of one epoch are `train_harness.py`'s, shared with
run_pretraining_fcmf.py; this file keeps the parser, the model and data, the 4 parameter groups, the loss and the evaluation.
Extra flags (not in the reference): --bf16, --synthetic_steps N (seeded synthetic batches with
precomputed features: no dataset / tokenizer / torchvision needed), --precomputed_features, --dump_attention_maps (the
test-set pass also writes `test_attention_maps.npz`: where each review's [CLS] looks in its photos, per aspect).
The host-side batch producer (vimacsa_dataset.MACSADataset, image decoding, ResNet-152 feature
extraction) is the "next" row of SURVEY.md section 8(f); with real data this driver imports the
user's `vimacsa_dataset` module and torchvision exactly as the reference does.
"""
import argparse
import logging
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from fcmf_framework import ops  # noqa: E402
from fcmf_framework.dp import GradArena, GradReducer  # noqa: E402
from fcmf_framework.fcmf_multimodal import FCMF  # noqa: E402
from fcmf_framework.optimization import FusedAdamW, get_linear_schedule_with_warmup  # noqa: E402
from device_prefetch import DevicePrefetcher  # noqa: E402
from train_harness import (add_adv_arguments, add_ema_arguments, add_loss_arguments, averaged, build_extractors,  # noqa: E402
                           check_adv_arguments, check_ema_arguments, check_loss_arguments, class_weight_tensor, init_run, load_resnets,
                           log_adv, log_rdrop, make_adversary, make_features, save_extractors, save_model, setup_ema, split_decay,
                           train_epoch, train_label_table, twice)


POLARITY_MAP = {0: 'None', 1: 'Negative', 2: 'Neutral', 3: 'Positive'}      # reference :28


def macro_f1(y_true, y_pred):
    from sklearn.metrics import precision_recall_fscore_support
    p, r, f, _ = precision_recall_fscore_support(y_true, y_pred, average='macro', zero_division=0)
    return p, r, f


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument("--data_dir", default='../vimacsa', type=str)
    parser.add_argument("--output_dir", default=None, type=str, required=True)
    parser.add_argument('--image_dir', default='../vimacsa/image')
    parser.add_argument('--resnet_label_path', default='/kaggle/input/resnet-output')
    parser.add_argument("--pretrained_hf_model", default=None, type=str, required=True)
    parser.add_argument("--pretrained_iaog_path", default=None, type=str)
    parser.add_argument("--resume_from_checkpoint", default=None, type=str)
    parser.add_argument("--model_checkpoint", default='checkpoint_path', type=str)
    parser.add_argument("--list_aspect", default=['Location', 'Food', 'Room', 'Facilities', 'Service', 'Public_area'], nargs='+')
    parser.add_argument("--num_polarity", default=4, type=int)
    parser.add_argument("--num_imgs", default=7, type=int)
    parser.add_argument("--num_rois", default=7, type=int)
    parser.add_argument("--max_seq_length", default=170, type=int)
    parser.add_argument("--do_train", action='store_true')
    parser.add_argument("--do_eval", action='store_true')
    parser.add_argument("--freeze_encoder", action='store_true')
    parser.add_argument("--train_batch_size", default=4, type=int)
    parser.add_argument("--eval_batch_size", default=4, type=int)
    parser.add_argument("--encoder_learning_rate", default=7e-5, type=float)
    parser.add_argument("--classifier_head_learning_rate", default=7e-4, type=float)
    parser.add_argument("--num_train_epochs", default=8.0, type=float)
    parser.add_argument("--warmup_proportion", default=0.1, type=float)
    parser.add_argument('--gradient_accumulation_steps', type=int, default=2)
    parser.add_argument('--seed', type=int, default=42)
    parser.add_argument('--fp16', action='store_true')
    parser.add_argument('--alpha', type=float, default=1)
    parser.add_argument('--fine_tune_cnn', action='store_true')
    parser.add_argument("--no_cuda", action='store_true')
    parser.add_argument("--ddp", action='store_true')
    parser.add_argument("--local_rank", type=int, default=-1)
    # ---- MI355X additions ----
    parser.add_argument('--bf16', action='store_true', help="bf16 activations on the MFMA kernels")
    parser.add_argument('--synthetic_steps', type=int, default=0,
                        help="train on N seeded synthetic batches per epoch (precomputed features); no dataset needed")
    parser.add_argument('--precomputed_features', action='store_true',
                        help="the dataset yields ResNet-152 features instead of pixels (BASELINE.json configs)")
    parser.add_argument('--synthetic_pixels', type=int, default=0,
                        help="with --synthetic_steps: batches carry SIZE x SIZE pixel crops and the ResNet-152 trunk runs inside "
                             "the step (reference :449-460); 0 = precomputed features")
    parser.add_argument('--resnet_checkpoint', default=None, type=str,
                        help="torchvision resnet152 state dict (.pth, loaded with weights_only=True) for the HIP trunk")
    parser.add_argument('--dump_attention_maps', action='store_true',
                        help="with --do_eval: the test-set pass also writes test_attention_maps.npz (head-averaged [CLS] "
                             "attention over each photo's patches and ROIs, per review and aspect) into --output_dir")
    add_loss_arguments(parser)
    add_ema_arguments(parser)
    add_adv_arguments(parser)
    return parser


def param_groups(model, args):
    """4 groups by substring match on the parameter names (reference :249-287): encoder / head x decay / no decay"""
    enc, head = [], []
    for n, p in model.named_parameters():
        if p.requires_grad:
            (head if any(h in n for h in ('classifier', 'text_pooler')) else enc).append((n, p))
    groups = []
    for named, lr in ((enc, args.encoder_learning_rate), (head, args.classifier_head_learning_rate)):
        decay, exempt = split_decay(named)
        groups += [{'params': decay, 'weight_decay': 0.01, 'lr': lr}, {'params': exempt, 'weight_decay': 0.0, 'lr': lr}]
    return groups


class SyntheticBatches:
    """seeded stand-in for DataLoader(MACSADataset): the reference's 9-tuple layout
    (vimacsa_dataset.py:202) with precomputed features in place of pixel tensors"""

    def __init__(self, cfg, steps, batch, S, num_imgs, num_rois, num_aspects, seed, pixels=0):
        self.cfg, self.steps, self.batch, self.S = cfg, steps, batch, S
        self.ni, self.nr, self.na, self.seed = num_imgs, num_rois, num_aspects, seed
        self.pixels = pixels

    def __len__(self):
        return self.steps

    def __iter__(self):
        import synthetic_data as synth
        for i in range(self.steps):
            b = synth.synth_batch(self.batch, self.cfg, S=self.S, num_imgs=self.ni, num_roi=self.nr,
                                  num_aspects=self.na, seed=self.seed + i)
            vis, roi = b["visual_embeds_att"], b["roi_embeds_att"]
            if self.pixels:          # the reference's pixel layout: float32 images, float64 ROI crops (vimacsa_dataset.py:175-199)
                vis, roi = synth.synth_pixel_batch(self.batch, self.ni, self.nr, self.pixels, self.seed + i, torch.float64)
            texts = [f"synthetic review {self.seed + i}:{j}" for j in range(self.batch)]
            yield (vis, roi, b["roi_coors"], b["input_ids"], b["token_type_ids"],
                   b["attention_mask"], b["added_attention_mask"], b["labels"], texts)


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.gradient_accumulation_steps < 1:
        raise ValueError("Invalid gradient_accumulation_steps parameter: {}, should be >= 1".format(args.gradient_accumulation_steps))
    weight_request = check_loss_arguments(args)
    check_ema_arguments(args)
    check_adv_arguments(args)
    fmt = logging.Formatter('%(asctime)s - %(levelname)s - %(name)s - %(message)s', datefmt='%m/%d/%Y %H:%M:%S')
    rank, _, world, device, master, logger = init_run(args, "fcmf", "training_fcmf.log", formatter=fmt, script="run_multimodal_fcmf.py")
    args.train_batch_size = int(args.train_batch_size / args.gradient_accumulation_steps)
    if master:
        logger.info("device: %s n_gpu: %d, distributed training: %s, bf16: %s", device, world, bool(args.ddp), args.bf16 or args.fp16)

    ASPECT = args.list_aspect
    model = FCMF(pretrained_path=args.pretrained_hf_model, num_labels=args.num_polarity, num_imgs=args.num_imgs,
                 num_roi=args.num_rois, alpha=args.alpha)
    cfg = model.encoder.bert.cell.config
    train_loader = dev_loader = test_loader = None
    resnet_img = resnet_roi = None
    if args.synthetic_steps > 0:
        cfgd = dict(vocab_size=cfg.vocab_size, pad_token_id=cfg.pad_token_id)
        S = min(args.max_seq_length, 128, cfg.max_position_embeddings - 2)
        synthetic = lambda steps, batch, seed: SyntheticBatches(cfgd, steps, batch, S, args.num_imgs, args.num_rois, len(ASPECT),
                                                                seed, pixels=args.synthetic_pixels)
        train_loader = synthetic(args.synthetic_steps, args.train_batch_size, args.seed + 1000 * rank)
        if args.do_eval:
            dev_loader = synthetic(max(1, args.synthetic_steps // 2), args.eval_batch_size, args.seed + 77)
            test_loader = synthetic(max(1, args.synthetic_steps // 2), args.eval_batch_size, args.seed + 99)
    elif args.do_train or args.do_eval:
        # real data: the reference's host-side producer (tokenizer, pandas, MACSADataset, torchvision ResNet-152)
        from transformers import AutoTokenizer
        import pandas as pd
        from torch.utils.data import DataLoader, DistributedSampler, RandomSampler, SequentialSampler
        from vimacsa_dataset import MACSADataset   # user-provided, same tuple layout as the reference
        tokenizer = AutoTokenizer.from_pretrained(args.pretrained_hf_model)
        model.encoder.bert.cell.resize_token_embeddings(len(tokenizer))
        roi_df = pd.read_csv(f"{args.data_dir}/roi_data.csv")
        roi_df['file_name'] = roi_df['file_name'] + '.png'
        import json
        with open(f'{args.data_dir}/resnet152_image_label.json') as f:
            dict_image_aspect = json.load(f)
        with open(f'{args.data_dir}/resnet152_roi_label.json') as f:
            dict_roi_aspect = json.load(f)
        mk = lambda df: MACSADataset(df, tokenizer, args.image_dir, roi_df, dict_image_aspect, dict_roi_aspect, args.num_imgs, args.num_rois)
        train_ds, dev_ds = mk(pd.read_json(f'{args.data_dir}/train.json')), mk(pd.read_json(f'{args.data_dir}/dev.json'))
        sampler = DistributedSampler(train_ds) if world > 1 else RandomSampler(train_ds)     # shard ONCE
        train_loader = DataLoader(train_ds, sampler=sampler, batch_size=args.train_batch_size, pin_memory=True)
        dev_loader = DataLoader(dev_ds, sampler=SequentialSampler(dev_ds), batch_size=args.eval_batch_size, pin_memory=True)
        if args.do_eval and os.path.exists(f'{args.data_dir}/test.json'):                     # reference :570-573
            test_ds = mk(pd.read_json(f'{args.data_dir}/test.json'))
            test_loader = DataLoader(test_ds, sampler=SequentialSampler(test_ds), batch_size=args.eval_batch_size, pin_memory=True)
    pixels = (args.synthetic_steps > 0 and args.synthetic_pixels > 0) or \
             (args.synthetic_steps <= 0 and (args.do_train or args.do_eval) and not args.precomputed_features)
    if pixels:
        # the ResNet-152 feature extractor of the step (reference :224-227) on the HIP trunk.  Weights: a local
        # torchvision checkpoint (--resnet_checkpoint), else torchvision's IMAGENET1K_V2 if torchvision is importable
        # and has them cached, else random initialisation (logged): nothing is ever downloaded.
        from fcmf_framework.resnet import resnet152

        def trunk():
            if args.resnet_checkpoint:
                return resnet152(weights=torch.load(args.resnet_checkpoint, map_location='cpu', weights_only=True))
            try:
                from torchvision.models import resnet152 as tv_resnet152, ResNet152_Weights
                return tv_resnet152(weights=ResNet152_Weights.IMAGENET1K_V2)       # adopted by the HIP trunk (from_module)
            except Exception as e:                                              # not installed / weights not cached
                if master:
                    logger.info("ResNet-152: no checkpoint given and torchvision weights unavailable (%s): random init", type(e).__name__)
                return resnet152()
        resnet_img, resnet_roi = build_extractors(trunk, args.fine_tune_cnn, device)

    model = model.to(device)
    if args.freeze_encoder:
        for p in model.encoder.parameters():
            p.requires_grad = False
    optimizer = FusedAdamW(param_groups(model, args), lr=args.classifier_head_learning_rate)
    ema = setup_ema(optimizer, args, logger, master)        # before a checkpoint's optimizer state is loaded: its 'ema' is kept
    steps_per_epoch = len(train_loader) if train_loader is not None else 0
    num_train_steps = int(steps_per_epoch / args.gradient_accumulation_steps * args.num_train_epochs)
    scheduler = get_linear_schedule_with_warmup(optimizer, int(num_train_steps * args.warmup_proportion), num_train_steps)
    # gradients live in one flat arena (one memset per step; buckets of it are all-reduced in place under --ddp)
    arena = GradArena.for_model(model)
    reducer = None
    if world > 1:
        reducer = GradReducer(arena)
        reducer.broadcast_parameters(0)

    start_epoch, max_f1 = 0, 0.0
    if args.resume_from_checkpoint and os.path.isfile(args.resume_from_checkpoint):
        ck = torch.load(args.resume_from_checkpoint, map_location=device, weights_only=True)
        model.load_state_dict(ck['model_state_dict'])
        optimizer.load_state_dict(ck['optimizer_state_dict'])
        if 'scheduler_state_dict' in ck:
            scheduler.load_state_dict(ck['scheduler_state_dict'])
        start_epoch, max_f1 = ck['epoch'] + 1, ck.get('best_score', 0.0)
        ops.shadows.clear()
        load_resnets(args.resume_from_checkpoint, resnet_img, resnet_roi, device, logger if master else None)   # reference :334-346
    elif args.pretrained_iaog_path and os.path.isfile(args.pretrained_iaog_path):
        sd = torch.load(args.pretrained_iaog_path, map_location='cpu', weights_only=True)['model_state_dict']
        model.load_state_dict({k: v for k, v in sd.items() if k.startswith('encoder.')}, strict=False)   # reference :385-391
        ops.shadows.clear()

    features = make_features(resnet_img, resnet_roi)
    # the training loss's options; the synthetic label table is rank 0's, so that every rank holds the same weights
    counted = synthetic(args.synthetic_steps, args.train_batch_size, args.seed) if args.synthetic_steps > 0 else train_loader
    class_weight = class_weight_tensor(weight_request, lambda: train_label_table(counted), len(ASPECT), args.num_polarity, device,
                                       args.output_dir, logger, master) if args.do_train else None
    if master and args.do_train:
        logger.info("training loss: label_smoothing %g focal_gamma %g class_weights %s", args.label_smoothing, args.focal_gamma,
                    args.class_weights)
        log_rdrop(args, logger)
        log_adv(args, logger)

    def loss_fn(batch):
        rdrop = args.rdrop_alpha if model.training else 0.0
        logits, labels, _ = forward_batch(model, batch, features, copies=2 if rdrop > 0 else 1)
        # sum over aspects of the batch-mean CE (each aspect over its own weight sum once an option is set)
        return model.loss_aspects(logits, labels, weight=class_weight, label_smoothing=args.label_smoothing,
                                  focal_gamma=args.focal_gamma, rdrop_alpha=rdrop)

    if args.do_train:
        for epoch in range(start_epoch, int(args.num_train_epochs)):
            if world > 1 and hasattr(train_loader, 'sampler') and hasattr(train_loader.sampler, 'set_epoch'):
                train_loader.sampler.set_epoch(epoch)
            model.train()
            if resnet_img is not None:
                resnet_img.train(); resnet_roi.train()                # reference :431 (BatchNorm in batch-statistics mode)
            log = lambda step, loss: logger.info("epoch %d step %d loss %.4f", epoch, step, loss)
            # next batch: pinned, on the copy stream (field 1 = the float64 ROI crops)
            train_epoch(DevicePrefetcher(train_loader, device, float32_fields=(1,)), loss_fn, arena=arena, reducer=reducer,
                        optimizer=optimizer, scheduler=scheduler, accum=args.gradient_accumulation_steps, log=log if master else None,
                        adversary=make_adversary(args))
            if master:
                logger.info("--> Epoch %d Completed. Encoder LR %.2e Head LR %.2e", epoch,
                            optimizer.param_groups[0]['lr'], optimizer.param_groups[2]['lr'])
            f1 = 0.0
            if dev_loader is not None and master:
                if resnet_img is not None:
                    resnet_img.eval(); resnet_roi.eval()              # reference :502
                with averaged(optimizer, ema):                        # the master alone swaps: no collective call inside
                    f1 = evaluate(model, dev_loader, device, features, len(ASPECT), logger)
            if world > 1:
                torch.distributed.barrier()
            if master:
                tags = ['last'] + (['best'] if f1 > max_f1 else [])
                max_f1 = max(max_f1, f1)
                for tag in tags:                                      # reference :555-563: the model and BOTH extractors
                    # with --ema_decay `best` holds the averaged weights that earned the score, `last` the raw ones + the average
                    with averaged(optimizer, ema and tag == 'best'):
                        save_model(f'{args.output_dir}/seed_{args.seed}_fcmf_model_{tag}.pth', model, optimizer, scheduler, epoch, max_f1)
                        save_extractors(args.output_dir, args.seed, tag, resnet_img, resnet_roi, optimizer, scheduler, epoch)
    # ---- 7. TEST EVALUATION (reference :567-694) ---------------------------------------------------------------------
    if args.do_eval and master and test_loader is not None:
        logger.info("===================== STARTING TEST EVALUATION =====================")
        best_path = args.model_checkpoint if os.path.exists(args.model_checkpoint) else \
            f'{args.output_dir}/seed_{args.seed}_fcmf_model_best.pth'
        if os.path.exists(best_path):
            logger.info("Loading Best Checkpoint from: %s", best_path)
            ck = torch.load(best_path, map_location=device, weights_only=True)
            model.load_state_dict(ck['model_state_dict'], strict=False)
            ops.shadows.clear()
            load_resnets(best_path, resnet_img, resnet_roi, device, logger, old="fcmf", strict=False)      # :588-598
            found = True
        else:
            logger.warning("No best model found! Using current weights.")
            found = False
        if resnet_img is not None:
            resnet_img.eval(); resnet_roi.eval()
        with averaged(optimizer, ema and not found):                  # (a best checkpoint already holds the averaged weights)
            test_evaluate(model, test_loader, device, features, ASPECT, args.output_dir, logger, dump_maps=args.dump_attention_maps)
    arena.deactivate()
    if world > 1:
        torch.distributed.destroy_process_group()


def forward_batch(model, batch, features, copies=1):
    """one batch of the reference's 9-tuple (vimacsa_dataset.py:202) -> (logits [B, aspects, polarities], labels, texts).
    copies=2 (an R-Drop training step): the model sees every review twice, logits [2B, ...], labels stay [B, ...]; the doubling
    comes AFTER the feature extractor, so under --fine_tune_cnn the trunks still see each crop once"""
    t_img, roi_img, roi_coors, ids, tts, ams, added, labels, texts = batch
    vis, roi = features(t_img, roi_img)
    if copies == 2:
        vis, roi, roi_coors, ids, tts, ams, added = twice(vis, roi, roi_coors, ids, tts, ams, added)
    logits = model.forward_aspects(input_ids=ids, token_type_ids=tts, attention_mask=ams, added_attention_mask=added,
                                   visual_embeds_att=vis, roi_embeds_att=roi, roi_coors=roi_coors)
    return logits, labels, texts


def cls_attention_maps(encoder, B, A):
    """the head-averaged [CLS] rows of the batch's fusion_attentions (eval-only torch arithmetic, as in decoding.py) ->
    patches [B, A, NI, P]: the text -> image-patch layer's row; rois [B, A, NI, NR]: the ROI columns of the text+ROI layer's
    row, renormalised over the photo's ROIs (every row of both sums to 1); roi_mass [B, A, NI]: the share of that row which
    lay on the ROIs and not on the text, i.e. what the renormalisation divided by"""
    fa = encoder.fusion_attentions
    patches = fa["text2img"].mean(2)                                      # [B*A, NI, P]
    roi = fa["text2roi"].mean(2)[..., -encoder.num_roi:]                  # [B*A, NI, NR]
    mass = roi.sum(-1, keepdim=True)
    rois = roi / mass.clamp_min(torch.finfo(torch.float32).tiny)
    return (patches.reshape(B, A, *patches.shape[1:]).cpu().numpy(), rois.reshape(B, A, *rois.shape[1:]).cpu().numpy(),
            mass.reshape(B, A, -1).cpu().numpy())


@torch.no_grad()
def predict(model, loader, device, features, maps=None):
    """eval-mode forward + argmax over a loader: (predictions [B, aspects], labels [B, aspects], texts) per batch, as numpy.
    maps (a list): every batch also appends its cls_attention_maps (ops.set_output_fusion_attentions is on for the pass)."""
    model.eval()
    was = ops.output_fusion_attentions()
    ops.set_output_fusion_attentions(was or maps is not None)
    try:
        for batch in DevicePrefetcher(loader, device, float32_fields=(1,)):
            logits, labels, texts = forward_batch(model, batch, features)
            if maps is not None:
                maps.append(cls_attention_maps(model.encoder, logits.shape[0], logits.shape[1]))
            yield logits.argmax(-1).cpu().numpy(), labels.cpu().numpy(), texts
    finally:
        ops.set_output_fusion_attentions(was)


def test_evaluate(model, loader, device, features, aspects, output_dir, logger, dump_maps=False):
    """test-set pass of the reference (:600-694): per-aspect precision / recall / macro-F1 into `test_results_fcmf.txt`, and
    one block per review with the predicted and gold polarity of every aspect into `test_predictions_formatted.txt`.
    dump_maps: also `test_attention_maps.npz` with patches [N, aspects, NI, 49], rois [N, aspects, NI, NR] and roi_mass
    [N, aspects, NI] (cls_attention_maps), review by review in the order of the loader."""
    true = {a: [] for a in aspects}
    pred = {a: [] for a in aspects}
    formatted = []
    maps = [] if dump_maps else None
    for p, y, texts in predict(model, loader, device, features, maps):
        logs = [{"text": t, "aspects": {}} for t in (texts if texts is not None else [""] * len(p))]
        for i, a in enumerate(aspects):
            true[a].append(y[:, i]); pred[a].append(p[:, i])
            for j, (pp, ll) in enumerate(zip(p[:, i], y[:, i])):
                logs[j]["aspects"][a] = {"predict": POLARITY_MAP.get(int(pp), "Unknown"), "label": POLARITY_MAP.get(int(ll), "Unknown")}
        formatted.extend(logs)
    with open(os.path.join(output_dir, "test_results_fcmf.txt"), "w") as w:
        w.write("***** Test results *****\n")
        all_f1 = 0.0
        for a in aspects:
            precision, recall, f1 = macro_f1(np.concatenate(true[a]), np.concatenate(pred[a]))
            all_f1 += f1
            w.write(f"{a} - P: {precision:.4f}, R: {recall:.4f}, F1: {f1:.4f}\n")
            logger.info("%s - F1: %.4f", a, f1)
        avg_f1 = all_f1 / len(aspects)
        w.write(f"Average F1: {avg_f1:.4f}\n")
        logger.info("Average F1: %.4f", avg_f1)
    log_path = f"{output_dir}/test_predictions_formatted.txt"
    with open(log_path, "w", encoding="utf-8") as f:
        f.write("TEST DETAILED PREDICTIONS\n")
        f.write(f"Average Macro F1: {avg_f1:.4f}\n")
        f.write("=" * 50 + "\n\n")
        for i, sample in enumerate(formatted):
            f.write("{\n")
            f.write(f"Sentence {i}: {sample['text']}\n")
            for a in aspects:
                res = sample['aspects'].get(a, {'predict': 'N/A', 'label': 'N/A'})
                f.write(f"{a}:\n")
                f.write(f"   predict: {res['predict']}\n")
                f.write(f"   label:   {res['label']}\n")
            f.write("}\n")
    logger.info("Formatted predictions saved to %s", log_path)
    if dump_maps:
        maps_path = os.path.join(output_dir, "test_attention_maps.npz")
        np.savez(maps_path, **{name: np.concatenate([m[i] for m in maps]) for i, name in enumerate(("patches", "rois", "roi_mass"))})
        logger.info("Attention maps saved to %s", maps_path)
    return avg_f1


def evaluate(model, loader, device, features, num_aspects, logger):
    """dev-set macro-F1 averaged over aspects (reference :500-552)"""
    true, pred = [[] for _ in range(num_aspects)], [[] for _ in range(num_aspects)]
    for p, y, _ in predict(model, loader, device, features):
        for a in range(num_aspects):
            true[a] += y[:, a].tolist()
            pred[a] += p[:, a].tolist()
    f1s = [macro_f1(true[a], pred[a])[2] for a in range(num_aspects)]
    logger.info("Dev macro-F1 per aspect: %s  mean %.4f", ["%.4f" % f for f in f1s], float(np.mean(f1s)))
    return float(np.mean(f1s))


if __name__ == "__main__":
    main()
