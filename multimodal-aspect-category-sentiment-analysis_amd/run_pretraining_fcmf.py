#!/usr/bin/env python3
"""IAOG seq2seq pre-training driver on MI355X -- drop-in for the reference's run_pretraining_fcmf.py.

Accepts every flag the reference declares (run_pretraining_fcmf.py:45-84; tests/test_surface.py feeds it the published
command line of Pretraining-Notebook.ipynb:6927-6945), same step (:284-337: FCMFSeq2Seq forward,
CE(ignore_index=-100) over [B,V,Ld], clip 1.0, AdamW (wd 1e-5 / 0, eps=--adam_epsilon), linear
schedule), same per-epoch checkpoint dict (:27-42,455-460).  Reference behaviours kept on purpose:
`model.decoder.embedding` is re-created after construction (:189), which un-ties it from the
encoder's word embeddings while `decoder.dense.weight` stays tied to them.
--fine_tune_cnn as in the reference (:203-207): the parameters of BOTH ResNet-152 extractors join the two AdamW groups
(and the gradient arena / the data-parallel exchange), so the trunks really train; the extractors are checkpointed as
`seed_{seed}_resimg_model_last.pth` / `..._resroi_model_last.pth` (:457-459) and restored on resume through the
reference's `iaog_model` -> `resimg_model` / `resroi_model` path rewrite (:244-255).
Extra flags: --bf16, --synthetic_steps N (seeded synthetic batches, precomputed features), --synthetic_pixels SIZE
(those batches carry pixel crops and the HIP ResNet-152 trunks run inside the step), --synthetic_eval_samples N.
--do_eval is the generation evaluation the reference keeps commented out (:376-452, :462-632), in `iaog_eval.py`: after every
epoch the master rank beam-search decodes the dev set (`dev_with_iaog.json`, or N seeded synthetic samples), scores the text against
the labels with BERTScore (`fcmf_framework/bertscore.py`: --bert_score_model must be a LOCAL model directory), keeps
`seed_{seed}_{iaog,resimg,resroi}_model_best.pth` by macro F1 and carries `best_score` in the `last` checkpoints; after training
the best checkpoint decodes the test set into `iaog_test_predictions_formatted.txt`.  Without --do_eval nothing of this runs.
--decode_strategy sample decodes --num_chains sampled chains per sample instead of a beam (--temperature, --top_k, --top_p,
--sample_seed; csrc/sample.hip) and keeps the best-scoring one; --length_penalty ranks the final choice of either strategy by
score / length ** penalty.  The defaults (beam, 0) are the reference's decode.
--repetition_penalty, --no_repeat_ngram_size, --min_length_decoder and --suppress_tokens constrain the logits of every decode step
of either strategy on the device (csrc/constrain.hip; they imply the batched step); their defaults (1, 0, 0, none) run no new code.
Process set-up, the checkpoint code, the extractors and the loop of one epoch are `train_harness.py`'s, shared with
run_multimodal_fcmf.py; this file keeps the parser, the model and data, the 2 parameter groups and the loss.
With real data the driver imports the user's `iaog_dataset.IAOGDataset` (host-side producer,
SURVEY.md section 8(f) "next") and torchvision, as the reference does.
"""
import argparse
import math
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from fcmf_framework import ops  # noqa: E402
from fcmf_framework.decoding import make_constraints  # noqa: E402
from fcmf_framework.dp import GradArena, GradReducer  # noqa: E402
from fcmf_framework.fcmf_pretraining import FCMFSeq2Seq  # noqa: E402
from fcmf_framework.optimization import FusedAdamW, get_linear_schedule_with_warmup  # noqa: E402
from device_prefetch import DevicePrefetcher  # noqa: E402
from train_harness import (add_adv_arguments, add_ema_arguments, add_loss_arguments, averaged, build_extractors,  # noqa: E402
                           check_adv_arguments, check_ema_arguments, check_loss_arguments, init_run, load_resnets, log_adv, log_rdrop,
                           make_adversary, make_features, save_extractors, save_model, setup_ema, split_decay, train_epoch)


DEFAULT_BERT_SCORE_MODEL = 'uitnlp/visobert'      # the reference's default (:53), a hub name


def build_parser():
    p = argparse.ArgumentParser()
    # (reference :47-48 marks both `required`; here they are only read by the real-data branch, so --synthetic_steps runs without)
    p.add_argument("--data_dir", default='../vimacsa', type=str)
    p.add_argument("--pretrained_data_dir", default='../iaog-pretraining', type=str)
    p.add_argument("--output_dir", default=None, type=str, required=True)
    p.add_argument('--image_dir', default='../vimacsa/image')
    p.add_argument("--pretrained_hf_model", default=None, type=str, required=True)
    p.add_argument("--resume_from_checkpoint", default=None, type=str)
    # declared exactly as the reference declares them (run_pretraining_fcmf.py:53,57,60,66,82).  --bert_score_model, --beam_size and
    # --eval_batch_size drive the --do_eval generation evaluation (the reference's commented-out half, :376-632, built here in
    # iaog_eval.py); --resnet_label_path is read nowhere, there or here
    p.add_argument('--bert_score_model', default=DEFAULT_BERT_SCORE_MODEL, type=str,
                   help="LOCAL model directory of the BERTScore encoder (--do_eval; a hub name cannot be fetched: download it first). "
                        "With --synthetic_steps the default is the --pretrained_hf_model directory")
    p.add_argument('--resnet_label_path', default='/kaggle/input/resnet-output')
    p.add_argument("--max_seq_length", default=170, type=int, help="encoder prompt length (the reference's dataset hard-codes 170)")
    p.add_argument("--beam_size", default=2, type=int)
    p.add_argument("--list_aspect", nargs='+', default=[],
                   help="aspect categories that produce IAOG samples (empty = the six ViMACSA categories, as the reference hard-codes)")
    p.add_argument("--num_imgs", default=7, type=int)
    p.add_argument("--num_rois", default=4, type=int)
    p.add_argument("--max_len_decoder", default=20, type=int)
    p.add_argument("--do_train", action='store_true')
    p.add_argument("--do_eval", action='store_true')
    p.add_argument("--train_batch_size", default=16, type=int)
    p.add_argument("--eval_batch_size", default=16, type=int)
    p.add_argument("--batched_decode", action='store_true',
                   help="--do_eval: decode a whole eval batch per decoder call (decoding.beam_search_batch) instead of sample by sample")
    p.add_argument("--decode_context", default="last", choices=("last", "prefix"),
                   help="--do_eval: what a decode step sees.  last: the beam's last token at position 0 (the reference's loop); prefix: "
                        "the whole prefix, as the decoder is trained (key cache + csrc/attn_decode.hip; implies the batched step)")
    p.add_argument("--decode_loop", default="host", choices=("host", "device"),
                   help="--do_eval: where the beam / chain bookkeeping runs.  host: the Python loops, one upload and one read per round; "
                        "device: the state stays on the device and csrc/beam.hip advances it (beams / chains <= 8; implies the batched step)")
    p.add_argument("--decode_poll_every", default=4, type=int,
                   help="--decode_loop device: read the done flags every N rounds to stop early (0 = never, run --max_len_decoder rounds)")
    p.add_argument("--decode_strategy", default="beam", choices=("beam", "sample"),
                   help="--do_eval: beam search (the reference's), or --num_chains sampled chains per sample, the best-scoring one kept "
                        "(csrc/sample.hip; implies the batched step)")
    p.add_argument("--temperature", default=1.0, type=float, help="--decode_strategy sample: logits are divided by it (> 0)")
    p.add_argument("--top_k", default=0, type=int, help="--decode_strategy sample: keep the k most probable tokens, ties included (0 = off)")
    p.add_argument("--top_p", default=1.0, type=float, help="--decode_strategy sample: keep the nucleus of this mass, in (0, 1] (1 = off)")
    p.add_argument("--num_chains", default=1, type=int, help="--decode_strategy sample: independent chains per sample")
    p.add_argument("--sample_seed", default=0, type=int, help="--decode_strategy sample: seed of the counter-based draws")
    p.add_argument("--length_penalty", default=0.0, type=float,
                   help="--do_eval: the final choice among the finished beams / the chains ranks by score / length ** this (0 = the raw score)")
    p.add_argument("--repetition_penalty", default=1.0, type=float,
                   help="--do_eval: logits of the tokens a sequence already holds are divided by it (multiplied when negative); > 0, 1 = off")
    p.add_argument("--no_repeat_ngram_size", default=0, type=int, help="--do_eval: no n-gram of this size occurs twice in a decoded sequence (0 = off)")
    p.add_argument("--min_length_decoder", default=0, type=int,
                   help="--do_eval: the separator cannot be decoded before this many tokens (0 = off; at most --max_len_decoder)")
    p.add_argument("--suppress_tokens", default=[], type=int, nargs="+", metavar="ID", help="--do_eval: token ids that are never decoded")
    p.add_argument("--learning_rate", default=3e-5, type=float)
    p.add_argument("--adam_epsilon", default=1e-8, type=float)
    p.add_argument("--num_train_epochs", default=8.0, type=float)
    p.add_argument("--warmup_proportion", default=0.1, type=float)
    p.add_argument('--gradient_accumulation_steps', type=int, default=1)
    p.add_argument('--seed', type=int, default=42)
    p.add_argument('--fp16', action='store_true')
    p.add_argument('--alpha', type=float, default=1)
    p.add_argument('--fine_tune_cnn', action='store_true')
    p.add_argument("--no_cuda", action='store_true')
    p.add_argument("--ddp", action='store_true')
    p.add_argument("--local_rank", type=int, default=-1)
    p.add_argument('--bf16', action='store_true')
    p.add_argument('--synthetic_steps', type=int, default=0)
    p.add_argument('--synthetic_dec_len', type=int, default=12)
    p.add_argument('--vocab_size', type=int, default=0, help="decoder vocabulary (len(tokenizer) with real data)")
    p.add_argument('--feature_cache_dir', default=None, type=str,
                   help="precomputed ResNet-152 features of the training reviews (feature_cache.build); else pixels + the HIP trunk")
    p.add_argument('--resnet_checkpoint', default=None, type=str, help="torchvision resnet152 state dict for the HIP trunk")
    p.add_argument('--synthetic_pixels', type=int, default=0,
                   help="with --synthetic_steps: batches carry SIZE x SIZE pixel crops and the ResNet-152 trunks run inside the step")
    p.add_argument('--synthetic_eval_samples', type=int, default=0,
                   help="with --synthetic_steps and --do_eval: dev and test sets of N seeded synthetic samples each")
    add_loss_arguments(p, class_weights=False)
    add_ema_arguments(p)
    add_adv_arguments(p)
    return p


def scorer_dir(args):
    """the BERTScore model directory of a --do_eval run, checked before anything is trained"""
    path = args.bert_score_model
    if args.synthetic_steps > 0 and path == DEFAULT_BERT_SCORE_MODEL:
        path = args.pretrained_hf_model
    if not os.path.isdir(path):
        raise ValueError(f"--bert_score_model {path!r}: --do_eval needs a local model directory (config.json + weights of a "
                         f"RoBERTa-family encoder, e.g. a downloaded uitnlp/visobert); nothing is fetched from a hub")
    return path


def main(argv=None):
    args = build_parser().parse_args(argv)
    bert_score_dir = scorer_dir(args) if args.do_eval else None
    if args.do_eval and args.batched_decode and not 1 <= args.beam_size <= ops.TOPK_MAX:      # before anything is trained
        raise ValueError(f"--batched_decode: --beam_size {args.beam_size} is outside the top-k kernel's 1 .. {ops.TOPK_MAX}; "
                         f"decode without --batched_decode")
    if args.do_eval and args.decode_context == "prefix":
        if not 1 <= args.beam_size <= ops.TOPK_MAX:
            raise ValueError(f"--decode_context prefix: --beam_size {args.beam_size} is outside the top-k kernel's 1 .. {ops.TOPK_MAX}")
        if not 1 <= args.max_len_decoder <= ops.DECODE_ATTN_MAX_T:
            raise ValueError(f"--decode_context prefix: --max_len_decoder {args.max_len_decoder} is outside the decode-attention "
                             f"kernel's 1 .. {ops.DECODE_ATTN_MAX_T} keys")
    if args.do_eval and args.decode_loop == "device":
        width = args.num_chains if args.decode_strategy == "sample" else args.beam_size
        try:
            ops.check_advance(width, args.max_len_decoder, "--num_chains" if args.decode_strategy == "sample" else "--beam_size")
        except ValueError as e:
            raise ValueError(f"--decode_loop device: {e}") from None
        if args.decode_poll_every < 0:
            raise ValueError(f"--decode_loop device: --decode_poll_every {args.decode_poll_every} must be >= 0")
    if args.do_eval and not math.isfinite(args.length_penalty):
        raise ValueError(f"--length_penalty {args.length_penalty} must be finite")
    if args.do_eval and args.decode_strategy == "sample":
        try:
            ops.check_sampler(args.temperature, args.top_k, args.top_p)
        except ValueError as e:
            raise ValueError(f"--decode_strategy sample: --temperature / --top_k / --top_p: {e}") from None
        if args.num_chains < 1:
            raise ValueError(f"--decode_strategy sample: --num_chains {args.num_chains} must be >= 1")
        if args.sample_seed < 0:
            raise ValueError(f"--decode_strategy sample: --sample_seed {args.sample_seed} must be >= 0")
        if args.vocab_size > ops.SAMPLE_MAX_V:
            raise ValueError(f"--decode_strategy sample: --vocab_size {args.vocab_size} is beyond the sampling kernel's {ops.SAMPLE_MAX_V} columns")
    constraints = None
    if args.do_eval:
        try:
            constraints = make_constraints(repetition_penalty=args.repetition_penalty, no_repeat_ngram_size=args.no_repeat_ngram_size,
                                           min_length=args.min_length_decoder, suppress_tokens=args.suppress_tokens)
        except ValueError as e:
            msg = str(e)                       # the argument's name opens the message: say the flag's instead
            for name, flag in (("repetition_penalty", "--repetition_penalty"), ("no_repeat_ngram_size", "--no_repeat_ngram_size"),
                               ("min_length", "--min_length_decoder"), ("suppress_tokens", "--suppress_tokens")):
                if msg.startswith(name + " "):
                    msg = flag + msg[len(name):]
            raise ValueError(msg) from None
        if args.min_length_decoder > args.max_len_decoder:
            raise ValueError(f"--min_length_decoder {args.min_length_decoder} is beyond --max_len_decoder {args.max_len_decoder}: no "
                             f"sequence could end")
        if constraints is not None:
            if not 1 <= args.max_len_decoder <= ops.CONSTRAIN_MAX_T:
                raise ValueError(f"--repetition_penalty / --no_repeat_ngram_size / --min_length_decoder / --suppress_tokens: "
                                 f"--max_len_decoder {args.max_len_decoder} is outside the constraint kernel's 1 .. {ops.CONSTRAIN_MAX_T} tokens")
            if args.decode_strategy == "beam" and not 1 <= args.beam_size <= ops.TOPK_MAX:      # constraints imply the batched step
                raise ValueError(f"--repetition_penalty / --no_repeat_ngram_size / --min_length_decoder / --suppress_tokens: --beam_size "
                                 f"{args.beam_size} is outside the top-k kernel's 1 .. {ops.TOPK_MAX}")
            width = args.beam_size if args.decode_strategy == "beam" else 1
            need = args.max_len_decoder + 1 + len(args.suppress_tokens) + width
            if 0 < args.vocab_size < need:     # (0: the tokenizer's size, known later; the decode checks it again)
                raise ValueError(f"--suppress_tokens / --max_len_decoder: --vocab_size {args.vocab_size} cannot keep {width} tokens "
                                 f"unbanned (needs >= {need})")
    check_loss_arguments(args)
    check_ema_arguments(args)
    check_adv_arguments(args)
    rank, _, world, device, master, logger = init_run(args, "iaog", "pretraining_iaog.log", script="run_pretraining_fcmf.py")

    tokenizer = None
    dev_set = test_set = None          # callables -> the batches of one pass (--do_eval)
    if args.synthetic_steps <= 0:
        from transformers import AutoTokenizer
        tokenizer = AutoTokenizer.from_pretrained(args.pretrained_hf_model)
    vocab = args.vocab_size or (len(tokenizer) if tokenizer is not None else 0)
    if vocab <= 0:
        from fcmf_framework.roberta import RobertaConfig
        vocab = RobertaConfig.from_pretrained(args.pretrained_hf_model).vocab_size
    model = FCMFSeq2Seq(vocab, args.max_len_decoder, args.pretrained_hf_model, args.num_imgs, args.num_rois, args.alpha)
    model.decoder.embedding = torch.nn.Embedding(vocab, model.decoder.num_hiddens)       # reference :189
    model = model.to(device)

    # the two ResNet-152 extractors (reference :191-194) whenever pixels enter the step: real data without a feature cache,
    # or --synthetic_pixels
    r_img = r_roi = None
    if args.do_eval and args.synthetic_steps <= 0 and args.feature_cache_dir:
        raise ValueError("--do_eval decodes the dev / test reviews from pixels: the feature cache holds the training reviews only, "
                         "run without --feature_cache_dir")
    if (args.synthetic_steps > 0 and args.synthetic_pixels > 0) or (args.synthetic_steps <= 0 and not args.feature_cache_dir):
        from fcmf_framework.resnet import resnet152
        sd = torch.load(args.resnet_checkpoint, map_location='cpu', weights_only=True) if args.resnet_checkpoint else None
        r_img, r_roi = build_extractors(lambda: resnet152(weights=sd), args.fine_tune_cnn, device)
        r_img.train(); r_roi.train()

    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    cnn_params = []
    if args.fine_tune_cnn and r_img is not None:                     # reference :203-207 (names: 'resnet.conv1.weight', ...)
        cnn_params = list(r_img.named_parameters()) + list(r_roi.named_parameters())
        named += cnn_params
    decay, exempt = split_decay(named)
    groups = [{'params': decay, 'weight_decay': 1e-5}, {'params': exempt, 'weight_decay': 0.0}]
    optimizer = FusedAdamW(groups, lr=args.learning_rate, eps=args.adam_epsilon)
    ema = setup_ema(optimizer, args, logger, master)        # before a checkpoint's optimizer state is loaded: its 'ema' is kept

    if args.synthetic_steps > 0:
        import synthetic_data as synth
        cfg = model.encoder.bert.cell.config
        cfgd = dict(vocab_size=cfg.vocab_size, pad_token_id=cfg.pad_token_id)

        def draw(B, batch_seed, dec_seed):
            b = synth.synth_batch(B, cfgd, S=min(args.max_seq_length, 128, cfg.max_position_embeddings - 2), num_imgs=args.num_imgs, num_roi=args.num_rois,
                                  num_aspects=1, seed=batch_seed, coord_dtype=torch.float32)
            g = torch.Generator().manual_seed(dec_seed)
            dec = torch.randint(3, vocab, (B, args.synthetic_dec_len), generator=g)
            lab = torch.roll(dec, -1, dims=1)
            lab[:, -1] = -100                                                           # iaog_dataset.py:93-96
            if args.synthetic_pixels:             # pixel crops in the IAOG dataset's float32 layout (iaog_dataset.py:148)
                b["visual_embeds_att"], b["roi_embeds_att"] = synth.synth_pixel_batch(
                    B, args.num_imgs, args.num_rois, args.synthetic_pixels, dec_seed, torch.float32)
            return (b["visual_embeds_att"], b["roi_embeds_att"], b["roi_coors"], b["input_ids"][:, 0],
                    b["token_type_ids"][:, 0], b["attention_mask"][:, 0], b["added_attention_mask"][:, 0], dec, lab)

        def batches():
            for i in range(args.synthetic_steps):
                # (the decoder / pixel seed lacks the `1000 * rank` term of the batch seed: every rank draws the same pixels)
                yield draw(args.train_batch_size, args.seed + 1000 * rank + i, args.seed + i)
        steps_per_epoch = args.synthetic_steps
        make_loader = batches

        if args.do_eval and args.synthetic_eval_samples > 0:
            # dev / test sets drawn like the training batches, in the dataset's 11-tuple; the text path runs through IdTokenizer
            from fcmf_framework.roberta import RobertaConfig
            from review_batches import ASPECTS
            aspects = list(args.list_aspect) or list(ASPECTS)
            tokenizer = score_tokenizer = synth.IdTokenizer(dict(
                vocab_size=min(vocab, RobertaConfig.from_pretrained(bert_score_dir).vocab_size), pad_token_id=cfg.pad_token_id))

            def eval_set(seed0):
                def it():
                    n = args.synthetic_eval_samples
                    for s0 in range(0, n, args.eval_batch_size):
                        B = min(args.eval_batch_size, n - s0)
                        vis, roi, coors, ids, tt, am, added, dec, lab = draw(B, seed0 + s0, seed0 + s0 + 7)
                        yield (vis, roi, coors, lab, dec, ids, tt, am, added, [aspects[(s0 + k) % len(aspects)] for k in range(B)],
                               [f"synthetic review {s0 + k}" for k in range(B)])
                return it
            dev_set, test_set = eval_set(args.seed + 500000), eval_set(args.seed + 600000)
    else:
        # real data (reference :130-183): reviews with `iaog_labels`, one sample per (review, aspect); photos through the
        # HIP ResNet-152 trunk inside the step, or a precomputed feature cache.  (The reference also runs underthesea's
        # Vietnamese text normalisation over the comments; that host-side text cleaning is not part of this build --
        # feed already-normalised JSON.)
        import json
        import pandas as pd
        from torch.utils.data import DataLoader, DistributedSampler, RandomSampler
        from iaog_dataset import IAOGDataset
        train_data = pd.read_json(f'{args.pretrained_data_dir}/train_with_iaog.json')
        if 'iaog_labels' not in train_data.columns:
            raise ValueError("'iaog_labels' column not found in data. Check JSON file structure.")
        roi_df = pd.read_csv(f"{args.data_dir}/roi_data.csv")
        roi_df['file_name'] = roi_df['file_name'] + '.png'
        with open(f'{args.data_dir}/resnet152_image_label.json') as f:
            dict_image_aspect = json.load(f)
        with open(f'{args.data_dir}/resnet152_roi_label.json') as f:
            dict_roi_aspect = json.load(f)
        cache = None
        if args.feature_cache_dir:
            from feature_cache import FeatureCache
            cache = FeatureCache(args.feature_cache_dir)
        train_ds = IAOGDataset(train_data, tokenizer, args.image_dir, roi_df, dict_image_aspect, dict_roi_aspect,
                               args.num_imgs, args.num_rois, args.max_len_decoder, feature_cache=cache,
                               max_seq_length=args.max_seq_length, list_aspect=args.list_aspect or None)
        if len(train_ds) == 0:
            raise SystemExit("train_dataset is empty: no 'sentiment_word#Aspect' labels in iaog_labels")
        sampler = DistributedSampler(train_ds) if world > 1 else RandomSampler(train_ds)      # shard once
        loader = DataLoader(train_ds, sampler=sampler, batch_size=args.train_batch_size, pin_memory=True)

        def batches():
            for t_img, roi_img, coors, labels, dec, enc_ids, enc_type, enc_mask, added, _, _ in loader:
                yield (t_img, roi_img, coors.float(), enc_ids, enc_type, enc_mask, added, dec, labels)
        steps_per_epoch = len(loader)
        make_loader = batches

        if args.do_eval:
            # dev (reference :133,175,282) and, if its file is there, test (:465-467): same plumbing as the train set, in order
            from torch.utils.data import SequentialSampler
            from transformers import AutoTokenizer
            aspects = list(train_ds.ASPECT)
            score_tokenizer = AutoTokenizer.from_pretrained(bert_score_dir, local_files_only=True)

            def eval_set(name):
                path = f'{args.pretrained_data_dir}/{name}_with_iaog.json'
                if not os.path.exists(path):
                    return None
                data = pd.read_json(path)
                if 'iaog_labels' not in data.columns:
                    raise ValueError(f"'iaog_labels' column not found in {path}")
                ds = IAOGDataset(data, tokenizer, args.image_dir, roi_df, dict_image_aspect, dict_roi_aspect, args.num_imgs,
                                 args.num_rois, args.max_len_decoder, max_seq_length=args.max_seq_length,
                                 list_aspect=args.list_aspect or None)
                return lambda: DataLoader(ds, sampler=SequentialSampler(ds), batch_size=args.eval_batch_size)
            dev_set, test_set = eval_set('dev'), eval_set('test')
            if dev_set is None:
                raise ValueError(f"--do_eval: {args.pretrained_data_dir}/dev_with_iaog.json not found")

    num_train_steps = int(steps_per_epoch / args.gradient_accumulation_steps * args.num_train_epochs)
    scheduler = get_linear_schedule_with_warmup(optimizer, int(num_train_steps * args.warmup_proportion), num_train_steps)
    # the trunks' gradients are produced LAST in backward (the extractors run first in the step): behind the model's in the arena
    arena = GradArena.for_model(model, extra=[p for _, p in cnn_params])
    reducer = None
    if world > 1:
        reducer = GradReducer(arena)
        reducer.broadcast_parameters(0)
    start_epoch = 0
    best_score = 0.0
    if args.resume_from_checkpoint and os.path.isfile(args.resume_from_checkpoint):
        ck = torch.load(args.resume_from_checkpoint, map_location=device, weights_only=True)
        model.load_state_dict(ck['model_state_dict'])
        optimizer.load_state_dict(ck['optimizer_state_dict'])
        scheduler.load_state_dict(ck['scheduler_state_dict'])
        start_epoch = ck['epoch'] + 1
        best_score = float(ck.get('best_score') or 0.0)                     # reference :271
        ops.shadows.clear()
        load_resnets(args.resume_from_checkpoint, r_img, r_roi, device, logger if master else None, old="iaog_model")   # reference :244-255

    features = make_features(r_img, r_roi)

    def loss_fn(batch):
        vis, roi, coors, enc_X, tt, am, added, dec_X, labels = batch
        vis, roi = features(vis, roi)
        # model(...) -> logits -> CrossEntropyLoss(ignore_index=-100) (reference :309-324) as one fused call
        return model.forward_loss(enc_X, dec_X, labels, vis, roi, coors, tt, am, added, ignore_index=-100,
                                  label_smoothing=args.label_smoothing, rdrop_alpha=args.rdrop_alpha if model.training else 0.0)

    evaluate = None
    if args.do_eval and master and dev_set is not None:
        from fcmf_framework.bertscore import BertScorer
        from iaog_eval import aspect_line, generate, macro_bertscore, write_predictions
        scorer = BertScorer(bert_score_dir, num_layers=12, device=device)
        score_fn = lambda cands, refs: scorer.score(cands, refs, score_tokenizer)

        def evaluate(batches):
            """-> (per_aspect, macro, results) of one pass over a dev / test set"""
            model.eval()
            if r_img is not None:
                r_img.eval(); r_roi.eval()
            preds, refs, results = generate(model, tokenizer, batches, features, args.beam_size, args.max_len_decoder, aspects,
                                               batched=args.batched_decode or args.decode_context == "prefix" or args.decode_loop == "device",
                                               context=args.decode_context, strategy=args.decode_strategy,
                                               sampler=dict(seed=args.sample_seed, temperature=args.temperature, top_k=args.top_k,
                                                            top_p=args.top_p),
                                               num_chains=args.num_chains, length_penalty=args.length_penalty,
                                               constraints=constraints, loop=args.decode_loop, poll_every=args.decode_poll_every)
            per_aspect, macro = macro_bertscore(preds, refs, aspects, score_fn)
            return per_aspect, macro, results
    elif args.do_eval and master:
        logger.info("--do_eval: no dev set (--synthetic_eval_samples is 0): nothing is evaluated")

    if args.do_train:
        if master:
            logger.info("training loss: label_smoothing %g", args.label_smoothing)
            log_rdrop(args, logger)
            log_adv(args, logger)
        for epoch in range(start_epoch, int(args.num_train_epochs)):
            model.train()
            if r_img is not None:
                r_img.train(); r_roi.train()
            log = lambda step, loss: logger.info("epoch %d step %d loss %.4f", epoch, step, loss)
            train_epoch(DevicePrefetcher(make_loader(), device), loss_fn, arena=arena, reducer=reducer, optimizer=optimizer,
                        scheduler=scheduler, accum=args.gradient_accumulation_steps, log=log if master else None,
                        adversary=make_adversary(args))
            if evaluate is not None:                                     # reference :376-452; the other ranks wait at the barrier below
                # (with --ema_decay the decode, the score and the best checkpoint are the averaged weights'; the master alone swaps)
                with averaged(optimizer, ema):
                    logger.info("***** Running evaluation on Dev Set with BEAM SEARCH *****")
                    per_aspect, macro, _ = evaluate(dev_set())
                    logger.info("Computing BERTScore for Dev Set using model: %s ...", bert_score_dir)
                    for a, m in per_aspect.items():
                        if m is not None:
                            logger.info("  Aspect: " + aspect_line(a, m))
                    logger.info("Epoch %d [Macro-Avg] F1: %.4f", epoch, macro[2])
                    if macro[2] > best_score:
                        best_score = macro[2]
                        logger.info("New Best F1-Score (%.4f)! Saving model...", best_score)
                        save_model(f'{args.output_dir}/seed_{args.seed}_iaog_model_best.pth', model, optimizer, scheduler, epoch, best_score)
                        save_extractors(args.output_dir, args.seed, 'best', r_img, r_roi, optimizer, scheduler, epoch, best_score)
            if world > 1:
                torch.distributed.barrier()
            if master:
                save_model(f'{args.output_dir}/seed_{args.seed}_iaog_model_last.pth', model, optimizer, scheduler, epoch, best_score)
                save_extractors(args.output_dir, args.seed, 'last', r_img, r_roi, optimizer, scheduler, epoch, best_score)   # reference :458-459
    if evaluate is not None and test_set is not None:                    # reference :462-632
        best = f'{args.output_dir}/seed_{args.seed}_iaog_model_best.pth'
        if os.path.exists(best):
            logger.info("Loading Best Checkpoint for Testing: %s", best)
            model.load_state_dict(torch.load(best, map_location=device, weights_only=True)['model_state_dict'])
            ops.shadows.clear()
            load_resnets(best, r_img, r_roi, device, logger, old="iaog_model")
        logger.info("Computing BERTScore for Test Set using model: %s ...", bert_score_dir)
        with averaged(optimizer, ema and not os.path.exists(best)):       # (a best checkpoint already holds the averaged weights)
            per_aspect, macro, results = evaluate(test_set())
        log_path = f"{args.output_dir}/iaog_test_predictions_formatted.txt"
        write_predictions(log_path, bert_score_dir, per_aspect, macro, results)
        for a, m in per_aspect.items():
            if m is not None:
                logger.info(aspect_line(a, m))
        logger.info("***** TEST RESULTS (Macro Avg) *****")
        logger.info("Test Precision: %.4f", macro[0])
        logger.info("Test Recall:    %.4f", macro[1])
        logger.info("Test F1-Score:  %.4f", macro[2])
        logger.info("Formatted predictions saved to %s", log_path)
    arena.deactivate()
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
