"""What run_multimodal_fcmf.py and run_pretraining_fcmf.py share: process / logger set-up, the checkpoint dictionary, the
ResNet-152 extractors with their checkpoints beside the model's, the weight-decay split and the loop of one epoch.  Each
driver keeps its parser, model, data, parameter groups, loss call and (fine-tuning) evaluation.  File:line citations are
into the reference's two drivers."""
import contextlib
import json
import logging
import math
import os
import random

import numpy as np
import torch

from fcmf_framework import ops
from fcmf_framework.resnet_utils import extract_features, myResNetImg, myResNetRoI

NO_DECAY = ['bias', 'LayerNorm.bias', 'LayerNorm.weight']      # run_multimodal_fcmf.py:249, run_pretraining_fcmf.py:203


def split_decay(named):
    """(name, parameter) pairs -> (parameters that get weight decay, parameters that do not), each in the given order"""
    decay, exempt = [], []
    for n, p in named:
        (exempt if any(nd in n for nd in NO_DECAY) else decay).append(p)
    return decay, exempt


# ---- the training loss's options (ops.cross_entropy / ops.vocab_cross_entropy) -----------------------------------------------
EVAL_LOSS_NOTE = ("evaluation is untouched: a dev / test eval_loss stays plain cross entropy, so result files compare across runs "
                  "with and without it")


def add_loss_arguments(parser, class_weights=True):
    """--label_smoothing, and for the aspect classifiers --class_weights / --focal_gamma (values are checked by check_loss_arguments)"""
    if class_weights:
        parser.add_argument('--class_weights', default='none', type=str,
                            help="training-loss class weights: none | balanced (per aspect N / (C * max(count, 1)) over the training "
                                 "split's labels) | a comma list of --num_polarity floats; every aspect is divided by its own weight "
                                 "sum; written to output_dir/class_weights.json; " + EVAL_LOSS_NOTE)
        parser.add_argument('--focal_gamma', default=0.0, type=float,
                            help="focal exponent of the training loss, (1 - p_y)^gamma; 0 = off, not together with --label_smoothing; "
                                 + EVAL_LOSS_NOTE)
    parser.add_argument('--label_smoothing', default=0.0, type=float,
                        help="label smoothing of the training loss, in [0, 1); " + EVAL_LOSS_NOTE)
    parser.add_argument('--rdrop_alpha', default=0.0, type=float,
                        help="R-Drop (Liang et al., 2021): every training sample runs twice under independent dropout masks and "
                             "alpha x the bidirectional KL divergence between the two predictions, 1/2 [KL(p||q) + KL(q||p)], is added "
                             "to the mean of the two cross entropies; 0 = off.  The KL term is the BATCH MEAN (per aspect; per live "
                             "target position for IAOG), not the sum over the batch of the authors' script.  Activation memory "
                             "doubles; " + EVAL_LOSS_NOTE)


def check_loss_arguments(args):
    """refuses bad loss flags with a ValueError that names the flag (call before anything is created or written)
    -> the class-weight request: None, "balanced" or a list of num_polarity floats"""
    eps, gamma = args.label_smoothing, getattr(args, "focal_gamma", 0.0)
    if not (math.isfinite(eps) and 0.0 <= eps < 1.0):
        raise ValueError(f"--label_smoothing must lie in [0, 1), got {eps}")
    if not (math.isfinite(gamma) and gamma >= 0.0):
        raise ValueError(f"--focal_gamma must be finite and >= 0, got {gamma}")
    if eps > 0.0 and gamma > 0.0:
        raise ValueError(f"--focal_gamma {gamma} and --label_smoothing {eps} cannot both be set")
    alpha = getattr(args, "rdrop_alpha", 0.0)
    if not (math.isfinite(alpha) and alpha >= 0.0):
        raise ValueError(f"--rdrop_alpha must be finite and >= 0 (0 = off), got {alpha}")
    spec = getattr(args, "class_weights", "none").strip()
    if spec.lower() in ("none", "balanced"):
        return None if spec.lower() == "none" else "balanced"
    try:
        values = [float(v) for v in spec.split(",")]
    except ValueError:
        raise ValueError(f"--class_weights must be none, balanced or a comma list of {args.num_polarity} floats, got {spec!r}") from None
    if len(values) != args.num_polarity:
        raise ValueError(f"--class_weights lists {len(values)} values, --num_polarity is {args.num_polarity}")
    if not all(math.isfinite(v) and v >= 0.0 for v in values) or sum(values) <= 0.0:
        raise ValueError(f"--class_weights must be finite, >= 0 and not all zero, got {spec!r}")
    return values


def log_rdrop(args, logger):
    """the line that goes beside "training loss:" when training starts"""
    logger.info("training loss: rdrop_alpha %g%s", args.rdrop_alpha,
                " (two dropout passes per sample + alpha x the batch-mean symmetric KL)" if args.rdrop_alpha > 0 else " (off)")


# ---- adversarial training on the text embeddings (ops.EmbeddingAdversary) ---------------------------------------------------------
def add_adv_arguments(parser):
    parser.add_argument('--adv_epsilon', default=0.0, type=float,
                        help="FGM adversarial training (Miyato et al., 2017) on the text encoder's token embeddings: every micro-batch "
                             "runs a second forward and backward with epsilon * g / ||g||_2 added to each sequence's embeddings (g: the "
                             "clean pass's gradient there, pad tokens excluded) and the two gradients are summed; 0 = off.  About two "
                             "steps of time per step; no value is recommended: accuracy has not been measured.  " + EVAL_LOSS_NOTE)


def check_adv_arguments(args):
    """refuses a bad --adv_epsilon with a ValueError that names the flag (call before anything is created or written)
    -> epsilon, 0.0 = off"""
    e = args.adv_epsilon
    if not (math.isfinite(e) and e >= 0.0):
        raise ValueError(f"--adv_epsilon must be finite and >= 0 (0 = off), got {e}")
    if e > 0.0 and getattr(args, "freeze_encoder", False):
        raise ValueError(f"--adv_epsilon {e} perturbs the text embeddings through their gradient: not together with --freeze_encoder")
    return e


def log_adv(args, logger):
    """the line that goes beside log_rdrop's"""
    logger.info("training loss: adv_epsilon %g%s", args.adv_epsilon,
                " (FGM: a second pass per micro-batch on the text embeddings + epsilon x their normalised gradient)"
                if args.adv_epsilon > 0 else " (off)")


def make_adversary(args):
    """train_epoch's `adversary` as --adv_epsilon asks: an ops.EmbeddingAdversary, or None (off)"""
    return ops.EmbeddingAdversary(args.adv_epsilon) if args.adv_epsilon > 0 else None


def twice(*tensors):
    """every tensor repeated along the batch axis (copy i and copy i + B of sample i): what an R-Drop step feeds the model"""
    return tuple(None if t is None else torch.cat((t, t), dim=0) for t in tensors)


# ---- averaged weights (FusedAdamW.set_ema / ema_weights) ------------------------------------------------------------------------
def add_ema_arguments(parser):
    parser.add_argument('--ema_decay', default=0.0, type=float,
                        help="keep an exponential moving average of the optimizer's parameters, updated inside the AdamW kernel, "
                             "with this decay in (0, 1); 0 = off.  The dev evaluation of every epoch runs on the averaged weights, "
                             "*_best.pth is chosen by their score and holds them, *_last.pth holds the raw weights and carries the "
                             "average in the optimizer state.  BatchNorm running statistics of the ResNet trunks are buffers, not "
                             "optimizer parameters: they are not averaged")
    parser.add_argument('--ema_no_warmup', action='store_true',
                        help="use --ema_decay from the first step on; default: step t uses min(ema_decay, (1 + t) / (10 + t))")


def check_ema_arguments(args):
    """refuses a bad --ema_decay with a ValueError that names the flag (call before anything is created or written)
    -> the decay, 0.0 = off"""
    d = args.ema_decay
    if not (math.isfinite(d) and 0.0 <= d < 1.0):
        raise ValueError(f"--ema_decay must lie in [0, 1), got {d}")
    return d


def setup_ema(optimizer, args, logger, master):
    """turn the average on as the flags ask (every rank: all of them take the same steps) -> whether it is on"""
    if args.ema_decay <= 0.0:
        return False
    optimizer.set_ema(args.ema_decay, warmup=not args.ema_no_warmup)
    if master:
        logger.info("weight EMA: decay %g, %s; dev evaluation and *_best.pth use the averaged weights", args.ema_decay,
                    "no warmup" if args.ema_no_warmup else "warmup min(decay, (1 + t) / (10 + t)) at optimizer step t")
    return True


def averaged(optimizer, on):
    """`with averaged(optimizer, ema and master):` -- the block runs on the averaged weights (one swap launch in, one out; no
    collective call, so one rank may enter alone), or on the parameters as they are"""
    return optimizer.ema_weights() if on else contextlib.nullcontext()


def balanced_class_weights(labels, num_classes):
    """labels: integers [N, A] (one column per aspect) -> float32 [A, num_classes], w[a, c] = N / (C * max(count[a, c], 1)):
    scikit-learn's class_weight="balanced" per aspect, a class that an aspect never shows counted once"""
    labels = np.asarray(labels, dtype=np.int64)
    if labels.ndim != 2 or labels.shape[0] == 0:
        raise ValueError(f"balanced class weights need a non-empty [reviews, aspects] label table, got shape {labels.shape}")
    if labels.min() < 0 or labels.max() >= num_classes:
        raise ValueError(f"labels outside [0, {num_classes}) in the training split")
    N, A = labels.shape
    counts = np.stack([np.bincount(labels[:, a], minlength=num_classes) for a in range(A)])
    return (N / (num_classes * np.maximum(counts, 1))).astype(np.float32)


def train_label_table(loader, first_wins=True):
    """the training split's labels [reviews, aspects] without touching a photo: from the dataset's frame where the loader has one
    (column 3, "Aspect#Polarity" lists, as the datasets read it), else from the (synthetic) batches' label field"""
    ds = getattr(loader, "dataset", None)
    if ds is not None and hasattr(ds, "data"):
        from review_batches import polarity_labels
        aspects = getattr(ds, "ASPECT")
        return np.stack([polarity_labels(ann, aspects, first_wins=first_wins).numpy() for ann in ds.data.iloc[:, 3]])
    return np.concatenate([np.asarray(batch[-2]) for batch in loader])


def class_weight_tensor(request, labels_fn, num_aspects, num_classes, device, output_dir, logger, master):
    """check_loss_arguments' request -> the loss's weight (float32 on the device: [A, C] balanced, [C] listed) or None; logged and
    written to output_dir/class_weights.json by the master.  labels_fn() returns the training label table (balanced only)."""
    if request is None:
        return None
    w = balanced_class_weights(labels_fn(), num_classes) if request == "balanced" else np.asarray(request, dtype=np.float32)
    if w.ndim == 2 and w.shape[0] != num_aspects:
        raise ValueError(f"--class_weights balanced: the label table has {w.shape[0]} aspects, --list_aspect names {num_aspects}")
    if master:
        logger.info("class weights (%s): %s", "aspect x polarity" if w.ndim == 2 else "polarity", w.tolist())
        with open(os.path.join(output_dir, "class_weights.json"), "w") as f:
            json.dump({"mode": "balanced" if request == "balanced" else "list", "weights": w.tolist()}, f)
    return torch.from_numpy(w).to(device)


def init_run(args, logger_name, log_file, formatter=None, script="this driver"):
    """device, seeds, process group, logger (handlers on the master only) and compute dtype of one driver process, under torchrun's
    RANK / LOCAL_RANK / WORLD_SIZE with --ddp (run_multimodal_fcmf.py:126-169, run_pretraining_fcmf.py:86-104)
    -> rank, local_rank, world, device, master, logger"""
    if args.no_cuda or not torch.cuda.is_available():
        raise SystemExit(f"{script} (MI355X build) has no CPU path: a ROCm GPU is required")
    rank, local_rank, world = [int(os.environ[k]) for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE')] if args.ddp else (0, 0, 1)
    torch.cuda.set_device(local_rank)
    device = torch.device('cuda', local_rank)
    random.seed(args.seed); np.random.seed(args.seed); torch.manual_seed(args.seed); ops.manual_seed(args.seed + rank)
    if world > 1:
        torch.distributed.init_process_group(backend='nccl', device_id=device)   # RCCL over xGMI
    logger = logging.getLogger(logger_name)
    if rank == 0:
        os.makedirs(args.output_dir, exist_ok=True)
        logger.setLevel(logging.INFO)
        for h in (logging.FileHandler(f'{args.output_dir}/{log_file}'), logging.StreamHandler()):
            if formatter is not None:
                h.setFormatter(formatter)
            logger.addHandler(h)
    ops.set_compute_dtype(torch.bfloat16 if (args.bf16 or args.fp16) else torch.float32)
    return rank, local_rank, world, device, rank == 0, logger


def save_model(path, model, optimizer, scheduler, epoch, best_score=0.0):
    """checkpoint dict of the reference (run_multimodal_fcmf.py:40-58, run_pretraining_fcmf.py:27-42)"""
    m = model.module if hasattr(model, 'module') else model
    torch.save({'epoch': epoch, 'best_score': best_score, 'model_state_dict': m.state_dict(),
                'optimizer_state_dict': optimizer.state_dict(), 'scheduler_state_dict': scheduler.state_dict()}, path)


def companion_path(path, old, new):
    """the reference's checkpoint-path rewrite (run_multimodal_fcmf.py: `checkpoint_path.replace("fcmf_model", "resimg_model")`,
    :334-335; `best_path.replace("fcmf", "resimg")`, :588,594) applied to the FILE NAME only -- a directory called e.g.
    `runs/fcmf/` must not be rewritten with it"""
    d, f = os.path.split(path)
    return os.path.join(d, f.replace(old, new))


def load_resnets(path, resnet_img, resnet_roi, device, logger=None, old="fcmf_model", strict=True):
    """restore the two extractors saved beside the model checkpoint `path` (run_multimodal_fcmf.py:334-346 / :588-598,
    run_pretraining_fcmf.py:244-255): `old` is the part of the file name that `resimg...` / `resroi...` replaces"""
    loaded = []
    for net, tag in ((resnet_img, "resimg"), (resnet_roi, "resroi")):
        q = companion_path(path, old, old.replace("fcmf", tag).replace("iaog", tag))
        if net is not None and os.path.exists(q):
            ck = torch.load(q, map_location=device, weights_only=True)
            net.load_state_dict(ck['model_state_dict'], strict=strict)
            loaded.append(q)
            if logger is not None:
                logger.info("    Loading ResNet %s from: %s", tag, q)
    if loaded:
        ops.shadows.clear()                  # cached bf16 weight matrices of the trunk are stale
    return loaded


def save_extractors(output_dir, seed, tag, resnet_img, resnet_roi, optimizer, scheduler, epoch, best_score=0.0):
    """the extractors (if any) beside the model checkpoint (run_multimodal_fcmf.py:557-563, run_pretraining_fcmf.py:457-459)"""
    for net, name in ((resnet_img, "resimg"), (resnet_roi, "resroi")):
        if net is not None:
            save_model(f'{output_dir}/seed_{seed}_{name}_model_{tag}.pth', net, optimizer, scheduler, epoch, best_score)


def build_extractors(make_trunk, fine_tune, device):
    """the two feature extractors, each on its own `make_trunk()` (run_multimodal_fcmf.py:224-227, run_pretraining_fcmf.py:191-194)"""
    return myResNetImg(make_trunk().to(device), fine_tune, device), myResNetRoI(make_trunk().to(device), fine_tune, device)


def make_features(resnet_img, resnet_roi):
    """-> features(images, roi_crops): pixels -> ResNet-152 features, the reference's num_imgs + num_imgs * num_rois trunk calls
    (run_multimodal_fcmf.py:445-460, run_pretraining_fcmf.py:299-317) as two batched passes; a batch of features passes through"""
    def features(t_img, roi_img):
        if resnet_img is None:
            return t_img, roi_img
        return extract_features(resnet_img, resnet_roi, t_img, roi_img.float())
    return features


def train_epoch(batches, loss_fn, *, arena, reducer, optimizer, scheduler, accum, log=None, adversary=None):
    """one epoch (run_multimodal_fcmf.py:427-489, run_pretraining_fcmf.py:284-337): `loss_fn(batch)` accumulates over `accum`
    steps, then the gradients are reduced across ranks (`reducer`, None on one rank), clipped to norm 1.0 and applied; a trailing
    partial group gets no optimizer step.  `log(step, loss)`, if given, sees the undivided loss of every 10th step.
    adversary (ops.EmbeddingAdversary): every micro-step is a clean pass under record(), never reduced, then a pass on the
    perturbed embeddings under attack() whose backward accumulates onto the first as a further micro-step does (temporaries that
    autograd adds; each backward flushes its own deferred weight gradients when the engine finishes); the logged loss is the
    clean one."""
    arena.zero()
    for step, batch in enumerate(batches):
        boundary = (step + 1) % accum == 0
        if adversary is not None:
            with adversary.record():
                loss = loss_fn(batch)
            if accum > 1:
                loss = loss / accum
            if reducer is not None:
                reducer.enabled = False
            loss.backward()
            with adversary.attack():
                adv_loss = loss_fn(batch)
            if accum > 1:
                adv_loss = adv_loss / accum
        else:
            loss = loss_fn(batch)
            if accum > 1:
                loss = loss / accum
            adv_loss = loss
        if reducer is not None:
            reducer.enabled = boundary                        # all-reduce only the accumulated gradients
        adv_loss.backward()
        if boundary:
            if reducer is not None:
                reducer.finish()
            optimizer.step(max_grad_norm=1.0)                 # clip_grad_norm_(1.0) fused into AdamW
            scheduler.step()
            arena.zero()
        if log is not None and step % 10 == 0:
            log(step, loss.item() * accum)
