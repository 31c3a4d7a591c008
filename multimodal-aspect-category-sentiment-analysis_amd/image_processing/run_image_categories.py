"""Photo categories (reference image_processing/run_image_categories.py) on the MI355X: fine-tunes ResNet-152 + a 5-way
multi-label head (BCE with logits, Adam, --learning_rate, keep the best dev accuracy) and labels every photo of --image_dir
into {output_dir}/resnet152_image_label.json, the file run_multimodal_fcmf.py / run_pretraining_fcmf.py read.

Same flags, defaults, log / checkpoint / result file names, split (70/15/15 over label rows, random_state=18), thresholds
(0.7 on dev / test, 0.45 for --get_cate) and epoch loop as the reference.  Preprocessing (resize + flip + normalise) is one
HIP launch per batch (fcmf_framework.image_ops.crop_batch); the trunk, head, loss and optimizer are the HIP kernels.
Extra flags: --resnet_checkpoint (a local torchvision ResNet-152 state dict: the reference's IMAGENET1K_V2 start), --bf16.

Deliberate differences from the reference:
  * the tag lists in the JSON are sorted (the FCMF prompt builder, ReviewProducer.visual_tags, sorts them anyway);
  * the shuffle and RandomHorizontalFlip draws come from a generator seeded with --seed, not from torch's global RNG stream.
As in the reference, the test metrics are accumulated into the lists of the last dev evaluation (they are not reset).
"""
import argparse
import json
import logging
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fcmf_framework import categories as CAT        # noqa: E402
from fcmf_framework import ops                      # noqa: E402
from fcmf_framework.image_ops import crop_batch     # noqa: E402
from fcmf_framework.optimization import FusedAdamW  # noqa: E402

ASPECT = CAT.IMAGE_ASPECTS


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument("--image_dir", default='../image', type=str, required=True)
    parser.add_argument("--image_label_path", default=None, type=str)
    parser.add_argument("--weight_path", default=None, type=str)
    parser.add_argument("--output_dir", default="../vimacsa", type=str)
    parser.add_argument("--do_train", action='store_true')
    parser.add_argument("--get_cate", action='store_true')
    parser.add_argument("--train_batch_size", default=8, type=int)
    parser.add_argument("--eval_batch_size", default=8, type=int)
    parser.add_argument("--learning_rate", default=3e-5, type=float)
    parser.add_argument("--num_train_epochs", default=8.0, type=float)
    parser.add_argument('--seed', type=int, default=42)
    parser.add_argument("--no_cuda", action='store_true')
    parser.add_argument("--resnet_checkpoint", default=None, type=str,
                        help="local torchvision ResNet-152 state dict to start from (nothing is downloaded)")
    parser.add_argument("--bf16", action='store_true', help="bf16 activations on the MFMA kernels")
    return parser


def _batches(df, image_dir, bs, order, flip_gen=None):
    """-> (crops on the GPU, float targets [B, 5] on the GPU) per batch of label rows"""
    for i in range(0, len(order), bs):
        rows = df.iloc[order[i:i + bs]]
        photos = CAT.load_photos([os.path.join(image_dir, n) for n in rows["file_name"]])
        x = crop_batch(photos, flip=flip_gen, dtype=ops.compute_dtype())
        y = torch.from_numpy(rows.iloc[:, 2:].values.astype(int)).float().cuda()
        yield x, y


def _evaluate(model, df, args, true_lists, pred_lists, loss_sum=None):
    model.eval()
    step = 0
    with torch.no_grad():
        for step, (x, y) in enumerate(_batches(df, args.image_dir, args.eval_batch_size, np.arange(len(df)))):
            logits = model(x)
            if loss_sum is not None:
                loss_sum[0] += ops.bce_with_logits(logits, y).item()
            probs = ops.sigmoid(logits).cpu().numpy()
            lab = y.cpu().numpy().astype(int)
            for a in range(len(ASPECT)):
                true_lists[ASPECT[a]].append(lab[:, a])
                pred_lists[ASPECT[a]].append(np.asarray(probs[:, a] > 0.7).astype(int))
    return step


def _scores(true_lists, pred_lists):
    out = []
    for asp in ASPECT:
        tr, pr = np.concatenate(true_lists[asp]), np.concatenate(pred_lists[asp])
        p, r, f, _ = CAT.precision_recall_fscore_support(tr, pr, labels=[0, 1], average='macro')
        out.append((asp, p, r, f, CAT.accuracy_score(tr, pr)))
    return out


def train(args, logger):
    if args.image_label_path is None:
        raise ValueError("Please provide annotated image file.")
    image_label = CAT.read_image_labels(args.image_label_path)
    train_data, dev_test_data = CAT.train_test_split(image_label, test_size=0.3, random_state=18)
    dev_data, test_data = CAT.train_test_split(dev_test_data, test_size=0.5, random_state=18)
    train_data, dev_data, test_data = (d.reset_index(drop=True) for d in (train_data, dev_data, test_data))

    model = CAT.make_model(CAT.MyImgModel, len(ASPECT), args.resnet_checkpoint).cuda()
    optimizer = FusedAdamW(model.parameters(), lr=args.learning_rate, weight_decay=0.0)      # torch.optim.Adam
    gen = torch.Generator().manual_seed(args.seed)
    ckpt = f'{args.output_dir}/seed_{args.seed}_image_model.pth'
    max_accuracy = 0.0
    true_lists = pred_lists = None
    logger.info("*************** Running training ***************")
    for epoch in range(int(args.num_train_epochs)):
        model.train()
        order = torch.randperm(len(train_data), generator=gen).numpy()
        for x, y in _batches(train_data, args.image_dir, args.train_batch_size, order, flip_gen=gen):
            loss = ops.bce_with_logits(model(x), y)
            loss.backward()
            optimizer.step()
            optimizer.zero_grad()
        logger.info("***** Running evaluation on Dev Set*****")
        true_lists, pred_lists = {a: [] for a in ASPECT}, {a: [] for a in ASPECT}
        _evaluate(model, dev_data, args, true_lists, pred_lists)
        all_accuracy = float(np.mean([s[4] for s in _scores(true_lists, pred_lists)]))
        if all_accuracy >= max_accuracy:
            CAT.save_model(ckpt, model, epoch)
            max_accuracy = all_accuracy
            logger.info(f"New Best Accuracy: {max_accuracy:.4f}")

    output_test_file = os.path.join(args.output_dir, "test_image_results.txt")
    with open(output_test_file, "a") as writer:
        writer.write("***** Running evaluation on Test Set *****\n")
        writer.write(f"  Num examples = {test_data.shape[0]}\n")
        writer.write(f"  Batch size = {args.eval_batch_size}\n")
    logger.info("***** Running evaluation on Test Set *****")
    logger.info("  Num examples = %d", test_data.shape[0])
    logger.info("  Batch size = %d", args.eval_batch_size)
    model.load_state_dict(CAT.load_model(ckpt)['model_state_dict'])
    if true_lists is None:
        true_lists, pred_lists = {a: [] for a in ASPECT}, {a: [] for a in ASPECT}
    loss_sum = [0.0]
    step = _evaluate(model, test_data, args, true_lists, pred_lists, loss_sum)
    test_loss = loss_sum[0] / (step if step else 1)          # (the reference divides by the last batch index)
    with open(output_test_file, "a") as writer:
        logger.info("***** Precision, Recall, F1-score, Accuracy for each Aspect *****")
        writer.write("***** Precision, Recall, F1-score, Accuracy for each Aspect *****\n")
        scores = _scores(true_lists, pred_lists)
        for asp, p, r, f, acc in scores:
            logger.info("  %s = %s", asp, str([p, r, f, acc]))
            writer.write(f"{asp} = {str([p, r, f, acc])}\n")
        results = {'eval_loss': test_loss,
                   'precision_score': float(np.mean([s[1] for s in scores])),
                   'recall_score': float(np.mean([s[2] for s in scores])),
                   'f_score': float(np.mean([s[3] for s in scores])),
                   'accuracy': float(np.mean([s[4] for s in scores]))}
        logger.info("***** Test Eval results *****")
        writer.write("***** Test Eval results *****\n")
        for key in sorted(results.keys()):
            logger.info("  %s = %s", key, str(results[key]))
            writer.write(f"{key} = {str(results[key])}\n")


def get_cate(args, logger):
    print("===================== GET IMAGE CATEGORIES =====================")
    model = CAT.make_model(CAT.MyImgModel, len(ASPECT), args.resnet_checkpoint).cuda()
    path = f'{args.output_dir}/seed_{args.seed}_image_model.pth' if args.do_train else args.weight_path
    if path is None:
        raise ValueError("--get_cate without --do_train needs --weight_path")
    model.load_state_dict(CAT.load_model(path)['model_state_dict'])
    model.eval()
    names = os.listdir(args.image_dir)
    labels = {}
    bs = args.eval_batch_size
    with torch.no_grad():
        for i in range(0, len(names), bs):
            batch = names[i:i + bs]
            x = crop_batch(CAT.load_photos([os.path.join(args.image_dir, n) for n in batch]), dtype=ops.compute_dtype())
            probs = ops.sigmoid(model(x)).cpu().numpy()
            for name, pr in zip(batch, probs):
                labels[name] = sorted(ASPECT[k] for k in np.where(pr > 0.45)[0])
    with open(f"{args.output_dir}/resnet152_image_label.json", "w", encoding='utf-8') as f:
        json.dump(labels, f, indent=2, ensure_ascii=False)
    logger.info("wrote %d photo labels", len(labels))


def main(argv=None):
    args = build_parser().parse_args(argv)
    print("===================== RUN IMAGE CATEGORIES =====================")
    os.makedirs(args.output_dir, exist_ok=True)
    logger = logging.getLogger("run_image_categories")
    logger.setLevel(logging.INFO)
    for h in list(logger.handlers):
        logger.removeHandler(h)
        h.close()
    fmt = logging.Formatter('%(asctime)s - %(levelname)s - %(name)s - %(message)s', datefmt='%m/%d/%Y %H:%M:%S')
    for h in (logging.FileHandler(f'{args.output_dir}/image_categories.log', mode='w'), logging.StreamHandler(sys.stdout)):
        h.setFormatter(fmt)
        logger.addHandler(h)
    if not args.do_train and not args.get_cate:
        raise ValueError("At least one of `do_train` or `get_cate` must be True.")
    if args.no_cuda:
        raise ValueError("--no_cuda: the classifiers run on the MI355X kernels only (there is no CPU path)")
    CAT.require_gpu()
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    ops.set_compute_dtype(torch.bfloat16 if args.bf16 else torch.float32)
    try:
        if args.do_train:
            train(args, logger)
        if args.get_cate:
            get_cate(args, logger)
    finally:
        ops.set_compute_dtype(torch.float32)
        for h in list(logger.handlers):
            logger.removeHandler(h)
            h.close()


if __name__ == "__main__":
    main()
