"""ROI categories (reference image_processing/run_roi_categories.py) on the MI355X: fine-tunes ResNet-152 + a 5-way head over
ROI crops (cross entropy, Adam, --learning_rate, keep the best dev accuracy) and labels every photo of the ROI file into
{output_dir}/resnet152_roi_label.json, the file run_multimodal_fcmf.py / run_pretraining_fcmf.py read.

Same flags, defaults, log / checkpoint / result file names, split (70/15/15 over unique file names, random_state=18:
prepare_roi_data_correctly) and epoch loop as the reference; --get_cate takes the first 6 ROIs of a photo, an argmax per ROI,
and keys `file_name + ".png"`.  All ROIs of a batch are cut from their uploaded photos by one HIP launch
(fcmf_framework.image_ops.crop_batch: a photo is uploaded once however many ROIs it has).
Extra flags: --resnet_checkpoint (a local torchvision ResNet-152 state dict: the reference's IMAGENET1K_V2 start), --bf16.

Deliberate differences from the reference:
  * the tag lists in the JSON are sorted (the reference's list(set(...)) order depends on the hash seed; the FCMF prompt
    builder, ReviewProducer.visual_tags, sorts them anyway);
  * the shuffle and RandomHorizontalFlip draws come from a generator seeded with --seed, not from torch's global RNG stream.
"""
import argparse
import json
import logging
import os
import sys
from collections import defaultdict

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fcmf_framework import categories as CAT        # noqa: E402
from fcmf_framework import ops                      # noqa: E402
from fcmf_framework.image_ops import crop_batch     # noqa: E402
from fcmf_framework.optimization import FusedAdamW  # noqa: E402

ASPECT = CAT.ROI_ASPECTS
NUM_ROI = 6


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument("--image_dir", default='../image', type=str, required=True)
    parser.add_argument("--roi_label_path", default=None, type=str, required=True)
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


def prepare_roi_data_correctly(roi_label_path, seed=18):
    """run_roi_categories.py:90-115: the 70/15/15 split over unique photos, every ROI of a photo on the same side"""
    roi_df = CAT.read_roi_labels(roi_label_path)
    unique_img_ids = roi_df['file_name'].unique()
    train_imgs, dev_test_imgs = CAT.train_test_split(unique_img_ids, test_size=0.3, random_state=seed)
    dev_imgs, test_imgs = CAT.train_test_split(dev_test_imgs, test_size=0.5, random_state=seed)
    pick = lambda imgs: roi_df[roi_df['file_name'].isin(imgs)].reset_index(drop=True)
    return pick(train_imgs), pick(dev_imgs), pick(test_imgs)


def _batches(df, image_dir, bs, order, flip_gen=None):
    """-> (crops on the GPU, labels on the GPU, photo names) per batch of ROI rows (each photo decoded once per batch)"""
    for i in range(0, len(order), bs):
        rows = df.iloc[order[i:i + bs]]
        names = [n + ".png" for n in rows["file_name"]]
        uniq = sorted(set(names))
        decoded = dict(zip(uniq, CAT.load_photos([os.path.join(image_dir, n) for n in uniq])))
        boxes = [[tuple(int(v) for v in rows.iloc[k, 1:5].values)] for k in range(len(rows))]
        x = crop_batch([decoded[n] for n in names], boxes, flip=flip_gen, dtype=ops.compute_dtype())
        y = torch.tensor([ASPECT.index(lb) for lb in rows['label']], dtype=torch.int64).cuda()
        yield x, y, names


def _predict(model, df, args):
    """-> (truth, predictions, photo names) over df in order"""
    model.eval()
    truth, pred, files = [], [], []
    with torch.no_grad():
        for x, y, names in _batches(df, args.image_dir, args.eval_batch_size, np.arange(len(df))):
            pred.extend(np.argmax(model(x).float().cpu().numpy(), axis=-1).tolist())
            truth.extend(y.cpu().numpy().tolist())
            files.extend(names)
    return truth, pred, files


def _per_class_accuracy(truth, pred):
    """confusion_matrix(...).diagonal() / row sums with NaN -> 0 (run_roi_categories.py:213-215) = per-class recall"""
    return CAT.precision_recall_fscore_support(truth, pred, labels=list(range(len(ASPECT))))[1]


def train(args, logger):
    if args.roi_label_path is None:
        raise ValueError("Please provide annotated RoI file.")
    train_data, dev_data, test_data = prepare_roi_data_correctly(args.roi_label_path, seed=18)
    logger.info("ROIs: train %d, dev %d, test %d", len(train_data), len(dev_data), len(test_data))
    model = CAT.make_model(CAT.MyRoIModel, len(ASPECT), args.resnet_checkpoint).cuda()
    optimizer = FusedAdamW(model.parameters(), lr=args.learning_rate, weight_decay=0.0)      # torch.optim.Adam
    gen = torch.Generator().manual_seed(args.seed)
    ckpt = f'{args.output_dir}/seed_{args.seed}_roi_model.pth'
    max_accuracy = 0.0
    logger.info("*************** Running training ***************")
    for epoch in range(int(args.num_train_epochs)):
        model.train()
        order = torch.randperm(len(train_data), generator=gen).numpy()
        for x, y, _ in _batches(train_data, args.image_dir, args.train_batch_size, order, flip_gen=gen):
            loss = ops.cross_entropy(model(x), y)
            loss.backward()
            optimizer.step()
            optimizer.zero_grad()
        logger.info("***** Running evaluation on Dev Set*****")
        truth, pred, _ = _predict(model, dev_data, args)
        all_accuracy = float(np.mean(_per_class_accuracy(truth, pred)))
        if all_accuracy >= max_accuracy:
            CAT.save_model(ckpt, model, epoch)
            max_accuracy = all_accuracy
            logger.info(f"New Best Accuracy: {max_accuracy:.4f}")

    logger.info("***** Running evaluation on Test Set *****")
    model.load_state_dict(CAT.load_model(ckpt)['model_state_dict'])
    truth, pred, files = _predict(model, test_data, args)
    results_map = defaultdict(lambda: {"gold": [], "pred": []})
    for f, t, p in zip(files, truth, pred):
        results_map[f]["gold"].append(ASPECT[t])
        results_map[f]["pred"].append(ASPECT[p])
    _, _, f1, _ = CAT.precision_recall_fscore_support(truth, pred, labels=list(range(len(ASPECT))))
    acc = _per_class_accuracy(truth, pred)
    with open(os.path.join(args.output_dir, "test_roi_results.txt"), "w") as writer:
        writer.write("***** TEST RESULTS (ROI Categories) *****\n")
        for a in range(len(ASPECT)):
            writer.write(f"{ASPECT[a]:<20} | F1: {f1[a]:.4f} | Acc: {acc[a]:.4f}\n")
    detail = os.path.join(args.output_dir, "test_roi_predictions_detail.txt")
    ordered = test_data['file_name'].unique()
    with open(detail, "w", encoding='utf-8') as f:
        for name in ordered:
            key = name + ".png"
            if key in results_map:
                content = results_map[key]
                f.write(f'"{key}": [\n')
                f.write(f'    Gold_Label: {json.dumps(sorted(content["gold"]), ensure_ascii=False)},\n')
                f.write(f'    Prediction: {json.dumps(sorted(content["pred"]), ensure_ascii=False)},\n')
                f.write('  ],\n')
    logger.info(f"Saved detailed predictions (Quantity: {len(ordered)}) to {detail}")


def get_cate(args, logger):
    print("===================== GET ROI CATEGORIES =====================")
    model = CAT.make_model(CAT.MyRoIModel, len(ASPECT), args.resnet_checkpoint).cuda()
    path = f'{args.output_dir}/seed_{args.seed}_roi_model.pth' if args.do_train else args.weight_path
    if path is None:
        raise ValueError("--get_cate without --do_train needs --weight_path")
    model.load_state_dict(CAT.load_model(path)['model_state_dict'])
    model.eval()
    roi_df = CAT.read_roi_labels(args.roi_label_path)
    names = list(roi_df['file_name'].unique())
    labels = {}
    bs = max(1, args.eval_batch_size)
    with torch.no_grad():
        for i in range(0, len(names), bs):
            batch = names[i:i + bs]
            photos = CAT.load_photos([os.path.join(args.image_dir, n + ".png") for n in batch])
            boxes = []
            for n in batch:
                rows = roi_df[roi_df['file_name'] == n][:NUM_ROI]
                boxes.append([(int(r.x1), int(r.x2), int(r.y1), int(r.y2)) for r in rows.itertuples()])
            keep = [k for k in range(len(batch)) if boxes[k]]
            preds = []
            if keep:
                x = crop_batch([photos[k] for k in keep], [boxes[k] for k in keep], dtype=ops.compute_dtype())
                preds = np.argmax(model(x).float().cpu().numpy(), axis=-1).tolist()
            pos = 0
            for k, n in enumerate(batch):
                got = preds[pos:pos + len(boxes[k])]
                pos += len(boxes[k])
                labels[n + ".png"] = sorted(set(ASPECT[p] for p in got))
    with open(f"{args.output_dir}/resnet152_roi_label.json", "w", encoding='utf-8') as f:
        json.dump(labels, f, indent=2, ensure_ascii=False)
    logger.info("wrote %d photo labels", len(labels))


def main(argv=None):
    args = build_parser().parse_args(argv)
    print("===================== RUN ROI CATEGORIES =====================")
    os.makedirs(args.output_dir, exist_ok=True)
    logger = logging.getLogger("run_roi_categories")
    logger.setLevel(logging.INFO)
    for h in list(logger.handlers):
        logger.removeHandler(h)
        h.close()
    fmt = logging.Formatter('%(asctime)s - %(levelname)s - %(name)s - %(message)s', datefmt='%m/%d/%Y %H:%M:%S')
    for h in (logging.FileHandler(f'{args.output_dir}/roi_categories.log', mode='w'), logging.StreamHandler(sys.stdout)):
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
