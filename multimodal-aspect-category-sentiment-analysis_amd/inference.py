"""Aspect polarities for unlabeled hotel reviews on the MI355X: the reference's inference.py on `fcmf_framework.predict.Predictor`.

    python inference.py --base_path_model CKPT_DIR --text "..." --image_list a.png b.png --detections dets.json \\
        --image_category_checkpoint img.pth --roi_category_checkpoint roi.pth [--output_file out.txt]
    python inference.py --base_path_model CKPT_DIR --reviews reviews.jsonl --batch_size 8 --output_file out.jsonl ...

The reference's flags are kept.  What it does that this build does not: it runs a YOLO detector (ultralytics) over every photo
and normalises the Vietnamese text (underthesea, text_preprocess.py).  Here the detector's output is an input -- `--detections`
names a JSON file {photo path: [{"category": str, "coordinates": [left, top, right, bottom]}, ...]} (or a list with one entry per
photo of --image_list) -- and the text is taken as given (`Predictor(normalize=...)` is the hook).

Checkpoints: CKPT_DIR/seed_42_fcmf_model_best.pth, loaded directly and, if keys are missing, through the reference's renames of
old checkpoints; the two extractors saved beside it (seed_42_resimg_model_best.pth, seed_42_resroi_model_best.pth) go into the
FEATURE trunks, strictly (`train_harness.load_resnets`).  The category classifiers have files of their own
(--image_category_checkpoint / --roi_category_checkpoint, written by image_processing/run_*_categories.py).

--reviews: batch mode, one JSON object per line in ({"text", "photos", "detections": one list per photo, "tags": optional
[photo tags, ROI tags]}) and one per line out ({"text", "polarities", "logits"}).  There is no CPU path.
"""
import argparse
import json
import logging
import os
import sys

import torch

from fcmf_framework import ops
from fcmf_framework.predict import ASPECTS, Predictor, load_fcmf_state, write_result

logger = logging.getLogger("fcmf.inference")
SEED = 42      # the reference's checkpoint names: seed_42_*_model_best.pth


def build_parser():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    # the reference's flags: names, aliases, types and defaults are the interface (inference.py:333-371)
    p.add_argument("--base_path_model", type=str, required=True,
                   help="directory that holds seed_42_fcmf_model_best.pth and the resimg / resroi companions")
    p.add_argument("--text", type=str, default=None, help="the review (one-review mode; excludes --reviews)")
    p.add_argument("--image_list", "--names-list", nargs='+', help="the review's photo files, in order")
    p.add_argument("--num_images", type=int, default=7, help="photo slots per review the model was trained with")
    p.add_argument("--num_rois", type=int, default=4, help="ROI slots per photo the model was trained with")
    p.add_argument("--pretrained_model", type=str, default='xlm-roberta-base', help="tokenizer / text encoder name or local directory")
    p.add_argument("--output_file", type=str, default=None, help="write the result here (text layout; JSON lines in batch mode)")
    # this build's
    p.add_argument("--detections", type=str, default=None, help="JSON file with the detector's boxes per photo")
    p.add_argument("--image_category_checkpoint", type=str, default=None, help="photo category classifier (run_image_categories.py)")
    p.add_argument("--roi_category_checkpoint", type=str, default=None, help="ROI category classifier (run_roi_categories.py)")
    p.add_argument("--resnet_checkpoint", type=str, default=None, help="local torchvision ResNet-152 state dict the trunks start from")
    p.add_argument("--bf16", action="store_true", help="bf16 compute (MFMA kernels)")
    p.add_argument("--no_fold_bn", action="store_true", help="run the trunks through trunk_nhwc instead of the folded eval trunk")
    p.add_argument("--reference_pooling", action="store_true", help="pool photos to 1x1 before the 7x7 map, as the reference's inference.py does")
    p.add_argument("--reviews", type=str, default=None, help="batch mode: a .jsonl file, one review per line")
    p.add_argument("--batch_size", type=int, default=8, help="reviews per forward pass in batch mode")
    return p


def parse_args(argv=None):
    p = build_parser()
    args = p.parse_args(argv)
    if args.reviews is not None and args.text is not None:
        p.error("--reviews (batch mode) and --text (one review) exclude each other")
    if args.reviews is None and args.text is None:
        p.error("one of --text and --reviews is required")
    if args.batch_size < 1:
        p.error("--batch_size must be positive")
    return args


def load_detections(path, image_list):
    """-> one detection list per photo of image_list: the file is {photo path or base name: [...]} or a list in image_list's order"""
    if path is None:
        return [[] for _ in image_list]
    with open(path, encoding="utf-8") as f:
        data = json.load(f)
    if isinstance(data, list):
        if len(data) != len(image_list):
            raise ValueError(f"{path}: {len(data)} detection lists for {len(image_list)} photos")
        return data
    return [data.get(p, data.get(os.path.basename(p), [])) for p in image_list]


def read_reviews(path):
    out = []
    with open(path, encoding="utf-8") as f:
        for line in f:
            if line.strip():
                r = json.loads(line)
                r.setdefault("photos", r.pop("image_list", []))
                out.append(r)
    return out


def write_jsonl(f, reviews, polarities, logits):
    for rev, pol, lg in zip(reviews, polarities, logits.tolist()):
        f.write(json.dumps({"text": rev["text"], "polarities": pol, "logits": lg}, ensure_ascii=False) + "\n")


def build_predictor(args, device, tokenizer=None, model=None, make_trunk=None, **predictor_kw):
    """models loaded once: FCMF + its two extractor companions, and the two category classifiers when their checkpoints are given.
    tokenizer / model / make_trunk default to what the flags name (AutoTokenizer, FCMF(--pretrained_model), ResNet-152);
    predictor_kw goes to Predictor (seq_len, image_loader, normalize, drop_categories, ...)"""
    from fcmf_framework import categories as C
    from fcmf_framework.fcmf_multimodal import FCMF
    from fcmf_framework.resnet import resnet152
    from train_harness import build_extractors, load_resnets
    if tokenizer is None:
        from transformers import AutoTokenizer
        tokenizer = AutoTokenizer.from_pretrained(args.pretrained_model)
    if model is None:
        model = FCMF(args.pretrained_model, num_imgs=args.num_images, num_roi=args.num_rois)
        model.encoder.bert.cell.resize_token_embeddings(len(tokenizer))
    model = model.to(device)
    path = os.path.join(args.base_path_model, f"seed_{SEED}_fcmf_model_best.pth")
    if not os.path.exists(path):
        raise FileNotFoundError(f"FCMF model not found at {path}")
    missing, unexpected, renamed = load_fcmf_state(model, torch.load(path, map_location=device, weights_only=True)["model_state_dict"])
    logger.info("FCMF checkpoint %s loaded%s", path, " through the old-key renames" if renamed else "")
    if missing or unexpected:
        logger.warning("FCMF checkpoint: %d missing keys %s, %d unexpected keys %s", len(missing), missing[:3], len(unexpected), unexpected[:3])

    def trunk():
        if args.resnet_checkpoint:
            return resnet152(weights=torch.load(args.resnet_checkpoint, map_location="cpu", weights_only=True))
        return resnet152()
    img, roi = build_extractors(make_trunk or trunk, False, device)
    loaded = load_resnets(path, img, roi, device, logger, old="fcmf", strict=True)
    if len(loaded) < 2:
        logger.warning("extractor checkpoints beside %s: found %d of 2; the others keep their initial weights", path, len(loaded))
    classifiers = []
    for cls, ck in ((C.MyImgModel, args.image_category_checkpoint), (C.MyRoIModel, args.roi_category_checkpoint)):
        if ck is None:
            classifiers.append(None)
            continue
        m = cls(len(C.IMAGE_ASPECTS), (make_trunk or trunk)())
        m.load_state_dict(C.load_model(ck)["model_state_dict"])
        classifiers.append(m.to(device).eval())
    return Predictor(model, tokenizer, img, roi, classifiers[0], classifiers[1], num_imgs=args.num_images, num_rois=args.num_rois,
                     fold_bn=not args.no_fold_bn, reference_pooling=args.reference_pooling, **predictor_kw)


def run(args, predictor):
    if args.reviews is not None:
        reviews = read_reviews(args.reviews)
        polarities, logits = predictor.predict(reviews, batch_size=args.batch_size)
        if args.output_file:
            with open(args.output_file, "w", encoding="utf-8") as f:
                write_jsonl(f, reviews, polarities, logits)
        else:
            write_jsonl(sys.stdout, reviews, polarities, logits)
        return polarities
    images = list(args.image_list or [])
    review = {"text": args.text, "photos": images, "detections": load_detections(args.detections, images)}
    (result,), _ = predictor.predict([review], batch_size=1)
    print(result)
    if args.output_file:
        write_result(args.output_file, args.text, images, result)
        logger.info("Results saved to: %s", args.output_file)
    return result


def main(argv=None):
    args = parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(levelname)s %(message)s")
    if not torch.cuda.is_available():
        raise SystemExit("inference.py (MI355X build) has no CPU path: a ROCm GPU is required")
    device = torch.device("cuda", torch.cuda.current_device())
    ops.set_compute_dtype(torch.bfloat16 if args.bf16 else torch.float32)
    logger.info("Using %d images and %d RoIs; %s for text features extraction.", args.num_images, args.num_rois, args.pretrained_model)
    logger.info("the text is taken as given: the reference's Vietnamese normalisation (underthesea) is not part of this build")
    return run(args, build_predictor(args, device))


if __name__ == "__main__":
    main()
