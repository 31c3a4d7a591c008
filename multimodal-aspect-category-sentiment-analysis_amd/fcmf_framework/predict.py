"""Aspect polarities for unlabeled hotel reviews (reference inference.py + fcmf_framework/image_process.py, behaviour restated).

One review = its text, its photos (paths or decoded uint8 arrays), per photo the detector's output
`[{"category": str, "coordinates": [left, top, right, bottom]}, ...]` (image_process.py:115-142) and, optionally, ready-made tags.
The detector itself (ultralytics) and the Vietnamese text normalisation (underthesea, text_preprocess.py) are not part of this
build: detections come from the caller (a JSON file, a callable), `normalize=` is the hook for the text.

`Predictor.predict` runs, per batch of reviews:
  1. box merging per photo (`merge_boxes`: greedy, in detection order, per category -- image_process.py:69-113);
  2. ONE `image_ops.crop_batch` call for the photos and ONE for the ROI crops: photo rows top:bottom, columns left:right, boxes
     [top, bottom, left, right] / 512 clipped to [0, 1], at most `num_rois` per photo, zero crops / zero boxes as padding -- the
     tensors `review_batches.ReviewProducer.pixels` yields for the same photos and boxes (image_process.py:229-317);
  3. tags: photo categories with sigmoid > `image_threshold`, ROI categories = argmax per merged box, unions over the review's
     first `num_imgs` photos, SORTED as `ReviewProducer.visual_tags` sorts them (the reference iterates a Python set, whose order
     is undefined; sorting is what training saw), ['empty'] when none;
  4. the six-aspect prompt of `ReviewProducer.encode`, unchanged;
  5. features as in training: photos -> `img_trunk` -> 7 x 7 patch map [49, 2048]; ROI crops -> `roi_trunk` -> global mean [2048]
     (`reference_pooling=True`: the photo is pooled to 1 x 1 first, inference.py:263-265, so its 49 tokens all equal the mean);
     padding slots hold the features of a zero crop, as they do in training, computed once per batch;
  6. `model.forward_aspects` on [R, 6, S] for the R reviews of the batch at once, argmax over the four polarities.
The trunks run through `resnet_eval.FoldedTrunk` (`fold_bn=True`) or `ResNet.trunk_nhwc` as it stands (`fold_bn=False`).
There is no CPU path.
"""
import os

import numpy as np
import torch

from . import _hip as H
from . import image_ops, ops
from . import resnet as R
from .categories import IMAGE_ASPECTS, ROI_ASPECTS

ASPECTS = ['Location', 'Food', 'Room', 'Facilities', 'Service', 'Public_area']
POLARITIES = ['None', 'Negative', 'Neutral', 'Positive']
PATCHES = 49


# ---- box merging (image_process.py:69-113) --------------------------------------------------------------------------------------
def _nearby(a, b, eps):
    return all(abs(p - q) <= eps for p, q in zip(a, b))


def merge_boxes(boxes, eps):
    """detections in detector order -> [(key, [left, top, right, bottom])] in the order the entries first appear.  The first box of
    a category is that category's merged box (key = the category); a later box of the category whose four coordinates each lie
    within `eps` of the CURRENT merged box widens it (min of the low corners, max of the high ones); any other box is an entry of
    its own, keyed `<category>_<n>` with n counting every non-first box of any category so far, and never merges again."""
    order, merged, n = [], {}, 1
    for box in boxes:
        cat, c = box["category"], list(box["coordinates"])
        if cat not in merged:
            merged[cat] = c
            order.append(cat)
            continue
        cur = merged[cat]
        if _nearby(cur, c, eps):
            merged[cat] = [min(cur[0], c[0]), min(cur[1], c[1]), max(cur[2], c[2]), max(cur[3], c[3])]
        else:
            key = f"{cat}_{n}"
            if key not in merged:
                order.append(key)
            merged[key] = c
        n += 1
    return [(k, merged[k]) for k in order]


def crop_boxes(detections, eps, drop_categories=()):
    """one photo's detections -> its merged boxes as ReviewProducer-style crop boxes (x1, x2, y1, y2) = (top, bottom, left, right),
    x = rows.  Negative coordinates are clamped to 0 (a detector emits none)."""
    kept = [d for d in (detections or []) if d["category"] not in drop_categories]
    out = []
    for _, (left, top, right, bottom) in merge_boxes(kept, eps):
        out.append(tuple(max(0, int(v)) for v in (top, bottom, left, right)))
    return out


# ---- checkpoints ----------------------------------------------------------------------------------------------------------------
def rename_old_keys(state_dict):
    """the renames inference.py:175-189 applies to checkpoints written by older code: ent2img / ent2roi -> text2img / text2roi,
    comb_attention -> mm_attention, the pooler and classifier out of `encoder.`, everything else under `encoder.`"""
    out = {}
    for k, v in state_dict.items():
        k = k.replace("ent2img", "text2img").replace("ent2roi", "text2roi").replace("comb_attention", "mm_attention")
        if k.startswith("encoder.text_pooler.") or k.startswith("encoder.classifier."):
            k = k[len("encoder."):]
        if not k.startswith(("encoder.", "decoder.", "text_pooler.", "classifier.")):
            k = "encoder." + k
        out[k] = v
    return out


def load_fcmf_state(model, state_dict):
    """directly first; if keys are missing, once more through `rename_old_keys` -> (missing, unexpected, renamed?)"""
    res = model.load_state_dict(state_dict, strict=False)
    renamed = False
    if res.missing_keys:
        res = model.load_state_dict(rename_old_keys(state_dict), strict=False)
        renamed = True
    ops.shadows.clear()
    return list(res.missing_keys), list(res.unexpected_keys), renamed


# ---- output layout (inference.py:426-437) ---------------------------------------------------------------------------------------
def format_result(text, image_list, result):
    """the text of the reference's result file: a header (the text, the photo count, the photo names when there are any), a ruled
    "PREDICTIONS:" banner between blank lines, one "<aspect>: <polarity>" line per aspect"""
    rule = "=" * 50
    header = ["Text: " + str(text), "Number of images: %d" % len(image_list)]
    if image_list:
        header.append("Images: " + ", ".join(image_list))
    body = ["%s: %s" % pair for pair in result.items()]
    return "\n".join(header + ["", rule, "PREDICTIONS:", rule, ""] + body) + "\n"


def write_result(path, text, image_list, result):
    with open(path, "w", encoding="utf-8") as f:
        f.write(format_result(text, image_list, result))


# ---- the predictor --------------------------------------------------------------------------------------------------------------
def _trunk_of(m):
    """a resnet.ResNet, or the myResNetImg / myResNetRoI wrapper that holds one"""
    return m if isinstance(m, R.ResNet) else R.from_module(getattr(m, "resnet", m))


def tags_from_outputs(image_logits, photo_of_image, roi_logits, photo_of_roi, n_reviews, review_of_photo, image_threshold=0.6):
    """classifier outputs of a batch -> per review (photo tags, ROI tags), sorted, ['empty'] when none.  image_logits [P, 5] one row
    per photo, roi_logits [Q, 5] one row per merged box; photo_of_* give each row's photo, review_of_photo each photo's review"""
    img = [set() for _ in range(n_reviews)]
    roi = [set() for _ in range(n_reviews)]
    if len(photo_of_image):
        on = torch.sigmoid(torch.as_tensor(image_logits).float()) > image_threshold
        for row, p in enumerate(photo_of_image):
            img[review_of_photo[p]].update(IMAGE_ASPECTS[j] for j in on[row].nonzero().flatten().tolist())
    if len(photo_of_roi):
        best = torch.as_tensor(roi_logits).float().argmax(-1).tolist()
        for row, p in enumerate(photo_of_roi):
            roi[review_of_photo[p]].add(ROI_ASPECTS[best[row]])
    return [((sorted(a) or ['empty']), (sorted(b) or ['empty'])) for a, b in zip(img, roi)]


class Predictor:
    def __init__(self, model, tokenizer, img_trunk, roi_trunk, image_classifier=None, roi_classifier=None, *, num_imgs=7, num_rois=4,
                 seq_len=170, fold_bn=True, reference_pooling=False, eps=30, image_threshold=0.6, drop_categories=(),
                 image_loader=None, normalize=None, crop_size=224):
        from review_batches import ReviewProducer, default_image_loader
        self.model = model.eval()
        self.num_imgs, self.num_rois, self.seq_len, self.size = num_imgs, num_rois, int(seq_len), crop_size
        self.fold_bn, self.reference_pooling = bool(fold_bn), bool(reference_pooling)
        self.eps, self.image_threshold, self.drop_categories = eps, image_threshold, frozenset(drop_categories)
        self.load, self.normalize = image_loader or default_image_loader, normalize
        self.producer = ReviewProducer(tokenizer, "", None, {}, {}, num_imgs, num_rois, seq_len=seq_len)
        self.device = next(model.parameters()).device
        self.classifiers = {"image_cls": image_classifier, "roi_cls": roi_classifier}      # (keys of self.nets too)
        for m in (image_classifier, roi_classifier):
            if m is not None:
                m.eval()
        nets = {"img": _trunk_of(img_trunk).eval(), "roi": _trunk_of(roi_trunk).eval()}
        for k, m in self.classifiers.items():
            if m is not None:
                nets[k] = m.feature_extractor
        self.nets, self.folded = nets, {}      # folded: one FoldedTrunk per network, snapshotted at its first use

    def refresh(self):
        """after the trunks' or classifiers' parameters changed (fold_bn: the snapshots are explicit)"""
        for f in self.folded.values():
            f.refresh()

    # ---- trunks ---------------------------------------------------------------------------------------------------------
    def _trunk(self, which, x):
        """x [n, 3, S, S] -> NHWC [n, h, w, C], eval mode, detached"""
        if self.fold_bn:
            if which not in self.folded:
                from .resnet_eval import FoldedTrunk
                self.folded[which] = FoldedTrunk(self.nets[which])
            return self.folded[which](x)
        net = self.nets[which]
        with torch.no_grad():
            outs = [net.trunk_nhwc(x[i:i + R.MAX_CROPS_PER_PASS]) for i in range(0, x.shape[0], R.MAX_CROPS_PER_PASS)]
        return outs[0] if len(outs) == 1 else torch.cat(outs, 0)

    def _classify(self, which, x):
        """the category model's own head on this predictor's trunk path"""
        with torch.no_grad():
            return self.classifiers[which].head(self._trunk(which, x)).float()

    # ---- one batch ------------------------------------------------------------------------------------------------------
    def _photos(self, review):
        """-> [(decoded photo or None when unreadable, its merged crop boxes)] of the review's first num_imgs photos"""
        photos = list(review.get("photos") or [])[:self.num_imgs]
        dets = review.get("detections") or []          # one list per photo, or a detector: callable(photo as given) -> list
        out = []
        for i, ph in enumerate(photos):
            found = dets(ph) if callable(dets) else dets[i] if i < len(dets) else []
            if isinstance(ph, (str, os.PathLike)):
                try:
                    ph = self.load(os.fspath(ph))
                except (OSError, RuntimeError, ValueError):
                    ph = None
            boxes = crop_boxes(found, self.eps, self.drop_categories)
            out.append((ph, boxes))
        return out

    def pixels(self, reviews):
        """-> (t_img [R, NI, 3, S, S], roi_img [R, NI, NR, 3, S, S], roi_coors [R, NI, NR, 4]) float32 on the device, and the crops
        of ALL merged boxes with their (review, photo) -- what the ROI classifier sees"""
        NI, NR, S, dev = self.num_imgs, self.num_rois, self.size, self.device
        n = len(reviews)
        t_img = torch.zeros((n, NI, 3, S, S), device=dev)
        roi_img = torch.zeros((n, NI, NR, 3, S, S), device=dev)
        coors = torch.zeros((n, NI, NR, 4), dtype=torch.float64)
        whole, whole_at, srcs, boxes, box_at = [], [], [], [], []
        for r, rev in enumerate(reviews):
            for i, (ph, bl) in enumerate(self._photos(rev)):
                if ph is not None:
                    whole.append(ph)
                    whole_at.append((r, i))
                else:       # unreadable: a zero image, and crops of a zero photo (ReviewProducer.pixels)
                    ph = np.zeros((S, S, 3), dtype=np.uint8)
                hh, ww = (ph.shape[1], ph.shape[2]) if torch.is_tensor(ph) else (ph.shape[0], ph.shape[1])
                live = []
                for k, (x1, x2, y1, y2) in enumerate(bl):
                    if k < NR:
                        coors[r, i, k] = torch.tensor(np.clip(np.array([x1, x2, y1, y2]) / 512.0, 0.0, 1.0))
                    if min(x2, hh) - x1 > 0 and min(y2, ww) - y1 > 0:          # (an empty crop stays a zero crop)
                        live.append((x1, x2, y1, y2))
                        box_at.append((r, i, k))
                if live:
                    srcs.append(ph)
                    boxes.append(live)
        if whole:
            x = image_ops.crop_batch(whole, size=S, device=dev)
            ri, ii = (torch.tensor(v, device=dev) for v in zip(*whole_at))
            t_img[ri, ii] = x
        crops = image_ops.crop_batch(srcs, boxes, size=S, device=dev) if srcs else torch.zeros((0, 3, S, S), device=dev)
        keep = [j for j, (_, _, k) in enumerate(box_at) if k < NR]
        if keep:
            ri, ii, ki = (torch.tensor(v, device=dev) for v in zip(*[box_at[j] for j in keep]))
            roi_img[ri, ii, ki] = crops[torch.tensor(keep, device=dev)]
        return t_img, roi_img, coors.float().to(dev), (whole_at, crops, box_at)

    def tags(self, reviews, t_img, extra):
        """per review (photo tags, ROI tags): the review's own `tags` when given, else the two classifiers' predictions"""
        need = [r for r, rev in enumerate(reviews) if rev.get("tags") is None]
        out = [None] * len(reviews)
        for r, rev in enumerate(reviews):
            if rev.get("tags") is not None:
                a, b = rev["tags"]
                out[r] = ((sorted(set(a)) or ['empty']), (sorted(set(b)) or ['empty']))
        if need:
            if self.classifiers["image_cls"] is None or self.classifiers["roi_cls"] is None:
                raise H.HipLibraryError("Predictor: a review without ready-made tags needs the image and ROI category classifiers")
            whole_at, crops, box_at = extra
            wanted = set(need)
            pi = [j for j, (r, _) in enumerate(whole_at) if r in wanted]
            qi = [j for j, (r, _, _) in enumerate(box_at) if r in wanted]
            index = lambda v: torch.tensor(v, device=self.device)
            il = self._classify("image_cls", t_img[tuple(index(v) for v in zip(*[whole_at[j] for j in pi]))]) if pi else []
            rl = self._classify("roi_cls", crops[index(qi)]) if qi else []
            photos = sorted({(r, i) for r, i in whole_at} | {(r, i) for r, i, _ in box_at})
            pid = {p: n for n, p in enumerate(photos)}
            got = tags_from_outputs(il.cpu() if pi else il, [pid[whole_at[j]] for j in pi], rl.cpu() if qi else rl,
                                    [pid[box_at[j][:2]] for j in qi], len(reviews), [r for r, _ in photos], self.image_threshold)
            for r in need:
                out[r] = got[r]
        return out

    def prompts(self, reviews, tags):
        """-> input_ids, token_type_ids, attention_mask [R, 6, S], added mask [R, 6, S + 49] (long, on the device)"""
        cols = [[], [], [], []]
        for rev, tg in zip(reviews, tags):
            text = rev["text"] if self.normalize is None else self.normalize(rev["text"])
            enc = [self.producer.encode(a, text, tg) for a in ASPECTS]
            for c, vals in zip(cols, zip(*enc)):
                c.append(torch.stack(vals))
        return tuple(torch.stack(c).to(self.device) for c in cols)

    def features(self, t_img, roi_img):
        """pixel tensors -> (vis [R, NI, 49, 2048], roi [R, NI, NR, 2048]) float32.  Slots that hold no crop get the features of ONE
        zero crop per trunk (the trunk is a per-crop function in eval mode: what training computed for each of them)"""
        n, NI, NR = t_img.shape[0], self.num_imgs, self.num_rois
        zero = torch.zeros((1, *t_img.shape[2:]), device=self.device)

        def run(which, flat, pool):
            live = flat.flatten(1).any(1)
            idx = live.nonzero().flatten()
            f = pool(self._trunk(which, torch.cat((zero, flat[idx]), 0)))
            out = f[:1].expand(flat.shape[0], *f.shape[1:]).clone()
            out[idx] = f[1:]
            return out

        def pool_img(y):
            if self.reference_pooling:
                return R.adaptive_avgpool_nhwc(y, 1, 1).flatten(1)[:, None, :].expand(-1, PATCHES, -1).contiguous()
            return R.adaptive_avgpool_nhwc(y, 7, 7, tokens=True)
        vis = run("img", t_img.flatten(0, 1), pool_img)
        roi = run("roi", roi_img.flatten(0, 2), lambda y: R.adaptive_avgpool_nhwc(y, 1, 1).flatten(1))
        return vis.view(n, NI, PATCHES, -1), roi.view(n, NI, NR, -1)

    @torch.no_grad()
    def predict_batch(self, reviews):
        H.require_cuda(next(self.model.parameters()))
        t_img, roi_img, coors, extra = self.pixels(reviews)
        tags = self.tags(reviews, t_img, extra)
        ids, tts, ams, added = self.prompts(reviews, tags)
        vis, roi = self.features(t_img, roi_img)
        logits = self.model.forward_aspects(input_ids=ids, token_type_ids=tts, attention_mask=ams, added_attention_mask=added,
                                            visual_embeds_att=vis, roi_embeds_att=roi, roi_coors=coors)
        return logits.float().cpu()

    def predict(self, reviews, batch_size=8):
        """reviews: dicts with "text", "photos" (paths or uint8 arrays), "detections" (one list per photo), optionally "tags" =
        (photo tags, ROI tags) -> ([{aspect: polarity}] per review, logits [n, 6, 4] float32 on the host)"""
        reviews = list(reviews)
        self.model.eval()
        outs = [self.predict_batch(reviews[i:i + batch_size]) for i in range(0, len(reviews), batch_size)]
        logits = torch.cat(outs, 0) if outs else torch.zeros((0, len(ASPECTS), len(POLARITIES)))
        best = logits.argmax(-1).tolist()
        return [{a: POLARITIES[p] for a, p in zip(ASPECTS, row)} for row in best], logits
