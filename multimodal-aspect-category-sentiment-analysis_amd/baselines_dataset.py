"""BaselineDataset: the batch producer of the three comparison baselines, one tuple per review in the layouts of the
reference's training scripts, on review_batches.py (prompts, labels, photos / cached features):

  mroberta   (visual [NI,..], roi [NI,NR,..], input_ids [6,170], attention_mask [6,170], labels [6], text)
  tomroberta (visual, roi, target_ids [6,16], target_mask [6,16], sentence_ids [6,170], sentence_mask [6,170], labels [6], text)
  ef_captr   (input_ids [6,max_len], attention_mask [6,max_len], labels [6], text)

visual / roi are pixel crops, or with `feature_cache=` the precomputed ResNet-152 features [NI,49,2048] / [NI,NR,2048].
The tokenizer is passed in.  Frames have the columns comment, list_img, -, text_img_label (as MACSADataset reads them)."""
import torch

from review_batches import (ASPECTS, ReviewProducer, caption_pair, caption_string, polarity_labels, sentence_prompt,
                            target_prompt)

MODELS = ("mroberta", "tomroberta", "ef_captr")


class BaselineDataset(torch.utils.data.Dataset):
    def __init__(self, data, tokenizer, model, img_folder=None, roi_df=None, num_img=7, num_roi=4, image_loader=None,
                 feature_cache=None, caption_dict=None, max_len=256):
        if model not in MODELS:
            raise ValueError(f"model must be one of {MODELS}")
        self.data, self.tokenizer, self.model = data, tokenizer, model
        self.ASPECT = list(ASPECTS)
        self.num_img, self.max_len, self.captions = num_img, max_len, caption_dict or {}
        self.producer = None
        if model != "ef_captr":
            self.producer = ReviewProducer(tokenizer, img_folder, roi_df, {}, {}, num_img, num_roi, image_loader=image_loader,
                                           feature_cache=feature_cache, roi_dtype=torch.float64)

    def __len__(self):
        return self.data.shape[0]

    def __getitem__(self, idx):
        row = self.data.iloc[idx, :].values
        text, photos, annotations = row[0], row[1], row[3]
        labels = polarity_labels(annotations, self.ASPECT, first_wins=self.model != "ef_captr")
        stack = lambda pairs: tuple(torch.stack(t) for t in zip(*pairs))
        if self.model == "ef_captr":
            caps = caption_string(photos, self.captions, self.num_img)
            ids, mask = stack([caption_pair(self.tokenizer, a, text, caps, self.max_len) for a in self.ASPECT])
            return ids, mask, labels, text
        vis, roi, _ = self.producer.visual(idx, photos)
        sids, smask = stack([sentence_prompt(self.tokenizer, a, text) for a in self.ASPECT])
        if self.model == "mroberta":
            return vis, roi, sids, smask, labels, text
        tids, tmask = stack([target_prompt(self.tokenizer, a) for a in self.ASPECT])
        return vis, roi, tids, tmask, sids, smask, labels, text
