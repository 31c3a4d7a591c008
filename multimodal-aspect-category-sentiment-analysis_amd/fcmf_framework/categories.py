"""Photo and ROI category classifiers (reference image_processing/run_image_categories.py, run_roi_categories.py) on the HIP
ResNet-152 trunk, and the host-side pieces their drivers need without torchvision / sklearn / openpyxl.

  * `MyImgModel` / `MyRoIModel`: the reference's modules (run_image_categories.py:51-60, run_roi_categories.py:55-64) with the
    same state-dict keys -- `feature_extractor.*` (its unused 1000-way `fc` included), `no_fc.{0,1,4..7}.*` aliasing the same
    modules, `linear.*` -- so checkpoints move both ways; a checkpoint saved under nn.DataParallel (`module.` prefix) loads too.
    The forward is trunk -> global average pool -> linear on the kernels (`trunk_nhwc`, `AvgPoolFn`, `ops.linear`); the `no_fc`
    Sequential exists for its keys and is never called module by module.
  * `load_photo`: PIL when importable, else torchvision.io, else a clear error.
  * `read_image_labels` / `read_roi_labels`: the reference's label files (.xlsx needs openpyxl; .csv with the same columns).
  * `train_test_split`: sklearn.model_selection.train_test_split(X, test_size, random_state) restated (ShuffleSplit's
    permutation of numpy's RandomState), so the splits are the reference's.
  * `precision_recall_fscore_support` / `accuracy_score`: the sklearn metrics the drivers use, restated (zero_division = 0,
    a fixed label list).
"""
import importlib.util
import math
import os

import numpy as np
import torch
import torch.nn as nn

from . import _hip as H
from . import ops
from . import resnet as R

IMAGE_ASPECTS = ['Food', 'Room', 'Facilities', 'Service', 'Public_area']        # run_image_categories.py:145
ROI_ASPECTS = ['food', 'room', 'facilities', 'service', 'public_area']          # run_roi_categories.py:157


class _CategoryModel(nn.Module):
    def __init__(self, num_classes, resnet=None):
        super().__init__()
        self.feature_extractor = resnet if resnet is not None else R.resnet152()
        self.no_fc = nn.Sequential(*(list(self.feature_extractor.children())[:-1]))
        self.linear = nn.Linear(self.feature_extractor.fc.in_features, num_classes)

    def forward(self, x):
        """x [N, 3, H, W] crops -> logits [N, num_classes] in the compute dtype.  train(): the trunk is fine-tuned with batch
        statistics (TrunkFn); eval(): running statistics, forward only"""
        return self.head(self.feature_extractor.trunk_nhwc(x, fine_tune=self.training))

    def head(self, feat):
        """trunk output NHWC [N, h, w, C] -> logits: global average pool + linear (also fed by predict.Predictor's eval trunks)"""
        if feat.requires_grad:
            pooled = R.AvgPoolFn.apply(feat, 1, 1, False)
        else:
            pooled = R.adaptive_avgpool_nhwc(feat, 1, 1)
        f = ops.cast_ad(pooled.flatten(1), ops.compute_dtype())
        return ops.linear(f, self.linear.weight, self.linear.bias)

    def load_state_dict(self, state_dict, strict=True, **kw):
        """also takes a checkpoint written under nn.DataParallel (every key prefixed `module.`)"""
        if len(state_dict) and all(k.startswith("module.") for k in state_dict):
            state_dict = {k[len("module."):]: v for k, v in state_dict.items()}
        return super().load_state_dict(state_dict, strict=strict, **kw)


class MyImgModel(_CategoryModel):
    """multi-label photo categories (run_image_categories.py:51-60): BCE-with-logits head"""


class MyRoIModel(_CategoryModel):
    """single-label ROI categories (run_roi_categories.py:55-64): cross-entropy head"""


# ---- photos ---------------------------------------------------------------------------------------------------------
def load_photo(path):
    """-> uint8 RGB photo: numpy [H, W, 3] through PIL, else a torch [3, H, W] tensor through torchvision.io"""
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        with Image.open(path) as im:
            return np.asarray(im.convert("RGB"))
    try:
        from torchvision.io import ImageReadMode, read_image
    except ImportError as e:
        raise RuntimeError("decoding photos needs PIL or torchvision.io; neither is importable") from e
    return read_image(path, mode=ImageReadMode.RGB)


_decoder = None


def load_photos(paths):
    """load_photo over a few threads (PIL's decoders release the GIL)"""
    global _decoder
    if _decoder is None:
        from concurrent.futures import ThreadPoolExecutor
        _decoder = ThreadPoolExecutor(8, thread_name_prefix="photo-decode")
    return list(_decoder.map(load_photo, paths))


# ---- label files ----------------------------------------------------------------------------------------------------
def _read_table(path):
    import pandas as pd
    ext = os.path.splitext(path)[1].lower()
    if ext in (".xlsx", ".xlsm", ".xls"):
        if importlib.util.find_spec("openpyxl") is None:
            raise RuntimeError(f"{path}: reading an Excel label file needs openpyxl, which is not installed; "
                               f"save the sheet as .csv (same columns) and pass that instead")
        return pd.read_excel(path)
    return pd.read_csv(path)


def read_image_labels(path):
    """run_image_categories.py:150-153: fillna(0), drop rows whose columns 1.. are all zero, renumber"""
    df = _read_table(path).fillna(0)
    df = df.loc[~(df.iloc[:, 1:] == 0).all(axis=1)]
    return df.reset_index(drop=True)


def read_roi_labels(path):
    import pandas as pd
    return pd.read_csv(path)


# ---- split and metrics (sklearn restated) ---------------------------------------------------------------------------
def split_indices(n, test_size, random_state=18):
    """-> (train indices, test indices) of sklearn's train_test_split(range(n), test_size=..., random_state=...) with a float
    test_size: n_test = ceil(test_size * n), permutation of RandomState(random_state); test first, train after it"""
    n_test = int(math.ceil(test_size * n))
    n_train = n - n_test
    if n_train <= 0 or n_test <= 0:
        raise ValueError(f"train_test_split: {n} samples cannot be split with test_size={test_size}")
    perm = np.random.RandomState(random_state).permutation(n)
    return perm[n_test:n_test + n_train], perm[:n_test]


def train_test_split(data, test_size, random_state=18):
    """a DataFrame or an array split as sklearn.model_selection.train_test_split(data, test_size, random_state) splits it"""
    tr, te = split_indices(len(data), test_size, random_state)
    if hasattr(data, "iloc"):
        return data.iloc[tr], data.iloc[te]
    a = np.asarray(data)
    return a[tr], a[te]


def precision_recall_fscore_support(y_true, y_pred, labels, average=None):
    """sklearn.metrics.precision_recall_fscore_support(..., labels=labels, zero_division=0, average=None | 'macro')"""
    t, p = np.asarray(y_true).reshape(-1), np.asarray(y_pred).reshape(-1)
    prec, rec, f1, sup = [], [], [], []
    for lab in labels:
        tp = float(np.sum((t == lab) & (p == lab)))
        ps, ts = float(np.sum(p == lab)), float(np.sum(t == lab))
        prec.append(tp / ps if ps else 0.0)
        rec.append(tp / ts if ts else 0.0)
        f1.append(2 * tp / (ts + ps) if (ts + ps) else 0.0)
        sup.append(int(ts))
    if average == "macro":
        return float(np.mean(prec)), float(np.mean(rec)), float(np.mean(f1)), None
    if average is not None:
        raise ValueError(f"average={average!r} is not restated")
    return np.array(prec), np.array(rec), np.array(f1), np.array(sup)


def accuracy_score(y_true, y_pred):
    t, p = np.asarray(y_true).reshape(-1), np.asarray(y_pred).reshape(-1)
    return float(np.mean(t == p)) if t.size else 0.0


def save_model(path, model, epoch):
    """run_image_categories.py:66-70"""
    torch.save({"epoch": epoch, "model_state_dict": model.state_dict()}, path)


def load_model(path):
    return torch.load(path, map_location=torch.device("cpu"), weights_only=False)


def make_model(cls, num_classes, resnet_checkpoint=None):
    """the reference starts from torchvision's IMAGENET1K_V2 weights: a local torchvision checkpoint (--resnet_checkpoint),
    else torchvision's cached weights if importable, else random initialisation -- nothing is downloaded"""
    if resnet_checkpoint:
        sd = torch.load(resnet_checkpoint, map_location="cpu", weights_only=True)
        layers = tuple(len({k.split(".")[1] for k in sd if k.startswith(f"layer{i}.")}) for i in range(1, 5))
        trunk = R.ResNet(layers, num_classes=sd["fc.weight"].shape[0] if "fc.weight" in sd else 1000)
        trunk.load_state_dict(sd, strict="fc.weight" in sd)
    else:
        try:
            from torchvision.models import ResNet152_Weights, resnet152 as tv_resnet152
            trunk = R.from_module(tv_resnet152(weights=ResNet152_Weights.IMAGENET1K_V2))
        except Exception:
            trunk = R.resnet152()
    return cls(num_classes, trunk)


def require_gpu():
    if not torch.cuda.is_available():
        raise H.HipLibraryError("the category classifiers run on the MI355X only (there is no CPU path)")
