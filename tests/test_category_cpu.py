"""CPU-side checks of the photo / ROI category classifiers (image_processing/run_{image,roi}_categories.py): flags, the sklearn
restatements (split and metrics), the label-file readers, the model's state-dict keys and the crop descriptor's ABI mirror."""
import importlib.util
import os
import re
import sys

import numpy as np
import pytest

from conftest import PKG, ROOT

sys.path.insert(0, os.path.join(PKG, "image_processing"))


def _drivers():
    import run_image_categories as img
    import run_roi_categories as roi
    return img, roi


REF_FLAGS = ["--image_dir", "d", "--weight_path", "w.pth", "--output_dir", "o", "--do_train", "--get_cate",
             "--train_batch_size", "4", "--eval_batch_size", "2", "--learning_rate", "1e-4", "--num_train_epochs", "2",
             "--seed", "7", "--no_cuda"]


def test_parsers_take_the_reference_flags():
    img, roi = _drivers()
    a = img.build_parser().parse_args(REF_FLAGS + ["--image_label_path", "l.csv", "--resnet_checkpoint", "r.pth", "--bf16"])
    assert (a.image_dir, a.image_label_path, a.train_batch_size, a.eval_batch_size, a.learning_rate, a.num_train_epochs,
            a.seed, a.no_cuda, a.bf16, a.resnet_checkpoint) == ("d", "l.csv", 4, 2, 1e-4, 2.0, 7, True, True, "r.pth")
    b = roi.build_parser().parse_args(REF_FLAGS + ["--roi_label_path", "r.csv"])
    assert b.roi_label_path == "r.csv" and b.do_train and b.get_cate and not b.bf16
    # the reference's defaults
    d = img.build_parser().parse_args(["--image_dir", "x"])
    assert (d.output_dir, d.train_batch_size, d.eval_batch_size, d.learning_rate, d.num_train_epochs, d.seed, d.weight_path,
            d.image_label_path) == ("../vimacsa", 8, 8, 3e-5, 8.0, 42, None, None)


@pytest.mark.parametrize("which, argv", [("img", []), ("roi", ["--image_dir", "d"]), ("roi", ["--roi_label_path", "r.csv"])])
def test_parsers_reject_a_missing_required_flag(which, argv):
    img, roi = _drivers()
    with pytest.raises(SystemExit):
        (img if which == "img" else roi).build_parser().parse_args(argv)


def test_split_matches_hard_coded_indices():
    from fcmf_framework import categories as CAT
    # sklearn 1.7.2: train_test_split(np.arange(10), test_size=0.3, random_state=18)
    tr, te = CAT.split_indices(10, 0.3, 18)
    assert (tr.tolist(), te.tolist()) == ([4, 2, 1, 6, 5, 8, 3], [7, 9, 0])


@pytest.mark.parametrize("n", [3, 7, 10, 24, 101])
@pytest.mark.parametrize("test_size", [0.3, 0.5])
def test_split_equals_sklearn(n, test_size):
    sk = pytest.importorskip("sklearn.model_selection")
    import pandas as pd
    from fcmf_framework import categories as CAT
    df = pd.DataFrame({"file_name": [f"p{i}.png" for i in range(n)], "v": np.arange(n) * 3})
    a_tr, a_te = sk.train_test_split(df, test_size=test_size, random_state=18)
    b_tr, b_te = CAT.train_test_split(df, test_size=test_size, random_state=18)
    assert a_tr.index.tolist() == b_tr.index.tolist() and a_te.index.tolist() == b_te.index.tolist()
    names = df["file_name"].unique()
    u_tr, u_te = sk.train_test_split(names, test_size=test_size, random_state=18)
    v_tr, v_te = CAT.train_test_split(names, test_size=test_size, random_state=18)
    assert list(u_tr) == list(v_tr) and list(u_te) == list(v_te)


def test_metrics_equal_sklearn():
    skm = pytest.importorskip("sklearn.metrics")
    from fcmf_framework import categories as CAT
    rng = np.random.RandomState(3)
    for labels, n in (([0, 1], 40), ([0, 1, 2, 3, 4], 57), ([0, 1, 2, 3, 4], 5)):
        t = rng.randint(0, len(labels) - (1 if len(labels) > 2 else 0), n)       # some labels never true: zero_division
        p = rng.randint(0, len(labels), n)
        for avg in (None, "macro"):
            a = skm.precision_recall_fscore_support(t, p, labels=labels, zero_division=0.0, average=avg)
            b = CAT.precision_recall_fscore_support(t, p, labels=labels, average=avg)
            for x, y in zip(a[:3], b[:3]):
                np.testing.assert_allclose(np.asarray(y, dtype=float), np.asarray(x, dtype=float), rtol=1e-12, atol=1e-12)
            if avg is None:
                assert list(a[3]) == list(b[3])
        assert CAT.accuracy_score(t, p) == pytest.approx(skm.accuracy_score(t, p), abs=1e-15)
        # ROI accuracy: confusion_matrix diagonal / row sums with NaN -> 0 is the per-class recall
        cm = skm.confusion_matrix(t, p, labels=labels)
        with np.errstate(invalid="ignore", divide="ignore"):
            acc = np.nan_to_num(cm.diagonal() / cm.sum(axis=1))
        np.testing.assert_allclose(CAT.precision_recall_fscore_support(t, p, labels=labels)[1], acc, atol=1e-15)


def test_image_label_reader_filters_like_the_reference(tmp_path):
    from fcmf_framework import categories as CAT
    p = tmp_path / "labels.csv"
    p.write_text("file_name,note,Food,Room,Facilities,Service,Public_area\n"
                 "a.png,1,1,0,0,0,0\nb.png,0,0,0,0,0,0\nc.png,,0,1,,0,1\nd.png,0,,,,,\n")
    df = CAT.read_image_labels(str(p))
    assert df["file_name"].tolist() == ["a.png", "c.png"] and df.index.tolist() == [0, 1]
    assert df.iloc[:, 2:].values.astype(int).tolist() == [[1, 0, 0, 0, 0], [0, 1, 0, 0, 1]]


def test_xlsx_without_openpyxl_is_a_clear_error(tmp_path, monkeypatch):
    from fcmf_framework import categories as CAT
    real = importlib.util.find_spec
    monkeypatch.setattr(importlib.util, "find_spec", lambda name, *a: None if name == "openpyxl" else real(name, *a))
    p = tmp_path / "labels.xlsx"
    p.write_bytes(b"PK\x03\x04")
    with pytest.raises(RuntimeError, match="openpyxl.*csv"):
        CAT.read_image_labels(str(p))


def _ref_keys(resnet_keys):
    """the reference's MyImgModel keys: feature_extractor.*, no_fc.{0,1,4..7}.* (torchvision children minus fc), linear.*"""
    child = {"conv1": 0, "bn1": 1, "layer1": 4, "layer2": 5, "layer3": 6, "layer4": 7}
    keys = {"feature_extractor." + k for k in resnet_keys}
    for k in resnet_keys:
        head, rest = k.split(".", 1)
        if head in child:
            keys.add(f"no_fc.{child[head]}.{rest}")
    return keys | {"linear.weight", "linear.bias"}


@pytest.mark.parametrize("cls", ["MyImgModel", "MyRoIModel"])
def test_state_dict_keys_are_the_references(cls):
    import synthetic_data as synth
    from fcmf_framework import categories as CAT
    from fcmf_framework.resnet import ResNet
    m = getattr(CAT, cls)(5, ResNet(synth.RESNET152_LAYERS))
    tv = set(synth.resnet_param_shapes(synth.RESNET152_LAYERS, with_fc=True))
    assert "fc.weight" in tv and "layer3.35.bn3.running_var" in tv
    sd = m.state_dict()
    assert set(sd) == _ref_keys(tv)
    assert sd["no_fc.6.35.conv3.weight"].data_ptr() == sd["feature_extractor.layer3.35.conv3.weight"].data_ptr()
    assert tuple(sd["linear.weight"].shape) == (5, 2048) and tuple(sd["feature_extractor.fc.weight"].shape) == (1000, 2048)
    # a checkpoint written under nn.DataParallel loads
    m2 = getattr(CAT, cls)(5, ResNet(synth.RESNET152_LAYERS))
    m2.load_state_dict({"module." + k: v for k, v in sd.items()})
    assert (m2.state_dict()["linear.weight"] == sd["linear.weight"]).all()


def test_crop_desc_mirror_matches_header():
    from fcmf_framework import _hip
    src = open(os.path.join(ROOT, "include", "fcmf_hip.h")).read()
    body = src[:src.index("} fcmf_crop_desc;")]
    body = body[body.rindex("typedef struct {") + len("typedef struct {"):]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            decl = re.sub(r"^(int64_t|int)\s+", "", decl)
            fields += [f.strip() for f in decl.split(",")]
    assert fields == [f[0] for f in _hip.CropDesc._fields_]
    import ctypes
    assert ctypes.sizeof(_hip.CropDesc) == 64
    assert "fcmf_crop_resize_normalize" in _hip.SIGNATURES and "fcmf_bce_logits" in _hip.SIGNATURES


def test_no_package_file_imports_oracle():
    bad = []
    for d, _, files in os.walk(PKG):
        for f in files:
            if f.endswith(".py"):
                text = open(os.path.join(d, f)).read()
                if re.search(r"^\s*(from\s+oracle\b|import\s+oracle\b)", text, flags=re.M):
                    bad.append(os.path.relpath(os.path.join(d, f), PKG))
    assert bad == []
