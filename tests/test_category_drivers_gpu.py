"""Both category drivers end to end on the GPU (image_processing/run_image_categories.py, run_roi_categories.py):
24 seeded synthetic photos written as PNG, a CSV photo label file and a ROI CSV; --do_train --get_cate for one epoch; every
output file, the JSON keys and values, the checkpoint round trip (also with a `module.` prefix) and the FCMF prompt builder
consuming the JSONs.  (A small ResNet stands in for ResNet-152 through --resnet_checkpoint.)"""
import json
import os
import sys

import numpy as np
import pytest
import torch

import synthetic_data as synth
from conftest import PKG

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(PKG, "image_processing"))

N_PHOTOS = 24
LAYERS = (1, 1, 1, 1)


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    Image = pytest.importorskip("PIL.Image")
    root = tmp_path_factory.mktemp("cat")
    img_dir = root / "images"
    img_dir.mkdir()
    rng = np.random.RandomState(0)
    names = []
    for i in range(N_PHOTOS):
        h, w = rng.randint(120, 300), rng.randint(120, 300)
        a = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        name = f"photo_{i:02d}"
        Image.fromarray(a).save(img_dir / f"{name}.png")
        names.append((name, h, w))
    aspects = ['Food', 'Room', 'Facilities', 'Service', 'Public_area']
    lines = ["file_name,text," + ",".join(aspects)]
    for i, (n, _, _) in enumerate(names):
        lab = [(i + k) % 3 == 0 for k in range(5)]
        lines.append(f"{n}.png,t{i}," + ",".join("1" if v else "" for v in lab))
    (root / "image_labels.csv").write_text("\n".join(lines) + "\n")
    roi_aspects = ['food', 'room', 'facilities', 'service', 'public_area']
    rows = ["file_name,x1,x2,y1,y2,label"]
    for i, (n, h, w) in enumerate(names):
        for r in range(1 + i % 8):                         # up to 8 ROIs: --get_cate keeps the first 6
            x1, y1 = rng.randint(0, h - 20), rng.randint(0, w - 20)
            rows.append(f"{n},{x1},{x1 + rng.randint(10, 400)},{y1},{y1 + rng.randint(10, 400)},{roi_aspects[(i + r) % 5]}")
    (root / "roi_labels.csv").write_text("\n".join(rows) + "\n")
    from fcmf_framework.resnet import ResNet
    sd = ResNet(LAYERS).state_dict()
    sd.update(synth.synth_resnet_params(synth.resnet_param_shapes(LAYERS), 0))
    torch.save(sd, root / "resnet.pth")
    return root, [n for n, _, _ in names]


def _load_fresh(cls, path, prefix=""):
    from fcmf_framework import categories as CAT
    from fcmf_framework.resnet import ResNet
    sd = torch.load(path, map_location="cpu", weights_only=False)["model_state_dict"]
    m = getattr(CAT, cls)(5, ResNet(LAYERS))
    m.load_state_dict({prefix + k: v for k, v in sd.items()})
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k]), k
    return sd


def _visual_tags(img_json, roi_json, photos):
    import review_batches as RB
    p = RB.ReviewProducer(None, "", None, img_json, roi_json, num_img=3, num_roi=4)
    return p.visual_tags(photos)


def test_image_driver(dev, data):
    import run_image_categories as drv
    root, names = data
    out = root / "out_img"
    drv.main(["--image_dir", str(root / "images"), "--image_label_path", str(root / "image_labels.csv"), "--output_dir", str(out),
              "--do_train", "--get_cate", "--num_train_epochs", "1", "--train_batch_size", "8", "--eval_batch_size", "8",
              "--resnet_checkpoint", str(root / "resnet.pth")])
    for f in ("image_categories.log", "seed_42_image_model.pth", "test_image_results.txt", "resnet152_image_label.json"):
        assert (out / f).is_file(), f
    assert "Test Eval results" in (out / "test_image_results.txt").read_text()
    labels = json.loads((out / "resnet152_image_label.json").read_text())
    assert set(labels) == {n + ".png" for n in names}
    aspects = {'Food', 'Room', 'Facilities', 'Service', 'Public_area'}
    assert all(set(v) <= aspects and v == sorted(v) for v in labels.values())
    _load_fresh("MyImgModel", out / "seed_42_image_model.pth")
    _load_fresh("MyImgModel", out / "seed_42_image_model.pth", prefix="module.")
    img_tags, _ = _visual_tags(labels, {}, [names[0] + ".png", names[1] + ".png"])
    assert img_tags == (sorted(set(labels[names[0] + ".png"] + labels[names[1] + ".png"])) or ["empty"])


def test_roi_driver(dev, data):
    import run_roi_categories as drv
    root, names = data
    out = root / "out_roi"
    drv.main(["--image_dir", str(root / "images"), "--roi_label_path", str(root / "roi_labels.csv"), "--output_dir", str(out),
              "--do_train", "--get_cate", "--num_train_epochs", "1", "--bf16", "--resnet_checkpoint", str(root / "resnet.pth")])
    for f in ("roi_categories.log", "seed_42_roi_model.pth", "test_roi_results.txt", "test_roi_predictions_detail.txt",
              "resnet152_roi_label.json"):
        assert (out / f).is_file(), f
    assert "TEST RESULTS" in (out / "test_roi_results.txt").read_text()
    labels = json.loads((out / "resnet152_roi_label.json").read_text())
    assert set(labels) == {n + ".png" for n in names}
    aspects = {'food', 'room', 'facilities', 'service', 'public_area'}
    assert all(set(v) <= aspects and v == sorted(v) and 1 <= len(v) <= 6 for v in labels.values())
    _load_fresh("MyRoIModel", out / "seed_42_roi_model.pth", prefix="module.")
    img = json.loads((root / "out_img" / "resnet152_image_label.json").read_text()) if (root / "out_img").exists() else {}
    _, roi_tags = _visual_tags(img, labels, [names[2] + ".png"])
    assert roi_tags == (labels[names[2] + ".png"] or ["empty"])
