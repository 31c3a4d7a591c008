"""Host side of fcmf_framework/predict.py and of the inference.py driver, without a GPU: box merging against outputs recorded from
the reference, the renames of old checkpoints, tags -> prompt, the driver's parser and its output file.

tests/golden/merge_boxes.json holds 21 box lists with what the reference's merge_boxes (fcmf_framework/image_process.py:69-113,
executed out of its file through `ast`: the file itself imports ultralytics and cv2) returned for them: [{"key", "coordinates"}] in
the order of its dictionary.  Where the reference tree is present the same comparison runs on 200 seeded random lists."""
import ast
import json
import os
import random

import pytest
import torch

from conftest import GOLD
import synthetic_data as synth

REFERENCE = os.path.join(os.environ.get("FCMF_REFERENCE_DIR", "/root/reference"), "fcmf_framework", "image_process.py")


def _mine(boxes, eps):
    from fcmf_framework.predict import merge_boxes
    return [{"key": k, "coordinates": list(c)} for k, c in merge_boxes(boxes, eps)]


def test_merge_boxes_golden():
    cases = json.load(open(os.path.join(GOLD, "merge_boxes.json")))
    assert len(cases) >= 20
    names = {c["name"] for c in cases}
    assert {"empty list", "exactly eps apart", "third near the merged box, not the first", "separate entry followed by a near box"} <= names
    for c in cases:
        before = json.dumps(c["boxes"])
        assert _mine(c["boxes"], c["eps"]) == c["merged"], c["name"]
        assert json.dumps(c["boxes"]) == before, "the detections were modified"


def test_merge_boxes_random_against_the_reference():
    if not os.path.exists(REFERENCE):
        pytest.skip("the reference tree is not on this machine")
    tree = ast.parse(open(REFERENCE).read())
    want = {"merge_boxes", "are_boxes_nearby", "merge_coordinates"}
    ns = {}
    exec(compile(ast.Module(body=[n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in want], type_ignores=[]), REFERENCE, "exec"), ns)
    rng = random.Random(20)
    cats = ["bed", "chair", "cup", "potted plant"]
    for _ in range(200):
        boxes = []
        for _ in range(rng.randint(0, 9)):
            l, t = rng.randint(0, 120), rng.randint(0, 120)
            boxes.append({"category": rng.choice(cats), "coordinates": [l, t, l + rng.randint(1, 90), t + rng.randint(1, 90)]})
        eps = rng.choice([0, 10, 30, 60])
        ref = ns["merge_boxes"]([dict(b, coordinates=list(b["coordinates"])) for b in boxes], eps)
        assert _mine(boxes, eps) == [{"key": k, "coordinates": list(e["coordinates"])} for k, e in ref.items()]


def test_crop_boxes_orientation_and_drop_list():
    from fcmf_framework.predict import crop_boxes
    dets = [{"category": "bed", "coordinates": [10, 20, 110, 220]}, {"category": "car", "coordinates": [0, 0, 5, 5]}]
    # [left, top, right, bottom] -> rows top:bottom, columns left:right
    assert crop_boxes(dets, 30) == [(20, 220, 10, 110), (0, 5, 0, 5)]
    assert crop_boxes(dets, 30, drop_categories=("car",)) == [(20, 220, 10, 110)]
    assert crop_boxes([], 30) == [] and crop_boxes(None, 30) == []


# ---- checkpoints ----------------------------------------------------------------------------------------------------------------
def _tiny_fcmf(seed=0, NI=2, NR=3):
    from helpers import build_fcmf
    return build_fcmf(synth.TINY_CFG, NI, NR, "cpu", seed=seed)[0]


def _old_names(sd):
    """a state dict as older code wrote it: the inverse of the reference's renames (inference.py:175-189)"""
    out = {}
    for k, v in sd.items():
        k = k.replace("text2img", "ent2img").replace("text2roi", "ent2roi").replace("mm_attention", "comb_attention")
        if k.startswith("text_pooler.") or k.startswith("classifier."):
            k = "encoder." + k
        elif k.startswith("encoder."):
            k = k[len("encoder."):]
        out[k] = v
    return out


def test_checkpoint_renames():
    from fcmf_framework.predict import load_fcmf_state
    src = _tiny_fcmf(seed=3)
    sd = {k: v.clone() for k, v in src.state_dict().items()}
    old = _old_names(sd)
    assert set(old) != set(sd) and any("ent2img" in k for k in old) and "encoder.classifier.weight" in old
    dst = _tiny_fcmf(seed=0)
    missing, unexpected, renamed = load_fcmf_state(dst, old)
    assert renamed and missing == [] and unexpected == []
    assert all(torch.equal(v, dst.state_dict()[k]) for k, v in sd.items())
    dst2 = _tiny_fcmf(seed=0)
    missing, unexpected, renamed = load_fcmf_state(dst2, sd)
    assert not renamed and missing == [] and unexpected == []
    assert all(torch.equal(v, dst2.state_dict()[k]) for k, v in sd.items())


# ---- tags and prompt ------------------------------------------------------------------------------------------------------------
PairTokenizer = synth.BytePairTokenizer      # ids = byte values of both segments: prompts compare position by position


def _predictor(**kw):
    from fcmf_framework import categories as C
    from fcmf_framework.predict import Predictor
    from fcmf_framework.resnet import ResNet
    tiny = lambda: ResNet(synth.RESNET_TINY_LAYERS)
    return Predictor(_tiny_fcmf(), PairTokenizer(), tiny(), tiny(), C.MyImgModel(5, tiny()), C.MyRoIModel(5, tiny()),
                     num_imgs=2, num_rois=3, seq_len=38, **kw)


def test_tags_and_prompt():
    from fcmf_framework.predict import ASPECTS, tags_from_outputs
    from review_batches import ReviewProducer
    big = 10.0
    # three photos: photos 0 and 1 belong to review 0, photo 2 to review 1; review 2 has none
    image_logits = torch.tensor([[-big, big, -big, -big, big], [big, -big, -big, -big, 0.3], [-big, -big, -big, -big, 0.3]])
    roi_logits = torch.tensor([[0.1, 0.2, 0.9, 0.0, 0.0], [2.0, 0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.9, 0.0, 0.0]])
    # merged boxes 0 and 1 lie on photo 0, box 2 on photo 2
    tags = tags_from_outputs(image_logits, [0, 1, 2], roi_logits, [0, 0, 2], 3, [0, 0, 1], image_threshold=0.6)
    # sigmoid(0.3) = 0.574 < 0.6: Public_area of photos 1 and 2 stays out; unions per review, sorted; 'empty' when none
    assert tags == [(['Food', 'Public_area', 'Room'], ['facilities', 'food']), (['empty'], ['facilities']), (['empty'], ['empty'])]
    reviews = [{"text": "phong rong va sach", "photos": [], "detections": []} for _ in range(3)]
    ids = {}
    for pooling in (False, True):
        p = _predictor(reference_pooling=pooling)
        got = p.prompts(reviews, tags)
        assert [tuple(t.shape) for t in got] == [(3, 6, 38), (3, 6, 38), (3, 6, 38), (3, 6, 38 + 49)]
        assert bool((got[3] == 1).all())
        ids[pooling] = got
        prod = ReviewProducer(PairTokenizer(), "", None, {}, {}, 2, 3, seq_len=38)
        for r in range(3):
            for a, aspect in enumerate(ASPECTS):
                want = prod.encode(aspect, reviews[r]["text"], tags[r])
                for k in range(4):
                    assert torch.equal(got[k][r, a].cpu(), want[k])
    assert all(torch.equal(x, y) for x, y in zip(ids[False], ids[True]))


def test_ready_made_tags_are_sorted_and_classifier_tags_go_through_predictor(monkeypatch):
    p = _predictor()
    calls = []

    def fake(which, x):
        calls.append((which, x.shape[0]))
        return torch.tensor([[9.0, -9.0, -9.0, -9.0, -9.0]]).repeat(x.shape[0], 1) if which == "image_cls" else \
            torch.tensor([[0.0, 0.0, 0.0, 5.0, 0.0]]).repeat(x.shape[0], 1)
    monkeypatch.setattr(p, "_classify", fake)
    reviews = [{"text": "a", "tags": (["Room", "Food", "Room"], [])}, {"text": "b"}, {"text": "c"}]
    t_img = torch.zeros(3, 2, 3, 4, 4)
    crops = torch.zeros(3, 3, 4, 4)
    # review 0: one photo with a box (ready-made tags: not classified); review 1: two photos, two boxes on the second; review 2: nothing
    extra = ([(0, 0), (1, 0), (1, 1)], crops, [(0, 0, 0), (1, 1, 0), (1, 1, 1)])
    tags = p.tags(reviews, t_img, extra)
    assert tags == [(['Food', 'Room'], ['empty']), (['Food'], ['service']), (['empty'], ['empty'])]
    assert calls == [("image_cls", 2), ("roi_cls", 2)]
    calls.clear()
    assert p.tags(reviews[:1], t_img[:1], ([(0, 0)], crops[:1], [(0, 0, 0)])) == [(['Food', 'Room'], ['empty'])]
    assert calls == []


# ---- driver ---------------------------------------------------------------------------------------------------------------------
def test_driver_parser_and_output_file(tmp_path):
    import inference as drv
    from fcmf_framework.predict import write_result
    a = drv.parse_args(["--base_path_model", "ckpt", "--text", "Phong dep", "--image_list", "a.png", "b.png", "--num_images", "7",
                        "--num_rois", "4", "--pretrained_model", "xlm-roberta-base", "--output_file", "out.txt"])
    assert (a.base_path_model, a.text, a.image_list, a.num_images, a.num_rois, a.pretrained_model, a.output_file) == \
        ("ckpt", "Phong dep", ["a.png", "b.png"], 7, 4, "xlm-roberta-base", "out.txt")
    assert drv.parse_args(["--base_path_model", "c", "--text", "t", "--names-list", "x.png"]).image_list == ["x.png"]
    d = drv.parse_args(["--base_path_model", "c", "--text", "t"])
    assert (d.num_images, d.num_rois, d.pretrained_model, d.output_file, d.image_list) == (7, 4, "xlm-roberta-base", None, None)
    assert not d.bf16 and not d.no_fold_bn and not d.reference_pooling and d.batch_size == 8
    b = drv.parse_args(["--base_path_model", "c", "--reviews", "r.jsonl", "--batch_size", "3", "--detections", "d.json", "--bf16",
                        "--no_fold_bn", "--reference_pooling", "--image_category_checkpoint", "i.pth", "--roi_category_checkpoint", "r.pth",
                        "--resnet_checkpoint", "tv.pth"])
    assert b.reviews == "r.jsonl" and b.batch_size == 3 and b.bf16 and b.no_fold_bn and b.reference_pooling
    with pytest.raises(SystemExit):
        drv.parse_args(["--base_path_model", "c", "--reviews", "r.jsonl", "--text", "t"])
    with pytest.raises(SystemExit):
        drv.parse_args(["--base_path_model", "c"])
    result = {"Location": "None", "Food": "Positive", "Room": "Negative", "Facilities": "None", "Service": "Neutral", "Public_area": "None"}
    out = tmp_path / "out.txt"
    write_result(str(out), "Phong dep", ["a.png", "b.png"], result)
    assert out.read_text(encoding="utf-8") == (
        "Text: Phong dep\nNumber of images: 2\nImages: a.png, b.png\n\n" + "=" * 50 + "\nPREDICTIONS:\n" + "=" * 50 + "\n\n"
        "Location: None\nFood: Positive\nRoom: Negative\nFacilities: None\nService: Neutral\nPublic_area: None\n")
    write_result(str(out), "x", [], {"Location": "None"})
    assert out.read_text(encoding="utf-8") == "Text: x\nNumber of images: 0\n\n" + "=" * 50 + "\nPREDICTIONS:\n" + "=" * 50 + "\n\nLocation: None\n"


def test_detections_file_forms(tmp_path):
    import inference as drv
    det = [{"category": "bed", "coordinates": [1, 2, 3, 4]}]
    f = tmp_path / "d.json"
    f.write_text(json.dumps({"/x/a.png": det, "b.png": []}))
    assert drv.load_detections(str(f), ["/x/a.png", "/y/b.png", "c.png"]) == [det, [], []]
    f.write_text(json.dumps([det, []]))
    assert drv.load_detections(str(f), ["a.png", "b.png"]) == [det, []]
    with pytest.raises(ValueError):
        drv.load_detections(str(f), ["a.png"])
    assert drv.load_detections(None, ["a.png"]) == [[]]


def test_detections_from_a_list_or_a_callable():
    photo = torch.zeros(3, 40, 50, dtype=torch.uint8)
    p = _predictor(image_loader=lambda path: photo)
    det = [{"category": "bed", "coordinates": [1, 2, 30, 20]}, {"category": "bed", "coordinates": [3, 4, 31, 22]}]
    seen = []
    listed = p._photos({"photos": ["a.png", "b.png", "c.png"], "detections": [det, []]})        # (num_imgs = 2: the third photo is not read)
    called = p._photos({"photos": ["a.png", "b.png"], "detections": lambda ph: seen.append(ph) or (det if ph == "a.png" else [])})
    assert seen == ["a.png", "b.png"]
    for got in (listed, called):
        assert [b for _, b in got] == [[(2, 22, 1, 31)], []] and all(ph is photo for ph, _ in got)
