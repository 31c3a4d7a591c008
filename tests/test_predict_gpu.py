"""fcmf_framework/predict.Predictor and the inference.py driver end to end on the GPU: a tiny FCMF (synthetic weights), tiny trunks
and tiny category classifiers, photos as seeded uint8 arrays of different sizes, seeded detections, a byte-level pair tokenizer.

Three reviews with 0, 2 and 9 photos (num_imgs = 2, num_rois = 3, 224 x 224 crops).  The oracle side is computed once: the
oracle trunk (oracle/resnet_oracle.py, eval mode) on the predictor's own pixel tensors, then oracle/fcmf_oracle.py per aspect.
Logits within 1e-3 of it in float32 (the project's asserted parity), with BatchNorm folded and not."""
import json

import pandas as pd
import pytest
import torch

from helpers import _recorded, build_fcmf
from oracle import fcmf_oracle as FO
from oracle import resnet_oracle as RO
import synthetic_data as synth
from test_image_preprocess_gpu import _check, _photo
from test_predict_cpu import PairTokenizer

pytestmark = pytest.mark.gpu

NI, NR, S = 2, 3, 38
TINY = synth.RESNET_TINY_LAYERS
SIZES = {"a.png": (300, 420), "b.png": (517, 389), **{f"c{i}.png": (240 + 10 * i, 200 + 7 * i) for i in range(9)}}
PHOTOS = {n: _photo(h, w, 50 + i) for i, (n, (h, w)) in enumerate(SIZES.items())}


def _loader(path):
    return PHOTOS[path]


def _dets(name, seed):
    """seeded detections inside the photo: two near boxes of one category (they merge), a far one, another category"""
    g = torch.Generator().manual_seed(seed)
    h, w = SIZES[name]
    out = []
    for cat, n in (("bed", 3), ("chair", 1)):
        l, t = int(torch.randint(0, w // 3, (1,), generator=g)), int(torch.randint(0, h // 3, (1,), generator=g))
        out.append({"category": cat, "coordinates": [l, t, l + w // 3, t + h // 3]})
        if n > 1:
            out.append({"category": cat, "coordinates": [l + 10, t + 5, l + w // 3 + 20, t + h // 3 + 10]})
            out.append({"category": cat, "coordinates": [w // 2, h // 2, w - 5, h + 40]})          # (reaches past the photo's end)
    return out


REVIEWS = [
    {"text": "vi tri xa trung tam", "photos": [], "detections": []},
    {"text": "phong rong, do an ngon", "photos": ["a.png", "b.png"], "detections": [_dets("a.png", 1), []]},
    {"text": "nhan vien than thien", "photos": [f"c{i}.png" for i in range(9)], "detections": [_dets(f"c{i}.png", 10 + i) for i in range(9)]},
]


def _trunk(dev, seed):
    from fcmf_framework.resnet import ResNet
    m = ResNet(TINY)
    P = synth.synth_resnet_params(synth.resnet_param_shapes(TINY), seed)
    m.load_state_dict(P, strict=False)
    return m.to(dev).eval(), P


def _classifier(cls, dev, seed):
    g = torch.Generator().manual_seed(seed)
    trunk, P = _trunk(dev, seed)
    m = cls(5, trunk)
    m.trunk_params = P
    m.linear.weight.data = (torch.randn(5, 2048, generator=g) * 0.05).to(dev)
    m.linear.bias.data = (torch.randn(5, generator=g) * 0.1).to(dev)
    return m.to(dev).eval()


class World:
    pass


@pytest.fixture(scope="module")
def world(dev):
    from fcmf_framework import categories as C
    from fcmf_framework import ops
    from fcmf_framework.predict import Predictor
    ops.set_compute_dtype(torch.float32)
    ops.shadows.clear()
    w = World()
    w.model, w.P = build_fcmf(synth.TINY_CFG, NI, NR, dev, seed=0)
    (w.img, w.Pimg), (w.roi, w.Proi) = _trunk(dev, 1), _trunk(dev, 2)
    w.cimg, w.croi = _classifier(C.MyImgModel, dev, 7), _classifier(C.MyRoIModel, dev, 4)
    w.Pcimg, w.Pcroi = w.cimg.trunk_params, w.croi.trunk_params
    w.make = lambda **kw: Predictor(w.model, PairTokenizer(), w.img, w.roi, w.cimg, w.croi, num_imgs=NI, num_rois=NR, seq_len=S,
                                    image_loader=_loader, **kw)
    w.pred = {fold: w.make(fold_bn=fold) for fold in (True, False)}
    # the oracle, once: its trunk on the predictor's pixel tensors, then the FCMF oracle per aspect
    p = w.pred[False]
    with torch.no_grad():
        t_img, roi_img, coors, extra = p.pixels(REVIEWS)
        w.pixels, w.extra = (t_img, roi_img, coors), extra
        w.tags = p.tags(REVIEWS, t_img, extra)
        ids, tts, ams, added = (t.cpu() for t in p.prompts(REVIEWS, w.tags))
        vis = RO.my_resnet_img(w.Pimg, t_img.flatten(0, 1).cpu(), TINY, 7).view(-1, 2048, 49).permute(0, 2, 1).reshape(3, NI, 49, 2048)
        roi = RO.my_resnet_roi(w.Proi, roi_img.flatten(0, 2).cpu(), TINY).reshape(3, NI, NR, 2048)
        w.vis_ref, w.roi_ref = vis, roi
        w.oracle = torch.stack([FO.fcmf_forward(w.P, synth.TINY_CFG, ids[:, a], vis, roi, coors.cpu(), tts[:, a], ams[:, a], added[:, a],
                                                NI, NR) for a in range(6)], 1).float()
    return w


def test_pixels_equal_review_producer(world):
    from fcmf_framework.predict import crop_boxes
    from review_batches import ReviewProducer
    rows = [(name, *box) for rev in REVIEWS for name, d in zip(rev["photos"], rev["detections"]) for box in crop_boxes(d, 30)]
    roi_df = pd.DataFrame(rows, columns=["file_name", "x1", "x2", "y1", "y2"])
    prod = ReviewProducer(PairTokenizer(), "", roi_df, {}, {}, NI, NR, image_loader=_loader, seq_len=S)
    t_img, roi_img, coors = world.pixels
    assert t_img.shape == (3, NI, 3, 224, 224) and roi_img.shape == (3, NI, NR, 3, 224, 224) and coors.shape == (3, NI, NR, 4)
    for r, rev in enumerate(REVIEWS):
        ti, ri, ci = prod.pixels(rev["photos"])
        _check(t_img[r], ti, torch.float32)
        _check(roi_img[r], ri.float(), torch.float32)
        assert torch.equal(coors[r].cpu().double(), ci.double().float().double())
    assert not t_img[0].any() and not roi_img[0].any() and not coors[0].any()          # the review without photos
    assert roi_img[1, 0].flatten(1).any(1).all() and coors[1, 0].any(1).all()           # photo a: bed (two merged), bed_2, chair
    assert not roi_img[1, 1].any() and not coors[1, 1].any()                            # photo b: no detections


@pytest.mark.parametrize("fold", [True, False], ids=["fold_bn", "plain"])
def test_features_match_the_oracle_trunk(world, fold):
    """the tiny FCMF's logits move by 1e-6 when its visual inputs are zeroed (synthetic weights of 0.02): the logit comparison below
    says little about the features, so they are compared themselves -- 1e-4 of the largest reference value, as the float32 trunk"""
    t_img, roi_img, _ = world.pixels
    with torch.no_grad():
        vis, roi = world.pred[fold].features(t_img, roi_img)
    for name, got, ref in (("vis", vis, world.vis_ref), ("roi", roi, world.roi_ref)):
        err, scale = float((got.cpu() - ref).abs().max()), float(ref.abs().max())
        print(f"MEASURED features fold_bn={fold} {name}: max error {err:.3e}, max|ref| {scale:.3e}")
        assert got.shape == ref.shape and err <= 1e-4 * scale
    assert float((world.vis_ref[0, 0] - world.vis_ref[1, 0]).abs().max()) > 1e-2 * float(world.vis_ref.abs().max())      # (a zero crop and a photo differ)


def test_tags_match_the_oracle_classifiers(world):
    from fcmf_framework.predict import tags_from_outputs
    t_img, _, _ = world.pixels
    whole_at, crops, box_at = world.extra
    assert whole_at == [(1, 0), (1, 1), (2, 0), (2, 1)] and len(box_at) == 9          # photo a and c0, c1: bed, bed_2, chair each
    head = lambda m, f: f @ m.linear.weight.detach().cpu().t() + m.linear.bias.detach().cpu()
    il = head(world.cimg, RO.my_resnet_roi(world.Pcimg, torch.stack([t_img[r, i] for r, i in whole_at]).cpu(), TINY))
    rl = head(world.croi, RO.my_resnet_roi(world.Pcroi, crops.cpu(), TINY))
    # the decisions are not close calls (else: another classifier seed)
    assert float((torch.sigmoid(il) - 0.6).abs().min()) > 1e-3
    top = rl.topk(2, -1).values
    assert float((top[:, 0] - top[:, 1]).min()) > 1e-3
    photos = sorted(set(whole_at) | {b[:2] for b in box_at})
    pid = {p: n for n, p in enumerate(photos)}
    want = tags_from_outputs(il, [pid[p] for p in whole_at], rl, [pid[b[:2]] for b in box_at], 3, [r for r, _ in photos], 0.6)
    assert world.tags == want
    assert world.tags[0] == (['empty'], ['empty'])
    assert any(t != (['empty'], ['empty']) for t in world.tags[1:])


@pytest.mark.parametrize("fold", [True, False], ids=["fold_bn", "plain"])
def test_logits_match_the_oracle_fp32(world, fold):
    from fcmf_framework.predict import ASPECTS, POLARITIES
    pol, logits = world.pred[fold].predict(REVIEWS, batch_size=8)
    assert logits.shape == (3, 6, 4) and logits.dtype == torch.float32 and not logits.is_cuda
    err = float((logits - world.oracle).abs().max())
    print(f"MEASURED predict fold_bn={fold}: max |logit - oracle| {err:.3e}")
    assert err <= 1e-3
    top = world.oracle.topk(2, -1)
    sure = (top.values[..., 0] - top.values[..., 1]) > 2e-3
    assert bool(sure.any()), "no (review, aspect) with an oracle margin above 2e-3: the polarity check would be vacuous"
    for r in range(3):
        assert list(pol[r]) == ASPECTS
        for a, asp in enumerate(ASPECTS):
            if sure[r, a]:
                assert pol[r][asp] == POLARITIES[int(top.indices[r, a, 0])]


def test_batch_invariance(world):
    p = world.pred[True]
    _, together = p.predict(REVIEWS, batch_size=8)
    _, single = p.predict(REVIEWS, batch_size=1)
    err = float((together - single).abs().max())
    print(f"MEASURED batch invariance: {err:.3e}")
    assert err <= 1e-5


def test_reference_pooling(world):
    t_img, roi_img, _ = world.pixels
    with torch.no_grad():
        vis_ref, roi_ref = world.make(reference_pooling=True).features(t_img, roi_img)
        vis, roi = world.pred[True].features(t_img, roi_img)
    assert vis_ref.shape == vis.shape == (3, NI, 49, 2048)
    assert torch.equal(vis_ref, vis_ref[:, :, :1].expand_as(vis_ref))                   # all 49 patch tokens are the same vector
    mean = vis.mean(2)                                                                  # ... the photo's global mean
    assert float((vis_ref[:, :, 0] - mean).abs().max()) <= 1e-5 * float(mean.abs().max())
    assert not torch.equal(vis, vis_ref) and torch.equal(roi, roi_ref)


def test_ready_made_tags_skip_the_classifiers(world):
    p = world.pred[True]
    tagged = [dict(rev, tags=t) for rev, t in zip(REVIEWS, world.tags)]
    passes = lambda calls: sum(c[0] == "fcmf_maxpool3x3s2" for c in calls)              # one per trunk pass
    out = {}
    with_tags = _recorded(lambda: out.setdefault("tagged", p.predict(tagged)))
    without = _recorded(lambda: out.setdefault("plain", p.predict(REVIEWS)))
    assert passes(with_tags) == 2 and passes(without) == 4                              # the two feature trunks (+ the two classifiers)
    assert float((out["tagged"][1] - out["plain"][1]).abs().max()) <= 1e-6              # the same tags, the same prompt
    from fcmf_framework.predict import Predictor
    bare = Predictor(world.model, PairTokenizer(), world.img, world.roi, num_imgs=NI, num_rois=NR, seq_len=S, image_loader=_loader)
    assert float((bare.predict(tagged)[1] - out["plain"][1]).abs().max()) <= 1e-6
    from fcmf_framework import _hip as H
    with pytest.raises(H.HipLibraryError):
        bare.predict(REVIEWS)


def test_driver_batch_mode(world, dev, tmp_path):
    import inference as drv
    from fcmf_framework import categories as C
    from fcmf_framework.resnet import ResNet
    from fcmf_framework.resnet_utils import myResNetImg, myResNetRoI
    ck = lambda sd: {"epoch": 0, "model_state_dict": sd}
    torch.save(ck(world.model.state_dict()), tmp_path / "seed_42_fcmf_model_best.pth")
    torch.save(ck(myResNetImg(world.img, False, dev).state_dict()), tmp_path / "seed_42_resimg_model_best.pth")
    torch.save(ck(myResNetRoI(world.roi, False, dev).state_dict()), tmp_path / "seed_42_resroi_model_best.pth")
    C.save_model(str(tmp_path / "img_cat.pth"), world.cimg, 0)
    C.save_model(str(tmp_path / "roi_cat.pth"), world.croi, 0)
    src, dst = tmp_path / "reviews.jsonl", tmp_path / "out.jsonl"
    src.write_text("".join(json.dumps({"text": r["text"], "image_list" if i == 1 else "photos": r["photos"], "detections": r["detections"]}) + "\n"
                           for i, r in enumerate(REVIEWS)))
    fresh, _ = build_fcmf(synth.TINY_CFG, NI, NR, dev, seed=5)                           # (other weights: the checkpoint must win)
    args = drv.parse_args(["--base_path_model", str(tmp_path), "--reviews", str(src), "--batch_size", "2", "--output_file", str(dst),
                           "--num_images", str(NI), "--num_rois", str(NR), "--image_category_checkpoint", str(tmp_path / "img_cat.pth"),
                           "--roi_category_checkpoint", str(tmp_path / "roi_cat.pth")])
    # (the driver's main() = parse_args + build_predictor + run; a tiny model, trunk and tokenizer stand in for what the flags name)
    predictor = drv.build_predictor(args, dev, tokenizer=PairTokenizer(), model=fresh, make_trunk=lambda: ResNet(TINY), seq_len=S,
                                    image_loader=_loader)
    drv.run(args, predictor)
    lines = [json.loads(l) for l in dst.read_text().splitlines()]
    want_pol, want_logits = world.pred[True].predict(REVIEWS)
    assert len(lines) == 3
    for line, rev, pol, lg in zip(lines, REVIEWS, want_pol, want_logits):
        assert line["text"] == rev["text"] and line["polarities"] == pol
        assert float((torch.tensor(line["logits"]) - lg).abs().max()) <= 1e-5
