"""CPU-side checks of the comparison baselines: the new layers and models carry torch's state-dict keys and shapes, the
constructor options the baselines do not use are refused, and the binding lists the new attention entry points."""
import pytest
import torch
import torch.nn as nn

from baseline_ref import CFG, RefM, RefT
from helpers import make_hf_dir


def _shapes(m):
    return {k: tuple(v.shape) for k, v in m.state_dict().items()}


def test_layers_carry_torch_state_dict_keys_and_shapes():
    from fcmf_framework import torch_layers as T
    assert _shapes(T.MultiheadAttention(128, 2, dropout=0.1, batch_first=True)) == \
        _shapes(nn.MultiheadAttention(128, 2, dropout=0.1, batch_first=True))
    mk = lambda mod: mod.TransformerEncoder(mod.TransformerEncoderLayer(d_model=128, nhead=2, dim_feedforward=256, dropout=0.1,
                                                                        activation="gelu", batch_first=True), num_layers=3)
    ours, theirs = _shapes(mk(T)), _shapes(mk(nn))
    assert ours == theirs and "layers.2.self_attn.in_proj_weight" in ours and "layers.0.norm2.bias" in ours
    # every layer of the stack starts from the same parameters, as torch's deep copies do
    enc = mk(T)
    assert torch.equal(enc.layers[0].linear1.weight, enc.layers[2].linear1.weight)
    assert enc.layers[0].linear1.weight.data_ptr() != enc.layers[2].linear1.weight.data_ptr()


def test_unused_constructor_options_are_refused():
    from fcmf_framework import torch_layers as T
    with pytest.raises(NotImplementedError):
        T.MultiheadAttention(128, 2)                               # batch_first=False
    with pytest.raises(NotImplementedError):
        T.MultiheadAttention(128, 2, batch_first=True, kdim=64)
    with pytest.raises(NotImplementedError):
        T.TransformerEncoderLayer(128, 2, batch_first=True)        # relu
    with pytest.raises(NotImplementedError):
        T.TransformerEncoderLayer(128, 2, activation="gelu", batch_first=True, norm_first=True)
    with pytest.raises(NotImplementedError):
        T.TransformerEncoder(T.TransformerEncoderLayer(128, 2, activation="gelu", batch_first=True), 1, norm=nn.LayerNorm(128))


def test_models_carry_the_training_scripts_state_dict_keys():
    """`roberta.*` is the text encoder's own key set; everything else equals the same model written with torch's modules"""
    from fcmf_framework import baselines
    from fcmf_framework.roberta import RobertaModel
    d = make_hf_dir(CFG)
    text = {"roberta." + k: v for k, v in _shapes(RobertaModel.from_pretrained(d)).items()}
    for cls, ref in ((baselines.mRoBERTa, RefM()), (baselines.TomBERT, RefT())):
        assert _shapes(cls(d, num_labels=4)) == {**text, **_shapes(ref)}, cls.__name__
    assert _shapes(baselines.EFCapTrRoBERTa(d)) == {**text, "classifier.weight": (4, 128), "classifier.bias": (4,)}
    tim = baselines.TargetImageMatching(128, 2, 0.1)
    assert {"mha.in_proj_weight", "mha.out_proj.bias", "feed_forward.0.weight", "feed_forward.2.bias", "norm2.weight"} <= set(_shapes(tim))


def test_binding_lists_the_long_key_attention():
    from fcmf_framework import _hip
    assert {"fcmf_attn_mfma_long_fwd", "fcmf_attn_mfma_long_bwd"} <= set(_hip.SIGNATURES)
    assert len(_hip.SIGNATURES["fcmf_attn_mfma_long_bwd"]) == len(_hip.SIGNATURES["fcmf_attn_mfma_bwd"]) + 2   # + kv_share, workspace, bytes; no colsum


PUBLISHED = {
    "mroberta": """--data_dir /kaggle/input/implicit-vimacsa --output_dir /kaggle/working/ViMACSA/output_mROBERTa
        --image_dir /kaggle/input/vimacsa/ViMACSA/image --pretrained_hf_model /kaggle/input/uitnlpvisobert/pytorch/default/1
        --list_aspect Location Food Room Facilities Service Public_area --num_polarity 4 --num_imgs 7 --num_rois 4
        --train_batch_size 4 --eval_batch_size 64 --num_train_epochs 13 --learning_rate 3e-5 --warmup_proportion 0.1
        --gradient_accumulation_steps 2 --do_train --do_eval --fp16 --seed 42""",
    "tomroberta": """--data_dir /kaggle/input/implicit-vimacsa --output_dir /kaggle/working/ViMACSA/output_tomROBERTa
        --image_dir /kaggle/input/vimacsa/ViMACSA/image --pretrained_hf_model /kaggle/input/uitnlpvisobert/pytorch/default/1
        --list_aspect Location Food Room Facilities Service Public_area --num_polarity 4 --num_imgs 7 --num_rois 4
        --train_batch_size 4 --eval_batch_size 64 --num_train_epochs 13 --learning_rate 3e-5 --warmup_proportion 0.1
        --gradient_accumulation_steps 2 --do_train --do_eval --fp16 --seed 42""",
    "ef_captr": """--data_dir /kaggle/input/implicit-vimacsa --caption_file /kaggle/working/captions_vi_CATr.json
        --output_dir /kaggle/working/ViMACSA/output_ef_captr_roberta --pretrained_hf_model /kaggle/input/uitnlpvisobert/pytorch/default/1
        --num_img 7 --max_len 200 --train_batch_size 4 --eval_batch_size 128 --num_train_epochs 13 --learning_rate 3e-5
        --gradient_accumulation_steps 2 --fp16 --do_train --do_eval""",
}


@pytest.mark.parametrize("model", sorted(PUBLISHED))
def test_parser_accepts_the_published_command_lines(model):
    """the command lines of the reference's result notebooks, with --model in front"""
    import run_baselines
    a = run_baselines.build_parser().parse_args(["--model", model] + PUBLISHED[model].split())
    assert a.model == model and a.num_imgs == 7 and a.train_batch_size == 4 and a.learning_rate == 3e-5 and a.fp16 and a.do_eval
    assert a.gradient_accumulation_steps == 2 and a.num_train_epochs == 13
    if model == "ef_captr":
        assert a.max_len == 200 and a.caption_file.endswith("CATr.json")
    else:
        assert a.num_rois == 4 and a.eval_batch_size == 64 and a.list_aspect[-1] == "Public_area"
    with pytest.raises(SystemExit):
        run_baselines.build_parser().parse_args(PUBLISHED[model].split())          # --model is required


class RecTokenizer:
    """records its calls; ids = byte values of the first text (and 250 + the length of the second), padded with 1"""

    def __init__(self):
        self.calls = []

    def __call__(self, first, second=None, max_length=170, truncation=None, padding=None, **unused):
        self.calls.append((first, second, max_length))
        ids = ([0] + [3 + (b % 200) for b in first.encode()] + ([2, 2, 250 + len(second) % 5] if second is not None else []))[:max_length - 1] + [2]
        n = len(ids)
        return {"input_ids": ids + [1] * (max_length - n), "attention_mask": [1] * n + [0] * (max_length - n)}


def _frame():
    import pandas as pd
    return pd.DataFrame({"comment": ["Phong_sach dep", "Do an ngon"], "list_img": [["a.png", "dir/c.png", "z.png"], []], "x": [0, 0],
                         "text_img_label": [["Room#Positive", "Public_area#Negative", "Room#Neutral"], ["Food#Positive"]]})


class _Cache:
    def __getitem__(self, i):
        return torch.full((2, 49, 2048), float(i)), torch.zeros(2, 4, 2048), torch.zeros(2, 4, 4)


def test_batch_layouts_of_the_three_baselines():
    from baselines_dataset import BaselineDataset
    tok = RecTokenizer()
    vis, roi, tids, tmask, sids, smask, labels, text = BaselineDataset(_frame(), tok, "tomroberta", num_img=2, num_roi=4,
                                                                       feature_cache=_Cache())[0]
    assert vis.shape == (2, 49, 2048) and roi.shape == (2, 4, 2048) and text == "Phong_sach dep"
    assert tids.shape == tmask.shape == (6, 16) and sids.shape == smask.shape == (6, 170)
    assert labels.tolist() == [0, 0, 3, 0, 0, 1]                       # aspect order; the FIRST mention of Room wins
    assert ("public area </s></s> phong sach dep", None, 170) in tok.calls and ("public area", None, 16) in tok.calls
    assert ("room", None, 16) in tok.calls and len(tok.calls) == 12
    assert int(tmask[2].sum()) == len("room") + 2 and int(tids[2, 0]) == 0 and bool((tids[2][tmask[2] == 0] == 1).all())
    tok.calls.clear()
    m = BaselineDataset(_frame(), tok, "mroberta", num_img=2, num_roi=4, feature_cache=_Cache())[1]
    assert len(m) == 6 and m[2].shape == m[3].shape == (6, 170) and m[4].tolist() == [0, 3, 0, 0, 0, 0] and float(m[0].max()) == 1.0
    assert tok.calls[1] == ("food </s></s> do an ngon", None, 170) and len(tok.calls) == 6      # the same sentence prompt, no target
    tok.calls.clear()
    caps = {"a.png": "mot can phong", "c.png": "ho boi", "z.png": "khong dung"}
    ids, mask, labels, text = BaselineDataset(_frame(), tok, "ef_captr", num_img=2, caption_dict=caps, max_len=64)[0]
    assert ids.shape == mask.shape == (6, 64) and labels.tolist() == [0, 0, 2, 0, 0, 1]          # the LAST mention of Room wins
    assert tok.calls[5] == ("Phong_sach dep", "Public area . mot can phong. ho boi", 64)          # base-name lookup, first 2 photos
    assert BaselineDataset(_frame(), tok, "ef_captr", num_img=2, caption_dict=caps, max_len=64)[1][3] == "Do an ngon"
    assert tok.calls[-1][1] == "Public area . hình ảnh bình thường"
    with pytest.raises(ValueError):
        BaselineDataset(_frame(), tok, "fcmf")
