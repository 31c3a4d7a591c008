"""The three training drivers with --rdrop_alpha, end to end on the GPU in synthetic mode at their tiniest geometry (after
tests/test_loss_drivers_gpu.py): --rdrop_alpha 0 logs the losses of a run without the flag, --rdrop_alpha 1.0 finishes with
finite losses and a checkpoint that loads."""
import logging
import math
import os
import re

import pytest
import torch

from helpers import make_hf_dir
import synthetic_data as synth

pytestmark = pytest.mark.gpu


def _run(drv, logger, argv, caplog):
    """the driver's main under argv -> (the logged step losses, every logged line)"""
    from fcmf_framework import ops
    caplog.clear()
    try:
        with caplog.at_level(logging.INFO, logger=logger):
            drv.main(argv)
    finally:
        ops.set_compute_dtype(torch.float32)
        ops.set_ffn_dropout(False)
    lines = [r.getMessage() for r in caplog.records]
    return [float(m.group(1)) for line in lines for m in [re.search(r"step \d+ loss (\S+)", line)] if m], lines


def _loads_finite(path):
    sd = torch.load(path, map_location="cpu", weights_only=True)["model_state_dict"]
    return len(sd) > 0 and all(torch.isfinite(v).all() for v in sd.values() if v.is_floating_point())


def _check(drv, logger, base, out_dir, checkpoint, caplog):
    plain, _ = _run(drv, logger, base + ["--output_dir", out_dir("plain")], caplog)
    zero, lines0 = _run(drv, logger, base + ["--output_dir", out_dir("zero"), "--rdrop_alpha", "0"], caplog)
    assert plain and zero == plain                                   # the flag at 0 is the run without it
    assert any("rdrop_alpha 0" in line for line in lines0)
    on, lines1 = _run(drv, logger, base + ["--output_dir", out_dir("on"), "--rdrop_alpha", "1.0"], caplog)
    assert len(on) == len(plain) and all(math.isfinite(v) and v > 0 for v in on)
    assert on != plain                                               # two dropout passes and a KL term: another loss
    assert any("rdrop_alpha 1" in line for line in lines1)
    assert _loads_finite(os.path.join(out_dir("on"), checkpoint))


def test_finetune_driver(tmp_path, dev, caplog):
    import run_multimodal_fcmf as drv
    base = ["--pretrained_hf_model", make_hf_dir(synth.TINY_CFG), "--do_train", "--num_imgs", "2", "--num_rois", "5",
            "--train_batch_size", "4", "--gradient_accumulation_steps", "1", "--synthetic_steps", "2", "--max_seq_length", "16",
            "--seed", "3", "--num_train_epochs", "1"]
    _check(drv, "fcmf", base, lambda tag: str(tmp_path / tag), "seed_3_fcmf_model_last.pth", caplog)


def test_baseline_driver(tmp_path, dev, caplog):
    import run_baselines as drv
    base = ["--model", "ef_captr", "--pretrained_hf_model", make_hf_dir(synth.TINY_CFG), "--do_train", "--train_batch_size", "4",
            "--synthetic_steps", "2", "--max_len", "16", "--seed", "3", "--num_train_epochs", "1"]
    _check(drv, "baselines", base, lambda tag: str(tmp_path / tag), "seed_3_ef_captr_model_last.pth", caplog)


def test_pretraining_driver(tmp_path, dev, caplog):
    import run_pretraining_fcmf as drv
    base = ["--pretrained_hf_model", make_hf_dir(synth.TINY_CFG), "--do_train", "--num_imgs", "2", "--num_rois", "5",
            "--train_batch_size", "3", "--synthetic_steps", "2", "--synthetic_dec_len", "6", "--num_train_epochs", "1", "--seed", "5"]
    _check(drv, "iaog", base, lambda tag: str(tmp_path / tag), "seed_5_iaog_model_last.pth", caplog)
