"""The three training drivers with --adv_epsilon, end to end on the GPU in synthetic mode at their tiniest geometry (after
tests/test_rdrop_drivers_gpu.py; eleven steps, so that the log holds the losses of steps 0 and 10): --adv_epsilon 0 logs the
losses of a run without the flag; --adv_epsilon 0.5 finishes with finite losses and a checkpoint that loads, logs the clean
loss (step 0 equals the plain run's: the clean pass comes first) and trains other weights (step 10 differs); one run combines
it with --rdrop_alpha and --ema_decay."""
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


def _check(drv, logger, base, out_dir, checkpoint, caplog, combined=False):
    from fcmf_framework import ops
    plain, _ = _run(drv, logger, base + ["--output_dir", out_dir("plain")], caplog)
    zero, lines0 = _run(drv, logger, base + ["--output_dir", out_dir("zero"), "--adv_epsilon", "0"], caplog)
    assert len(plain) == 2 and zero == plain                         # steps 0 and 10; the flag at 0 is the run without it
    assert any("adv_epsilon 0 (off)" in line for line in lines0)
    on, lines1 = _run(drv, logger, base + ["--output_dir", out_dir("on"), "--adv_epsilon", "0.5"], caplog)
    assert len(on) == 2 and all(math.isfinite(v) and v > 0 for v in on)
    assert on[0] == plain[0]                                         # the clean pass comes first and is what is logged
    assert on[1] != plain[1]                                         # ten steps on two gradients each: other weights
    assert any("adv_epsilon 0.5 (FGM" in line for line in lines1)
    assert _loads_finite(os.path.join(out_dir("on"), checkpoint))
    assert ops._adversary is None
    if combined:
        both, lines2 = _run(drv, logger, base + ["--output_dir", out_dir("both"), "--adv_epsilon", "0.5", "--rdrop_alpha", "1.0",
                                                 "--ema_decay", "0.9"], caplog)
        assert len(both) == 2 and all(math.isfinite(v) and v > 0 for v in both)
        assert any("adv_epsilon 0.5" in line for line in lines2) and any("rdrop_alpha 1" in line for line in lines2)
        assert _loads_finite(os.path.join(out_dir("both"), checkpoint))


def test_finetune_driver(tmp_path, dev, caplog):
    import run_multimodal_fcmf as drv
    base = ["--pretrained_hf_model", make_hf_dir(synth.TINY_CFG), "--do_train", "--num_imgs", "2", "--num_rois", "5",
            "--train_batch_size", "4", "--gradient_accumulation_steps", "1", "--synthetic_steps", "11", "--max_seq_length", "16",
            "--seed", "3", "--num_train_epochs", "1"]
    _check(drv, "fcmf", base, lambda tag: str(tmp_path / tag), "seed_3_fcmf_model_last.pth", caplog, combined=True)


def test_baseline_driver(tmp_path, dev, caplog):
    import run_baselines as drv
    base = ["--model", "ef_captr", "--pretrained_hf_model", make_hf_dir(synth.TINY_CFG), "--do_train", "--train_batch_size", "4",
            "--synthetic_steps", "11", "--max_len", "16", "--seed", "3", "--num_train_epochs", "1"]
    _check(drv, "baselines", base, lambda tag: str(tmp_path / tag), "seed_3_ef_captr_model_last.pth", caplog)


def test_pretraining_driver(tmp_path, dev, caplog):
    import run_pretraining_fcmf as drv
    base = ["--pretrained_hf_model", make_hf_dir(synth.TINY_CFG), "--do_train", "--num_imgs", "2", "--num_rois", "5",
            "--train_batch_size", "3", "--synthetic_steps", "11", "--synthetic_dec_len", "6", "--num_train_epochs", "1", "--seed", "5"]
    _check(drv, "iaog", base, lambda tag: str(tmp_path / tag), "seed_5_iaog_model_last.pth", caplog)
