"""The training drivers with the loss options, end to end on the GPU in synthetic mode (tiny text encoder), after
tests/test_drivers_gpu.py: two steps run, the logged loss is finite, the weights land in class_weights.json."""
import json
import logging
import math
import os
import re

import numpy as np
import pytest
import torch

from helpers import make_hf_dir
import synthetic_data as synth

pytestmark = pytest.mark.gpu


def _logged_losses(caplog):
    return [float(m.group(1)) for r in caplog.records for m in [re.search(r"step \d+ loss (\S+)", r.getMessage())] if m]


def _finite_checkpoint(path):
    sd = torch.load(path, map_location="cpu", weights_only=True)["model_state_dict"]
    return all(torch.isfinite(v).all() for v in sd.values() if v.is_floating_point())


@pytest.mark.parametrize("extra", [["--label_smoothing", "0.1"], ["--focal_gamma", "2"]])
def test_finetune_driver_balanced_weights(tmp_path, dev, caplog, extra):
    import run_multimodal_fcmf as drv
    from fcmf_framework import ops
    from train_harness import balanced_class_weights
    hf = make_hf_dir(synth.TINY_CFG)
    out = str(tmp_path / "ft")
    try:
        with caplog.at_level(logging.INFO, logger="fcmf"):
            drv.main(["--output_dir", out, "--pretrained_hf_model", hf, "--do_train", "--num_imgs", "2", "--num_rois", "5",
                      "--train_batch_size", "4", "--gradient_accumulation_steps", "1", "--synthetic_steps", "2", "--max_seq_length", "16",
                      "--seed", "3", "--num_train_epochs", "1", "--class_weights", "balanced"] + extra)
    finally:
        ops.set_compute_dtype(torch.float32)
    losses = _logged_losses(caplog)
    assert losses and all(math.isfinite(v) and v > 0 for v in losses)
    assert _finite_checkpoint(os.path.join(out, "seed_3_fcmf_model_last.pth"))
    # the expected array: N / (C * max(count, 1)) per aspect over the two synthetic batches' labels (seeds 3 and 4)
    labels = np.concatenate([synth.synth_batch(4, synth.TINY_CFG, S=16, num_imgs=2, num_roi=5, seed=3 + i)["labels"].numpy() for i in range(2)])
    counts = np.stack([np.bincount(labels[:, a], minlength=4) for a in range(6)])
    want = (8 / (4 * np.maximum(counts, 1))).astype(np.float32)
    assert np.array_equal(want, balanced_class_weights(labels, 4))
    got = json.load(open(os.path.join(out, "class_weights.json")))
    assert got["mode"] == "balanced" and np.array_equal(np.asarray(got["weights"], dtype=np.float32), want)


def test_finetune_driver_listed_weights(tmp_path, dev, caplog):
    import run_baselines as drv
    from fcmf_framework import ops
    hf = make_hf_dir(synth.TINY_CFG)
    out = str(tmp_path / "bl")
    try:
        with caplog.at_level(logging.INFO, logger="baselines"):
            drv.main(["--model", "ef_captr", "--output_dir", out, "--pretrained_hf_model", hf, "--do_train", "--train_batch_size", "4",
                      "--synthetic_steps", "2", "--max_len", "16", "--seed", "3", "--num_train_epochs", "1",
                      "--class_weights", "0.5,2,1,1.5", "--label_smoothing", "0.05"])
    finally:
        ops.set_compute_dtype(torch.float32)
        ops.set_ffn_dropout(False)
    losses = _logged_losses(caplog)
    assert losses and all(math.isfinite(v) and v > 0 for v in losses)
    got = json.load(open(os.path.join(out, "class_weights.json")))
    assert got == {"mode": "list", "weights": [0.5, 2.0, 1.0, 1.5]}


def test_pretraining_driver_label_smoothing(tmp_path, dev, caplog):
    import run_pretraining_fcmf as drv
    from fcmf_framework import ops
    hf = make_hf_dir(synth.TINY_CFG)
    out = str(tmp_path / "pt")
    try:
        with caplog.at_level(logging.INFO, logger="iaog"):
            drv.main(["--output_dir", out, "--pretrained_hf_model", hf, "--do_train", "--num_imgs", "2", "--num_rois", "5",
                      "--train_batch_size", "3", "--synthetic_steps", "2", "--synthetic_dec_len", "6", "--num_train_epochs", "1",
                      "--seed", "5", "--label_smoothing", "0.1"])
    finally:
        ops.set_compute_dtype(torch.float32)
    losses = _logged_losses(caplog)
    assert losses and all(math.isfinite(v) and v > 0 for v in losses)
    assert _finite_checkpoint(os.path.join(out, "seed_5_iaog_model_last.pth"))
    assert not os.path.exists(os.path.join(out, "class_weights.json"))
