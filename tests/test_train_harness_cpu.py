"""train_harness.py, the code the two training drivers share, on the CPU: the call order of one epoch, the extractor
checkpoints beside the model's and their path rewrite, the synthetic pixel crops, the fine-tune parameter groups."""
import os

import pytest
import torch

from helpers import make_hf_dir
import synthetic_data as synth
import train_harness as H


class Recorder:
    """stand-ins for arena / reducer / optimizer / scheduler that write what is done to them into one list"""

    def __init__(self):
        self.calls = []
        rec = self

        class Arena:
            def zero(self):
                rec.calls.append("zero")

        class Reducer:
            def __setattr__(self, name, value):
                rec.calls.append(f"{name}={value}")

            def finish(self):
                rec.calls.append("finish")

        class Optimizer:
            def step(self, **kw):
                rec.calls.append("step(" + ", ".join(f"{k}={v}" for k, v in kw.items()) + ")")

        class Scheduler:
            def step(self):
                rec.calls.append("sched")

        self.arena, self.reducer, self.optimizer, self.scheduler = Arena(), Reducer(), Optimizer(), Scheduler()


BOUNDARY = ["finish", "step(max_grad_norm=1.0)", "sched", "zero"]


def test_train_epoch_call_order_and_loss_scaling():
    r = Recorder()
    w = torch.nn.Parameter(torch.tensor(1.0))
    grads = []

    def loss_fn(batch):
        grads.append(None if w.grad is None else float(w.grad))       # what the backwards so far have left
        r.calls.append(f"loss({batch})")
        return w * batch

    H.train_epoch([1.0, 2.0, 3.0, 4.0, 5.0], loss_fn, arena=r.arena, reducer=r.reducer, optimizer=r.optimizer,
                  scheduler=r.scheduler, accum=2)
    assert r.calls == (["zero", "loss(1.0)", "enabled=False", "loss(2.0)", "enabled=True"] + BOUNDARY +
                       ["loss(3.0)", "enabled=False", "loss(4.0)", "enabled=True"] + BOUNDARY +
                       ["loss(5.0)", "enabled=False"])                                   # nothing after step 4's backward
    # d(w * batch / 2)/dw = batch / 2 per step, boundary or not (the stand-in arena does not clear w.grad, so it adds up)
    assert grads == [None, 0.5, 1.5, 3.0, 5.0] and float(w.grad) == 7.5


def test_train_epoch_every_step_a_boundary_without_accumulation_and_the_log():
    r = Recorder()
    w = torch.nn.Parameter(torch.tensor(2.0))
    H.train_epoch([1.0, 2.0, 3.0], lambda b: w * b, arena=r.arena, reducer=None, optimizer=r.optimizer, scheduler=r.scheduler, accum=1)
    assert r.calls == ["zero"] + 3 * BOUNDARY[1:] and float(w.grad) == 6.0              # (no reducer: no `enabled`, no `finish`)
    for accum in (1, 3):
        r, logged = Recorder(), []
        H.train_epoch([float(i) for i in range(12)], lambda b: w * b, arena=r.arena, reducer=r.reducer, optimizer=r.optimizer,
                      scheduler=r.scheduler, accum=accum, log=lambda step, loss: logged.append((step, loss)))
        assert [s for s, _ in logged] == [0, 10]
        assert logged[0][1] == 0.0 and logged[1][1] == pytest.approx(20.0, rel=1e-6)    # the undivided loss w * batch
        assert r.calls.count("sched") == 12 // accum


def _extractors(seed):
    torch.manual_seed(seed)
    return torch.nn.Linear(3, 2), torch.nn.Linear(4, 2)


def test_extractor_checkpoints_beside_the_model(tmp_path):
    from fcmf_framework import ops
    d = tmp_path / "runs" / "fcmf"
    d.mkdir(parents=True)
    img, roi = _extractors(0)
    opt = torch.optim.SGD(list(img.parameters()) + list(roi.parameters()), lr=0.1)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: 1.0)
    H.save_extractors(str(d), 1, "last", img, roi, opt, sched, 3)
    assert sorted(os.listdir(d)) == ["seed_1_resimg_model_last.pth", "seed_1_resroi_model_last.pth"]
    ck = torch.load(d / "seed_1_resimg_model_last.pth", weights_only=True)
    assert set(ck) == {"epoch", "best_score", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict"}
    assert ck["epoch"] == 3 and ck["best_score"] == 0.0 and set(ck["model_state_dict"]) == {"weight", "bias"}
    want = [str(d / "seed_1_resimg_model_last.pth"), str(d / "seed_1_resroi_model_last.pth")]
    for name, kw in (("seed_1_fcmf_model_last.pth", dict(old="fcmf_model")), ("seed_1_fcmf_model_last.pth", dict(old="fcmf", strict=False)),
                     ("seed_1_iaog_model_last.pth", dict(old="iaog_model")), ("seed_1_fcmf_model_last.pth", {})):
        img2, roi2 = _extractors(1)
        assert not torch.equal(img2.weight, img.weight)
        ops.shadows.derived(img2.weight, "stale", torch.clone)
        got = H.load_resnets(str(d / name), img2, roi2, "cpu", **kw)
        assert got == want, (name, kw, got)                  # image first; the directory `runs/fcmf` keeps its name
        assert torch.equal(img2.weight, img.weight) and torch.equal(roi2.bias, roi.bias)
        assert len(ops.shadows) == 0                         # cached copies of the old weights are dropped
    # nothing to load: an extractor that is None, or no file beside the checkpoint
    img2, roi2 = _extractors(1)
    before = img2.weight.detach().clone()
    kept = ops.shadows.derived(img2.weight, "kept", torch.clone)
    try:
        assert H.load_resnets(str(d / "seed_1_fcmf_model_last.pth"), None, None, "cpu") == []
        assert H.load_resnets(str(d / "seed_2_fcmf_model_last.pth"), img2, roi2, "cpu") == []
        assert H.load_resnets(str(tmp_path / "runs" / "seed_1_fcmf_model_last.pth"), img2, roi2, "cpu") == []
        assert torch.equal(img2.weight, before) and len(ops.shadows) == 1 and ops.shadows.lookup("derived", img2.weight, "kept").payload is kept
        assert H.load_resnets(str(d / "seed_1_fcmf_model_last.pth"), None, roi2, "cpu") == want[1:]
    finally:
        ops.shadows.clear()
    H.save_extractors(str(tmp_path), 1, "best", None, None, opt, sched, 0)
    assert sorted(os.listdir(tmp_path)) == ["runs"]


def test_synth_pixel_batch_is_the_two_seeded_crop_draws():
    seed = 11
    vis, roi = synth.synth_pixel_batch(2, 2, 3, 16, seed, torch.float64)
    assert vis.shape == (2, 2, 3, 16, 16) and vis.dtype == torch.float32
    assert roi.shape == (2, 2, 3, 3, 16, 16) and roi.dtype == torch.float64
    assert torch.equal(vis, synth.synth_crops(4, 16, seed=seed).view(2, 2, 3, 16, 16))
    assert torch.equal(roi, synth.synth_crops(12, 16, seed=seed + 7919).view(2, 2, 3, 3, 16, 16).double())
    assert synth.synth_pixel_batch(2, 2, 3, 16, seed, torch.float32)[1].dtype == torch.float32
    from run_multimodal_fcmf import SyntheticBatches
    cfgd = dict(vocab_size=synth.TINY_CFG["vocab_size"], pad_token_id=synth.TINY_CFG["pad_token_id"])
    first = next(iter(SyntheticBatches(cfgd, 2, 2, 16, 2, 3, 6, seed, pixels=16)))
    assert torch.equal(first[0], vis) and first[1].dtype == torch.float64 and torch.equal(first[1], roi)


def test_finetune_param_groups_are_the_four_substring_groups():
    import run_multimodal_fcmf as drv
    from fcmf_framework.fcmf_multimodal import FCMF
    hf = make_hf_dir(synth.TINY_CFG)
    model = FCMF(pretrained_path=hf, num_labels=4, num_imgs=2, num_roi=3)
    for p in model.encoder.text2img_pooler.parameters():
        p.requires_grad = False                              # (frozen parameters are in no group)
    args = drv.build_parser().parse_args(["--output_dir", "o", "--pretrained_hf_model", hf, "--encoder_learning_rate", "3e-5",
                                          "--classifier_head_learning_rate", "2e-4"])
    groups = drv.param_groups(model, args)
    is_head = lambda n: any(s in n for s in ("classifier", "text_pooler"))
    no_decay = lambda n: any(s in n for s in ("bias", "LayerNorm.bias", "LayerNorm.weight"))
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    assert len(groups) == 4
    for g, (head, nd) in zip(groups, ((False, False), (False, True), (True, False), (True, True))):
        want = [p for n, p in named if is_head(n) == head and no_decay(n) == nd]
        assert len(want) > 0 and len(g["params"]) == len(want) and all(a is b for a, b in zip(g["params"], want))
        assert g["lr"] == (2e-4 if head else 3e-5) and g["weight_decay"] == (0.0 if nd else 0.01)
        assert set(g) == {"params", "weight_decay", "lr"}
    assert sum(len(g["params"]) for g in groups) == len(named) < len(list(model.parameters()))
