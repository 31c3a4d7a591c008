"""The training loss's options without a GPU: the float64 reference against torch's own criterion, the `balanced` class weights by
hand, the drivers' flags (accepted, and refused before anything is written) and the C entry points' refusals, which return before
any launch and so can be asked with host buffers."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_ref as R


def _case(n, C, segments, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(n, C, generator=g, dtype=torch.float64) * 2).requires_grad_(True)
    y = torch.randint(0, C, (n,), generator=g)
    y[1] = -100
    y[2] = C - 1
    return x, y, torch.rand(C, generator=g, dtype=torch.float64) + 0.5, torch.rand(segments, C, generator=g, dtype=torch.float64) + 0.5


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("weighted", [False, True])
def test_formula_is_torch_cross_entropy(eps, weighted):
    """the stated function at gamma = 0 is F.cross_entropy(weight=, label_smoothing=, ignore_index=), value and gradient"""
    x, y, w, _ = _case(24, 5, 1)
    w = w if weighted else None
    got = R.loss_formula(x, y, w, eps=eps)
    g_got, = torch.autograd.grad(got, x)
    want = F.cross_entropy(x, y, weight=w, label_smoothing=eps, ignore_index=-100)
    g_want, = torch.autograd.grad(want, x)
    assert abs(got.item() - want.item()) < 1e-13 * abs(want.item())
    assert (g_got - g_want).abs().max().item() < 1e-15
    assert torch.equal(R.loss_ref(x, y, w, eps=eps), want)


def test_segments_are_per_aspect_criteria():
    """row r belongs to segment r % segments: [B, A, C] logits flattened, one criterion per aspect with its own weight row"""
    B, A, C = 8, 3, 4
    x, y, _, w = _case(B * A, C, A, seed=1)
    want = sum(F.cross_entropy(x.view(B, A, C)[:, a], y.view(B, A)[:, a], weight=w[a], label_smoothing=0.1) for a in range(A))
    for f in (R.loss_ref, R.loss_formula):
        assert abs(f(x, y, w, eps=0.1, segments=A).item() - want.item()) < 1e-13 * abs(want.item())
    assert abs(R.loss_ref(x, y, w, eps=0.1, segments=A, mult=2.0).item() - 2 * want.item()) < 1e-12


def test_focal_gradient_is_the_stated_one():
    """d/dx_j = w_y [gamma p_y (1 - p_y)^(gamma - 1) log p_y - (1 - p_y)^gamma] ([j == y] - p_j) / D"""
    x, y, w, _ = _case(12, 5, 1, seed=2)
    for gamma in (2.0, 0.5):
        g, = torch.autograd.grad(R.loss_ref(x, y, w, gamma=gamma), x)
        p = F.softmax(x.detach(), 1)
        live = y != -100
        yy = torch.where(live, y, torch.zeros_like(y))
        py, wy = p.gather(1, yy[:, None])[:, 0], w[yy]
        k = wy * (gamma * py * (1 - py) ** (gamma - 1) * py.log() - (1 - py) ** gamma)
        want = k[:, None] * (F.one_hot(yy, 5) - p) / wy[live].sum() * live[:, None]
        assert (g - want).abs().max().item() < 1e-14


def test_balanced_weights_by_hand():
    """w[a, c] = N / (C * max(count[a, c], 1)); aspect 1 never shows class 2"""
    from train_harness import balanced_class_weights
    labels = np.array([[0, 0], [0, 1], [0, 1], [1, 1], [2, 0], [0, 0]])
    w = balanced_class_weights(labels, 3)
    assert w.dtype == np.float32 and w.shape == (2, 3)
    want = np.array([[6 / (3 * 4), 6 / (3 * 1), 6 / (3 * 1)], [6 / (3 * 3), 6 / (3 * 3), 6 / (3 * 1)]], dtype=np.float32)
    assert np.array_equal(w, want)
    with pytest.raises(ValueError):
        balanced_class_weights(np.array([[0, 3]]), 3)


def test_train_label_table_reads_the_batches():
    from train_harness import train_label_table
    batches = [(None, torch.tensor([[0, 1], [2, 3]]), ["a", "b"]), (None, torch.tensor([[1, 1]]), ["c"])]
    assert np.array_equal(train_label_table(batches), np.array([[0, 1], [2, 3], [1, 1]]))


def _drivers():
    import run_baselines
    import run_multimodal_fcmf
    import run_pretraining_fcmf
    return run_multimodal_fcmf, run_baselines, run_pretraining_fcmf


def test_parsers_accept_the_loss_flags():
    from train_harness import check_loss_arguments
    ft, bl, pt = _drivers()
    for drv, head in ((ft, ["--pretrained_hf_model", "x"]), (bl, ["--model", "mroberta"])):
        args = drv.build_parser().parse_args(["--output_dir", "o"] + head + ["--class_weights", "balanced", "--label_smoothing", "0.1"])
        assert check_loss_arguments(args) == "balanced" and args.label_smoothing == 0.1 and args.focal_gamma == 0.0
        args = drv.build_parser().parse_args(["--output_dir", "o"] + head + ["--class_weights", "1,2,0.5,4", "--focal_gamma", "2"])
        assert check_loss_arguments(args) == [1.0, 2.0, 0.5, 4.0] and args.focal_gamma == 2.0
        args = drv.build_parser().parse_args(["--output_dir", "o"] + head)
        assert check_loss_arguments(args) is None and args.label_smoothing == 0.0 and args.focal_gamma == 0.0
        assert "plain cross entropy" in drv.build_parser().format_help()
    args = pt.build_parser().parse_args(["--output_dir", "o", "--pretrained_hf_model", "x", "--label_smoothing", "0.1"])
    assert args.label_smoothing == 0.1 and not hasattr(args, "class_weights")
    assert "plain cross entropy" in pt.build_parser().format_help()


@pytest.mark.parametrize("flags,named", [
    (["--label_smoothing", "1.0"], "--label_smoothing"), (["--label_smoothing", "-0.1"], "--label_smoothing"),
    (["--label_smoothing", "nan"], "--label_smoothing"), (["--focal_gamma", "-1"], "--focal_gamma"),
    (["--focal_gamma", "inf"], "--focal_gamma"), (["--focal_gamma", "2", "--label_smoothing", "0.1"], "--focal_gamma"),
    (["--class_weights", "1,2,3"], "--class_weights"), (["--class_weights", "1,2,x,4"], "--class_weights"),
    (["--class_weights", "1,-2,3,4"], "--class_weights"), (["--class_weights", "heavy"], "--class_weights")])
def test_drivers_refuse_bad_loss_flags_before_anything_is_written(tmp_path, flags, named):
    ft, bl, pt = _drivers()
    runs = [(ft, ["--pretrained_hf_model", "x", "--do_train"]), (bl, ["--model", "mroberta", "--do_train"])]
    if all(f in ("--label_smoothing",) or not f.startswith("--") for f in flags):
        runs.append((pt, ["--pretrained_hf_model", "x", "--do_train"]))
    for i, (drv, head) in enumerate(runs):
        out = str(tmp_path / f"out{i}")
        with pytest.raises(ValueError, match=named):
            drv.main(["--output_dir", out] + head + flags)
        assert not os.path.exists(out)
    with pytest.raises(SystemExit):           # the pre-training driver has no class-weight / focal flag at all
        pt.build_parser().parse_args(["--output_dir", "o", "--pretrained_hf_model", "x", "--focal_gamma", "2"])


def test_ops_refuse_bad_values_by_name():
    from fcmf_framework import ops
    x, y = torch.zeros(4, 3), torch.zeros(4, dtype=torch.long)
    for kw, named in ((dict(label_smoothing=1.0), "label_smoothing"), (dict(label_smoothing=-0.5), "label_smoothing"),
                      (dict(focal_gamma=-1.0), "focal_gamma"), (dict(focal_gamma=2.0, label_smoothing=0.1), "focal_gamma"),
                      (dict(segments=0), "segments")):
        with pytest.raises(ValueError, match=named):
            ops.cross_entropy(x, y, **kw)
    with pytest.raises(ValueError, match="label_smoothing"):
        ops.vocab_cross_entropy(torch.zeros(2, 3, 4), torch.zeros(9, 4), None, torch.zeros(2, 3, dtype=torch.long), label_smoothing=1.5)


def test_entry_points_refuse_before_any_launch():
    """FCMF_ERR_ARG (-1) / FCMF_ERR_UNSUPPORTED (-3) on host buffers: a call that launched would fail otherwise"""
    from fcmf_framework import _hip as H
    L = H.lib()
    n, C = 6, 5
    lg, lb = np.zeros((n, C), np.float32), np.zeros(n, np.int64)
    w, num, den, d = np.ones(C, np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros((n, C), np.float32)
    out = np.zeros(4, np.float32)
    P = lambda a: a.ctypes.data

    def fwd(logits=P(lg), labels=P(lb), weight=P(w), wstride=0, num_=P(num), den_=P(den), n_=n, C_=C, seg=1, eps=0.0, gamma=0.0, dt=H.F32, ld=C):
        return L.fcmf_xent_fwd_ex(logits, ld, labels, weight, wstride, num_, den_, n_, C_, seg, -100, eps, gamma, dt, None)

    def bwd(logits=P(lg), labels=P(lb), dl=P(d), scales=P(out), n_=n, C_=C, seg=1, eps=0.0, gamma=0.0, dt=H.F32, ldd=C):
        return L.fcmf_xent_bwd_ex(logits, C, labels, P(w), 0, dl, ldd, scales, None, n_, C_, seg, -100, eps, gamma, dt, None)

    for call in (fwd, bwd):
        assert call(logits=None) == H.ERR_ARG and call(labels=None) == H.ERR_ARG
        assert call(seg=0) == H.ERR_ARG and call(seg=-2) == H.ERR_ARG
        assert call(seg=4) == H.ERR_ARG                       # 6 rows do not divide into 4 segments
        assert call(eps=1.0) == H.ERR_ARG and call(eps=-0.25) == H.ERR_ARG and call(eps=float("nan")) == H.ERR_ARG
        assert call(gamma=-1.0) == H.ERR_ARG and call(gamma=float("inf")) == H.ERR_ARG
        assert call(eps=0.1, gamma=2.0) == H.ERR_UNSUPPORTED
        assert call(dt=H.F64) == H.ERR_UNSUPPORTED
        assert call(C_=0) == H.ERR_ARG and call(n_=-1) == H.ERR_ARG
        assert call(n_=0) == 0                                # nothing to do: no launch either
    assert fwd(num_=None) == H.ERR_ARG and fwd(den_=None) == H.ERR_ARG
    assert fwd(ld=C - 1) == H.ERR_ARG and fwd(wstride=C - 1, seg=2) == H.ERR_ARG
    assert bwd(dl=None) == H.ERR_ARG and bwd(scales=None) == H.ERR_ARG and bwd(ldd=C - 1) == H.ERR_ARG
    red = lambda num_=P(num), den_=P(den), n_=n, seg=1, loss=P(out), scales=P(out) + 4: \
        L.fcmf_xent_reduce_ex(num_, den_, n_, seg, 1.0, loss, scales, None)
    assert red(num_=None) == H.ERR_ARG and red(den_=None) == H.ERR_ARG and red(loss=None) == H.ERR_ARG and red(scales=None) == H.ERR_ARG
    assert red(seg=0) == H.ERR_ARG and red(seg=4) == H.ERR_ARG and red(n_=-1) == H.ERR_ARG
