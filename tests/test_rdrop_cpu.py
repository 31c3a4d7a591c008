"""R-Drop without a GPU: the closed form of the symmetric KL and its two gradient formulas (include/fcmf_hip.h) against torch's
F.kl_div statement and its autograd in float64 (tests/symkl_ref.py), the drivers' --rdrop_alpha flag (accepted with every
existing loss option, refused before anything is written), and the refusals of the two C entry points, which return before
any launch and so can be asked with host buffers."""
import os

import numpy as np
import pytest
import torch

import symkl_ref as R


def _pair(n, C, seed, offset=0.0, noise=None):
    """two independent rows, or (noise given) b = a + noise * N(0, 1) + offset"""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(n, C, generator=g, dtype=torch.float64) * 2
    r = torch.randn(n, C, generator=g, dtype=torch.float64)
    b = r * 2 if noise is None else a + noise * r + offset
    return a.requires_grad_(True), b.requires_grad_(True)


@pytest.mark.parametrize("C", [1, 3, 4, 65, 1500])
@pytest.mark.parametrize("offset,noise", [(0.0, None), (8.0, 1e-2)])
def test_closed_form_is_the_kl_div_statement(C, offset, noise):
    """k = 1/2 sum (p - q) d and the stated dk/da, dk/db == F.kl_div in both directions and its autograd; a constant added to
    d = a - b changes none of them"""
    a, b = _pair(7, C, seed=C, offset=offset, noise=noise)
    want = R.rows(a, b)
    ga, gb = torch.autograd.grad(want.sum(), (a, b))
    # the statement's own float64 error: it subtracts log-softmax values of magnitude up to ~20 (eps 2.2e-16 each, p sums to 1),
    # i.e. ~1e-14 absolute whatever the size of k; 1e-13 leaves a factor of ten
    floor = 1e-13
    scale = want.abs().max().item()
    assert (R.closed_form(a, b).detach() - want.detach()).abs().max().item() <= 1e-11 * scale + floor
    fa, fb = R.closed_form_grads(a.detach(), b.detach())
    gscale = ga.abs().max().item()
    assert (fa - ga).abs().max().item() <= 1e-11 * gscale + floor and (fb - gb).abs().max().item() <= 1e-11 * gscale + floor
    shifted = R.closed_form(a.detach() + 3.0, b.detach())             # d + 3
    assert (shifted - want.detach()).abs().max().item() <= 1e-11 * scale + floor
    if C == 1:
        assert not want.detach().any() and not ga.any() and not gb.any()


def test_segment_mean_and_liveness():
    """pair r belongs to segment r % segments; a pair whose label is ignore_index is left out of numerator and count"""
    B, A, C = 5, 3, 4
    a, b = _pair(B * A, C, seed=9)
    lb = torch.zeros(B * A, dtype=torch.long)
    lb[4] = -100                                                      # segment 1, second pair
    k = R.rows(a, b).detach()
    want = 0.7 * (k[0::A].mean() + (k[1::A].sum() - k[4]) / (B - 1) + k[2::A].mean())
    got = R.loss(a, b, lb, alpha=0.7, segments=A)
    assert abs(got.item() - want.item()) < 1e-13 * want.item()
    ga, = torch.autograd.grad(got, a)
    assert not ga[4].any() and ga[3].any()
    assert torch.equal(R.loss(a.view(B, A, C), b.view(B, A, C), None, alpha=1.0, segments=1), k.mean())
    dead = lb.clone()
    dead[2::A] = -100
    assert torch.isnan(R.loss(a, b, dead, segments=A)).item()         # 0 / 0, as a cross entropy without a live row


def _drivers():
    import run_baselines
    import run_multimodal_fcmf
    import run_pretraining_fcmf
    return run_multimodal_fcmf, run_baselines, run_pretraining_fcmf


def test_all_three_parsers_know_the_flag():
    ft, bl, pt = _drivers()
    for drv, head in ((ft, ["--pretrained_hf_model", "x"]), (bl, ["--model", "mroberta"]), (pt, ["--pretrained_hf_model", "x"])):
        assert drv.build_parser().parse_args(["--output_dir", "o"] + head).rdrop_alpha == 0.0
        assert drv.build_parser().parse_args(["--output_dir", "o"] + head + ["--rdrop_alpha", "1.5"]).rdrop_alpha == 1.5
        text = " ".join(drv.build_parser().format_help().split())
        assert "--rdrop_alpha" in text and "BATCH MEAN" in text and "Activation memory doubles" in text
        assert "evaluation is untouched" in text


@pytest.mark.parametrize("alpha", ["0", "1.5"])
@pytest.mark.parametrize("option", [[], ["--label_smoothing", "0.1"], ["--focal_gamma", "2"], ["--class_weights", "balanced"],
                                    ["--class_weights", "1,2,0.5,4"]])
def test_check_accepts_the_flag_with_each_existing_option(alpha, option):
    from train_harness import check_loss_arguments
    ft, bl, pt = _drivers()
    want = None if "--class_weights" not in option else ("balanced" if option[1] == "balanced" else [1.0, 2.0, 0.5, 4.0])
    for drv, head in ((ft, ["--pretrained_hf_model", "x"]), (bl, ["--model", "mroberta"])):
        args = drv.build_parser().parse_args(["--output_dir", "o"] + head + option + ["--rdrop_alpha", alpha])
        assert check_loss_arguments(args) == want and args.rdrop_alpha == float(alpha)
    if option in ([], ["--label_smoothing", "0.1"]):
        args = pt.build_parser().parse_args(["--output_dir", "o", "--pretrained_hf_model", "x"] + option + ["--rdrop_alpha", alpha])
        assert check_loss_arguments(args) is None and args.rdrop_alpha == float(alpha)


@pytest.mark.parametrize("value", ["-1", "nan", "inf"])
def test_drivers_refuse_a_bad_rdrop_alpha_before_anything_is_written(tmp_path, value):
    from train_harness import check_loss_arguments
    ft, bl, pt = _drivers()
    runs = [(ft, ["--pretrained_hf_model", "x", "--do_train"]), (bl, ["--model", "mroberta", "--do_train"]),
            (pt, ["--pretrained_hf_model", "x", "--do_train"])]
    for i, (drv, head) in enumerate(runs):
        out = str(tmp_path / f"out{i}")
        argv = ["--output_dir", out] + head + ["--rdrop_alpha", value]
        with pytest.raises(ValueError, match="--rdrop_alpha"):
            check_loss_arguments(drv.build_parser().parse_args(argv))
        with pytest.raises(ValueError, match="--rdrop_alpha"):
            drv.main(argv)
        assert not os.path.exists(out)


def test_ops_refuse_bad_values_by_name():
    from fcmf_framework import ops
    a = torch.zeros(4, 3)
    for kw, named in ((dict(alpha=-1.0), "alpha"), (dict(alpha=float("nan")), "alpha"), (dict(alpha=float("inf")), "alpha"),
                      (dict(alpha="1"), "alpha"), (dict(segments=0), "segments"), (dict(segments=1.0), "segments")):
        with pytest.raises(ValueError, match=named):
            ops.symmetric_kl(a, a, **kw)
    for bad in (-0.5, float("nan")):
        with pytest.raises(ValueError, match="rdrop_alpha"):
            ops.vocab_cross_entropy(torch.zeros(2, 3, 4), torch.zeros(9, 4), None, torch.zeros(3, dtype=torch.long), rdrop_alpha=bad)


def test_entry_points_refuse_before_any_launch():
    """FCMF_ERR_ARG (-1) / FCMF_ERR_UNSUPPORTED (-3) on host buffers: a call that launched would fail otherwise"""
    from fcmf_framework import _hip as H
    L = H.lib()
    n, C = 6, 5
    a, b = np.zeros((n, C), np.float32), np.zeros((n, C), np.float32)
    da, db = np.zeros((n, C), np.float32), np.zeros((n, C), np.float32)
    lb, num, den, sc = np.zeros(n, np.int64), np.zeros(n, np.float32), np.zeros(n, np.float32), np.ones(n, np.float32)
    P = lambda t: t.ctypes.data

    def fwd(a_=P(a), b_=P(b), labels=P(lb), num_=P(num), den_=P(den), n_=n, C_=C, seg=1, dt=H.F32, lda=C, ldb=C):
        return L.fcmf_symkl_fwd(a_, lda, b_, ldb, labels, num_, den_, n_, C_, seg, -100, dt, None)

    def bwd(a_=P(a), b_=P(b), labels=P(lb), da_=P(da), db_=P(db), scales=P(sc), n_=n, C_=C, seg=1, dt=H.F32, lda=C, ldb=C, ldda=C,
            lddb=C, acc=0):
        return L.fcmf_symkl_bwd(a_, lda, b_, ldb, labels, da_, ldda, db_, lddb, scales, None, n_, C_, seg, -100, acc, dt, None)

    for call in (fwd, bwd):
        assert call(a_=None) == H.ERR_ARG and call(b_=None) == H.ERR_ARG
        assert call(seg=0) == H.ERR_ARG and call(seg=-2) == H.ERR_ARG
        assert call(seg=4) == H.ERR_ARG                       # 6 pairs do not divide into 4 segments
        assert call(lda=C - 1) == H.ERR_ARG and call(ldb=C - 1) == H.ERR_ARG
        assert call(dt=H.F64) == H.ERR_UNSUPPORTED
        assert call(C_=0) == H.ERR_ARG and call(n_=-1) == H.ERR_ARG
        assert call(n_=0) == 0 and call(n_=0, labels=None) == 0       # nothing to do: no launch either
    assert fwd(num_=None) == H.ERR_ARG and fwd(den_=None) == H.ERR_ARG
    assert bwd(da_=None) == H.ERR_ARG and bwd(db_=None) == H.ERR_ARG and bwd(scales=None) == H.ERR_ARG
    assert bwd(ldda=C - 1) == H.ERR_ARG and bwd(lddb=C - 1) == H.ERR_ARG
    assert bwd(acc=2) == H.ERR_ARG and bwd(acc=-1) == H.ERR_ARG
    # the destinations may not be the logits, nor overlap them or each other
    assert bwd(da_=P(a)) == H.ERR_ARG and bwd(db_=P(b)) == H.ERR_ARG and bwd(da_=P(b)) == H.ERR_ARG and bwd(db_=P(a)) == H.ERR_ARG
    assert bwd(da_=P(a) + 4 * C) == H.ERR_ARG and bwd(db_=P(da)) == H.ERR_ARG
