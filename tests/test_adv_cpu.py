"""FGM adversarial training on the text embeddings, without a GPU: header, binding and entry-point count agree; the two C entry
points refuse before any launch (so they can be asked with host buffers); the three drivers' --adv_epsilon flag; the float64
reference itself (tests/adv_ref.py): the perturbation has norm epsilon over every sequence's live tokens, is 0 at pads, and
raises a loss by epsilon * sum_s ||g_s|| to first order; the record / attack protocol errors that need no device."""
import math
import os
import re

import numpy as np
import pytest
import torch

import adv_ref as A
from conftest import ROOT


# ---- header, binding, count -----------------------------------------------------------------------------------------------------
def _header():
    return open(os.path.join(ROOT, "include", "fcmf_hip.h")).read()


def test_header_binding_and_count_agree():
    from fcmf_framework import _hip as H
    src = _header()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("fcmf_adv_scale", "fcmf_embed_ln_adv_fwd"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m, name
        assert len(m.group(1).split(",")) == len(H.SIGNATURES[name])
        assert hasattr(H.lib(), name)
    plain = re.search(r"\bint\s+fcmf_embed_ln_fwd\s*\(([^)]*)\)\s*;", code).group(1)
    adv = re.search(r"\bint\s+fcmf_embed_ln_adv_fwd\s*\(([^)]*)\)\s*;", code).group(1)
    squash = lambda s: " ".join(s.split())
    assert squash(adv).startswith(squash(plain) + ",")               # the plain entry point's arguments, then the four new ones
    assert H.SIGNATURES["fcmf_embed_ln_adv_fwd"][:len(H.SIGNATURES["fcmf_embed_ln_fwd"])] == H.SIGNATURES["fcmf_embed_ln_fwd"]
    assert len(H.SIGNATURES) == 99 and H.lib().fcmf_abi_version() == 4
    for doc in ("README.md", "DESIGN.md"):
        assert re.search(r"\b99\s+(?:`extern \"C\"`\s+)?entry points", open(os.path.join(ROOT, doc)).read()), doc
    text = " ".join(src.split())
    assert "scale[s] = epsilon /" in text and "ids[s, t] != pad_id" in text and "never materialised" in text


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_before_any_launch():
    """FCMF_ERR_ARG (-1) / FCMF_ERR_UNSUPPORTED (-3) / FCMF_OK for nothing to do, on host buffers: a call that launched would
    fail otherwise"""
    from fcmf_framework import _hip as H
    L = H.lib()
    nseq, S, Hd = 2, 3, 8
    ntok = nseq * S
    dz = np.zeros((ntok, Hd), np.float32)
    ids = np.zeros(ntok, np.int64)
    sc = np.zeros(nseq, np.float32)
    P = lambda t: t.ctypes.data
    assert P(dz) % 16 == 0

    def scale(dz_=P(dz), ids_=P(ids), sc_=P(sc), n=nseq, S_=S, H_=Hd, eps=1.0, dt=H.F32):
        return L.fcmf_adv_scale(dz_, ids_, sc_, n, S_, H_, 1, eps, dt, None)

    assert scale(dz_=None) == H.ERR_ARG and scale(ids_=None) == H.ERR_ARG and scale(sc_=None) == H.ERR_ARG
    assert scale(S_=0) == H.ERR_ARG and scale(S_=-1) == H.ERR_ARG
    assert scale(n=-1) == H.ERR_ARG and scale(H_=-4) == H.ERR_ARG
    for bad in (-0.5, float("nan"), float("inf"), -float("inf")):
        assert scale(eps=bad) == H.ERR_ARG
    assert scale(H_=6) == H.ERR_UNSUPPORTED and scale(H_=7) == H.ERR_UNSUPPORTED
    assert scale(dt=H.F64) == H.ERR_UNSUPPORTED and scale(dt=7) == H.ERR_UNSUPPORTED
    assert scale(dz_=P(dz) + 4) == H.ERR_UNSUPPORTED                 # a float32 gradient off its 16-byte boundary
    assert scale(n=0) == 0 and scale(n=0, eps=0.0) == 0

    tab = np.zeros((4, Hd), np.float32)
    gb = np.zeros(Hd, np.float32)
    y, z = np.zeros((ntok, Hd), np.float32), np.zeros((ntok, Hd), np.float32)
    mean, rstd = np.zeros(ntok, np.float32), np.zeros(ntok, np.float32)

    def fwd(ids_=P(ids), pos=P(ids), tt=P(ids), word=P(tab), ptab=P(tab), ttab=P(tab), gamma=P(gb), beta=P(gb), y_=P(y), z_=P(z),
            mean_=P(mean), rstd_=P(rstd), n=ntok, H_=Hd, dt=H.F32, g=P(dz), sc_=P(sc), S_=S):
        return L.fcmf_embed_ln_adv_fwd(ids_, pos, tt, word, ptab, ttab, gamma, beta, y_, z_, mean_, rstd_, n, H_, 1e-5, 0.0, 0, dt,
                                       None, g, sc_, S_, 1)

    for name in ("ids_", "pos", "word", "ptab", "ttab", "gamma", "beta", "y_", "mean_", "rstd_", "g", "sc_"):
        assert fwd(**{name: None}) == H.ERR_ARG, name
    assert fwd(S_=0) == H.ERR_ARG and fwd(S_=-3) == H.ERR_ARG
    assert fwd(n=-1) == H.ERR_ARG and fwd(H_=-8) == H.ERR_ARG
    assert fwd(S_=4) == H.ERR_ARG                                     # six tokens are not whole sequences of four
    assert fwd(H_=6) == H.ERR_UNSUPPORTED and fwd(H_=2052) == H.ERR_UNSUPPORTED
    assert fwd(dt=H.F64) == H.ERR_UNSUPPORTED
    assert fwd(g=P(dz) + 4) == H.ERR_UNSUPPORTED
    assert fwd(n=0) == 0 and fwd(n=0, tt=None, z_=None) == 0


# ---- the drivers' flag ------------------------------------------------------------------------------------------------------------
def _drivers():
    import run_baselines
    import run_multimodal_fcmf
    import run_pretraining_fcmf
    return ((run_multimodal_fcmf, ["--pretrained_hf_model", "x"]), (run_baselines, ["--model", "ef_captr"]),
            (run_pretraining_fcmf, ["--pretrained_hf_model", "x"]))


def test_all_three_parsers_know_the_flag():
    from train_harness import check_adv_arguments
    for drv, head in _drivers():
        args = drv.build_parser().parse_args(["--output_dir", "o"] + head)
        assert args.adv_epsilon == 0.0 and check_adv_arguments(args) == 0.0
        args = drv.build_parser().parse_args(["--output_dir", "o"] + head + ["--adv_epsilon", "0.5", "--rdrop_alpha", "1", "--ema_decay",
                                                                             "0.9", "--label_smoothing", "0.1"])
        assert check_adv_arguments(args) == 0.5
        text = " ".join(drv.build_parser().format_help().split())
        assert "--adv_epsilon" in text and "FGM" in text and "evaluation is untouched" in text
        assert "accuracy has not been measured" in text


@pytest.mark.parametrize("value", ["-1", "nan", "inf"])
def test_drivers_refuse_a_bad_epsilon_before_anything_is_written(tmp_path, value):
    from train_harness import check_adv_arguments
    for i, (drv, head) in enumerate(_drivers()):
        out = str(tmp_path / f"out{i}")
        argv = ["--output_dir", out] + head + ["--do_train", "--adv_epsilon", value]
        with pytest.raises(ValueError, match="--adv_epsilon"):
            check_adv_arguments(drv.build_parser().parse_args(argv))
        with pytest.raises(ValueError, match="--adv_epsilon"):
            drv.main(argv)
        assert not os.path.exists(out)


def test_epsilon_with_a_frozen_encoder_is_refused_up_front(tmp_path):
    import run_multimodal_fcmf as drv
    out = str(tmp_path / "out")
    argv = ["--output_dir", out, "--pretrained_hf_model", "x", "--do_train", "--freeze_encoder", "--adv_epsilon", "0.5"]
    with pytest.raises(ValueError, match="--adv_epsilon.*--freeze_encoder"):
        drv.main(argv)
    assert not os.path.exists(out)
    drv_args = drv.build_parser().parse_args(argv[:-2])               # frozen, epsilon 0: nothing to refuse
    from train_harness import check_adv_arguments
    assert check_adv_arguments(drv_args) == 0.0


# ---- the reference itself -------------------------------------------------------------------------------------------------------
def _case(nseq, S, H_, pad, seed):
    gen = torch.Generator().manual_seed(seed)
    ids = torch.randint(pad + 1, 40, (nseq, S), generator=gen)
    ids[0, S - 2:] = pad
    ids[1, 0] = pad
    ids[2, 1] = pad
    ids[3] = pad                                                      # nothing but pads
    g = torch.randn(nseq, S, H_, generator=gen, dtype=torch.float64)
    g[ids.eq(pad)] = float("nan")                                     # never read
    return ids, g


def test_reference_perturbation_has_norm_epsilon_and_is_zero_at_pads():
    pad, eps = 1, 0.37
    ids, g = _case(5, 6, 8, pad, seed=0)
    g[4] = 0.0                                                        # a zero gradient
    sc = A.scale(g, ids, pad, eps)
    d = A.perturbation(g, ids, pad, sc)
    assert torch.isfinite(d).all()
    assert not d[ids.eq(pad)].any()
    n = d.pow(2).sum((1, 2)).sqrt()
    for s in (0, 1, 2):
        assert abs(n[s].item() - eps) <= 4 * 2.0 ** -52 * eps         # one sqrt, one divide, one multiply per element
    assert sc[3] == 0 and sc[4] == 0 and n[3] == 0 and n[4] == 0
    # ids of any rank: the last axis is the sequence
    assert torch.equal(A.scale(g.view(5, 1, 6, 8), ids.view(5, 1, 6), pad, eps), sc)


def test_first_order_rise_of_a_tiny_model():
    """L(x + delta) - L(x) = eps * sum_s ||g_s|| + O(eps^2): halving eps twice must quarter the remainder each time (within the
    next order), on embed -> LayerNorm -> linear -> cross entropy in float64"""
    pad, V, S, nseq, H_ = 1, 30, 5, 4, 8
    gen = torch.Generator().manual_seed(3)
    ids = torch.randint(2, V, (nseq, S), generator=gen)
    ids[0, 3:] = pad
    ids[1, 0] = pad
    pos = (torch.cumsum(ids.ne(pad).long(), 1) * ids.ne(pad).long() + pad)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    word, ptab, ttab, gamma, beta, W = rnd(V, H_), rnd(S + 2, H_), rnd(2, H_), 1 + 0.1 * rnd(H_), rnd(H_), rnd(3, H_)
    labels = torch.randint(0, 3, (nseq,), generator=gen)

    def loss(delta):
        z = ((word[ids] + ttab[torch.zeros_like(ids)]) + ptab[pos]) + delta
        y = torch.nn.functional.layer_norm(z, (H_,), gamma, beta, 1e-5)
        return torch.nn.functional.cross_entropy(y[:, 0] @ W.t() + y.mean(1) @ W.t(), labels, reduction="sum")

    zero = torch.zeros(nseq, S, H_, dtype=torch.float64, requires_grad=True)
    base = loss(zero)
    g, = torch.autograd.grad(base, zero)
    gsum = A.norms(g, ids, pad).sum().item()
    rem = []
    for eps in (1e-2, 5e-3, 2.5e-3):
        d = A.perturbation(g, ids, pad, A.scale(g, ids, pad, eps))
        assert not d[ids.eq(pad)].any()
        rem.append((loss(d) - base).item() - eps * gsum)
    assert all(abs(r) < 1e-2 * eps * gsum for r, eps in zip(rem, (1e-2, 5e-3, 2.5e-3)))      # first order dominates
    for a, b in zip(rem, rem[1:]):
        assert 3.0 < a / b < 5.0                                      # a pure eps^2 term gives 4; the eps^3 term moves it a little


# ---- the protocol, no device ------------------------------------------------------------------------------------------------------
def test_adversary_refuses_bad_epsilons_and_an_attack_on_nothing():
    from fcmf_framework import ops
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="epsilon"):
            ops.EmbeddingAdversary(bad)
    adv = ops.EmbeddingAdversary(0.5)
    assert adv.epsilon == 0.5 and adv.recorded() == 0
    with adv.record():
        pass                                                          # a frozen or no-grad encoder: no call registers
    with pytest.raises(ValueError, match="must be trainable"):
        with adv.attack():
            pass
    assert ops._adversary is None                                     # the refused block did not stay active
    with adv.record():
        with pytest.raises(RuntimeError, match="do not nest"):
            with ops.EmbeddingAdversary(1.0).record():
                pass
    assert ops._adversary is None


def test_attack_checks_counts_shapes_and_the_deposited_gradient():
    """the mismatch errors are raised before any library call: host tensors reach them"""
    from fcmf_framework import ops
    ids = torch.zeros(2, 3, dtype=torch.long)
    word = torch.zeros(5, 4, requires_grad=True)
    args = (ids, ids, None, word, word, word, torch.ones(4), torch.zeros(4), 1e-5, 0.0, True, 1, torch.float32)
    adv = ops.EmbeddingAdversary(0.5)
    adv._records = [None]                                             # registered, backward never ran
    with pytest.raises(ValueError, match="backward"):
        with adv.attack():
            ops.embed_layer_norm(*args)
    assert adv.recorded() == 0 and ops._adversary is None             # released on the way out
    adv._records = [(torch.zeros(6, 4), torch.zeros(3, 2, dtype=torch.long))]
    with pytest.raises(ValueError, match="ids"):
        with adv.attack():
            ops.embed_layer_norm(*args)
    adv._records = [(torch.zeros(6, 4, dtype=torch.bfloat16), ids)]
    with pytest.raises(ValueError, match="bfloat16"):
        with adv.attack():
            ops.embed_layer_norm(*args)
    adv._records = [(torch.zeros(6, 4), ids), (torch.zeros(6, 4), ids)]
    with pytest.raises(ValueError, match="made 0 embedding calls, the clean pass recorded 2"):
        with adv.attack():
            pass
    assert adv.recorded() == 0
