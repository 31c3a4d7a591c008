"""The weight EMA without a GPU: the decay schedule, the drivers' flags (accepted, and refused before anything is written), the
C ABI's two entry points in the header and the binding, and their refusals, which return before any launch and so can be asked
with host buffers."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT


# ---- the decay schedule --------------------------------------------------------------------------------------------------------
def test_decay_without_warmup_is_the_decay():
    from fcmf_framework.optimization import ema_decay_at
    for t in (1, 2, 10, 10 ** 6):
        assert ema_decay_at(0.999, t, False) == 0.999 and ema_decay_at(0.5, t, warmup=False) == 0.5


def test_decay_warmup_values():
    from fcmf_framework.optimization import ema_decay_at
    assert ema_decay_at(0.999, 1, True) == 2.0 / 11.0 and ema_decay_at(0.999, 1) == 2.0 / 11.0      # warmup is the default
    assert ema_decay_at(0.1, 1, True) == 0.1                                                        # a small decay caps at once
    # (1 + t) / (10 + t) >= 0.999  <=>  t >= 8990: the cap is first reached there and never exceeded
    assert ema_decay_at(0.999, 8989, True) < 0.999
    assert ema_decay_at(0.999, 8990, True) == 0.999
    values = [ema_decay_at(0.999, t, True) for t in range(1, 20000)]
    assert max(values) == 0.999 and values.index(0.999) == 8990 - 1
    assert all(b >= a for a, b in zip(values, values[1:]))                                          # monotone non-decreasing
    assert all(0.0 < v < 1.0 for v in values)


# ---- drivers -------------------------------------------------------------------------------------------------------------------
def _drivers():
    import run_baselines
    import run_multimodal_fcmf
    import run_pretraining_fcmf
    return ((run_multimodal_fcmf, ["--pretrained_hf_model", "x"]), (run_baselines, ["--model", "mroberta"]),
            (run_pretraining_fcmf, ["--pretrained_hf_model", "x"]))


def test_parsers_accept_the_ema_flags():
    from train_harness import check_ema_arguments
    for drv, head in _drivers():
        args = drv.build_parser().parse_args(["--output_dir", "o"] + head + ["--ema_decay", "0.99", "--ema_no_warmup"])
        assert args.ema_decay == 0.99 and args.ema_no_warmup is True and check_ema_arguments(args) == 0.99
        args = drv.build_parser().parse_args(["--output_dir", "o"] + head)
        assert args.ema_decay == 0.0 and args.ema_no_warmup is False and check_ema_arguments(args) == 0.0      # off by default
        text = " ".join(drv.build_parser().format_help().split())
        assert "--ema_decay" in text and "BatchNorm running statistics" in text and "not averaged" in text


@pytest.mark.parametrize("value", ["1.0", "-0.1", "nan", "inf"])
def test_drivers_refuse_a_bad_decay_before_anything_is_written(tmp_path, value):
    for i, (drv, head) in enumerate(_drivers()):
        out = str(tmp_path / f"out{i}")
        with pytest.raises(ValueError, match="--ema_decay"):
            drv.main(["--output_dir", out] + head + ["--do_train", "--ema_decay", value])
        assert not os.path.exists(out)


def test_set_ema_refuses_bad_decays():
    import torch
    from fcmf_framework.optimization import FusedAdamW
    opt = FusedAdamW([torch.nn.Parameter(torch.zeros(3))])
    for bad in (1.0, -0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="decay"):
            opt.set_ema(bad)
    opt.set_ema(0.9, warmup=False)
    assert opt.ema == (0.9, False)
    opt.set_ema(None)
    assert opt.ema is None
    opt.set_ema(0.5)
    opt.set_ema(0.0)
    assert opt.ema is None


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------
def test_binding_exposes_both_entry_points():
    from fcmf_framework import _hip as H
    S = H.SIGNATURES
    assert S["fcmf_multi_adamw_ema"] == S["fcmf_multi_adamw"] + [ctypes.c_void_p, ctypes.c_float]
    assert S["fcmf_multi_swap"] == [ctypes.c_void_p] * 6 + [ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    L = H.lib()
    assert L.fcmf_multi_adamw_ema.argtypes == S["fcmf_multi_adamw_ema"] and L.fcmf_multi_swap.argtypes == S["fcmf_multi_swap"]
    assert L.fcmf_abi_version() == 4                      # additive: the version stays


def test_header_declares_both_and_states_the_formula():
    src = open(os.path.join(ROOT, "include", "fcmf_hip.h")).read()
    assert re.search(r"\bint\s+fcmf_multi_adamw_ema\s*\(", src) and re.search(r"\bint\s+fcmf_multi_swap\s*\(", src)
    assert "e = ema_decay * e + (1.0f - ema_decay) * p_new" in src
    decl = src[src.index("int fcmf_multi_adamw_ema("):]
    decl = " ".join(decl[:decl.index(";")].split())
    plain = src[src.index("int fcmf_multi_adamw("):]
    plain = " ".join(plain[:plain.index(";")].split())
    # every argument of fcmf_multi_adamw in the same order, then the table and the decay
    assert decl == plain.replace("fcmf_multi_adamw(", "fcmf_multi_adamw_ema(")[:-1] + ", const int64_t* ema_ptrs, float ema_decay)"


def test_entry_points_refuse_before_any_launch():
    """FCMF_ERR_ARG (-1) on host buffers: a call that launched would fail otherwise"""
    from fcmf_framework import _hip as H
    L = H.lib()
    tab = np.zeros(4, np.int64)
    i32 = np.zeros(4, np.int32)
    P = lambda a: a.ctypes.data
    lr, wd = (ctypes.c_float * 8)(), (ctypes.c_float * 8)()

    def adamw(fn, tail=(), p=P(tab), nchunks=1, chunk=256, ngroups=1, step=1):
        return fn(p, P(tab), P(tab), P(tab), None, P(tab), P(i32), P(i32), P(tab), nchunks, chunk, lr, wd, ngroups, 0.9, 0.999, 1e-8,
                  step, None, -1.0, None, *tail)

    def ema(ptrs=P(tab), decay=0.5, **kw):
        return adamw(L.fcmf_multi_adamw_ema, (ptrs, decay), **kw)

    assert ema(ptrs=None) == H.ERR_ARG
    for d in (1.0, -0.5, float("nan"), float("inf"), 1.5):
        assert ema(decay=d) == H.ERR_ARG
    # whatever fcmf_multi_adamw refuses, with the same answer
    for kw in (dict(p=None), dict(nchunks=-1), dict(chunk=0), dict(chunk=-4), dict(ngroups=0), dict(ngroups=9), dict(step=0)):
        assert adamw(L.fcmf_multi_adamw, **kw) == H.ERR_ARG and ema(**kw) == H.ERR_ARG, kw
    # no chunk, nothing to do: fcmf_multi_adamw answers 0 without a launch, and so does the EMA entry point -- after its checks
    assert adamw(L.fcmf_multi_adamw, nchunks=0) == 0 and ema(nchunks=0) == 0
    assert ema(nchunks=0, ptrs=None) == H.ERR_ARG and ema(nchunks=0, decay=1.0) == H.ERR_ARG

    def swap(a=P(tab), b=P(tab), sizes=P(tab), ct=P(i32), co=P(tab), nchunks=1, chunk=256):
        return L.fcmf_multi_swap(a, b, None, sizes, ct, co, nchunks, chunk, None)

    for kw in (dict(a=None), dict(b=None), dict(sizes=None), dict(ct=None), dict(co=None), dict(nchunks=-1), dict(chunk=0),
               dict(chunk=-1)):
        assert swap(**kw) == H.ERR_ARG, kw
    assert swap(nchunks=0) == 0
    assert not math.isnan(tab.sum()) and not tab.any() and not i32.any()       # the tables were never written
