"""Feed-forward dropout of the torch-named encoder layer (fcmf_gemm_drop, ops.set_ffn_dropout), the part that needs no GPU: the
surface -- header, binding, switch, signature, the argument checks the entry points make before they plan anything -- and, on
rowwise_ref alone, what tests/test_ffn_dropout_gpu.py relies on when it compares kept sets with the stated mask.

FFN_MASK_CASES lists every (seed, M, N, p) for which a GPU test takes the mask of the two FFN GEMMs.  The (p, seed) pairs are
(0.1, SEED_HI) and (0.5, SEED_LO).  A shape with few rows takes the second pair only: at p = 0.1 a column of 37 (32) elements is
all kept with probability 0.9^37 = 2 % (0.9^32 = 3.4 %), so some of the 261 (256) columns would have no dropped element and the
row / column condition below could not hold."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest

import rowwise_ref as RR
from conftest import ROOT

PAIRS = [(0.1, RR.SEED_HI), (0.5, RR.SEED_LO)]
HALF = [(0.5, RR.SEED_LO)]
# kernel family -> (M, N, K) -> the (p, seed) pairs it runs with (parts A and B of the GPU tests)
GEMM_CASES = {
    "generic": {(200, 256, 128): PAIRS, (37, 261, 64): HALF},
    "tile128": {(200, 256, 128): PAIRS, (300, 264, 32): PAIRS},
    # (4096 x 4096 x 64: 256 tiles of 256 rows are one round, 352 of 192 rows two -- the shape that stays on the 256-row, 64-deep kernel)
    "tile256": {(300, 264, 32): PAIRS, (1100, 776, 160): PAIRS, (4400, 4104, 64): PAIRS, (4096, 4096, 64): HALF},
    "tile192": {(300, 264, 32): PAIRS, (1100, 776, 160): PAIRS, (4400, 4104, 64): PAIRS},
    "planner": {(768, 768, 768): PAIRS},
}
# part C: name -> (G, T, H, heads, I, (p_f, seed_f)); the mask of the FFN GEMMs is [G * T, I]
LAYER_CASES = {"small": (2, 16, 128, 2, 256, HALF[0]), "tile256": (4, 80, 256, 4, 1024, PAIRS[0])}
FFN_MASK_CASES = sorted({(seed, M, N, p) for shapes in GEMM_CASES.values() for (M, N, _), pairs in shapes.items() for p, seed in pairs} |
                        {(seed, G * T, I, p) for G, T, _, _, I, (p, seed) in LAYER_CASES.values()})


# ---- surface ------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_epilogues_and_the_entry_point():
    src = open(os.path.join(ROOT, "include", "fcmf_hip.h")).read()
    assert re.search(r"#define\s+FCMF_EPI_GELU_DROP\s+6\b", src) and re.search(r"#define\s+FCMF_EPI_DGELU_DROP\s+7\b", src)
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"int\s+fcmf_gemm_drop\s*\(([^)]*)\)", code)
    assert m, "fcmf_gemm_drop is not declared"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 21 and args[-4:] == ["int epilogue", "float dropout_p", "uint64_t seed", "void* stream"], args


def test_binding_and_abi_version():
    from fcmf_framework import _hip as H
    assert (H.EPI_GELU_DROP, H.EPI_DGELU_DROP) == (6, 7)
    sig = H.SIGNATURES["fcmf_gemm_drop"]
    assert len(sig) == 21 and sig[-3] is ctypes.c_float and sig[-2] is ctypes.c_uint64
    assert sig[:18] == H.SIGNATURES["fcmf_gemm"][:18]               # fcmf_gemm's arguments up to the epilogue ...
    assert len(H.SIGNATURES["fcmf_gemm"]) == 20                     # ... and fcmf_gemm itself as it was
    assert H.lib().fcmf_abi_version() == 4


def test_switch_defaults_off():
    from fcmf_framework import ops
    assert ops.ffn_dropout() is False
    ops.set_ffn_dropout(True)
    try:
        assert ops.ffn_dropout() is True
    finally:
        ops.set_ffn_dropout(False)
    assert ops.ffn_dropout() is False


def test_layer_and_op_signatures():
    from fcmf_framework import fused, ops
    names = list(inspect.signature(fused.SelfLayerFn.forward).parameters)
    assert names[-3:] == ["probs", "p_f", "seed_f"]
    par = inspect.signature(fused.SelfLayerFn.forward).parameters
    assert par["probs"].default is None and par["p_f"].default == 0.0 and par["seed_f"].default == 0
    for fn in (ops.gemm, ops.gemm_nt, ops.gemm_dx):
        assert inspect.signature(fn).parameters["drop"].default is None
    for fn in (fused._post_fwd, fused._post_bwd):
        par = inspect.signature(fn).parameters
        assert par["p_f"].default == 0.0 and par["seed_f"].default == 0


def test_driver_flag_defaults_off():
    import run_baselines as drv
    base = ["--model", "tomroberta", "--output_dir", "x"]
    assert drv.build_parser().parse_args(base).ffn_dropout is False
    assert drv.build_parser().parse_args(base + ["--ffn_dropout"]).ffn_dropout is True


def test_argument_checks_come_before_any_launch():
    """what the entry points refuse, they refuse while planning (no device is touched: this runs without one)"""
    from fcmf_framework import _hip as H
    L = H.lib()
    buf = ctypes.create_string_buffer(4096 + 16)
    q = (ctypes.addressof(buf) + 15) & ~15                          # non-NULL, 16-byte aligned; never dereferenced
    drop = lambda epi, p, aux=q, M=16: L.fcmf_gemm_drop(None, q, q, q, None, aux, None, M, 16, 32, 32, 32, 16, 0, 0, H.BF16, H.BF16, epi, p, 1, None)
    ARG, UNSUPPORTED = -1, -3
    for p in (0.0, 1.0, -0.1, 1.5, float("nan")):
        assert drop(H.EPI_GELU_DROP, p) == ARG, p
    for epi in (H.EPI_NONE, H.EPI_GELU, H.EPI_DGELU, H.EPI_ADD, H.EPI_TANH):
        assert drop(epi, 0.1) == ARG, epi
    assert drop(H.EPI_DGELU_DROP, 0.1, aux=None) == ARG             # gelu' needs the pre-activation
    assert drop(H.EPI_GELU_DROP, 0.1, M=0) == 0                     # an empty output: nothing to do
    for epi in (H.EPI_GELU_DROP, H.EPI_DGELU_DROP):                 # fcmf_gemm has no rate to give; the e4m3 kernel has no such epilogue
        assert L.fcmf_gemm(None, q, q, q, None, q, None, 16, 16, 32, 32, 32, 16, 0, 0, H.BF16, H.BF16, epi, 0, None) == ARG
        assert L.fcmf_gemm_fp8(None, q, q, q, q, q, None, q, None, 256, 256, 128, 128, 128, 256, epi, None) == UNSUPPORTED


# ---- what the GPU tests rely on ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,M,N,p", FFN_MASK_CASES)
def test_mask_keeps_the_stated_fraction_and_marks_every_row_and_column(seed, M, N, p):
    """kept fraction within 4 standard deviations of 1 - p, and every row and every column of the [M, N] mask holds a kept and a
    dropped element -- otherwise a kernel with a wrong row or column offset could show the stated kept set"""
    kept = RR.dropout_mask(seed, 0, M * N, p)
    q = 1.0 - RR.dropout_threshold(p) / 65536.0
    assert abs(kept.mean() - q) <= 4.0 * math.sqrt(q * (1.0 - q) / (M * N)), (kept.mean(), q)
    kept = kept.reshape(M, N)
    for axis in (0, 1):
        assert kept.any(axis).all() and (~kept).any(axis).all(), axis


def test_probe_values_are_nonzero_in_bf16():
    """the probes make "non-zero" mean "kept": gelu(1) / (1 - p) and 0.5 / (1 - p) are far from zero in bf16, and 1 / K is a
    positive bf16 number for every K of GEMM_CASES (so the backward probe's accumulator is about 1)"""
    import torch
    for p, _ in PAIRS:
        for v in (0.8413447 * RR.inv_keep(p), 0.5 * RR.inv_keep(p)):
            assert float(torch.tensor(v).bfloat16()) > 0.5
    for shapes in GEMM_CASES.values():
        for _, _, K in shapes:
            acc = K * float(torch.tensor(1.0 / K).bfloat16())
            assert 0.99 < acc < 1.01, (K, acc)


def test_the_mask_is_that_of_a_contiguous_dropout_call():
    """m(i * N + j): row i of the [M, N] mask starts at index i * N, whatever the output's leading dimension"""
    M, N, p, seed = 37, 261, 0.5, RR.SEED_LO
    full = RR.mask_tensor(seed, (M, N), p)
    for i in (0, 1, 36):
        assert np.array_equal(full[i].numpy() != 0, RR.dropout_mask(seed, i * N, N, p))
