"""FCMF_EPI_RELU / FCMF_EPI_ADD_RELU through fcmf_gemm and fcmf_conv_gemm_epi on dyadic operands (tests/gemm_ref.py): the result
EQUALS the float64 reference max(acc + bias (+ aux), 0).  Operands lie in NaN-poisoned allocations with padded rows, outputs in
guarded buffers with ldc > N (the convolution entry point takes no leading dimension: frames only).

All shifts are 0: an accumulator is an integer |n| <= K, bias and aux integers of [-8, 8], and every case asserts on the float64
side that |acc + bias + aux| <= 256, so the bf16 output holds the reference exactly.  About half of the pre-activations are
negative, so a kernel that skips the ReLU, or applies it before the residual, cannot pass; FCMF_EPI_RELU is run with a NaN aux
operand where the case says so (the epilogue must not read it).

One shape per kernel family, the smallest that reaches it, asserted through fcmf_gemm_ctx_last_kernel:
    64 x 64 kernel            64 x 64 x 64
    128 x 128 kernel          200 x 136 x 72, both operands transposed (K-contiguous operands need K % 32 == 0: that kernel's
                              partial k-tile exists in the transposed layouts only)
    persistent kernel         512 x 256 x 128 under tile = 256: the cost model gives it the 192-row tile (three tiles in one round
                              against two); 1000 x 264 x K on 8 workgroups holds the 256-row instantiations that are built
    narrow-N route            8192 x 64 x 64: RELU on the 8 x 1-wave layout, ADD_RELU (no aux operand there) on the 64 x 64 kernel
    generic kernel, float32   37 x 19 x 23
"""
import pytest
import torch

import gemm_ref as GR
import rowwise_ref as RR
from test_gemm_exact_gpu import DEFAULTS, Out, _equal

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
RELU, ADD_RELU = 8, 9
ERR_ARG, ERR_UNSUPPORTED = -1, -3
SMALL = "gemm_bf16_small_kernel<bf16>"


def _H():
    from fcmf_framework import _hip
    return _hip


def _want(acc, bias, aux, epi):
    v = acc + bias[None, :] + (aux if epi == ADD_RELU else 0.0)
    assert GR.on_grid(v, 0, 256), "the pre-activation leaves the bf16 grid: another seed"
    neg = float((v < 0).double().mean())
    assert 0.2 < neg < 0.8, neg          # the ReLU has something to do, and something to keep
    return v.clamp(min=0.0)


# (id, M, N, K, ta, tb, dtype, tuning, {epilogue: kernel})
GEMM_CASES = [
    ("small", 64, 64, 64, 0, 0, BF16, {}, {RELU: SMALL, ADD_RELU: SMALL}),
    ("tile128", 200, 136, 72, 1, 1, BF16, {}, {RELU: "gemm_bf16_kernel<1,1,bf16>", ADD_RELU: "gemm_bf16_kernel<1,1,bf16>"}),
    ("persistent", 512, 256, 128, 0, 0, BF16, dict(tile=256),
     {RELU: "gemm_bf16_tile192k64_kernel<RELU>", ADD_RELU: "gemm_bf16_tile192k64_kernel<ADD_RELU>"}),
    ("persistent-256rows-k64", 1000, 264, 128, 0, 0, BF16, dict(tile=256, cus=8),
     {RELU: "gemm_bf16_tile256k64_kernel<RELU>", ADD_RELU: "gemm_bf16_tile192k64_kernel<ADD_RELU>"}),
    ("persistent-256rows-k32", 1000, 264, 96, 0, 0, BF16, dict(tile=256, kb=32, cus=8),
     {RELU: "gemm_bf16_tile256_kernel<0,0,bf16,RELU>", ADD_RELU: "gemm_bf16_tile256_kernel<0,0,bf16,ADD_RELU>"}),
    ("persistent-transposed-b", 1000, 264, 96, 0, 1, BF16, dict(tile=256, kb=32, cus=8),
     {RELU: "gemm_bf16_tile192_kernel<1,RELU>", ADD_RELU: "gemm_bf16_tile192_kernel<1,ADD_RELU>"}),
    ("persistent-transposed-a", 304, 264, 96, 1, 0, BF16, dict(tile=256, kb=32),
     {RELU: "gemm_bf16_kernel<1,0,bf16>", ADD_RELU: "gemm_bf16_kernel<1,0,bf16>"}),
    ("narrow", 8192, 64, 64, 0, 0, BF16, {}, {RELU: "gemm_bf16_tile256k64_n64_relu_kernel", ADD_RELU: SMALL}),
    ("narrow-n128", 8192, 128, 192, 0, 0, BF16, {}, {RELU: "gemm_bf16_tile256k64_n128_relu_kernel", ADD_RELU: SMALL}),
    ("generic", 37, 19, 23, 0, 0, F32, {}, {RELU: "gemm_generic_kernel", ADD_RELU: "gemm_generic_kernel"}),
]


@pytest.mark.parametrize("epi", [RELU, ADD_RELU], ids=["RELU", "ADD_RELU"])
@pytest.mark.parametrize("case", GEMM_CASES, ids=[c[0] for c in GEMM_CASES])
def test_gemm_relu(dev, case, epi):
    H = _H()
    _, M, N, K, ta, tb, dt, tuning, kernels = case
    seed = 4000 + 10 * GEMM_CASES.index(case)
    A, B = GR.dyadic((K, M) if ta else (M, K), seed), GR.dyadic((K, N) if tb else (N, K), seed + 1)
    bias, aux = GR.dyadic_ints((N,), seed + 2), GR.dyadic_ints((M, N), seed + 3)
    want = _want(GR.product(A, B, ta, tb), bias, aux, epi)
    pad = 8 if dt == BF16 else 3
    lda, ldb, ldc = (M if ta else K) + pad, (N if tb else K) + pad, N + pad          # ldc > N
    Ad, Bd = GR.poisoned(A.to(dt), lda, 3, dev), GR.poisoned(B.to(dt), ldb, 3, dev)
    bd = GR.poisoned(bias.float(), N + 4, 1, dev)
    # FCMF_EPI_RELU takes no aux: it is handed a NaN operand of the right shape, which must not be read
    xd = GR.poisoned(aux.to(dt) if epi == ADD_RELU else torch.full((M, N), float("nan"), dtype=dt), ldc, 3, dev)
    C = Out(M, N, ldc, dt, dev)
    H.set_gemm_tuning(**{**DEFAULTS, **tuning})
    try:
        H.check(H.lib().fcmf_gemm(H.gemm_ctx(workspace=True), Ad.data_ptr(), Bd.data_ptr(), C.ptr(), bd.data_ptr(), xd.data_ptr(), None, M, N, K,
                                  lda, ldb, ldc, ta, tb, H.dt(Ad.view), H.dt(C.live), epi, 0, H.stream()), "fcmf_gemm")
        name = H.last_gemm_kernel()
    finally:
        H.set_gemm_tuning(**DEFAULTS)
    torch.cuda.synchronize()
    assert name == kernels[epi], name
    _equal(C.live, want, dt, "C")
    C.check()


def test_add_relu_needs_aux_and_the_other_entry_points_refuse(dev):
    H = _H()
    L = H.lib()
    M = N = K = 256
    A = torch.zeros((M, K), dtype=BF16, device=dev)
    B = torch.zeros((N, K), dtype=BF16, device=dev)
    C = torch.zeros((M, N), dtype=BF16, device=dev)
    Cf = torch.zeros((M, N), dtype=F32, device=dev)
    sa, sb = torch.ones(M, device=dev), torch.ones(N, device=dev)
    q = torch.zeros((M, K), dtype=torch.uint8, device=dev)
    ctx, st = H.gemm_ctx(workspace=True), H.stream()
    p = lambda t: t.data_ptr()
    for out in (C, Cf):          # bf16 and float32 outputs
        assert L.fcmf_gemm(ctx, p(A), p(B), p(out), None, None, None, M, N, K, K, K, N, 0, 0, H.BF16, H.dt(out), ADD_RELU, 0, st) == ERR_ARG
    Af = torch.zeros((M, K), dtype=F32, device=dev)
    assert L.fcmf_gemm(ctx, p(Af), p(Af), p(Cf), None, None, None, M, N, K, K, K, N, 0, 0, H.F32, H.F32, ADD_RELU, 0, st) == ERR_ARG
    for epi in (RELU, ADD_RELU):
        assert L.fcmf_gemm_fp8(ctx, p(q), p(sa), p(q), p(sb), p(C), None, p(C), None, M, N, K, K, K, N, epi, st) == ERR_UNSUPPORTED
        assert L.fcmf_gemm_drop(ctx, p(A), p(B), p(C), None, p(C), None, M, N, K, K, K, N, 0, 0, H.BF16, H.BF16, epi, 0.1, 1, st) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert not C.any() and not Cf.any()          # nothing was launched


# ---- fcmf_conv_gemm_epi ----------------------------------------------------------------------------------------------------------
T128 = "gemm_bf16_kernel<0,0,bf16>"
# (id, C, Cout, k, stride, n, hw of the unpadded input, tuning, {epilogue: kernel})
CONV_CASES = [
    ("3x3-c64", 64, 64, 3, 1, 5, 14, {}, {RELU: T128, ADD_RELU: T128}),
    ("3x3-c128-s2", 128, 128, 3, 2, 3, 28, {}, {RELU: T128, ADD_RELU: T128}),
    ("shortcut-1x1-s2", 512, 1024, 1, 2, 8, 16, {}, {RELU: T128, ADD_RELU: T128}),
    # beyond the three above: the persistent and the narrow layouts with the convolution's addressing
    ("3x3-c64-persistent", 64, 264, 3, 1, 2, 8, dict(tile=256),
     {RELU: "gemm_bf16_tile192k64_kernel<RELU>", ADD_RELU: "gemm_bf16_tile192k64_kernel<ADD_RELU>"}),
    ("3x3-c64-narrow", 64, 64, 3, 1, 2, 64, {}, {RELU: "gemm_bf16_tile256k64_n64_relu_kernel", ADD_RELU: T128}),
]


@pytest.mark.parametrize("epi", [RELU, ADD_RELU], ids=["RELU", "ADD_RELU"])
@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv_gemm_epi(dev, case, epi):
    H = _H()
    _, Cin, Cout, k, stride, n, hw, tuning, kernels = case
    seed = 5000 + 10 * CONV_CASES.index(case)
    pad = k // 2
    Hp = hw + 2 * pad
    Ho = (Hp - k) // stride + 1
    M, K = n * Ho * Ho, k * k * Cin
    x = torch.zeros(n, Hp, Hp, Cin, dtype=torch.float64)
    x[:, pad:pad + hw, pad:pad + hw] = GR.dyadic((n, hw, hw, Cin), seed)          # the zero border is part of the operand
    w = GR.dyadic((Cout, k, k, Cin), seed + 1)
    bias, aux = GR.dyadic_ints((Cout,), seed + 2), GR.dyadic_ints((M, Cout), seed + 3)
    want = _want(GR.conv_nhwc(x, w, stride, Ho, Ho), bias, aux, epi)
    xd = GR.poisoned(x.to(BF16), x.numel() + 8, 1, dev)
    wd = GR.poisoned(w.reshape(Cout, K).to(BF16), K, 3, dev)
    bd = GR.poisoned(bias.float(), Cout + 4, 1, dev)
    ad = GR.poisoned(aux.to(BF16) if epi == ADD_RELU else torch.full((M, Cout), float("nan"), dtype=BF16), Cout, 3, dev)
    y = RR.guarded((M, Cout), BF16, dev)
    H.set_gemm_tuning(**{**DEFAULTS, **tuning})
    try:
        H.check(H.lib().fcmf_conv_gemm_epi(H.gemm_ctx(), xd.data_ptr(), wd.data_ptr(), y.view.data_ptr(), bd.data_ptr(), ad.data_ptr(), epi,
                                           n, Hp, Hp, Cin, Ho, Ho, k, k, stride, Cout, H.stream()), "fcmf_conv_gemm_epi")
        name = H.last_gemm_kernel()
    finally:
        H.set_gemm_tuning(**DEFAULTS)
    torch.cuda.synchronize()
    assert name == kernels[epi], name
    _equal(y.view, want, BF16, "y")
    y.check()


def test_conv_gemm_epi_arguments(dev):
    H = _H()
    L = H.lib()
    x = torch.zeros((1, 10, 10, 64), dtype=BF16, device=dev)
    w = torch.zeros((64, 576), dtype=BF16, device=dev)
    y = torch.zeros((64, 64), dtype=BF16, device=dev)
    b = torch.zeros(64, device=dev)
    geom = (1, 10, 10, 64, 8, 8, 3, 3, 1, 64)
    p = lambda t: t.data_ptr()
    for epi in (1, 2, 3, 4, 6, 7, 10):          # GELU, TANH, DGELU, DTANH, the dropout pair, an unknown value
        assert L.fcmf_conv_gemm_epi(H.gemm_ctx(), p(x), p(w), p(y), p(b), p(y), epi, *geom, H.stream()) == ERR_ARG
    assert L.fcmf_conv_gemm_epi(H.gemm_ctx(), p(x), p(w), p(y), p(b), None, ADD_RELU, *geom, H.stream()) == ERR_ARG
    assert L.fcmf_conv_gemm_epi(H.gemm_ctx(), p(x), p(w), p(y), None, None, RELU, *geom, H.stream()) == ERR_ARG
    H.check(L.fcmf_conv_gemm_epi(H.gemm_ctx(), p(x), p(w), p(y), p(b), None, 0, *geom, H.stream()), "fcmf_conv_gemm_epi")
    torch.cuda.synchronize()
