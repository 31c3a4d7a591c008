"""Every kernel family of csrc/gemm.hip on dyadic operands (tests/gemm_ref.py): the result EQUALS the float64 reference, in guarded
output buffers with ldc > N and three rows below the output, on operands that lie in NaN-poisoned allocations with padded rows.

Each case of test_gemm_exact_cpu.CASES asserts, in this order: the kernel name the case is listed under; torch.equal(C[:, :N],
reference cast to C's dtype) -- and the same for the aux that FCMF_EPI_GELU writes, the column sums and the block statistics; the
guard frames, the columns N .. ldc and the extra rows still hold the sentinel.  The activations (GELU, gelu', tanh) cannot be
exact and are bounded per element, never relative to a tensor's maximum:
    bf16 GELU   |C - f64| <= 2^-8 |f64| + 1.4e-4            bf16 gelu'  |C - f64| <= 2^-8 |f64| + 2e-4 |acc|
      (the polynomial bounds stated above phi_poly4 in csrc/gemm.hip, plus one bf16 ulp)
    bf16 tanh   |C - f64| <= 2^-8 |f64| + 2e-6   (tanhf to the float32 bound below, plus one bf16 ulp)
    float32     |C - f64| <= 2e-6 max(1, |f64|)
FCMF_EPI_DTANH, acc * (1 - aux^2), IS exact for aux in {-1/2, 0, 1/2}.

Not reachable at the smallest shapes, and listed where they run (test_gemm_exact_cpu.py): a transposed A of 130 / 300 rows is the
generic kernel's (M % 8 != 0), so the MFMA cases with a transposed A have 136 / 304 / 704 rows; under tile = 256 the cost model
moves (300, 264, K > 32) and (700, 520, 96) to 192 rows, so (1000, 264, K) on 8 workgroups holds the 256-row kernels; block
statistics of a convolution need 256 output rows (n = 5 / 11), or 8192 for 64 channels; fcmf_conv_gemm* take no leading
dimension of the output, so their outputs are guarded by frames only; e4m3 cases with a bias draw their scales from 2^-1 .. 2^0.

Measured on an MI355X (143 tests, 1.4 s in all; the slowest, the first call of the process, 0.33 s, every other at most 0.09 s): every
case reached the kernel it is listed under; C, aux, column sums and block statistics equal to the reference in every family
(generic, 128 x 128, 64 x 64, persistent 256 / 192 rows at both k-tile depths, narrow n64 / n128, e4m3, column blocks, work lists,
statistics, the three convolutions), every guard intact; no kernel or planner bug was found.  Largest error as a fraction of its
bound: bf16 GELU 0.79 (generic, 64 x 64) and 0.92 (128 x 128, persistent); bf16 gelu' 0.89 in every family; bf16 tanh 0.67;
float32 GELU 0.04, gelu' 0.26, tanh 0.02.
"""
import ctypes

import pytest
import torch

import gemm_ref as GR
import rowwise_ref as RR
from test_gemm_exact_cpu import BY_ID, CASES, DT, EXACT_EPI, IDS, reference

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
EPI_CODE = {"NONE": 0, "GELU": 1, "TANH": 2, "DGELU": 3, "DTANH": 4, "ADD": 5}
DEFAULTS = dict(tile=0, kb=64, cus=256)


def _H():
    from fcmf_framework import _hip
    return _hip


class Out:
    """an output [rows, cols] as the first columns of a guarded [rows + extra, ld] buffer"""

    def __init__(self, rows, cols, ld, dtype, dev, extra=3):
        self.g = RR.guarded((rows + extra, ld), dtype, dev)
        self.rows, self.cols, self.s = rows, cols, RR._SENTINEL[dtype]
        self.live = self.g.view[:rows, :cols]

    def ptr(self):
        return self.g.view.data_ptr()

    def check(self):
        self.g.check()
        assert bool((self.g.view[:self.rows, self.cols:] == self.s).all()), "store into the columns N .. ldc of an inner row"
        assert bool((self.g.view[self.rows:] == self.s).all()), "store into the rows below the output"


def _tuned(H, c, cus=None):
    H.set_gemm_tuning(tile=c["tile"], kb=c["kb"], cus=c["cus"] if cus is None else cus)


def _ctx(H, c):
    if not c["ws"]:
        H.drop_gemm_workspace()
        return H.gemm_ctx()
    return H.gemm_ctx(workspace=True)


def _equal(got, want, dtype, what):
    want, got = want.cpu().to(dtype), got.cpu()
    assert got.shape == want.shape
    if not torch.equal(got, want):
        bad = (got != want) | (got != got)
        idx = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {idx}: "
                             f"{got[tuple(idx)].item()} against {want[tuple(idx)].item()}")


def _bounded(c, got, r):
    """the activation outputs, per element"""
    ref, err = r["C"], (got.cpu().double() - r["C"]).abs()
    if c["out"] == "f32":
        bound = 2e-6 * ref.abs().clamp(min=1.0)
    elif c["epi"] == "GELU":
        bound = 2.0 ** -8 * ref.abs() + 1.4e-4
    elif c["epi"] == "DGELU":
        bound = 2.0 ** -8 * ref.abs() + 2e-4 * r["acc"].abs()
    else:
        bound = 2.0 ** -8 * ref.abs() + 2e-6
    live = bound > 0          # (gelu' of a zero accumulator: error and bound are both 0)
    ratio = float((err[live] / bound[live]).max())
    print(f"{c['id']}: largest error {float(err.max()):.3e}, largest error / bound {ratio:.3f}")
    assert bool((err <= bound).all()), f"{int((err > bound).sum())} elements above the bound, worst at {ratio:.3f} of it"


# ---- fcmf_gemm -------------------------------------------------------------------------------------------------------------------
def _gemm_once(dev, c, r, cus=None):
    H = _H()
    M, N, K, ta, tb = c["M"], c["N"], c["K"], c["ta"], c["tb"]
    out_dt = DT[c["out"]]
    lda, ldb, ldc = (M if ta else K) + c["pad_a"], (N if tb else K) + c["pad_b"], N + c["pad_c"]
    A, B = GR.poisoned(r["A"], lda, c["rows_extra"], dev), GR.poisoned(r["B"], ldb, c["rows_extra"], dev)
    bias = GR.poisoned(r["bias"].float(), N + 4, 1, dev) if r["bias"] is not None else None
    aux_in = GR.poisoned(r["aux_in"].to(out_dt), ldc, c["rows_extra"], dev) if r["aux_in"] is not None else None
    C = Out(M, N, ldc, out_dt, dev)
    U = Out(M, N, ldc, out_dt, dev) if c["epi"] == "GELU" else None
    cs = RR.guarded((N,), F32, dev) if c["colsum"] else None
    if cs is not None:
        cs.view.zero_()
    if c["prior"] == "dyadic":
        C.live.copy_(r["prior"].to(out_dt))
    elif c["prior"] == "nan":
        C.live.fill_(float("nan"))
    aux_ptr = U.ptr() if U is not None else aux_in.data_ptr() if aux_in is not None else None
    _tuned(H, c, cus)
    try:
        ctx = _ctx(H, c)
        H.check(H.lib().fcmf_gemm(ctx, A.data_ptr(), B.data_ptr(), C.ptr(), None if bias is None else bias.data_ptr(), aux_ptr,
                                  None if cs is None else cs.view.data_ptr(), M, N, K, lda, ldb, ldc, ta, tb, H.dt(r["A"]), H.dt(C.live),
                                  EPI_CODE[c["epi"]], int(c["acc"]), H.stream()), "fcmf_gemm")
        name = H.last_gemm_kernel()
    finally:
        H.set_gemm_tuning(**DEFAULTS)
        if not c["ws"]:
            H.gemm_ctx(workspace=True)          # (leave the context as the other tests find it)
    torch.cuda.synchronize()
    return name, C, U, cs


GEMM_IDS = [c["id"] for c in CASES if c["entry"] == "gemm"]


@pytest.mark.parametrize("cid", GEMM_IDS)
def test_gemm(dev, cid):
    c, r = BY_ID[cid], reference(cid)
    out_dt = DT[c["out"]]
    name, C, U, cs = _gemm_once(dev, c, r)
    assert name == c["kernel"], name
    if c["epi"] in EXACT_EPI:
        _equal(C.live, r["C"], out_dt, "C")
    else:
        _bounded(c, C.live, r)
    if U is not None:
        _equal(U.live, r["aux_out"], out_dt, "aux (the pre-activation)")
    if cs is not None:
        _equal(cs.view, r["colsum"], F32, "column sums")
        _equal(cs.view, C.live.double().sum(0), F32, "column sums against the stored C")
    C.check()
    RR.check_all(cs)
    if U is not None:
        U.check()
    if c["also_cus"]:          # a split of K into other slices: every partial sum is exact, so the tensor is the same
        name2, C2, _, _ = _gemm_once(dev, c, r, cus=c["also_cus"])
        assert name2 == c["kernel"], name2
        assert torch.equal(C2.live, C.live)
        C2.check()


# ---- fcmf_gemm_fp8 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c["id"] for c in CASES if c["entry"] == "fp8"])
def test_gemm_fp8(dev, cid):
    H = _H()
    c, r = BY_ID[cid], reference(cid)
    M, N, K = c["M"], c["N"], c["K"]
    lda, ldb, ldc = K + c["pad_a"], K + c["pad_b"], N + c["pad_c"]
    A, B = GR.poisoned(r["A"], lda, 3, dev), GR.poisoned(r["B"], ldb, 3, dev)
    assert int(A.buf[A.pad + K]) == GR.NAN_BYTE          # the padding of row 0 is the e4m3 NaN
    sa, sb = GR.poisoned(r["sa"].float(), M + 4, 1, dev), GR.poisoned(r["sb"].float(), N + 4, 1, dev)
    bias = GR.poisoned(r["bias"].float(), N + 4, 1, dev) if r["bias"] is not None else None
    aux = GR.poisoned(r["aux_in"].to(BF16), ldc, 3, dev) if r["aux_in"] is not None else None
    C = Out(M, N, ldc, BF16, dev)
    H.check(H.lib().fcmf_gemm_fp8(H.gemm_ctx(), A.data_ptr(), sa.data_ptr(), B.data_ptr(), sb.data_ptr(), C.ptr(),
                                  None if bias is None else bias.data_ptr(), None if aux is None else aux.data_ptr(), None, M, N, K, lda, ldb, ldc,
                                  EPI_CODE[c["epi"]], H.stream()), "fcmf_gemm_fp8")
    name = H.last_gemm_kernel()
    torch.cuda.synchronize()
    assert name == c["kernel"], name
    _equal(C.live, r["C"], BF16, "C")
    C.check()


# ---- fcmf_gemm_colblocks ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c["id"] for c in CASES if c["entry"] == "colblocks"])
def test_gemm_colblocks(dev, cid):
    H = _H()
    c, r = BY_ID[cid], reference(cid)
    M, N, K, cb = c["M"], c["N"], c["K"], c["col_block"]
    lda, ldb, ldc = M + c["pad_a"], N + c["pad_b"], cb + c["pad_c"]
    stride = M * ldc + c["blk_gap"]          # > M * ldc: sentinel between the blocks
    nblk = N // cb
    A, B = GR.poisoned(r["A"], lda, 3, dev), GR.poisoned(r["B"], ldb, 3, dev)
    g = RR.guarded(((nblk - 1) * stride + (M + 3) * ldc,), F32, dev)
    live = torch.as_strided(g.view, (nblk, M, cb), (stride, ldc, 1))
    if r["prior"] is not None:
        live.copy_(GR.colblocks(r["prior"], cb).float())
    H.check(H.lib().fcmf_gemm_colblocks(H.gemm_ctx(workspace=True), A.data_ptr(), B.data_ptr(), g.view.data_ptr(), M, N, K, lda, ldb, ldc,
                                        1, 1, cb, stride, int(c["acc"]), H.stream()), "fcmf_gemm_colblocks")
    name = H.last_gemm_kernel()
    torch.cuda.synchronize()
    assert name == c["kernel"], name
    _equal(live, GR.colblocks(r["C"], cb), F32, "the column blocks")
    g.check()
    outside = torch.ones(g.view.numel(), dtype=torch.bool, device=dev)
    torch.as_strided(outside, (nblk, M, cb), (stride, ldc, 1)).fill_(False)
    assert bool((g.view[outside] == RR._SENTINEL[F32]).all()), "store between the rows or the blocks of the column-blocked output"


# ---- fcmf_gemm_dw_list / fcmf_gemm_dw_batched ------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c["id"] for c in CASES if c["entry"] in ("dw_list", "dw_batched")])
def test_gemm_dw_lists(dev, cid):
    H = _H()
    c, r = BY_ID[cid], reference(cid)
    probs = c["probs"]
    n = len(probs)
    A = [GR.poisoned(r["A"][i], probs[i][0] + 8, 3, dev) for i in range(n)]
    B = [GR.poisoned(r["B"][i], probs[i][1] + 8, 3, dev) for i in range(n)]
    outs = {}
    for m, nn, k, d in probs:
        if d not in outs:
            outs[d] = Out(m, nn, nn + 8, F32, dev)
            if r["prior"][d] is not None:
                outs[d].live.copy_(r["prior"][d].float())
            else:
                outs[d].live.fill_(float("nan"))          # accumulate off: the destination is written, whatever it held
    ptrs = lambda xs: (ctypes.c_void_p * n)(*xs)
    ints = lambda col: (ctypes.c_int * n)(*[p[col] for p in probs])
    lds = lambda col: (ctypes.c_int64 * n)(*[p[col] + 8 for p in probs])
    pa, pb, pc = ptrs([a.data_ptr() for a in A]), ptrs([b.data_ptr() for b in B]), ptrs([outs[p[3]].ptr() for p in probs])
    H.set_gemm_tuning(cus=c["cus"])
    try:
        ctx = H.gemm_ctx(workspace=True)
        if c["entry"] == "dw_batched":
            m, nn, k, _ = probs[0]
            H.check(H.lib().fcmf_gemm_dw_batched(ctx, n, pa, pb, pc, m, nn, k, m + 8, nn + 8, nn + 8, int(c["acc"]), H.stream()), "fcmf_gemm_dw_batched")
        else:
            H.check(H.lib().fcmf_gemm_dw_list(ctx, n, pa, pb, pc, ints(0), ints(1), ints(2), lds(0), lds(1), lds(1), int(c["acc"]), H.stream()),
                    "fcmf_gemm_dw_list")
        name = H.last_gemm_kernel()
    finally:
        H.set_gemm_tuning(**DEFAULTS)
    torch.cuda.synchronize()
    assert name == c["kernel"], name
    for d, o in outs.items():
        _equal(o.live, r["C"][d], F32, f"destination {d}")
    for o in outs.values():
        o.check()


# ---- fcmf_gemm_colstats ----------------------------------------------------------------------------------------------------------
def _check_stats(c, r, C, st, name):
    assert name == c["kernel"], name
    _equal(C.live if isinstance(C, Out) else C.view, r["C"], BF16, "C")
    _equal(st.view, r["stats"], F32, "block statistics")
    stored = (C.live if isinstance(C, Out) else C.view).cpu().double()
    _equal(st.view, GR.colstats(stored, c["block_rows"]), F32, "block statistics against the stored C")
    C.check()
    st.check()


@pytest.mark.parametrize("cid", [c["id"] for c in CASES if c["entry"] == "colstats"])
def test_gemm_colstats(dev, cid):
    H = _H()
    c, r = BY_ID[cid], reference(cid)
    M, N, K = c["M"], c["N"], c["K"]
    lda, ldb, ldc = K + c["pad_a"], K + c["pad_b"], N + c["pad_c"]
    A, B = GR.poisoned(r["A"], lda, 3, dev), GR.poisoned(r["B"], ldb, 3, dev)
    C = Out(M, N, ldc, BF16, dev)
    R = c["block_rows"]
    assert H.lib().fcmf_gemm_colstats_block_rows(H.gemm_ctx(), M, N, K) == R
    st = RR.guarded(((M + R - 1) // R, N, 2), F32, dev)
    H.check(H.lib().fcmf_gemm_colstats(H.gemm_ctx(), A.data_ptr(), B.data_ptr(), C.ptr(), st.view.data_ptr(), M, N, K, lda, ldb, ldc, H.stream()),
            "fcmf_gemm_colstats")
    name = H.last_gemm_kernel()
    torch.cuda.synchronize()
    _check_stats(c, r, C, st, name)


# ---- implicit convolutions -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c["id"] for c in CASES if c["entry"] in ("conv", "conv_colstats", "conv_runs")])
def test_conv_gemm(dev, cid):
    H = _H()
    c, r = BY_ID[cid], reference(cid)
    M, N, K = c["M"], c["N"], c["K"]
    x = GR.poisoned(r["A"], r["A"].numel() + 8, 1, dev)          # poisoned OUTSIDE [n, Hp, Wp, C] only: the zero border is the operand's
    w = GR.poisoned(r["B"], K, 3, dev)                            # (the entry points take dense weights and a dense output)
    y = RR.guarded((M, N), BF16, dev)
    st = None
    L = H.lib()
    _tuned(H, c)
    try:
        ctx = H.gemm_ctx()
        if c["entry"] == "conv_runs":
            n, Hp, Wp, pix, run, Ho, Wo, kh, stride = c["runs"]
            H.check(L.fcmf_conv_gemm_runs(ctx, x.data_ptr(), w.data_ptr(), y.view.data_ptr(), None, n, Hp, Wp, pix, run, Ho, Wo, kh, stride, N, H.stream()),
                    "fcmf_conv_gemm_runs")
        else:
            n, Hp, Wp, Cin, stride = c["conv"]
            Ho, Wo = (Hp - 3) // stride + 1, (Wp - 3) // stride + 1
            geom = (n, Hp, Wp, Cin, Ho, Wo, 3, 3, stride, N)
            if c["entry"] == "conv_colstats":
                R = c["block_rows"]
                assert L.fcmf_gemm_colstats_block_rows(ctx, M, N, K) == R
                st = RR.guarded(((M + R - 1) // R, N, 2), F32, dev)
                H.check(L.fcmf_conv_gemm_colstats(ctx, x.data_ptr(), w.data_ptr(), y.view.data_ptr(), st.view.data_ptr(), *geom, H.stream()),
                        "fcmf_conv_gemm_colstats")
            else:
                H.check(L.fcmf_conv_gemm(ctx, x.data_ptr(), w.data_ptr(), y.view.data_ptr(), *geom, H.stream()), "fcmf_conv_gemm")
        name = H.last_gemm_kernel()
    finally:
        H.set_gemm_tuning(**DEFAULTS)
    torch.cuda.synchronize()
    if st is not None:
        _check_stats(c, r, y, st, name)
        return
    assert name == c["kernel"], name
    _equal(y.view, r["C"], BF16, "y")
    y.check()


def test_every_case_has_a_test():
    assert {c["entry"] for c in CASES} == {"gemm", "fp8", "colblocks", "dw_list", "dw_batched", "colstats", "conv", "conv_colstats", "conv_runs"}
    assert len(IDS) == len(set(IDS))
