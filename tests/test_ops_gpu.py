"""Per-kernel parity: every C-ABI entry point against a plain torch fp32 restatement of the same op.
Tolerances: fp32 path ~1e-5 relative (exact-f32 MFMA fmaf chains vs torch's summation order),
bf16 path 2e-2 relative to the tensor's max (bf16 storage has 8 significant bits)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import max_err, mfma_attention, rel_err

pytestmark = pytest.mark.gpu


def _ops():
    from fcmf_framework import ops, _hip
    return ops, _hip


def _rand(shape, dev, dtype=torch.float32, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype).to(dev)


TOL = {torch.float32: 2e-5, torch.bfloat16: 2e-2}


# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("M,N,K", [(300, 256, 192), (128, 128, 64), (37, 4, 70), (200, 768, 2048), (5, 136, 8)])
def test_gemm_layouts(dev, dtype, ta, tb, M, N, K):
    ops, H = _ops()
    A = _rand((K, M) if ta else (M, K), dev, dtype, seed=1)
    B = _rand((K, N) if tb else (N, K), dev, dtype, seed=2)
    bias = _rand((N,), dev, seed=3)
    C = torch.empty((M, N), dtype=dtype, device=dev)
    ops.gemm(A, B, C, M, N, K, A.shape[1], B.shape[1], N, ta, tb, bias=bias)
    Af = A.float().cpu().t() if ta else A.float().cpu()
    Bf = B.float().cpu() if tb else B.float().cpu().t()
    ref = Af @ Bf + bias.cpu()
    assert rel_err(C, ref) < TOL[dtype], (ta, tb, M, N, K)


@pytest.mark.parametrize("tile", [128, 256, 192])
@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("M,N,K", [(700, 520, 96), (256, 256, 32), (1000, 776, 224), (700, 520, 128), (1000, 776, 320)])
def test_gemm_bf16_both_tile_kernels(dev, tile, ta, tb, M, N, K):
    """all MFMA tile kernels (128x128, persistent 256x256 / 192x256 ping-pong) on ragged M/N edges and odd k-tile counts;
    K % 64 == 0 with both operands K-contiguous runs the 64-deep k-tile variant (2-stage ring, whole-line DMA)"""
    ops, H = _ops()
    A = _rand((K, M) if ta else (M, K), dev, torch.bfloat16, seed=1)
    B = _rand((K, N) if tb else (N, K), dev, torch.bfloat16, seed=2)
    bias = _rand((N,), dev, seed=3)
    C = torch.empty((M, N), dtype=torch.bfloat16, device=dev)
    H.set_gemm_tuning(tile=tile)
    try:
        ops.gemm(A, B, C, M, N, K, A.shape[1], B.shape[1], N, ta, tb, bias=bias)
        Cf = torch.full((M, N), 0.5, dtype=torch.float32, device=dev)
        ops.gemm(A, B, Cf, M, N, K, A.shape[1], B.shape[1], N, ta, tb, acc=True)
    finally:
        H.set_gemm_tuning(tile=0)
    Af = A.float().cpu().t() if ta else A.float().cpu()
    Bf = B.float().cpu() if tb else B.float().cpu().t()
    assert rel_err(C, Af @ Bf + bias.cpu()) < 2e-2
    assert rel_err(Cf, Af @ Bf + 0.5) < 1e-3


@pytest.mark.parametrize("epi", ["none", "gelu", "dgelu", "add"])
@pytest.mark.parametrize("M,N,K", [(1000, 776, 320), (4400, 4104, 128), (6144, 768, 768)])
def test_gemm_k64_and_k32_kernels_agree_bitwise(dev, M, N, K, epi):
    """the 64-deep k-tile kernels (whole-line DMA, five-slot ring) issue the same MFMAs in the same order as the 32-deep
    ones: every output bit must agree, for every epilogue"""
    ops, H = _ops()
    A, B = _rand((M, K), dev, torch.bfloat16, seed=1), _rand((N, K), dev, torch.bfloat16, 0.2, seed=2)
    bias = _rand((N,), dev, seed=3)
    u = _rand((M, N), dev, torch.bfloat16, 1.5, seed=5)
    outs = []
    for kb in (32, 64):
        H.set_gemm_tuning(kb=kb)
        H.set_gemm_tuning(tile=256)          # the persistent kernels also for the small ragged case
        try:
            C = torch.empty((M, N), dtype=torch.bfloat16, device=dev)
            aux = torch.empty_like(C)
            if epi == "none":
                ops.gemm(A, B, C, M, N, K, K, K, N, False, False, bias=bias)
            elif epi == "gelu":
                ops.gemm(A, B, C, M, N, K, K, K, N, False, False, bias=bias, aux=aux, epi=H.EPI_GELU)
            elif epi == "dgelu":
                ops.gemm(A, B, C, M, N, K, K, K, N, False, False, aux=u, epi=H.EPI_DGELU)
            else:
                ops.gemm(A, B, C, M, N, K, K, K, N, False, False, bias=bias, aux=u, epi=H.EPI_ADD)
            outs.append((C.clone(), aux.clone() if epi == "gelu" else None, H.last_gemm_kernel()))
        finally:
            H.set_gemm_tuning(kb=64)
            H.set_gemm_tuning(tile=0)
    assert "k64" not in outs[0][2] and "k64" in outs[1][2], (outs[0][2], outs[1][2])
    assert torch.equal(outs[0][0], outs[1][0])
    if epi == "gelu":
        assert torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("epi", ["none", "gelu", "dgelu", "add", "tanh", "f32acc"])
@pytest.mark.parametrize("M,N,K", [(768, 768, 768), (960, 1536, 768), (100, 136, 128), (768, 64, 64), (1000, 776, 3072)])
def test_gemm_small_output_kernel_matches_the_128_tile_kernel(dev, M, N, K, epi):
    """gemm_bf16_small_kernel (64 x 64 tiles, 64-deep k-tiles: the IAOG decoder's 768 x 768 x 768 products, where 128 x 128 tiles
    occupy 36 of 256 CUs): same products summed in the same order per output element as the 128 x 128 kernel -> every output
    BIT agrees, for every epilogue the fragment-layout epilogue serves (bias, GELU + pre-activation output, gelu', residual add,
    tanh, f32 accumulate, column sums); and against the float64 product.  Ragged edges, one k-tile, K = 3072."""
    ops, H = _ops()
    A, B = _rand((M, K), dev, torch.bfloat16, seed=1), _rand((N, K), dev, torch.bfloat16, 0.2, seed=2)
    bias = _rand((N,), dev, seed=3)
    u = _rand((M, N), dev, torch.bfloat16, 1.5, seed=5)
    outs = []
    for tile in (128, 0):
        H.set_gemm_tuning(tile=tile)
        try:
            C = torch.empty((M, N), dtype=torch.bfloat16, device=dev)
            aux = torch.empty_like(C)
            cs = torch.zeros(N, dtype=torch.float32, device=dev)
            if epi == "none":
                ops.gemm(A, B, C, M, N, K, K, K, N, False, False, bias=bias, colsum=cs)
            elif epi == "gelu":
                ops.gemm(A, B, C, M, N, K, K, K, N, False, False, bias=bias, aux=aux, epi=H.EPI_GELU)
            elif epi == "dgelu":
                ops.gemm(A, B, C, M, N, K, K, K, N, False, False, aux=u, epi=H.EPI_DGELU, colsum=cs)
            elif epi == "add":
                ops.gemm(A, B, C, M, N, K, K, K, N, False, False, bias=bias, aux=u, epi=H.EPI_ADD)
            elif epi == "tanh":
                ops.gemm(A, B, C, M, N, K, K, K, N, False, False, bias=bias, epi=H.EPI_TANH)
            else:
                C = torch.full((M, N), 0.25, dtype=torch.float32, device=dev)
                ops.gemm(A, B, C, M, N, K, K, K, N, False, False, acc=True)
            outs.append((C.clone(), aux.clone(), cs.clone(), H.last_gemm_kernel()))
        finally:
            H.set_gemm_tuning(tile=0)
    assert outs[0][3].startswith("gemm_bf16_kernel"), outs[0][3]
    if epi != "f32acc":      # (f32 accumulation with K >= 512 belongs to the split-K paths of the persistent / 128 x 128 kernels; the small kernel takes it below that)
        assert outs[1][3].startswith("gemm_bf16_small_kernel"), outs[1][3]
    if epi == "f32acc":
        assert rel_err(outs[1][0], outs[0][0]) < 1e-5            # (the 128 x 128 kernel splits K and adds with float atomics: another summation order)
    else:
        assert torch.equal(outs[0][0], outs[1][0])
    if epi == "gelu":
        assert torch.equal(outs[0][1], outs[1][1])
    if epi in ("none", "dgelu"):
        assert rel_err(outs[1][2], outs[0][2]) < 1e-5            # (float atomics: order not fixed)
    pre = A.double().cpu() @ B.double().cpu().t()
    if epi == "none":
        assert rel_err(outs[1][0], pre + bias.double().cpu()) < 2e-2
        assert rel_err(outs[1][2], outs[1][0].double().cpu().sum(0)) < 1e-3
    elif epi == "f32acc":
        assert rel_err(outs[1][0], pre + 0.25) < 1e-3


@pytest.mark.parametrize("M,N,K,nk_note", [(700, 520, 96, "3 k-tiles"), (4400, 4104, 64, "306 tiles: two rounds of work items per CU"),
                                           (300, 264, 32, "1 k-tile"), (1100, 776, 160, "5 k-tiles"),
                                           (1100, 776, 192, "3 k-tiles of 64"), (4400, 4104, 128, "2 k-tiles of 64, two rounds"),
                                           (49152 // 8, 768, 768, "12 k-tiles of 64: a slice of the step's own shape")])
@pytest.mark.parametrize("tile", [256, 192])
def test_gemm_tile256_epilogues(dev, tile, M, N, K, nk_note):
    """persistent 256x256 / 192x256 kernels, bf16 outputs: every fused epilogue kind (bias / GELU + aux / gelu' / residual
    add / column sums) on ragged edges, with more work items than workgroups (ring position and next-tile
    prefetch carried across items) and with 1..5 k-tiles (shorter than the 4-stage ring)"""
    ops, H = _ops()
    A, B = _rand((M, K), dev, torch.bfloat16, seed=1), _rand((N, K), dev, torch.bfloat16, 0.2, seed=2)
    bias = _rand((N,), dev, seed=3)
    Af, Bf = A.float().cpu(), B.float().cpu()
    pre = Af @ Bf.t() + bias.cpu()
    H.set_gemm_tuning(tile=tile)
    try:
        C = torch.empty((M, N), dtype=torch.bfloat16, device=dev)
        aux = torch.empty_like(C)
        ops.gemm(A, B, C, M, N, K, K, K, N, False, False, bias=bias, aux=aux, epi=H.EPI_GELU)
        assert rel_err(aux, pre) < 2e-2
        assert rel_err(C, torch.nn.functional.gelu(pre)) < 2e-2
        C2 = torch.empty_like(C)
        ops.gemm(A, B, C2, M, N, K, K, K, N, False, False, bias=bias, epi=H.EPI_GELU)      # no aux: single pass
        assert torch.equal(C2, C)
        u = _rand((M, N), dev, torch.bfloat16, 1.5, seed=5)
        uf = u.float().cpu()
        cs = torch.zeros(N, dtype=torch.float32, device=dev)
        ops.gemm(A, B, C, M, N, K, K, K, N, False, False, aux=u, epi=H.EPI_DGELU, colsum=cs)
        phi = 0.5 * (1 + torch.erf(uf / 2 ** 0.5))
        dg = phi + uf * torch.exp(-0.5 * uf * uf) / (2 * 3.141592653589793) ** 0.5
        ref = (Af @ Bf.t()) * dg
        assert rel_err(C, ref) < 2e-2
        assert rel_err(cs, C.float().cpu().sum(0)) < 2e-3          # sums of the values as stored
        ops.gemm(A, B, C, M, N, K, K, K, N, False, False, bias=bias, aux=u, epi=H.EPI_ADD)
        assert rel_err(C, pre + uf) < 2e-2
    finally:
        H.set_gemm_tuning(tile=0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_gemm_epilogues(dev, dtype):
    ops, H = _ops()
    M, N, K = 200, 256, 128
    A, B = _rand((M, K), dev, dtype, seed=1), _rand((N, K), dev, dtype, 0.2, seed=2)
    bias = _rand((N,), dev, seed=3)
    pre = A.float().cpu() @ B.float().cpu().t() + bias.cpu()
    # GELU with saved pre-activation
    C = torch.empty((M, N), dtype=dtype, device=dev)
    U = torch.empty_like(C)
    ops.gemm(A, B, C, M, N, K, K, K, N, 0, 0, bias=bias, aux=U, epi=H.EPI_GELU)
    assert rel_err(U, pre) < TOL[dtype]
    assert rel_err(C, F.gelu(pre)) < TOL[dtype]
    # tanh
    ops.gemm(A, B, C, M, N, K, K, K, N, 0, 0, bias=bias, epi=H.EPI_TANH)
    assert rel_err(C, torch.tanh(pre)) < TOL[dtype]
    # dgelu / dtanh epilogues read aux at the output coordinates
    aux = _rand((M, N), dev, dtype, seed=5)
    ops.gemm(A, B, C, M, N, K, K, K, N, 0, 0, aux=aux, epi=H.EPI_DGELU)
    a = aux.float().cpu().requires_grad_(True)
    F.gelu(a).sum().backward()
    assert rel_err(C, (pre - bias.cpu()) * a.grad) < TOL[dtype] * 2
    ops.gemm(A, B, C, M, N, K, K, K, N, 0, 0, aux=aux, epi=H.EPI_DTANH)
    assert rel_err(C, (pre - bias.cpu()) * (1 - aux.float().cpu() ** 2)) < TOL[dtype] * 2


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("Mtok", [4096, 1000])
def test_gemm_weight_grad_splitk(dev, dtype, Mtok):
    """dW[N,K] += dY^T X : the split-K / float-atomic path (K of the GEMM = number of tokens)"""
    ops, H = _ops()
    N, K = 192, 128
    dY, X = _rand((Mtok, N), dev, dtype, seed=1), _rand((Mtok, K), dev, dtype, seed=2)
    dW = torch.ones((N, K), dtype=torch.float32, device=dev)
    ops.gemm(dY, X, dW, N, K, Mtok, N, K, K, 1, 1, acc=True)
    ref = dY.float().cpu().t() @ X.float().cpu() + 1.0
    assert rel_err(dW, ref) < 1e-4 if dtype == torch.float32 else rel_err(dW, ref) < 2e-3


@pytest.mark.parametrize("N,K,Mtok", [(768, 768, 768), (1536, 768, 960), (768, 3072, 8200), (304, 264, 4096), (300, 264, 4096)])
def test_gemm_weight_grad_fresh_buffer_needs_no_zero_fill(dev, N, K, Mtok):
    """dW = dY^T X into a FRESH float32 buffer (accumulate = 0): the persistent kernel still splits K through the context's
    workspace -- partial tiles in the fragment layout, the reduce pass WRITES their sum -- so the buffer needs no zero fill
    (the IAOG decoder's per-block weight gradients: 5 torch.zeros per block gone).  NaN-poisoned output, ragged tile edges."""
    ops, H = _ops()
    dY, X = _rand((Mtok, N), dev, torch.bfloat16, seed=1), _rand((Mtok, K), dev, torch.bfloat16, seed=2)
    dW = torch.full((N, K), float("nan"), dtype=torch.float32, device=dev)
    ops.gemm(dY, X, dW, N, K, Mtok, N, K, K, 1, 1)
    ref = dY.float().cpu().t() @ X.float().cpu()
    assert torch.isfinite(dW).all()
    assert rel_err(dW, ref) < 2e-3
    if N >= 256 and K >= 256 and N % 8 == 0:     # (rows of 300 bf16 are not 16-byte aligned: the generic kernel, by design)
        assert H.last_gemm_kernel() == "gemm_bf16_tile256_kernel<1,1,f32,NONE>"


@pytest.mark.parametrize("workspace", [True, False])
def test_gemm_weight_grad_splitk_workspace_and_atomics(dev, workspace):
    """the persistent kernel's two split-K reductions (partial tiles in a registered workspace + reduce pass, float
    atomics without one) give the same weight gradient; 9 tiles x 8 splits, ragged token count"""
    ops, H = _ops()
    N, K, Mtok = 768, 768, 8200
    dY, X = _rand((Mtok, N), dev, torch.bfloat16, seed=1), _rand((Mtok, K), dev, torch.bfloat16, seed=2)
    dW = torch.ones((N, K), dtype=torch.float32, device=dev)
    try:
        if not workspace:
            H.drop_gemm_workspace()        # a context without a workspace: k-split partials are added with float atomics
            H.check(H.lib().fcmf_gemm(H.gemm_ctx(), H.ptr(dY), H.ptr(X), H.ptr(dW), None, None, None, N, K, Mtok, N, K, K, 1, 1,
                                      H.dt(dY), H.dt(dW), H.EPI_NONE, 1, H.stream()), "fcmf_gemm")
            # ... and a NULL context (defaults) is legal too
            dW0 = torch.ones((N, K), dtype=torch.float32, device=dev)
            H.check(H.lib().fcmf_gemm(None, H.ptr(dY), H.ptr(X), H.ptr(dW0), None, None, None, N, K, Mtok, N, K, K, 1, 1,
                                      H.dt(dY), H.dt(dW0), H.EPI_NONE, 1, H.stream()), "fcmf_gemm")
            assert rel_err(dW0, dW) < 1e-5
        else:
            ops.gemm(dY, X, dW, N, K, Mtok, N, K, K, 1, 1, acc=True)
        assert H.last_gemm_kernel() == "gemm_bf16_tile256_kernel<1,1,f32,NONE>"
        ref = dY.float().cpu().t() @ X.float().cpu() + 1.0
        assert rel_err(dW, ref) < 2e-3
    finally:
        pass                               # (the next accumulate GEMM re-registers a workspace with its context)


def test_gemm_strided_rows(dev):
    """A row stride > K: the pooler's row-0 gather (mm_modeling.py:428) is just lda = S*H"""
    ops, H = _ops()
    x = _rand((6, 10, 64), dev, seed=1)
    w = _rand((32, 64), dev, seed=2)
    y = torch.empty((6, 32), device=dev)
    first = x[:, 0]
    ops.gemm(first, w, y, 6, 32, 64, first.stride(0), 64, 32, 0, 0)
    assert rel_err(y, x[:, 0].cpu() @ w.cpu().t()) < 2e-5


def test_vocab_linear_ragged_vocabulary_bf16(dev):
    """IAOG vocabulary projection (64001 rows in the reference: not a multiple of 8): the padded MFMA path must
    give the same logits and gradients as a plain linear layer, and leave the padding rows of the shadow at zero
    after an optimizer step refreshed it"""
    ops, H = _ops()
    from fcmf_framework.optimization import FusedAdamW
    V, K, M = 1003, 64, 70
    ops.set_compute_dtype(torch.bfloat16)
    ops.shadows.clear()
    try:
        w = torch.nn.Parameter(_rand((V, K), dev, seed=1) * 0.3)
        b = torch.nn.Parameter(_rand((V,), dev, seed=2))
        x = _rand((5, 14, K), dev, torch.bfloat16, seed=3).requires_grad_(True)
        y = ops.vocab_linear(x, w, b)
        assert y.shape == (5, 14, V)
        g = _rand(y.shape, dev, torch.bfloat16, seed=4)
        (y.float() * g.float()).sum().backward()
        xr = x.detach().float().cpu().requires_grad_(True)
        wr = w.detach().cpu().to(torch.bfloat16).float().requires_grad_(True)
        br = b.detach().cpu().clone().requires_grad_(True)
        ref = xr @ wr.t() + br
        (ref * g.float().cpu()).sum().backward()
        assert rel_err(y, ref) < 2e-2
        assert rel_err(x.grad, xr.grad) < 2e-2
        assert rel_err(w.grad, wr.grad) < 2e-2
        assert rel_err(b.grad, br.grad) < 2e-2
        pad = ops.shadows.padded(w)
        assert pad.shape[0] % 32 == 0 and pad.shape[0] >= V and float(pad[V:].abs().max()) == 0.0
        opt = FusedAdamW([w, b], lr=1e-2)
        opt.step(max_grad_norm=1.0)
        pad2 = ops.shadows.padded(w)
        assert pad2.data_ptr() == pad.data_ptr() and float(pad2[V:].abs().max()) == 0.0
        assert rel_err(pad2[:V], w.detach().to(torch.bfloat16)) < 1e-6
    finally:
        ops.set_compute_dtype(torch.float32)
        ops.shadows.clear()


def test_transposed_weight_shadow_follows_optimizer_steps(dev):
    """bf16 dX GEMMs multiply by a cached transposed copy of the float32 master weight: it must be rebuilt after a
    FusedAdamW step and after an in-place torch update (version counter)"""
    ops, H = _ops()
    from fcmf_framework.optimization import FusedAdamW
    ops.set_compute_dtype(torch.bfloat16)
    ops.shadows.clear()
    try:
        w = torch.nn.Parameter(_rand((96, 160), dev, seed=1) * 0.2)
        x = _rand((300, 160), dev, torch.bfloat16, seed=2)
        g = _rand((300, 96), dev, torch.bfloat16, seed=3)

        def dx_of():
            xi = x.clone().requires_grad_(True)
            ops.linear(xi, w).backward(g)
            return xi.grad.float().cpu()

        def ref():
            return g.float().cpu() @ w.detach().to(torch.bfloat16).float().cpu()

        assert rel_err(dx_of(), ref()) < 2e-2
        wt0 = ops.shadows.get_t(w).clone()
        opt = FusedAdamW([w], lr=5e-2)
        w.grad = torch.ones_like(w)
        opt.step()
        assert rel_err(dx_of(), ref()) < 2e-2
        assert not torch.equal(ops.shadows.get_t(w), wt0)
        with torch.no_grad():
            w.mul_(-1.5)                      # in-place torch update: only the version counter tells
        assert rel_err(dx_of(), ref()) < 2e-2
        assert rel_err(ops.shadows.get_t(w).float().t(), w.detach().to(torch.bfloat16).float()) < 1e-6
    finally:
        ops.set_compute_dtype(torch.float32)
        ops.shadows.clear()


def test_colsum(dev):
    ops, H = _ops()
    for dtype in (torch.float32, torch.bfloat16):
        x = _rand((1037, 200), dev, dtype)
        assert rel_err(ops.colsum(x, 1037, 200, 200), x.float().cpu().sum(0)) < 1e-3


# ---------------------------------------------------------------------------------------
def _attn_ref(q, k1, v1, k2, v2, mask, bias, heads, group_div, scale, causal=False):
    """plain torch restatement of the two-segment attention (float64 for a tight reference)"""
    G, R, HD = q.shape
    d = HD // heads
    outs = []
    for g in range(G):
        g2 = g // group_div
        rows = []
        for r in range(R):
            ks, vs = [], []
            if k1 is not None:
                ks.append(k1[g]); vs.append(v1[g])
            if k2 is not None:
                ks.append(k2[g2, r]); vs.append(v2[g2, r])
            Kc, Vc = torch.cat(ks, 0), torch.cat(vs, 0)                       # [T,HD]
            qh = q[g, r].view(heads, 1, d)
            kh = Kc.view(-1, heads, d).transpose(0, 1)
            vh = Vc.view(-1, heads, d).transpose(0, 1)
            s = (qh @ kh.transpose(1, 2)).squeeze(1) * scale                  # [heads,T]
            if mask is not None:
                s = s + mask[g][None, :]
            if bias is not None:
                s = s + bias[g2, :, r, :]
            if causal:
                t = torch.arange(s.shape[1])
                s = torch.where(t[None, :] > r, torch.full_like(s, -1e4), s)
            p = torch.softmax(s, -1)
            rows.append((p.unsqueeze(1) @ vh).reshape(HD))
        outs.append(torch.stack(rows))
    return torch.stack(outs)


ATTN_CASES = [
    # G, R, heads, d, T1, T2, group_div, mask, bias, causal
    (3, 20, 4, 16, 20, 0, 1, True, False, False),     # plain self attention
    (4, 3, 2, 16, 10, 7, 2, True, False, False),      # shared + private segment, groups share K2
    (4, 3, 2, 16, 0, 9, 2, True, False, False),       # private segment only (pruned cross attention)
    (2, 9, 8, 12, 9, 0, 1, False, True, False),       # box attention: bias, d_k = 96/8
    (2, 6, 2, 96, 6, 0, 1, False, True, False),       # head dim > 64
    (2, 5, 4, 16, 170, 0, 1, True, False, False),     # T1 > 128: two backward key chunks
    (2, 7, 2, 64, 128, 36, 1, True, False, False),    # the pruned mm layer geometry
    (3, 6, 4, 16, 6, 0, 1, False, False, True),       # causal fill (IAOG decoder)
    (1, 150, 2, 64, 130, 20, 1, True, False, False),  # rows staged in several blocks x two key chunks x private keys
    (2, 40, 3, 20, 33, 5, 2, True, True, False),      # head dim not a multiple of 8: scalar staging / dot paths, bias + groups
    (12, 7, 3, 64, 128, 36, 6, True, False, False),   # the step's text+ROI layer: 6 aspects share the 36 private ROI keys (8 waves, d = 64)
    (12, 7, 3, 64, 0, 49, 6, True, False, False),     # the step's text->patch cross attention: private keys only, 6 aspects per review
    (6, 5, 2, 64, 40, 70, 3, True, False, False),     # > 64 private keys: three rounds of the 16-byte private-key walk
    (16, 3, 2, 16, 10, 7, 16, True, False, False),    # group of 16 > 8: per-group rows + host-side sum (ungrouped fallback)
    (4, 36, 8, 96, 36, 0, 1, False, True, False),     # the step's ROI box attention (bf16: the all-in-LDS "tiny dense" kernels)
    (4, 36, 8, 96, 36, 0, 2, True, True, False),      # the same with a key mask and a bias shared by groups of 2
    (2, 64, 2, 64, 64, 0, 1, True, False, False),     # the tiny kernels' limits: 64 rows x 64 keys
    (2, 65, 2, 64, 64, 0, 1, True, False, False),     # one row more: the row-blocked backward, all 65 rows in one block (the forward stays the 64-key kernel)
    (2, 100, 8, 128, 100, 0, 1, False, True, False),  # FCMF-large's ROI box attention: 100 x 100, heads of 128 (two row blocks)
    (4, 100, 2, 128, 100, 0, 2, True, True, False),   # the same with a key mask and a bias shared by groups of 2
    (2, 128, 2, 64, 128, 0, 1, True, True, False),    # the wide kernels' limits: 128 rows x 128 keys
    (2, 128, 1, 128, 128, 0, 1, True, False, False),  # ... with heads of 128: the backward in six blocks of 22 rows (forward: general kernel)
    (2, 30, 2, 96, 100, 0, 1, True, True, False),     # few rows, > 64 keys
    (2, 100, 2, 96, 30, 0, 1, False, True, False),    # > 64 rows, few keys
    (2, 129, 2, 64, 64, 0, 1, True, False, False),    # one row more than the wide limit: the general kernel
    (2, 16, 2, 128, 100, 20, 1, True, False, False),  # the flat kernels' row limit, but heads of 128: 65 KiB of LDS, past their 64 -- the general kernels
    (3, 1, 2, 64, 0, 2, 1, False, False, False),      # the flat few-rows kernels: one row, two private keys
    (6, 2, 4, 32, 17, 3, 3, True, False, False),      # ... groups of 3, odd key counts
    (2, 17, 2, 64, 100, 20, 1, True, False, False),   # one row past the flat kernels' limit: the general kernels
]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", ATTN_CASES)
def test_attention_fwd_bwd(dev, dtype, case):
    ops, H = _ops()
    G, R, heads, d, T1, T2, gd, use_mask, use_bias, causal = case
    HD, T = heads * d, T1 + T2
    mk = lambda shape, s: _rand(shape, dev, dtype, 0.7, seed=s).requires_grad_(True)
    q = mk((G, R, HD), 1)
    k1 = mk((G, T1, HD), 2) if T1 else None
    v1 = mk((G, T1, HD), 3) if T1 else None
    k2 = mk((G // gd, R, T2, HD), 4) if T2 else None
    v2 = mk((G // gd, R, T2, HD), 5) if T2 else None
    mask = None
    if use_mask:
        m01 = (torch.rand(G, T, generator=torch.Generator().manual_seed(7)) > 0.2).float()
        m01[:, 0] = 1
        mask = ((1 - m01) * -10000.0).to(dev)
    bias = (_rand((G // gd, heads, R, T), dev, seed=8).requires_grad_(True)) if use_bias else None
    out = ops.attention(q, k1, v1, k2, v2, mask=mask, bias=bias, heads=heads, group_div=gd, causal=causal)
    w = _rand(out.shape, dev, dtype, seed=9)
    (out.float() * w.float()).sum().backward()

    c = lambda t: None if t is None else t.detach().double().cpu().requires_grad_(True)
    qr, k1r, v1r, k2r, v2r, br = c(q), c(k1), c(v1), c(k2), c(v2), c(bias)
    ref = _attn_ref(qr, k1r, v1r, k2r, v2r, None if mask is None else mask.double().cpu(), br, heads, gd,
                    1 / math.sqrt(d), causal)
    (ref * w.double().cpu()).sum().backward()
    tol = 3e-5 if dtype == torch.float32 else 3e-2
    assert rel_err(out, ref) < tol
    for name, a, b in (("dq", q, qr), ("dk1", k1, k1r), ("dv1", v1, v1r), ("dk2", k2, k2r), ("dv2", v2, v2r),
                       ("dbias", bias, br)):
        if a is not None:
            assert rel_err(a.grad, b.grad) < tol * 2, name


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_attention_expanded_query_rows_read_in_place(dev, dtype):
    """one query row per group expanded over R rows (row stride 0: the [CLS] query against each image's private keys,
    fcmf_pretraining.py:84-93) is read in place: same output and gradients as the materialised copy, bit for bit"""
    ops, H = _ops()
    G, R, heads, d, T2, gd = 12, 7, 3, 64, 49, 6
    HD = heads * d
    q1 = _rand((G, HD), dev, dtype, 0.7, seed=1)
    k2 = _rand((G // gd, R, T2, HD), dev, dtype, 0.7, seed=2)
    v2 = _rand((G // gd, R, T2, HD), dev, dtype, 0.7, seed=3)
    w = _rand((G, R, HD), dev, dtype, seed=4)
    res = []
    for materialise in (False, True):
        qa = q1.clone().requires_grad_(True)
        ka, va = k2.clone().requires_grad_(True), v2.clone().requires_grad_(True)
        q = qa.unsqueeze(1).expand(G, R, HD)
        assert q.stride(1) == 0
        if materialise:
            q = q.contiguous()
        out = ops.attention(q, k2=ka, v2=va, heads=heads, group_div=gd)
        (out.float() * w.float()).sum().backward()
        res.append((out.detach(), qa.grad, ka.grad, va.grad))
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_attention_few_rows_dropout_consistent(dev):
    """the flat few-rows kernels (bf16, R <= 16, shared + private keys): with V = I split over the two segments the output IS the
    dropped probability matrix; kept entries are the plain probabilities / (1 - p), and the backward regenerates the same mask
    (dV1 = P_drop[:, :T1]^T dO, dV2 = P_drop[:, T1:] per row)"""
    ops, H = _ops()
    G, R, T1, T2, p = 5, 7, 32, 32, 0.3
    d = T1 + T2
    eye = torch.eye(d, device=dev, dtype=torch.bfloat16)
    q = _rand((G, R, d), dev, torch.bfloat16, seed=1)
    k1 = _rand((G, T1, d), dev, torch.bfloat16, seed=2)
    k2 = _rand((G, R, T2, d), dev, torch.bfloat16, seed=3)
    v1 = eye[:T1].expand(G, T1, d).contiguous().requires_grad_(True)
    v2 = eye[T1:].expand(G, R, T2, d).contiguous().requires_grad_(True)
    ops.manual_seed(77)
    out = ops.attention(q, k1, v1, k2, v2, heads=1, p=p, training=True)
    plain = ops.attention(q, k1, v1, k2, v2, heads=1, p=0.0, training=False)
    pdrop, pfull = out.detach().float(), plain.detach().float()
    kept = pdrop != 0
    assert 0.55 < kept.float().mean().item() < 0.85
    assert torch.allclose(pdrop[kept], pfull[kept] / (1 - p), rtol=2e-2, atol=1e-3)
    out.sum().backward()                                   # dO = 1
    assert torch.allclose(v1.grad.float()[:, :, 0], pdrop[:, :, :T1].sum(1), rtol=2e-2, atol=2e-2)
    assert torch.allclose(v2.grad.float()[:, :, :, 0], pdrop[:, :, T1:], rtol=2e-2, atol=2e-2)


@pytest.mark.parametrize("R,T", [(16, 16), (100, 104), (128, 128)])
def test_attention_tiny_dropout_consistent(dev, R, T):
    """the all-in-LDS kernels (bf16, <= 64 rows / keys; wide / row-blocked up to 128): with V = I the output IS the dropped
    probability matrix; kept entries are the plain probabilities / (1 - p), and the backward uses the same mask (dV = P_drop^T dO)."""
    ops, H = _ops()
    G, p = 6, 0.3
    q = _rand((G, R, T), dev, torch.bfloat16, seed=1)
    k = _rand((G, T, T), dev, torch.bfloat16, seed=2)
    v = torch.eye(T, device=dev, dtype=torch.bfloat16).expand(G, T, T).contiguous().requires_grad_(True)
    ops.manual_seed(321)
    out = ops.attention(q, k, v, heads=1, p=p, training=True)
    plain = ops.attention(q, k, v, heads=1, p=0.0, training=False)
    pdrop, pfull = out.detach().float(), plain.detach().float()
    kept = pdrop != 0
    assert 0.55 < kept.float().mean().item() < 0.85
    assert torch.allclose(pdrop[kept], pfull[kept] / (1 - p), rtol=2e-2, atol=1e-3)
    out.sum().backward()                       # dO = 1: dV[t][c] = sum_r P_drop[r][t] for every column c
    assert torch.allclose(v.grad.float()[:, :, 0], pdrop.sum(1), rtol=2e-2, atol=2e-2)


def test_attention_dropout_consistent(dev):
    """with p>0 the forward is out = P_drop V; recover P_drop with V = I and check that the
    backward uses the same mask (dV = P_drop^T dO) and that kept entries are scaled by 1/(1-p)."""
    ops, H = _ops()
    G, R, T, p = 5, 8, 8, 0.3
    q = _rand((G, R, T), dev, seed=1)
    k = _rand((G, T, T), dev, seed=2)
    v = torch.eye(T, device=dev).expand(G, T, T).contiguous().requires_grad_(True)
    ops.manual_seed(123)
    out = ops.attention(q, k, v, heads=1, p=p, training=True)
    ops.manual_seed(123)
    plain = ops.attention(q, k, v, heads=1, p=0.0, training=False)
    pdrop, pfull = out.detach(), plain.detach()
    kept = pdrop != 0
    assert 0.55 < kept.float().mean().item() < 0.85
    assert torch.allclose(pdrop[kept], pfull[kept] / (1 - p), rtol=1e-5, atol=1e-7)
    dO = _rand(out.shape, dev, seed=3)
    out.backward(dO)
    assert rel_err(v.grad, pdrop.transpose(1, 2) @ dO) < 1e-5


# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("H_", [64, 768, 1024])
def test_add_layer_norm(dev, dtype, H_):
    ops, H = _ops()
    rows = 37
    x = _rand((rows, H_), dev, dtype, seed=1).requires_grad_(True)
    big = _rand((rows, 3, H_), dev, dtype, seed=2).requires_grad_(True)
    g = (1 + 0.1 * _rand((H_,), dev, seed=3)).requires_grad_(True)
    b = _rand((H_,), dev, seed=4).requires_grad_(True)
    y = ops.add_layer_norm(x, big[:, 0], g, b, 1e-12)          # residual with a row stride
    w = _rand(y.shape, dev, seed=5)
    (y.float() * w).sum().backward()
    xr, rr, gr, br = (t.detach().float().cpu().requires_grad_(True) for t in (x, big, g, b))
    z = xr + rr[:, 0]
    u = z.mean(-1, keepdim=True)
    s = (z - u).pow(2).mean(-1, keepdim=True)
    ref = gr * ((z - u) / torch.sqrt(s + 1e-12)) + br
    (ref * w.cpu()).sum().backward()
    tol = 2e-5 if dtype == torch.float32 else 3e-2
    assert rel_err(y, ref) < tol
    assert rel_err(x.grad, xr.grad) < tol * 2
    assert rel_err(big.grad, rr.grad) < tol * 2
    assert rel_err(g.grad, gr.grad) < tol * 2
    assert rel_err(b.grad, br.grad) < tol * 2


def test_add_layer_norm_dropout(dev):
    ops, H = _ops()
    rows, H_, p = 64, 256, 0.25
    x = torch.ones((rows, H_), device=dev).requires_grad_(True)
    g = torch.ones(H_, device=dev)
    b = torch.zeros(H_, device=dev)
    from fcmf_framework.ops import AddLNFn
    seed = 99
    y = AddLNFn.apply(x, None, g, b, 1e-5, p, seed)
    # same seed -> same mask via the standalone dropout kernel (index convention row*H + col)
    mult = ops.DropoutFn.apply(torch.ones_like(x), p, seed).detach()
    assert 0.65 < (mult != 0).float().mean().item() < 0.85
    ref = F.layer_norm(mult.cpu(), (H_,), eps=1e-5)
    assert max_err(y, ref) < 1e-4
    w = _rand(y.shape, dev, seed=1)
    (y * w).sum().backward()
    zr = mult.cpu().clone().requires_grad_(True)
    (F.layer_norm(zr, (H_,), eps=1e-5) * w.cpu()).sum().backward()
    assert rel_err(x.grad, zr.grad * mult.cpu()) < 1e-4


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,S,H_", [(4, 12, 64), (70, 9, 768), (5, 12, 36)])      # (70 sequences: two sequence groups of the fused
def test_embedding_layer_norm(dev, dtype, B, S, H_):                              #  position + type gradient kernel; H 36: its fallback)
    ops, H = _ops()
    V, Pn, pad = 50, 40, 1
    ids = torch.randint(3, V, (B, S), generator=torch.Generator().manual_seed(1))
    ids[0, 7:] = pad
    ids[2, 3:] = pad
    ids[3, 0] = pad        # a leading pad: this sequence's position ids lag the others' at every offset (the
    ids[1, 5] = pad        # per-token fallback of the position-gradient kernel), an interior pad likewise
    word, ptab, ttab = (_rand(s, dev, seed=i).requires_grad_(True) for i, s in enumerate(((V, H_), (Pn, H_), (2, H_))))
    g = (1 + 0.1 * _rand((H_,), dev, seed=7)).requires_grad_(True)
    b = _rand((H_,), dev, seed=8).requires_grad_(True)
    tt = torch.zeros_like(ids)
    tt[1] = 1
    idd, ttd = ids.to(dev), tt.to(dev)
    pos = ops.position_ids(idd, pad)
    m = ids.ne(pad).int()
    pos_ref = (torch.cumsum(m, 1) * m).long() + pad
    assert torch.equal(pos.cpu(), pos_ref)
    y = ops.embed_layer_norm(idd, pos, ttd, word, ptab, ttab, g, b, 1e-5, 0.0, False, pad, dtype)
    w = _rand(y.shape, dev, seed=9)
    (y.float() * w).sum().backward()
    wr, pr, tr, gr, br = (t.detach().cpu().requires_grad_(True) for t in (word, ptab, ttab, g, b))
    e = F.embedding(ids, wr, padding_idx=pad) + tr[tt] + F.embedding(pos_ref, pr, padding_idx=pad)
    ref = F.layer_norm(e, (H_,), gr, br, 1e-5)
    (ref * w.cpu()).sum().backward()
    tol = 2e-5 if dtype == torch.float32 else 3e-2
    assert rel_err(y, ref) < tol
    for a, r in ((word, wr), (ptab, pr), (ttab, tr), (g, gr), (b, br)):
        assert rel_err(a.grad, r.grad) < tol * 2


# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("cdtype", [torch.float64, torch.float32])
def test_box_bias(dev, cdtype):
    ops, H = _ops()
    from oracle import fcmf_oracle as O
    rng = np.random.Generator(np.random.PCG64(3))
    G, N = 3, 7
    xs, ys = np.sort(rng.random((G, N, 2)), -1), np.sort(rng.random((G, N, 2)), -1)
    c = torch.from_numpy(np.concatenate([xs, ys], -1)).to(cdtype)
    c[1, 5:] = 0
    emb = ops.box_embedding(c.to(dev))
    ref_emb = O.box_relational_embedding(c).float()
    assert max_err(emb, ref_emb) < (1e-6 if cdtype == torch.float64 else 2e-3)
    ww = (0.1 * _rand((8, 64), dev, seed=1) + 0.05).requires_grad_(True)
    wb = (0.1 * _rand((8,), dev, seed=2)).requires_grad_(True)
    bias = ops.box_bias(c.to(dev), ww, wb)
    wgt = _rand(bias.shape, dev, seed=3)
    (bias * wgt).sum().backward()
    wr, br = ww.detach().cpu().requires_grad_(True), wb.detach().cpu().requires_grad_(True)
    pre = torch.einsum("gije,he->ghij", ref_emb, wr) + br.view(1, 8, 1, 1)
    ref = torch.log(torch.clamp(F.relu(pre), min=1e-6))
    (ref * wgt.cpu()).sum().backward()
    tol = 1e-4 if cdtype == torch.float64 else 5e-3
    live = ref > math.log(2e-6)            # away from the clamp boundary
    assert (bias.cpu()[live] - ref[live]).abs().max().item() < tol
    gtol = 1e-3 if cdtype == torch.float64 else 1e-2   # 1/x near the clamp amplifies f32-coordinate rounding
    assert rel_err(ww.grad, wr.grad) < gtol and rel_err(wb.grad, br.grad) < gtol


def test_box_bias_bf16_mode_fast_trig(dev):
    """bf16 compute mode: float32 coordinates and the hardware's sine / cosine (FCMF_BOX_FAST_TRIG).  The bias -- which the
    attention consumes in bf16 (rounding 3e-2 at its typical magnitude) -- stays within 1e-2 of the float64 reference where the
    pre-activation is not small (2e-3 in the pre-activation everywhere); the WG gradients within 2e-2 when the upstream
    gradient leaves out the entries next to the clamp (d log x = dx / x: there ANY arithmetic's last digits decide the sum)."""
    ops, H = _ops()
    from oracle import fcmf_oracle as O
    rng = np.random.Generator(np.random.PCG64(5))
    G, N = 4, 36
    xs, ys = np.sort(rng.random((G, N, 2)), -1) * 200, np.sort(rng.random((G, N, 2)), -1) * 150
    c = torch.from_numpy(np.concatenate([xs, ys], -1))
    c[1, 30:] = 0
    ref_emb = O.box_relational_embedding(c).float()
    ww = (0.1 * _rand((8, 64), dev, seed=1) + 0.05).requires_grad_(True)
    wb = (0.1 * _rand((8,), dev, seed=2)).requires_grad_(True)
    wr, br = ww.detach().cpu().requires_grad_(True), wb.detach().cpu().requires_grad_(True)
    pre = torch.einsum("gije,he->ghij", ref_emb, wr) + br.view(1, 8, 1, 1)
    ref = torch.log(torch.clamp(F.relu(pre), min=1e-6))
    wgt = _rand(ref.shape, "cpu", seed=3) * (pre.detach() > 0.1)
    (ref * wgt).sum().backward()
    ops.set_compute_dtype(torch.bfloat16)
    try:
        bias = ops.box_bias(c.to(dev), ww, wb)
        (bias * wgt.to(dev)).sum().backward()
    finally:
        ops.set_compute_dtype(torch.float32)
    live = pre > 1e-2
    assert live.float().mean() > 0.5
    assert (torch.exp(bias.detach().cpu()[live]) - pre.detach()[live]).abs().max().item() < 2e-3
    big = pre > 0.2
    assert (bias.detach().cpu()[big] - ref.detach()[big]).abs().max().item() < 1e-2
    assert rel_err(ww.grad, wr.grad) < 2e-2 and rel_err(wb.grad, br.grad) < 2e-2


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_cross_entropy(dev, dtype):
    ops, H = _ops()
    n, C = 37, 4
    lg = _rand((n, C), dev, dtype, 2.0, seed=1).requires_grad_(True)
    lb = torch.randint(0, C, (n,), generator=torch.Generator().manual_seed(2))
    lb[5] = -100
    loss = ops.cross_entropy(lg, lb.to(dev))
    (loss * 3.0).backward()
    lr = lg.detach().float().cpu().requires_grad_(True)
    ref = F.cross_entropy(lr, lb, ignore_index=-100)
    (ref * 3.0).backward()
    tol = 1e-5 if dtype == torch.float32 else 2e-2
    assert abs(loss.item() - ref.item()) < tol * max(1, abs(ref.item()))
    assert rel_err(lg.grad, lr.grad) < tol * 2


def test_cross_entropy_mult_and_all_ignored(dev):
    """ops.cross_entropy(..., mult=A) = A x the mean over the non-ignored rows (the driver's sum of the 6 aspects' batch
    means, run_multimodal_fcmf.py:463-475) with its gradient; every row ignored: NaN loss as torch, zero gradient rows"""
    ops, H = _ops()
    n, C, A = 384, 4, 6
    lg = _rand((n, C), dev, torch.float32, 2.0, seed=1).requires_grad_(True)
    lb = torch.randint(0, C, (n,), generator=torch.Generator().manual_seed(2))
    lb[::7] = -100
    loss = ops.cross_entropy(lg, lb.to(dev), mult=float(A))
    (loss / 2).backward()
    lr = lg.detach().cpu().double().requires_grad_(True)
    ref = F.cross_entropy(lr, lb, ignore_index=-100) * A
    (ref / 2).backward()
    assert abs(loss.item() - ref.item()) < 1e-6 * abs(ref.item())
    assert rel_err(lg.grad, lr.grad) < 1e-6
    lg2 = _rand((5, C), dev, torch.float32, 2.0, seed=3).requires_grad_(True)
    dead = ops.cross_entropy(lg2, torch.full((5,), -100, device=dev))
    assert torch.isnan(dead).item()
    dead.backward()
    assert not lg2.grad.any()


@pytest.mark.parametrize("value", [-10000.0, float(torch.finfo(torch.float32).min)])
def test_additive_mask_matches_torch_formula(dev, value):
    """layers.additive_mask on an int64 0 / 1 mask (one launch, fcmf_additive_mask) == (1 - mask[:, :L]) * value, bit for
    bit, for a leading slice of a wider mask (fcmf_pretraining.py:53-56,97-100,133-136; HF extended mask = finfo.min)"""
    from fcmf_framework import layers
    m = (torch.rand(37, 190, generator=torch.Generator().manual_seed(1)) > 0.3).long().to(dev)
    for Lc in (190, 164, 49, 15, 1):
        got = layers.additive_mask(m, Lc, value)
        want = (1.0 - m[:, :Lc].float()) * value
        assert got.dtype == torch.float32 and got.shape == (37, Lc)
        assert torch.equal(got, want)
    _, H = _ops()
    out = torch.empty(4, device=dev)
    assert H.lib().fcmf_additive_mask(H.ptr(m), 2, H.ptr(out), 1, 4, -1.0, 0) == -1      # row stride < columns


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C,ld", [(64001, 64032), (64001, 64001), (2048, 2048), (1500, 1504)])
def test_cross_entropy_wide_vocabulary(dev, dtype, C, ld):
    """the IAOG loss over a wide, possibly ragged class axis read with a row stride (the column-padded logits buffer):
    16-byte path (aligned rows) and scalar path (odd row stride), ignored rows, and the in-place backward"""
    ops, H = _ops()
    n = 21
    buf = _rand((n, ld), dev, dtype, 3.0, seed=1)
    lg = buf[:, :C]
    lb = torch.randint(0, C, (n,), generator=torch.Generator().manual_seed(2))
    lb[3] = -100
    lb[7] = C - 1
    lbd = lb.to(dev)
    rows = torch.empty(n, dtype=torch.float32, device=dev)
    nvalid = torch.zeros(1, dtype=torch.float32, device=dev)
    H.check(H.lib().fcmf_xent_fwd(H.ptr(buf), ld, H.ptr(lbd), H.ptr(rows), H.ptr(nvalid), n, C, -100, H.dt(buf), H.stream()), "xent_fwd")
    lr = lg.detach().float().cpu().requires_grad_(True)
    ref_rows = F.cross_entropy(lr, lb, ignore_index=-100, reduction="none")
    tol = 1e-5 if dtype == torch.float32 else 2e-2
    assert int(nvalid.item()) == n - 1
    assert max_err(rows, ref_rows.detach()) < tol * 12
    ref_rows.sum().backward()
    scale = torch.full((1,), 0.5, dtype=torch.float32, device=dev)
    d = torch.full_like(buf, 7.0)
    H.check(H.lib().fcmf_xent_bwd(H.ptr(buf), ld, H.ptr(lbd), H.ptr(d), ld, H.ptr(scale), 2.0, n, C, -100, H.dt(buf), H.stream()), "xent_bwd")
    assert max_err(d[:, :C], lr.grad) < (1e-6 if dtype == torch.float32 else 4e-3)
    assert (d[:, C:] == 7.0).all()                              # columns past C are not touched
    keep = buf.clone()
    H.check(H.lib().fcmf_xent_bwd(H.ptr(buf), ld, H.ptr(lbd), H.ptr(buf), ld, H.ptr(scale), 2.0, n, C, -100, H.dt(buf), H.stream()), "xent_bwd")
    assert torch.equal(buf[:, :C], d[:, :C]) and torch.equal(buf[:, C:], keep[:, C:])     # in place == out of place


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_vocab_cross_entropy_fused_node(dev, dtype):
    """ops.vocab_cross_entropy == cross_entropy(vocab_linear(x)) (value and all three gradients), ragged vocabulary"""
    ops, H = _ops()
    ops.set_compute_dtype(dtype)
    ops.shadows.clear()
    try:
        V, K, B, Ld = 1999, 64, 3, 5
        w = _rand((V, K), dev, scale=0.3, seed=1).requires_grad_(True)
        b = _rand((V,), dev, scale=0.1, seed=2).requires_grad_(True)
        x = _rand((B, Ld, K), dev, dtype, seed=3).requires_grad_(True)
        lb = torch.randint(0, V, (B, Ld), generator=torch.Generator().manual_seed(4))
        lb[:, -1] = -100
        loss = ops.vocab_cross_entropy(x, w, b, lb.to(dev))
        loss.backward()
        xr, wr, br = (a.detach().float().cpu().requires_grad_(True) for a in (x, w, b))
        wc = wr if dtype == torch.float32 else wr.bfloat16().float()
        ref = F.cross_entropy(F.linear(xr, wc, br).permute(0, 2, 1), lb, ignore_index=-100)
        ref.backward()
        tol = 1e-5 if dtype == torch.float32 else 2e-2
        assert abs(loss.item() - ref.item()) < tol * abs(ref.item())
        for got, want in ((x.grad, xr.grad), (w.grad, wr.grad), (b.grad, br.grad)):
            assert rel_err(got, want) < (1e-4 if dtype == torch.float32 else 3e-2)
    finally:
        ops.set_compute_dtype(torch.float32)
        ops.shadows.clear()


# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_linear_and_ffn_autograd(dev, dtype):
    ops, H = _ops()
    x = _rand((5, 9, 64), dev, dtype, seed=1).requires_grad_(True)
    w1, b1 = _rand((128, 64), dev, scale=0.2, seed=2).requires_grad_(True), _rand((128,), dev, seed=3).requires_grad_(True)
    w2, b2 = _rand((64, 128), dev, scale=0.2, seed=4).requires_grad_(True), _rand((64,), dev, seed=5).requires_grad_(True)
    y = ops.ffn(x, w1, b1, w2, b2)
    t = ops.linear(y, w1, b1, act="tanh")
    wgt = _rand(t.shape, dev, seed=6)
    (t.float() * wgt).sum().backward()
    xr, w1r, b1r, w2r, b2r = (a.detach().float().cpu().requires_grad_(True) for a in (x, w1, b1, w2, b2))
    w1c, w2c = (w1r, w2r) if dtype == torch.float32 else (w1r.bfloat16().float(), w2r.bfloat16().float())
    yr = F.linear(F.gelu(F.linear(xr, w1c, b1r)), w2c, b2r)
    tr = torch.tanh(F.linear(yr, w1c, b1r))
    (tr * wgt.cpu()).sum().backward()
    tol = 3e-5 if dtype == torch.float32 else 4e-2
    assert rel_err(t, tr) < tol
    for a, r in ((x, xr), (w1, w1r), (b1, b1r), (w2, w2r), (b2, b2r)):
        assert rel_err(a.grad, r.grad) < tol * 2


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_shared_input_projections_as_one_node(dev, dtype):
    """ops.linear_multi (q / k / v of the box attention, key / value pairs on one input) and ops.seq_fan (key / value projections +
    the [CLS] row of the text encoder's output): outputs and every gradient equal the separate nn.Linear / slicing graph
    (roi_modeling.py:170-173, fcmf_pretraining.py:97-124) -- the input gradient is accumulated by the dX GEMMs' add epilogue,
    the [CLS] gradient lands in row 0; a weight shared between two projections accumulates in place; an unused output is fine"""
    ops, H = _ops()
    G, S, Hd = 6, 10, 64
    x = _rand((G, S, Hd), dev, dtype, seed=1).requires_grad_(True)
    ws = [_rand((Hd, Hd), dev, scale=0.2, seed=2 + i).requires_grad_(True) for i in range(3)]
    bs = [_rand((Hd,), dev, seed=7 + i).requires_grad_(True) for i in range(3)]
    wg = [_rand((G, S, Hd), dev, seed=20 + i) for i in range(3)]
    wc = _rand((G, Hd), dev, seed=30)
    q, k, v = ops.linear_multi(x, ws[0], bs[0], ws[1], bs[1], ws[2], bs[2])
    k2, v2, cls = ops.seq_fan(x, ws[1], bs[1], ws[2], None)                 # (weights 1 and 2 used a second time; one without bias)
    loss = sum((t.float() * w_).sum() for t, w_ in zip((q, k, v), wg)) + (k2.float() * wg[0]).sum() + (cls.float() * wc).sum()
    loss.backward()                                                          # (v2 unused: its gradient arrives as None)
    xr = x.detach().float().cpu().requires_grad_(True)
    wr = [w.detach().cpu().requires_grad_(True) for w in ws]
    br = [b.detach().cpu().requires_grad_(True) for b in bs]
    wcast = (lambda w: w) if dtype == torch.float32 else (lambda w: w.bfloat16().float())
    qr, kr, vr = (F.linear(xr, wcast(wr[i]), br[i]) for i in range(3))
    k2r = F.linear(xr, wcast(wr[1]), br[1])
    ref = sum((t * w_.cpu()).sum() for t, w_ in zip((qr, kr, vr), wg)) + (k2r * wg[0].cpu()).sum() + (xr[:, 0] * wc.cpu()).sum()
    ref.backward()
    tol = 3e-5 if dtype == torch.float32 else 3e-2
    for a, r in ((q, qr), (k, kr), (v, vr), (k2, k2r), (v2, F.linear(xr, wcast(wr[2]))), (cls, xr[:, 0])):
        assert rel_err(a, r) < tol
    assert rel_err(x.grad, xr.grad) < tol * 2
    for a, r in zip(ws + bs, wr + br):
        assert rel_err(a.grad, r.grad) < tol * 2


def test_fused_adamw_matches_torch(dev):
    """clip_grad_norm_(1.0) + torch.optim.AdamW (run_multimodal_fcmf.py:485-487) in two kernels"""
    from fcmf_framework.optimization import FusedAdamW
    shapes = [(300, 70), (70,), (1000, 33), (5,)]
    ps = [torch.nn.Parameter(_rand(s, dev, seed=i)) for i, s in enumerate(shapes)]
    rs = [torch.nn.Parameter(p.detach().cpu().clone()) for p in ps]
    groups = lambda q: [dict(params=[q[0], q[2]], weight_decay=0.01, lr=7e-5), dict(params=[q[1], q[3]], weight_decay=0.0, lr=7e-4)]
    opt, ref = FusedAdamW(groups(ps), lr=7e-4), torch.optim.AdamW(groups(rs), lr=7e-4)
    for it in range(3):
        for i, (p, r) in enumerate(zip(ps, rs)):
            g = _rand(p.shape, dev, scale=0.5 + it, seed=10 * it + i)
            p.grad, r.grad = g, g.cpu().clone()
        norm_ref = torch.nn.utils.clip_grad_norm_(rs, 1.0)
        ref.step()
        opt.step(max_grad_norm=1.0)
        assert abs(opt.grad_norm().item() - norm_ref.item()) < 1e-4 * norm_ref.item()
        for p, r in zip(ps, rs):
            assert max_err(p, r) < 2e-6


def test_fused_adamw_resumes_from_torch_adamw_checkpoint(dev):
    """a checkpoint written by the reference's torch.optim.AdamW (tensor `step`, its own exp_avg tensors) loads into
    FusedAdamW AFTER it has already stepped (cached pointer tables must be dropped) and the trajectories agree"""
    from fcmf_framework.optimization import FusedAdamW
    shapes = [(64, 48), (48,)]
    ps = [torch.nn.Parameter(_rand(s, dev, seed=i)) for i, s in enumerate(shapes)]
    rs = [torch.nn.Parameter(p.detach().cpu().clone()) for p in ps]
    opt, ref = FusedAdamW(ps, lr=1e-3), torch.optim.AdamW(rs, lr=1e-3)

    def both(it):
        for i, (p, r) in enumerate(zip(ps, rs)):
            g = _rand(p.shape, dev, scale=1.0, seed=100 + 10 * it + i)
            p.grad, r.grad = g, g.cpu().clone()
        ref.step()
        opt.step()
    both(0)
    for i, r in enumerate(rs):                       # the reference runs two more steps on its own
        r.grad = _rand(r.shape, dev, scale=1.0, seed=500 + i).cpu()
    ref.step()
    for p, r in zip(ps, rs):
        p.data.copy_(r.data.to(dev))
    sd = ref.state_dict()
    assert torch.is_tensor(sd["state"][0]["step"])
    opt.load_state_dict(sd)
    assert all(isinstance(st["step"], int) for st in opt.state.values())
    both(2)
    for p, r in zip(ps, rs):
        assert max_err(p, r) < 2e-6
    for p, r in zip(ps, rs):                         # the kernel wrote the LOADED moment tensors
        assert max_err(opt.state[p]["exp_avg"], ref.state[r]["exp_avg"]) < 1e-6


def test_transposed_weight_copies_refreshed_in_one_launch(dev):
    """the bf16 transposed copies the dX GEMMs read are rebuilt by ONE multi-tensor launch inside FusedAdamW.step: they
    must equal the transpose of the UPDATED weights (ragged tile edges included) without any lazy per-weight rebuild"""
    ops, H = _ops()
    from fcmf_framework.optimization import FusedAdamW
    ops.shadows.clear()
    ws = [torch.nn.Parameter(_rand(s, dev, seed=i)) for i, s in enumerate([(768, 96), (100, 200), (64, 64)])]
    bias = torch.nn.Parameter(_rand((96,), dev, seed=9))
    for w in ws:
        assert torch.equal(ops.shadows.get_t(w), w.detach().t().contiguous().bfloat16())
    opt = FusedAdamW(ws + [bias], lr=1e-2)
    for p in ws + [bias]:
        p.grad = _rand(p.shape, dev, seed=20 + p.numel() % 7)
    before = [w.detach().clone() for w in ws]
    opt.step()
    for w, b in zip(ws, before):
        ent = ops.shadows.lookup("t", w)
        assert ent.stale is False and ent.version == w._version  # fresh: nothing left to rebuild lazily
        assert not torch.equal(w.detach(), b)
        assert torch.equal(ent.payload, w.detach().t().contiguous().bfloat16())
    ops.shadows.clear()


def test_transposed_copies_of_freed_weights_are_dropped(dev):
    """round-2 advisor finding: `refresh_transposed` re-reads every cached source by RAW address.  A weight that has been
    freed (another model of the same process) must leave the cache before the pointer tables are built -- its address may
    be unmapped or belong to a different tensor by then -- and a new weight at a recycled address gets a fresh copy."""
    import gc
    ops, H = _ops()
    from fcmf_framework.optimization import FusedAdamW
    ops.shadows.clear()
    keep = torch.nn.Parameter(_rand((128, 64), dev, seed=1))
    gone = torch.nn.Parameter(_rand((256, 64), dev, seed=2))
    view_owner = torch.nn.Parameter(_rand((96, 64), dev, seed=3))
    ops.shadows.get_t(keep); ops.shadows.get_t(gone)
    ops.shadows.get_t(view_owner.detach()[:64], owner=view_owner)      # a temporary view keyed on its Parameter
    assert len(ops.shadows) == 3 and ops.shadows.lookup("t", gone) is not None
    del gone
    gc.collect()
    opt = FusedAdamW([keep], lr=1e-2)
    keep.grad = _rand(keep.shape, dev, seed=4)
    opt.step()                                                         # -> refresh_transposed()
    assert len(ops.shadows) == 2 and ops.shadows.lookup("t", view_owner.detach()[:64], owner=view_owner) is not None   # (gone's is the one dropped)
    assert torch.equal(ops.shadows.lookup("t", keep).payload, keep.detach().t().contiguous().bfloat16())
    # a NEW weight that lands on the recycled address is never served the dead weight's copy
    fresh = torch.nn.Parameter(_rand((256, 64), dev, seed=5))
    assert torch.equal(ops.shadows.get_t(fresh), fresh.detach().t().contiguous().bfloat16())
    ops.shadows.clear()


def test_bertadam_matches_golden(dev):
    import os
    from conftest import GOLD
    from fcmf_framework.optimization import BertAdam
    z = np.load(os.path.join(GOLD, "bertadam.npz"))
    p = torch.nn.Parameter(torch.from_numpy(z["p0"]).to(dev))
    opt = BertAdam([p], lr=1e-2, warmup=0.1, t_total=20, weight_decay=0.01)
    for i, g in enumerate(z["grads"]):
        p.grad = torch.from_numpy(g).to(dev)
        opt.step()
        assert max_err(p, torch.from_numpy(z["traj"][i])) < 1e-6
        assert abs(opt.get_lr()[0] - z["lrs"][i]) < 1e-9


# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [128, 77, 256, 130])
@pytest.mark.parametrize("p", [0.0, 0.2])
def test_attention_mfma_backward_column_sums(dev, T, p):
    """the fused q|k|v bias gradient: per-sequence column sums of dq | dk | dv out of the MFMA backward's f32
    accumulators == column sums of the dqkv it stores (to bf16 rounding of the stored values)"""
    from fcmf_framework import fused, ops
    G, heads, d = 5, 3, 64
    Hd = heads * d
    qkv = _rand((G * T, 3 * Hd), dev, torch.bfloat16, 0.8, seed=1)
    m01 = (torch.rand(G, T, generator=torch.Generator().manual_seed(7)) > 0.25).float()
    m01[:, 0] = 1
    mask = ((1 - m01) * torch.finfo(torch.float32).min).to(dev)
    out, lse = fused.self_attention_fwd(qkv, mask, G, T, Hd, heads, p, 11)
    dout = _rand((G * T, Hd), dev, torch.bfloat16, 1.0, seed=3)
    bg = torch.full((3 * Hd,), 0.25, dtype=torch.float32, device=dev)        # accumulated into
    dqkv = fused.self_attention_bwd(qkv, mask, out, lse, dout, G, T, Hd, heads, p, 11, bias_grad=bg)
    dqkv2 = fused.self_attention_bwd(qkv, mask, out, lse, dout, G, T, Hd, heads, p, 11)
    assert torch.equal(dqkv, dqkv2)
    ref = dqkv.float().sum(0) + 0.25
    assert (bg - ref).abs().max().item() < 2e-2 * ref.abs().max().item() + 1e-3


@pytest.mark.parametrize("T", [128, 256, 100])
@pytest.mark.parametrize("p", [0.0, 0.2])
def test_attention_mfma_padded_sequences_skip_is_exact(dev, T, p):
    """padding = a hard-masked (finfo.min) key suffix: the MFMA kernels skip the fully masked trailing key fragments /
    chunks.  Results must equal the VALU kernel's (same dropout seed) on every valid row, dk / dv of the padded keys must be
    exactly zero, and lengths 1 .. T (incl. chunk boundaries) must all work."""
    from fcmf_framework import ops
    heads, d = 2, 64
    HD = heads * d
    lens = [1, 5, 16, 17, 31, 32, 33, 63, 64, 65, 96, 97, T - 1, T]
    lens = [min(l, T) for l in lens]
    G = len(lens)
    mk = lambda shape, s: _rand(shape, dev, torch.bfloat16, 0.8, seed=s)
    q0, k0, v0 = mk((G, T, HD), 1), mk((G, T, HD), 2), mk((G, T, HD), 3)
    m01 = torch.zeros(G, T)
    for g, l in enumerate(lens):
        m01[g, :l] = 1
    mask = ((1 - m01) * torch.finfo(torch.float32).min).to(dev)
    w = mk((G, T, HD), 9)
    res = {}
    for use in (True, False):
        with mfma_attention(use):
            q, k, v = (t.clone().requires_grad_(True) for t in (q0, k0, v0))
            ops.manual_seed(5)
            out = ops.attention(q, k, v, mask=mask, heads=heads, p=p, training=p > 0)
            (out.float() * w.float()).sum().backward()
            res[use] = (out.detach(), q.grad, k.grad, v.grad)
    for a, b, name in zip(res[True], res[False], ("out", "dq", "dk", "dv")):
        assert rel_err(a, b) < 3e-2, name
    for g, l in enumerate(lens):           # padded keys receive exactly zero gradient
        assert not res[True][2][g, l:].any() and not res[True][3][g, l:].any()


@pytest.mark.parametrize("T", [128, 100, 48])      # (48: the VALU leg runs the one-block all-in-LDS kernels)
def test_attention_mfma_fully_masked_sequence_is_uniform(dev, T):
    """a sequence whose EVERY key carries the hard (finfo.min) mask: torch / the reference absorb the scores into finfo.min
    and softmax is uniform over all T keys (HF eager attention, modeling_roberta.py:158-183).  The MFMA kernels must not
    shorten such a row to its first key fragment (round-2 advisor finding): out = mean of V, dv = dout / T per key,
    in both the MFMA and the VALU kernel, next to a normal and a half-padded sequence in the same launch.
    The backward recomputes probabilities from the saved logsumexp, which for such a row is finfo.min itself (log T is absorbed)."""
    from fcmf_framework import ops
    heads, d = 2, 64
    HD = heads * d
    mk = lambda shape, s: _rand(shape, dev, torch.bfloat16, 0.8, seed=s)
    q0, k0, v0, w = mk((3, T, HD), 1), mk((3, T, HD), 2), mk((3, T, HD), 3), mk((3, T, HD), 4)
    m01 = torch.ones(3, T)
    m01[1] = 0                      # sequence 1: no live key at all
    m01[2, T // 2:] = 0
    mask = ((1 - m01) * torch.finfo(torch.float32).min).to(dev)
    # torch fp32 reference of the same op
    qr, kr, vr = (t.float().clone().requires_grad_(True) for t in (q0, k0, v0))
    sp = lambda t: t.view(3, T, heads, d).transpose(1, 2)
    sc = sp(qr) @ sp(kr).transpose(-1, -2) / math.sqrt(d) + mask[:, None, None, :]
    ref = (torch.softmax(sc, -1) @ sp(vr)).transpose(1, 2).reshape(3, T, HD)
    (ref * w.float()).sum().backward()
    for use in (True, False):
        with mfma_attention(use):
            q, k, v = (t.clone().requires_grad_(True) for t in (q0, k0, v0))
            out = ops.attention(q, k, v, mask=mask, heads=heads, p=0.0, training=False)
            (out.float() * w.float()).sum().backward()
        assert rel_err(out, ref) < 2e-2, use
        assert rel_err(v.grad, vr.grad) < 3e-2, use
        # (autograd semantics: the gradient flows through `scores + mask` with derivative 1 although finfo.min absorbs the
        #  scores in the forward, so dq / dk of the fully masked sequence are those of uniform probabilities, not zero)
        assert rel_err(q.grad, qr.grad) < 3e-2 and rel_err(k.grad, kr.grad) < 3e-2, use


@pytest.mark.parametrize("Tq,Tk", [(128, 128), (77, 128), (128, 50), (33, 17), (256, 256), (200, 256), (256, 150), (130, 129)])
@pytest.mark.parametrize("p", [0.0, 0.2])
def test_attention_mfma_matches_reference_and_valu_kernel(dev, Tq, Tk, p):
    """bf16 / head-dim-64 text-encoder attention on the MFMA kernel: against the fp64 reference
    (p = 0) and against the VALU kernel with the SAME dropout seed (identical masks by construction)"""
    from fcmf_framework import ops
    G, heads, d = 3, 2, 64
    HD = heads * d
    mk = lambda shape, s: _rand(shape, dev, torch.bfloat16, 0.8, seed=s)
    q0, k0, v0 = mk((G, Tq, HD), 1), mk((G, Tk, HD), 2), mk((G, Tk, HD), 3)
    m01 = (torch.rand(G, Tk, generator=torch.Generator().manual_seed(7)) > 0.25).float()
    m01[:, 0] = 1
    mask = ((1 - m01) * torch.finfo(torch.float32).min).to(dev)
    w = mk((G, Tq, HD), 9)
    res = {}
    for use in (True, False):
        with mfma_attention(use):
            q, k, v = (t.clone().requires_grad_(True) for t in (q0, k0, v0))
            ops.manual_seed(5)
            out = ops.attention(q, k, v, mask=mask, heads=heads, p=p, training=p > 0)
            (out.float() * w.float()).sum().backward()
            res[use] = (out.detach(), q.grad, k.grad, v.grad)
    for a, b, name in zip(res[True], res[False], ("out", "dq", "dk", "dv")):
        assert rel_err(a, b) < 3e-2, name
    if p == 0.0:
        c = lambda t: t.detach().double().cpu().requires_grad_(True)
        qr, kr, vr = c(q0), c(k0), c(v0)
        ref = _attn_ref(qr, kr, vr, None, None, mask.double().cpu(), None, heads, 1, 1 / math.sqrt(d))
        (ref * w.double().cpu()).sum().backward()
        for a, b, name in zip(res[True], (ref, qr.grad, kr.grad, vr.grad), ("out", "dq", "dk", "dv")):
            assert rel_err(a, b) < 3e-2, name


def test_dp_allreduce_bucket_c_abi_single_rank(dev):
    """the RCCL entry points of the C ABI (include/fcmf_hip.h `fcmf_dp_*`; reference: init_process_group("nccl") + DDP,
    run_multimodal_fcmf.py:169,237-240) on the one GPU of this box: unique id, a 1-rank communicator, the in-place mean of a
    float32 and of a bf16 bucket on a side stream (= identity at world size 1), argument errors, destroy.  The multi-rank
    exchange itself is covered by the gloo tests (tests/test_dp_gloo.py); RCCL across GPUs needs the 8-GPU node."""
    import ctypes
    ops, H = _ops()
    L = H.lib()
    uid = (ctypes.c_char * 128)()
    H.check(L.fcmf_dp_unique_id(ctypes.cast(uid, ctypes.c_void_p)), "fcmf_dp_unique_id")
    assert any(bytes(uid))
    h = ctypes.c_void_p()
    torch.cuda.set_device(dev)
    H.check(L.fcmf_dp_comm_create(ctypes.byref(h), ctypes.cast(uid, ctypes.c_void_p), 1, 0), "fcmf_dp_comm_create")
    assert h.value
    side = torch.cuda.Stream(device=dev)
    for dtype in (torch.float32, torch.bfloat16):
        buf = _rand((1 << 20,), dev, dtype, seed=3)
        want = buf.clone()
        side.wait_stream(torch.cuda.current_stream(dev))
        H.check(L.fcmf_dp_allreduce_bucket(h, H.ptr(buf), buf.numel(), H.dt(buf), 1, side.cuda_stream), "fcmf_dp_allreduce_bucket")
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize()
        assert torch.equal(buf, want)
    assert L.fcmf_dp_allreduce_bucket(h, 0, 4, H.F32, 1, 0) == -1                     # null buffer
    assert L.fcmf_dp_allreduce_bucket(h, H.ptr(buf), 4, H.F64, 1, 0) == -3            # unsupported dtype
    assert L.fcmf_dp_comm_create(ctypes.byref(ctypes.c_void_p()), ctypes.cast(uid, ctypes.c_void_p), 2, 5) == -1
    H.check(L.fcmf_dp_comm_destroy(h), "fcmf_dp_comm_destroy")


# ---------------------------------------------------------------------------------------------------------------------
# fp8 (e4m3) path of BASELINE configs[4]
# ---------------------------------------------------------------------------------------------------------------------
def _e4m3_decode(q):
    """uint8 e4m3fn bytes -> float32 (host restatement of the OCP format: bias 7, no infinities, 0x7F / 0xFF = NaN)"""
    q = q.cpu().to(torch.int32)
    sgn, e, m = (q >> 7) & 1, (q >> 3) & 15, q & 7
    mag = torch.where(e == 0, m.float() * 2.0 ** -9, (1.0 + m.float() / 8.0) * torch.pow(2.0, (e - 7).float()))
    return torch.where(sgn == 1, -mag, mag)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_quant_fp8_rows_matches_torch_float8(dev, dtype):
    """fcmf_quant_fp8_rows: scale = amax / 448 per row, round-to-nearest-even onto OCP e4m3fn -- bit for bit what
    torch's float8_e4m3fn cast gives for the same scaled values (zero rows, one huge outlier, ragged row count)"""
    ops, H = _ops()
    rows, K = 1003, 384
    x = _rand((rows, K), dev, dtype, 3.0, seed=1)
    x[5] = 0
    x[7, 11] = 3.0e4
    x[9] *= 1e-6
    q, sc = ops.quant_fp8_rows(x, rows, K, K)
    xf = x.float().cpu()
    amax = xf.abs().amax(1)
    want_sc = torch.where(amax > 0, amax * (1.0 / 448.0), torch.ones_like(amax))
    assert torch.allclose(sc.cpu(), want_sc, rtol=1e-6, atol=0)
    ref = (xf * (1.0 / sc.cpu())[:, None]).to(torch.float8_e4m3fn).view(torch.uint8)
    got = q.cpu()
    same = (got == ref) | (((got & 0x7F) == 0) & ((ref & 0x7F) == 0))            # +0 / -0
    assert same.all(), (same.numel() - same.sum().item())
    assert (_e4m3_decode(got).abs().amax(1)[amax > 0] == 448.0).all()           # every non-zero row uses the full range
    assert torch.equal(_e4m3_decode(ref), ref.view(torch.float8_e4m3fn).float())   # (the decoder itself against torch)


@pytest.mark.parametrize("epi", ["none", "gelu", "dgelu", "add"])
@pytest.mark.parametrize("M,N,K", [(1000, 776, 384), (4416, 4104, 128), (6144, 1024, 1024), (300, 256, 2048)])
def test_gemm_fp8_matches_dequantised_reference(dev, M, N, K, epi):
    """fcmf_gemm_fp8 on v_mfma_scale_f32_16x16x128_f8f6f4 against the SAME quantised operands multiplied in float64: pins the
    operand layout (32 consecutive k per lane group through the permuted LDS image), the unit block scales, the row-scale
    epilogue and every fused epilogue, on ragged M / N edges and 1..16 k-tiles.  Tolerance = float32 accumulation + the bf16
    rounding of the output."""
    ops, H = _ops()
    A, W = _rand((M, K), dev, torch.bfloat16, 1.0, seed=1), _rand((N, K), dev, torch.bfloat16, 0.2, seed=2)
    bias = _rand((N,), dev, seed=3)
    u = _rand((M, N), dev, torch.bfloat16, 1.5, seed=5)
    aq, sa = ops.quant_fp8_rows(A, M, K, K)
    wq, sw = ops.quant_fp8_rows(W, N, K, K)
    ref = (_e4m3_decode(aq).double() @ _e4m3_decode(wq).double().t()) * sa.cpu().double()[:, None] * sw.cpu().double()[None, :]
    C = torch.empty((M, N), dtype=torch.bfloat16, device=dev)
    aux = torch.empty_like(C)
    cs = torch.zeros(N, dtype=torch.float32, device=dev)
    uf = u.float().cpu().double()
    if epi == "none":
        ops.gemm_fp8(aq, sa, wq, sw, C, M, N, K, bias=bias, colsum=cs)
        want = ref + bias.cpu().double()
    elif epi == "gelu":
        ops.gemm_fp8(aq, sa, wq, sw, C, M, N, K, bias=bias, aux=aux, epi=H.EPI_GELU)
        pre = ref + bias.cpu().double()
        assert rel_err(aux, pre.float()) < 1e-2
        want = torch.nn.functional.gelu(pre)
    elif epi == "dgelu":
        ops.gemm_fp8(aq, sa, wq, sw, C, M, N, K, aux=u, epi=H.EPI_DGELU, colsum=cs)
        phi = 0.5 * (1 + torch.erf(uf / 2 ** 0.5))
        want = ref * (phi + uf * torch.exp(-0.5 * uf * uf) / (2 * 3.141592653589793) ** 0.5)
    else:
        ops.gemm_fp8(aq, sa, wq, sw, C, M, N, K, bias=bias, aux=u, epi=H.EPI_ADD)
        want = ref + bias.cpu().double() + uf
    assert H.last_gemm_kernel().startswith("gemm_fp8_tile192_kernel")
    assert rel_err(C, want.float()) < 1e-2, rel_err(C, want.float())           # bf16 output rounding (2^-9) of O(1) values
    if epi in ("none", "dgelu"):
        assert rel_err(cs, C.float().cpu().sum(0)) < 2e-3
    # and against the UNquantised product: the e4m3 quantisation noise itself (3 mantissa bits per operand, averaged over K)
    exact = A.float().cpu().double() @ W.float().cpu().double().t()
    noise = ((ref - exact).norm() / exact.norm()).item()
    assert noise < 6e-2, noise


def test_fp8_linear_layers_forward_backward(dev):
    """ops.set_fp8(True): nn.Linear forward and dX run on the e4m3 kernel (dW stays bf16), through the autograd Functions the
    model uses (ProjectFn, FFNFn): against the float64 reference within e4m3 quantisation noise, and the quantised weight copies
    follow the parameter (rebuilt after an optimizer step)"""
    ops, H = _ops()
    from fcmf_framework.optimization import FusedAdamW
    M, Hd, I = 2048, 1024, 4096
    ops.set_compute_dtype(torch.bfloat16)
    ops.shadows.clear()
    try:
        x0 = _rand((M, Hd), dev, torch.bfloat16, 1.0, seed=1)
        w1, b1 = torch.nn.Parameter(_rand((I, Hd), dev, scale=0.03, seed=2)), torch.nn.Parameter(_rand((I,), dev, scale=0.1, seed=3))
        w2, b2 = torch.nn.Parameter(_rand((Hd, I), dev, scale=0.03, seed=4)), torch.nn.Parameter(_rand((Hd,), dev, scale=0.1, seed=5))
        g = _rand((M, Hd), dev, torch.bfloat16, 1.0, seed=6)

        def run(fp8):
            ops.set_fp8(fp8)
            for p in (w1, b1, w2, b2):
                p.grad = None
            x = x0.clone().requires_grad_(True)
            y = ops.ffn(x, w1, b1, w2, b2)
            names = []
            ops.gemm_trace_begin()
            y2 = ops.ffn(x, w1, b1, w2, b2)
            (y2.float() * g.float()).sum().backward()
            names = [n for n, _, _ in ops.gemm_trace_end()]
            return y.detach().float().cpu(), x.grad.float().cpu(), w1.grad.float().cpu(), w2.grad.float().cpu(), names
        y8, dx8, dw1_8, dw2_8, n8 = run(True)
        y16, dx16, dw1_16, dw2_16, n16 = run(False)
        assert sum(n.startswith("gemm_fp8") for n in n8) == 4 and not any(n.startswith("gemm_fp8") for n in n16)   # 2 fwd + 2 dX
        assert sum("f32" in n for n in n8) == 2                                                                     # dW: bf16 operands
        xd, w1d, w2d = x0.float().cpu().double(), w1.detach().cpu().double(), w2.detach().cpu().double()
        pre = xd @ w1d.t() + b1.detach().cpu().double()
        yref = torch.nn.functional.gelu(pre) @ w2d.t() + b2.detach().cpu().double()
        e8, e16 = ((y8 - yref).norm() / yref.norm()).item(), ((y16 - yref).norm() / yref.norm()).item()
        assert e16 < 1e-2 and e8 < 6e-2, (e8, e16)
        for a8, a16, nm in ((dx8, dx16, "dx"), (dw1_8, dw1_16, "dw1"), (dw2_8, dw2_16, "dw2")):
            r = ((a8 - a16).norm() / a16.norm()).item()
            assert r < 8e-2, (nm, r)
        # the quantised copies follow the parameter
        ops.set_fp8(True)
        q_before = ops.shadows.get_fp8(w1)[0].clone()
        opt = FusedAdamW([w1, b1, w2, b2], lr=1e-2)
        opt.step()
        assert not torch.equal(ops.shadows.get_fp8(w1)[0], q_before)
        q, sc = ops.shadows.get_fp8(w1)
        q2, sc2 = ops.quant_fp8_rows(w1.detach().bfloat16(), I, Hd, Hd)
        assert torch.equal(q, q2) and torch.equal(sc, sc2)
    finally:
        ops.set_fp8(False)
        ops.set_compute_dtype(torch.float32)
        ops.shadows.clear()


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_layernorm_emits_the_fp8_copy_its_consumer_needs(dev, p):
    """fcmf_add_ln_fwd_fp8 / fcmf_add_ln_bwd_fp8: the e4m3 copy + row scales they emit are BIT-IDENTICAL to a separate
    fcmf_quant_fp8_rows pass over the bf16 tensor they store (y; the gradient into the producing Linear), and every other
    output is untouched -- the fp8 mode drops three quantisation passes per layer (ffn1 input, ffn2 / out-proj dX inputs)"""
    ops, H = _ops()
    rows, Hd = 1000, 1024
    x = _rand((rows, Hd), dev, torch.bfloat16, 1.0, seed=1)
    res = _rand((rows, Hd), dev, torch.bfloat16, 1.0, seed=2)
    g, b = _rand((Hd,), dev, seed=3) + 1.0, _rand((Hd,), dev, seed=4)
    z0, z1 = x.clone(), x.clone()                      # (the pre-LN sum overwrites the input, as in the fused layers)
    y0, m0, r0, none = ops.ln_fwd(z0, res, Hd, g, b, 1e-5, p, 77, z0)
    y1, m1, r1, (q, sc) = ops.ln_fwd(z1, res, Hd, g, b, 1e-5, p, 77, z1, quant=True)
    assert none is None and torch.equal(y0, y1) and torch.equal(z0, z1) and torch.equal(m0, m1) and torch.equal(r0, r1)
    q2, sc2 = ops.quant_fp8_rows(y1, rows, Hd, Hd)
    assert torch.equal(q, q2) and torch.equal(sc, sc2)
    dy = _rand((rows, Hd), dev, torch.bfloat16, 1.0, seed=5)
    outs = []
    for quant in (False, True):
        dg, db, dxs = (torch.zeros(Hd, device=dev) for _ in range(3))
        dz, dx, dq = ops.ln_bwd(dy, z1, g, m1, r1, p, 99, dg, db, dxs, quant=quant)
        outs.append((dz, dx, dg, db, dxs, dq))
    for a, b_ in zip(outs[0][:2], outs[1][:2]):
        assert torch.equal(a, b_)
    for a, b_ in zip(outs[0][2:5], outs[1][2:5]):      # (column sums: float atomics over 8 partial groups, order not fixed)
        assert rel_err(a, b_) < 1e-5
    q, sc = outs[1][5]
    q2, sc2 = ops.quant_fp8_rows(outs[1][1], rows, Hd, Hd)
    assert torch.equal(q, q2) and torch.equal(sc, sc2)


@pytest.mark.parametrize("count,N,K,Mtok,acc", [(12, 768, 768, 8200, 1), (40, 256, 512, 1024, 0), (3, 776, 520, 4096, 1), (5, 128, 768, 2048, 1),
                                                (1, 768, 768, 4096, 1), (7, 3072, 768, 2048, 0)])
def test_gemm_dw_batched_matches_separate_weight_gradients(dev, count, N, K, Mtok, acc):
    """fcmf_gemm_dw_batched (the tiles of `count` same-shape weight gradients as ONE work list of the persistent kernel, k-split
    chosen for whole rounds, batched reduce pass) against `count` fcmf_gemm calls and the float64 product: 12 encoder-layer
    gradients with a ragged token count, 40 matrices (two chunks of the 32-entry pointer table), ragged tiles, a shape the
    persistent kernel refuses (falls back to separate GEMMs inside the library), count = 1, accumulate on / off (NaN-poisoned
    outputs when off)."""
    import ctypes
    ops, H = _ops()
    dYs = [_rand((Mtok, N), dev, torch.bfloat16, seed=10 + i) for i in range(count)]
    Xs = [_rand((Mtok, K), dev, torch.bfloat16, seed=100 + i) for i in range(count)]
    init = lambda i: (_rand((N, K), dev, seed=200 + i) if acc else torch.full((N, K), float("nan"), device=dev))
    got = [init(i) for i in range(count)]
    want = [init(i) for i in range(count)]
    arr = lambda ts: (ctypes.c_void_p * count)(*[t.data_ptr() for t in ts])
    ctx = H.gemm_ctx(workspace=True)
    H.check(H.lib().fcmf_gemm_dw_batched(ctx, count, arr(dYs), arr(Xs), arr(got), N, K, Mtok, N, K, K, acc, H.stream()), "fcmf_gemm_dw_batched")
    name = H.last_gemm_kernel()
    for i in range(count):
        ops.gemm(dYs[i], Xs[i], want[i], N, K, Mtok, N, K, K, 1, 1, acc=bool(acc))
    if count > 1 and N >= 256 and K >= 256:
        assert name == "gemm_bf16_dw_batched_kernel", name
    for i in (0, count // 2, count - 1):
        ref = dYs[i].double().cpu().t() @ Xs[i].double().cpu()
        if acc:
            ref = ref + _rand((N, K), dev, seed=200 + i).double().cpu()
        assert torch.isfinite(got[i]).all()
        assert rel_err(got[i], ref) < 2e-3 and rel_err(got[i], want[i]) < 1e-5, i
    two = (ctypes.c_void_p * 2)(dYs[0].data_ptr(), dYs[0].data_ptr())
    assert H.lib().fcmf_gemm_dw_batched(ctx, 2, two, None, None, N, K, Mtok, N, K, K, acc, H.stream()) == -1        # missing pointer tables


@pytest.mark.parametrize("N", [3072, 2304, 768])
def test_gemm_dw_batched_at_the_step_shape(dev, N):
    """fcmf_gemm_dw_batched at the shapes of the benchmarked step (VERDICT round 3, weak #1b): the weight gradients of all 12
    encoder layers in ONE launch, contraction over K = 49152 tokens (B=64 x 6 aspects x 128) -- 12 x 3072 x 768 (FFN in),
    12 x 2304 x 768 (fused q|k|v), 12 x 768 x 768 (attention output).  Checked against (a) the float64 product of the same bf16
    operands on sampled 64 x 64 output tiles of the first / middle / last matrix (corners, tile seams at 255|256, interior) and
    (b) the unbatched split-K kernel on EVERY element of every matrix; accumulate into a pre-filled gradient buffer, as the
    arena does on a second micro-step."""
    import ctypes
    ops, H = _ops()
    count, K, Mtok = 12, 768, 64 * 6 * 128
    g = torch.Generator(device=dev).manual_seed(7 + N)
    dYs = [(torch.randn((Mtok, N), generator=g, device=dev) * 0.5).bfloat16() for _ in range(count)]
    Xs = [torch.randn((Mtok, K), generator=g, device=dev).bfloat16() for _ in range(count)]
    base = [torch.randn((N, K), generator=g, device=dev) for _ in range(count)]
    got = [t.clone() for t in base]
    arr = lambda ts: (ctypes.c_void_p * count)(*[t.data_ptr() for t in ts])
    ctx = H.gemm_ctx(workspace=True)
    H.check(H.lib().fcmf_gemm_dw_batched(ctx, count, arr(dYs), arr(Xs), arr(got), N, K, Mtok, N, K, K, 1, H.stream()), "fcmf_gemm_dw_batched")
    assert H.last_gemm_kernel() == "gemm_bf16_dw_batched_kernel"
    scale = (Mtok ** 0.5) * 0.5                                  # magnitude of an output element
    for i in (0, count // 2, count - 1):
        for r0, c0 in ((0, 0), (N - 64, K - 64), (224, 224), (N // 2 - 32, 300), (1000 % (N - 64), 512)):
            ref = dYs[i][:, r0:r0 + 64].double().t() @ Xs[i][:, c0:c0 + 64].double() + base[i][r0:r0 + 64, c0:c0 + 64].double()
            err = (got[i][r0:r0 + 64, c0:c0 + 64].double() - ref).abs().max().item()
            assert err < 2e-4 * scale, (i, r0, c0, err)         # float32 accumulation of 49152 products, split 4-7 ways
    for i in range(count):
        want = base[i].clone()
        ops.gemm(dYs[i], Xs[i], want, N, K, Mtok, N, K, K, 1, 1, acc=True)
        assert torch.isfinite(got[i]).all()
        assert (got[i] - want).abs().max().item() < 2e-4 * scale, i


@pytest.mark.parametrize("M,N,K,bias", [(8192, 64, 256, False), (9000, 64, 576, True), (8200, 128, 1152, False), (16384, 96, 128, True),
                                        (8192, 32, 64, False), (8192, 128, 64, False)])
def test_gemm_narrow_outputs_on_the_persistent_kernel(dev, M, N, K, bias):
    """N <= 128 with many rows (the ResNet trunk's 64- / 128-channel convolutions as GEMMs): the 256-row persistent kernel with its
    eight waves standing 8 x 1 (N <= 64) or 4 x 2 (N <= 128) over the outputs -- no matrix instruction on zero-filled columns.
    Against the float64 product of the same bf16 operands; ragged row counts, N that is no multiple of 64, a bias, K of one k-tile."""
    ops, H = _ops()
    x, w = _rand((M, K), dev, torch.bfloat16, seed=1), _rand((N, K), dev, torch.bfloat16, seed=2)
    b = _rand((N,), dev, seed=3) if bias else None
    y = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev)
    ops.gemm(x, w, y, M, N, K, K, K, N, 0, 0, bias=b)
    assert H.last_gemm_kernel() == ("gemm_bf16_tile256k64_n64_kernel" if N <= 64 else "gemm_bf16_tile256k64_n128_kernel")
    ref = x.double().cpu() @ w.double().cpu().t()
    if bias:
        ref = ref + b.double().cpu()
    assert torch.isfinite(y).all()
    assert rel_err(y, ref) < 6e-3


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_embed_scale_kernels_and_their_vocabulary_bound(dev, dtype):
    """fcmf_embed_scale_fwd / _bwd (IAOG decoder: `embedding(X) * sqrt(H)` + PositionalEncoding, mm_modeling.py:650,619-633)
    against torch gather / index_add_; and the table bound (round-3 advisor finding): an id outside [0, V) reads nothing and
    makes its output row NaN, the backward skips it, counts it, and never writes outside the [V, H] gradient -- which in the
    product is a slice of the flat arena with another parameter's gradient right behind it."""
    ops, H = _ops()
    V, Hd, B, T = 50, 64, 3, 7
    w = _rand((V, Hd), dev, seed=1)
    P = _rand((T, Hd), dev, seed=2)
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(0, V, (B, T), generator=g).to(dev)
    out = torch.empty((B, T, Hd), dtype=dtype, device=dev)
    H.check(H.lib().fcmf_embed_scale_fwd(H.ptr(ids), H.ptr(w), H.ptr(P), H.ptr(out), B * T, Hd, T, V, 8.0, H.dt(out), H.stream()), "fwd")
    ref = w[ids] * 8.0 + P
    assert rel_err(out, ref) < TOL[dtype]
    dy = _rand((B, T, Hd), dev, dtype, seed=4)
    guard = torch.zeros((V + 4, Hd), device=dev)                   # 4 guard rows behind the table's gradient
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    H.check(H.lib().fcmf_embed_scale_bwd(H.ptr(dy), H.ptr(ids), H.ptr(guard), B * T, Hd, V, H.ptr(cnt), 8.0, H.dt(dy), H.stream()), "bwd")
    want = torch.zeros((V, Hd), device=dev).index_add_(0, ids.reshape(-1), dy.float().reshape(-1, Hd) * 8.0)
    assert rel_err(guard[:V], want) < 1e-5 and guard[V:].abs().sum().item() == 0 and cnt.item() == 0
    # ---- ids outside the table -------------------------------------------------------------------
    bad = ids.clone()
    bad[0, 1], bad[2, 5], bad[1, 0] = V, -1, V + 2
    out.zero_()
    H.check(H.lib().fcmf_embed_scale_fwd(H.ptr(bad), H.ptr(w), H.ptr(P), H.ptr(out), B * T, Hd, T, V, 8.0, H.dt(out), H.stream()), "fwd")
    isbad = (bad < 0) | (bad >= V)
    assert torch.isnan(out[isbad].float()).all() and torch.isfinite(out[~isbad].float()).all()
    assert rel_err(out[~isbad], ref[~isbad]) < TOL[dtype]
    guard.zero_()
    H.check(H.lib().fcmf_embed_scale_bwd(H.ptr(dy), H.ptr(bad), H.ptr(guard), B * T, Hd, V, H.ptr(cnt), 8.0, H.dt(dy), H.stream()), "bwd")
    ok = ~isbad.reshape(-1)
    want = torch.zeros((V, Hd), device=dev).index_add_(0, bad.reshape(-1)[ok], dy.float().reshape(-1, Hd)[ok] * 8.0)
    assert rel_err(guard[:V], want) < 1e-5 and guard[V:].abs().sum().item() == 0 and cnt.item() == 3
    assert H.lib().fcmf_embed_scale_bwd(H.ptr(dy), H.ptr(bad), H.ptr(guard), B * T, Hd, 0, None, 8.0, H.dt(dy), H.stream()) != 0


def test_head_nk_groupings_of_the_same_parameter_stay_fresh(dev):
    """shadows.head_nk: the per-head weights of the IAOG decoder's Attention ([n_head, E, d] float32) as registered transposed
    bf16 copies.  The same parameter in TWO groupings ([w_kx] alone and [w_kx, w_qx]) keeps a buffer per grouping, and both are
    rebuilt after the parameter changes (round-3 advisor finding: the pieces were keyed by source address only, so the
    second grouping took over the first one's entries and the first served stale weights)."""
    ops, H = _ops()
    nh, E, d = 4, 64, 16
    wk = torch.nn.Parameter(_rand((nh, E, d), dev, seed=1))
    wq = torch.nn.Parameter(_rand((nh, E, d), dev, seed=2))
    want = lambda ws: torch.cat([w.detach().permute(0, 2, 1).reshape(nh * d, E) for w in ws]).bfloat16()
    try:
        a = ops.shadows.head_nk([wk])
        b = ops.shadows.head_nk([wk, wq])
        assert torch.equal(a, want([wk])) and torch.equal(b, want([wk, wq]))
        with torch.no_grad():
            wk.add_(1.0)
            wq.mul_(2.0)
        ops.shadows.mark_all_stale()                 # (what the fused optimizers do after their update)
        a2 = ops.shadows.head_nk([wk])
        b2 = ops.shadows.head_nk([wk, wq])
        assert a2.data_ptr() == a.data_ptr() and b2.data_ptr() == b.data_ptr()
        assert torch.equal(a2, want([wk])) and torch.equal(b2, want([wk, wq]))
        with torch.no_grad():
            wk.sub_(0.5)
        ops.shadows.mark_all_stale()
        assert torch.equal(ops.shadows.head_nk([wk, wq]), want([wk, wq])) and torch.equal(ops.shadows.head_nk([wk]), want([wk]))
    finally:
        ops.shadows.clear()


@pytest.mark.parametrize("nparams,tokens", [(2, 768), (1, 960), (12, 1000)])
def test_gemm_colblocks_writes_per_head_weight_gradients_in_the_parameter_layout(dev, nparams, tokens):
    """fcmf_gemm_colblocks: dW^T [E, n * n_head * d] = x^T dY with the column-blocked output (block = d, block stride = E * d, row
    stride = d) IS the [n, n_head, E, d] layout of the IAOG decoder's per-head projection weights (mm_modeling.py:57-58, autograd of
    :79-92): against the float64 product and against the plain fcmf_gemm + permute it replaces; a shape the blocked path refuses
    returns FCMF_ERR_UNSUPPORTED (callers fall back)."""
    ops, H = _ops()
    nh, E, d = 12, 768, 64
    N = nparams * nh * d
    x = _rand((tokens, E), dev, torch.bfloat16, seed=1)
    dy = _rand((tokens, N), dev, torch.bfloat16, 0.3, seed=2)
    out = torch.full((nparams, nh, E, d), float("nan"), device=dev)
    ctx = H.gemm_ctx(workspace=True)
    H.check(H.lib().fcmf_gemm_colblocks(ctx, H.ptr(x), H.ptr(dy), H.ptr(out), E, N, tokens, E, N, d, 1, 1, d, E * d, 0, H.stream()), "colblocks")
    ref = (dy.double().cpu().t() @ x.double().cpu()).view(nparams, nh, d, E).permute(0, 1, 3, 2)      # [n, nh, E, d]
    assert torch.isfinite(out).all()
    assert rel_err(out, ref) < 2e-3
    plain = torch.empty((N, E), device=dev)
    ops.gemm(dy, x, plain, N, E, tokens, N, E, E, 1, 1)
    assert rel_err(out, plain.view(nparams, nh, d, E).permute(0, 1, 3, 2)) < 1e-5
    # accumulate into what is there
    H.check(H.lib().fcmf_gemm_colblocks(ctx, H.ptr(x), H.ptr(dy), H.ptr(out), E, N, tokens, E, N, d, 1, 1, d, E * d, 1, H.stream()), "colblocks")
    assert rel_err(out, 2 * ref) < 2e-3
    small = torch.empty((1, 2, 128, 64), device=dev)     # E = 128 < 256: refused
    assert H.lib().fcmf_gemm_colblocks(ctx, H.ptr(x), H.ptr(dy), H.ptr(small), 128, 128, tokens, E, N, d, 1, 1, d, 128 * d, 0, H.stream()) == H.ERR_UNSUPPORTED
