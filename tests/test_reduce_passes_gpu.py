"""The two column-sum passes that share colsum_block (csrc/common.h): fcmf_colsum (csrc/gemm.hip) and the reduce pass behind
fcmf_add_ln_bwd's workspace (csrc/norm.hip), through the C ABI.

Column sums: against the float64 sum of the values as stored, per column within 1e-5 * sum_rows |x| (the bound of
test_norm_gpu.py), bf16 and float32, accumulate = 0 and 1 into a pre-filled, guard-banded destination.  The shapes are the
edges of the kernel's geometry: a workgroup of 16 waves sums `rpb` rows of a 256-column block, rpb = ceil(M * column blocks /
256) rounded up to 16 rows (32 for bf16 rows read 16 bytes per lane, two rows per wave instruction) and capped at 2048; a wave
keeps 8 row groups in flight, so a workgroup's full batch is 128 rows (256 for wide bf16).  With N = 8 (one column block):
    M = 4095 / 4097        rpb 16 -> 32 (float32, narrow bf16)          M = 8191 / 8193       rpb 32 -> 64 (wide bf16)
    M = 32767 / 32769      rpb 128 = one full batch -> 144 (float32)    M = 65535 / 65537     rpb 256 -> 288 (wide bf16)
    M = 524287 / 524289    rpb reaches the cap of 2048: 256 -> 257 row blocks
and each of them is also one row short of / one row past a whole number of row blocks.  Lane layouts: N = 4, 260, 772 take the
8-byte bf16 layout (ldx % 8 = 4), 768 / 520 / 2304 / 8 the 16-byte one, the pointer offset by 2 elements the scalar path.
M = 0 adds nothing: with accumulate = 1 the destination is untouched, with accumulate = 0 it is the sum of no rows, zero (the
memset comes before the row count is looked at, as it always did).

LayerNorm backward: helpers, reference and bounds of test_norm_gpu.py (NaN-filled workspace of exactly
fcmf_add_ln_bwd_workspace floats, pre-filled dgamma / dbeta / dxsum, column sums within 1e-5 * sum_rows |term|) at
rows = 4 cap - 1, 4 cap, 4 cap + 5 and 5, where cap is the workgroup cap of the backward (read off the workspace size of a
million rows), for H = 4, 768, 1028, 2048; dxsum present, and NULL at rows = 5 and 4 cap + 5.
"""
import pytest
import torch

import rowwise_ref as R
import test_norm_gpu as TN

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16


def _lib():
    from fcmf_framework import _hip as H
    return H.lib(), H


def _colsum_case(dev, dtype, accumulate, M, N, ld=None, offset=0, seed=1):
    """one fcmf_colsum call on the [M, N] block (row stride ld) that starts `offset` elements into a 16-byte-aligned buffer"""
    L, H = _lib()
    ld = N if ld is None else ld
    g = torch.Generator().manual_seed(seed + M + N)
    buf = torch.randn(offset + max(M, 1) * ld, generator=g).to(dtype).to(dev)
    x = buf[offset:offset + M * ld].view(M, ld)[:, :N]
    assert buf.data_ptr() % 16 == 0
    pre = torch.randn(N, generator=g)
    out = R.guarded((N,), F32, dev)
    out.view.copy_(pre)
    rc = L.fcmf_colsum(x.data_ptr() if M else buf.data_ptr(), H.ptr(out.view), M, N, ld, H.dt(buf), accumulate, H.stream())
    assert rc == 0
    torch.cuda.synchronize()
    out.check()
    got = out.view.cpu()
    if M == 0:
        assert torch.equal(got, pre if accumulate else torch.zeros(N))
        return
    x64 = x.double().cpu()
    ref = x64.sum(0) + (pre.double() if accumulate else 0.0)
    bound = 1e-5 * x64.abs().sum(0)
    assert torch.isfinite(got).all()
    ratio = ((got.double() - ref).abs() / bound).max().item()
    print(f"colsum {str(dtype)[6:]:8s} M={M} N={N} ld={ld} off={offset} acc={accumulate}: worst err/bound {ratio:.3f}")
    assert ratio <= 1.0


SHAPES = [
    dict(M=1, N=4), dict(M=3, N=260), dict(M=17, N=772, offset=2), dict(M=4099, N=768, ld=2304), dict(M=4099, N=520),
    dict(M=384, N=2304), dict(M=0, N=260),
] + [dict(M=m, N=8) for m in (4095, 4097, 8191, 8193, 32767, 32769, 65535, 65537, 524287, 524289)]


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s.values()))
def test_colsum(dev, shape, dtype, accumulate):
    _colsum_case(dev, dtype, accumulate, **shape)


def test_colsum_column_block_of_a_wider_buffer_reads_only_its_columns(dev):
    """the [4099, 768] middle block of a [4099, 2304] buffer whose other columns are NaN"""
    L, H = _lib()
    for dtype in (F32, BF16):
        big = torch.full((4099, 2304), float("nan"), dtype=dtype, device=dev)
        x = TN._randn((4099, 768), 31, dtype)
        big[:, 768:1536] = x.to(dev)
        out = R.guarded((768,), F32, dev)
        assert L.fcmf_colsum(big[:, 768:].data_ptr(), H.ptr(out.view), 4099, 768, 2304, H.dt(big), 0, H.stream()) == 0
        torch.cuda.synchronize()
        out.check()
        err = (out.view.cpu().double() - x.double().sum(0)).abs() / (1e-5 * x.double().abs().sum(0))
        assert err.max().item() <= 1.0


def _cap():
    L, _ = _lib()
    return L.fcmf_add_ln_bwd_workspace(1000000, 4) // 12


@pytest.mark.parametrize("H_", [4, 768, 1028, 2048])
@pytest.mark.parametrize("which", ["4cap-1", "4cap", "4cap+5", "5"])
def test_ln_bwd_reduce_pass(dev, which, H_):
    L, _ = _lib()
    cap = _cap()
    rows = {"4cap-1": 4 * cap - 1, "4cap": 4 * cap, "4cap+5": 4 * cap + 5, "5": 5}[which]
    assert L.fcmf_add_ln_bwd_workspace(rows, H_) >= min((rows + 3) // 4, cap) * 3 * H_
    z, dy = TN._randn((rows, H_), 41), TN._randn((rows, H_), 42)
    gamma, _ = TN._params(H_)
    TN._check_bwd(TN._bwd(dev, dy, z, gamma, 1e-12, prefill=True), F32)
    if which in ("5", "4cap+5"):
        TN._check_bwd(TN._bwd(dev, dy, z, gamma, 1e-12, prefill=True, want_dxsum=False), F32, dxsum=False)


@pytest.mark.parametrize("which", ["4cap-1", "4cap+5"])
def test_ln_bwd_reduce_pass_bf16(dev, which):
    cap = _cap()
    rows, H_ = (4 * cap - 1 if which == "4cap-1" else 4 * cap + 5), 768
    z, dy = TN._randn((rows, H_), 43, BF16), TN._randn((rows, H_), 44, BF16)
    gamma, _ = TN._params(H_)
    TN._check_bwd(TN._bwd(dev, dy, z, gamma, 1e-12, prefill=True), BF16)
