"""log-softmax + top-k (csrc/topk.hip, fcmf_logsoftmax_topk / ops.logsoftmax_topk) against float64 on the CPU, computed on the
SAME stored values (the bf16 tensor upcast to float64): log_softmax for the values, torch.sort(descending, stable) truncated to k for
the ids.  ids must be equal exactly -- the selection is made on stored values, so it carries no rounding, and ties go to the lower
column -- and logp within 1e-4 absolute: the float32 accumulation bound is (251 terms per thread + 8 merge levels) * 2^-24 = 1.5e-5
relative on a sum whose logarithm is taken, with the margin test_bertscore_gpu.py takes over its bound.
Layouts: ld = V; ld = V rounded up to 32 with NaN in the padding (nothing beyond V may reach a result); float32 also ld = V + 1 with
the base 4 bytes off a 16-byte boundary (rows unaligned: the one-element path).  Every comparison prints its figure before it asserts."""
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-4
VS = [1, 2, 63, 64, 65, 255, 257, 1000, 4099, 64001]
KS = [1, 2, 3, 5, 8, 16]
KINDS = [("f32", torch.float32, 3.0), ("bf16", torch.bfloat16, 3.0), ("bf16-ties", torch.bfloat16, 0.05)]


def place(x, ld, dev, offset=0):
    """the rows of x [rows, V] at row stride ld in a NaN-filled device buffer, `offset` elements from its start"""
    rows, V = x.shape
    buf = torch.full((offset + rows * ld,), float("nan"), dtype=x.dtype)
    torch.as_strided(buf, (rows, V), (ld, 1), offset).copy_(x)
    buf = buf.to(dev)
    return buf, torch.as_strided(buf, (rows, V), (ld, 1), offset)


def reference(x):
    """(float64 log_softmax sorted descending and stable [rows, V], the sort's indices)"""
    xd = x.double()
    order = torch.sort(xd, dim=1, descending=True, stable=True).indices
    return torch.log_softmax(xd, dim=1).gather(1, order), order


def launch(view, ld, V, k, dtype_code=None):
    from fcmf_framework import _hip as H
    rows = view.shape[0]
    logp = torch.full((rows, k), float("nan"), dtype=torch.float32, device=view.device)
    ids = torch.full((rows, k), -1, dtype=torch.int32, device=view.device)
    rc = H.lib().fcmf_logsoftmax_topk(view.data_ptr(), ld, rows, V, k, logp.data_ptr(), ids.data_ptr(),
                                      H.dt(view) if dtype_code is None else dtype_code, H.stream())
    torch.cuda.synchronize()
    return rc, logp.cpu(), ids.cpu()


def check(view, ld, V, k, ref, what):
    rc, logp, ids = launch(view, ld, V, k)
    assert rc == 0, (what, rc)
    rl, ro = ref
    assert torch.equal(ids.long(), ro[:, :k]), (what, "ids")
    want = rl[:, :k]
    inf = torch.isinf(want)
    assert torch.equal(torch.isinf(logp) & (logp < 0), inf), (what, "-inf entries")
    err = (logp.double() - want).masked_fill(inf, 0.0).abs().max().item()
    assert err < TOL, (what, err)
    return err


@pytest.mark.parametrize("V", VS)
def test_topk_grid(dev, V):
    worst = 0.0
    for rows in ((3,) if V == 64001 else (1, 3, 70)):
        for name, dtype, scale in KINDS:
            g = torch.Generator().manual_seed(1000 * rows + V)
            x = (torch.randn(rows, V, generator=g) * scale).to(dtype)
            ref = reference(x)
            layouts = [("ld=V", V, 0), ("ld=pad32", (V + 31) // 32 * 32, 0)]
            if dtype == torch.float32:
                layouts.append(("ld=V+1, base+4B", V + 1, 1))
            for lname, ld, off in layouts:
                _, view = place(x, ld, dev, off)
                for k in KS:
                    if k <= V:
                        worst = max(worst, check(view, ld, V, k, ref, (V, rows, name, lname, k)))
    print(f"V {V}: max |logp - float64| {worst:.3e} (bound {TOL})")


def test_topk_fill_value_rows(dev):
    """+-1e4, the reference's mask fill value: without the row maximum subtracted exp overflows.  More +1e4 entries than k, so
    every result is -log(count) and float32 can hold it to the bound"""
    V = 1000
    for dtype in (torch.float32, torch.bfloat16):
        x = torch.full((3, V), -1e4)
        x[:, 5::7] = 1e4
        x = x.to(dtype)
        _, view = place(x, V, dev)
        err = check(view, V, V, 5, reference(x), ("fill", dtype))
        print(f"+-1e4 rows {dtype}: {err:.3e}")


def test_topk_minus_inf_and_constant_rows(dev):
    V = 300
    x = torch.full((2, V), float("-inf"))
    x[0, 17], x[0, 250] = 0.5, 1.5
    x[1, 0], x[1, 299] = -2.0, -2.0
    _, view = place(x, V, dev)
    rc, logp, ids = launch(view, V, V, 3)
    assert rc == 0
    assert ids.tolist() == [[250, 17, 0], [0, 299, 1]]          # the third result: -inf at the lowest -inf column
    assert torch.isinf(logp[:, 2]).all() and (logp[:, 2] < 0).all()
    check(view, V, V, 3, reference(x), "-inf")
    for dtype in (torch.float32, torch.bfloat16):
        c = torch.full((1, 4099), 0.375).to(dtype)
        _, view = place(c, 4099, dev)
        for k in (1, 5, 16):
            rc, logp, ids = launch(view, 4099, 4099, k)
            assert rc == 0 and ids[0].tolist() == list(range(k))
            check(view, 4099, 4099, k, reference(c), ("constant", dtype, k))


def test_topk_deterministic_and_limits(dev):
    from fcmf_framework import _hip as H
    V = 4099
    x = (torch.randn(5, V, generator=torch.Generator().manual_seed(3)) * 3).to(torch.bfloat16)
    _, view = place(x, 4128, dev)
    a, b = launch(view, 4128, V, 8), launch(view, 4128, V, 8)
    assert a[0] == 0 and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)) and torch.equal(a[2], b[2])
    assert launch(view, 4128, V, 17)[0] == H.ERR_UNSUPPORTED
    assert launch(view[:, :4], 4128, 4, 5)[0] == H.ERR_UNSUPPORTED          # k > V
    assert launch(view, 4128, V, 3, dtype_code=H.F64)[0] == H.ERR_UNSUPPORTED
    out = torch.full((3,), 7.0, device=dev), torch.full((3,), 7, dtype=torch.int32, device=dev)
    rc = H.lib().fcmf_logsoftmax_topk(view.data_ptr(), 4128, 0, V, 3, out[0].data_ptr(), out[1].data_ptr(), H.BF16, H.stream())
    torch.cuda.synchronize()
    assert rc == 0 and out[0].tolist() == [7.0] * 3 and out[1].tolist() == [7] * 3      # rows = 0: nothing to do, nothing written


def test_ops_logsoftmax_topk_reads_strided_rows(dev):
    """the wrapper hands the row stride of a column-padded buffer through"""
    from fcmf_framework import ops
    x = (torch.randn(6, 1000, generator=torch.Generator().manual_seed(4)) * 3)
    _, view = place(x, 1024, dev)
    buf2d = torch.as_strided(view, (6, 1024), (1024, 1))
    logp, ids = ops.logsoftmax_topk(buf2d, 1000, 3)
    rl, ro = reference(x)
    assert torch.equal(ids.cpu().long(), ro[:, :3])
    assert (logp.cpu().double() - rl[:, :3]).abs().max().item() < TOL


def test_ops_logsoftmax_topk_refuses_overlapping_rows(dev):
    from fcmf_framework import _hip as H, ops
    x = torch.randn(1, 40, device=dev)
    with pytest.raises(H.HipLibraryError, match="overlap"):
        ops.logsoftmax_topk(x.expand(3, 40), 40, 2)
    logp, ids = ops.logsoftmax_topk(x.expand(1, 40), 40, 2)          # one row: whatever its stride says
    assert ids[0].tolist() == torch.topk(x[0], 2).indices.tolist()
