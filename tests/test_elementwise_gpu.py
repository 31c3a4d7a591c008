"""The streaming kernels of csrc/misc.hip through the C ABI, each against a plain restatement: fcmf_dropout (the numpy mask of
rowwise_ref.py, bit for bit), fcmf_cast (round to nearest even, tails, unaligned views), fcmf_cast_transpose and its multi-tensor
form (ragged 64 x 64 tiles, 8-byte and scalar stores), fcmf_act_bwd, fcmf_sum_axis and fcmf_head_gather -- at n & 3 tails, one
element, and sizes beyond the 4096-block cap of the grid.  Every output lies in a sentinel frame (rowwise_ref.guarded)."""
import pytest
import torch

import rowwise_ref as R

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]


def _lib():
    from fcmf_framework import _hip as H
    return H.lib(), H


def _randn(shape, seed, dtype=F32, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dtype)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def _within(got, ref, dtype, f32_bound):
    """|got - ref| <= f32_bound (a tensor or a number), plus one bf16 rounding (unit roundoff 2^-8) for bf16 outputs"""
    got, ref = got.double().cpu(), ref.double()
    bound = f32_bound + (2.0 ** -8 * ref.abs() if dtype == BF16 else 0.0)
    assert torch.isfinite(got).all()
    bad = (got - ref).abs() > bound
    assert not bad.any(), f"{int(bad.sum())} elements off, worst {((got - ref).abs() - bound).max().item():.3e} over the bound"


# ---- dropout ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("seed", [R.SEED_LO, R.SEED_HI])
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("n", [1, 255, 257, 1048576 + 7])
def test_dropout_matches_the_numpy_mask_bitwise(dev, dtype, n, p, seed):
    """y = x * m * float32(1 / (1 - p)): one float32 multiply, rounded once more for bf16.  1048576 + 7: the grid is capped at
    4096 blocks of 256, so the last 7 elements are a second trip of the grid-stride loop."""
    L, H = _lib()
    x = _randn((n,), 21, dtype)
    xd = x.to(dev)
    y = R.guarded((n,), dtype, dev)
    assert L.fcmf_dropout(H.ptr(xd), H.ptr(y.view), n, p, seed, H.dt(xd), H.stream()) == 0
    torch.cuda.synchronize()
    y.check()
    mult = R.mask_tensor(seed, (n,), p).float() * R.inv_keep(p)
    ref = (x.float() * mult).to(dtype)
    assert torch.equal(_bits(y.view.cpu()), _bits(ref))
    if p == 0.0:
        assert torch.equal(_bits(y.view.cpu()), _bits(x))


def test_dropout_refuses_p_outside_0_1(dev):
    L, H = _lib()
    x = torch.ones(16, device=dev)
    y = R.guarded((16,), F32, dev)
    for p in (1.0, -0.1, 1.5):
        assert L.fcmf_dropout(H.ptr(x), H.ptr(y.view), 16, p, 1, H.F32, H.stream()) == -1
    assert L.fcmf_dropout(H.ptr(x), H.ptr(y.view), -1, 0.1, 1, H.F32, H.stream()) == -1
    torch.cuda.synchronize()
    y.check()
    assert bool((y.view == 12345.0).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_dropout_backward_applies_the_same_mask(dev, dtype):
    from fcmf_framework import ops
    n, p, seed = 1027, 0.1, R.SEED_HI
    x = _randn((n,), 22, dtype).to(dev).requires_grad_(True)
    dy = _randn((n,), 23, dtype)
    y = ops.DropoutFn.apply(x, p, seed)
    y.backward(dy.to(dev))
    mult = R.mask_tensor(seed, (n,), p).float() * R.inv_keep(p)
    assert torch.equal(_bits(y.detach().cpu()), _bits((x.detach().cpu().float() * mult).to(dtype)))
    assert torch.equal(_bits(x.grad.cpu()), _bits((dy.float() * mult).to(dtype)))


# ---- cast -------------------------------------------------------------------------------------------------------------------
def _specials():
    """float32 values whose bf16 rounding is decided by the rule: exact ties (to even, both ways), signed zeros, infinities, NaN,
    denormals, and the largest finite values (3.3895e38 rounds to inf)"""
    return torch.tensor([1.00390625, 1.01171875, -1.00390625, -1.01171875, 0.0, -0.0, float("inf"), float("-inf"), float("nan"),
                         1e-40, -1e-40, 1.4e-45, 9.1835e-41, 3.3895e38, -3.3895e38, 3.3893e38, 1.0 + 2.0 ** -8 + 2.0 ** -20,
                         1.0 + 2.0 ** -8 - 2.0 ** -20], dtype=F32)


def _cast_source(n, src):
    x = _randn((n,), 24, src, scale=3.0)
    if src == F32:
        s = _specials()
        k = min(n, s.numel())
        x[:k] = s[:k]
        if n > 2 * s.numel():
            x[-s.numel():] = s.flip(0)           # the n & 3 tail sees them too
    return x


def _assert_cast(got, x, dst):
    ref = x.to(dst)
    nan = torch.isnan(ref.float())
    assert torch.equal(torch.isnan(got.float()), nan)                      # NaN stays NaN (the payload is not compared)
    assert torch.equal(_bits(got)[~nan], _bits(ref)[~nan])


@pytest.mark.parametrize("src,dst", [(F32, BF16), (BF16, F32), (F32, F32), (BF16, BF16)])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 1027, 4194304 + 1024 + 3])
def test_cast_all_pairs_tails_and_grid_stride(dev, src, dst, n):
    """float32 -> bf16 is torch's round to nearest even bit for bit; bf16 -> float32 is exact.  4194304 + 1027 elements: past
    the 4096 x 1024 elements of one grid trip, with an n & 3 tail of 3"""
    L, H = _lib()
    x = _cast_source(n, src)
    xd = x.to(dev)
    y = R.guarded((n,), dst, dev)
    assert L.fcmf_cast(H.ptr(xd), H.ptr(y.view), n, H.dt(xd), H.dt(y.view), H.stream()) == 0
    torch.cuda.synchronize()
    y.check()
    _assert_cast(y.view.cpu(), x, dst)


@pytest.mark.parametrize("src,dst", [(F32, BF16), (BF16, F32)])
@pytest.mark.parametrize("n", [5, 1027])
def test_cast_of_views_at_odd_element_offsets(dev, src, dst, n):
    """a contiguous view that starts 1..7 elements into a buffer (a slice of a packed buffer, a dy view) is not 16-byte aligned:
    fcmf_cast takes it one element per lane instead of refusing it"""
    from fcmf_framework import ops
    L, H = _lib()
    base = _cast_source(n + 8, src)
    bd = base.to(dev)
    for off in range(1, 8):
        _assert_cast(ops.cast(bd[off:off + n], dst).cpu(), base[off:off + n], dst)
    # an unaligned destination, straight through the ABI: the neighbours of the destination range stay as they were
    y = R.guarded((n + 2,), dst, dev)
    assert L.fcmf_cast(H.ptr(bd), H.ptr(y.view[1:]), n, H.dt(bd), H.dt(y.view), H.stream()) == 0
    torch.cuda.synchronize()
    y.check()
    out = y.view.cpu()
    assert out[0].item() == out[-1].item() and out[0].item() in (12345.0, 12352.0)
    _assert_cast(out[1:-1], base[:n], dst)
    # a pointer that is not even aligned to its element is a caller's mistake
    assert L.fcmf_cast(H.ptr(bd) + 1, H.ptr(y.view), n, H.dt(bd), H.dt(y.view), H.stream()) == -1


# ---- cast + transpose -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Rr,C", [(1, 1), (3, 5), (4, 4), (64, 64), (65, 63), (66, 4), (130, 68), (100, 200), (200, 100)])
def test_cast_transpose_ragged_tiles_both_store_paths(dev, Rr, C):
    """R % 4 == 0 takes the 8-byte store path, anything else the scalar one; both with ragged tiles in both dimensions"""
    L, H = _lib()
    src = _randn((Rr, C), 25)
    sd = src.to(dev)
    dst = R.guarded((C, Rr), BF16, dev)
    assert L.fcmf_cast_transpose(H.ptr(sd), H.ptr(dst.view), Rr, C, H.stream()) == 0
    torch.cuda.synchronize()
    dst.check()
    assert torch.equal(_bits(dst.view.cpu()), _bits(src.t().contiguous().bfloat16()))


def test_multi_tensor_cast_transpose_after_an_optimizer_step(dev):
    """shadows.get_t + FusedAdamW.step: the transposed copies of all weights are rebuilt by one fcmf_multi_cast_transpose launch
    (ragged tiles; a one-row weight)"""
    from fcmf_framework import ops
    from fcmf_framework.optimization import FusedAdamW
    ops.shadows.clear()
    try:
        ws = [torch.nn.Parameter(_randn(s, 26 + i).to(dev)) for i, s in enumerate([(70, 33), (33, 70), (1, 130)])]
        for w in ws:
            assert torch.equal(_bits(ops.shadows.get_t(w)), _bits(w.detach().t().contiguous().bfloat16()))
        opt = FusedAdamW(ws, lr=1e-2)
        for i, w in enumerate(ws):
            w.grad = _randn(w.shape, 30 + i).to(dev)
        before = [w.detach().clone() for w in ws]
        opt.step()
        for w, b in zip(ws, before):
            ent = ops.shadows.lookup("t", w)
            assert ent.stale is False and ent.version == w._version
            assert not torch.equal(w.detach(), b)
            assert torch.equal(_bits(ent.payload), _bits(w.detach().t().contiguous().bfloat16()))
    finally:
        ops.shadows.clear()


# ---- activation backward ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("n", [1, 257, 1048576 + 5])
def test_act_bwd_tanh_and_gelu(dev, dtype, kind, n):
    """kind 0: dy * (1 - a^2) with a = tanh output in (-1, 1); kind 1: dy * gelu'(a), exact erf, a over [-10, 10] (both tails)"""
    L, H = _lib()
    dy = _randn((n,), 31, dtype)
    if kind == 0:
        aux = torch.tanh(_randn((n,), 32, scale=2.0)).to(dtype)
        deriv = R.tanh_grad_from_output(aux)
    else:
        aux = torch.rand((n,), generator=torch.Generator().manual_seed(33)) * 20.0 - 10.0
        if n > 1:
            aux[0], aux[-1] = -10.0, 10.0
        else:
            aux[0] = 0.75                          # (a single element cannot span the range)
        aux = aux.to(dtype)
        deriv = R.gelu_grad(aux)
    ref = dy.double() * deriv
    dyd, ad = dy.to(dev), aux.to(dev)
    out = R.guarded((n,), dtype, dev)
    assert L.fcmf_act_bwd(H.ptr(dyd), H.ptr(ad), H.ptr(out.view), n, kind, H.dt(dyd), H.stream()) == 0
    torch.cuda.synchronize()
    out.check()
    _within(out.view, ref, dtype, 1e-5 * ref.abs().max().item())


def test_act_bwd_refuses_an_unknown_kind(dev):
    L, H = _lib()
    x = torch.ones(8, device=dev)
    out = R.guarded((8,), F32, dev)
    assert L.fcmf_act_bwd(H.ptr(x), H.ptr(x), H.ptr(out.view), 8, 2, H.F32, H.stream()) == -1
    torch.cuda.synchronize()
    assert bool((out.view == 12345.0).all())


# ---- sum over a middle axis -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("outer,reps,inner", [(1, 2, 5), (3, 6, 7), (1, 16, 1028), (1, 2, 1048581)])
def test_sum_axis(dev, dtype, outer, reps, inner):
    """out[o, c] = sum_r in[o, r, c], float32 accumulation in order: error <= reps * 2^-23 * sum |terms|"""
    L, H = _lib()
    x = _randn((outer, reps, inner), 34, dtype)
    xd = x.to(dev)
    out = R.guarded((outer, inner), dtype, dev)
    assert L.fcmf_sum_axis(H.ptr(xd), H.ptr(out.view), outer, reps, inner, H.dt(xd), H.stream()) == 0
    torch.cuda.synchronize()
    out.check()
    _within(out.view, x.double().sum(1), dtype, reps * 2.0 ** -23 * x.double().abs().sum(1))


# ---- decoder head gather ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [4, 64])
@pytest.mark.parametrize("extra", [0, 8])
def test_head_gather(dev, dtype, d, extra):
    """out[g, t, h] = sum of the slots s with (s * G + g) % heads == h; heads that no slot reads (heads 4, G 2: heads 1 and 3
    of g = 0) come out zero; with ldo > heads * d the pad columns are left alone"""
    L, H = _lib()
    T = 3
    unread = 0
    for G in (1, 2, 3, 4, 5):
        for heads in (2, 3, 4, 8):
            ldo = heads * d + extra
            slot = _randn((G, T, heads, d), 35 + G, dtype)
            sd = slot.to(dev)
            out = R.guarded((G, T, ldo), dtype, dev)
            assert L.fcmf_head_gather(H.ptr(sd), H.ptr(out.view), ldo, G, T, heads, d, H.dt(sd), H.stream()) == 0
            torch.cuda.synchronize()
            out.check()
            got = out.view.cpu()
            assert bool((got[:, :, heads * d:] == got.new_tensor(12345.0 if dtype == F32 else 12352.0)).all())
            ref = R.head_gather(slot, G, T, heads, d)
            absum = R.head_gather(slot.abs(), G, T, heads, d)
            got = got[:, :, :heads * d].reshape(G, T, heads, d)
            _within(got, ref, dtype, heads * 2.0 ** -23 * absum)
            for g in range(G):
                for h in set(range(heads)) - {(s * G + g) % heads for s in range(heads)}:
                    unread += 1
                    assert bool((got[g, :, h] == 0).all())
    assert unread > 0


def test_head_gather_refusals(dev):
    L, H = _lib()
    x = torch.ones(2 * 3 * 4 * 8, device=dev)
    out = R.guarded((2 * 3 * 4 * 8,), F32, dev)
    st = H.stream()
    assert L.fcmf_head_gather(H.ptr(x), H.ptr(out.view), 24, 2, 3, 4, 6, H.F32, st) == -1      # d % 4
    assert L.fcmf_head_gather(H.ptr(x), H.ptr(out.view), 31, 2, 3, 4, 8, H.F32, st) == -1      # ldo < heads * d
    assert L.fcmf_head_gather(H.ptr(x), H.ptr(out.view), 32, 0, 3, 4, 8, H.F32, st) == 0       # no batch elements: nothing written
    torch.cuda.synchronize()
    out.check()
    assert bool((out.view == 12345.0).all())
