"""BERTScore greedy matching (csrc/bertscore.hip, fcmf_bertscore / ops.bertscore) against a float64 numpy restatement of the
definition in include/fcmf_hip.h, computed on the SAME stored values (the bf16 tensor upcast to float64):
    s[i][j] = <c_i, r_j> / (|c_i| |r_j|)  over valid rows;  P = sum wc[i] max_j s / sum wc;  R = sum wr[j] max_i s / sum wr;  F = 2PR / (P+R)
Tolerance 1e-4 on P, R, F: the kernel accumulates dot products and norms in float32 and divides afterwards, so a similarity is off
by at most about H * 2^-24 * |c||r| relative to |c||r|, 4.6e-5 at H = 768; the bound is twice that.  Rows are 0.6 * base + noise
with one base per pair (base ~ N(0, 1), noise ~ N(0, 0.6^2)), which keeps the float64 P + R >= 0.49 at every shape and seed here
(asserted on the reference before anything is compared), so F = 2PR / (P + R) is well conditioned.
Padding rows and the gaps of a padded row stride are NaN: nothing beyond a pair's lengths may reach its scores.
Every comparison prints its figure before it asserts."""
import numpy as np
import pytest
import torch

from bertscore_ref import ref_scores

pytestmark = pytest.mark.gpu

TOL = 1e-4
SHAPES = [(1, 1), (3, 17), (16, 16), (17, 15), (33, 64), (65, 130), (200, 512)]
N = 5


def make_side(L, H, lens, base, dtype, dev, seed, pad_ld=0, pad_pair=0):
    """[N, L, H] view (row stride H + pad_ld, pair stride L * ld + pad_pair) of a NaN-filled buffer: valid rows 0.6 * base + noise"""
    g = torch.Generator().manual_seed(seed)
    n = len(lens)
    ld = H + pad_ld
    sp = L * ld + pad_pair
    buf = torch.full((n * sp,), float("nan"), dtype=dtype)
    x = torch.as_strided(buf, (n, L, H), (sp, ld, 1))
    for i, l in enumerate(lens):
        x[i, :l] = (0.6 * base[i][None, :] + 0.6 * torch.randn(l, H, generator=g)).to(dtype)
    return torch.as_strided(buf.to(dev), (n, L, H), (sp, ld, 1))


def edge_weights(L, lens):
    """1 per token, 0 on the first and last valid token of a sentence of 3 or more (<s>, </s>); NaN beyond the length"""
    w = torch.full((len(lens), L), float("nan"))
    for i, l in enumerate(lens):
        w[i, :l] = 1.0
        if l >= 3:
            w[i, 0] = w[i, l - 1] = 0.0
    return w


def make_case(Lc, Lr, H, dtype, dev, seed=0, strided=False):
    rng = np.random.Generator(np.random.PCG64(seed + 1000 * Lc + Lr))
    lc = [Lc, 1] + [int(rng.integers(1, Lc + 1)) for _ in range(N - 2)]
    lr = [Lr, 1] + [int(rng.integers(1, Lr + 1)) for _ in range(N - 2)]
    base = torch.randn(N, H, generator=torch.Generator().manual_seed(seed + 7))
    pad = (16, 24) if strided else (0, 0)
    c = make_side(Lc, H, lc, base, dtype, dev, seed + 1, *pad)
    r = make_side(Lr, H, lr, base, dtype, dev, seed + 2, *pad)
    return c, r, lc, lr, edge_weights(Lc, lc), edge_weights(Lr, lr)


def _np(x):
    return x.detach().double().cpu().numpy()


def _i32(l, dev):
    return torch.tensor(l, dtype=torch.int32, device=dev)


def _check(name, got, want, tol):
    assert torch.isfinite(got).all(), (name, got)
    assert want[:, :2].sum(1).min() >= 0.49, (name, want)           # the data recipe: F is well conditioned
    err = np.abs(_np(got) - want).max(0)
    print(f"{name}: max |dP| {err[0]:.3e}  |dR| {err[1]:.3e}  |dF| {err[2]:.3e}  min P+R {want[:, :2].sum(1).min():.3f}")
    assert err.max() <= tol, (name, err)
    return err.max()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("H", [64, 768])
@pytest.mark.parametrize("Lc,Lr", SHAPES)
def test_kernel_against_float64(Lc, Lr, H, dtype, dev):
    from fcmf_framework import ops
    strided = Lc in (3, 17, 65)                         # row stride H + 16, pair stride beyond L * ld
    c, r, lc, lr, wc, wr = make_case(Lc, Lr, H, dtype, dev, strided=strided)
    if strided:
        assert c.stride(1) > H
    got = ops.bertscore(c, r, _i32(lc, dev), _i32(lr, dev), wc.to(dev), wr.to(dev))
    assert got.shape == (N, 3) and got.dtype == torch.float32
    want = ref_scores(_np(c), _np(r), lc, lr, wc.numpy(), wr.numpy())
    _check(f"bertscore {Lc}x{Lr} H={H} {dtype}", got, want, TOL)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_null_weights(dtype, dev):
    from fcmf_framework import ops
    c, r, lc, lr, _, _ = make_case(33, 64, 768, dtype, dev, seed=3)
    got = ops.bertscore(c, r, _i32(lc, dev), _i32(lr, dev))
    _check(f"bertscore NULL weights {dtype}", got, ref_scores(_np(c), _np(r), lc, lr), TOL)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_degenerate_pairs_are_zero_and_leave_neighbours_alone(dtype, dev):
    from fcmf_framework import ops
    Lc, Lr, H = 17, 15, 64
    c, r, lc, lr, wc, wr = make_case(Lc, Lr, H, dtype, dev, seed=5)      # 5 normal pairs
    g = torch.Generator().manual_seed(11)
    n = 10
    C = torch.full((n, Lc, H), float("nan"), dtype=dtype, device=dev)
    R = torch.full((n, Lr, H), float("nan"), dtype=dtype, device=dev)
    WC, WR = torch.full((n, Lc), float("nan")), torch.full((n, Lr), float("nan"))
    LC, LR = [0] * n, [0] * n
    normal = [0, 2, 4, 7, 9]
    for k, i in enumerate(normal):
        C[i], R[i], WC[i], WR[i], LC[i], LR[i] = c[k], r[k], wc[k], wr[k], lc[k], lr[k]
    fill = lambda l: torch.randn(l, H, generator=g).to(dtype).to(dev)
    # 1: empty candidate; 3: empty reference; 5 / 6: an all-zero weight row on either side; 8: two orthogonal one-token sentences
    LC[1], LR[1] = 0, 7
    R[1, :7] = fill(7); WR[1, :7] = 1.0
    LC[3], LR[3] = 6, 0
    C[3, :6] = fill(6); WC[3, :6] = 1.0
    for i, (zc, zr) in ((5, (0.0, 1.0)), (6, (1.0, 0.0))):
        LC[i], LR[i] = 4, 5
        C[i, :4] = fill(4); R[i, :5] = fill(5)
        WC[i, :4] = zc; WR[i, :5] = zr
    LC[8] = LR[8] = 1
    e = torch.zeros(2, H)
    e[0, :H // 2] = 1.0
    e[1, H // 2:] = -2.0
    C[8, 0], R[8, 0] = e[0].to(dtype).to(dev), e[1].to(dtype).to(dev)
    WC[8, 0] = WR[8, 0] = 1.0
    got = ops.bertscore(C, R, _i32(LC, dev), _i32(LR, dev), WC.to(dev), WR.to(dev))
    print("degenerate rows:", got[[1, 3, 5, 6, 8]].tolist())
    assert torch.isfinite(got).all()
    assert torch.equal(got[[1, 3, 5, 6, 8]], torch.zeros(5, 3, device=dev))
    alone = ops.bertscore(c, r, _i32(lc, dev), _i32(lr, dev), wc.to(dev), wr.to(dev))
    assert torch.equal(got[normal], alone)                       # same bits as without the degenerate neighbours
    _check(f"normal pairs beside degenerate ones {dtype}", got[normal], ref_scores(_np(c), _np(r), lc, lr, wc.numpy(), wr.numpy()), TOL)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_identical_sentences_score_one(dtype, dev):
    from fcmf_framework import ops
    c, _, lc, _, wc, _ = make_case(33, 33, 768, dtype, dev, seed=9)
    got = ops.bertscore(c, c.clone(), _i32(lc, dev), _i32(lc, dev), wc.to(dev), wc.to(dev))
    err = (got - 1).abs().max().item()
    print(f"identical {dtype}: max |score - 1| {err:.3e}")
    assert err <= 1e-5


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_swapping_operands_swaps_p_and_r(dtype, dev):
    from fcmf_framework import ops
    c, r, lc, lr, wc, wr = make_case(33, 64, 768, dtype, dev, seed=13)
    a = ops.bertscore(c, r, _i32(lc, dev), _i32(lr, dev), wc.to(dev), wr.to(dev))
    b = ops.bertscore(r, c, _i32(lr, dev), _i32(lc, dev), wr.to(dev), wc.to(dev))
    err = (a - b[:, [1, 0, 2]]).abs().max().item()
    print(f"swap {dtype}: max |(P, R, F) - (R', P', F')| {err:.3e}")
    assert err <= 1e-5


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_two_launches_give_the_same_bits(dtype, dev):
    from fcmf_framework import ops
    c, r, lc, lr, wc, wr = make_case(200, 512, 768, dtype, dev, seed=17)
    args = (c, r, _i32(lc, dev), _i32(lr, dev), wc.to(dev), wr.to(dev))
    a = ops.bertscore(*args)
    b = ops.bertscore(*args)
    assert torch.equal(a, b)


def test_limits_are_loud(dev):
    from fcmf_framework import _hip as H, ops
    L = H.lib()
    x = torch.zeros(2 * 513 * 64, dtype=torch.bfloat16, device=dev)
    ln = torch.ones(2, dtype=torch.int32, device=dev)
    o = torch.zeros(2, 3, device=dev)

    def call(Lc, Lr, Hd, ld=None, dtype=H.BF16, cand=x.data_ptr(), lens=ln.data_ptr()):
        ld = Hd if ld is None else ld
        return L.fcmf_bertscore(cand, x.data_ptr(), lens, ln.data_ptr(), None, None, o.data_ptr(), 2, Lc, Lr, Hd, ld, Lc * ld,
                                ld, Lr * ld, dtype, H.stream())
    assert call(16, 16, 64) == 0
    assert call(16, 16, 60) == H.ERR_UNSUPPORTED                  # H % 8
    assert call(513, 16, 64) == H.ERR_UNSUPPORTED                 # beyond the encoder's position limit, either side
    assert call(16, 513, 64) == H.ERR_UNSUPPORTED
    assert call(16, 16, 64, ld=68) == H.ERR_UNSUPPORTED           # rows not 16-byte aligned
    assert call(16, 16, 64, cand=x.data_ptr() + 2) == H.ERR_UNSUPPORTED
    assert call(16, 16, 64, dtype=H.F64) == H.ERR_UNSUPPORTED
    assert call(-1, 16, 64) == -1 and call(16, 16, 0) == -1       # FCMF_ERR_ARG
    assert call(16, 16, 64, cand=None) == -1 and call(16, 16, 64, lens=None) == -1
    torch.cuda.synchronize()
    one = torch.ones(2, dtype=torch.int32, device=dev)
    with pytest.raises(H.HipLibraryError):
        ops.bertscore(torch.zeros(2, 4, 60, device=dev), torch.zeros(2, 4, 60, device=dev), one, one)
    with pytest.raises(H.HipLibraryError):
        ops.bertscore(torch.zeros(2, 513, 64, device=dev), torch.zeros(2, 4, 64, device=dev), one, one)
    with pytest.raises(H.HipLibraryError):
        ops.bertscore(torch.zeros(2, 4, 64), torch.zeros(2, 4, 64, device=dev), one, one)      # a CPU tensor
    with pytest.raises(H.HipLibraryError):
        ops.bertscore(torch.zeros(2, 4, 64, device=dev), torch.zeros(2, 4, 64, device=dev), one.cpu(), one)
