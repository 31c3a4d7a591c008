"""fcmf_logits_constrain (csrc/constrain.hip, ops.logits_constrain) against tests/constraints_ref.py, the numpy statement of its
contract, BIT FOR BIT: the kernel's arithmetic is one float32 multiply or correctly rounded divide and one rounding, so there is no
tolerance.  The logits live in NaN-filled interiors of rowwise_ref.guarded buffers in the three layouts of test_sample_gpu.py
(aligned / column-padded / unaligned with an odd stride); after a launch the WHOLE interior -- edited columns, unedited columns,
the NaN padding at and beyond V, the gaps between rows -- is compared as integers with the expected image, and the guard frame is
checked.  Every row of a case has its own sequence, drawn from a small alphabet (so tokens repeat and n-grams recur) with ids
outside [0, V) mixed in.  Then the kernel followed by ops.logsoftmax_topk / ops.sample_token against float64 on the edited rows,
with the bounds of test_topk_gpu.py / test_sample_gpu.py (1e-4; every sampled row decided)."""
import itertools

import numpy as np
import pytest
import torch

import constraints_ref as C
import rowwise_ref as R
import sampling_ref as S
from test_sample_gpu import BF16, F32, Rows

pytestmark = pytest.mark.gpu

INF = float("inf")
INT = {F32: torch.int32, BF16: torch.int16}


def image(rows):
    """the whole interior of the guarded buffer as integers, on the CPU"""
    return rows.g.view.view(INT[rows.x.dtype]).cpu().clone()


def expected_image(rows, before, want):
    """`before` with the [rows, V] window replaced by `want` (float32 numpy holding storage-type values)"""
    exp = before.clone()
    w = torch.from_numpy(np.ascontiguousarray(want)).to(rows.x.dtype).view(INT[rows.x.dtype])
    off = rows.view.storage_offset() - rows.g.view.storage_offset()
    torch.as_strided(exp, (rows.rows, rows.V), (rows.ld, 1), off).copy_(w)
    return exp


def device_hist(hist, transposed, dev):
    """hist int64 [n, L] on the device: contiguous, or the transposed view of a [L, n] tensor"""
    h = torch.as_tensor(np.asarray(hist), dtype=torch.int64)
    return h.t().contiguous().to(dev).t() if transposed else h.contiguous().to(dev)


def launch(rows, hist, theta=1.0, n=0, m=0, sep=-1, ban=None, n_rows=None, V=None, ld=None, L=None, dtype_code=None, n_ban=None,
           logits_ptr=None, hist_ptr=None):
    from fcmf_framework import _hip as H
    rc = H.lib().fcmf_logits_constrain(rows.view.data_ptr() if logits_ptr is None else logits_ptr, rows.ld if ld is None else ld,
                                       rows.rows if n_rows is None else n_rows, rows.V if V is None else V,
                                       hist.data_ptr() if hist_ptr is None else hist_ptr, hist.stride(0), hist.stride(1),
                                       hist.shape[1] if L is None else L, theta, n, m, sep, None if ban is None else ban.data_ptr(),
                                       (0 if ban is None else ban.shape[0]) if n_ban is None else n_ban,
                                       H.dt(rows.view) if dtype_code is None else dtype_code, H.stream())
    torch.cuda.synchronize()
    rows.g.check()
    return rc


def check(rows, hist, transposed, dev, what, theta=1.0, n=0, m=0, sep=-1, ban=()):
    """launch on `rows` and compare the whole interior with the reference's image -> the number of -inf written"""
    bf16 = rows.x.dtype == BF16
    want = C.constrain_rows(rows.x.float().numpy(), hist, rows.V, bf16=bf16, repetition_penalty=theta, no_repeat_ngram_size=n,
                            min_length=m, sep_id=sep, ban_ids=ban)
    before = image(rows)
    ban_t = torch.tensor(list(ban), dtype=torch.int32, device=dev) if len(ban) else None
    rc = launch(rows, device_hist(hist, transposed, dev), theta, n, m, sep, ban_t)
    assert rc == 0, (what, rc)
    got, exp = image(rows), expected_image(rows, before, want)
    bad = (got != exp).nonzero().flatten().tolist()
    print(f"{what}: {int((exp != before).sum())} elements edited, {int(np.isneginf(want).sum() - np.isneginf(rows.x.float().numpy()).sum())} "
          f"new -inf, {len(bad)} elements differ from the reference")
    assert not bad, (what, bad[:8])
    return int(np.isneginf(want).sum())


SPECIAL = [0.0, -0.0, -INF, 1e30, -1e30, 3e38, -3e38, 1.5, -2.25, 1e-30]


def make_case(V, dtype, rows, L, seed, alphabet=None):
    """x [rows, V] with the special values on the alphabet's columns, and hist [rows, L] over alphabet + out-of-range ids"""
    rng = np.random.RandomState(seed)
    x = (torch.randn(rows, V, generator=torch.Generator().manual_seed(seed)) * 3.0)
    k = alphabet or max(2, min(V, max(3, L // 3)))
    hist = np.empty((rows, L), dtype=np.int64)
    for r in range(rows):
        alpha = np.unique(np.concatenate((rng.randint(0, V, size=k), [0, V - 1] if r % 2 else [V // 2])))
        for j, a in enumerate(alpha):
            if (j + r) % 2 == 0:
                x[r, a] = SPECIAL[(j + r) % len(SPECIAL)]
        pool = np.concatenate((alpha, alpha, alpha, [-1, V, V + 5]))
        hist[r] = pool[rng.randint(0, len(pool), size=L)]
    return x.to(dtype), hist


def bans(V, count, seed):
    rng = np.random.RandomState(seed)
    if count == 0:
        return []
    if count == 1:
        return [int(rng.randint(0, V))]
    return [-1, V, V + 5] + rng.randint(-3, V + 9, size=count - 3).tolist()


LS = [1, 2, 3, 64, 65, 257, 512]
GRID = [(V, dtype, kind, i) for i, (V, dtype, kind) in
        enumerate(itertools.product((1, 7, 512, 64001), (F32, BF16), ("aligned", "padded", "odd")))]


@pytest.mark.parametrize("V,dtype,kind,i", GRID, ids=lambda v: {F32: "f32", BF16: "bf16"}.get(v, str(v)))
def test_constrain_grid(dev, V, dtype, kind, i):
    """every V x dtype x layout once; L, rows, theta, n, the minimum length (L = m - 1 / L = m), the ban count, sep inside or outside
    and the layout of hist cycle through their values along the grid (7, 3, 3, 5, 2, 3, 4 and 2 values: coprime enough that every
    value meets every V)"""
    for j in (i, i + 11):
        L, rows = LS[j % 7], (1, 5, 130)[j % 3]
        theta, n, n_ban = (0.5, 1.3, 2.0)[(j // 3) % 3], j % 5, (0, 1, 1024)[(j // 2) % 3]
        m = L + 1 if j % 2 else L
        sep = (V // 3, -1, V, V + 5)[j % 4] if j % 2 else V // 3
        x, hist = make_case(V, dtype, rows, L, 100 + j)
        what = f"V {V} {dtype} {kind} rows {rows} L {L} theta {theta} n {n} m {m} sep {sep} n_ban {n_ban} hist^T {j % 2 == 0}"
        check(Rows(x, kind, dev), hist, j % 2 == 0, dev, what, theta, n, m, sep, bans(V, n_ban, j))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_every_L_and_ngram_edge(dev, dtype):
    """every L of the list with n = 2 and a penalty, then n in 1 .. 4 at L = n - 1, n, n + 1 over two tokens (every start matches or
    nearly does), V 512 and V 7, five rows"""
    for L in LS:
        x, hist = make_case(512, dtype, 5, L, 300 + L)
        check(Rows(x, "padded", dev), hist, L % 2 == 0, dev, f"{dtype} L {L}", 1.3, 2, L + 1, 2, bans(512, 1, L))
    for n in (1, 2, 3, 4):
        for L in (n - 1, n, n + 1, n + 4):
            if L >= 1:
                rng = np.random.RandomState(10 * n + L)
                x = (torch.randn(5, 7, generator=torch.Generator().manual_seed(n + L)) * 3.0).to(dtype)
                # one token throughout (every start matches, the matches overlap the suffix), two alternating, two at random (twice),
                # one token with an id outside [0, V) as the last
                hist = np.stack([np.full(L, 3), np.arange(L) % 2 * 4 + 1, rng.randint(0, 2, L) + 5, rng.randint(0, 2, L) * 6,
                                 np.concatenate((np.full(L - 1, 2), [7]))]).astype(np.int64)
                got = check(Rows(x, "odd", dev), hist, L % 2 == 1, dev, f"{dtype} n {n} L {L}", 1.0, n)
                assert got == 0 if L < n else got >= 1 + (L > n), (n, L, got)      # L < n bans nothing; the constant row always does


def test_hand_worked_rows(dev):
    """one token 2 .. 5 times: penalised once; [a, a, a] with n = 2; several matches of the suffix; a column penalised and banned"""
    V = 16
    x = torch.tensor([[4.0, -4.0, 0.0, 2.0, -0.0, -INF, 8.0, 1e30] + [3.0] * 8] * 6)
    hist = np.array([[0, 0, 1, 1, 1, 6],          # 0 twice, 1 three times
                     [6, 6, 6, 6, 0, 0],          # 6 four times
                     [1, 1, 1, 1, 1, 4],          # 1 five times
                     [3, 3, 3, 3, 3, 3],          # [a, a, a, ...], n = 2 bans a
                     [3, 4, 3, 6, 2, 3],          # suffix 3: followed by 4 and by 6
                     [7, 5, 7, 5, 7, 5]])
    for dtype in (F32, BF16):
        rows = Rows(x.to(dtype), "aligned", dev)
        check(rows, hist, False, dev, f"hand {dtype} theta 2", 2.0)
        got = rows.view.float().cpu()
        assert got[0, :2].tolist() == [2.0, -8.0] and got[1, 6].item() == 4.0 and got[2, 1].item() == -8.0      # once, not theta^k
        assert got[0, 6].item() == 4.0 and got[5, 7].item() == torch.tensor(1e30).to(dtype).float().item() / 2
        rows = Rows(x.to(dtype), "odd", dev)
        check(rows, hist, True, dev, f"hand {dtype} theta 2 n 2", 2.0, 2)
        got = rows.view.float().cpu()
        assert torch.isneginf(got[3, 3]) and torch.isneginf(got[4, [4, 6]]).all() and got[4, 3].item() == 1.0      # penalised AND banned: -inf
        assert torch.isneginf(got[5, 7]) and got[5, 5].item() == -INF and torch.isfinite(got[0, :5]).all()


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_everything_off_touches_nothing_and_two_launches_agree(dev, dtype):
    x, hist = make_case(1000, dtype, 5, 65, 7)
    rows = Rows(x, "padded", dev)
    before = image(rows)
    h = device_hist(hist, False, dev)
    assert launch(rows, h) == 0                                          # theta 1, n 0, m 0, no bans
    assert launch(rows, h, m=65, sep=3) == 0                             # L == m: nothing to do either
    assert launch(rows, h, theta=2.0, n=2, n_rows=0) == 0                # no rows
    assert torch.equal(image(rows), before)
    ban = torch.tensor(bans(1000, 1024, 1), dtype=torch.int32, device=dev)
    a, b = Rows(x, "padded", dev), Rows(x, "padded", dev)
    for r in (a, b):
        assert launch(r, h, 1.3, 3, 80, 5, ban) == 0
    assert torch.equal(image(a), image(b)) and not torch.equal(image(a), before)


def test_argument_errors_come_back_without_a_launch(dev):
    from fcmf_framework import _hip as H
    x, hist = make_case(40, F32, 3, 6, 9)
    rows = Rows(x, "aligned", dev)
    before = image(rows)
    h = device_hist(hist, False, dev)
    ban = torch.tensor([1, 2], dtype=torch.int32, device=dev)
    long_h = torch.zeros(3, 513, dtype=torch.int64, device=dev)
    many = torch.zeros(1025, dtype=torch.int32, device=dev)
    on = dict(theta=2.0, n=2)
    for kw, code in ((dict(theta=0.0), H.ERR_ARG), (dict(theta=-1.0), H.ERR_ARG), (dict(theta=INF), H.ERR_ARG), (dict(theta=float("nan")), H.ERR_ARG),
                     (dict(n=-1), H.ERR_ARG), (dict(m=-1), H.ERR_ARG), (dict(n_ban=-1), H.ERR_ARG), (dict(n_ban=2), H.ERR_ARG),
                     (dict(n_rows=-1), H.ERR_ARG), (dict(V=0), H.ERR_ARG), (dict(ld=39), H.ERR_ARG), (dict(L=0), H.ERR_ARG),
                     (dict(logits_ptr=0), H.ERR_ARG), (dict(hist_ptr=0), H.ERR_ARG), (dict(dtype_code=H.F64), H.ERR_UNSUPPORTED)):
        assert launch(rows, h, **{**on, **kw}) == code, kw
    assert launch(rows, long_h, **on) == H.ERR_UNSUPPORTED               # 513 tokens
    assert launch(rows, h, ban=many, **on) == H.ERR_UNSUPPORTED          # 1025 suppressed ids
    assert launch(rows, h, ban=ban, n_ban=0) == 0
    assert torch.equal(image(rows), before)


def test_ops_logits_constrain_takes_strided_views_and_checks_its_arguments(dev):
    from fcmf_framework import _hip as H, ops
    x, hist = make_case(1000, BF16, 6, 9, 11)
    rows = Rows(x, "padded", dev)
    before = image(rows)
    buf2d = torch.as_strided(rows.view, (6, rows.ld), (rows.ld, 1))
    ban = torch.tensor([5, 999, 1000], dtype=torch.int32, device=dev)
    assert ops.logits_constrain(buf2d, 1000, device_hist(hist, True, dev), repetition_penalty=1.3, no_repeat_ngram_size=2, min_length=12,
                                sep_id=2, ban_ids=ban) is None
    want = C.constrain_rows(x.float().numpy(), hist, 1000, bf16=True, repetition_penalty=1.3, no_repeat_ngram_size=2, min_length=12, sep_id=2,
                            ban_ids=[5, 999, 1000])
    torch.cuda.synchronize()
    rows.g.check()
    assert torch.equal(image(rows), expected_image(rows, before, want))
    h = device_hist(hist, False, dev)
    with pytest.raises(H.HipLibraryError, match="overlap"):
        ops.logits_constrain(x[:1].to(dev).expand(3, 1000), 1000, h[:3], repetition_penalty=2.0)
    with pytest.raises(H.HipLibraryError, match="history"):
        ops.logits_constrain(buf2d, 1000, h[:5], repetition_penalty=2.0)
    with pytest.raises(H.HipLibraryError, match="history"):
        ops.logits_constrain(buf2d, 1000, h.int(), repetition_penalty=2.0)
    with pytest.raises(H.HipLibraryError, match="beyond"):
        ops.logits_constrain(buf2d, 1000, torch.zeros(6, 513, dtype=torch.int64, device=dev), repetition_penalty=2.0)
    with pytest.raises(H.HipLibraryError, match="ban_ids"):
        ops.logits_constrain(buf2d, 1000, h, ban_ids=ban.long())
    with pytest.raises(ValueError, match="repetition_penalty"):
        ops.logits_constrain(buf2d, 1000, h, repetition_penalty=0.0)
    with pytest.raises(ValueError, match="no_repeat_ngram_size"):
        ops.logits_constrain(buf2d, 1000, h, no_repeat_ngram_size=-1)


# ---- the kernel followed by the two tails -----------------------------------------------------------------------------------
TAIL = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_length=40, sep_id=2)
TOL = 1e-4


def tail_case(dtype, dev, seed):
    V, n, L = 4099, 12, 33
    rng = np.random.RandomState(seed)
    x = (torch.randn(n, V, generator=torch.Generator().manual_seed(seed)) * 3.0).to(dtype)
    top = torch.topk(x.float(), 6, dim=1).indices.numpy()              # the sequences hold the rows' own best tokens: the edit moves the top
    hist = np.stack([top[r][rng.randint(0, 6, size=L)] for r in range(n)])
    ban = [int(top[r, 0]) for r in range(0, n, 3)] + [V, -1]
    rows = Rows(x, "padded", dev)
    want = C.constrain_rows(x.float().numpy(), hist, V, bf16=dtype == BF16, ban_ids=ban, **TAIL)
    buf2d = torch.as_strided(rows.view, (n, rows.ld), (rows.ld, 1))
    return rows, buf2d, hist, ban, want


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_constrain_then_logsoftmax_topk(dev, dtype):
    from fcmf_framework import ops
    rows, buf2d, hist, ban, want = tail_case(dtype, dev, 21)
    K, V = 8, rows.V
    plain = torch.sort(rows.x.double(), dim=1, descending=True, stable=True).indices[:, :K]
    ops.logits_constrain(buf2d, V, device_hist(hist, False, dev), ban_ids=torch.tensor(ban, dtype=torch.int32, device=dev), **TAIL)
    logp, ids = ops.logsoftmax_topk(buf2d, V, K)
    wd = torch.from_numpy(want).double()
    order = torch.sort(wd, dim=1, descending=True, stable=True).indices[:, :K]
    ref = torch.log_softmax(wd, dim=1).gather(1, order)
    err = (logp.cpu().double() - ref).abs().max().item()
    moved = int((order != plain).any(dim=1).sum())
    print(f"{dtype}: constrained top-{K} log-probabilities vs float64, max |d| {err:.3e} (bound {TOL}); rows whose top-{K} the edit changed: {moved}")
    assert torch.equal(ids.cpu().long(), order) and torch.isfinite(logp).all()
    assert err < TOL
    assert moved == rows.rows
    assert np.isneginf(want[np.arange(rows.rows), 2]).all() and not (ids.cpu() == 2).any()      # sep below the minimum length


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_constrain_then_sample_token(dev, dtype):
    from fcmf_framework import ops
    rows, buf2d, hist, ban, want = tail_case(dtype, dev, 22)
    V, n = rows.V, rows.rows
    ctr = [50 + 3 * r for r in range(n)]
    sampler = dict(temperature=0.7, top_k=50, top_p=0.9)
    want_ids, want_logp, ok, lead = S.sample_rows(want.astype(np.float64), ctr, R.SEED_HI, 0.7, 50, 0.9)
    print(f"{dtype}: smallest lead {lead.min():.3e}, undecided rows {(~ok).sum()}")
    assert ok.all(), "rows not decided: choose another seed"
    plain_ids = S.sample_rows(rows.x.double().numpy(), ctr, R.SEED_HI, 0.7, 50, 0.9)[0]
    ops.logits_constrain(buf2d, V, device_hist(hist, True, dev), ban_ids=torch.tensor(ban, dtype=torch.int32, device=dev), **TAIL)
    ids, logp = ops.sample_token(buf2d, V, torch.tensor(ctr, device=dev), R.SEED_HI, **sampler)
    err = np.abs(logp.cpu().double().numpy() - want_logp).max()
    print(f"{dtype}: constrained draws vs float64, max |logp - float64| {err:.3e} (bound {TOL}); draws the edit changed: {(plain_ids != want_ids).sum()}")
    assert ids.cpu().tolist() == want_ids.tolist()
    assert err < TOL
    assert (plain_ids != want_ids).sum() >= n // 2
