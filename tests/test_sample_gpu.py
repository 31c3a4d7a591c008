"""fcmf_sample_token (csrc/sample.hip, ops.sample_token) against tests/sampling_ref.py, the float64 statement of its contract on
the SAME stored values.  ids must be equal exactly and logp within 1e-4 (test_topk_gpu.py's bound for the same quantity).  Every
row of every case is asserted DECIDED on the CPU first (sampling_ref's header): no column within 1e-4 of the nucleus boundary may
win, and the winner leads by 1e-3; the seeds below were chosen for that, and a seed that breaks it fails the test.
Inputs live in NaN-filled interiors of rowwise_ref.guarded buffers (padding columns are NaN), outputs in guarded buffers.
Layouts: "aligned" (16-byte rows, ld the next multiple of 16 bytes), "padded" (ld = V rounded up to 32 columns: 64001 -> 64032, the
vocabulary projection's buffer), "odd" (base one element off a 16-byte boundary and an odd ld: the one-element path).
At most 24 rows per case.  Every comparison prints its figure before it asserts."""
import numpy as np
import pytest
import torch

import rowwise_ref as R
import sampling_ref as S

pytestmark = pytest.mark.gpu

TOL = 1e-4
F32, BF16 = torch.float32, torch.bfloat16


def layout(V, dtype, kind):
    """-> (ld, offset) in elements"""
    per16 = 16 // torch.empty((), dtype=dtype).element_size()
    if kind == "aligned":
        return (V + per16 - 1) // per16 * per16, 0
    if kind == "padded":
        return (V + 31) // 32 * 32, 0
    ld = V + 1 if V % 2 == 0 else V + 2
    return ld, 1


class Rows:
    """x [rows, V] placed at (ld, offset) inside a NaN-filled guarded buffer on the device"""

    def __init__(self, x, kind, dev):
        self.x = x
        self.rows, self.V = x.shape
        self.ld, off = layout(self.V, x.dtype, kind)
        self.g = R.guarded((off + self.rows * self.ld + 8,), x.dtype, dev)
        self.g.view.fill_(float("nan"))
        self.view = torch.as_strided(self.g.view, (self.rows, self.V), (self.ld, 1), self.g.view.storage_offset() + off)
        self.view.copy_(x.to(dev))
        assert (self.view.data_ptr() % 16 == 0) == (kind != "odd")


def launch(rows, ctr, seed, T, top_k, top_p, dtype_code=None, n=None, V=None, ld=None):
    """-> (rc, ids int32 [rows], logp float32 [rows]) on the CPU; the guard bands of both outputs are checked"""
    from fcmf_framework import _hip as H
    dev = rows.view.device
    n = rows.rows if n is None else n
    gi, gl = R.guarded((max(rows.rows, 1),), F32, dev), R.guarded((max(rows.rows, 1),), F32, dev)
    gi.view.view(torch.int32).fill_(-1)
    gl.view.fill_(float("nan"))
    c = torch.tensor(list(ctr), dtype=torch.int64, device=dev)
    rc = H.lib().fcmf_sample_token(rows.view.data_ptr(), rows.ld if ld is None else ld, n, rows.V if V is None else V, T, top_k, top_p,
                                   seed, c.data_ptr(), gi.view.data_ptr(), gl.view.data_ptr(),
                                   H.dt(rows.view) if dtype_code is None else dtype_code, H.stream())
    torch.cuda.synchronize()
    R.check_all(gi, gl, rows.g)
    return rc, gi.view.view(torch.int32).cpu().clone(), gl.view.cpu().clone()


def reference(x, ctr, seed, T, top_k, top_p, what):
    ids, logp, ok, lead = S.sample_rows(x.double().numpy(), ctr, seed, T, top_k, top_p)
    print(f"{what}: smallest lead {lead.min():.3e}, undecided rows {(~ok).sum()}")
    assert ok.all(), (what, "rows not decided: choose another seed", np.nonzero(~ok)[0].tolist())
    return ids, logp


def check(rows, ctr, seed, T, top_k, top_p, what):
    want_ids, want_logp = reference(rows.x, ctr, seed, T, top_k, top_p, what)
    rc, ids, logp = launch(rows, ctr, seed, T, top_k, top_p)
    assert rc == 0, (what, rc)
    err = np.abs(logp.double().numpy() - want_logp).max()
    print(f"{what}: max |logp - float64| {err:.3e} (bound {TOL})")
    assert ids.tolist() == want_ids.tolist(), (what, "ids")
    assert err < TOL, (what, err)
    return ids, logp


def normal(rows, V, sigma, dtype, seed):
    return (torch.randn(rows, V, generator=torch.Generator().manual_seed(seed)) * sigma).to(dtype)


# (V, dtype, layout, temperature, top_k, top_p, rows, sigma, seed of the logits, seed of the draw)
CASES = [
    (64001, BF16, "padded", 0.7, 50, 0.9, 24, 3.0, 1, R.SEED_HI),
    (64001, BF16, "padded", 1.0, 0, 0.9, 24, 3.0, 2, R.SEED_LO),
    (64001, BF16, "aligned", 1.3, 0, 0.95, 12, 1.0, 3, R.SEED_HI),
    (64001, BF16, "odd", 1.0, 0, 1.0, 12, 3.0, 4, R.SEED_LO),
    (64001, F32, "odd", 2.0, 5, 1.0, 8, 3.0, 5, R.SEED_HI),
    (64001, F32, "aligned", 0.25, 0, 0.8, 8, 3.0, 6, R.SEED_LO),
    (64001, F32, "padded", 0.7, 50, 0.95, 8, 3.0, 7, R.SEED_HI),
    (64001, F32, "padded", 1.0, 70000, 1e-6, 8, 3.0, 8, R.SEED_LO),
    (1000, F32, "aligned", 0.7, 0, 0.8, 24, 4.0, 9, R.SEED_HI),
    (1000, BF16, "odd", 2.0, 50, 0.95, 24, 4.0, 10, R.SEED_LO),
    (1000, F32, "padded", 1.0, 1000, 1e-6, 24, 4.0, 11, R.SEED_HI),
    (1000, BF16, "padded", 0.25, 5, 0.8, 24, 2.0, 12, R.SEED_LO),
    (37, F32, "odd", 1.0, 5, 1.0, 24, 2.0, 13, R.SEED_HI),
    (37, BF16, "aligned", 0.25, 50, 0.95, 24, 2.0, 14, R.SEED_LO),
    (37, BF16, "padded", 2.0, 0, 0.8, 24, 2.0, 15, R.SEED_HI),
    (7, F32, "aligned", 0.7, 5, 0.8, 24, 2.0, 16, R.SEED_LO),
    (7, BF16, "odd", 2.0, 1, 1.0, 24, 2.0, 17, R.SEED_HI),
    (7, F32, "padded", 1.0, 0, 0.95, 24, 2.0, 18, R.SEED_LO),
    (1, F32, "aligned", 0.7, 0, 0.8, 5, 2.0, 19, R.SEED_HI),
    (1, BF16, "odd", 2.0, 1, 1e-6, 5, 2.0, 20, R.SEED_LO),
]


def case_inputs(case):
    V, dtype, kind, T, top_k, top_p, rows, sigma, xseed, seed = case
    x = normal(rows, V, sigma, dtype, xseed)
    ctr = [1000 * xseed + 37 * r for r in range(rows)]
    return x, ctr


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"V{c[0]}-{'f32' if c[1] == F32 else 'bf16'}-{c[2]}-T{c[3]}-k{c[4]}-p{c[5]}")
def test_sample_grid(dev, case):
    V, dtype, kind, T, top_k, top_p, rows, sigma, xseed, seed = case
    x, ctr = case_inputs(case)
    check(Rows(x, kind, dev), ctr, seed, T, top_k, top_p, f"V {V} {dtype} {kind} T {T} k {top_k} p {top_p}")


def topk1_rows():
    """rows whose maximum is unique (a tied maximum is kept whole by the contract, and then the seed does choose)"""
    x = normal(24, 4099, 3.0, BF16, 30)
    x[torch.arange(24), (torch.arange(24) * 173) % 4099] = 40.0
    return x


def test_top_k_1_returns_the_maximum_whatever_the_seed(dev):
    for x, kind in ((topk1_rows(), "padded"), (normal(24, 1000, 3.0, F32, 31), "odd")):
        want = torch.sort(x.double(), dim=1, descending=True, stable=True).indices[:, 0]
        assert (x.double().max(dim=1).values[:, None] == x.double()).sum(dim=1).tolist() == [1] * 24
        rows = Rows(x, kind, dev)
        for seed in (R.SEED_LO, R.SEED_HI, 12345):
            rc, ids, logp = launch(rows, range(24), seed, 0.7, 1, 0.9)
            assert rc == 0 and ids.tolist() == want.tolist()
            err = max(abs(logp[r].item() - S.logp_of(x[r].double().numpy(), int(want[r]))) for r in range(24))
            assert err < TOL, err


def tie_rows(V, seed):
    """bf16 rows of nine distinct values: 2 .. 4, 7 .. 11, 15 .. 19, 40 .. 44, 70 .. 74, 150 .. 154 columns (by row) at 6, 5, 4, 3, 2, 1
    and the rest at 0, -1, -2 (20 / 30 / 50 %), each row in its own random order -- so top_k = 5, 20 and 50 all cut through a tied
    value, and the nucleus boundary falls between tied groups"""
    g = torch.Generator().manual_seed(seed)
    x = torch.empty(24, V)
    for r in range(24):
        counts = [c + (r % 3) * i for i, c in enumerate((2, 7, 15, 40, 70, 150))]
        rest = V - sum(counts)
        counts += [rest * 2 // 10, rest * 3 // 10, rest - rest * 2 // 10 - rest * 3 // 10]
        vals = torch.cat([torch.full((c,), v) for c, v in zip(counts, (6.0, 5.0, 4.0, 3.0, 2.0, 1.0, 0.0, -1.0, -2.0))])
        x[r] = vals[torch.randperm(V, generator=g)]
    return x.to(BF16)


TIE_CASES = [(1000, "odd", 1.0, 20, 0.6, 40, R.SEED_LO), (1000, "padded", 0.7, 50, 0.8, 41, R.SEED_HI),
             (64001, "padded", 1.0, 50, 0.5, 42, R.SEED_LO), (64001, "aligned", 2.0, 0, 0.6, 43, R.SEED_HI),
             (1000, "aligned", 1.0, 5, 1.0, 44, R.SEED_LO)]


@pytest.mark.parametrize("case", TIE_CASES, ids=lambda c: f"V{c[0]}-{c[1]}-T{c[2]}-k{c[3]}-p{c[4]}")
def test_bf16_rows_with_ties_at_both_boundaries(dev, case):
    V, kind, T, top_k, top_p, xseed, seed = case
    x = tie_rows(V, xseed)
    xd = x.double().numpy()
    # the test's own power: the k-th value is tied beyond k in every row, and the kept nucleus is neither one value nor all of K
    ties = 0
    for r in range(24):
        K, _, M = S.filtered(xd[r], T, top_k, top_p)
        if top_k:
            assert K.sum() > top_k, (r, K.sum())
        kept = np.unique(xd[r][K & (M < top_p)]).shape[0]
        ties += 1 < kept < np.unique(xd[r][K]).shape[0]
    assert ties >= 12 or top_p == 1.0, ties
    ids, _ = check(Rows(x, kind, dev), [500 + r for r in range(24)], seed, T, top_k, top_p, f"ties V {V} {kind} T {T} k {top_k} p {top_p}")
    assert len(set(ids.tolist())) > 6                   # draws spread over the tied columns


def minus_inf_rows(dtype):
    x = normal(24, 300, 2.0, dtype, 50)
    x[:, ::3] = float("-inf")
    x[5, :] = float("-inf")
    x[5, 17], x[5, 250] = 0.5, 1.5                      # two finite columns in all
    x[6, :] = float("-inf")
    x[6, 299] = -2.0                                    # one
    return x


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_minus_inf_columns_are_never_drawn(dev, dtype):
    x = minus_inf_rows(dtype)
    for T, top_k, top_p, seed in ((1.0, 0, 1.0, R.SEED_LO), (0.7, 250, 0.9, R.SEED_HI), (2.0, 0, 0.95, R.SEED_LO)):
        ids, logp = check(Rows(x, "odd" if dtype == F32 else "padded", dev), range(24), seed, T, top_k, top_p, f"-inf {dtype} T {T} k {top_k} p {top_p}")
        assert torch.isfinite(x[torch.arange(24), ids.long()].float()).all() and torch.isfinite(logp).all()
        assert ids[6].item() == 299 and ids[5].item() in (17, 250)


def test_row_independence_and_counters(dev):
    """the same (logits, ctr) as row 0 of one launch and as row 17 of another: the same bits; equal logits under 24 different
    counters: different draws somewhere"""
    V = 4099
    x = normal(24, V, 3.0, BF16, 60)
    one = x[3:4].expand(24, V).contiguous()
    for T, top_k, top_p in ((1.0, 0, 1.0), (0.7, 50, 0.9)):
        a = x.clone()
        b = normal(24, V, 3.0, BF16, 61)
        b[17] = a[0]
        ca, cb = [900 + r for r in range(24)], [77 + 5 * r for r in range(24)]
        cb[17] = ca[0]
        ra = launch(Rows(a, "padded", dev), ca, R.SEED_HI, T, top_k, top_p)
        rb = launch(Rows(b, "padded", dev), cb, R.SEED_HI, T, top_k, top_p)
        assert ra[0] == 0 and rb[0] == 0
        assert ra[1][0].item() == rb[1][17].item()
        assert ra[2][0:1].view(torch.int32).item() == rb[2][17:18].view(torch.int32).item()
        rc, ids, logp = launch(Rows(one, "padded", dev), ca, R.SEED_HI, T, top_k, top_p)
        assert rc == 0 and len(set(ids.tolist())) > 1, ids.tolist()
        same = launch(Rows(one, "padded", dev), [ca[0]] * 24, R.SEED_HI, T, top_k, top_p)
        assert len(set(same[1].tolist())) == 1          # one counter: one draw, whatever the row index


def test_two_launches_are_bit_identical(dev):
    for dtype, kind in ((BF16, "padded"), (F32, "odd")):
        rows = Rows(normal(24, 64001, 3.0, dtype, 70), kind, dev)
        a = launch(rows, range(24), R.SEED_LO, 0.7, 50, 0.9)
        b = launch(rows, range(24), R.SEED_LO, 0.7, 50, 0.9)
        assert a[0] == 0 and torch.equal(a[1], b[1]) and torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))


def test_argument_errors_come_back_without_a_launch(dev):
    from fcmf_framework import _hip as H
    rows = Rows(normal(3, 40, 2.0, F32, 80), "aligned", dev)
    ok = dict(ctr=[0, 1, 2], seed=1, T=1.0, top_k=0, top_p=1.0)
    untouched = lambda r: r[1].tolist() == [-1] * 3 and torch.isnan(r[2]).all()
    for change, code in ((dict(T=0.0), H.ERR_ARG), (dict(T=-1.0), H.ERR_ARG), (dict(T=float("inf")), H.ERR_ARG),
                         (dict(T=float("nan")), H.ERR_ARG), (dict(top_k=-1), H.ERR_ARG), (dict(top_p=0.0), H.ERR_ARG),
                         (dict(top_p=1.5), H.ERR_ARG), (dict(top_p=float("nan")), H.ERR_ARG), (dict(n=-1), H.ERR_ARG),
                         (dict(ld=39), H.ERR_ARG), (dict(V=0), H.ERR_UNSUPPORTED), (dict(V=(1 << 20) + 1, ld=1 << 21), H.ERR_UNSUPPORTED),
                         (dict(dtype_code=H.F64), H.ERR_UNSUPPORTED)):
        r = launch(rows, **{**ok, **change})
        assert r[0] == code and untouched(r), (change, r[0])
    r = launch(rows, **{**ok, "n": 0})
    assert r[0] == 0 and untouched(r)                   # rows = 0: nothing to do, nothing written
    c = torch.zeros(3, dtype=torch.int64, device=dev)
    out = torch.zeros(3, dtype=torch.int32, device=dev), torch.zeros(3, device=dev)
    for args in ((0, c.data_ptr(), out[0].data_ptr(), out[1].data_ptr()), (rows.view.data_ptr(), 0, out[0].data_ptr(), out[1].data_ptr()),
                 (rows.view.data_ptr(), c.data_ptr(), 0, out[1].data_ptr()), (rows.view.data_ptr(), c.data_ptr(), out[0].data_ptr(), 0)):
        assert H.lib().fcmf_sample_token(args[0], 40, 3, 40, 1.0, 0, 1.0, 1, args[1], args[2], args[3], H.F32, H.stream()) == H.ERR_ARG


def test_ops_sample_token_reads_strided_rows_and_checks_its_arguments(dev):
    from fcmf_framework import _hip as H, ops
    assert ops.SAMPLE_MAX_V == 1 << 20
    x = normal(6, 1000, 3.0, F32, 90)
    rows = Rows(x, "padded", dev)
    buf2d = torch.as_strided(rows.view, (6, rows.ld), (rows.ld, 1))
    ctr = torch.arange(6, device=dev) + 40
    want_ids, want_logp = reference(x, ctr.tolist(), R.SEED_HI, 0.7, 50, 0.9, "ops.sample_token")
    ids, logp = ops.sample_token(buf2d, 1000, ctr, R.SEED_HI, temperature=0.7, top_k=50, top_p=0.9)
    assert ids.dtype == torch.int32 and ids.shape == (6,) and logp.dtype == torch.float32 and logp.shape == (6,)
    assert ids.cpu().tolist() == want_ids.tolist() and np.abs(logp.cpu().double().numpy() - want_logp).max() < TOL
    with pytest.raises(H.HipLibraryError, match="overlap"):
        ops.sample_token(x[:1].to(dev).expand(3, 1000), 1000, ctr[:3], 1)
    with pytest.raises(H.HipLibraryError, match="counter"):
        ops.sample_token(buf2d, 1000, ctr[:5], 1)
    with pytest.raises(ValueError, match="top_p"):
        ops.sample_token(buf2d, 1000, ctr, 1, top_p=0.0)
    with pytest.raises(ValueError, match="temperature"):
        ops.sample_token(buf2d, 1000, ctr, 1, temperature=0.0)
