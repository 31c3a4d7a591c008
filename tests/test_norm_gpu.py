"""fcmf_add_ln_fwd / fcmf_add_ln_bwd (csrc/norm.hip) through the C ABI against the float64 references of rowwise_ref.py: every
pass count NP with full and ragged last passes, row tails, the multi-row walk of a wave (software pipeline, z in place), residual
strides, dropout against the numpy mask, and the column sums (workspace and atomics paths, pre-filled destinations).

Bounds (derived in the issue that asked for these tests, not tuned): float32 y/z rel_err < 2e-5, dz/dx < 4e-5; mean within
1e-5 max|z_row|, rstd relative 1e-5; bf16 outputs elementwise within 2^-8 |ref| + 4e-5 max|ref| (one bf16 rounding, doubled, plus
the float32 bound); column sums per column within 1e-5 sum_rows |term| (workspace path, longest chain of additions ~48) and
2e-5 (atomics path, 517 rows, ~133).

Measured worst error / bound per family, one MI355X run of this file:

    family                      worst err/bound
    f32 y, z (rel_err)          0.006
    f32 dz, dx (rel_err)        0.004
    mean                        0.008
    rstd                        0.015
    offset-1000 y               0.020
    bf16 y, z, dz, dx           0.983   (2^-8 is exactly the unit roundoff of bf16: a value just above a power of two meets it)
    column sums, workspace      0.021
    column sums, atomics        0.007

The table is printed again at the end of every run of this module (pytest -s).
"""
import pytest
import torch

import rowwise_ref as R

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nworst measured error / bound per family (test_norm_gpu):")
    for k in sorted(WORST):
        print(f"    {k:28s} {WORST[k]:.3f}")


def _lib():
    from fcmf_framework import _hip as H
    return H.lib(), H


def _note(family, err, bound):
    """record err / bound for the table, then hold the bound"""
    ratio = float(err) / float(bound) if bound > 0 else (0.0 if err == 0 else float("inf"))
    WORST[family] = max(WORST.get(family, 0.0), ratio)
    assert ratio <= 1.0, f"{family}: error {float(err):.3e} exceeds the bound {float(bound):.3e}"


def _randn(shape, seed, dtype=F32, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale + shift).to(dtype)


def _params(H_, seed=3):
    return 1 + 0.1 * _randn((H_,), seed), _randn((H_,), seed + 1)


def _close(family, got, ref, dtype, f32_tol):
    """float32: the project's rel_err bound; bf16: elementwise, one rounding (doubled) + the float32 bound"""
    got, ref = got.double().cpu(), ref.double()
    assert torch.isfinite(got).all()
    mx = ref.abs().max().item() + 1e-300
    if dtype == F32:
        _note(f"f32 {family} (rel_err)", (got - ref).abs().max().item() / mx, f32_tol)
    else:
        excess = ((got - ref).abs() / (2.0 ** -8 * ref.abs() + 4e-5 * mx)).max().item()
        _note("bf16 y, z, dz, dx", excess, 1.0)


def _residual(kind, rows, H_, dtype, dev, seed=11):
    """-> (device tensor handed to the kernel or None, its row stride, the float64 [rows, H] it stands for)"""
    if kind == "none":
        return None, 0, torch.zeros(rows, H_, dtype=torch.float64)
    if kind == "contig":
        r = _randn((rows, H_), seed, dtype).to(dev)
        return r, H_, r.double().cpu()
    if kind == "stride3H":                     # a column block of a wider buffer
        big = _randn((rows, 3 * H_), seed, dtype).to(dev)
        r = big[:, H_:2 * H_]
        return r, 3 * H_, r.double().cpu()
    assert kind == "stride0"                   # one row broadcast over all rows
    r = _randn((1, H_), seed, dtype).to(dev)
    return r, 0, r.double().cpu().expand(rows, H_)


def _fwd(dev, x, res, res_stride, gamma, beta, eps, p=0.0, seed=0, zmode="separate"):
    """one fcmf_add_ln_fwd call with guarded outputs -> y, z (None for zmode 'null'), mean, rstd on the CPU"""
    L, H = _lib()
    rows, H_ = x.shape
    dtype = x.dtype
    xg = R.guarded((rows, H_), dtype, dev)     # (guarded too: with z in place the kernel writes it)
    xg.view.copy_(x)
    y = R.guarded((rows, H_), dtype, dev)
    zg = R.guarded((rows, H_), dtype, dev) if zmode == "separate" else None
    mean, rstd = R.guarded((rows,), F32, dev), R.guarded((rows,), F32, dev)
    zp = {"separate": lambda: H.ptr(zg.view), "inplace": lambda: H.ptr(xg.view), "null": lambda: 0}[zmode]()
    g, b = gamma.to(dev), beta.to(dev)
    rc = L.fcmf_add_ln_fwd(H.ptr(xg.view), H.ptr(res), res_stride, H.ptr(g), H.ptr(b), H.ptr(y.view), zp, H.ptr(mean.view),
                           H.ptr(rstd.view), rows, H_, eps, p, seed, H.dt(x), H.stream())
    assert rc == 0
    torch.cuda.synchronize()
    R.check_all(xg, y, zg, mean, rstd)
    z = None if zmode == "null" else (zg.view if zmode == "separate" else xg.view).cpu()
    if zmode != "inplace":
        assert torch.equal(xg.view.cpu(), x.cpu())           # the input is read only
    return y.view.cpu(), z, mean.view.cpu(), rstd.view.cpu()


def _check_fwd(x, res64, gamma, beta, eps, y, z, mean, rstd, mask=None, p=0.0):
    dtype = x.dtype
    zr = x.double().cpu()
    if mask is not None:
        zr = zr * mask * R.inv_keep(p)
    zr = zr + res64
    yr, mr, rr = R.ln_fwd(zr, gamma, beta, eps)
    _close("y, z", y, yr, dtype, 2e-5)
    if z is not None:
        _close("y, z", z, zr, dtype, 2e-5)
    _note("mean", ((mean.double() - mr).abs() / (1e-5 * zr.abs().max(-1).values + 1e-300)).max().item(), 1.0)
    _note("rstd", ((rstd.double() - rr).abs() / rr).max().item(), 1e-5)
    return zr


def _bwd(dev, dy, z, gamma, eps, p=0.0, seed=0, workspace=True, prefill=False, want_dxsum=True, want_dx=None):
    """one fcmf_add_ln_bwd call, driven with float64 statistics rounded to float32 -> dict of CPU results and references"""
    L, H = _lib()
    rows, H_ = z.shape
    dtype = z.dtype
    mean64, rstd64 = R.ln_stats(z.double(), eps)
    mean, rstd = mean64.float(), rstd64.float()
    dz = R.guarded((rows, H_), dtype, dev)
    want_dx = p > 0 if want_dx is None else want_dx
    dx = R.guarded((rows, H_), dtype, dev) if want_dx else None
    outs = {}
    for i, name in enumerate(("dgamma", "dbeta", "dxsum")):
        o = R.guarded((H_,), F32, dev)
        pre = _randn((H_,), 50 + i) if prefill else torch.zeros(H_)
        o.view.copy_(pre)
        outs[name] = (o, pre)
    ws = None
    if workspace:
        n = L.fcmf_add_ln_bwd_workspace(rows, H_)
        ws = R.guarded((n,), F32, dev)
        ws.view.fill_(float("nan"))            # every call rewrites what it reads (ops.ln_bwd): NaN must not reach a result
    dyd, zd, gd, md, rd = (t.to(dev) for t in (dy, z, gamma, mean, rstd))        # (held until the synchronize below)
    rc = L.fcmf_add_ln_bwd(H.ptr(dyd), H.ptr(zd), H.ptr(gd), H.ptr(md), H.ptr(rd), H.ptr(dz.view),
                           0 if dx is None else H.ptr(dx.view), H.ptr(outs["dgamma"][0].view), H.ptr(outs["dbeta"][0].view), H.ptr(outs["dxsum"][0].view) if want_dxsum else 0,
                           0 if ws is None else H.ptr(ws.view), rows, H_, p, seed, H.dt(z), H.stream())
    assert rc == 0
    torch.cuda.synchronize()
    R.check_all(dz, dx, ws, *(o for o, _ in outs.values()))
    dzr, tg, tb = R.ln_bwd(dy, z, gamma, mean, rstd)
    res = dict(dz=dz.view.cpu(), dx=None if dx is None else dx.view.cpu(), dz_ref=dzr, tg=tg, tb=tb)
    for name, (o, pre) in outs.items():
        res[name], res[name + "_pre"] = o.view.cpu(), pre
    return res


def _check_colsum(family, got, pre, terms, tol):
    """per column: |got - (prefill + sum)| <= tol * sum_rows |term|"""
    ref = pre.double() + terms.sum(0)
    assert torch.isfinite(got).all()
    _note(family, ((got.double() - ref).abs() / (terms.abs().sum(0) + 1e-300)).max().item(), tol)


def _check_bwd(r, dtype, family="column sums, workspace", tol=1e-5, mask=None, p=0.0, dxsum=True):
    _close("dz, dx", r["dz"], r["dz_ref"], dtype, 4e-5)
    dxr = r["dz_ref"] if mask is None else r["dz_ref"] * mask * R.inv_keep(p)
    if r["dx"] is not None:
        _close("dz, dx", r["dx"], dxr, dtype, 4e-5)
    _check_colsum(family, r["dgamma"], r["dgamma_pre"], r["tg"], tol)
    _check_colsum(family, r["dbeta"], r["dbeta_pre"], r["tb"], tol)
    if dxsum:
        _check_colsum(family, r["dxsum"], r["dxsum_pre"], dxr, tol)
    else:
        assert torch.equal(r["dxsum"], r["dxsum_pre"])       # dxsum = NULL: the buffer was not handed over and is untouched


# ---- pass counts and ragged passes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H_", [4, 36, 64, 260, 512, 768, 1028, 2048])
def test_every_pass_count_full_and_ragged(dev, dtype, H_):
    """NP = 1 (4, 36, 64), 2 (260, 512), 3 (768), 8 (1028: most passes empty; 2048: all full); 37 rows: three idle waves"""
    rows = 37
    x, dy = _randn((rows, H_), 1, dtype), _randn((rows, H_), 2, dtype)
    gamma, beta = _params(H_)
    res, ld, res64 = _residual("contig", rows, H_, dtype, dev)
    y, z, mean, rstd = _fwd(dev, x.to(dev), res, ld, gamma, beta, 1e-12)
    _check_fwd(x, res64, gamma, beta, 1e-12, y, z, mean, rstd)
    _check_bwd(_bwd(dev, dy, z, gamma, 1e-12), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows", [1, 3, 4, 5])
def test_row_tails(dev, dtype, rows):
    H_ = 64
    x, dy = _randn((rows, H_), 5, dtype), _randn((rows, H_), 6, dtype)
    gamma, beta = _params(H_)
    y, z, mean, rstd = _fwd(dev, x.to(dev), None, 0, gamma, beta, 1e-5)
    _check_fwd(x, 0.0, gamma, beta, 1e-5, y, z, mean, rstd)
    _check_bwd(_bwd(dev, dy, z, gamma, 1e-5), dtype)


# ---- the multi-row walk -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,H_", [(8197, 64), (4101, 260)])
def test_multi_row_walk_and_z_in_place(dev, dtype, rows, H_):
    """8197 rows: the forward's grid is capped at 2048 workgroups, so 5 waves walk to a second row with the next row's loads
    issued before the current row's stores; the backward (1024 workgroups) gives every wave 2 or 3 rows.  4101 x 260: NP = 2,
    second rows in the backward only.  z separate / z == x in place / z NULL must give the same bits."""
    x, dy = _randn((rows, H_), 7, dtype), _randn((rows, H_), 8, dtype)
    gamma, beta = _params(H_)
    res, ld, res64 = _residual("contig", rows, H_, dtype, dev)
    xd = x.to(dev)
    y, z, mean, rstd = _fwd(dev, xd, res, ld, gamma, beta, 1e-12)
    _check_fwd(x, res64, gamma, beta, 1e-12, y, z, mean, rstd)
    for zmode in ("inplace", "null"):
        y2, z2, mean2, rstd2 = _fwd(dev, xd, res, ld, gamma, beta, 1e-12, zmode=zmode)
        assert torch.equal(y2.view(torch.uint8), y.view(torch.uint8)), zmode
        assert torch.equal(mean2, mean) and torch.equal(rstd2, rstd), zmode
        assert z2 is None or torch.equal(z2.view(torch.uint8), z.view(torch.uint8))
    # column sums through the workspace (NaN-filled) into pre-filled destinations: the kernels ADD
    _check_bwd(_bwd(dev, dy, z, gamma, 1e-12, prefill=True), dtype)
    r = _bwd(dev, dy, z, gamma, 1e-12, prefill=True, want_dxsum=False)
    _check_bwd(r, dtype, dxsum=False)


# ---- residual layouts, eps --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("eps", [1e-12, 1e-5])
@pytest.mark.parametrize("kind", ["none", "contig", "stride3H", "stride0"])
def test_residual_layouts(dev, dtype, kind, eps):
    rows, H_ = 37, 260
    x = _randn((rows, H_), 9, dtype)
    gamma, beta = _params(H_)
    res, ld, res64 = _residual(kind, rows, H_, dtype, dev)
    y, z, mean, rstd = _fwd(dev, x.to(dev), res, ld, gamma, beta, eps)
    _check_fwd(x, res64, gamma, beta, eps, y, z, mean, rstd)


@pytest.mark.parametrize("H_", [64, 768])
def test_rows_offset_by_1000_need_a_two_pass_variance(dev, H_):
    """std 1 around 1000: E[z^2] - E[z]^2 in float32 would be wrong by ~10 %.  Bound: the float32 mean's error (about 16 ulp
    of max|z| for a lane-then-butterfly sum = 4e-6 max|z| with margin) scaled by rstd * gamma."""
    rows = 37
    x, dy = _randn((rows, H_), 12, shift=1000.0), _randn((rows, H_), 13)
    gamma, beta = _params(H_)
    y, z, mean, rstd = _fwd(dev, x.to(dev), None, 0, gamma, beta, 1e-12)
    yr, mr, rr = R.ln_fwd(x, gamma, beta, 1e-12)
    bound = 4e-6 * x.double().abs().max(-1).values * rr * gamma.abs().max().item()
    _note("offset-1000 y", ((y.double() - yr).abs().max(-1).values / bound).max().item(), 1.0)
    _note("mean", ((mean.double() - mr).abs() / (1e-5 * x.double().abs().max(-1).values)).max().item(), 1.0)
    _note("rstd", ((rstd.double() - rr).abs() / rr).max().item(), 1e-5)
    assert torch.equal(z, x)


@pytest.mark.parametrize("dtype", DTYPES)
def test_all_zero_row(dev, dtype):
    rows, H_ = 5, 260
    x, dy = _randn((rows, H_), 14, dtype), _randn((rows, H_), 15, dtype)
    x[2] = 0
    gamma, beta = _params(H_)
    y, z, mean, rstd = _fwd(dev, x.to(dev), None, 0, gamma, beta, 1e-12)
    _check_fwd(x, 0.0, gamma, beta, 1e-12, y, z, mean, rstd)
    assert torch.equal(y[2], beta.to(dtype))                 # (0 - 0) * rstd * gamma + beta, exactly
    assert mean[2].item() == 0.0 and torch.isfinite(rstd).all() and abs(rstd[2].item() - 1e6) < 10.0
    r = _bwd(dev, dy, z, gamma, 1e-12)
    assert all(torch.isfinite(r[k]).all() for k in ("dz", "dgamma", "dbeta", "dxsum"))
    # The zero row has rstd = 1e6: its dz = rstd * (g - mean(g)) carries the float32 error of mean(g), ~1e-7, a million times
    # over, which no bound relative to the result covers in a column where g is close to its mean.  So that row (and dxsum,
    # which it dominates) is held to "finite"; the other rows and the two sums it enters with exact terms (xhat = 0) to the bounds.
    keep = [0, 1, 3, 4]
    _close("dz, dx", r["dz"][keep], r["dz_ref"][keep], dtype, 4e-5)
    _check_colsum("column sums, workspace", r["dgamma"], r["dgamma_pre"], r["tg"], 1e-5)
    _check_colsum("column sums, workspace", r["dbeta"], r["dbeta_pre"], r["tb"], 1e-5)
    assert bool((r["tg"][2] == 0).all())


# ---- dropout inside the LayerNorm -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("p,seed", [(0.1, R.SEED_LO), (0.25, R.SEED_HI), (0.1, R.SEED_HI), (0.25, R.SEED_LO)])
@pytest.mark.parametrize("rows,H_", [(8197, 64), (37, 260)])
def test_dropout_forward_matches_the_numpy_mask(dev, dtype, rows, H_, p, seed, with_res):
    """z = x * m / (1 - p) + res with m = dropout_mask at index row * H + c (37 x 260: row * H is no multiple of 256)"""
    x = _randn((rows, H_), 16, dtype)
    gamma, beta = _params(H_)
    res, ld, res64 = _residual("contig" if with_res else "none", rows, H_, dtype, dev)
    m = R.mask_tensor(seed, (rows, H_), p)
    y, z, mean, rstd = _fwd(dev, x.to(dev), res, ld, gamma, beta, 1e-5, p=p, seed=seed)
    if not with_res:
        assert torch.equal(z != 0, m.bool())                 # exactly the elements of the specification are dropped
    _check_fwd(x, res64, gamma, beta, 1e-5, y, z, mean, rstd, mask=m, p=p)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("p,seed", [(0.1, R.SEED_HI), (0.25, R.SEED_LO)])
@pytest.mark.parametrize("rows,H_", [(8197, 64), (37, 260)])
def test_dropout_backward_masks_dx_and_sums_it(dev, dtype, rows, H_, p, seed):
    """dx = dz * m / (1 - p) elementwise, dz itself (the residual's gradient) unmasked, dxsum = column sums of dx as computed
    in float32, before it is rounded to the storage type"""
    z, dy = _randn((rows, H_), 17, dtype), _randn((rows, H_), 18, dtype)
    gamma, _ = _params(H_)
    m = R.mask_tensor(seed, (rows, H_), p)
    r = _bwd(dev, dy, z, gamma, 1e-5, p=p, seed=seed, prefill=True)
    assert torch.equal(r["dx"] != 0, m.bool() & (r["dz"] != 0))
    if dtype == F32:
        assert torch.equal(r["dx"], r["dz"] * (m.float() * R.inv_keep(p)))      # one float32 multiply by float32(1 / (1 - p))
    _check_bwd(r, dtype, mask=m, p=p)


def test_dropout_backward_without_dx_is_refused(dev):
    L, H = _lib()
    rows, H_ = 5, 64
    t = torch.zeros(rows, H_, device=dev)
    v = torch.ones(rows, device=dev)
    g = torch.ones(H_, device=dev)
    dg, db = R.guarded((H_,), F32, dev), R.guarded((H_,), F32, dev)
    dz = R.guarded((rows, H_), F32, dev)
    rc = L.fcmf_add_ln_bwd(H.ptr(t), H.ptr(t), H.ptr(g), H.ptr(v), H.ptr(v), H.ptr(dz.view), 0, H.ptr(dg.view), H.ptr(db.view), 0, 0,
                           rows, H_, 0.1, 7, H.F32, H.stream())
    assert rc == -1
    torch.cuda.synchronize()
    R.check_all(dg, db, dz)
    assert bool((dz.view == 12345.0).all())                  # refused before any launch


# ---- column sums without a workspace ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("p", [0.0, 0.25])
def test_column_sums_atomics_path(dev, dtype, p):
    """workspace = NULL: 130 workgroups add their sums with float atomics into pre-filled destinations (H = 1028: NP = 8)"""
    rows, H_ = 517, 1028
    z, dy = _randn((rows, H_), 19, dtype), _randn((rows, H_), 20, dtype)
    gamma, _ = _params(H_)
    m = R.mask_tensor(R.SEED_HI, (rows, H_), p) if p > 0 else None
    r = _bwd(dev, dy, z, gamma, 1e-12, p=p, seed=R.SEED_HI, workspace=False, prefill=True)
    _check_bwd(r, dtype, family="column sums, atomics", tol=2e-5, mask=m, p=p)
    r = _bwd(dev, dy, z, gamma, 1e-12, p=p, seed=R.SEED_HI, workspace=False, prefill=True, want_dxsum=False)
    _check_bwd(r, dtype, family="column sums, atomics", tol=2e-5, mask=m, p=p, dxsum=False)


# ---- arguments the host refuses before any launch ---------------------------------------------------------------------------
def test_refusals_and_empty_input(dev):
    L, H = _lib()
    st = H.stream()
    buf = torch.zeros(8 * 2052, device=dev)
    vec = torch.ones(2052, device=dev)
    y, mean, rstd = R.guarded((8 * 2052,), F32, dev), R.guarded((8,), F32, dev), R.guarded((8,), F32, dev)
    dg, db = R.guarded((2052,), F32, dev), R.guarded((2052,), F32, dev)

    def fwd(rows, H_, res=None, ld=0):
        return L.fcmf_add_ln_fwd(H.ptr(buf), H.ptr(res), ld, H.ptr(vec), H.ptr(vec), H.ptr(y.view), 0, H.ptr(mean.view),
                                 H.ptr(rstd.view), rows, H_, 1e-5, 0.0, 0, H.F32, st)

    def bwd(rows, H_):
        return L.fcmf_add_ln_bwd(H.ptr(buf), H.ptr(buf), H.ptr(vec), H.ptr(vec), H.ptr(vec), H.ptr(y.view), 0, H.ptr(dg.view),
                                 H.ptr(db.view), 0, 0, rows, H_, 0.0, 0, H.F32, st)

    assert fwd(8, 6) == H.ERR_UNSUPPORTED and bwd(8, 6) == H.ERR_UNSUPPORTED            # H % 4
    assert fwd(8, 2052) == H.ERR_UNSUPPORTED and bwd(8, 2052) == H.ERR_UNSUPPORTED      # more than 8 passes
    assert fwd(8, 64, res=buf, ld=3) == H.ERR_UNSUPPORTED                               # residual rows not 16-byte aligned
    assert fwd(-1, 64) == -1 and bwd(-1, 64) == -1
    assert fwd(0, 64) == 0 and bwd(0, 64) == 0                                          # nothing to do, nothing written
    torch.cuda.synchronize()
    R.check_all(y, mean, rstd, dg, db)
    for g in (y, mean, rstd, dg, db):
        assert bool((g.view == 12345.0).all())
