"""The forward streaming kernels of the ResNet trunk (csrc/conv.hip), each through its C entry point, against the float64 references
of tests/trunk_ref.py: patch matrix (im2col_kernel, im2col_nhwc8_kernel), stem packing (pack_rgb0_kernel), grouped BatchNorm
(bn_stats_kernel, bn_reduce_chunks_kernel, bn_reduce_blocks_kernel, bn_finalize_kernel, bn_apply_kernel, bn_finalize_apply_kernel)
and the pools (maxpool3x3s2_kernel, avgpool_kernel).  The forward counterpart of test_resnet_bwd_gpu.py, to the standard of
test_gemm_exact_gpu.py: the kernels move data, take maxima or do arithmetic that is exact on the dyadic inputs of trunk_ref, so
every case of test_trunk_kernels_cpu.CASES asserts the return code and torch.equal(output, reference cast to the output's dtype).

Every output lives in a sentinel-filled guarded buffer whose frames are checked after the call (none of these entry points takes a
leading dimension); padded outputs (fcmf_pack_rgb0, fcmf_bn_apply_pad, fcmf_bn_finalize_apply with pad = 1) must leave their
border and their spare columns holding the sentinel; a refused call must leave everything holding it.  Inputs lie in NaN-poisoned
allocations: padded rows where the entry point takes strides (fcmf_conv_im2col, fcmf_pack_rgb0), NaN frames around contiguous
tensors.  The statistics workspace is allocated at exactly fcmf_bn_stats_workspace() doubles and pre-filled with the sentinel, and
the totals are read (or planted) at its last groups * C * 2 doubles, where fcmf_bn_finalize looks for them.

Bounded, each bound derived and none measured (the largest error / bound of every bounded case is printed):
  running statistics after training: double -> float, then one float EMA of three roundings per group:
      |got - f64| <= (2 + 3 groups) 2^-24 max(|running mean|, |running var|, |means|, |unbiased variances|) per channel;
  average pool where the window size is no power of two: one correctly rounded float division of an exact sum,
      |got - f64| <= 2^-24 |f64| (windows of 1, 2 or 4 elements are held to equality);
  one realistic BatchNorm per dtype (normal data, eps = 1e-5): |y - f64| <= 8 * 2^-24 (|x scale| + |shift| + |res|), + 2^-8 |f64| in bf16,
      f64 being x * scale + shift + res evaluated in float64 on what the apply kernel is handed: x, res and the finalize kernel's
      float32 scale and shift (against the float64 scale and shift the bound cannot hold -- shift = beta - mean * scale cancels, and
      the rounding of mean * scale does not shrink with it: the first run measured 1.30 of the bound that way); those two are
      bounded on their own, |scale - f64| <= 4 * 2^-24 |f64| and |shift - f64| <= 2^-24 |f64| + 6 * 2^-24 |mean scale|;
  the variance clamp (a channel of constant 0.1 over 1000 rows, eps = 1e-3): a thread's float partial covers <= 1024 values, so sum
      and sum of squares are off by <= 1024 * 2^-24 relative, the variance by <= 2 * 0.01 * 6.2e-5 < 0.2 % of eps:
      rstd is finite and |rstd - eps^-1/2| <= 1e-3 eps^-1/2.

The 4096-row cap of bn_chunking needs groups * rows_per_group > 2^22 / (channel slabs): 2^28 elements at C = 64 and 2^30 at C >= 256,
which no test of the suite reaches (the full-depth trunk of test_resnet_gpu.py runs in eval mode, without batch statistics).  At
C = 4 it is 2^24 elements, and one bf16 case (stats-chunk-cap-c4-g1r4194306-bf16, 34 MB) reaches it here.

Measured on an MI355X (462 tests, 3.7 s in all; the slowest are the grid-stride cases: max pool 0.69 s, BatchNorm apply 0.35 s, the
chunk-cap statistics 0.28 s, average pool 0.22 s, the first call of the process 0.29 s; every other test at most 0.1 s): every
equality holds and every guard frame, border and refused buffer is intact.  Largest error / bound: running mean 0.21, running
variance 0.27 (0 to 0.11 on the dyadic cases); average pool 0.87 (7 x 7 -> 1 x 1) and 0.79 (13 x 16 -> 3 x 5); realistic BatchNorm
y 0.22 (float32) and 0.996 (bf16: half an ulp just above 8), both paths alike, its scale 0.62 and shift 0.97; variance clamp:
rstd 31.62277 in both dtypes and paths against 31.62278, 4e-4 of the bound.
Found: fcmf_conv_im2col accepted a kernel larger than the padded input when (H + 2 pad - kh) / stride truncated to 0 (stride 2,
H + 2 pad = kh - 1) and wrote a patch row for an output that does not exist: it now returns FCMF_ERR_ARG
(im2col-refuse-no-output-s2).  fcmf_pack_rgb0 rounds a float64 source ONCE to bf16, not through float32 as its source line
read: the compiler had folded the two casts; source, header and reference now say what runs.  The statistics do not depend on
the workspace's prior contents (sentinel-filled here): the kernel comment that asked for a zeroed workspace was stale.
"""
import pytest
import torch

import trunk_ref as TR
from test_trunk_kernels_cpu import BY_ID, CASES, DT, ES, OF, reference

pytestmark = pytest.mark.gpu

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
U24 = 2.0 ** -24


def _H():
    from fcmf_framework import _hip
    return _hip


def _code(name):
    H = _H()
    return {"f32": H.F32, "bf16": H.BF16, "f64": H.F64}[name]


def _equal(got, want, dtype, what):
    want, got = want.cpu().to(dtype), got.cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    if not torch.equal(got, want):
        bad = (got != want) | (got != got)
        idx = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {idx}: "
                             f"{got[tuple(idx)].item()} against {want[tuple(idx)].item()}")


def _bounded(cid, what, got, ref, bound):
    err = (got.cpu().double() - ref).abs()
    live = bound > 0
    ratio = float((err[live] / bound[live]).max()) if bool(live.any()) else 0.0
    print(f"{cid}: {what}: largest error {float(err.max()):.3e}, largest error / bound {ratio:.3f}")
    assert bool(torch.isfinite(got).all()), f"{what}: not finite"
    assert bool((err <= bound).all()), f"{what}: {int((err > bound).sum())} elements above the bound, worst at {ratio:.3f} of it"


def _untouched(g, what):
    g.check()
    assert bool((g.view == TR._SENTINEL[g.buf.dtype]).all()), f"{what}: written by a call that was refused"


class In:
    """a contiguous input between NaN frames, optionally `shift` elements behind a 16-byte boundary"""

    def __init__(self, t, dev, shift=0):
        flat = t.reshape(-1)
        if shift:
            flat = torch.cat([torch.full((shift,), float("nan"), dtype=t.dtype), flat])
        self.p = TR.poisoned(flat, flat.numel(), 0, dev)
        self.ptr = self.p.data_ptr() + shift * t.element_size()
        self.live = self.p.view.reshape(-1)[shift:].view(t.shape)


def _filled(vals, dev):
    """a guarded float32 / float64 buffer holding `vals`"""
    g = TR.guarded(tuple(vals.shape), vals.dtype, dev)
    g.view.copy_(vals)
    return g


# ---- fcmf_conv_im2col -----------------------------------------------------------------------------------------------------------
def _im2col_source(c, x, dev):
    """-> (keep-alive, pointer, (sn, sh, sw, sc)): the logical x [N, H, W, C] in the case's layout, NaN wherever the tensor is not"""
    N, H, W, C = x.shape
    es = x.element_size()
    if c["layout"] == "nchw":          # rows of W elements with 5 NaN behind each
        ld = W + 5
        p = TR.poisoned(x.permute(0, 3, 1, 2).reshape(N * C * H, W), ld, 2, dev)
        return p, p.data_ptr(), (C * H * ld, ld, 1, H * ld)
    if c["layout"] == "nhwc-sn":       # channels-last images 8 elements apart: sn is not H * W * C
        ld = H * W * C + 8
        p = TR.poisoned(x.reshape(N, H * W * C), ld, 1, dev)
        return p, p.data_ptr(), (ld, W * C, C, 1)
    s = In(x, dev, c["off"])
    assert (s.ptr % 16 == 0) == (c["off"] * es % 16 == 0)
    return s, s.ptr, (H * W * C, W * C, C, 1)


@pytest.mark.parametrize("cid", OF("im2col"))
def test_im2col(dev, cid):
    H = _H()
    c, r = BY_ID[cid], reference(cid)
    N, Hh, W, C, k = c["N"], c["H"], c["W"], c["C"], c["k"]
    keep, ptr, (sn, sh, sw, sc) = _im2col_source(c, r["x"].to(DT[c["src"]]), dev)
    rows = r["A"].shape[0] if not c["refuse"] else N * Hh * W
    out = TR.guarded((rows, max(r["Kpad"], r["K"])), DT[c["dst"]], dev)
    rc = H.lib().fcmf_conv_im2col(ptr, _code(c["src"]), out.view.data_ptr(), _code(c["dst"]), N, Hh, W, C, sn, sh, sw, sc, k, k, c["stride"],
                                  c["pad"], r["Kpad"], H.stream())
    torch.cuda.synchronize()
    if c["refuse"]:
        assert rc == H.ERR_ARG, rc
        _untouched(out, "patch matrix")
        return
    assert rc == 0, rc
    _equal(out.view, r["A"], DT[c["dst"]], "patch matrix")
    out.check()


# ---- fcmf_pack_rgb0 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", OF("pack"))
def test_pack_rgb0(dev, cid):
    H = _H()
    c, r = BY_ID[cid], reference(cid)
    N, Hh, W, pad, Wp = c["N"], c["H"], c["W"], c["pad"], r["Wp"]
    x = r["x"]
    if c["layout"] == "nhwc":
        src = In(x, dev)
        ptr, strides = src.ptr, (Hh * W * 3, W * 3, 3, 1)
    elif c["layout"] == "nchw":
        src = In(x.permute(0, 3, 1, 2).contiguous(), dev)
        ptr, strides = src.ptr, (3 * Hh * W, W, 1, Hh * W)
    else:          # a crop at (2, 3) of NCHW images of (H + 4) x (W + 6), NaN around it and between the rows
        Hb, Wb, ld = Hh + 4, W + 6, W + 6 + 2
        big = torch.full((N, 3, Hb, Wb), float("nan"), dtype=x.dtype)
        big[:, :, 2:2 + Hh, 3:3 + W] = x.permute(0, 3, 1, 2)
        src = TR.poisoned(big.reshape(N * 3 * Hb, Wb), ld, 1, dev)
        ptr, strides = src.data_ptr() + (2 * ld + 3) * x.element_size(), (3 * Hb * ld, ld, 1, Hb * ld)
    out = TR.guarded((N, Hh + 2 * pad, max(Wp, W + 2 * pad), 4), BF16, dev)          # holds the sentinel, not zero
    rc = H.lib().fcmf_pack_rgb0(ptr, _code(c["src"]), out.view.data_ptr(), N, Hh, W, *strides, pad, Wp, H.stream())
    torch.cuda.synchronize()
    if c["refuse"]:
        assert rc == H.ERR_ARG, rc
        _untouched(out, "packed input")
        return
    assert rc == 0, rc
    got, mask = out.view.cpu(), r["mask"]
    _equal(got[mask], r["vals"][mask], BF16, "interior pixels")
    assert bool((got[~mask] == TR._SENTINEL[BF16]).all()), "store into the border or the columns W + 2 pad .. Wp"
    out.check()


# ---- fcmf_bn_stats / fcmf_bn_stats_workspace ------------------------------------------------------------------------------------
def _workspace(H, c, dev):
    """-> (guarded workspace of exactly the size the library asks for, holding the sentinel; its totals [groups, C, 2] view)"""
    G, C = c["groups"], c["C"]
    n = H.lib().fcmf_bn_stats_workspace(c["rpg"], G, C)
    if TR.bn_stats_ok(C):
        assert n == TR.bn_workspace(c["rpg"], G, C), (n, TR.bn_workspace(c["rpg"], G, C))
    else:
        assert n == 0, n
        n = TR.bn_workspace(c["rpg"], G, C)
    ws = TR.guarded((n,), F64, dev)
    return ws, ws.view[n - G * C * 2:].view(G, C, 2)


@pytest.mark.parametrize("cid", OF("stats"))
def test_bn_stats(dev, cid):
    H = _H()
    c, r = BY_ID[cid], reference(cid)
    G, rpg, C = c["groups"], c["rpg"], c["C"]
    x = In(r["x"].to(DT[c["dt"]]), dev)
    ws, totals = _workspace(H, c, dev)
    rc = H.lib().fcmf_bn_stats(x.ptr, ws.view.data_ptr(), rpg, G, C, _code(c["dt"]), H.stream())
    torch.cuda.synchronize()
    if c["refuse"]:
        assert rc == H.ERR_ARG, rc
        _untouched(ws, "statistics workspace")
        return
    assert rc == 0, rc
    # the workspace held the sentinel, not zero: the kernels store, they do not accumulate
    _equal(totals, r["totals"], F64, "totals")
    chunks = TR.bn_chunks(rpg, G, C)[0]
    partials = ws.view[:G * chunks * C * 2].view(G, chunks, C, 2).cpu()
    assert not bool((partials == TR._SENTINEL[F64]).any()), "a chunk partial was not written"
    _equal(partials.sum(1), r["totals"], F64, "sum of the chunk partials")
    ws.check()


# ---- fcmf_bn_stats_blocks -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", OF("blocks"))
def test_bn_stats_blocks(dev, cid):
    H = _H()
    c, r = BY_ID[cid], reference(cid)
    G, C = c["groups"], c["C"]
    st = In(r["stats"].float(), dev)
    ws, totals = _workspace(H, c, dev)
    rc = H.lib().fcmf_bn_stats_blocks(st.ptr, ws.view.data_ptr(), c["rpg"], G, C, c["block_rows"], H.stream())
    torch.cuda.synchronize()
    if c["refuse"]:
        assert rc == (H.ERR_ARG if c["refuse"] == "arg" else H.ERR_UNSUPPORTED), rc
        _untouched(ws, "statistics workspace")
        return
    assert rc == 0, rc
    _equal(totals, r["totals"], F64, "totals")
    assert bool((ws.view[:ws.n - G * C * 2] == TR._SENTINEL[F64]).all()), "store in front of the totals"
    ws.check()


# ---- fcmf_bn_finalize + fcmf_bn_apply(_pad), fcmf_bn_finalize_apply -------------------------------------------------------------
class BN:
    """the device operands of one BatchNorm case; fresh outputs and running statistics for every path that is run on them"""

    def __init__(self, c, r, dev):
        H = _H()
        self.c, self.r, self.dev = c, r, dev
        dt = DT[c["dt"]]
        self.dt, self.G, self.C = dt, c["groups"], c["C"]
        self.rows = c["groups"] * c["rpg"]
        k = 8 // ES[c["dt"]]          # elements in 8 bytes
        self.k = {w: (k if c["misalign"] == w else 0) for w in ("x", "y", "res")}
        self.x = In(r["x"].to(dt), dev, self.k["x"])
        self.res = In(r["res"].to(dt), dev, self.k["res"]) if r["res"] is not None else None
        self.gamma, self.beta = In(r["gamma"].float(), dev), In(r["beta"].float(), dev)
        self.ws = None
        if c["train"]:
            self.ws, self.totals = _workspace(H, c, dev)
            if c["mode"] != "both":
                self.totals.copy_(r["totals"])          # planted where bn_totals() looks; the partials in front hold the sentinel
        self.SG = self.G if c["train"] else 1           # rows of scale / shift / mean / rstd

    def fresh(self):
        c, r, dev, C = self.c, self.r, self.dev, self.C
        self.rm, self.rv = _filled(r["rmean"].float(), dev), _filled(r["rvar"].float(), dev)
        self.scale, self.shift, self.mean, self.rstd = (TR.guarded((self.SG, C), F32, dev) for _ in range(4))
        if c["hw"]:
            Hh, W = c["hw"]
            self.y = TR.guarded((self.rows // (Hh * W), Hh + 2, W + 2, C), self.dt, dev)
        else:
            self.y = TR.guarded((self.rows * C + self.k["y"],), self.dt, dev)
        self.y_ptr = self.y.view.data_ptr() + self.k["y"] * ES[c["dt"]]
        self.x_ptr = self.x.ptr
        if c["alias"]:
            self.y.view.copy_(self.x.live.reshape(-1))
            self.x_ptr = self.y_ptr

    def args(self):
        H, c = _H(), self.c
        so = (self.mean.view.data_ptr(), self.rstd.view.data_ptr()) if c["stats_out"] else (None, None)
        return H, c, so, (None if self.res is None else self.res.ptr), (self.ws.view.data_ptr() if self.ws is not None else None)

    def separate(self, stats_out=None):
        H, c, so, res, ws = self.args()
        so = so if stats_out is None else stats_out
        L, st = H.lib(), H.stream()
        rc = L.fcmf_bn_finalize(ws, self.gamma.ptr, self.beta.ptr, self.rm.view.data_ptr(), self.rv.view.data_ptr(), self.scale.view.data_ptr(),
                                self.shift.view.data_ptr(), so[0], so[1], self.C, self.G, c["rpg"] if c["train"] else self.rows, c["mom"], c["eps"], st)
        if rc != 0:
            return rc
        common = (self.x_ptr, res, self.y_ptr, self.scale.view.data_ptr(), self.shift.view.data_ptr(), self.rows, self.C,
                  c["rpg"] if c["train"] else self.rows, c["relu"])
        if c["hw"]:
            return L.fcmf_bn_apply_pad(*common, c["hw"][0], c["hw"][1], 1, _code(c["dt"]), st)
        return L.fcmf_bn_apply(*common, _code(c["dt"]), st)

    def fused(self, stats_out=None):
        H, c, so, res, ws = self.args()
        so = so if stats_out is None else stats_out
        hw = c["hw"] or (1, 1)
        return H.lib().fcmf_bn_finalize_apply(self.x_ptr, res, self.y_ptr, ws, self.gamma.ptr, self.beta.ptr, self.rm.view.data_ptr(),
                                              self.rv.view.data_ptr(), so[0], so[1], self.C, self.G, c["rpg"] if c["train"] else self.rows, c["mom"],
                                              c["eps"], c["relu"], hw[0], hw[1], 1 if c["hw"] else 0, _code(c["dt"]), H.stream())

    def y_live(self):
        """-> (the rows the kernel should have written [rows, C], everything else of the output buffer)"""
        c = self.c
        if c["hw"]:
            flat = self.y.view.reshape(-1, self.C).cpu()
            idx = TR.pad_rows(self.rows // (c["hw"][0] * c["hw"][1]), c["hw"][0], c["hw"][1], 1)
            rest = torch.ones(flat.shape[0], dtype=torch.bool)
            rest[idx] = False
            return flat[idx], flat[rest]
        v = self.y.view.cpu()
        return v[self.k["y"]:].view(self.rows, self.C), v[:self.k["y"]]

    def guards(self):
        TR.check_all(self.rm, self.rv, self.scale, self.shift, self.mean, self.rstd, self.y, self.ws)

    def nothing_written(self):
        for g, what in ((self.y, "y"), (self.scale, "scale"), (self.shift, "shift"), (self.mean, "mean"), (self.rstd, "rstd")):
            if not (g is self.y and self.c["alias"]):
                _untouched(g, what)
        _equal(self.rm.view, self.r["rmean"], F32, "running mean of a refused call")
        _equal(self.rv.view, self.r["rvar"], F32, "running variance of a refused call")

    def check_running(self, cid):
        c, r = self.c, self.r
        if not c["train"]:
            _equal(self.rm.view, r["rmean"], F32, "running mean (eval: unchanged)")
            _equal(self.rv.view, r["rvar"], F32, "running variance (eval: unchanged)")
            return
        bound = (2 + 3 * self.G) * U24 * r["f_terms"]
        _bounded(cid, "running mean", self.rm.view, r["f_rmean"], bound)
        _bounded(cid, "running variance", self.rv.view, r["f_rvar"], bound)

    def check_exact(self, cid, fused):
        c, r = self.c, self.r
        sg = (self.SG, self.C)
        if not fused:
            _equal(self.scale.view, r["f_scale"].reshape(sg), F32, "scale")
            _equal(self.shift.view, r["f_shift"].reshape(sg), F32, "shift")
        if c["stats_out"]:
            _equal(self.mean.view, r["f_mean"].reshape(sg), F32, "mean_out")
            _equal(self.rstd.view, r["f_rstd"].reshape(sg), F32, "rstd_out")
        else:
            _untouched(self.mean, "mean_out")
            _untouched(self.rstd, "rstd_out")
        live, rest = self.y_live()
        _equal(live, r["y"], self.dt, "y")
        assert bool((rest == TR._SENTINEL[self.dt]).all()), "store into the border of the padded output"
        self.check_running(cid)
        self.guards()


BN_OK = [c["id"] for c in CASES if c["fam"] == "bn" and c["expect"] == "ok" and c["kind"] == "dyadic"]


@pytest.mark.parametrize("cid", BN_OK)
def test_batchnorm_exact(dev, cid):
    c, r = BY_ID[cid], reference(cid)
    b = BN(c, r, dev)
    b.fresh()
    rc = b.fused() if c["mode"] == "fused" else b.separate()
    torch.cuda.synchronize()
    assert rc == 0, rc
    b.check_exact(cid, c["mode"] == "fused")
    if b.ws is not None:
        assert bool((b.ws.view[:b.ws.n - b.G * b.C * 2] == TR._SENTINEL[F64]).all()), "store in front of the totals"


@pytest.mark.parametrize("cid", [c["id"] for c in CASES if c["fam"] == "bn" and c["expect"] == "unsupported"])
def test_fused_batchnorm_declines_and_the_separate_kernels_take_over(dev, cid):
    H = _H()
    c, r = BY_ID[cid], reference(cid)
    b = BN(c, r, dev)
    b.fresh()
    rc = b.fused()
    torch.cuda.synchronize()
    assert rc == H.ERR_UNSUPPORTED, rc
    b.nothing_written()
    rc = b.separate()          # the fall-back of resnet.batchnorm_nhwc_, on the same operands
    torch.cuda.synchronize()
    assert rc == 0, rc
    b.check_exact(cid, False)


def test_batchnorm_argument_errors(dev):
    H = _H()
    L = H.lib()
    c = BY_ID["bn-sep-refuse-one-null-c64-g3r30-f32"]
    b = BN(c, reference(c["id"]), dev)
    b.fresh()
    for so in ((b.mean.view.data_ptr(), None), (None, b.rstd.view.data_ptr())):          # mean_out and rstd_out: both or neither
        assert b.separate(stats_out=so) == H.ERR_ARG
        assert b.fused(stats_out=so) == H.ERR_ARG
    torch.cuda.synchronize()
    b.nothing_written()
    c = BY_ID["bn-sep-rows-0-c64-g3r30-f32"]
    b = BN(c, reference(c["id"]), dev)
    b.fresh()
    sc, sh = _filled(torch.ones(3, 64), dev), _filled(torch.ones(3, 64), dev)
    assert L.fcmf_bn_apply(b.x_ptr, None, b.y_ptr, sc.view.data_ptr(), sh.view.data_ptr(), 0, 64, 30, 1, H.F32, H.stream()) == 0
    torch.cuda.synchronize()
    _untouched(b.y, "y of a call with rows = 0")
    c = BY_ID["bn-sep-pad-refuse-rows-c64-g1r32-f32-pad3x5"]          # 32 rows are no whole number of 3 x 5 images
    b = BN(c, reference(c["id"]), dev)
    b.y = TR.guarded((3, 5, 7, 64), F32, dev)
    b.rm, b.rv = _filled(b.r["rmean"].float(), dev), _filled(b.r["rvar"].float(), dev)
    args = (b.x.ptr, None, b.y.view.data_ptr(), sc.view.data_ptr(), sh.view.data_ptr(), 32, 64, 32, 1, 3, 5, 1, H.F32, H.stream())
    assert L.fcmf_bn_apply_pad(*args) == H.ERR_ARG
    assert L.fcmf_bn_finalize_apply(b.x.ptr, None, b.y.view.data_ptr(), b.ws.view.data_ptr(), b.gamma.ptr, b.beta.ptr, b.rm.view.data_ptr(),
                                    b.rv.view.data_ptr(), None, None, 64, 1, 32, 0.25, 0.0, 1, 3, 5, 1, H.F32, H.stream()) == H.ERR_ARG
    torch.cuda.synchronize()
    _untouched(b.y, "padded y of a refused call")
    _equal(b.rm.view, b.r["rmean"], F32, "running mean of a refused call")


@pytest.mark.parametrize("cid", [c["id"] for c in CASES if c["fam"] == "bn" and c["mode"] == "both"])
def test_batchnorm_bounded(dev, cid):
    """statistics kernel -> separate kernels, and -> the fused kernel, on data that is not dyadic"""
    H = _H()
    c, r = BY_ID[cid], reference(cid)
    b = BN(c, r, dev)
    assert H.lib().fcmf_bn_stats(b.x.ptr, b.ws.view.data_ptr(), c["rpg"], b.G, b.C, _code(c["dt"]), H.stream()) == 0
    for fused in (False, True):
        b.fresh()
        rc = b.fused() if fused else b.separate()
        torch.cuda.synchronize()
        assert rc == 0, rc
        tag = "fused" if fused else "separate"
        rstd = b.rstd.view.cpu().double()
        assert bool(torch.isfinite(rstd).all())
        if c["kind"] == "constant":
            want = c["eps"] ** -0.5
            err = abs(float(rstd[0, 5]) - want)
            print(f"{cid}: {tag}: rstd of the constant channel {float(rstd[0, 5]):.6f} against {want:.6f}, error / bound {err / (1e-3 * want):.3f}")
            assert err <= 1e-3 * want
        else:
            if not fused:
                # scale = gamma / sqrt(var + eps): the casts of var and of the sum, sqrtf (which halves what came before), the division
                # and the product round once each: 4 * 2^-24 relative.  shift = beta - mean * scale: the cast of the mean, the
                # product and the error of scale act on |mean scale| (6 * 2^-24), the subtraction on |shift|.
                sc, sh = b.scale.view.cpu().double(), b.shift.view.cpu().double()
                _bounded(cid, "scale", sc, r["f_scale"], 4 * U24 * r["f_scale"].abs())
                _bounded(cid, "shift", sh, r["f_shift"], U24 * r["f_shift"].abs() + 6 * U24 * (r["f_mean"] * r["f_scale"]).abs())
            # y: the float64 value of x * scale + shift + res on what the apply kernel is handed -- x, res and the float32 scale and
            # shift of the finalize kernel (the fused kernel derives the same two with the same arithmetic)
            g = torch.arange(b.rows) // c["rpg"]
            want = TR.bn_apply_ref(r["x"], r["res"], sc, sh, c["rpg"], c["relu"])
            bound = 8 * U24 * ((r["x"] * sc[g]).abs() + sh[g].abs() + r["res"].abs())
            if c["dt"] == "bf16":
                bound = bound + 2.0 ** -8 * want.abs()
            _bounded(cid, f"{tag}: y", b.y_live()[0], want, bound)
        b.check_running(f"{cid}: {tag}")
        b.guards()


# ---- fcmf_maxpool3x3s2 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", OF("maxpool"))
def test_maxpool(dev, cid):
    H = _H()
    c, r = BY_ID[cid], reference(cid)
    dt = DT[c["dt"]]
    N, Hh, W, C = c["N"], c["H"], c["W"], c["C"]
    x = In(r["x"].to(dt), dev)
    y = TR.guarded((N, TR.conv_out(Hh, 3, 2, 1), TR.conv_out(W, 3, 2, 1), C), dt, dev)
    rc = H.lib().fcmf_maxpool3x3s2(x.ptr, y.view.data_ptr(), N, Hh, W, C, _code(c["dt"]), H.stream())
    torch.cuda.synchronize()
    if c["refuse"]:
        assert rc == H.ERR_ARG, rc
        _untouched(y, "pooled output")
        return
    assert rc == 0, rc
    _equal(y.view, r["y"], dt, "pooled output")
    y.check()


# ---- fcmf_adaptive_avgpool ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", OF("avgpool"))
def test_avgpool(dev, cid):
    H = _H()
    c, r = BY_ID[cid], reference(cid)
    N, Hh, W, C, oh, ow = c["N"], c["H"], c["W"], c["C"], c["oh"], c["ow"]
    x = In(r["x"].to(DT[c["dt"]]), dev)
    y = TR.guarded((N, C, oh, ow) if c["layout"] == 0 else (N, oh * ow, C), F32, dev)
    rc = H.lib().fcmf_adaptive_avgpool(x.ptr, y.view.data_ptr(), N, Hh, W, C, oh, ow, c["layout"], _code(c["dt"]), H.stream())
    torch.cuda.synchronize()
    if c["refuse"]:
        assert rc == H.ERR_ARG, rc
        _untouched(y, "pooled output")
        return
    assert rc == 0, rc
    exact = torch.from_numpy(TR.is_pow2(r["cnt"].numpy()))
    got = y.view.cpu()
    _equal(got[exact], r["y"][exact], F32, "windows of 1, 2 or 4 elements")
    if not bool(exact.all()):          # an exact window sum (test_trunk_kernels_cpu.py), one float division
        _bounded(cid, "windows of other sizes", got[~exact], r["y"][~exact], U24 * r["y"][~exact].abs())
    y.check()


def test_every_case_has_a_test():
    assert {c["fam"] for c in CASES} == {"im2col", "pack", "stats", "blocks", "bn", "maxpool", "avgpool"}
    assert {c["expect"] for c in CASES if c["fam"] == "bn"} == {"ok", "unsupported", "one-null", "rows0", "pad-rows"}
    assert {c["mode"] for c in CASES if c["fam"] == "bn" and c["kind"] != "dyadic"} == {"both"}
