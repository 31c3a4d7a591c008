"""The cases of test_trunk_kernels_gpu.py and, without a GPU, what its equalities rest on (tests/trunk_ref.py):

  * the references are right: im2col_ref against F.unfold permuted to the (r, s, c) column order, bn_finalize_ref + bn_apply_ref
    against F.batch_norm called once per group in training mode and once in eval mode (running statistics included), maxpool_ref
    against F.max_pool2d, avgpool_ref against F.adaptive_avg_pool2d, pack_rgb0_ref and pad_rows against index arithmetic -- at the
    shapes of the case table;
  * the builders deliver what they promise: the float64 mean, biased variance and rstd of every BatchNorm input are exactly the
    intended dyadic values, and every expected output survives the cast to the case's dtype;
  * the table claims every branch the kernels and their host wrappers have (BRANCHES), each case is routed where its id says
    (im2col_path restates the wrapper's choice), and no case allocates more than 128 MB on the device.

CASES lists every GPU case.  A case names the branch it exists for in its id and in `claims`.  These are conditions, not
measurements: if a seed breaks one, the seed changes, never the condition."""
import functools

import pytest
import torch
import torch.nn.functional as F

import trunk_ref as TR

DT = TR.DT
ES = {"f32": 4, "bf16": 2, "f64": 8}
CAP = TR.GRID_CAP
CASES = []


def case(fam, name, claims, **kw):
    c = dict(fam=fam, claims=tuple(claims), **kw)
    c["id"] = f"{fam}-{name}"
    c.setdefault("seed", 3000 + 13 * len(CASES))
    assert all(o["id"] != c["id"] for o in CASES), c["id"]
    CASES.append(c)


# ---- fcmf_conv_im2col -----------------------------------------------------------------------------------------------------------
def im2col(name, claims, C, k, stride, pad, N, H, W, kextra=0, src="f32", dst=None, layout="nhwc", off=0, path="fast", refuse=None):
    case("im2col", f"{name}-c{C}k{k}s{stride}p{pad}-n{N}h{H}w{W}-K+{kextra}-{src}>{dst or src}", claims, C=C, k=k, stride=stride, pad=pad, N=N,
         H=H, W=W, kextra=kextra, src=src, dst=dst or src, layout=layout, off=off, path=path, refuse=refuse)


for dt in ("f32", "bf16"):
    for C, k, s, p in ((8, 3, 1, 1), (64, 3, 2, 1), (16, 1, 2, 0), (8, 7, 2, 3)):
        for H, W in ((5, 7), (14, 15), (2, 3)) + (((1, 1),) if k == 3 else ()):
            for kextra in (0, 8):
                im2col("fast", ["im2col:fast"] + ["im2col:fast-tail-columns"] * (kextra > 0) + ["im2col:fast-1x1"] * (H == 1),
                       C, k, s, p, 3, H, W, kextra, src=dt)
    # the generic kernel, by each disqualifier of the fast path on its own
    im2col("generic-c12", ["im2col:generic-c%8"], 12, 3, 1, 1, 3, 5, 7, 4, src=dt, path="generic")
    im2col("generic-kpad+4", ["im2col:generic-kpad%8"], 8, 3, 1, 1, 3, 5, 7, 4, src=dt, path="generic")
    im2col("generic-src+8bytes", ["im2col:generic-misaligned"], 8, 3, 1, 1, 3, 5, 7, 0, src=dt, off=4 if dt == "bf16" else 2, path="generic")
    im2col("generic-padded-sn", ["im2col:generic-padded-sn"], 8, 3, 2, 1, 3, 5, 7, 8, src=dt, layout="nhwc-sn", path="generic")
    # the stem: NCHW float32 crops, K = 147 padded to 160
    im2col("generic-stem", ["im2col:generic-stem-nchw"], 3, 7, 2, 3, 3, 14, 15, 13, src="f32", dst=dt, layout="nchw", path="generic")
im2col("generic-bf16>f32", ["im2col:generic-dtype-change"], 8, 3, 1, 1, 3, 5, 7, 0, src="bf16", dst="f32", path="generic")
# grid-stride loops.  The fast kernel's item is an 8-channel piece: rows * Kpad / 8 = 18 * 57 * 57 * 72 = 4 210 704 items, 0.4 % above
# the cap of 16384 * 256 (two images of 57 x 57 stay far below it).  The generic kernel's item is a patch row per wave, four per
# workgroup: its loop wraps above 16384 * 4 = 65 536 rows; 2 * 183 * 183 = 66 978 rows, 2.2 % above.
im2col("gridstride-fast", ["im2col:grid-stride-fast"], 64, 3, 1, 1, 18, 57, 57, 0, src="bf16")
im2col("gridstride-generic", ["im2col:grid-stride-generic"], 3, 7, 2, 3, 2, 365, 365, 13, src="f32", dst="bf16", layout="nchw", path="generic")
im2col("refuse-kpad", ["im2col:refuse-kpad"], 8, 3, 1, 1, 3, 5, 7, -8, refuse="arg")
im2col("refuse-stride0", ["im2col:refuse-stride0"], 8, 3, 0, 1, 3, 5, 7, 0, refuse="arg")
im2col("refuse-no-output-s1", ["im2col:refuse-ho"], 8, 7, 1, 1, 3, 4, 7, 0, refuse="arg")          # H + 2 pad = 6 < 7
im2col("refuse-no-output-s2", ["im2col:refuse-ho"], 8, 7, 2, 1, 3, 4, 7, 0, refuse="arg")          # (6 - 7) / 2 truncates to 0 in C


def im2col_path(c):
    """the wrapper's choice, restated from its conditions (include/fcmf_hip.h: NHWC, C % 8, Kpad % 8, one dtype, 16-byte aligned)"""
    K = c["k"] * c["k"] * c["C"]
    ok = (c["layout"] == "nhwc", c["C"] % 8 == 0, (K + c["kextra"]) % 8 == 0, c["src"] == c["dst"], c["off"] * ES[c["src"]] % 16 == 0)
    return ("fast" if all(ok) else "generic"), ok


# ---- fcmf_pack_rgb0 -------------------------------------------------------------------------------------------------------------
for src in ("f32", "f64", "bf16"):
    for layout in ("nchw", "nhwc", "crop"):
        for H, W in ((5, 7), (1, 1), (37, 30)):
            for pad in (0, 3):
                for wextra in (0, 5):
                    case("pack", f"{src}-{layout}-h{H}w{W}-pad{pad}-Wp+{wextra}",
                         [f"pack:{src}", f"pack:{layout}", f"pack:pad{pad}"] + ["pack:wp-wider"] * (wextra > 0), src=src, layout=layout, N=2, H=H, W=W,
                         pad=pad, wextra=wextra, refuse=None)
case("pack", "refuse-wp", ["pack:refuse-wp"], src="f32", layout="nchw", N=2, H=5, W=7, pad=3, wextra=-1, refuse="arg")

# ---- fcmf_bn_stats --------------------------------------------------------------------------------------------------------------
STATS_SHAPES = {(1, 2): "stats:one-short-chunk", (1, 50): "stats:last-chunk-of-2-rows", (3, 274): "stats:more-than-16-chunks",
                (7, 30): "stats:odd-groups", (64, 1026): "stats:four-in-flight-plus-tail"}
for dt in ("f32", "bf16"):
    for C, cname in ((4, "stats:c4-rpp256"), (64, "stats:c64"), (128, "stats:c128"), (256, "stats:one-slab"), (512, "stats:two-slabs"),
                     (2048, "stats:eight-slabs")):
        for (G, rpg), sname in STATS_SHAPES.items():
            if rpg == 1026 and C != 64:
                continue
            case("stats", f"c{C}-g{G}r{rpg}-{dt}", [cname, sname], dt=dt, C=C, groups=G, rpg=rpg, refuse=None)
# the 4096-row cap of the chunking: rows_per_group > 4096 * 1024 / (slabs * groups).  At the trunk's channel counts that is 2^28 (C = 64)
# to 2^30 (C >= 256) elements; at C = 4 it is 2^24, 34 MB of bf16 (a thread's float partial then covers 16 rows)
case("stats", "chunk-cap-c4-g1r4194306-bf16", ["stats:c4-rpp256", "stats:chunk-cap-4096"], dt="bf16", C=4, groups=1, rpg=4096 * 1024 + 2, refuse=None)
for C in (12, 6, 320):
    case("stats", f"refuse-c{C}", ["stats:refuse-c"], dt="f32", C=C, groups=1, rpg=50, refuse="arg")

# ---- fcmf_bn_stats_blocks -------------------------------------------------------------------------------------------------------
for C in (64, 512):
    for G in (1, 3):
        for nb in (1, 15, 16, 17, 49, 64, 65, 113, 130):
            branch = "blocks:fewer-than-16" if nb < 16 else "blocks:tail-only" if nb <= 48 else "blocks:four-in-flight" + ("-plus-tail" if nb % 64 else "")
            case("blocks", f"c{C}-g{G}-nb{nb}", [branch], C=C, groups=G, nb=nb, block_rows=128, rpg=nb * 128, refuse=None)
case("blocks", "refuse-c320", ["blocks:refuse-c"], C=320, groups=1, nb=16, block_rows=128, rpg=2048, refuse="arg")
case("blocks", "unsupported-partial-block", ["blocks:unsupported-rows"], C=64, groups=3, nb=16, block_rows=128, rpg=2048 + 2, refuse="unsupported")


# ---- BatchNorm: finalize + apply, separate ("sep") and in one launch ("fused") -------------------------------------------------
def bn(mode, name, claims, dt, C, groups, rpg, train=True, res=False, relu=0, alias=False, hw=None, eps=0.0, mom=0.25, stats_out=True,
       kind="dyadic", expect="ok", misalign=None):
    tag = f"{mode}-{name}-c{C}-g{groups}r{rpg}-{dt}" + ("" if train else "-eval") + ("-res" * res) + ("-relu" * relu) + ("-inplace" * alias) + \
        (f"-pad{hw[0]}x{hw[1]}" if hw else "")
    case("bn", tag, claims, mode=mode, dt=dt, C=C, groups=groups, rpg=rpg, train=train, res=res, relu=relu, alias=alias, hw=hw, eps=eps, mom=mom,
         stats_out=stats_out, kind=kind, expect=expect, misalign=misalign)


for dt in ("f32", "bf16"):
    for C in (4, 64, 2048):
        bn("sep", "train", ["bn:train", "apply:plain"], dt, C, 1, 30)
        bn("sep", "train", ["bn:train", "apply:res", "apply:relu"], dt, C, 3, 30, res=True, relu=1, mom=0.5)
        bn("sep", "eval", ["bn:eval", "apply:relu"], dt, C, 1, 31, train=False, relu=1)
    bn("sep", "inplace", ["apply:alias"], dt, 64, 3, 30, relu=1, alias=True)
    bn("sep", "no-stats-out", ["bn:null-stats-out"], dt, 64, 3, 30, res=True, stats_out=False)
    bn("sep", "one-row", ["bn:count-1"], dt, 64, 3, 1, eps=0.25)
    for hw in ((1, 1), (3, 5), (7, 7)):
        bn("sep", "pad", ["apply:pad"], dt, 64, 2, hw[0] * hw[1] * 2, res=True, relu=1, hw=hw)
    # fused: C / E over the powers of two the trunk uses and at its limits (E = 4 float32, 8 bf16 channels per lane)
    small, wide = (4, 1024) if dt == "f32" else (8, 2048)
    bn("fused", "n<256", ["fused:n-below-256", "fused:ce-1"], dt, small, 3, 2, res=True, relu=1)
    bn("fused", "multi-block-multi-stage", ["fused:blocks>1-stages>1", "fused:ema-once"], dt, 64, 2, 2050, res=True, relu=1, mom=0.5)
    bn("fused", "ragged", ["fused:n-not-multiple-of-sweep"], dt, 256 if dt == "f32" else 64, 3, 30, relu=1)
    bn("fused", "ce-256", ["fused:ce-256", "fused:n-not-multiple-of-sweep"], dt, wide, 1 if dt == "f32" else 3, 50 if dt == "f32" else 274)
    bn("fused", "inplace", ["fused:inplace"], dt, 64, 3, 30, relu=1, alias=True)
    bn("fused", "eval", ["fused:eval"], dt, 64, 1, 31, train=False, res=True, relu=1)
    bn("fused", "no-stats-out", ["fused:null-stats-out"], dt, 64, 3, 30, stats_out=False)
    bn("fused", "one-row", ["fused:count-1"], dt, 64, 3, 1, eps=0.25)
    for hw in ((1, 1), (3, 5), (7, 7)):
        bn("fused", "pad", ["fused:pad"], dt, 64, 2, hw[0] * hw[1] * 2, res=True, relu=1, hw=hw)
    bn("fused", "pad-multi-block", ["fused:pad", "fused:blocks>1-stages>1"], dt, 64, 2, 49 * 42, relu=1, hw=(7, 7))
    # what the fused entry point declines (FCMF_ERR_UNSUPPORTED, nothing written); the separate entry points then give the reference
    bn("fused", "unsupported-c96", ["fused:unsupported-c96"], dt, 96, 3, 30, res=True, relu=1, expect="unsupported")
    for which in ("x", "y", "res"):
        bn("fused", f"unsupported-{which}+8bytes", ["fused:unsupported-misaligned"], dt, 64, 3, 30, res=True, relu=1, expect="unsupported", misalign=which)
    # bounded, not exact: normal data with eps = 1e-5, and a constant non-dyadic channel whose variance must clamp at 0
    bn("both", "realistic", ["bn:realistic"], dt, 64, 3, 274, res=True, relu=0, eps=1e-5, mom=0.1, kind="normal")
    bn("both", "variance-clamp", ["bn:variance-clamp"], dt, 64, 1, 1000, eps=1e-3, mom=0.1, kind="constant")
bn("fused", "unsupported-f32-c2048", ["fused:unsupported-ce-512"], "f32", 2048, 3, 30, res=True, relu=1, expect="unsupported")
bn("fused", "unsupported-bf16-c4", ["fused:unsupported-c%8"], "bf16", 4, 3, 30, res=True, relu=1, expect="unsupported")
# rows * C / 4 = 262 200 * 16 = 4 195 200 vectors, 0.02 % above the cap; in place, so that the case holds one 67 MB tensor
bn("sep", "gridstride", ["apply:grid-stride"], "f32", 64, 3, 87400, relu=1, alias=True)
bn("sep", "refuse-one-null", ["bn:refuse-one-null"], "f32", 64, 3, 30, expect="one-null")
bn("sep", "rows-0", ["apply:rows-0"], "f32", 64, 3, 30, expect="rows0")
bn("sep", "pad-refuse-rows", ["apply:pad-refuse-rows"], "f32", 64, 1, 32, hw=(3, 5), expect="pad-rows")

# ---- fcmf_maxpool3x3s2 ----------------------------------------------------------------------------------------------------------
for dt in ("f32", "bf16"):
    for C in (4, 64):
        for H, W in ((1, 1), (2, 2), (3, 5), (13, 16)):
            for kind in ("continuous", "ties", "negative", "neg-inf-window"):
                case("maxpool", f"{kind}-c{C}-h{H}w{W}-{dt}", ["maxpool:" + kind] + ["maxpool:odd-edge"] * (H == 13), dt=dt, C=C, N=3, H=H, W=W,
                     kind=kind, refuse=None)
case("maxpool", "continuous-c4-h112w112-f32", ["maxpool:stem-size"], dt="f32", C=4, N=3, H=112, W=112, kind="continuous", refuse=None)
# N * Ho * Wo * C / 4 = 3 * 87400 * 16 = 4 195 200 vectors, 0.02 % above the cap; one image row, so that input + output stay at 100 MB
case("maxpool", "gridstride-c64-h1w174800-bf16", ["maxpool:grid-stride"], dt="bf16", C=64, N=3, H=1, W=174800, kind="ties", refuse=None)
case("maxpool", "refuse-c6", ["maxpool:refuse-c"], dt="f32", C=6, N=3, H=3, W=5, kind="continuous", refuse="arg")

# ---- fcmf_adaptive_avgpool ------------------------------------------------------------------------------------------------------
for dt in ("f32", "bf16"):
    for C in (3, 64):
        for layout in (0, 1):
            for (H, W, oh, ow), branch in (((7, 7, 7, 7), "identity"), ((7, 7, 1, 1), "global-49"), ((14, 14, 7, 7), "2x2"),
                                           ((13, 16, 3, 5), "uneven-overlapping"), ((5, 5, 7, 7), "upsampling"), ((1, 1, 7, 7), "broadcast")):
                case("avgpool", f"{branch}-{H}x{W}>{oh}x{ow}-c{C}-layout{layout}-{dt}", ["avgpool:" + branch, f"avgpool:layout{layout}"], dt=dt, C=C,
                     N=3, H=H, W=W, oh=oh, ow=ow, layout=layout, refuse=None)
case("avgpool", "gridstride-7x7>7x7-c1024-n86-bf16", ["avgpool:grid-stride"], dt="bf16", C=1024, N=86, H=7, W=7, oh=7, ow=7, layout=1, refuse=None)
case("avgpool", "refuse-layout2", ["avgpool:refuse-layout"], dt="f32", C=3, N=3, H=7, W=7, oh=7, ow=7, layout=2, refuse="arg")

IDS = [c["id"] for c in CASES]
BY_ID = {c["id"]: c for c in CASES}
OF = lambda fam: [c["id"] for c in CASES if c["fam"] == fam]

# every branch named for the kernels and wrappers of csrc/conv.hip: the table must claim each
BRANCHES = """im2col:fast im2col:fast-tail-columns im2col:fast-1x1 im2col:generic-stem-nchw im2col:generic-c%8 im2col:generic-kpad%8
im2col:generic-misaligned im2col:generic-dtype-change im2col:generic-padded-sn im2col:grid-stride-fast im2col:grid-stride-generic
im2col:refuse-kpad im2col:refuse-stride0 im2col:refuse-ho
pack:f32 pack:f64 pack:bf16 pack:nchw pack:nhwc pack:crop pack:pad0 pack:pad3 pack:wp-wider pack:refuse-wp
stats:c4-rpp256 stats:c64 stats:c128 stats:one-slab stats:two-slabs stats:eight-slabs stats:one-short-chunk stats:last-chunk-of-2-rows
stats:more-than-16-chunks stats:odd-groups stats:four-in-flight-plus-tail stats:chunk-cap-4096 stats:refuse-c
blocks:fewer-than-16 blocks:tail-only blocks:four-in-flight blocks:four-in-flight-plus-tail blocks:refuse-c blocks:unsupported-rows
bn:train bn:eval bn:null-stats-out bn:count-1 bn:refuse-one-null bn:realistic bn:variance-clamp
apply:plain apply:res apply:relu apply:alias apply:rows-0 apply:grid-stride apply:pad apply:pad-refuse-rows
fused:n-below-256 fused:ce-1 fused:ce-256 fused:n-not-multiple-of-sweep fused:blocks>1-stages>1 fused:ema-once fused:pad fused:inplace fused:eval
fused:null-stats-out fused:count-1 fused:unsupported-ce-512 fused:unsupported-c96 fused:unsupported-c%8 fused:unsupported-misaligned
maxpool:continuous maxpool:ties maxpool:negative maxpool:neg-inf-window maxpool:odd-edge maxpool:stem-size maxpool:grid-stride maxpool:refuse-c
avgpool:identity avgpool:global-49 avgpool:2x2 avgpool:uneven-overlapping avgpool:upsampling avgpool:broadcast avgpool:layout0 avgpool:layout1
avgpool:grid-stride avgpool:refuse-layout""".split()


# ---- inputs and expected outputs of a case (float64; shared by the checks below and the GPU file) --------------------------------
@functools.lru_cache(maxsize=2)
def reference(cid):
    c = BY_ID[cid]
    return globals()["_ref_" + c["fam"]](c)


def _ref_im2col(c):
    x = TR.grid_values((c["N"], c["H"], c["W"], c["C"]), c["seed"])          # eighths up to 2: exact in bf16
    K = c["k"] * c["k"] * c["C"]
    r = dict(x=x, K=K, Kpad=K + c["kextra"])
    if not c["refuse"]:
        r["A"] = TR.im2col_ref(x, c["k"], c["k"], c["stride"], c["pad"], r["Kpad"])
    return r


def _ref_pack(c):
    g = TR._gen(c["seed"])
    x = torch.randn(c["N"], c["H"], c["W"], 3, generator=g, dtype=torch.float64) * 2          # NOT bf16 values: the conversion rounds
    x = x.to(DT[c["src"]])
    r = dict(x=x, Wp=c["W"] + 2 * c["pad"] + c["wextra"])
    if not c["refuse"]:
        r["mask"], r["vals"] = TR.pack_rgb0_ref(x, c["pad"], r["Wp"])
    return r


def _ref_stats(c):
    if c["refuse"]:
        return dict(x=TR.grid_values((c["groups"] * c["rpg"], c["C"]), c["seed"]))
    x, m, a = TR.bn_input(c["groups"], c["rpg"], c["C"], c["seed"])
    return dict(x=x, m=m, a=a, totals=TR.bn_totals_ref(x, c["groups"]))


def _ref_blocks(c):
    # block sums in quarters up to 64, block sums of squares in sixteenths up to 64: 130 of them add up exactly in any order
    G, nb, C = c["groups"], c["nb"], c["C"]
    s = TR.grid_values((G * nb, C), c["seed"], 0.25, 64.0)
    q = TR.grid_values((G * nb, C), c["seed"] + 1, 0.0625, 32.0) + 32.0
    st = torch.stack([s, q], -1)
    return dict(stats=st, totals=st.reshape(G, nb, C, 2).sum(1))


def _ref_bn(c):
    G, rpg, C, dt = c["groups"], c["rpg"], c["C"], DT[c["dt"]]
    rows = G * rpg
    gamma, beta, rmean, rvar = TR.bn_params(C, c["seed"] + 7)
    if c["kind"] == "normal":
        g = TR._gen(c["seed"])
        x = (torch.randn(rows, C, generator=g, dtype=torch.float64) * 1.5 + 0.5).to(dt).double()          # the kernel's own input values
        gamma, beta = gamma + 0.3, beta + 0.1
        rvar = rvar + 0.37
    elif c["kind"] == "constant":
        g = TR._gen(c["seed"])
        x = torch.randn(rows, C, generator=g, dtype=torch.float64).to(dt).double()
        x[:, 5] = torch.tensor(0.1).to(dt).double()
    elif c["train"]:
        x, m, a = TR.bn_input(G, rpg, C, c["seed"])
    else:
        x, rmean, rvar = TR.bn_eval_input(rows, C, c["seed"])
    res = TR.grid_values((rows, C), c["seed"] + 3) if c["res"] else None
    if c["kind"] == "normal":
        res = torch.randn(rows, C, generator=g, dtype=torch.float64).to(dt).double()
    totals = TR.bn_totals_ref(x, G) if c["train"] else None
    f = TR.bn_finalize_ref(totals, gamma, beta, rmean, rvar, rpg, c["mom"], c["eps"])
    y = TR.bn_apply_ref(x, res, f["scale"], f["shift"], rpg if c["train"] else rows, c["relu"])
    r = dict(x=x, res=res, gamma=gamma, beta=beta, rmean=rmean, rvar=rvar, totals=totals, y=y, **{"f_" + k: v for k, v in f.items()})
    if c["kind"] == "dyadic" and c["train"]:
        r["m"], r["a"] = m, a
    return r


def _ref_maxpool(c):
    N, H, W, C = c["N"], c["H"], c["W"], c["C"]
    x = TR.grid_values((N, H, W, C), c["seed"], 0.125, 4.0)
    if c["kind"] == "ties":
        x = x.clamp(min=0.0)          # post-ReLU: half zeros, and few distinct values
    elif c["kind"] == "negative":
        x = -x.abs() - 0.125          # a padding tap taken for 0 would win every border window
    elif c["kind"] == "neg-inf-window":
        x[1, :3, :3] = float("-inf")          # the window of output (0, 0) of image 1 covers rows / columns -1 .. 1: all -inf
    return dict(x=x, y=TR.maxpool_ref(x) if not c["refuse"] else None)


def _ref_avgpool(c):
    x = TR.grid_values((c["N"], c["H"], c["W"], c["C"]), c["seed"], 0.125, 4.0)
    if c["refuse"]:
        return dict(x=x)
    y, cnt, mag = TR.avgpool_ref(x, c["oh"], c["ow"], c["layout"])
    return dict(x=x, y=y, cnt=cnt, mag=mag)


def device_bytes(c):
    """what the GPU test of the case allocates, frames aside"""
    f = c["fam"]
    if f == "im2col":
        rows = c["N"] * max(1, TR.conv_out(c["H"], c["k"], max(1, c["stride"]), c["pad"])) * max(1, TR.conv_out(c["W"], c["k"], max(1, c["stride"]), c["pad"]))
        return c["N"] * c["H"] * c["W"] * c["C"] * ES[c["src"]] + rows * (c["k"] ** 2 * c["C"] + abs(c["kextra"])) * ES[c["dst"]]
    if f == "pack":
        return 4 * c["N"] * (c["H"] + 8) * (c["W"] + 16) * 3 * ES[c["src"]] + c["N"] * (c["H"] + 6) * (c["W"] + 11) * 8
    if f == "stats":
        return c["groups"] * c["rpg"] * c["C"] * ES[c["dt"]] + 8 * TR.bn_workspace(c["rpg"], c["groups"], c["C"])
    if f == "blocks":
        return c["groups"] * c["nb"] * c["C"] * 8 + 8 * TR.bn_workspace(c["rpg"], c["groups"], c["C"])
    if f == "bn":
        n = c["groups"] * c["rpg"] * c["C"] * ES[c["dt"]]
        grow = (c["hw"][0] + 2) * (c["hw"][1] + 2) / (c["hw"][0] * c["hw"][1]) if c["hw"] else 1
        return int(n * ((0 if c["alias"] else 1) + (1 if c["res"] else 0) + grow * (2 if c["mode"] == "both" else 1))) + 8 * TR.bn_workspace(c["rpg"], c["groups"], c["C"])
    if f == "maxpool":
        return c["N"] * c["C"] * ES[c["dt"]] * (c["H"] * c["W"] + TR.conv_out(c["H"], 3, 2, 1) * TR.conv_out(c["W"], 3, 2, 1))
    return c["N"] * c["C"] * (c["H"] * c["W"] * ES[c["dt"]] + c["oh"] * c["ow"] * 4)


# ---- the table ------------------------------------------------------------------------------------------------------------------
def test_table_claims_every_branch():
    claimed = {b for c in CASES for b in c["claims"]}
    missing = [b for b in BRANCHES if b not in claimed]
    assert not missing, missing
    assert claimed <= set(BRANCHES), sorted(claimed - set(BRANCHES))
    assert len(IDS) == len(set(IDS))
    assert {c["fam"] for c in CASES} == {"im2col", "pack", "stats", "blocks", "bn", "maxpool", "avgpool"}


def test_no_case_allocates_more_than_128_mb():
    worst = max(CASES, key=device_bytes)
    print(f"largest case: {worst['id']}, {device_bytes(worst) / 2 ** 20:.1f} MB")
    assert device_bytes(worst) <= 128 << 20, worst["id"]


def test_im2col_cases_take_the_path_they_are_listed_under():
    for c in CASES:
        if c["fam"] != "im2col" or c["refuse"]:
            continue
        path, ok = im2col_path(c)
        assert path == c["path"], c["id"]
        if path == "generic" and c["layout"] != "nchw":
            assert sum(not o for o in ok) == 1, (c["id"], ok)          # one disqualifier on its own


def test_grid_stride_cases_sit_just_above_the_cap():
    def work(c):
        f = c["fam"]
        if f == "im2col":
            rows = c["N"] * TR.conv_out(c["H"], c["k"], c["stride"], c["pad"]) * TR.conv_out(c["W"], c["k"], c["stride"], c["pad"])
            return rows * (c["k"] ** 2 * c["C"] + c["kextra"]) // 8 if c["path"] == "fast" else rows * 64          # a wave of 64 lanes per row
        if f == "bn":
            return c["groups"] * c["rpg"] * c["C"] // 4
        if f == "maxpool":
            return c["N"] * TR.conv_out(c["H"], 3, 2, 1) * TR.conv_out(c["W"], 3, 2, 1) * c["C"] // 4
        return c["N"] * c["oh"] * c["ow"] * c["C"]
    seen = 0
    for c in CASES:
        if any("grid-stride" in b for b in c["claims"]):
            seen += 1
            assert CAP < work(c) <= CAP * 1.1, (c["id"], work(c) / CAP)
    assert seen == 5


def test_chunking_of_the_statistics_cases():
    """the (groups, rows_per_group) pairs reach the chunk shapes their ids name (trunk_ref.bn_chunks restates the library's rule)"""
    assert TR.bn_chunks(2, 1, 64) == (1, 16)
    assert TR.bn_chunks(50, 1, 64) == (4, 16)                    # rows 48, 49 are the last chunk
    assert TR.bn_chunks(274, 3, 64)[0] == 18                     # more than the 16 waves of the reduce kernel
    assert TR.bn_chunks(1026, 64, 64) == (16, 65)                # 65 rows on 16 rows per pass: one round of four, then one row
    assert TR.bn_chunks(274, 3, 512)[0] == 18 and TR.bn_chunks(30, 7, 2048) == (2, 16)
    assert TR.bn_chunks(4096 * 1024 + 2, 1, 4) == (1025, 4096)   # 4097 rows per chunk asked for, 4096 given: one more chunk, of 2 rows
    assert TR.bn_chunks(4096 * 1024, 1, 4) == (1024, 4096)
    assert [C for C in (4, 8, 12, 6, 64, 96, 128, 256, 320, 512, 2048) if not TR.bn_stats_ok(C)] == [12, 6, 96, 320]


# ---- the references against torch -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [i for i in OF("im2col") if not BY_ID[i]["refuse"]])
def test_im2col_ref_is_unfold(cid):
    c, r = BY_ID[cid], reference(cid)
    k, C, K = c["k"], c["C"], r["K"]
    cols = F.unfold(r["x"].permute(0, 3, 1, 2), k, padding=c["pad"], stride=c["stride"])          # [N, C * k * k, L], channel-major
    N, _, L = cols.shape
    want = cols.reshape(N, C, k * k, L).permute(0, 3, 2, 1).reshape(N * L, K)                      # -> (r, s, c)
    assert torch.equal(r["A"][:, :K], want)
    assert bool((r["A"][:, K:] == 0).all())
    assert TR.representable(r["A"], DT[c["dst"]]) and float(r["A"].abs().max()) > 0


def test_pack_ref_and_pad_rows():
    for cid in OF("pack"):
        c, r = BY_ID[cid], reference(cid)
        if c["refuse"]:
            continue
        N, H, W, pad, Wp = c["N"], c["H"], c["W"], c["pad"], r["Wp"]
        assert int(r["mask"].sum()) == N * H * W * 4
        for n, h, w in ((0, 0, 0), (N - 1, H - 1, W - 1), (1, H // 2, W // 3)):
            want = r["x"][n, h, w].float().bfloat16().double() if c["src"] != "f64" else TR.nearest_bf16(r["x"][n, h, w])
            assert torch.equal(r["vals"][n, h + pad, w + pad, :3], want) and float(r["vals"][n, h + pad, w + pad, 3]) == 0
            assert bool(r["mask"][n, h + pad, w + pad].all())
        assert not bool(r["mask"][:, :, W + 2 * pad:].any()) and not bool(r["mask"][:, :pad].any())
        assert TR.representable(r["vals"], torch.bfloat16)
    # one rounding, not two: just beyond the midpoint of 1.53125 and 1.5390625 the nearest bf16 is the upper one, while the detour
    # through float32 lands on the midpoint and then on the even, lower one (the GPU test's first run met two such pixels)
    mid = torch.tensor([1.53515625, 1.53515625 + 2.0 ** -40, -1.53515625 - 2.0 ** -40, 1.53515625 - 2.0 ** -40, 1.546875, 0.0, 3.0], dtype=torch.float64)
    assert TR.nearest_bf16(mid).tolist() == [1.53125, 1.5390625, -1.5390625, 1.53125, 1.546875, 0.0, 3.0]
    assert mid.float().bfloat16().double().tolist()[1:3] == [1.53125, -1.53125]
    v = torch.randn(20000, generator=TR._gen(5), dtype=torch.float64) * 3
    assert torch.equal(TR.nearest_bf16(v.float()), v.float().bfloat16().double())          # float32 and bf16 sources: torch's cast is the one rounding
    assert float((TR.nearest_bf16(v) - v).abs().max()) <= float(((v.float().bfloat16().double()) - v).abs().max())
    for N, H, W, pad in ((2, 3, 5, 1), (4, 1, 1, 1), (2, 7, 7, 1), (2, 5, 7, 3)):
        rows = TR.pad_rows(N, H, W, pad)
        flat = torch.zeros(N, H + 2 * pad, W + 2 * pad)
        flat[:, pad:pad + H, pad:pad + W] = 1 + torch.arange(N * H * W).reshape(N, H, W).float()
        assert torch.equal(flat.reshape(-1)[rows], 1 + torch.arange(N * H * W).float())
        assert int((flat != 0).sum()) == rows.numel() == len(set(rows.tolist()))


def _var(x):
    """two-pass biased variance over the rows of x [groups, rows, C]: exact on the builder's inputs (torch.var's update form is not)"""
    d = x - x.mean(1, keepdim=True)
    return (d * d).sum(1) / x.shape[1]


BN_EXACT = [i for i in OF("bn") if BY_ID[i]["kind"] == "dyadic" and BY_ID[i]["expect"] in ("ok", "unsupported")]


@pytest.mark.parametrize("cid", OF("stats"))
def test_stats_inputs_are_what_the_builder_promises(cid):
    c, r = BY_ID[cid], reference(cid)
    if c["refuse"]:
        return
    x = r["x"].reshape(c["groups"], c["rpg"], c["C"])
    assert torch.equal(x.mean(1), r["m"]) and torch.equal(_var(x), r["a"] ** 2)
    assert torch.equal(r["totals"][..., 0], r["m"] * c["rpg"]) and torch.equal(r["totals"][..., 1], (r["m"] ** 2 + r["a"] ** 2) * c["rpg"])
    assert TR.representable(r["x"], DT[c["dt"]])
    assert bool((r["x"] * 4 == (r["x"] * 4).round()).all()) and float(r["x"].abs().max()) <= 4
    if c["rpg"] > 2 and c["C"] > 4:          # shuffled: neither sorted by sign nor the same in every channel
        s = (x[0] > r["m"][0]).double()
        assert 0 < float(s[: c["rpg"] // 2].mean()) < 1 and not torch.equal(s[:, 0], s[:, 1])


@pytest.mark.parametrize("cid", BN_EXACT)
def test_bn_cases_are_exact_by_construction(cid):
    c, r = BY_ID[cid], reference(cid)
    dt, G, rpg, C = DT[c["dt"]], c["groups"], c["rpg"], c["C"]
    if c["train"]:
        x = r["x"].reshape(G, rpg, C)
        assert torch.equal(x.mean(1), r["m"]) and torch.equal(_var(x), r["a"] ** 2)
        assert torch.equal(r["f_mean"], r["m"])
        assert torch.equal(r["f_rstd"], 1.0 / r["a"] if rpg > 1 else torch.full_like(r["a"], 2.0))
    else:
        assert set(r["rvar"].tolist()) <= {0.25, 1.0, 4.0} and torch.equal(r["f_rmean"], r["rmean"]) and torch.equal(r["f_rvar"], r["rvar"])
    lg = torch.log2(r["f_rstd"])
    assert torch.equal(lg, lg.round())          # a power of two: 1 / sqrtf returns it exactly
    for k in ("f_scale", "f_shift", "f_mean", "f_rstd"):
        assert TR.representable(r[k], torch.float32)
    assert TR.representable(r["x"], dt) and TR.representable(r["y"], dt) and (r["res"] is None or TR.representable(r["res"], dt))
    assert bool((r["y"] * 8 == (r["y"] * 8).round()).all()) and float(r["y"].abs().max()) <= 8
    if c["relu"]:          # both signs reach the ReLU
        pre = TR.bn_apply_ref(r["x"], r["res"], r["f_scale"], r["f_shift"], rpg if c["train"] else G * rpg, 0)
        assert float((pre < 0).double().mean()) > 0.1 and float((pre > 0).double().mean()) > 0.1
    # x * scale + shift is exact in float32 step by step, not only in the end
    g = torch.arange(G * rpg) // (rpg if c["train"] else G * rpg)
    prod = r["x"] * r["f_scale"].reshape(-1, C)[g]
    assert TR.representable(prod, torch.float32) and TR.representable(prod + r["f_shift"].reshape(-1, C)[g], torch.float32)


@pytest.mark.parametrize("cid", [i for i in OF("bn") if BY_ID[i]["expect"] in ("ok", "unsupported") and BY_ID[i]["groups"] * BY_ID[i]["rpg"] < 10000])
def test_bn_refs_are_torch_batch_norm(cid):
    """one F.batch_norm call per group in training mode (torch's own running-statistics update), one call in eval mode"""
    c, r = BY_ID[cid], reference(cid)
    G, rpg, C = c["groups"], c["rpg"], c["C"]
    rm, rv = r["rmean"].clone(), r["rvar"].clone()
    x = r["x"].reshape(G, rpg, C)
    ys = []
    for g in range(G):
        if c["train"] and rpg == 1:          # (torch refuses one value per channel in training mode: normalise by hand, biased = unbiased)
            ys.append((x[g] - x[g]) * r["gamma"] + r["beta"])
            rm, rv = (1 - c["mom"]) * rm + c["mom"] * x[g, 0], (1 - c["mom"]) * rv
        else:
            # (torch.batch_norm: the operator behind F.batch_norm, which itself refuses eps = 0)
            ys.append(torch.batch_norm(x[g], r["gamma"], r["beta"], rm, rv, c["train"], c["mom"], c["eps"], False))
    y = torch.cat(ys)
    if r["res"] is not None:
        y = y + r["res"]
    if c["relu"]:
        y = y.clamp(min=0)
    tol = dict(rtol=1e-12, atol=1e-12)
    assert torch.allclose(r["y"], y, **tol)
    assert torch.allclose(r["f_rmean"], rm, **tol) and torch.allclose(r["f_rvar"], rv, **tol)
    if c["train"]:
        assert torch.allclose(r["f_mean"], x.mean(1), **tol) and torch.allclose(r["f_rstd"], 1 / torch.sqrt(_var(x) + c["eps"]), **tol)


def test_bn_bounded_cases_are_what_they_say():
    for cid in OF("bn"):
        c, r = BY_ID[cid], reference(cid)
        if c["kind"] == "constant":
            v = r["x"][:, 5]
            assert bool((v == v[0]).all()) and float(v[0] * 8) != round(float(v[0] * 8))          # constant and not dyadic
            assert abs(float(r["f_rstd"][0, 5]) - c["eps"] ** -0.5) < 1e-9 * c["eps"] ** -0.5
        if c["kind"] == "normal":
            assert TR.representable(r["x"], DT[c["dt"]]) and not TR.representable(r["f_scale"], torch.float32)


@pytest.mark.parametrize("cid", [i for i in OF("maxpool") if not BY_ID[i]["refuse"]])
def test_maxpool_ref_is_torch(cid):
    c, r = BY_ID[cid], reference(cid)
    want = F.max_pool2d(r["x"].permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    assert torch.equal(r["y"], want) and TR.representable(r["y"], DT[c["dt"]]) and TR.representable(r["x"], DT[c["dt"]])
    if c["kind"] == "negative":
        assert float(r["y"].max()) < 0
    if c["kind"] == "neg-inf-window":
        assert bool((r["y"][1, 0, 0] == float("-inf")).all()) and (c["H"] < 4 or bool(torch.isfinite(r["y"][0]).all()))
    if c["kind"] == "ties" and r["x"].numel() >= 100:
        assert 0.3 < float((r["x"] == 0).double().mean()) < 0.7


@pytest.mark.parametrize("cid", [i for i in OF("avgpool") if not BY_ID[i]["refuse"]])
def test_avgpool_ref_is_torch(cid):
    c, r = BY_ID[cid], reference(cid)
    want = F.adaptive_avg_pool2d(r["x"].permute(0, 3, 1, 2), (c["oh"], c["ow"]))
    if c["layout"] == 1:
        want = want.permute(0, 2, 3, 1).reshape(c["N"], c["oh"] * c["ow"], c["C"])
    assert torch.allclose(r["y"], want, rtol=1e-14, atol=1e-14)
    assert TR.representable(r["x"], DT[c["dt"]])
    # every window sum is exact in float32: eighths, at most 49 * 4 * 8 units
    assert float(r["mag"].max()) * 8 < 2 ** 24
    exact = TR.is_pow2(r["cnt"].numpy())
    assert TR.representable(r["y"][torch.from_numpy(exact)], torch.float32)
    assert exact.all() == (c["claims"][0] in ("avgpool:identity", "avgpool:2x2", "avgpool:upsampling", "avgpool:broadcast", "avgpool:grid-stride"))


def test_blocks_cases_sum_exactly():
    for cid in OF("blocks"):
        r = reference(cid)
        assert TR.representable(r["stats"], torch.float32) and bool((r["totals"] * 16 == (r["totals"] * 16).round()).all())
        assert float(r["totals"].abs().max()) * 16 < 2 ** 24
