"""The cases of test_gemm_exact_gpu.py and, on the float64 reference alone, what its equalities rely on (tests/gemm_ref.py):

  * every value a kernel has to hold exactly -- accumulator, pre-activation, output, aux, column sum, block statistic -- is
    n * 2^-s with |n| <= 256 where it is stored as bf16 and |n| < 2^24 where it is float32 (and survives the cast to its dtype);
  * at least 30 % of the outputs are non-zero;
  * a dropped contraction index changes at least a quarter of the outputs: recomputed with the last index zeroed, and with the
    last index of the first k-tile zeroed;
  * every block sum of squares of the statistics cases is below 2^24.

These are conditions, not measurements: if a seed breaks one, the seed changes, never the bound.

CASES lists every GPU case: entry point, family, the kernel name it must reach, shape, layouts, dtypes, epilogue, leading
dimensions (as paddings of the contiguous extent), tuning knobs and seed.  A case is listed under the kernel the planner gives it.
The MFMA loaders refuse a transposed A of 130 or 300 rows (M % 8 != 0): those shapes are listed under the generic kernel, where
they run, and their neighbours with M = 136 / 304 / 704 under the MFMA family."""
import functools

import pytest
import torch

import gemm_ref as GR

F32_LIM = float(2 ** 24 - 1)
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
EXACT_EPI = ("NONE", "ADD", "DTANH")          # epilogues whose output is on the grid; the activations are bounded per element

CASES = []


def case(entry, family, kernel, M, N, K, **kw):
    c = dict(entry=entry, family=family, kernel=kernel, M=M, N=N, K=K, ta=0, tb=0, inp="bf16", out="bf16", epi="NONE", bias=False,
             colsum=False, acc=False, prior=None, ws=True, tile=0, kb=64, cus=256, pad_a=8, pad_b=8, pad_c=8, rows_extra=3,
             shift_a=0, shift_b=0, also_cus=None, ktile=32, note="")
    c.update(kw)
    if "conv" in c:          # n, Hp, Wp, C, stride of a 3 x 3 convolution: M = its output pixels
        n, Hp, Wp, _, stride = c["conv"]
        c["M"], c["note"] = M = n * ((Hp - 3) // stride + 1) * ((Wp - 3) // stride + 1), f"n{n}h{Hp}s{stride}"
    if "runs" in c:          # n, Hp, Wp, pix, run, Ho, Wo, kh, stride
        c["M"] = M = c["runs"][0] * c["runs"][5] * c["runs"][6]
    if c["acc"] and c["prior"] is None:
        c["prior"] = "dyadic"
    c["seed"] = kw.get("seed", 1000 + 7 * len(CASES))
    flags = "".join(f"-{f}" for f in ("bias", "colsum", "acc") if c[f]) + ("" if c["ws"] else "-nows") + (f"-{c['note']}" if c["note"] else "")
    c["id"] = (f"{entry}-{family}-{M}x{N}x{K}-{c['ta']}{c['tb']}-{c['inp']}>{c['out']}-{c['epi']}{flags}"
               f"-t{c['tile']}k{c['kb']}c{c['cus']}-ldc+{c['pad_c']}")
    assert all(o["id"] != c["id"] for o in CASES), c["id"]
    CASES.append(c)


LAYOUTS = [(0, 0), (0, 1), (1, 0), (1, 1)]
GEN = "gemm_generic_kernel"


def _epilogue_cases(family, kernel_of, M, N, K, epis, **kw):
    """bias, ADD, column sums, GELU with its aux (B in steps of 1/8), gelu', and the tanh pair where the kernel carries it"""
    case("gemm", family, kernel_of("NONE"), M, N, K, colsum=True, bias=True, **kw)
    for epi in epis:
        case("gemm", family, kernel_of(epi), M, N, K, epi=epi, bias=epi in ("ADD", "GELU", "TANH"), shift_b=3 if epi in ("GELU", "TANH") else 0, **kw)


ALL_EPIS = ("ADD", "GELU", "DGELU", "TANH", "DTANH")
TILE_EPIS = ("ADD", "GELU", "DGELU")          # the persistent kernels carry no tanh epilogue (plan_mfma: the 128 x 128 kernel)

# ---- generic kernel: float32 in and out, and bf16 shapes the MFMA loaders refuse ------------------------------------------------
for inp in ("f32", "bf16"):
    for M, N, K in ((37, 5, 70), (70, 36, 300)):
        for ta, tb in LAYOUTS:
            case("gemm", "generic", GEN, M, N, K, ta=ta, tb=tb, inp=inp, out=inp, bias=True, pad_a=3, pad_b=3, pad_c=8 if ta else 3, ktile=16,
                 **(dict(seed=6) if N == 5 else {}))          # (five columns: a seed under which indices 15 and 69 reach enough of them)
# its split-K: accumulate, fewer than 128 blocks, K >= 128
case("gemm", "generic", GEN, 70, 36, 300, ta=1, tb=1, inp="f32", out="f32", acc=True, pad_a=3, pad_b=3, ktile=16)
case("gemm", "generic", GEN, 70, 36, 300, inp="bf16", out="f32", acc=True, pad_a=3, pad_b=3, ktile=16)
case("gemm", "generic", GEN, 300, 264, 2048, ta=1, tb=1, out="f32", acc=True, ktile=16, note="m-not-x8")
# a transposed A whose rows are no multiple of 8 elements, at the MFMA families' shapes: the generic kernel, by design
for tb in (0, 1):
    case("gemm", "generic", GEN, 130, 136, 96, ta=1, tb=tb, tile=128, ktile=16, note="m-not-x8")
    case("gemm", "generic", GEN, 300, 264, 96, ta=1, tb=tb, tile=256, kb=32, ktile=16, note="m-not-x8")
_epilogue_cases("generic", lambda e: GEN, 70, 36, 300, ALL_EPIS, inp="f32", out="f32", pad_a=3, pad_b=3, pad_c=4, ktile=16)
_epilogue_cases("generic", lambda e: GEN, 70, 36, 300, ("GELU", "DGELU"), pad_a=3, pad_b=3, ktile=16)

# ---- 128 x 128 kernel (tile = 128) ----------------------------------------------------------------------------------------------
T128 = lambda ta, tb, out: f"gemm_bf16_kernel<{ta},{tb},{out}>"
for out in ("bf16", "f32"):
    for ta, tb in LAYOUTS:
        case("gemm", "tile128", T128(ta, tb, out), 136 if ta else 130, 136, 96, ta=ta, tb=tb, out=out, bias=True, tile=128)
case("gemm", "tile128", T128(0, 0, "bf16"), 130, 136, 32, bias=True, tile=128, note="one-k-tile")
case("gemm", "tile128", T128(0, 0, "bf16"), 130, 136, 160, bias=True, tile=128, note="ring+1")
case("gemm", "tile128", T128(1, 1, "bf16"), 136, 136, 72, ta=1, tb=1, bias=True, tile=128, note="partial-k-tile")
case("gemm", "tile128", T128(0, 0, "bf16"), 130, 136, 96, bias=True, tile=128, pad_c=4)          # ldc % 4 only
case("gemm", "tile128", T128(0, 0, "f32"), 130, 136, 512, out="f32", acc=True, tile=128, note="splitk-atomics")
_epilogue_cases("tile128", lambda e: T128(0, 0, "bf16"), 130, 136, 96, ALL_EPIS, tile=128)
case("gemm", "tile128", T128(0, 0, "f32"), 130, 136, 96, out="f32", epi="GELU", bias=True, shift_b=3, tile=128)

# ---- 64 x 64 kernel (tile = 0) --------------------------------------------------------------------------------------------------
SMALL = lambda out: f"gemm_bf16_small_kernel<{out}>"
for M, N, K in ((100, 136, 128), (70, 64, 64)):
    case("gemm", "small", SMALL("bf16"), M, N, K, bias=True, ktile=64)
    case("gemm", "small", SMALL("f32"), M, N, K, out="f32", acc=True, ktile=64)
_epilogue_cases("small", lambda e: SMALL("bf16"), 100, 136, 128, ALL_EPIS, ktile=64)

# ---- persistent kernels ---------------------------------------------------------------------------------------------------------
# The planner's cost model takes 192 rows wherever they save time, also under tile = 256: of (300, 264, K) only K = 32
# stays on 256 rows.  (1000, 264, K) on 8 workgroups -- 8 tiles of 256 rows in one round against 12 of 192 in two -- stays there for
# every K; so do a transposed A and a float32 output, which exist with 256 rows only.
P256 = lambda ta, tb, out, epi="NONE": f"gemm_bf16_tile256_kernel<{ta},{tb},{out},{epi}>"
P192 = lambda tb, epi="NONE": f"gemm_bf16_tile192_kernel<{tb},{epi}>"
P256K = lambda epi="NONE": f"gemm_bf16_tile256k64_kernel<{epi}>"
P192K = lambda epi="NONE": f"gemm_bf16_tile192k64_kernel<{epi}>"
case("gemm", "tile256", P256(0, 0, "bf16"), 300, 264, 32, bias=True, tile=256, kb=32, note="one-k-tile")
for K in (96, 160):
    case("gemm", "tile192", P192(0), 300, 264, K, bias=True, tile=256, kb=32, note="cost-model")
    case("gemm", "tile256", P256(0, 0, "bf16"), 1000, 264, K, bias=True, tile=256, kb=32, cus=8)
for K in (64, 128, 320):
    case("gemm", "tile192k64", P192K(), 300, 264, K, bias=True, tile=256, ktile=64, note="cost-model")
    case("gemm", "tile256k64", P256K(), 1000, 264, K, bias=True, tile=256, cus=8, ktile=64)
case("gemm", "tile192", P192(1), 300, 264, 96, tb=1, bias=True, tile=256, kb=32, note="cost-model")
case("gemm", "tile256", P256(0, 1, "bf16"), 1000, 264, 96, tb=1, bias=True, tile=256, kb=32, cus=8)
for tb in (0, 1):
    case("gemm", "tile256", P256(1, tb, "bf16"), 304, 264, 96, ta=1, tb=tb, bias=True, tile=256, kb=32)
case("gemm", "tile256", P256(0, 0, "f32"), 300, 264, 96, out="f32", bias=True, tile=256)
for tb in (0, 1):
    for K in (32, 96, 160):
        case("gemm", "tile192", P192(tb), 300, 264, K, tb=tb, bias=True, tile=192, kb=32)
    for K in (64, 128, 320):
        case("gemm", "tile192k64" if not tb else "tile192", P192(1) if tb else P192K(), 300, 264, K, tb=tb, bias=True, tile=192, ktile=32 if tb else 64)
# more items than workgroups: the ring position and the next-tile prefetch carried across items
case("gemm", "tile192", P192(0), 700, 520, 96, bias=True, tile=256, kb=32, cus=8, note="12-tiles-on-8")
case("gemm", "tile256", P256(1, 0, "bf16"), 704, 520, 96, ta=1, bias=True, tile=256, kb=32, cus=8, note="9-tiles-on-8")
case("gemm", "tile192k64", P192K(), 700, 520, 128, bias=True, tile=256, cus=8, ktile=64, note="12-tiles-on-8")
case("gemm", "tile256k64", P256K(), 1000, 520, 128, bias=True, tile=256, cus=8, ktile=64, note="12-tiles-on-8")
# split-K, float32 out: partial tiles through the workspace (RED_FRAG writes / adds, RED_ROWS with a bias), float atomics without one
SPLIT = dict(out="f32", also_cus=8)
case("gemm", "tile256", P256(1, 1, "f32"), 304, 264, 2048, ta=1, tb=1, prior="nan", note="red-frag-writes", **SPLIT)
case("gemm", "tile256", P256(1, 1, "f32"), 304, 264, 2048, ta=1, tb=1, acc=True, note="red-frag-adds", **SPLIT)
case("gemm", "tile256", P256(1, 1, "f32"), 304, 264, 2048, ta=1, tb=1, acc=True, bias=True, note="red-rows", **SPLIT)
case("gemm", "tile256", P256(1, 1, "f32"), 304, 264, 2048, ta=1, tb=1, acc=True, ws=False, note="atomics", **SPLIT)
case("gemm", "tile256", P256(0, 0, "f32"), 300, 264, 2048, acc=True, note="red-frag-adds", **SPLIT)
# narrow outputs
case("gemm", "narrow", "gemm_bf16_tile256k64_n64_kernel", 8232, 64, 64, bias=True, ktile=64)
case("gemm", "narrow", "gemm_bf16_tile256k64_n128_kernel", 8232, 128, 192, bias=True, ktile=64)
# epilogues of the four persistent instantiations
_epilogue_cases("tile192", lambda e: P192(0, e), 300, 264, 96, TILE_EPIS, tile=192, kb=32)
_epilogue_cases("tile256", lambda e: P256(0, 0, "bf16", e), 1000, 264, 96, TILE_EPIS, tile=256, kb=32, cus=8)
_epilogue_cases("tile192k64", P192K, 300, 264, 128, TILE_EPIS, tile=192, ktile=64)
_epilogue_cases("tile256k64", P256K, 1000, 264, 128, TILE_EPIS, tile=256, cus=8, ktile=64)

# ---- e4m3 -----------------------------------------------------------------------------------------------------------------------
# Scales 2^-2 .. 2^2 per row under FCMF_EPI_NONE: n * sa[i] * sb[j] is exact in bf16 for |n| <= 256.  With a bias or a residual
# the sum n * 2^e + b has to fit eight bits too, which a nine-octave range of e cannot give: those cases draw 2^-1 .. 2^0.
for K in (128, 384):
    case("fp8", "fp8", "gemm_fp8_tile192_kernel<NONE>", 300, 264, K, pad_a=16, pad_b=16, ktile=128, scale_lo=-2, scale_hi=2)
    case("fp8", "fp8", "gemm_fp8_tile192_kernel<NONE>", 300, 264, K, bias=True, pad_a=16, pad_b=16, ktile=128, scale_lo=-1, scale_hi=0)
    case("fp8", "fp8", "gemm_fp8_tile192_kernel<ADD>", 300, 264, K, epi="ADD", bias=True, pad_a=16, pad_b=16, ktile=128, scale_lo=-1, scale_hi=0)

# ---- column-blocked weight gradients --------------------------------------------------------------------------------------------
for acc in (False, True):
    case("colblocks", "tile256", P256(1, 1, "f32"), 256, 256, 1024, ta=1, tb=1, out="f32", acc=acc, col_block=64, blk_gap=40)

# ---- weight-gradient work lists on 8 workgroups: (M, N, K, destination) ----------------------------------------------------------
# The 256 x 256 tile kernel takes problems 0, 3 and 4: whole rounds of problem 4's nine tiles run unsplit, the two producers of
# destination 0 and the ninth tile form the tail, whose pieces the list reduce sums.  Problems 1 and 2 ride behind as GEMMs.
DW_LIST = [(256, 264, 512, 0), (130, 136, 256, 1), (768, 64, 1024, 2), (256, 264, 256, 0), (768, 520, 256, 4)]
DW_BATCHED = [(256, 264, 512, 0), (256, 264, 512, 1), (256, 264, 512, 0)]
for acc in (False, True):
    case("dw_list", "dw", "gemm_bf16_dw_batched_kernel", 0, 0, 0, out="f32", acc=acc, cus=8, probs=DW_LIST)
    case("dw_batched", "dw", "gemm_bf16_dw_batched_kernel", 0, 0, 0, out="f32", acc=acc, cus=8, probs=DW_BATCHED)

# ---- block statistics -----------------------------------------------------------------------------------------------------------
case("colstats", "tile256", P256(0, 0, "bf16"), 300, 264, 96, block_rows=128)
case("colstats", "tile256k64", P256K(), 300, 264, 128, ktile=64, block_rows=128)
case("colstats", "narrow", "gemm_bf16_tile256k64_n64_kernel", 8232, 64, 64, ktile=64, block_rows=256)

# ---- implicit convolution: n, Hp, Wp, C, stride, Cout (3 x 3; the zero border of one pixel is part of the activation) -----------
# n = 2 gives 128 and 50 output rows: the 128 x 128 kernel, or the 192-row persistent one under tile = 256.  Statistics exist from
# 256 rows up (n = 5 / 11) and, for 64 channels, on the narrow layout from 8192 rows up (66 x 66).
for Hp, stride in ((10, 1), (11, 2)):
    for Cout in (64, 264):
        case("conv", "tile128", T128(0, 0, "bf16"), 0, Cout, 576, conv=(2, Hp, Hp, 64, stride))
    case("conv", "tile192k64", P192K(), 0, 264, 576, conv=(2, Hp, Hp, 64, stride), tile=256, ktile=64)
case("conv_colstats", "tile256k64", P256K(), 0, 264, 576, conv=(5, 10, 10, 64, 1), ktile=64, block_rows=128)
case("conv_colstats", "tile256k64", P256K(), 0, 264, 576, conv=(11, 11, 11, 64, 2), ktile=64, block_rows=128)
case("conv_colstats", "narrow", "gemm_bf16_tile256k64_n64_kernel", 0, 64, 576, conv=(2, 66, 66, 64, 1), ktile=64, block_rows=256)
# the stem's layout: 4 elements per pixel, runs of 32, 7 kernel rows, stride 2
case("conv_runs", "tile128", T128(0, 0, "bf16"), 0, 64, 224, runs=(2, 21, 22, 4, 32, 8, 8, 7, 2))

IDS = [c["id"] for c in CASES]
BY_ID = {c["id"]: c for c in CASES}


# ---- operands and float64 results of a case --------------------------------------------------------------------------------------
def _conv_dims(c):
    n, Hp, Wp, C, stride = c["conv"]
    Ho, Wo = (Hp - 3) // stride + 1, (Wp - 3) // stride + 1
    return n, Hp, Wp, C, stride, Ho, Wo


def _drop(B, tb, k):
    if k is not None:
        B = B.clone()
        if tb:
            B[k, :] = 0
        else:
            B[:, k] = 0
    return B


def _build(c, drop_k=None):
    """-> dict of CPU tensors: operands in their stored layout and dtype, expected outputs in float64"""
    e, seed, M, N, K = c["entry"], c["seed"], c["M"], c["N"], c["K"]
    out_dt = DT[c["out"]]
    if e in ("gemm", "colblocks", "colstats"):
        ta, tb, s = c["ta"], c["tb"], c["shift_a"] + c["shift_b"]
        A = GR.dyadic((K, M) if ta else (M, K), seed, c["shift_a"])
        B = _drop(GR.dyadic((K, N) if tb else (N, K), seed + 1, c["shift_b"]), tb, drop_k)
        r = dict(A=A.to(DT[c["inp"]]), B=B.to(DT[c["inp"]]), shift=s, out_shift=s + 2 if c["epi"] == "DTANH" else s)
        r["bias"] = GR.dyadic_ints((N,), seed + 2, s) if c["bias"] else None
        epi = c["epi"]
        r["aux_in"] = (GR.dyadic_ints((M, N), seed + 3, s) if epi == "ADD" else GR.dyadic_ints((M, N), seed + 3, 3, lim=40) if epi == "DGELU"
                       else GR.dyadic((M, N), seed + 3, 1) if epi == "DTANH" else None)
        r["prior"] = GR.dyadic_ints((M, N), seed + 4, s) if c["prior"] == "dyadic" else None
        r["acc"] = GR.product(A, B, ta, tb)
        r["pre"] = r["acc"] + (0.0 if r["bias"] is None else r["bias"])
        r["C"], r["aux_out"] = GR.epilogue(r["acc"], epi, r["bias"], r["aux_in"])
        if r["prior"] is not None:
            r["C"] = r["C"] + r["prior"]
        stored = r["C"].to(out_dt).double()
        r["colsum"] = GR.colsum(stored) if c["colsum"] else None
        r["stats"] = GR.colstats(stored, c["block_rows"]) if e == "colstats" else None
        return r
    if e == "fp8":
        A, B = GR.dyadic((M, K), seed), _drop(GR.dyadic((N, K), seed + 1), 0, drop_k)
        sa, sb = GR.pow2_scales(M, seed + 5, c["scale_lo"], c["scale_hi"]), GR.pow2_scales(N, seed + 6, c["scale_lo"], c["scale_hi"])
        r = dict(A=GR.e4m3_bytes(A), B=GR.e4m3_bytes(B), sa=sa, sb=sb, shift=0, out_shift=-2 * c["scale_lo"])
        r["bias"] = GR.dyadic_ints((N,), seed + 2) if c["bias"] else None
        r["aux_in"] = GR.dyadic_ints((M, N), seed + 3) if c["epi"] == "ADD" else None
        r["acc"] = A @ B.t()
        r["pre"] = r["acc"]
        r["C"], _ = GR.epilogue(r["acc"] * sa[:, None] * sb[None, :], c["epi"], r["bias"], r["aux_in"])
        return r
    if e in ("dw_list", "dw_batched"):
        probs, r = c["probs"], dict(A=[], B=[], C={}, acc={}, prior={}, shift=0, out_shift=0)
        for i, (m, n, k, d) in enumerate(probs):
            A, B = GR.dyadic((k, m), seed + 10 * i), GR.dyadic((k, n), seed + 10 * i + 1)
            if drop_k is not None:
                B = _drop(B, 1, k - 1 if drop_k < 0 else drop_k)
            r["A"].append(A.to(torch.bfloat16)); r["B"].append(B.to(torch.bfloat16))
            if d not in r["C"]:
                r["prior"][d] = GR.dyadic_ints((m, n), seed + 10 * d + 4) if c["acc"] else None
                r["C"][d] = torch.zeros(m, n, dtype=torch.float64) if r["prior"][d] is None else r["prior"][d].clone()
            r["C"][d] += A.t() @ B
        return r
    if e in ("conv", "conv_colstats"):
        n, Hp, Wp, C, stride, Ho, Wo = _conv_dims(c)
        x = GR.dyadic((n, Hp, Wp, C), seed)
        x[:, 0], x[:, -1], x[:, :, 0], x[:, :, -1] = 0, 0, 0, 0          # the border the convolution pads with
        w = _drop(GR.dyadic((N, K), seed + 1), 0, drop_k)
        r = dict(A=x.to(torch.bfloat16), B=w.to(torch.bfloat16), shift=0, out_shift=0, M=n * Ho * Wo)
        r["C"] = r["acc"] = r["pre"] = GR.conv_nhwc(x, w.reshape(N, 3, 3, C), stride, Ho, Wo)
        r["stats"] = GR.colstats(r["C"].to(out_dt).double(), c["block_rows"]) if e == "conv_colstats" else None
        return r
    if e == "conv_runs":
        n, Hp, Wp, pix, run, Ho, Wo, kh, stride = c["runs"]
        x = GR.dyadic((n, Hp, Wp, pix), seed)
        w = GR.dyadic((N, kh, run // pix, pix), seed + 1)
        w[:, :, 7:, :] = 0          # kx >= kw
        w[:, :, :, 3] = 0           # the padding channel
        w = _drop(w.reshape(N, K), 0, drop_k)
        r = dict(A=x.to(torch.bfloat16), B=w.to(torch.bfloat16), shift=0, out_shift=0, M=n * Ho * Wo, stats=None)
        r["C"] = r["acc"] = r["pre"] = GR.conv_runs(x, w.reshape(N, kh, run), stride, Ho, Wo)
        return r
    raise ValueError(e)


@functools.lru_cache(maxsize=None)
def reference(cid):
    """operands and float64 results of case `cid`: computed once, shared by the CPU and GPU tests, never written to"""
    return _build(BY_ID[cid])


def _outputs(r):
    return list(r["C"].values()) if isinstance(r["C"], dict) else [r["C"]]


def _last_live_k(c, k):
    """conv_runs: the run's last elements meet zero weights by construction; step back to the last index that carries one"""
    if c["entry"] == "conv_runs":
        while k % 32 >= 28 or k % 4 == 3:
            k -= 1
    return k


# ---- the conditions --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", IDS)
def test_every_stored_value_is_on_the_grid(cid):
    c, r = BY_ID[cid], reference(cid)
    out_dt = DT[c["out"]]
    lim = 256.0 if out_dt == torch.bfloat16 else F32_LIM
    for a in ([] if isinstance(r["acc"], dict) else [r["acc"]]):          # the accumulator: float32 partial sums in any order
        assert GR.on_grid(a, r["shift"], F32_LIM)
    if c["entry"] in ("gemm", "colblocks", "colstats"):
        assert GR.on_grid(r["pre"], r["shift"], lim if c["epi"] == "GELU" else F32_LIM)          # GELU stores it as aux
    for C in _outputs(r):
        if c["epi"] in EXACT_EPI:
            if c["entry"] == "fp8" and c["scale_hi"] > 0:          # n * 2^e: exact in bf16 through |n| alone
                assert GR.on_grid(r["acc"], 0, lim)
            else:
                assert GR.on_grid(C, r["out_shift"], lim), GR.max_n(C, r["out_shift"])
            assert torch.equal(C.to(out_dt).double(), C)
    for name in ("bias", "aux_in", "prior"):
        t = r.get(name)
        for v in (t.values() if isinstance(t, dict) else [t]):
            if v is not None:
                dt_ = torch.float32 if name in ("bias", "prior") else out_dt
                assert torch.equal(v.to(dt_).double(), v)
    if r.get("colsum") is not None:
        assert GR.on_grid(r["colsum"], r["out_shift"], F32_LIM)
    if r.get("stats") is not None:
        assert GR.on_grid(r["stats"], 2 * r["out_shift"], F32_LIM) and float(r["stats"][:, :, 1].max()) < 2 ** 24


@pytest.mark.parametrize("cid", IDS)
def test_outputs_are_mostly_nonzero_and_feel_every_contraction_index(cid):
    c, r = BY_ID[cid], reference(cid)
    outs = _outputs(r)
    for C in outs:
        assert float((C != 0).double().mean()) >= 0.30
    if c["entry"] in ("dw_list", "dw_batched"):
        drops = (-1, c["ktile"] - 1)
    else:
        drops = (_last_live_k(c, c["K"] - 1), _last_live_k(c, c["ktile"] - 1))
    for k in drops:
        for C, D in zip(outs, _outputs(_build(c, drop_k=k))):
            assert float((C != D).double().mean()) >= 0.25, (k, float((C != D).double().mean()))


def test_every_family_has_a_guarded_and_a_poisoned_case():
    fams = {c["family"] for c in CASES}
    assert fams == {"generic", "tile128", "small", "tile256", "tile192", "tile256k64", "tile192k64", "narrow", "fp8", "dw"}
    for f in fams - {"dw"}:
        assert any(c["family"] == f and c["pad_c"] > 0 and c["rows_extra"] == 3 and c["entry"] in ("gemm", "fp8", "colstats") for c in CASES), f
    names = {c["kernel"] for c in CASES}
    for n in ("gemm_generic_kernel", "gemm_bf16_kernel<0,0,bf16>", "gemm_bf16_small_kernel<bf16>", "gemm_bf16_tile256_kernel<0,0,bf16,NONE>",
              "gemm_bf16_tile256_kernel<1,1,f32,NONE>", "gemm_bf16_tile192_kernel<0,NONE>", "gemm_bf16_tile256k64_kernel<NONE>",
              "gemm_bf16_tile192k64_kernel<NONE>", "gemm_bf16_tile256k64_n64_kernel", "gemm_bf16_tile256k64_n128_kernel",
              "gemm_fp8_tile192_kernel<NONE>", "gemm_bf16_dw_batched_kernel"):
        assert n in names, n


def test_the_work_list_has_unsplit_rounds_a_tail_with_pieces_and_a_reduce():
    """fcmf_gemm_dw_list_plan (host only) for the problems of DW_LIST that the tile kernel takes, on 8 workgroups"""
    from test_dw_list_cpu import _plan
    taken = [p for p in DW_LIST if p[0] >= 256 and p[1] >= 256]
    first = {}
    mats = [(m, n, k, first.setdefault(d, i)) for i, (m, n, k, d) in enumerate(taken)]
    items, red, info = _plan(mats, cus=8)
    unsplit = items[items[:, 5] < 0]
    pieces = items[items[:, 5] >= 0]
    assert len(unsplit) >= 8 and set(unsplit[:, 0]) == {2}      # at least a round of tiles that write C themselves
    assert len(pieces) > 0 and len(red) > 0                     # the tail leaves partial tiles to the list reduce
    assert set(pieces[:, 0]) == {0, 1}                          # both producers of the shared destination are in the tail
    assert any(p[3] > 0 for p in pieces)                        # and a contraction is cut into pieces
    assert len(items) > 8                                       # more items than workgroups
