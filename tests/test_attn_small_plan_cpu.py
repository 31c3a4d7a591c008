"""The host plan of the VALU attention (fcmf_attn_small_plan: pure host code, no device): which kernel every row of
test_ops_gpu.ATTN_CASES goes to, the boundaries between the kernel families, the LDS layout of the dense kernels and the float32
key limit.  The kernel names and sizes below were recorded from the dispatch of the commit BEFORE the plan existed
(tools/attn_small_dispatch_probe.cpp linked against that commit's attn_small.o): they are not computed by the code under test."""
import pytest

from test_ops_gpu import ATTN_CASES

F32, BF16 = 0, 1
OK, UNSUPPORTED = 0, -3
FWD = "attn_small_fwd_kernel<%s>"
BWD = "attn_small_bwd_kernel<%s>"
PRIV = " + attn_private_grad_kernel<%s>"
TINY_F, TINY_FW, TINY_B, TINY_BB = "attn_tiny_fwd_kernel<false>", "attn_tiny_fwd_kernel<true>", "attn_tiny_bwd_kernel", "attn_tiny_bwd_blocked_kernel"
FLAT_F, FLAT_B = "attn_rows_flat_fwd_kernel", "attn_rows_flat_bwd_kernel" + PRIV % "bf16_t"

# one row per row of ATTN_CASES: (float32 forward, float32 backward, bf16 forward, bf16 backward); the backward as ops.attention
# calls it (dbias with a bias, dv1 present, the grouped entry point whenever there are private keys and group_div <= 8)
KERNELS = [
    (FWD % "float, 4, 0", BWD % "float, true, false", TINY_F, TINY_B),
    (FWD % "float, 4, 0", BWD % "float, true, true" + PRIV % "float", FLAT_F, FLAT_B),
    (FWD % "float, 4, 0", BWD % "float, true, true" + PRIV % "float", FLAT_F, FLAT_B),
    (FWD % "float, 4, 0", BWD % "float, true, false", FWD % "bf16_t, 4, 0", BWD % "bf16_t, true, false"),
    (FWD % "float, 4, 0", BWD % "float, true, false", TINY_F, TINY_B),
    (FWD % "float, 4, 0", BWD % "float, true, false", FWD % "bf16_t, 4, 0", BWD % "bf16_t, true, false"),
    (FWD % "float, 4, 64", BWD % "float, true, true" + PRIV % "float", FLAT_F, FLAT_B),
    (FWD % "float, 4, 0", BWD % "float, true, false", FWD % "bf16_t, 4, 0", BWD % "bf16_t, true, false"),
    (FWD % "float, 4, 64", BWD % "float, false, true" + PRIV % "float", FWD % "bf16_t, 4, 64", BWD % "bf16_t, false, true" + PRIV % "bf16_t"),
    (FWD % "float, 4, 0", BWD % "float, true, true" + PRIV % "float", FWD % "bf16_t, 4, 0", BWD % "bf16_t, true, true" + PRIV % "bf16_t"),
    (FWD % "float, 4, 64", BWD % "float, true, true" + PRIV % "float", FLAT_F, FLAT_B),
    (FWD % "float, 4, 64", BWD % "float, true, true" + PRIV % "float", FLAT_F, FLAT_B),
    (FWD % "float, 4, 64", BWD % "float, true, true" + PRIV % "float", FLAT_F, FLAT_B),
    (FWD % "float, 4, 0", BWD % "float, true, false", FLAT_F, BWD % "bf16_t, true, false"),
    (FWD % "float, 4, 0", BWD % "float, true, false", TINY_F, TINY_B),
    (FWD % "float, 4, 0", BWD % "float, true, false", TINY_F, TINY_B),
    (FWD % "float, 4, 64", BWD % "float, false, false", TINY_F, TINY_B),
    (FWD % "float, 4, 64", BWD % "float, false, false", TINY_F, TINY_BB),
    (FWD % "float, 4, 0", BWD % "float, false, false", TINY_FW, TINY_BB),
    (FWD % "float, 4, 0", BWD % "float, false, false", TINY_FW, TINY_BB),
    (FWD % "float, 4, 64", BWD % "float, false, false", TINY_FW, TINY_BB),
    (FWD % "float, 4, 0", BWD % "float, false, false", FWD % "bf16_t, 4, 0", TINY_BB),
    (FWD % "float, 4, 0", BWD % "float, true, false", TINY_FW, TINY_BB),
    (FWD % "float, 4, 0", BWD % "float, false, false", TINY_F, TINY_BB),
    (FWD % "float, 4, 64", BWD % "float, false, false", FWD % "bf16_t, 4, 64", BWD % "bf16_t, false, false"),
    (FWD % "float, 4, 0", BWD % "float, true, true" + PRIV % "float", FWD % "bf16_t, 4, 0", BWD % "bf16_t, false, true" + PRIV % "bf16_t"),
    (FWD % "float, 4, 64", BWD % "float, true, true" + PRIV % "float", FLAT_F, FLAT_B),
    (FWD % "float, 4, 0", BWD % "float, true, true" + PRIV % "float", FLAT_F, FLAT_B),
    (FWD % "float, 4, 64", BWD % "float, true, true" + PRIV % "float", FWD % "bf16_t, 4, 64", BWD % "bf16_t, true, true" + PRIV % "bf16_t"),
]
I_KERNEL, I_GX, I_GY, I_SMEM, I_RB, I_TLP, I_KVF, I_KERNEL2, I_G2X, I_G2Y, I_SMEM2 = range(11)


def _desc(dtype, G, R, heads, d, T1, T2, gd, mask=False, bias=False, causal=False):
    """dense strides, fake 16-byte aligned addresses: the plan reads no memory"""
    from fcmf_framework import _hip
    a = _hip.AttnDesc()
    HD = heads * d
    a.dtype, a.G, a.heads, a.d, a.R, a.T1, a.T2, a.group_div = dtype, G, heads, d, R, T1, T2, gd
    a.q_sg, a.q_sr, a.o_sg, a.o_sr = R * HD, HD, R * HD, HD
    a.q = 0x10000000
    if T1:
        a.k1_sg, a.k1_st, a.k1, a.v1 = T1 * HD, HD, 0x20000000, 0x28000000
    if T2:
        a.k2_sg, a.k2_sr, a.k2_st, a.k2, a.v2 = R * T2 * HD, T2 * HD, HD, 0x30000000, 0x38000000
    a.mask = 0x78000000 if mask else None
    a.bias = 0x80000000 if bias else None
    a.scale, a.dropout_p, a.seed, a.causal = 0.125, 0.1, 1234, int(causal)
    return a


def _plans(case, dtype, aligned=True):
    """-> (forward, backward) plans of a row of ATTN_CASES, each (rc, info, 'kernel' or 'kernel + follow-up kernel')"""
    from fcmf_framework import attn
    G, R, heads, d, T1, T2, gd, mask, bias, causal = case
    a = _desc(dtype, G, R, heads, d, T1, T2, gd, mask, bias, causal)
    grouped = T2 > 0 and gd <= 8 and G % gd == 0
    out = []
    for rc, info, names in (attn.small_plan(a, ptrs_aligned=aligned), attn.small_plan(a, True, grouped, bias, True, aligned)):
        out.append((rc, info, None if rc else names[0] + (" + " + names[1] if names[1] else "")))
    return out


def dense_lds(R, rows, T1, T2, d, backward, frag_pad):
    """the LDS layout of the tiny / rows_flat kernels as csrc/attn_small.hip documents it -> [(array, first byte, bytes)]:
    bf16 images with row pitch d + 8 (Q, dO in the backward, K, V), then float32 arrays with row pitch T1 + T2 + 1 (PD [rows]; in
    the backward also DS [rows] and delta [R]), then the pad that keeps the 15 rows a score fragment may read past the last image
    inside the allocation"""
    dp, TP = d + 8, T1 + T2 + 1
    arrays = [("q", R * dp * 2)] + ([("dout", R * dp * 2)] if backward else []) + [("k", T1 * dp * 2), ("v", T1 * dp * 2)]
    arrays += [("pd", rows * TP * 4)] + ([("ds", rows * TP * 4), ("delta", R * 4)] if backward else [])
    behind = 4 * (2 * min(R, 16) * TP + R) if backward else T1 * dp * 2 + 4 * R * TP
    arrays.append(("pad", max(0, 15 * dp * 2 - behind) if frag_pad else 0))
    out, at = [], 0
    for name, n in arrays:
        out.append((name, at, n))
        at += n
    return out


def test_cases_run_on_the_kernels_they_ran_on_before_the_plan():
    assert len(KERNELS) == len(ATTN_CASES)
    for case, want in zip(ATTN_CASES, KERNELS):
        for dtype, (wf, wb) in ((F32, want[:2]), (BF16, want[2:])):
            (rf, _, nf), (rb, _, nb) = _plans(case, dtype)
            assert (rf, rb) == (OK, OK), (case, dtype)
            assert (nf, nb) == (wf, wb), (case, dtype)


def test_every_plan_fits_the_lds_and_dense_plans_match_the_documented_layout():
    dense = 0
    for case in ATTN_CASES:
        G, R, heads, d, T1, T2, gd = case[:7]
        for dtype in (F32, BF16):
            for backward, (rc, info, name) in enumerate(_plans(case, dtype)):
                assert rc == OK and 0 < info[I_SMEM] <= 160 * 1024, (case, dtype, backward)
                assert info[I_GX] == G * heads and info[I_GY] == (max(1, (T1 + 127) // 128) if "small_bwd" in name else 1)
                if "tiny" in name or "flat" in name:
                    rows = info[I_RB] if "blocked" in name else R
                    lay = dense_lds(R, rows, T1, T2, d, bool(backward), "tiny" in name)
                    assert lay[-1][1] + lay[-1][2] == info[I_SMEM], (case, name, lay, info)
                    assert info[I_SMEM] <= (160 if "tiny" in name else 64) * 1024
                    dense += 1
    assert dense >= 30


def test_layout_bytes_worked_by_hand():
    """36 x 36 at d 96 (pitches 104 and 37), 100 x 100 at d 128 (136, 101; backward in two blocks of 50 rows), 7 rows against
    128 + 36 keys at d 64 (72, 165)"""
    from fcmf_framework import attn
    box = _desc(BF16, 4, 36, 8, 96, 36, 0, 1, bias=True)
    assert attn.small_plan(box)[1][I_SMEM] == (36 + 2 * 36) * 104 * 2 + 4 * 36 * 37 == 27792
    assert attn.small_plan(box, True, False, True)[1][I_SMEM] == (2 * 36 + 2 * 36) * 104 * 2 + 4 * (2 * 36 * 37 + 36) == 40752
    large = _desc(BF16, 2, 100, 8, 128, 100, 0, 1, bias=True)
    assert attn.small_plan(large)[1][I_SMEM] == 300 * 136 * 2 + 4 * 100 * 101 == 122000
    rc, info, names = attn.small_plan(large, True, False, True)
    assert (rc, info[I_RB], info[I_SMEM], names[0]) == (OK, 50, 400 * 136 * 2 + 4 * (2 * 50 * 101 + 100), TINY_BB) and info[I_SMEM] == 149600
    mm = _desc(BF16, 12, 7, 3, 64, 128, 36, 6, mask=True)
    assert attn.small_plan(mm)[1][I_SMEM] == (7 + 2 * 128) * 72 * 2 + 4 * 7 * 165 == 42492
    rc, info, names = attn.small_plan(mm, True, True)
    assert (rc, info[I_SMEM]) == (OK, (14 + 2 * 128) * 72 * 2 + 4 * (2 * 7 * 165 + 7)) and info[I_SMEM] == 48148
    assert names == ("attn_rows_flat_bwd_kernel", "attn_private_grad_kernel<bf16_t>")
    assert info[I_KERNEL2:] == [info[I_KERNEL2], 2 * 7, 4, 4 * 2 * 6 * 3 * 36] and info[I_SMEM2] == 5184


def test_boundaries_between_the_families():
    from fcmf_framework import attn
    names = lambda a, *args, **kw: attn.small_plan(a, *args, **kw)[2][0]
    # 64 rows x 64 keys: the last one-block tiny backward; one row more: the row-blocked kernel (all 65 rows in one block)
    assert names(_desc(BF16, 2, 64, 2, 64, 64, 0, 1), True) == TINY_B
    rc, info, n = attn.small_plan(_desc(BF16, 2, 65, 2, 64, 64, 0, 1), True)
    assert (n[0], info[I_RB], info[I_SMEM]) == (TINY_BB, 65, 71212)
    assert names(_desc(BF16, 2, 65, 2, 64, 64, 0, 1)) == TINY_F              # (the wide forward is for > 64 KEYS)
    assert names(_desc(BF16, 2, 64, 2, 64, 65, 0, 1)) == TINY_FW
    # 128 x 128 with heads of 128: the forward's images no longer fit (general kernel), the backward runs in blocks of 22 rows
    a = _desc(BF16, 2, 128, 1, 128, 128, 0, 1, mask=True)
    rc, info, n = attn.small_plan(a)
    assert (n[0], info[I_RB], info[I_SMEM], info[I_KVF]) == (FWD % "bf16_t, 4, 0", 16, 81920, 17408)
    rc, info, n = attn.small_plan(a, True)
    assert (n[0], info[I_RB], info[I_SMEM]) == (TINY_BB, 22, 162480) and -(-128 // 22) == 6
    # 129 rows: the general kernels
    a = _desc(BF16, 2, 129, 2, 64, 64, 0, 1, mask=True)
    assert (names(a), names(a, True)) == (FWD % "bf16_t, 4, 64", BWD % "bf16_t, false, false")
    # the flat kernels take 16 rows, not 17; and only what fits 64 KiB (heads of 128 against 100 keys do not)
    a16, a17, wide = (_desc(BF16, 2, R, 2, d, 100, 20, 1, mask=True) for R, d in ((16, 64), (17, 64), (16, 128)))
    assert attn.small_plan(a16)[1][I_SMEM] == 38848 and attn.small_plan(a16, True, True)[1][I_SMEM] == 48960
    assert (names(a16), names(a16, True, True)) == (FLAT_F, "attn_rows_flat_bwd_kernel")
    assert (names(a17), names(a17, True, True)) == (FWD % "bf16_t, 4, 64", BWD % "bf16_t, true, true")
    assert (names(wide), names(wide, True, True)) == (FWD % "bf16_t, 4, 0", BWD % "bf16_t, false, true")
    assert names(a16, True, False) == BWD % "bf16_t, true, false"             # private keys, ungrouped entry point: general
    # an output / gradient pointer that is not 16-byte aligned: tiny and flat give way to the general kernels
    box = _desc(BF16, 4, 36, 8, 96, 36, 0, 1, bias=True)
    assert (names(box, ptrs_aligned=False), names(box, True, False, True, True, False)) == (FWD % "bf16_t, 4, 0", BWD % "bf16_t, true, false")
    assert (names(a16, ptrs_aligned=False), names(a16, True, True, False, True, False)) == (FWD % "bf16_t, 4, 64", BWD % "bf16_t, true, true")
    # groups of 16 share private keys: not the grouped entry point's business
    a = _desc(BF16, 16, 3, 2, 16, 10, 7, 16, mask=True)
    rc, info, n = attn.small_plan(a, True, True)
    assert rc == UNSUPPORTED and info[I_KERNEL] == -1 and n == (None, None)
    assert attn.small_plan(_desc(BF16, 4, 36, 8, 96, 36, 0, 1), True, True)[0] == UNSUPPORTED      # grouped without private keys
    # more keys than the LDS holds in float32 / a bad descriptor
    assert attn.small_plan(_desc(F32, 1, 1, 1, 128, 151, 0, 1))[0] == UNSUPPORTED
    assert attn.small_plan(_desc(F32, 1, 1, 1, 128, 513, 0, 1))[0] == -1


@pytest.mark.parametrize("d,limit", [(16, 512), (64, 285), (96, 199), (128, 150)])
def test_float32_key_limit(d, limit):
    from fcmf_framework import attn, ops
    assert attn.valu_float32_key_limit(d) == limit == ops.valu_float32_key_limit(d)
