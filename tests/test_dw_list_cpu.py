"""The planner of the weight-gradient work list (fcmf_gemm_dw_list_plan: pure host code, no device): coverage, the
same-destination rule, the minimum piece depth, the workspace bound and the planned efficiency."""
import ctypes

import numpy as np
import pytest

CUS = 256
GB = 256
MIN_KT = 8


def _plan(mats, cus=CUS, ws_bytes=None):
    """mats: [(M, N, K, dest)] -> (items [n, 6], reduce [m, 5], info)"""
    from fcmf_framework import _hip
    ws_bytes = _hip.SPLITK_WORKSPACE_BYTES if ws_bytes is None else ws_bytes
    arr = lambda col: (ctypes.c_int * len(mats))(*[m[col] for m in mats])
    M, N, K, D = arr(0), arr(1), arr(2), arr(3)
    info = (ctypes.c_int64 * 6)()
    lib = _hip.lib()
    rc = lib.fcmf_gemm_dw_list_plan(len(mats), M, N, K, D, cus, ws_bytes, None, 0, None, 0, info)
    assert rc == 0, rc
    items = np.zeros((max(1, info[0]), 6), dtype=np.int32)
    red = np.zeros((max(1, info[1]), 5), dtype=np.int32)
    rc = lib.fcmf_gemm_dw_list_plan(len(mats), M, N, K, D, cus, ws_bytes, items.ctypes.data, len(items), red.ctypes.data, len(red), info)
    assert rc == 0, rc
    return items[:info[0]], red[:info[1]], list(info)


def _with_dest(mats, shared=()):
    """(M, N, K) triples -> + dest: index of the first matrix of its `shared` group, else itself"""
    out = []
    for i, m in enumerate(mats):
        grp = next((g for g in shared if i in g), None)
        out.append(tuple(m) + (min(grp) if grp else i,))
    return out


def bench_list():
    """the flush of the benchmarked step (FCMF-base, B = 64 x 6 aspects, seq 128, 7 images x 49 patches, 36 ROIs) as the entry
    point hands it to the planner, recorded from a benchmark run: 12 x the four encoder shapes at 49152 tokens, then the matrices
    outside the text encoder with their token counts (49152, 21952, 16128, 5760, 2688, 384).  The mm layer's weights have several
    uses -- key / value over the text rows (49152), the ROIs (16128) and the fusion layer (5760, the row panels of its fused
    query | key | value gradient), query at 384 and 5760, output / FFN at 2688 and 5760: groups of one destination."""
    H, I, T = 768, 3072, 49152
    mats, shared = [], []

    def add(M, N, K, group=None):
        if group is not None:
            while len(shared) <= group:
                shared.append(set())
            shared[group].add(len(mats))
        mats.append((M, N, K))

    add(H, I, 5760, 0); add(I, H, 5760, 1); add(H, H, 5760, 2)              # fusion layer: FFN out, FFN in, attention output
    add(H, H, 5760, 3); add(H, H, 5760, 4); add(H, H, 5760, 5)              # ... its query | key | value gradient, cut into row panels
    add(H, I, 2688, 0); add(I, H, 2688, 1); add(H, H, 2688, 2); add(H, H, 384, 3)   # mm layer, live row; mm query
    add(H, I, 2688); add(I, H, 2688); add(H, H, 2688); add(H, H, 384)       # cross layer, live row; cross query
    add(H, H, 16128, 4); add(H, H, 16128, 5)                                # mm key, value over the ROIs
    for _ in range(4):
        add(H, H, 16128)                                                    # box head
    add(H, 2048, 16128)                                                     # roimap2text
    add(H, H, 21952); add(H, H, 21952); add(H, 2048, 21952)                 # cross key, value over the patches; vismap2text
    add(H, H, T, 4); add(H, H, T, 5)                                        # mm key, value over the text rows
    for _ in range(12):
        add(H, I, T); add(I, H, T); add(3 * H, H, T); add(H, H, T)
    return _with_dest(mats, shared)


def small_lists():
    # ragged tiles, a token count that is no multiple of 32, and a shared destination with different token counts
    a = _with_dest([(512, 256, 2048)] * 5 + [(776, 520, 1000)] * 3 + [(256, 768, 4104)] * 2 + [(512, 512, 2688), (512, 512, 1024), (512, 512, 64)],
                   [{10, 11, 12}])
    # more tiles than workgroups at one depth: a whole unsplit round and a tail that cannot be split (8 k-tiles)
    b = _with_dest([(512, 512, 256)] * 65)
    return [a, b]


def _check(mats, cus=CUS, ws_bytes=None):
    items, red, info = _plan(mats, cus, ws_bytes)
    n_items, n_red, slots, table_bytes, ws_need, eff6 = info
    shared = {d for i, (_, _, _, d) in enumerate(mats) if d != i}
    is_shared = lambda m: mats[m][3] in shared
    cover = {}        # (matrix, tile row, tile column) -> k-tile hit counts
    direct = {}       # destination tile -> direct-write items
    slot_owner = {}
    for mat, tm, tn, k0, nkt, slot in items:
        M, N, K, dest = mats[mat]
        nk = (K + 31) // 32
        assert 0 <= tm < (M + GB - 1) // GB and 0 <= tn < (N + GB - 1) // GB and nkt >= 1 and 0 <= k0 and k0 + nkt <= nk
        cover.setdefault((mat, tm, tn), np.zeros(nk, dtype=np.int32))[k0:k0 + nkt] += 1
        if slot < 0:
            assert nkt == nk, "an item that writes C covers the whole contraction"
            assert not is_shared(mat), "a destination with several producers is workspace-only"
            direct[(dest, tm, tn)] = direct.get((dest, tm, tn), 0) + 1
        else:
            assert 0 <= slot < slots and slot not in slot_owner
            slot_owner[slot] = (dest, tm, tn)
        if nkt < nk:
            assert nkt >= MIN_KT, (mat, nkt, nk)
    # every (tile, k-tile) exactly once
    want = sum(((M + GB - 1) // GB) * ((N + GB - 1) // GB) for M, N, _, _ in mats)
    assert len(cover) == want
    assert all((c == 1).all() for c in cover.values())
    assert all(v == 1 for v in direct.values())
    # the reduce table: every slot in exactly one entry, an entry's slots all belong to its C tile, no tile both direct and reduced
    seen = set()
    for slot0, cnt, mat, tm, tn in red:
        assert cnt >= 1 and mats[mat][3] == mat
        for s in range(slot0, slot0 + cnt):
            assert s not in seen and slot_owner[s] == (mat, tm, tn)
            seen.add(s)
        assert (mat, tm, tn) not in direct
    assert seen == set(slot_owner) and len(seen) == slots
    assert len({(m, a, b) for _, _, m, a, b in red}) == n_red
    # workspace
    from fcmf_framework import _hip
    assert ws_need == table_bytes + slots * GB * GB * 4
    assert ws_need <= (_hip.SPLITK_WORKSPACE_BYTES if ws_bytes is None else ws_bytes)
    assert 16 * n_items + 16 * n_red + 64 * len(mats) <= table_bytes
    # efficiency as planned: item i runs on workgroup i % cus
    load = np.zeros(cus, dtype=np.int64)
    np.add.at(load, np.arange(n_items) % cus, items[:, 4])
    eff = load.mean() / load.max()
    assert abs(eff - eff6 / 1e6) < 1e-5
    return eff, info


def test_benchmark_list_plan():
    mats = bench_list()
    eff, info = _check(mats)
    print(f"benchmark list: {len(mats)} matrices, {info[0]} items, {info[1]} reduce entries, {info[2]} partial tiles "
          f"({info[2] * GB * GB * 4 / 2 ** 20:.0f} MiB), workspace need {info[4] / 2 ** 20:.1f} MiB, planned efficiency {eff:.4f}")
    assert eff >= 0.97, eff
    items, _, _ = _plan(mats)
    # five whole rounds of the 1536-deep encoder tiles run unsplit
    assert (items[:5 * CUS, 4] == 1536).all() and (items[:5 * CUS, 5] == -1).all()


@pytest.mark.parametrize("which", [0, 1])
def test_small_list_plans(which):
    mats = small_lists()[which]
    eff, info = _check(mats)
    print(f"small list {which}: {info[0]} items, {info[2]} partial tiles, planned efficiency {eff:.4f}")
    if which == 1:
        items, _, _ = _plan(mats)
        assert (items[:, 5] == -1).all() and len(items) == 260      # one unsplit round + 4 tiles too shallow to split


def test_plan_with_a_small_workspace():
    """a workspace that holds the tables and a few tiles: single producers run whole, the shared destination keeps its partial tiles;
    none at all: unsupported (the entry point then multiplies matrix by matrix)"""
    mats = small_lists()[0]
    eff, info = _check(mats, ws_bytes=2 * GB * GB * 4 + 12 * GB * GB * 4)
    assert info[2] == 12
    from fcmf_framework import _hip
    arr = lambda col: (ctypes.c_int * len(mats))(*[m[col] for m in mats])
    info = (ctypes.c_int64 * 6)()
    assert _hip.lib().fcmf_gemm_dw_list_plan(len(mats), arr(0), arr(1), arr(2), arr(3), CUS, 0, None, 0, None, 0, info) == -3
    bad = (ctypes.c_int * len(mats))(*([1] + [m[3] for m in mats[1:]]))     # dest[0] must be 0
    assert _hip.lib().fcmf_gemm_dw_list_plan(len(mats), arr(0), arr(1), arr(2), bad, CUS, 1 << 29, None, 0, None, 0, info) == -1
