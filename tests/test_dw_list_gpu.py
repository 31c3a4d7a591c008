"""fcmf_gemm_dw_list: weight gradients of mixed shapes as ONE work list (unsplit whole rounds, a split tail, one reduce launch),
against the float64 product of the same bf16 operands and against per-matrix ops.gemm.  Bounds as in
test_gemm_dw_batched_matches_separate_weight_gradients: rel_err < 2e-3 against float64, < 1e-5 against the separate GEMMs."""
import ctypes

import pytest
import torch

from helpers import rel_err

pytestmark = pytest.mark.gpu


def _ops():
    from fcmf_framework import ops, _hip
    return ops, _hip


def _rand(shape, dev, dtype=torch.float32, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).to(dtype).to(dev)


def _problems(spec, dev):
    """spec: [(count, M, N, tokens)] -> [(dY [tokens, M], X [tokens, N])]"""
    out = []
    for count, M, N, tok in spec:
        for _ in range(count):
            i = len(out)
            out.append((_rand((tok, M), dev, torch.bfloat16, seed=10 + i), _rand((tok, N), dev, torch.bfloat16, seed=500 + i)))
    return out


def _run_list(H, probs, dests, acc):
    n = len(probs)
    ptrs = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])
    ints = lambda vs: (ctypes.c_int * n)(*vs)
    i64s = lambda vs: (ctypes.c_int64 * n)(*vs)
    M = [dy.shape[1] for dy, _ in probs]
    N = [x.shape[1] for _, x in probs]
    K = [x.shape[0] for _, x in probs]
    ctx = H.gemm_ctx(workspace=True)
    H.check(H.lib().fcmf_gemm_dw_list(ctx, n, ptrs([p[0] for p in probs]), ptrs([p[1] for p in probs]), ptrs(dests), ints(M), ints(N), ints(K),
                                      i64s(M), i64s(N), i64s(N), int(acc), H.stream()), "fcmf_gemm_dw_list")
    return H.last_gemm_kernel()


def _check_separate(ops, probs, got, acc, dev, idx=None):
    """every matrix against the float64 product and the separate GEMM"""
    for i, (dy, x) in enumerate(probs):
        if idx is not None and i not in idx:
            continue
        M, N, K = dy.shape[1], x.shape[1], x.shape[0]
        base = _rand((M, N), dev, seed=900 + i) if acc else None
        want = base.clone() if acc else torch.full((M, N), float("nan"), device=dev)
        ops.gemm(dy, x, want, M, N, K, M, N, N, 1, 1, acc=bool(acc))
        ref = dy.double().t() @ x.double()
        if acc:
            ref = ref + base.double()
        assert torch.isfinite(got[i]).all(), i
        e64, esep = rel_err(got[i], ref), rel_err(got[i], want)
        print(f"matrix {i} [{M} x {N}, {K} tokens]: rel_err {e64:.2e} (float64), {esep:.2e} (separate GEMM)")
        assert e64 < 2e-3 and esep < 1e-5, (i, e64, esep)


def _outputs(probs, acc, dev):
    return [_rand((dy.shape[1], x.shape[1]), dev, seed=900 + i) if acc else torch.full((dy.shape[1], x.shape[1]), float("nan"), device=dev)
            for i, (dy, x) in enumerate(probs)]


MIXED = [(5, 512, 256, 2048), (3, 776, 520, 1000), (2, 256, 768, 4104)]


@pytest.mark.parametrize("acc", [1, 0])
def test_mixed_shapes_in_one_list(dev, acc):
    """three shapes in one call: ragged tiles (776 x 520), a token count that is no multiple of 32 (1000); accumulate onto random C,
    or overwrite NaN-filled C.  Twice: the outputs are bit-identical (plain stores, fixed summation order)."""
    ops, H = _ops()
    probs = _problems(MIXED, dev)
    got = _outputs(probs, acc, dev)
    assert _run_list(H, probs, got, acc) == "gemm_bf16_dw_batched_kernel"
    _check_separate(ops, probs, got, acc, dev)
    again = _outputs(probs, acc, dev)
    _run_list(H, probs, again, acc)
    for a, b in zip(got, again):
        assert torch.equal(a, b)


def test_more_tiles_than_workgroups(dev):
    """65 x (512 x 512, 256 tokens) = 260 tiles on 256 workgroups: a whole unsplit round and a tail in one list"""
    ops, H = _ops()
    probs = _problems([(65, 512, 512, 256)], dev)
    got = _outputs(probs, 1, dev)
    assert _run_list(H, probs, got, 1) == "gemm_bf16_dw_batched_kernel"
    _check_separate(ops, probs, got, 1, dev, idx={0, 31, 63, 64})


@pytest.mark.parametrize("producers", [2, 3])
@pytest.mark.parametrize("acc", [1, 0])
def test_several_producers_of_one_destination(dev, producers, acc):
    """a weight applied several times: producers with different token counts (2688, 1024, 2688) name the same C, which receives
    their sum (plus C when accumulating) -- beside two matrices of their own"""
    ops, H = _ops()
    M, N = 512, 768
    toks = [2688, 1024, 2688][:producers]
    probs = _problems([(1, M, N, t) for t in toks] + [(2, 256, 512, 2048)], dev)
    base = _rand((M, N), dev, seed=77)
    shared = base.clone() if acc else torch.full((M, N), float("nan"), device=dev)
    own = _outputs(probs, acc, dev)[producers:]
    dests = [shared] * producers + own
    assert _run_list(H, probs, dests, acc) == "gemm_bf16_dw_batched_kernel"
    ref = sum(dy.double().t() @ x.double() for dy, x in probs[:producers])
    want = base.clone() if acc else torch.zeros((M, N), device=dev)
    for dy, x in probs[:producers]:
        ops.gemm(dy, x, want, M, N, x.shape[0], M, N, N, 1, 1, acc=True)
    if acc:
        ref = ref + base.double()
    assert torch.isfinite(shared).all()
    e64, esep = rel_err(shared, ref), rel_err(shared, want)
    print(f"{producers} producers, acc {acc}: rel_err {e64:.2e} (float64), {esep:.2e} (separate GEMMs)")
    assert e64 < 2e-3 and esep < 1e-5
    for i, g in enumerate(own):
        dy, x = probs[producers + i]
        assert rel_err(g, dy.double().t() @ x.double() + (_rand(g.shape, dev, seed=900 + producers + i).double() if acc else 0)) < 2e-3


def test_hundred_matrices(dev):
    """more matrices than the 32-entry pointer table of the same-shape kernel held: 100 x (256 x 256, 512 tokens)"""
    ops, H = _ops()
    probs = _problems([(100, 256, 256, 512)], dev)
    got = _outputs(probs, 0, dev)
    assert _run_list(H, probs, got, 0) == "gemm_bf16_dw_batched_kernel"
    _check_separate(ops, probs, got, 0, dev, idx={0, 31, 32, 33, 64, 99})
    for i, (dy, x) in enumerate(probs):
        assert rel_err(got[i], dy.float().t() @ x.float()) < 2e-3, i


def test_list_with_a_refused_shape(dev):
    """a 128 x 768 matrix (the tile kernel takes 256 rows and more) among ones it takes: multiplied inside the call all the same"""
    ops, H = _ops()
    probs = _problems([(2, 512, 256, 2048), (1, 128, 768, 2048), (2, 256, 768, 1000)], dev)
    got = _outputs(probs, 1, dev)
    _run_list(H, probs, got, 1)
    _check_separate(ops, probs, got, 1, dev)


def test_fused_destination_over_shared_slices(dev):
    """the fusion layer's case: one producer writes a fused [768, 512] block whose three 256-row slices are destinations of their
    own with further producers (other token counts).  The entry point cuts the fused producer into row panels; every slice
    receives the sum of its producers on top of what it held."""
    ops, H = _ops()
    N = 512
    block = _rand((768, N), dev, seed=5)
    base = block.clone()
    fused = (_rand((1000, 768), dev, torch.bfloat16, seed=1), _rand((1000, N), dev, torch.bfloat16, seed=2))
    parts = [(_rand((2048, 256), dev, torch.bfloat16, seed=3), _rand((2048, N), dev, torch.bfloat16, seed=4)),       # rows 0..255
             (_rand((520, 256), dev, torch.bfloat16, seed=6), _rand((520, N), dev, torch.bfloat16, seed=7))]         # rows 512..767
    own = _problems([(2, 256, 768, 1024)], dev)
    own_out = _outputs(own, 1, dev)
    probs = [fused] + parts + own
    dests = [block, block[0:256], block[512:768]] + own_out
    assert _run_list(H, probs, dests, 1) == "gemm_bf16_dw_batched_kernel"
    ref = base.double() + fused[0].double().t() @ fused[1].double()
    ref[0:256] += parts[0][0].double().t() @ parts[0][1].double()
    ref[512:768] += parts[1][0].double().t() @ parts[1][1].double()
    want = base.clone()
    ops.gemm(fused[0], fused[1], want, 768, N, 1000, 768, N, N, 1, 1, acc=True)
    ops.gemm(parts[0][0], parts[0][1], want[0:256], 256, N, 2048, 256, N, N, 1, 1, acc=True)
    ops.gemm(parts[1][0], parts[1][1], want[512:768], 256, N, 520, 256, N, N, 1, 1, acc=True)
    e64, esep = rel_err(block, ref), rel_err(block, want)
    print(f"fused destination: rel_err {e64:.2e} (float64), {esep:.2e} (separate GEMMs)")
    assert torch.isfinite(block).all() and e64 < 2e-3 and esep < 1e-5
    _check_separate(ops, own, own_out, 1, dev)
