"""The IAOG decoder's per-head projections (ops.head_linear: HeadLinearFn over ops.head_project / ops.head_project_bwd) on their
own against float64 autograd, and the library calls a whole decoder step makes."""
import pytest
import torch

from helpers import _calls_digest, _recorded, rel_err

pytestmark = pytest.mark.gpu

NH, E, D = 4, 256, 64      # the smallest sizes at which ops.head_weight_grad's own gate (E >= 256, N >= 256) lets the direct path be tried


def _rand(shape, dev, dtype=torch.float32, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype).to(dev)


def _set(dtype):
    from fcmf_framework import ops
    ops.set_compute_dtype(dtype)
    ops.shadows.clear()


# ------------------------------------------------------------------------------------------------------------------------
# the projection alone
# ------------------------------------------------------------------------------------------------------------------------
def _weights(dev, nw):
    return [torch.nn.Parameter(_rand((NH, E, D), dev, scale=E ** -0.5, seed=10 + i)) for i in range(nw)]


def _project(dev, dtype, ws, xshape=(3, 8, E), wide=0, unused=None):
    """ops.head_linear of a seeded input by the weights `ws`, and the backward of sum_i <y_i, g_i> (output `unused` left out)
    -> (outputs, x.grad, weights, the same four from torch.einsum on float64 CPU copies; bf16: on the bf16-rounded weights).
    wide: the input is the first E columns of a tensor with that many more (row stride E + wide)."""
    from fcmf_framework import ops
    full = _rand(xshape[:-1] + (E + wide,), dev, dtype, seed=1).requires_grad_(True)
    nw = len(ws)
    gs = [_rand(xshape[:-1] + (NH * D,), dev, dtype, seed=20 + i).float() for i in range(nw)]
    x = full[..., :E] if wide else full
    ys = ops.head_linear(x, *ws)
    assert isinstance(ys, torch.Tensor) if nw == 1 else (isinstance(ys, tuple) and len(ys) == nw)
    ys = (ys,) if nw == 1 else ys
    sum((y.float() * g).sum() for i, (y, g) in enumerate(zip(ys, gs)) if i != unused).backward()
    fr = full.detach().double().cpu().requires_grad_(True)
    wr = [w.detach().double().cpu().requires_grad_(True) for w in ws]
    wc = wr if dtype == torch.float32 else [w.bfloat16().double() for w in wr]
    yr = [torch.einsum('...e,hej->...hj', fr[..., :E], w).flatten(-2) for w in wc]
    sum((y * g.double().cpu()).sum() for i, (y, g) in enumerate(zip(yr, gs)) if i != unused).backward()
    return ys, full.grad, ws, yr, fr.grad, wr


def _check(dtype, got, skip_grad=None):
    ys, dx, ws, yr, dxr, wr = got
    tol = 3e-5 if dtype == torch.float32 else 4e-2
    for y, r in zip(ys, yr):
        assert y.shape == r.shape and y.dtype == dtype
        err = rel_err(y, r)
        print("output", err)
        assert err < tol
    err = rel_err(dx, dxr)
    print("x.grad", err)
    assert dx.shape == dxr.shape and err < tol * 2
    for i, (w, r) in enumerate(zip(ws, wr)):
        if i == skip_grad:      # (the weight of an unused output: no gradient in the reference, exact zeros from the shared zero block)
            assert r.grad is None and not w.grad.any()
            continue
        err = rel_err(w.grad, r.grad)
        print("w.grad", i, err)
        assert w.grad.shape == (NH, E, D) and err < tol * 2


VARIANTS = {"1w": dict(nw=1), "2w": dict(nw=2), "3w": dict(nw=3), "2d": dict(nw=2, xshape=(24, E)),
            "strided": dict(nw=2, wide=64), "unused": dict(nw=3, unused=1)}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_head_projection_matches_float64_autograd(dev, dtype, variant):
    """y_i[..., h*d + j] = sum_e x[..., e] w_i[h, e, j] for 1, 2 and 3 weights as one node (one forward, one dX and one dW GEMM): 24
    tokens of n_head=4, E=256, d=64; a 2-D input; an input whose rows are E + 64 apart (the padding columns get a zero gradient);
    an output that is never used (its gradient arrives as None and counts as zeros).  No arena: the weight gradients come from
    the plain [N, E] GEMM + permuted view."""
    _set(dtype)
    try:
        v = dict(VARIANTS[variant])
        got = _project(dev, dtype, _weights(dev, v.pop("nw")), **v)
        _check(dtype, got, skip_grad=v.get("unused"))
        if v.get("wide"):
            assert not got[1][..., E:].any()
    finally:
        _set(torch.float32)


@pytest.mark.parametrize("tokens", [24, 352, 360])
@pytest.mark.parametrize("nw", [1, 2, 3])
def test_head_projection_weight_gradients_in_the_arena(dev, nw, tokens):
    """bf16 under a dp.GradArena that holds the weights as one adjacent block: ops.head_weight_grad claims their slices and asks
    fcmf_gemm_colblocks to write dW straight into them in the parameters' [n_head, E, d] layout.
    At 24 tokens the library REFUSES (FCMF_ERR_UNSUPPORTED: the blocked layout is written by the split-K reduce pass, and the
    persistent kernel splits a contraction only into parts at least six 32-deep k-tiles long, so it takes 12 k-tiles -- more than
    352 tokens -- to split at all).  352 tokens are therefore refused as well, and 360 is the smallest multiple of 8 that is
    accepted, for every N = 256..768 here.  Accepted: every w.grad IS its arena slice.  Refused: the slices are given back
    (arena.release: a later claim is the first again) and the fallback GEMM's gradients are what autograd holds."""
    from fcmf_framework import _hip as H, dp
    _set(torch.bfloat16)
    arena = None
    try:
        ws = _weights(dev, nw)
        arena = dp.GradArena(ws, blocks=[ws])
        arena.zero()
        got = []
        calls = _recorded(lambda: got.append(_project(dev, torch.bfloat16, ws, xshape=(tokens // 8, 8, E))))
        rcs = [c[2] for c in calls if c[0] == "fcmf_gemm_colblocks"]
        print("fcmf_gemm_colblocks", tokens, "tokens ->", rcs)
        assert rcs == [0 if tokens == 360 else H.ERR_UNSUPPORTED]
        _check(torch.bfloat16, got[0])
        if tokens == 360:
            for w in ws:
                assert w.grad.data_ptr() == arena.view[id(w)].data_ptr()
        else:
            assert all(w.grad.data_ptr() != arena.view[id(w)].data_ptr() for w in ws)
            for w in ws:
                w.grad = None
            assert arena.claim(ws)[1]
    finally:
        if arena is not None:
            arena.deactivate()
        _set(torch.float32)


# ------------------------------------------------------------------------------------------------------------------------
# the decoder's library calls, in order
# ------------------------------------------------------------------------------------------------------------------------
def _decoder_calls(dev, case, desc=False):
    """[(entry point, scalar arguments, return code)] of one pass of a 2-block, 4-head, 256-wide IAOGDecoder over B = 3 sequences
    of 8 tokens and a [3, 16, 256] encoder output that requires grad.  case: "fp32" / "bf16" / "bf16-arena" (loss + backward, the
    last under GradArena.for_model) or "bf16-project" (project_encoder under no_grad).  desc: helpers._recorded's option"""
    from fcmf_framework import dp, ops
    from fcmf_framework.iaog_modeling import IAOGDecoder
    _set(torch.float32 if case == "fp32" else torch.bfloat16)
    ops.manual_seed(0)
    torch.manual_seed(0)
    m = IAOGDecoder(vocab_size=96, hidden_size=256, num_layers=2, num_heads=4).to(dev).train()
    g = torch.Generator().manual_seed(1)
    enc = torch.randn((3, 16, 256), generator=g).to(dev).requires_grad_(True)
    ids, labels = (torch.randint(0, 96, (3, 8), generator=g).to(dev) for _ in range(2))
    arena = dp.GradArena.for_model(m) if case == "bf16-arena" else None

    def run():
        if case == "bf16-project":
            with torch.no_grad():
                m.project_encoder(enc)
        else:
            m.loss(ids, m.init_state(enc, None), labels).backward()
    try:
        if arena is not None:
            arena.zero()
        return _recorded(run, desc=desc)
    finally:
        if arena is not None:
            arena.deactivate()
        _set(torch.float32)


# Entry-point names in call order, and the SHA-256 of repr([(name, scalar arguments, return code), ...]).  Both were generated by
# running _decoder_calls at the commit BEFORE the decoder's three projection nodes (HeadLinearFn, _SelfQuirkAttentionFn,
# _HoistedKeysFn) came to share ops.head_project / ops.head_project_bwd, not at the commit under test: the shared helpers have to
# issue what the three nodes issued.  (With 24 decoder and 48 encoder tokens every fcmf_gemm_colblocks call of "bf16-arena" is
# refused and followed by the fallback fcmf_gemm: the accepted direct path is what the 360-token test above covers.)
DECODER_CALLS = {
    "fp32": ("""
        fcmf_embed_scale_fwd fcmf_dropout fcmf_gemm fcmf_gemm fcmf_attn_small_fwd fcmf_gemm fcmf_add_ln_fwd
        fcmf_gemm fcmf_attn_small_fwd fcmf_gemm fcmf_add_ln_fwd fcmf_gemm fcmf_gemm fcmf_add_ln_fwd
        fcmf_gemm fcmf_attn_small_fwd fcmf_gemm fcmf_add_ln_fwd fcmf_gemm fcmf_attn_small_fwd fcmf_gemm
        fcmf_add_ln_fwd fcmf_gemm fcmf_gemm fcmf_add_ln_fwd fcmf_gemm fcmf_xent_fwd fcmf_xent_bwd fcmf_gemm
        fcmf_gemm fcmf_colsum fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_gemm fcmf_gemm fcmf_colsum
        fcmf_gemm fcmf_gemm fcmf_colsum fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_gemm fcmf_gemm
        fcmf_colsum fcmf_attn_small_bwd fcmf_head_gather fcmf_head_gather fcmf_gemm fcmf_gemm
        fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_gemm fcmf_gemm fcmf_colsum fcmf_attn_small_bwd
        fcmf_head_gather fcmf_head_gather fcmf_gemm fcmf_gemm fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd
        fcmf_gemm fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm fcmf_colsum fcmf_add_ln_bwd_workspace
        fcmf_add_ln_bwd fcmf_gemm fcmf_gemm fcmf_colsum fcmf_attn_small_bwd fcmf_head_gather
        fcmf_head_gather fcmf_gemm fcmf_gemm fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_gemm fcmf_gemm
        fcmf_colsum fcmf_attn_small_bwd fcmf_head_gather fcmf_head_gather fcmf_gemm fcmf_gemm fcmf_gemm
        fcmf_gemm fcmf_dropout fcmf_embed_scale_bwd
        """, "20c865cbaed41f11b17fb06b699f7f9bd172e10f04dd1f268f4d6121bd9dfea4"),
    "bf16": ("""
        fcmf_embed_scale_fwd fcmf_dropout fcmf_cast fcmf_multi_cast_transpose fcmf_gemm
        fcmf_multi_cast_transpose fcmf_gemm fcmf_attn_small_fwd fcmf_cast fcmf_gemm fcmf_add_ln_fwd
        fcmf_cast fcmf_multi_cast_transpose fcmf_gemm fcmf_attn_small_fwd fcmf_cast fcmf_gemm
        fcmf_add_ln_fwd fcmf_cast fcmf_cast fcmf_gemm fcmf_gemm fcmf_add_ln_fwd fcmf_multi_cast_transpose
        fcmf_gemm fcmf_attn_small_fwd fcmf_cast fcmf_gemm fcmf_add_ln_fwd fcmf_cast
        fcmf_multi_cast_transpose fcmf_gemm fcmf_attn_small_fwd fcmf_cast fcmf_gemm fcmf_add_ln_fwd
        fcmf_cast fcmf_cast fcmf_gemm fcmf_gemm fcmf_add_ln_fwd fcmf_cast fcmf_gemm fcmf_xent_fwd
        fcmf_xent_bwd fcmf_gemm fcmf_gemm fcmf_colsum fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd
        fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_colsum fcmf_cast_transpose fcmf_gemm fcmf_gemm
        fcmf_colsum fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_cast_transpose fcmf_gemm fcmf_gemm
        fcmf_colsum fcmf_attn_small_bwd fcmf_head_gather fcmf_head_gather fcmf_gemm fcmf_gemm
        fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_colsum
        fcmf_attn_small_bwd fcmf_head_gather fcmf_head_gather fcmf_gemm fcmf_gemm fcmf_add_ln_bwd_workspace
        fcmf_add_ln_bwd fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_colsum fcmf_cast_transpose fcmf_gemm
        fcmf_gemm fcmf_colsum fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_cast_transpose fcmf_gemm
        fcmf_gemm fcmf_colsum fcmf_attn_small_bwd fcmf_head_gather fcmf_head_gather fcmf_gemm fcmf_gemm
        fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_colsum
        fcmf_attn_small_bwd fcmf_head_gather fcmf_head_gather fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm
        fcmf_cast fcmf_dropout fcmf_embed_scale_bwd
        """, "9c9e2f64c8c3ee26d98b64e3aad34529795f405ff8136071e2ddb05581fc7430"),
    "bf16-arena": ("""
        fcmf_embed_scale_fwd fcmf_dropout fcmf_cast fcmf_multi_cast_transpose fcmf_gemm
        fcmf_multi_cast_transpose fcmf_gemm fcmf_attn_small_fwd fcmf_cast fcmf_gemm fcmf_add_ln_fwd
        fcmf_cast fcmf_multi_cast_transpose fcmf_gemm fcmf_attn_small_fwd fcmf_cast fcmf_gemm
        fcmf_add_ln_fwd fcmf_cast fcmf_cast fcmf_gemm fcmf_gemm fcmf_add_ln_fwd fcmf_multi_cast_transpose
        fcmf_gemm fcmf_attn_small_fwd fcmf_cast fcmf_gemm fcmf_add_ln_fwd fcmf_cast
        fcmf_multi_cast_transpose fcmf_gemm fcmf_attn_small_fwd fcmf_cast fcmf_gemm fcmf_add_ln_fwd
        fcmf_cast fcmf_cast fcmf_gemm fcmf_gemm fcmf_add_ln_fwd fcmf_cast fcmf_gemm fcmf_xent_fwd
        fcmf_xent_bwd fcmf_gemm fcmf_gemm fcmf_colsum fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd
        fcmf_cast_transpose fcmf_gemm fcmf_colsum fcmf_cast_transpose fcmf_gemm fcmf_colsum
        fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_cast_transpose fcmf_gemm fcmf_colsum
        fcmf_attn_small_bwd fcmf_head_gather fcmf_head_gather fcmf_gemm fcmf_gemm_colblocks fcmf_gemm
        fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_cast_transpose fcmf_gemm fcmf_colsum
        fcmf_attn_small_bwd fcmf_head_gather fcmf_head_gather fcmf_gemm fcmf_gemm_colblocks fcmf_gemm
        fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_cast_transpose fcmf_gemm fcmf_colsum
        fcmf_cast_transpose fcmf_gemm fcmf_colsum fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd
        fcmf_cast_transpose fcmf_gemm fcmf_colsum fcmf_attn_small_bwd fcmf_head_gather fcmf_head_gather
        fcmf_gemm fcmf_gemm_colblocks fcmf_gemm fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd
        fcmf_cast_transpose fcmf_gemm fcmf_colsum fcmf_attn_small_bwd fcmf_head_gather fcmf_head_gather
        fcmf_gemm fcmf_gemm_colblocks fcmf_gemm fcmf_gemm fcmf_gemm_colblocks fcmf_gemm fcmf_cast
        fcmf_dropout fcmf_embed_scale_bwd fcmf_gemm_dw_batched
        """, "f504e803dff287395d743b3a030fb017016a4f52d25bfc8f39387f030fc74b24"),
    "bf16-project": ("""
        fcmf_cast fcmf_multi_cast_transpose fcmf_gemm
        """, "aedc90daf5af28907fcde7235742ef7b0dd9698b07e758c341488855e99a25cc"),
}


@pytest.mark.parametrize("case", ["fp32", "bf16", "bf16-arena", "bf16-project"])
def test_decoder_library_call_sequence(dev, case):
    calls = _decoder_calls(dev, case)
    names = [c[0] for c in calls]
    print("MEASURED", case, len(names), _calls_digest(calls))
    exp_names, exp_digest = DECODER_CALLS[case]
    assert names == exp_names.split()
    assert _calls_digest(calls) == exp_digest
