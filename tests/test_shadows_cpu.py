"""The bookkeeping of the weight-shadow cache (fcmf_framework/shadows.py) without a GPU: a stand-in for the library records
(entry point, scalar arguments) and returns 0, so what is checked is WHEN a copy is built, for whom, and when it is dropped.
The values of the copies are checked on the GPU (test_shadows_gpu.py)."""
import ctypes
import gc

import pytest
import torch

from fcmf_framework import _hip as H, fused, ops

KINDS = ["get", "padded", "get_t", "get_fp8", "get_fp8_t", "head_nk", "derived"]
SHAPE = {"padded": (70, 128), "head_nk": (2, 32, 16)}      # (70 rows pad to 96); every other kind: (64, 128)


class _Lib:
    def __init__(self):
        self.calls = []
        self._scalars = {n: [i for i, t in enumerate(sig) if t is not ctypes.c_void_p and not issubclass(t, ctypes._Pointer)]
                         for n, sig in H.SIGNATURES.items()}

    def __getattr__(self, name):
        keep = self._scalars[name]

        def call(*args):
            self.calls.append((name, tuple(args[i] for i in keep)))
            return 0
        return call


@pytest.fixture
def lib(monkeypatch):
    rec = _Lib()
    monkeypatch.setattr(H, "_lib", rec)
    monkeypatch.setattr(H, "stream", lambda: 0)
    ops.shadows.clear()
    yield rec
    ops.shadows.clear()


def _param(kind, seed=0):
    return torch.nn.Parameter(torch.randn(SHAPE.get(kind, (64, 128)), generator=torch.Generator().manual_seed(seed)))


def _twin(a):
    """a second Parameter over `a`'s storage, of the same version: what the next model's parameter is to a freed model's"""
    b = torch.nn.Parameter(a.data)
    assert a.data_ptr() == b.data_ptr() and a._version == b._version and a is not b
    return b


def _ask(kind, p):
    if kind == "head_nk":
        return ops.shadows.head_nk([p])
    if kind == "derived":
        return ops.shadows.derived(p, "t", lambda src: src.t().contiguous())
    return getattr(ops.shadows, kind)(p)


def _ptr(payload):
    return (payload[0] if isinstance(payload, tuple) else payload).data_ptr()


BUILDS = {"get": ["fcmf_cast"], "padded": ["fcmf_cast"], "get_t": ["fcmf_cast_transpose"], "get_fp8": ["fcmf_cast", "fcmf_quant_fp8_rows"],
          "get_fp8_t": ["fcmf_cast_transpose", "fcmf_quant_fp8_rows"], "head_nk": ["fcmf_multi_cast_transpose"], "derived": []}


@pytest.mark.parametrize("kind", KINDS)
def test_a_second_parameter_at_the_same_address_gets_its_own_copy(lib, kind):
    a = _param(kind)
    b = _twin(a)
    pa = _ask(kind, a)
    assert [c[0] for c in lib.calls] == BUILDS[kind]
    n = len(lib.calls)
    assert _ptr(_ask(kind, a)) == _ptr(pa) and len(lib.calls) == n           # a hit: no call
    pb = _ask(kind, b)
    assert [c[0] for c in lib.calls[n:]] == BUILDS[kind]                     # exactly one more build ...
    assert _ptr(pb) != _ptr(pa)                                              # ... into a buffer of its own
    n = len(lib.calls)
    assert _ptr(_ask(kind, b)) == _ptr(pb) and _ptr(_ask(kind, b)) == _ptr(pb) and len(lib.calls) == n
    pa2 = _ask(kind, a)                                                      # (b's entry took the slot: a builds again, once)
    assert len(lib.calls) == n + len(BUILDS[kind]) and _ptr(pa2) != _ptr(pb)
    n = len(lib.calls)
    assert _ptr(_ask(kind, a)) == _ptr(pa2) and len(lib.calls) == n
    if kind == "padded":
        assert tuple(pa.shape) == (96, 128) and tuple(ops.shadows.get(a).shape) == (70, 128) and len(lib.calls) == n


def test_derived_shadow_is_not_served_to_another_parameter_at_the_same_address():
    """a freed model's parameter addresses are recycled for the next model's parameters of the same shape and version: the
    re-layout cached for the first must not come back for the second (two Parameters over one storage stand in for that)"""
    from fcmf_framework import ops
    a = torch.nn.Parameter(torch.arange(6.0).view(2, 3))
    b = torch.nn.Parameter(a.data)
    assert a.data_ptr() == b.data_ptr() and a._version == b._version and a is not b
    built = []
    build = lambda owner: lambda src: built.append(owner) or src.t().contiguous()
    try:
        ta = ops.shadows.derived(a, "t", build("a"))
        assert ops.shadows.derived(a, "t", build("a")) is ta and built == ["a"]
        tb = ops.shadows.derived(b, "t", build("b"))
        assert tb is not ta and built == ["a", "b"]
        assert ops.shadows.derived(b, "t", build("b")) is tb and built == ["a", "b"]
    finally:
        ops.shadows.clear()


@pytest.mark.parametrize("grad", [True, False], ids=["autograd", "no_grad"])
def test_fresh_view_objects_of_one_parameter_hit_one_entry(lib, grad):
    """the baselines' packed in_proj_weight: every forward slices W[:E] anew.  The views are temporaries, W is the owner"""
    W = torch.nn.Parameter(torch.randn(192, 64))
    with torch.set_grad_enabled(grad):
        assert W[:64]._base is W and W[:64] is not W[:64]
        for getter, name in ((ops.shadows.get, "fcmf_cast"), (ops.shadows.get_t, "fcmf_cast_transpose")):
            del lib.calls[:]
            first = getter(W[64:128])
            gc.collect()
            assert getter(W[64:128]).data_ptr() == first.data_ptr() and getter(W[64:128]).data_ptr() == first.data_ptr()
            assert [c[0] for c in lib.calls] == [name]
        assert len(ops.shadows) == 2
        e = ops.shadows.lookup("t", W[64:128])
        assert e.owner() is W and e.offset == 64 * 64 * 4 and e.dense


def test_the_fused_qkv_block_belongs_to_its_first_parameter(lib):
    """fused._fused_weight builds an as_strided temporary over the adjacent q|k|v weights: cast once, not once per call -- with
    three Parameters in one buffer (the text encoder) and with three views of one packed Parameter (the baselines)"""
    buf = torch.randn(192, 64)
    ws = [torch.nn.Parameter(torch.empty(0)) for _ in range(3)]
    for i, w in enumerate(ws):
        w.data = buf[64 * i:64 * (i + 1)]
    first = fused._fused_weight(ws, torch.bfloat16)
    assert tuple(first.shape) == (192, 64) and fused._fused_weight(ws, torch.bfloat16).data_ptr() == first.data_ptr()
    assert lib.calls == [("fcmf_cast", (192 * 64, H.F32, H.BF16))]
    assert ops.shadows.lookup("bf16", fused._fused_weight(ws, torch.float32), owner=ws[0]).owner() is ws[0]
    W = torch.nn.Parameter(torch.randn(192, 64))
    for _ in range(2):
        packed = fused._fused_weight([W[:64], W[64:128], W[128:]], torch.bfloat16)
    assert len(lib.calls) == 2 and ops.shadows.peek(W).data_ptr() == packed.data_ptr()      # (the packed block IS W's bf16 copy)


def _everything(p, heads):
    return [_ptr(_ask(k, p)) for k in ("get", "get_t", "get_fp8", "get_fp8_t", "derived")] + [_ptr(ops.shadows.head_nk([heads]))]


def test_a_dead_owner_leaves_no_entry_and_no_block_in_the_refresh(lib):
    keep, keep_h, gone, gone_h = _param("get", 1), _param("head_nk", 2), _param("get", 3), _param("head_nk", 4)
    _everything(keep, keep_h)
    n_keep = len(ops.shadows)
    assert n_keep == 5 + 1 + 2                                   # five kinds, the head group and its two pieces
    _everything(gone, gone_h)
    assert len(ops.shadows) == 2 * n_keep
    ops.shadows.refresh_transposed()
    blocks = lib.calls[-1][1][0]
    assert lib.calls[-1][0] == "fcmf_multi_cast_transpose" and blocks == 2 * (2 + 2 * 1)      # [64, 128]: 1 x 2 tiles of 64; [32, 16] x 2: 1 each
    del gone, gone_h
    gc.collect()
    ops.shadows.mark_all_stale()
    assert len(ops.shadows) == n_keep
    for kind in ("bf16", "t", "fp8", "fp8_t"):
        assert ops.shadows.lookup(kind, keep) is not None
    assert ops.shadows.lookup("derived", keep, "t") is not None and ops.shadows.lookup("heads", keep_h, (keep_h.data_ptr(),)) is not None
    ops.shadows.refresh_transposed()
    assert lib.calls[-1] == ("fcmf_multi_cast_transpose", (blocks // 2,))


@pytest.mark.parametrize("kind", KINDS)
def test_a_moved_parameter_is_not_served_its_old_copy(lib, kind):
    p = _param(kind)
    old = _ptr(_ask(kind, p))
    n, entries = len(lib.calls), len(ops.shadows)
    p.data = p.data.clone()
    assert _ptr(_ask(kind, p)) != old and len(lib.calls) == n + len(BUILDS[kind])
    ops.shadows.mark_all_stale()                                 # ... and the copies of the old storage go with the next prune
    assert len(ops.shadows) == entries


def test_everything_rebuilds_once_after_mark_all_stale(lib):
    a, heads = _param("get", 1), _param("head_nk", 2)
    built = []
    derived = lambda: ops.shadows.derived(a, "recorded", lambda src: built.append(1) or src.t().contiguous())
    ptrs = _everything(a, heads), derived()
    del lib.calls[:]
    assert _everything(a, heads) == ptrs[0] and derived() is ptrs[1] and not lib.calls and built == [1]
    ops.shadows.mark_all_stale()
    assert ops.shadows.peek(a).data_ptr() == ptrs[0][0]         # (stale, but a's own: FusedAdamW writes it in its update kernel)
    again = _everything(a, heads)
    assert again[:4] + again[5:] == ptrs[0][:4] + ptrs[0][5:]    # rebuilt in place: the addresses the optimizer's tables hold stay
    ptrs = again, ptrs[1]                                        # (a derived tensor is whatever its builder returns: a new one)
    derived()
    assert sorted(c[0] for c in lib.calls) == ["fcmf_cast", "fcmf_cast_transpose", "fcmf_multi_cast_transpose", "fcmf_quant_fp8_rows",
                                               "fcmf_quant_fp8_rows"] and built == [1, 1]
    del lib.calls[:]
    assert _everything(a, heads) == ptrs[0] and not lib.calls
    ops.shadows.mark_all_stale()
    ops.shadows.mark_fresh(a)
    assert ops.shadows.get(a).data_ptr() == ptrs[0][0] and ops.as_compute(a, torch.bfloat16).data_ptr() == ptrs[0][0] and not lib.calls
    b = _twin(a)
    assert ops.shadows.peek(b) is None and ops.shadows.peek(a) is not None
    ops.shadows.mark_all_stale()
    ops.shadows.mark_fresh(b)                                    # (not b's entry: nothing is marked)
    ops.shadows.get(a)
    assert [c[0] for c in lib.calls] == ["fcmf_cast"]
