"""The library calls of the projection, vocabulary-projection and LayerNorm autograd nodes of fcmf_framework/ops.py, in order
(helpers._recorded(nulls=True): every call's scalar arguments, its return code and which of its pointer arguments were NULL --
"bias given or not", "dx wanted or not", "dxsum or not" show only there).

EXPECTED was printed by this file (the MEASURED lines) at commit 1fa020f, the commit BEFORE ops.linear / linear_multi / seq_fan came
to share one autograd node, the three vocabulary projections two helpers and the five LayerNorm call sites ops.ln_fwd / ops.ln_bwd,
with nothing but the recorder's `nulls` option added there: the shared code has to issue what the separate copies issued.

Every scene is one forward and one backward on seeded inputs, in float32 and in bf16; "arena": under dp.GradArena.for_model over a
small module that owns the scene's parameters (the record then ends with the deferred weight-gradient flush)."""
import pytest
import torch

from helpers import _calls_digest, _recorded

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DT = {"f32": F32, "bf16": BF16}


def _rand(shape, dev, dtype=F32, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype).to(dev)


def _set(dtype):
    from fcmf_framework import ops
    ops.set_compute_dtype(dtype)
    ops.shadows.clear()


class _Params(torch.nn.Module):
    """owns a scene's parameters (what dp.GradArena.for_model walks); None entries are kept as plain attributes"""

    def __init__(self, frozen=(), **tensors):
        super().__init__()
        for n, t in tensors.items():
            setattr(self, n, None if t is None else torch.nn.Parameter(t, requires_grad=n not in frozen))


def _weighted(ys, seed=40):
    """a loss that gives every tensor of `ys` its own seeded output gradient"""
    return sum((y.float() * _rand(y.shape, y.device, seed=seed + i)).sum() for i, y in enumerate(ys))


# ------------------------------------------------------------------------------------------------------------------------
# scenes: (dev, dtype, case) -> (module, step); step() runs forward + backward and returns the tensors to compare
# ------------------------------------------------------------------------------------------------------------------------
def _linear(dev, dtype, case):
    from fcmf_framework import ops
    m = _Params(w=_rand((128, 64), dev, scale=0.2, seed=2), b=None if case == "nobias" else _rand((128,), dev, seed=3),
                frozen=("w",) if case == "wfrozen" else ())
    x = _rand((5, 9, 64), dev, dtype, seed=1).requires_grad_(case != "xnograd")

    def step():
        y = ops.linear(x, m.w, m.b, act="tanh" if case == "tanh" else None)
        _weighted([y]).backward()
        return dict(y=y, dx=x.grad)
    return m, step


def _fan_params(dev):
    return _Params(**{f"w{i}": _rand((64, 64), dev, scale=0.2, seed=2 + i) for i in range(3)},
                   **{f"b{i}": _rand((64,), dev, seed=7 + i) for i in range(3)})


def _linear_multi(dev, dtype, case):
    from fcmf_framework import ops
    m = _fan_params(dev)
    x = _rand((6, 10, 64), dev, dtype, seed=1).requires_grad_(True)

    def step():
        ys = ops.linear_multi(x, m.w0, m.b0, m.w1, m.b1, m.w2, m.b2)
        _weighted([y for i, y in enumerate(ys) if case == "all" or i != 1]).backward()
        return dict(q=ys[0], k=ys[1], v=ys[2], dx=x.grad)
    return m, step


def _seq_fan(dev, dtype, case):
    """ops.linear_multi over all three weights, then ops.seq_fan over weights 1 and 2 again (a second producer for their gradient
    slices), the second without its bias.  case: which of seq_fan's outputs (key, value, row 0) reach the loss"""
    from fcmf_framework import ops
    m = _fan_params(dev)
    x = _rand((6, 10, 64), dev, dtype, seed=1).requires_grad_(True)
    used = dict(all=(0, 1, 2), nov=(0, 2), row0only=(2,), norow0=(0, 1))[case]

    def step():
        ys = ops.linear_multi(x, m.w0, m.b0, m.w1, m.b1, m.w2, m.b2)
        fan = ops.seq_fan(x, m.w1, m.b1, m.w2, None)
        (_weighted(ys) + _weighted([fan[i] for i in used], seed=50)).backward()
        return dict(q=ys[0], k=ys[1], v=ys[2], k2=fan[0], v2=fan[1], cls=fan[2], dx=x.grad)
    return m, step


def _seq_fan_cold(dev, dtype, case):
    """ops.seq_fan alone: in bf16 both weight shadows are still to be cast when its forward starts"""
    from fcmf_framework import ops
    m = _fan_params(dev)
    x = _rand((6, 10, 64), dev, dtype, seed=1).requires_grad_(True)

    def step():
        fan = ops.seq_fan(x, m.w1, m.b1, m.w2, None)
        _weighted(fan, seed=50).backward()
        return dict(k2=fan[0], v2=fan[1], cls=fan[2], dx=x.grad)
    return m, step


def _vocab_linear(dev, dtype, case):
    from fcmf_framework import ops
    m = _Params(w=_rand((1003, 64), dev, scale=0.3, seed=1), b=_rand((1003,), dev, seed=2))
    x = _rand((5, 14, 64), dev, dtype, seed=3).requires_grad_(True)

    def step():
        y = ops.vocab_linear(x, m.w, m.b)
        _weighted([y]).backward()
        return dict(y=y, dx=x.grad)
    return m, step


def _vocab_xent(dev, dtype, case):
    """the tied matrix: looked up by ops.embed_layer_norm and multiplied by ops.vocab_cross_entropy -- two producers of its gradient.
    case: "v1999", "v1999-nobias", "v8193" (Vp = 8224 >= 8192: the split-K float32 branch of ops.gemm_dx_long_k in bf16)"""
    from fcmf_framework import ops
    V, K, pad = (8193 if case == "v8193" else 1999), 64, 1
    m = _Params(word=_rand((V, K), dev, scale=0.3, seed=1), bias=None if case.endswith("nobias") else _rand((V,), dev, scale=0.1, seed=2),
                ptab=_rand((40, K), dev, seed=3), ttab=_rand((2, K), dev, seed=4), g=1 + 0.1 * _rand((K,), dev, seed=5),
                b=_rand((K,), dev, seed=6))
    gen = torch.Generator().manual_seed(7)
    ids = torch.randint(3, V, (3, 5), generator=gen).to(dev)
    lb = torch.randint(0, V, (3, 5), generator=gen)
    lb[:, -1] = -100
    lb = lb.to(dev)
    pos = ops.position_ids(ids, pad)

    def step():
        h = ops.embed_layer_norm(ids, pos, None, m.word, m.ptab, m.ttab, m.g, m.b, 1e-5, 0.0, False, pad, dtype)
        loss = ops.vocab_cross_entropy(h, m.word, m.bias, lb)
        loss.backward()
        return dict(loss=loss)
    return m, step


def _vocab_topk(dev, dtype, case):
    """the decode step's projection, three times: cold (the weight shadow is built), and twice more.  The later calls are checked
    against each other in the test below: the padded bias cached on the Parameter adds no library call"""
    from fcmf_framework import ops
    m = _Params(w=_rand((1003, 64), dev, scale=0.3, seed=1), b=_rand((1003,), dev, seed=2))
    x = _rand((6, 64), dev, dtype, seed=3)

    def step():
        out = {}
        for i in range(3):
            out[f"logp{i}"], out[f"ids{i}"] = ops.vocab_topk(x, m.w, m.b, 4)
        return out
    return m, step


def _add_ln(dev, dtype, case):
    """case: "<H>-<nores | strided | drop>": no residual / a residual with a row stride / the same with p = 0.1 in training"""
    from fcmf_framework import ops
    Hd, kind = case.split("-")
    Hd, rows = int(Hd), 37
    m = _Params(g=1 + 0.1 * _rand((Hd,), dev, seed=3), b=_rand((Hd,), dev, seed=4))
    x = _rand((rows, Hd), dev, dtype, seed=1).requires_grad_(True)
    big = _rand((rows, 3, Hd), dev, dtype, seed=2).requires_grad_(True)

    def step():
        y = ops.add_layer_norm(x, None if kind == "nores" else big[:, 0], m.g, m.b, 1e-12, p=0.1, training=kind == "drop")
        _weighted([y]).backward()
        return dict(y=y, dx=x.grad, dres=big.grad)
    return m, step


def _embed_ln(dev, dtype, case):
    """case: "<H>-<tt | nott>[-drop]": H 64 takes the fused position + type gradient kernel, H 36 its fallback"""
    from fcmf_framework import ops
    parts = case.split("-")
    Hd, V, pad = int(parts[0]), 50, 1
    ids = torch.randint(3, V, (4, 12), generator=torch.Generator().manual_seed(1))
    ids[0, 7:] = pad
    ids[2, 3:] = pad
    ids[3, 0] = pad
    ids[1, 5] = pad
    tt = None
    if parts[1] == "tt":
        tt = torch.zeros_like(ids)
        tt[1] = 1
        tt = tt.to(dev)
    ids = ids.to(dev)
    m = _Params(word=_rand((V, Hd), dev, seed=10), ptab=_rand((40, Hd), dev, seed=11), ttab=_rand((2, Hd), dev, seed=12),
                g=1 + 0.1 * _rand((Hd,), dev, seed=7), b=_rand((Hd,), dev, seed=8))
    pos = ops.position_ids(ids, pad)

    def step():
        y = ops.embed_layer_norm(ids, pos, tt, m.word, m.ptab, m.ttab, m.g, m.b, 1e-5, 0.1, parts[-1] == "drop", pad, dtype)
        _weighted([y]).backward()
        return dict(y=y)
    return m, step


# scene -> (builder, its cases, dtypes, also under the arena)
SCENES = {
    "linear": (_linear, ["bias", "nobias", "tanh", "xnograd", "wfrozen"], ["f32", "bf16"], True),
    "linear_multi": (_linear_multi, ["mid-unused", "all"], ["f32", "bf16"], True),
    "seq_fan": (_seq_fan, ["all", "nov", "row0only", "norow0"], ["f32", "bf16"], True),
    "seq_fan_cold": (_seq_fan_cold, ["all"], ["f32", "bf16"], True),
    "vocab_linear": (_vocab_linear, ["ragged"], ["f32", "bf16"], False),
    "vocab_xent": (_vocab_xent, ["v1999", "v1999-nobias", "v8193"], ["f32", "bf16"], True),
    "vocab_topk": (_vocab_topk, ["k4"], ["f32", "bf16"], False),
    "add_ln": (_add_ln, [f"{h}-{k}" for h in (64, 768) for k in ("nores", "strided", "drop")], ["f32", "bf16"], True),
    "embed_ln": (_embed_ln, [f"{h}-{t}" for h in (64, 36) for t in ("tt", "nott")] + ["64-tt-drop", "64-nott-drop"], ["f32", "bf16"], True),
}
ONE_DTYPE = {("vocab_xent", "v1999-nobias"): "bf16", ("vocab_xent", "v8193"): "bf16"}
CASES = [f"{s}/{c}/{d}{'/arena' if a else ''}" for s, (_, cases, dts, arena) in SCENES.items() for c in cases for d in dts
         if ONE_DTYPE.get((s, c), d) == d for a in ((False, True) if arena else (False,))]


def run_case(dev, case):
    """-> (the recorded calls, name -> tensor: what the scene's step returned and every parameter's gradient)"""
    from fcmf_framework import dp, ops
    scene, name, dt, *rest = case.split("/")
    _set(DT[dt])
    ops.manual_seed(0)
    arena = None
    try:
        m, step = SCENES[scene][0](dev, DT[dt], name)
        if rest:
            arena = dp.GradArena.for_model(m)
            arena.zero()
        out = {}
        calls = _recorded(lambda: out.update(step()), nulls=True)
        out.update({"d" + n: p.grad for n, p in m.named_parameters()})
        return calls, {k: v.detach().clone() for k, v in out.items() if v is not None}
    finally:
        if arena is not None:
            arena.deactivate()
        _set(F32)


# case -> (entry-point names in call order, SHA-256 of repr([(name, scalar arguments, return code, NULL flags), ...]))
EXPECTED = {
    "linear/bias/f32": ("fcmf_gemm fcmf_gemm fcmf_gemm fcmf_colsum",
        "7cf5d67e0719d4dcbaa99876a90a0ea53bfdaf966b1350499a6ea13934cb7eee"),
    "linear/bias/f32/arena": ("fcmf_gemm fcmf_gemm fcmf_gemm fcmf_colsum",
        "7cf5d67e0719d4dcbaa99876a90a0ea53bfdaf966b1350499a6ea13934cb7eee"),
    "linear/bias/bf16": ("fcmf_cast fcmf_gemm fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_colsum",
        "96917bc28d78f45871052ec17a415b01d7db0e11a2fdfa53e575ffac76b235a5"),
    "linear/bias/bf16/arena": ("fcmf_cast fcmf_gemm fcmf_cast_transpose fcmf_gemm fcmf_colsum fcmf_gemm_dw_batched",
        "c6a57779cd54c15c2cd57b3633c75abc59b0af310472e1d7f3adc057b2ce3bc8"),
    "linear/nobias/f32": ("fcmf_gemm fcmf_gemm fcmf_gemm",
        "c093f12375fb601e304e0fbe7d6c085ffa05463cf1d7d63b2fd4d0dbf4ace1fd"),
    "linear/nobias/f32/arena": ("fcmf_gemm fcmf_gemm fcmf_gemm",
        "c093f12375fb601e304e0fbe7d6c085ffa05463cf1d7d63b2fd4d0dbf4ace1fd"),
    "linear/nobias/bf16": ("fcmf_cast fcmf_gemm fcmf_cast_transpose fcmf_gemm fcmf_gemm",
        "2276df7b63d91881041dc9eea33622dee479930856e843ac0700ee8bdf7ecc5a"),
    "linear/nobias/bf16/arena": ("fcmf_cast fcmf_gemm fcmf_cast_transpose fcmf_gemm fcmf_gemm_dw_batched",
        "3f10e8e0c00e611fa919bb68e31f71fbff93926f65339f70138c2c3c01603e74"),
    "linear/tanh/f32": ("fcmf_gemm fcmf_act_bwd fcmf_gemm fcmf_gemm fcmf_colsum",
        "690879a57963b34b532b4a1481683e3f3acaf6c9aa3d69681c9404b4ee980c69"),
    "linear/tanh/f32/arena": ("fcmf_gemm fcmf_act_bwd fcmf_gemm fcmf_gemm fcmf_colsum",
        "690879a57963b34b532b4a1481683e3f3acaf6c9aa3d69681c9404b4ee980c69"),
    "linear/tanh/bf16": ("fcmf_cast fcmf_gemm fcmf_act_bwd fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_colsum",
        "7bf3cd5adcb0bf8d11cef72f3d0b8078b70ecc1dd584d8cf512156e168811690"),
    "linear/tanh/bf16/arena": ("fcmf_cast fcmf_gemm fcmf_act_bwd fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_colsum",
        "7bf3cd5adcb0bf8d11cef72f3d0b8078b70ecc1dd584d8cf512156e168811690"),
    "linear/xnograd/f32": ("fcmf_gemm fcmf_gemm fcmf_colsum",
        "97b654e8190fcef0f295b1f0f45ebe05aea3fcc9f0dae5af33262651ca1eba76"),
    "linear/xnograd/f32/arena": ("fcmf_gemm fcmf_gemm fcmf_colsum",
        "97b654e8190fcef0f295b1f0f45ebe05aea3fcc9f0dae5af33262651ca1eba76"),
    "linear/xnograd/bf16": ("fcmf_cast fcmf_gemm fcmf_gemm fcmf_colsum",
        "657e4dfbc1f79d88d9fa0a85a03c5519adb287dd7c1c763a27e12c8c56592378"),
    "linear/xnograd/bf16/arena": ("fcmf_cast fcmf_gemm fcmf_colsum fcmf_gemm_dw_batched",
        "4c40e969e2cdd508b8770fec48e17d11d3e371d56782e1a92aa1829618cefd33"),
    "linear/wfrozen/f32": ("fcmf_gemm fcmf_gemm fcmf_colsum",
        "4f107e83f134cebd7929c1ec2a37c6bbde62cee9df7328b4a81b093c9424ed51"),
    "linear/wfrozen/f32/arena": ("fcmf_gemm fcmf_gemm fcmf_colsum",
        "4f107e83f134cebd7929c1ec2a37c6bbde62cee9df7328b4a81b093c9424ed51"),
    "linear/wfrozen/bf16": ("fcmf_cast fcmf_gemm fcmf_cast_transpose fcmf_gemm fcmf_colsum",
        "4d6e93ad6f482fd7dba4ef1be15fffc742c66c2276581602b6a6b70089a2efa3"),
    "linear/wfrozen/bf16/arena": ("fcmf_cast fcmf_gemm fcmf_cast_transpose fcmf_gemm fcmf_colsum",
        "4d6e93ad6f482fd7dba4ef1be15fffc742c66c2276581602b6a6b70089a2efa3"),
    "linear_multi/mid-unused/f32": ("""
        fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm
        fcmf_colsum
        """, "fadcb69eb7ac609a115115c3ba3f08a2fa541379b1d8d9adfa1c22cf82148188"),
    "linear_multi/mid-unused/f32/arena": ("""
        fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm
        fcmf_colsum
        """, "fadcb69eb7ac609a115115c3ba3f08a2fa541379b1d8d9adfa1c22cf82148188"),
    "linear_multi/mid-unused/bf16": ("""
        fcmf_cast fcmf_gemm fcmf_cast fcmf_gemm fcmf_cast fcmf_gemm fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_colsum
        fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_colsum fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_colsum
        """, "20ccad69fbd0b426b9083b8c54b02527df1798e58fc771d1820ce5b5231be522"),
    "linear_multi/mid-unused/bf16/arena": ("""
        fcmf_cast fcmf_gemm fcmf_cast fcmf_gemm fcmf_cast fcmf_gemm fcmf_cast_transpose fcmf_gemm fcmf_colsum
        fcmf_cast_transpose fcmf_gemm fcmf_colsum fcmf_cast_transpose fcmf_gemm fcmf_colsum fcmf_gemm_dw_batched
        """, "43429c01c12a843dbf90d11c7da948f24c4aa7116a04b97baff937f01c79be76"),
    "linear_multi/all/f32": ("""
        fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm
        fcmf_colsum
        """, "fadcb69eb7ac609a115115c3ba3f08a2fa541379b1d8d9adfa1c22cf82148188"),
    "linear_multi/all/f32/arena": ("""
        fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm
        fcmf_colsum
        """, "fadcb69eb7ac609a115115c3ba3f08a2fa541379b1d8d9adfa1c22cf82148188"),
    "linear_multi/all/bf16": ("""
        fcmf_cast fcmf_gemm fcmf_cast fcmf_gemm fcmf_cast fcmf_gemm fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_colsum
        fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_colsum fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_colsum
        """, "20ccad69fbd0b426b9083b8c54b02527df1798e58fc771d1820ce5b5231be522"),
    "linear_multi/all/bf16/arena": ("""
        fcmf_cast fcmf_gemm fcmf_cast fcmf_gemm fcmf_cast fcmf_gemm fcmf_cast_transpose fcmf_gemm fcmf_colsum
        fcmf_cast_transpose fcmf_gemm fcmf_colsum fcmf_cast_transpose fcmf_gemm fcmf_colsum fcmf_gemm_dw_batched
        """, "43429c01c12a843dbf90d11c7da948f24c4aa7116a04b97baff937f01c79be76"),
    "seq_fan/all/f32": ("""
        fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm fcmf_gemm
        fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm fcmf_colsum
        """, "098f6eaf0af2bb0109df9c8eaefb9cc38f3c3f58c6762ac8a6764357f1216aa2"),
    "seq_fan/all/f32/arena": ("""
        fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm fcmf_gemm
        fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm fcmf_colsum
        """, "098f6eaf0af2bb0109df9c8eaefb9cc38f3c3f58c6762ac8a6764357f1216aa2"),
    "seq_fan/all/bf16": ("""
        fcmf_cast fcmf_gemm fcmf_cast fcmf_gemm fcmf_cast fcmf_gemm fcmf_gemm fcmf_gemm fcmf_cast_transpose fcmf_gemm
        fcmf_gemm fcmf_colsum fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_colsum
        fcmf_gemm fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm fcmf_colsum
        """, "1a4d8878a4e896f46974f3f48d69d72bd9f7e71d9672bdd971b51d5a59d58939"),
    "seq_fan/all/bf16/arena": ("""
        fcmf_cast fcmf_gemm fcmf_cast fcmf_gemm fcmf_cast fcmf_gemm fcmf_gemm fcmf_gemm fcmf_cast_transpose fcmf_gemm
        fcmf_colsum fcmf_cast_transpose fcmf_gemm fcmf_cast_transpose fcmf_gemm fcmf_colsum fcmf_gemm fcmf_colsum fcmf_gemm
        fcmf_colsum fcmf_gemm_dw_batched
        """, "9d1b31fb94fbc512379b2f2bb4b69e46364bb10f7f65ef4cbe623661ca8bcf3f"),
    "seq_fan/nov/f32": ("""
        fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm fcmf_gemm
        fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm fcmf_colsum
        """, "098f6eaf0af2bb0109df9c8eaefb9cc38f3c3f58c6762ac8a6764357f1216aa2"),
    "seq_fan/nov/f32/arena": ("""
        fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm fcmf_gemm
        fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm fcmf_colsum
        """, "098f6eaf0af2bb0109df9c8eaefb9cc38f3c3f58c6762ac8a6764357f1216aa2"),
    "seq_fan/nov/bf16": ("""
        fcmf_cast fcmf_gemm fcmf_cast fcmf_gemm fcmf_cast fcmf_gemm fcmf_gemm fcmf_gemm fcmf_cast_transpose fcmf_gemm
        fcmf_gemm fcmf_colsum fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_colsum
        fcmf_gemm fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm fcmf_colsum
        """, "1a4d8878a4e896f46974f3f48d69d72bd9f7e71d9672bdd971b51d5a59d58939"),
    "seq_fan/nov/bf16/arena": ("""
        fcmf_cast fcmf_gemm fcmf_cast fcmf_gemm fcmf_cast fcmf_gemm fcmf_gemm fcmf_gemm fcmf_cast_transpose fcmf_gemm
        fcmf_colsum fcmf_cast_transpose fcmf_gemm fcmf_cast_transpose fcmf_gemm fcmf_colsum fcmf_gemm fcmf_colsum fcmf_gemm
        fcmf_colsum fcmf_gemm_dw_batched
        """, "9d1b31fb94fbc512379b2f2bb4b69e46364bb10f7f65ef4cbe623661ca8bcf3f"),
    "seq_fan/row0only/f32": ("""
        fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm fcmf_gemm
        fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm fcmf_colsum
        """, "098f6eaf0af2bb0109df9c8eaefb9cc38f3c3f58c6762ac8a6764357f1216aa2"),
    "seq_fan/row0only/f32/arena": ("""
        fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm fcmf_gemm
        fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm fcmf_colsum
        """, "098f6eaf0af2bb0109df9c8eaefb9cc38f3c3f58c6762ac8a6764357f1216aa2"),
    "seq_fan/row0only/bf16": ("""
        fcmf_cast fcmf_gemm fcmf_cast fcmf_gemm fcmf_cast fcmf_gemm fcmf_gemm fcmf_gemm fcmf_cast_transpose fcmf_gemm
        fcmf_gemm fcmf_colsum fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_colsum
        fcmf_gemm fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm fcmf_colsum
        """, "1a4d8878a4e896f46974f3f48d69d72bd9f7e71d9672bdd971b51d5a59d58939"),
    "seq_fan/row0only/bf16/arena": ("""
        fcmf_cast fcmf_gemm fcmf_cast fcmf_gemm fcmf_cast fcmf_gemm fcmf_gemm fcmf_gemm fcmf_cast_transpose fcmf_gemm
        fcmf_colsum fcmf_cast_transpose fcmf_gemm fcmf_cast_transpose fcmf_gemm fcmf_colsum fcmf_gemm fcmf_colsum fcmf_gemm
        fcmf_colsum fcmf_gemm_dw_batched
        """, "9d1b31fb94fbc512379b2f2bb4b69e46364bb10f7f65ef4cbe623661ca8bcf3f"),
    "seq_fan/norow0/f32": ("""
        fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm fcmf_gemm
        fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm fcmf_colsum
        """, "098f6eaf0af2bb0109df9c8eaefb9cc38f3c3f58c6762ac8a6764357f1216aa2"),
    "seq_fan/norow0/f32/arena": ("""
        fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm fcmf_gemm
        fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm fcmf_colsum
        """, "098f6eaf0af2bb0109df9c8eaefb9cc38f3c3f58c6762ac8a6764357f1216aa2"),
    "seq_fan/norow0/bf16": ("""
        fcmf_cast fcmf_gemm fcmf_cast fcmf_gemm fcmf_cast fcmf_gemm fcmf_gemm fcmf_gemm fcmf_cast_transpose fcmf_gemm
        fcmf_gemm fcmf_colsum fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_colsum
        fcmf_gemm fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm fcmf_colsum
        """, "1a4d8878a4e896f46974f3f48d69d72bd9f7e71d9672bdd971b51d5a59d58939"),
    "seq_fan/norow0/bf16/arena": ("""
        fcmf_cast fcmf_gemm fcmf_cast fcmf_gemm fcmf_cast fcmf_gemm fcmf_gemm fcmf_gemm fcmf_cast_transpose fcmf_gemm
        fcmf_colsum fcmf_cast_transpose fcmf_gemm fcmf_cast_transpose fcmf_gemm fcmf_colsum fcmf_gemm fcmf_colsum fcmf_gemm
        fcmf_colsum fcmf_gemm_dw_batched
        """, "9d1b31fb94fbc512379b2f2bb4b69e46364bb10f7f65ef4cbe623661ca8bcf3f"),
    "seq_fan_cold/all/f32": ("fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm",
        "48c580941a5ecb8934eccdb59800ca71430498e9918ff4636d623f2dd10ae270"),
    "seq_fan_cold/all/f32/arena": ("fcmf_gemm fcmf_gemm fcmf_gemm fcmf_gemm fcmf_colsum fcmf_gemm fcmf_gemm",
        "48c580941a5ecb8934eccdb59800ca71430498e9918ff4636d623f2dd10ae270"),
    "seq_fan_cold/all/bf16": ("""
        fcmf_cast fcmf_cast fcmf_gemm fcmf_gemm fcmf_cast_transpose fcmf_gemm fcmf_gemm fcmf_colsum fcmf_cast_transpose
        fcmf_gemm fcmf_gemm
        """, "d186648cfd5dcb0349435247531e1917f3f6521116c934ff93152a615206eb12"),
    "seq_fan_cold/all/bf16/arena": ("""
        fcmf_cast fcmf_cast fcmf_gemm fcmf_gemm fcmf_cast_transpose fcmf_gemm fcmf_colsum fcmf_cast_transpose fcmf_gemm
        fcmf_gemm_dw_batched
        """, "0832a29ab9f166080a0f84a007683ef38af9428d10fa8569185d06e91ce6c221"),
    "vocab_linear/ragged/f32": ("fcmf_gemm fcmf_gemm fcmf_gemm fcmf_colsum",
        "f949c7903528f33fce9b83d4f7944996c1dc9e58f94fe1003ac6eaae45545fd8"),
    "vocab_linear/ragged/bf16": ("fcmf_cast fcmf_gemm fcmf_gemm fcmf_gemm fcmf_colsum",
        "d17f349ce17805498cc39b6cfd00d90325cee35c4aa11e09f42b91512d5b4187"),
    "vocab_xent/v1999/f32": ("""
        fcmf_embed_ln_fwd fcmf_gemm fcmf_xent_fwd fcmf_xent_bwd fcmf_gemm fcmf_gemm fcmf_colsum fcmf_add_ln_bwd_workspace
        fcmf_add_ln_bwd fcmf_embed_pos_type_bwd fcmf_embed_bwd
        """, "d0bacb4d52fad2fdcc851e45be4e8a8a871554f2f5ecde85ef656acac62395de"),
    "vocab_xent/v1999/f32/arena": ("""
        fcmf_embed_ln_fwd fcmf_gemm fcmf_xent_fwd fcmf_xent_bwd fcmf_gemm fcmf_gemm fcmf_colsum fcmf_add_ln_bwd_workspace
        fcmf_add_ln_bwd fcmf_embed_pos_type_bwd fcmf_embed_bwd
        """, "d0bacb4d52fad2fdcc851e45be4e8a8a871554f2f5ecde85ef656acac62395de"),
    "vocab_xent/v1999/bf16": ("""
        fcmf_embed_ln_fwd fcmf_cast fcmf_gemm fcmf_xent_fwd fcmf_xent_bwd fcmf_gemm fcmf_gemm fcmf_colsum
        fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_embed_pos_type_bwd fcmf_embed_bwd
        """, "3ba5a4be54057b2a3d33da13077d5d9c7e0413b7b7e3199c45785527a26a597e"),
    "vocab_xent/v1999/bf16/arena": ("""
        fcmf_embed_ln_fwd fcmf_cast fcmf_gemm fcmf_xent_fwd fcmf_xent_bwd fcmf_gemm fcmf_gemm fcmf_colsum
        fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_embed_pos_type_bwd fcmf_embed_bwd
        """, "3ba5a4be54057b2a3d33da13077d5d9c7e0413b7b7e3199c45785527a26a597e"),
    "vocab_xent/v1999-nobias/bf16": ("""
        fcmf_embed_ln_fwd fcmf_cast fcmf_gemm fcmf_xent_fwd fcmf_xent_bwd fcmf_gemm fcmf_gemm fcmf_add_ln_bwd_workspace
        fcmf_add_ln_bwd fcmf_embed_pos_type_bwd fcmf_embed_bwd
        """, "b109fbc93ac3f5df45fd7ab5f39115fd83498e9fed57a182db09a70544278039"),
    "vocab_xent/v1999-nobias/bf16/arena": ("""
        fcmf_embed_ln_fwd fcmf_cast fcmf_gemm fcmf_xent_fwd fcmf_xent_bwd fcmf_gemm fcmf_gemm fcmf_add_ln_bwd_workspace
        fcmf_add_ln_bwd fcmf_embed_pos_type_bwd fcmf_embed_bwd
        """, "b109fbc93ac3f5df45fd7ab5f39115fd83498e9fed57a182db09a70544278039"),
    "vocab_xent/v8193/bf16": ("""
        fcmf_embed_ln_fwd fcmf_cast fcmf_gemm fcmf_xent_fwd fcmf_xent_bwd fcmf_gemm fcmf_cast fcmf_gemm fcmf_colsum
        fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_embed_pos_type_bwd fcmf_embed_bwd
        """, "8978213d7c4bae290018db9566fd71f6c276117dd6c62622b7944c07ccc5ab2e"),
    "vocab_xent/v8193/bf16/arena": ("""
        fcmf_embed_ln_fwd fcmf_cast fcmf_gemm fcmf_xent_fwd fcmf_xent_bwd fcmf_gemm fcmf_cast fcmf_gemm fcmf_colsum
        fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_embed_pos_type_bwd fcmf_embed_bwd
        """, "8978213d7c4bae290018db9566fd71f6c276117dd6c62622b7944c07ccc5ab2e"),
    "vocab_topk/k4/f32": ("fcmf_gemm fcmf_logsoftmax_topk fcmf_gemm fcmf_logsoftmax_topk fcmf_gemm fcmf_logsoftmax_topk",
        "5c5cb85954e3b3f876147a4a9946f0e4ac950676258a17a1d7da63b8d457c891"),
    "vocab_topk/k4/bf16": ("fcmf_cast fcmf_gemm fcmf_logsoftmax_topk fcmf_gemm fcmf_logsoftmax_topk fcmf_gemm fcmf_logsoftmax_topk",
        "eeb630979f7d128feace821cafe519fd10f9d1a04300738d09e67afe458b783c"),
    "add_ln/64-nores/f32": ("fcmf_add_ln_fwd fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd",
        "9ff44a45cb2ca95676d1c505affb3357cac17c16e5a6c9c2a3d3af232183ba39"),
    "add_ln/64-nores/f32/arena": ("fcmf_add_ln_fwd fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd",
        "9ff44a45cb2ca95676d1c505affb3357cac17c16e5a6c9c2a3d3af232183ba39"),
    "add_ln/64-nores/bf16": ("fcmf_add_ln_fwd fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd",
        "51fe3db74b36353b5236e40cf7017ef69c8d42efee5541fbdbfaf4554c06bb59"),
    "add_ln/64-nores/bf16/arena": ("fcmf_add_ln_fwd fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd",
        "51fe3db74b36353b5236e40cf7017ef69c8d42efee5541fbdbfaf4554c06bb59"),
    "add_ln/64-strided/f32": ("fcmf_add_ln_fwd fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd",
        "31cdd43bc2a8756a33f71c7d3f6a2e388bd9f5868366018281a025ab139ab368"),
    "add_ln/64-strided/f32/arena": ("fcmf_add_ln_fwd fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd",
        "31cdd43bc2a8756a33f71c7d3f6a2e388bd9f5868366018281a025ab139ab368"),
    "add_ln/64-strided/bf16": ("fcmf_add_ln_fwd fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd",
        "2bbd37ca8fec725ac9e323c8855dbbb6b7422bc902d0fa0c33aa09d87c1bb354"),
    "add_ln/64-strided/bf16/arena": ("fcmf_add_ln_fwd fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd",
        "2bbd37ca8fec725ac9e323c8855dbbb6b7422bc902d0fa0c33aa09d87c1bb354"),
    "add_ln/64-drop/f32": ("fcmf_add_ln_fwd fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd",
        "ec355f7d0e3dd7d9a4b1ebea8302723866661b1e11ef6ffb33a8dadb428057bb"),
    "add_ln/64-drop/f32/arena": ("fcmf_add_ln_fwd fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd",
        "ec355f7d0e3dd7d9a4b1ebea8302723866661b1e11ef6ffb33a8dadb428057bb"),
    "add_ln/64-drop/bf16": ("fcmf_add_ln_fwd fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd",
        "089690f4d07ac2193f6f25f70c375ad1241fe2bc1265e433915dbff45c23de1a"),
    "add_ln/64-drop/bf16/arena": ("fcmf_add_ln_fwd fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd",
        "089690f4d07ac2193f6f25f70c375ad1241fe2bc1265e433915dbff45c23de1a"),
    "add_ln/768-nores/f32": ("fcmf_add_ln_fwd fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd",
        "cc8a14c704c3765fb89af922dd36d0332de4964a8b71b26bff8d949a62a7d725"),
    "add_ln/768-nores/f32/arena": ("fcmf_add_ln_fwd fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd",
        "cc8a14c704c3765fb89af922dd36d0332de4964a8b71b26bff8d949a62a7d725"),
    "add_ln/768-nores/bf16": ("fcmf_add_ln_fwd fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd",
        "03337f9a736dbb4c96021087b711b8461367c0beca9f9418c2621f7fb516d10c"),
    "add_ln/768-nores/bf16/arena": ("fcmf_add_ln_fwd fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd",
        "03337f9a736dbb4c96021087b711b8461367c0beca9f9418c2621f7fb516d10c"),
    "add_ln/768-strided/f32": ("fcmf_add_ln_fwd fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd",
        "131df0f251cbf0a44772054c9076c8ef7682e3b6fbba2488107835911a773863"),
    "add_ln/768-strided/f32/arena": ("fcmf_add_ln_fwd fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd",
        "131df0f251cbf0a44772054c9076c8ef7682e3b6fbba2488107835911a773863"),
    "add_ln/768-strided/bf16": ("fcmf_add_ln_fwd fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd",
        "da745dcc289eeb42a794dd36a2516c7ffff3d36186d750e8057fbb7501fe4c30"),
    "add_ln/768-strided/bf16/arena": ("fcmf_add_ln_fwd fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd",
        "da745dcc289eeb42a794dd36a2516c7ffff3d36186d750e8057fbb7501fe4c30"),
    "add_ln/768-drop/f32": ("fcmf_add_ln_fwd fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd",
        "674481038bb9d399fd0e6f97f650301c45636965b58c380c012a1076f9e2efe3"),
    "add_ln/768-drop/f32/arena": ("fcmf_add_ln_fwd fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd",
        "674481038bb9d399fd0e6f97f650301c45636965b58c380c012a1076f9e2efe3"),
    "add_ln/768-drop/bf16": ("fcmf_add_ln_fwd fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd",
        "178448f9466ec47447fefc199866839daf69bfcc68e9061156f6baf6c07fee07"),
    "add_ln/768-drop/bf16/arena": ("fcmf_add_ln_fwd fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd",
        "178448f9466ec47447fefc199866839daf69bfcc68e9061156f6baf6c07fee07"),
    "embed_ln/64-tt/f32": ("fcmf_embed_ln_fwd fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_embed_pos_type_bwd fcmf_embed_bwd",
        "bd6eede8f333b7ffa490948413c8235a34a6ff5b387c3ac5f557ce29b1e2ed76"),
    "embed_ln/64-tt/f32/arena": ("fcmf_embed_ln_fwd fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_embed_pos_type_bwd fcmf_embed_bwd",
        "bd6eede8f333b7ffa490948413c8235a34a6ff5b387c3ac5f557ce29b1e2ed76"),
    "embed_ln/64-tt/bf16": ("fcmf_embed_ln_fwd fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_embed_pos_type_bwd fcmf_embed_bwd",
        "6b24bbbb1a0ee92f6b2e6674badfaefca893cf3fc5ff55f16f5dd75a66a1581b"),
    "embed_ln/64-tt/bf16/arena": ("fcmf_embed_ln_fwd fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_embed_pos_type_bwd fcmf_embed_bwd",
        "6b24bbbb1a0ee92f6b2e6674badfaefca893cf3fc5ff55f16f5dd75a66a1581b"),
    "embed_ln/64-nott/f32": ("fcmf_embed_ln_fwd fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_embed_pos_type_bwd fcmf_embed_bwd",
        "33868f28e65c002dada7d6c73f5fe817441fb460621dca19d1bed0b01ca4cb93"),
    "embed_ln/64-nott/f32/arena": ("fcmf_embed_ln_fwd fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_embed_pos_type_bwd fcmf_embed_bwd",
        "33868f28e65c002dada7d6c73f5fe817441fb460621dca19d1bed0b01ca4cb93"),
    "embed_ln/64-nott/bf16": ("fcmf_embed_ln_fwd fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_embed_pos_type_bwd fcmf_embed_bwd",
        "b638de1cfa7a80d27fca71b6fe787178c195746f22a7591e8603eebe495173f6"),
    "embed_ln/64-nott/bf16/arena": ("fcmf_embed_ln_fwd fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_embed_pos_type_bwd fcmf_embed_bwd",
        "b638de1cfa7a80d27fca71b6fe787178c195746f22a7591e8603eebe495173f6"),
    "embed_ln/36-tt/f32": ("fcmf_embed_ln_fwd fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_embed_pos_type_bwd fcmf_embed_bwd",
        "33c9512c9597cc19e0c406fbdc9658a611e7fbfb67c9d0579be6e05511ec34ff"),
    "embed_ln/36-tt/f32/arena": ("fcmf_embed_ln_fwd fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_embed_pos_type_bwd fcmf_embed_bwd",
        "33c9512c9597cc19e0c406fbdc9658a611e7fbfb67c9d0579be6e05511ec34ff"),
    "embed_ln/36-tt/bf16": ("fcmf_embed_ln_fwd fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_embed_pos_type_bwd fcmf_embed_bwd fcmf_embed_pos_bwd",
        "5535f98f70fe49206b951dbc48e52c28bf2d4b506973c195e2ae89b0de9aefed"),
    "embed_ln/36-tt/bf16/arena": ("fcmf_embed_ln_fwd fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_embed_pos_type_bwd fcmf_embed_bwd fcmf_embed_pos_bwd",
        "5535f98f70fe49206b951dbc48e52c28bf2d4b506973c195e2ae89b0de9aefed"),
    "embed_ln/36-nott/f32": ("fcmf_embed_ln_fwd fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_embed_pos_type_bwd fcmf_embed_bwd",
        "74fe0c8fd576bb0c8e1fec680fbd48d22e656bafddc4067da4dab1629aebe51e"),
    "embed_ln/36-nott/f32/arena": ("fcmf_embed_ln_fwd fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_embed_pos_type_bwd fcmf_embed_bwd",
        "74fe0c8fd576bb0c8e1fec680fbd48d22e656bafddc4067da4dab1629aebe51e"),
    "embed_ln/36-nott/bf16": ("fcmf_embed_ln_fwd fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_embed_pos_type_bwd fcmf_embed_bwd fcmf_embed_pos_bwd",
        "429d13d0429fdb8525416e51728d4dee7a123595cbb6d97231f01f53356a020b"),
    "embed_ln/36-nott/bf16/arena": ("fcmf_embed_ln_fwd fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_embed_pos_type_bwd fcmf_embed_bwd fcmf_embed_pos_bwd",
        "429d13d0429fdb8525416e51728d4dee7a123595cbb6d97231f01f53356a020b"),
    "embed_ln/64-tt-drop/f32": ("fcmf_embed_ln_fwd fcmf_dropout fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_embed_pos_type_bwd fcmf_embed_bwd",
        "393c786c9d85231d715b07e1a4f022183846fdcbfd90944dabfc49b83d7c70d7"),
    "embed_ln/64-tt-drop/f32/arena": ("fcmf_embed_ln_fwd fcmf_dropout fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_embed_pos_type_bwd fcmf_embed_bwd",
        "393c786c9d85231d715b07e1a4f022183846fdcbfd90944dabfc49b83d7c70d7"),
    "embed_ln/64-tt-drop/bf16": ("fcmf_embed_ln_fwd fcmf_dropout fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_embed_pos_type_bwd fcmf_embed_bwd",
        "d8adf4c5f05e8991492ebcfa59ee530cc249e76401138df3c0ceae15c2f2cc43"),
    "embed_ln/64-tt-drop/bf16/arena": ("fcmf_embed_ln_fwd fcmf_dropout fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_embed_pos_type_bwd fcmf_embed_bwd",
        "d8adf4c5f05e8991492ebcfa59ee530cc249e76401138df3c0ceae15c2f2cc43"),
    "embed_ln/64-nott-drop/f32": ("fcmf_embed_ln_fwd fcmf_dropout fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_embed_pos_type_bwd fcmf_embed_bwd",
        "6ec9367fac48d1ee3d1da05aa165fb0a41514e14e9564f86502ffbf082b26103"),
    "embed_ln/64-nott-drop/f32/arena": ("fcmf_embed_ln_fwd fcmf_dropout fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_embed_pos_type_bwd fcmf_embed_bwd",
        "6ec9367fac48d1ee3d1da05aa165fb0a41514e14e9564f86502ffbf082b26103"),
    "embed_ln/64-nott-drop/bf16": ("fcmf_embed_ln_fwd fcmf_dropout fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_embed_pos_type_bwd fcmf_embed_bwd",
        "9230c2d72ddfb95e5a2e97b6a64488b16c4f5cad9fb77dde5ae3f5aaa19c9d44"),
    "embed_ln/64-nott-drop/bf16/arena": ("fcmf_embed_ln_fwd fcmf_dropout fcmf_add_ln_bwd_workspace fcmf_add_ln_bwd fcmf_embed_pos_type_bwd fcmf_embed_bwd",
        "9230c2d72ddfb95e5a2e97b6a64488b16c4f5cad9fb77dde5ae3f5aaa19c9d44"),
}


@pytest.mark.parametrize("case", CASES)
def test_projection_library_calls(dev, case):
    calls, _ = run_case(dev, case)
    names = [c[0] for c in calls]
    print("MEASURED", repr(case), (" ".join(names), _calls_digest(calls)))
    exp_names, exp_digest = EXPECTED[case]
    assert names == exp_names.split()
    assert _calls_digest(calls) == exp_digest
    if case.startswith("vocab_topk"):      # the warm calls: one GEMM, one top-k, the same arguments both times
        assert names[-4:] == ["fcmf_gemm", "fcmf_logsoftmax_topk"] * 2 and calls[-4:-2] == calls[-2:]
