"""Long-key, shared-K/V MFMA attention (csrc/attn_long.hip, ops.shared_kv_attention) against a float64 torch restatement
on the same bf16 operands, against the VALU kernel under dropout, and against itself (determinism, the adjoint identity
that ties the backward's dropout mask to the forward's).  heads 2, head dim 64.

Bounds: rel_err < 3e-2 is the bound of the existing MFMA attention tests (test_ops_gpu.py, bf16 storage: 8 significant
bits); the adjoint identity uses the rtol 2e-2 of test_attention_dropout_consistent's neighbours."""
import math

import pytest
import torch

from helpers import mfma_attention, rel_err

pytestmark = pytest.mark.gpu

HEADS, D = 2, 64
HD = HEADS * D
FMIN = torch.finfo(torch.float32).min
#        G  kv_share  Tq   Tk
CASES = [(4, 2, 16, 257), (6, 6, 170, 371), (4, 1, 170, 595), (2, 2, 256, 640), (6, 3, 1, 300), (3, 1, 33, 129)]
IDS = ["G%d-share%d-Tq%d-Tk%d" % c for c in CASES]


def _rand(shape, dev, seed, scale=0.8):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(torch.bfloat16).to(dev)


def _operands(G, share, Tq, Tk, dev):
    return (_rand((G, Tq, HD), dev, 1), _rand((G // share, Tk, HD), dev, 2), _rand((G // share, Tk, HD), dev, 3),
            _rand((G, Tq, HD), dev, 4))


def _mask(G, Tk, roles, seed=7):
    """additive float32 key mask [G, Tk]; the role of group g is roles[g]:
       random   25 % of the keys hard-masked, key 0 live
       interior keys 128..383 masked (whole 128-key tiles), 25 % of the rest too, key 0 live
       last     only key Tk-1 live
       full     no live key at all (softmax is uniform over all keys)"""
    gen = torch.Generator().manual_seed(seed)
    dead = torch.rand(G, Tk, generator=gen) < 0.25
    dead[:, 0] = False
    for g, role in enumerate(roles):
        if role == "interior":
            dead[g, 128:384] = True
        elif role == "last":
            dead[g] = True
            dead[g, Tk - 1] = False
        elif role == "full":
            dead[g] = True
    return dead.float() * FMIN


def _roles(G):
    return (["interior", "last", "full"] + ["random"] * G)[:G]


def _ref(q, k, v, mask, share, w):
    """float64 restatement on the CPU: out, dq, dk, dv (dk / dv summed over the sharing groups by autograd)"""
    c = lambda t: t.detach().double().cpu().requires_grad_(True)
    qr, kr, vr = c(q), c(k), c(v)
    G, Tq, _ = q.shape
    sp = lambda t: t.view(t.shape[0], t.shape[1], HEADS, D).transpose(1, 2)
    ke, ve = kr.repeat_interleave(share, 0), vr.repeat_interleave(share, 0)
    sc = sp(qr) @ sp(ke).transpose(-1, -2) / math.sqrt(D)
    if mask is not None:
        sc = sc + mask.double().cpu()[:, None, None, :]
    out = (torch.softmax(sc, -1) @ sp(ve)).transpose(1, 2).reshape(G, Tq, HD)
    (out * w.double().cpu()).sum().backward()
    return out.detach(), qr.grad, kr.grad, vr.grad


def _run(ops, q0, k0, v0, w, mask, share, p=0.0, seed=5):
    q, k, v = (t.clone().requires_grad_(True) for t in (q0, k0, v0))
    ops.manual_seed(seed)
    out = ops.shared_kv_attention(q, k, v, mask=mask, heads=HEADS, kv_share=share, p=p, training=p > 0)
    (out.float() * w.float()).sum().backward()
    return out.detach(), q.grad, k.grad, v.grad


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "masks"])
@pytest.mark.parametrize("G,share,Tq,Tk", CASES, ids=IDS)
def test_long_attention_matches_float64(dev, G, share, Tq, Tk, masked):
    """p = 0: out, dq, dk, dv.  With masks: whole interior tiles masked, a single live key at the very end, a group with no
    live key (uniform; dq / dk as autograd gives them) and random holes; keys that are hard-masked for every group of a key
    set (none of which is the uniform one) get dk = dv = 0 exactly."""
    from fcmf_framework import ops
    q0, k0, v0, w = _operands(G, share, Tq, Tk, dev)
    roles = _roles(G)
    mask = _mask(G, Tk, roles).to(dev) if masked else None
    got = _run(ops, q0, k0, v0, w, mask, share)
    ref = _ref(q0, k0, v0, mask, share, w)
    errs = {n: rel_err(a, b) for a, b, n in zip(got, ref, ("out", "dq", "dk", "dv"))}
    print(IDS[CASES.index((G, share, Tq, Tk))], "masked" if masked else "plain", errs)
    for n, e in errs.items():
        assert e < 3e-2, (n, e)
    if masked:
        dead = (mask.cpu() < -1e30).view(G // share, share, Tk)
        uniform = dead.all(2).any(1)                         # key sets read by a group without any live key
        zero = dead.all(1) & ~uniform[:, None]               # [G/share, Tk]
        for t in got[2:]:
            assert (t.float().cpu()[zero] == 0).all()


def test_keys_masked_for_all_sharers_get_exactly_zero_gradients(dev):
    """three groups per key set, every group with live keys: the keys (and whole 32-key chunks and 128-key tiles) that all
    three mask have dk = dv = 0, the others match float64"""
    from fcmf_framework import ops
    G, share, Tq, Tk = 6, 3, 40, 300
    q0, k0, v0, w = _operands(G, share, Tq, Tk, dev)
    mask = _mask(G, Tk, ["random"] * G)
    mask[:, 3:9] = FMIN
    mask[:, 120:260] = FMIN
    mask[:3, 290:] = FMIN          # the tail of key set 0 only
    mask = mask.to(dev)
    got = _run(ops, q0, k0, v0, w, mask, share)
    ref = _ref(q0, k0, v0, mask, share, w)
    for a, b, n in zip(got, ref, ("out", "dq", "dk", "dv")):
        assert rel_err(a, b) < 3e-2, n
    zero = (mask.cpu() < -1e30).view(G // share, share, Tk).all(1)
    assert zero[:, 120:260].all() and zero[0, 290:].all() and not zero[1, 290:].all()
    for t in got[2:]:
        assert (t.float().cpu()[zero] == 0).all()
        assert (t.float().cpu()[~zero] != 0).any()


@pytest.mark.parametrize("G,Tq,Tk", [(c[0], c[2], c[3]) for c in CASES if c[3] <= 512],
                         ids=[i for c, i in zip(CASES, IDS) if c[3] <= 512])
def test_long_attention_dropout_equals_valu_kernel(dev, G, Tq, Tk):
    """p = 0.2, kv_share = 1, Tk <= 512: the dropout counter is the VALU kernel's, so at the same seed both drop the same
    elements (odd Tk: per-element hashes in the backward; even Tk: the pair-sharing form)"""
    from fcmf_framework import ops
    q0, k0, v0, w = _operands(G, 1, Tq, Tk, dev)
    mask = _mask(G, Tk, ["random"] * G).to(dev)
    got = _run(ops, q0, k0, v0, w, mask, 1, p=0.2)
    with mfma_attention(False):
        q, k, v = (t.clone().requires_grad_(True) for t in (q0, k0, v0))
        ops.manual_seed(5)
        out = ops.attention(q, k, v, mask=mask, heads=HEADS, p=0.2, training=True)
        (out.float() * w.float()).sum().backward()
    for a, b, n in zip(got, (out, q.grad, k.grad, v.grad), ("out", "dq", "dk", "dv")):
        e = rel_err(a, b)
        print(G, Tq, Tk, n, e)
        assert e < 3e-2, (n, e)


@pytest.mark.parametrize("G,share,Tq,Tk", CASES, ids=IDS)
def test_long_attention_dropout_deterministic_and_adjoint(dev, G, share, Tq, Tk):
    """p = 0.2 at a fixed seed: two runs give identical outputs, and the backward drops what the forward dropped --
    out is linear in V under a fixed mask, so sum(dv * V2) = sum(w * out(q, k, V2)) for any V2.  V2 = dv itself keeps
    the identity well conditioned (both sides are |dv|^2 when the masks agree; with independent masks they differ by the
    mask's variance, tens of percent)."""
    from fcmf_framework import ops
    q0, k0, v0, w = _operands(G, share, Tq, Tk, dev)
    mask = _mask(G, Tk, ["random"] * G).to(dev)
    a = _run(ops, q0, k0, v0, w, mask, share, p=0.2)
    b = _run(ops, q0, k0, v0, w, mask, share, p=0.2)
    assert torch.equal(a[0], b[0])
    plain = _run(ops, q0, k0, v0, w, mask, share)
    assert not torch.equal(a[0], plain[0])
    v2 = a[3].detach().clone()
    ops.manual_seed(5)
    out2 = ops.shared_kv_attention(q0, k0, v2, mask=mask, heads=HEADS, kv_share=share, p=0.2, training=True)
    lhs = (a[3].double() * v2.double()).sum().item()
    rhs = (w.double() * out2.double()).sum().item()
    print(IDS[CASES.index((G, share, Tq, Tk))], "adjoint", lhs, rhs, abs(lhs - rhs) / abs(rhs))
    assert lhs > 0 and abs(lhs - rhs) <= 2e-2 * abs(rhs)


@pytest.mark.parametrize("Tk", [285, 286, 595])
def test_float32_parity_mode(dev, Tk):
    """float32 runs the VALU kernels once per sharing member: in one piece up to the number of keys whose float32 K / V images
    fit in LDS (285 at head dim 64), beyond that in chunks of 256 merged by their logsumexps (286: a chunk of 30 keys; 595:
    three chunks, one of them wholly masked for a group).  Against float64; 1e-4 = float32 sums over <= 595 terms with room."""
    from fcmf_framework import ops
    assert ops.valu_float32_key_limit(D) == 285
    G, share, Tq = 6, 3, 20
    q0, k0, v0, w = _operands(G, share, Tq, Tk, dev)
    mask = _mask(G, Tk, ["interior", "last"] + ["random"] * 4).to(dev)      # (a group without live keys: not covered by the chunks)
    got = _run(ops, q0.float(), k0.float(), v0.float(), w, mask, share)
    ref = _ref(q0, k0, v0, mask, share, w)
    for a, b, n in zip(got, ref, ("out", "dq", "dk", "dv")):
        e = rel_err(a, b)
        print("float32", Tk, n, e)
        assert e < 1e-4, (n, e)


def test_unsupported_configurations_say_so(dev):
    from fcmf_framework import ops
    from fcmf_framework._hip import HipLibraryError
    bf = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device=dev)
    for q, k, heads in ((bf(2, 257, HD), bf(2, 300, HD), HEADS),        # Tq > 256
                        (bf(2, 16, HD), bf(2, 300, HD), 4)):            # bf16 with head dim 32
        with pytest.raises(HipLibraryError, match="unsupported"):
            ops.shared_kv_attention(q, k, k, heads=heads)
    with pytest.raises(HipLibraryError, match="query groups per key set"):
        ops.shared_kv_attention(bf(3, 16, HD), bf(2, 300, HD), bf(2, 300, HD), heads=HEADS, kv_share=2)
