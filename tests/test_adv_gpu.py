"""FGM adversarial training on the text embeddings, on the GPU: fcmf_adv_scale and fcmf_embed_ln_adv_fwd (csrc/norm.hip) against
tests/adv_ref.py in guarded buffers, with NaN in the gradient rows of pad tokens (never read), and ops.EmbeddingAdversary's two
passes against float64 autograd running the same two passes on the device's own dz."""
import contextlib
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import adv_ref as A
import rowwise_ref as R
from helpers import _CallRecorder, rel_err

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
PAD = 1
SHAPES = [(1, 1, 4), (3, 5, 8), (2, 64, 768), (4, 170, 768), (2, 65, 1028), (1, 512, 2048)]


def _ops():
    from fcmf_framework import ops, _hip
    return ops, _hip


def _randn(shape, seed, dtype=F32):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dtype)


def _ids(nseq, S, seed=0, all_pad=None):
    """pads leading (odd sequences), interior (every sequence) and trailing (every third), where the sequence is long enough;
    all_pad: that sequence is nothing but pads"""
    ids = torch.randint(PAD + 1, 50, (nseq, S), generator=torch.Generator().manual_seed(seed))
    for s in range(nseq):
        if S >= 2 and s % 2 == 1:
            ids[s, 0] = PAD
        if S >= 3:
            ids[s, S // 2] = PAD
        if S >= 5 and s % 3 == 0:
            ids[s, S - S // 4:] = PAD
    if all_pad is not None:
        ids[all_pad] = PAD
    return ids


def _poison(g, ids):
    g = g.clone()
    g[ids.eq(PAD)] = float("nan")
    return g


def _scale(dev, g, ids, eps):
    """fcmf_adv_scale on g [nseq, S, H] (its dtype) -> float32 [nseq] on the host, out of a guarded buffer"""
    _, H = _ops()
    nseq, S, Hd = g.shape
    gd, idd = g.to(dev).contiguous(), ids.to(dev)
    out = R.guarded((nseq,), F32, dev)
    rc = H.lib().fcmf_adv_scale(H.ptr(gd), H.ptr(idd), H.ptr(out.view), nseq, S, Hd, PAD, eps, H.dt(gd), H.stream())
    assert rc == 0
    torch.cuda.synchronize()
    out.check()
    return out.view.cpu().clone()


# ---- fcmf_adv_scale ---------------------------------------------------------------------------------------------------------------
def scale_bound(S, Hd, dtype):
    """Relative error bound of scale[s], from the kernel's own summation (csrc/norm.hip adv_scale_kernel), u = 2^-24:
    * the values are divided by a power of two: exact.  A lane owns V = 4 (float32; bf16 rows that are no multiple of 8) or 8
      adjacent elements of every 64 * V columns of every fourth row: L = ceil(S / 4) * ceil(H / (64 * V)) * V terms, each
      squared (one rounding, none where the compiler contracts to an fma) and added serially (one rounding per add): a
      term's relative error is at most L * u to first order;
    * wave_sum adds 64 lanes in 6 steps, thread 0 adds the 4 waves in 3: 9 more roundings.  The terms are >= 0, so the sum's
      relative error is at most (L + 9) * u;
    * the square root halves it and rounds once (correctly rounded: + u), the divide rounds once (+ u), the final power of two
      is exact: ((L + 9) / 2 + 2) * u.  Second-order terms: (L + 9) * u <= 2.5e-4 at the largest shape, so a factor 1.001."""
    V = 4 if dtype == F32 or Hd % 8 else 8
    L = math.ceil(S / 4) * math.ceil(Hd / (64 * V)) * V
    return ((L + 9) / 2 + 2) * 2.0 ** -24 * 1.001


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("shape", SHAPES)
def test_scale_against_float64_on_the_same_operands(dev, shape, dtype):
    """general data with pads leading, interior and trailing and NaN in their rows; from three sequences on, the last one is all
    pad and the one before it has a zero gradient: scale 0.  Bound: scale_bound's docstring"""
    nseq, S, Hd = shape
    eps = 0.625
    ids = _ids(nseq, S, seed=S, all_pad=nseq - 1 if nseq >= 3 else None)
    g = _randn(shape, seed=Hd, dtype=dtype)
    if nseq >= 3:
        g[nseq - 2] = 0
    g = _poison(g, ids)
    got = _scale(dev, g, ids, eps)
    want = A.scale(g, ids, PAD, eps)
    assert torch.isfinite(got).all()
    if nseq >= 3:
        assert got[nseq - 1] == 0 and got[nseq - 2] == 0 and want[nseq - 1] == 0 and want[nseq - 2] == 0
    live = want > 0
    assert live.any()
    err = ((got.double() - want).abs()[live] / want[live]).max().item()
    bound = scale_bound(S, Hd, dtype)
    print(f"adv_scale {shape} {dtype}: max relative error {err:.3e}, bound {bound:.3e}, ratio {err / bound:.4f}")
    assert err <= bound


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("shape", [(3, 5, 8), (2, 65, 1028), (4, 170, 768)])
def test_scale_of_one_nonzero_element_is_exact(dev, shape, dtype):
    """one element +-2^k per sequence, zeros elsewhere, NaN at pads: scale = epsilon * 2^-k exactly (the normalised value is 1)"""
    nseq, S, Hd = shape
    eps = 0.75
    ids = _ids(nseq, S, seed=2)
    for k in (-100, -3, 0, 7, 100):
        g = torch.zeros(shape, dtype=dtype)
        for s in range(nseq):
            t = int(ids[s].ne(PAD).nonzero()[-1 if s % 2 else 0])      # the first or the last live token
            g[s, t, (5 * s + 3) % Hd] = (-1.0) ** s * 2.0 ** k
        got = _scale(dev, _poison(g, ids), ids, eps)
        want = torch.full((nseq,), float(np.float32(eps) * np.float32(2.0 ** -k)))
        assert torch.equal(got, want), k


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("shape,ms", [((3, 5, 8), (0, 1, 2)), ((4, 170, 768), (3, 8)), ((1, 512, 2048), (10,))])
def test_scale_of_a_power_of_four_equal_elements_is_exact(dev, shape, ms, dtype):
    """4^m elements 2^k (the first ones of the live region, zeros after them) and epsilon = 2^j: every partial sum is an
    integer below 2^24, the root is 2^m: scale = 2^(j - m - k) exactly, in any order of summation"""
    nseq, S, Hd = shape
    ids = _ids(nseq, S, seed=3) if nseq > 1 else torch.full((1, S), PAD + 1)
    for m in ms:
        for k, j in ((-40, 3), (0, 0), (5, -2), (60, 1)):
            g = torch.zeros(shape, dtype=dtype)
            for s in range(nseq):
                livet = ids[s].ne(PAD).nonzero().flatten()
                assert 4 ** m <= livet.numel() * Hd
                flat = g[s, livet].reshape(-1)
                flat[:4 ** m] = 2.0 ** k
                g[s, livet] = flat.view(-1, Hd)
            got = _scale(dev, _poison(g, ids), ids, 2.0 ** j)
            assert torch.equal(got, torch.full((nseq,), 2.0 ** (j - m - k))), (m, k, j)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("shape", [(3, 5, 8), (2, 65, 1028), (4, 170, 768)])
def test_scaling_the_gradient_by_a_power_of_two_scales_the_result_exactly(dev, shape, dtype):
    """dz * 2^k, k in [-70, 70], divides scale by exactly 2^k, bit for bit: a plain sum of squares would underflow to 0 or
    overflow to inf in float32.  Magnitudes are kept in [2^-10, 2^3] so that 2^k * dz is exact in the storage type"""
    nseq, S, Hd = shape
    ids = _ids(nseq, S, seed=4)
    g = _randn(shape, seed=11).clamp(-8, 8)
    g = torch.where(g.abs() < 2.0 ** -10, torch.full_like(g, 2.0 ** -10), g).to(dtype)
    base = _scale(dev, _poison(g, ids), ids, 1.5)
    assert torch.isfinite(base).all() and (base > 0).all()
    for k in (-70, -13, 1, 70):
        gk = (g.double() * 2.0 ** k).to(dtype)
        assert torch.equal(gk.double(), g.double() * 2.0 ** k)          # exact in the storage type
        got = _scale(dev, _poison(gk, ids), ids, 1.5)
        assert torch.equal(got.double() * 2.0 ** k, base.double()), k
    again = _scale(dev, _poison(g, ids), ids, 1.5)
    assert torch.equal(again, base)                                     # no atomics: the same bits every run


# ---- fcmf_embed_ln_adv_fwd ----------------------------------------------------------------------------------------------------------
def _fwd_case(ntok, Hd, dtype):
    nseq, S = {1: (1, 1), 15: (3, 5), 340: (2, 170)}[ntok]
    V, Pn = 50, S + PAD + 1
    ids = _ids(nseq, S, seed=Hd)
    m = ids.ne(PAD).long()
    pos = torch.cumsum(m, 1) * m + PAD
    tt = torch.zeros_like(ids)
    tt[:, S // 2:] = 1
    # (the word table carries an offset: rel_err is relative to the largest reference entry, which for ntok = 1 is the one row's
    #  mean -- around 0 a sum that cancels, whose float32 error of an ulp of its TERMS says nothing about the kernel)
    word, ptab, ttab = 2.0 + _randn((V, Hd), 1), _randn((Pn, Hd), 2), _randn((2, Hd), 3)
    gamma, beta = 1 + 0.1 * _randn((Hd,), 4), _randn((Hd,), 5)
    g = _randn((nseq, S, Hd), 6, dtype)
    sc = (0.25 + torch.rand(nseq, generator=torch.Generator().manual_seed(7))).float()
    return ids, pos, tt, (word, ptab, ttab, gamma, beta), g, sc


def _launch(dev, name, ids, pos, tt, params, dtype, p, seed, g=None, sc=None):
    """one of the two forward entry points into guarded outputs -> y, z, mean, rstd on the host"""
    _, H = _ops()
    ntok, Hd = ids.numel(), params[0].shape[1]
    d = lambda t: None if t is None else t.to(dev).contiguous()
    idd, pd, td = d(ids), d(pos), d(tt)
    pr = [d(t) for t in params]
    outs = [R.guarded((ntok, Hd), dtype, dev), R.guarded((ntok, Hd), dtype, dev), R.guarded((ntok,), F32, dev),
            R.guarded((ntok,), F32, dev)]
    args = [H.ptr(idd), H.ptr(pd), H.ptr(td), *map(H.ptr, pr), *(H.ptr(o.view) for o in outs), ntok, Hd, 1e-5, p, seed,
            H.dt(outs[0].view), H.stream()]
    if g is not None:
        gd, sd = d(g), d(sc)
        args += [H.ptr(gd), H.ptr(sd), ids.shape[-1], PAD]
    assert getattr(H.lib(), name)(*args) == 0
    torch.cuda.synchronize()
    R.check_all(*outs)
    return [o.view.cpu().clone() for o in outs]


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("ntok", [1, 15, 340])
@pytest.mark.parametrize("Hd", [4, 8, 256, 260, 768, 1028, 2048])
def test_adv_forward_against_the_reference(dev, Hd, ntok, dtype):
    """every pass count (H 4 .. 2048) at token counts that are no multiple of the four rows per workgroup, with and without type
    ids, p 0 and 0.1: y, z, mean, rstd within the plain kernel's bounds (tests/test_embed_gpu.py: 2e-5 float32, 3e-2 bf16
    rel_err); pad rows equal the plain kernel's; with scale 0 and a finite g every output equals the plain kernel's"""
    ids, pos, tt, params, g, sc = _fwd_case(ntok, Hd, dtype)
    tol = 2e-5 if dtype == F32 else 3e-2
    padrow = ids.reshape(-1).eq(PAD)
    gp = _poison(g, ids)
    for types in (tt, None):
        for p in (0.0, 0.1):
            seed = R.EMBED_SEED if p > 0 else 0
            mask = R.mask_tensor(seed, (ntok, Hd), p) if p > 0 else None
            got = _launch(dev, "fcmf_embed_ln_adv_fwd", ids, pos, types, params, dtype, p, seed, gp, sc)
            want = A.embed_ln_adv(ids, pos, types, *params, 1e-5, gp, sc, PAD, mask, p)
            for name, a, r in zip(("y", "z", "mean", "rstd"), got, want):
                assert torch.isfinite(a.float()).all(), name
                assert rel_err(a, r) < tol, (name, types is None, p)
            if mask is not None:
                assert torch.equal(got[0] != 0, mask.bool() & (want[0] != 0))
            plain = _launch(dev, "fcmf_embed_ln_fwd", ids, pos, types, params, dtype, p, seed)
            for name, a, b in zip(("y", "z", "mean", "rstd"), got, plain):
                assert torch.equal(a[padrow], b[padrow]), name
            if (~padrow).any():
                assert not torch.equal(got[1][~padrow], plain[1][~padrow])      # ... and the live rows do not
            zero = _launch(dev, "fcmf_embed_ln_adv_fwd", ids, pos, types, params, dtype, p, seed, g, torch.zeros_like(sc))
            for name, a, b in zip(("y", "z", "mean", "rstd"), zero, plain):
                assert torch.equal(a, b), name


# ---- ops.EmbeddingAdversary -----------------------------------------------------------------------------------------------------------
class _Tiny:
    """embed -> (mean over tokens) -> linear -> cross entropy over one or several id tensors, parameters on the device"""

    def __init__(self, dev, Hd, dtype, V=50, Pn=24, C=3):
        shapes = ((V, Hd), (Pn, Hd), (2, Hd))
        self.tables = [_randn(s, i).to(dev).requires_grad_(True) for i, s in enumerate(shapes)]
        self.gamma = (1 + 0.1 * _randn((Hd,), 7)).to(dev).requires_grad_(True)
        self.beta = _randn((Hd,), 8).to(dev).requires_grad_(True)
        self.W = _randn((C, Hd), 9).to(dev).requires_grad_(True)
        self.dtype, self.dev, self.C = dtype, dev, C
        self.ys = []

    def params(self):
        return [*self.tables, self.gamma, self.beta, self.W]

    def loss(self, id_list, training=True):
        ops, _ = _ops()
        self.ys, total = [], 0.0
        for n, ids in enumerate(id_list):
            idd = ids.to(self.dev)
            pos = ops.position_ids(idd.view(-1, ids.shape[-1]), PAD).view(ids.shape)
            y = ops.embed_layer_norm(idd, pos, None, *self.tables, self.gamma, self.beta, 1e-5, 0.0, training, PAD, self.dtype)
            self.ys.append(y)
            logits = y.float().mean(-2).reshape(-1, y.shape[-1]) @ self.W.t()
            labels = (torch.arange(logits.shape[0], device=self.dev) + n) % self.C
            total = total + F.cross_entropy(logits, labels, reduction="sum")
        return total


def _reference_two_passes(model, id_list, deltas):
    """float64 autograd of the clean loss plus the loss on embeddings + deltas (constants) -> the adversarial pass's y per call,
    the summed gradients of model.params()"""
    P = [t.detach().double().cpu().requires_grad_(True) for t in model.params()]
    word, ptab, ttab, gamma, beta, W = P
    ys = []
    for delta_list in (None, deltas):
        total = 0.0
        for n, ids in enumerate(id_list):
            m = ids.ne(PAD).long()
            pos = torch.cumsum(m, -1) * m + PAD
            e = (F.embedding(ids, word, padding_idx=PAD) + ttab[torch.zeros_like(ids)]) + F.embedding(pos, ptab, padding_idx=PAD)
            if delta_list is not None:
                e = e + delta_list[n].view(e.shape)
            y = F.layer_norm(e, (e.shape[-1],), gamma, beta, 1e-5)
            if delta_list is not None:
                ys.append(y.detach())
            logits = y.mean(-2).reshape(-1, y.shape[-1]) @ W.t()
            total = total + F.cross_entropy(logits, (torch.arange(logits.shape[0]) + n) % model.C, reduction="sum")
        total.backward()
    return ys, [t.grad for t in P]


def _two_passes(dev, dtype, id_list, eps, Hd=64):
    ops, _ = _ops()
    model = _Tiny(dev, Hd, dtype)
    adv = ops.EmbeddingAdversary(eps)
    with adv.record():
        clean = model.loss(id_list)
    assert adv.recorded() == len(id_list)
    clean.backward()
    recs = [(dz.detach().cpu().clone(), ids.cpu().clone()) for dz, ids in adv._records]
    with adv.attack():
        attacked = model.loss(id_list)
    assert adv.recorded() == 0                                          # released
    ys = [y.detach().cpu() for y in model.ys]
    attacked.backward()
    torch.cuda.synchronize()
    deltas = []
    for (dz, rids), ids in zip(recs, id_list):                          # matched in order
        assert torch.equal(rids, ids) and dz.dtype == dtype and dz.shape == (ids.numel(), Hd)
        g = dz.view(-1, ids.shape[-1], Hd)
        deltas.append(A.perturbation(g, ids, PAD, A.scale(g, ids, PAD, eps)))
    ref_ys, ref_grads = _reference_two_passes(model, id_list, deltas)
    return model, clean, attacked, ys, ref_ys, ref_grads


def _batch(shape, seed):
    ids = torch.randint(PAD + 1, 50, shape, generator=torch.Generator().manual_seed(seed))
    flat = ids.view(-1, shape[-1])
    flat[0, 3:] = PAD
    flat[1, 0] = PAD
    flat[2 % flat.shape[0], 2] = PAD
    return ids


@pytest.mark.parametrize("layout", ["one_call", "two_calls", "3d"])
def test_adversary_gradients_against_float64_autograd_of_the_same_two_passes(dev, layout):
    """float32: the summed gradient of every parameter after clean + adversarial backward against float64 autograd running the
    same two passes, the reference's perturbation built from the device's own dz (only forward and backward error enters);
    bounds of tests/test_embed_gpu.py: 2e-5 forward, twice that for gradients.  two_calls: two embedding calls per forward (a
    target and a sentence of other shapes) are matched in order; 3d: ids [B, A, S]"""
    id_list = {"one_call": [_batch((3, 5), 1)], "two_calls": [_batch((2, 4), 2), _batch((3, 7), 3)],
               "3d": [_batch((2, 2, 5), 4)]}[layout]
    model, clean, attacked, ys, ref_ys, ref_grads = _two_passes(dev, F32, id_list, eps=0.5)
    assert math.isfinite(clean.item()) and math.isfinite(attacked.item())
    assert attacked.item() != clean.item()
    for y, r in zip(ys, ref_ys):
        assert rel_err(y, r) < 2e-5
    for name, a, r in zip(("word", "pos", "type", "gamma", "beta", "W"), model.params(), ref_grads):
        assert torch.isfinite(a.grad).all()
        assert rel_err(a.grad, r) < 4e-5, name


def test_adversary_forward_in_bf16(dev):
    """the bf16 adversarial forward against the reference on the device's own (bf16) dz: 3e-2 rel_err"""
    model, clean, attacked, ys, ref_ys, _ = _two_passes(dev, BF16, [_batch((3, 5), 1), _batch((2, 9), 5)], eps=0.5)
    assert math.isfinite(clean.item()) and math.isfinite(attacked.item())
    for y, r in zip(ys, ref_ys):
        assert y.dtype == BF16 and rel_err(y, r) < 3e-2


def test_adversary_mismatches_and_a_frozen_table_raise(dev):
    ops, _ = _ops()
    model = _Tiny(dev, 16, F32)
    a, b = _batch((3, 5), 1), _batch((3, 6), 2)
    adv = ops.EmbeddingAdversary(0.5)
    with adv.record():
        loss = model.loss([a])
    loss.backward()
    with pytest.raises(ValueError, match="more embedding calls"):
        with adv.attack():
            model.loss([a, a])
    assert adv.recorded() == 0 and ops._adversary is None
    with adv.record():
        loss = model.loss([a, b])
    loss.backward()
    with pytest.raises(ValueError, match="made 1 embedding calls, the clean pass recorded 2"):
        with adv.attack():
            model.loss([a])
    with adv.record():
        loss = model.loss([a])
    loss.backward()
    with pytest.raises(ValueError, match="ids"):
        with adv.attack():
            model.loss([b])
    with adv.record():
        model.loss([a])                                                 # no backward
    with pytest.raises(ValueError, match="backward"):
        with adv.attack():
            model.loss([a])
    model.tables[0].requires_grad_(False)                               # a frozen word table registers nothing
    with adv.record():
        model.loss([a]).backward()
    assert adv.recorded() == 0
    with pytest.raises(ValueError, match="must be trainable"):
        with adv.attack():
            model.loss([a])


def test_eval_mode_and_no_grad_record_nothing(dev):
    ops, _ = _ops()
    model = _Tiny(dev, 16, F32)
    a = _batch((3, 5), 1)
    adv = ops.EmbeddingAdversary(0.5)
    with adv.record():
        plain = model.loss([a], training=False)
        assert adv.recorded() == 0
        with torch.no_grad():
            model.loss([a])
        assert adv.recorded() == 0
        model.loss([a])
        assert adv.recorded() == 1
    # inside attack(), calls that take no part run the plain kernel and use up no record
    with adv.record():
        model.loss([a]).backward()
    with adv.attack():
        again = model.loss([a], training=False)
        with torch.no_grad():
            model.loss([a])
        model.loss([a])
    assert torch.equal(plain.detach(), again.detach())


@contextlib.contextmanager
def _recording():
    _, H = _ops()
    real = H.lib()
    H._lib = rec = _CallRecorder(real, H.SIGNATURES)
    try:
        yield rec
    finally:
        H._lib = real


def test_a_plain_training_pass_makes_the_calls_it_always_made(dev):
    """forward + backward with no adversary active: the same library calls before an adversary has run as after one has, and
    they are the plain step's (no fcmf_adv_scale, no fcmf_embed_ln_adv_fwd); with dropout, so that the seed draws count too"""
    ops, _ = _ops()
    ids = _batch((3, 5), 1)

    def plain_pass():
        ops.manual_seed(7)
        model = _Tiny(dev, 64, BF16)
        idd = ids.to(dev)
        pos = ops.position_ids(idd, PAD)
        with _recording() as rec:
            y = ops.embed_layer_norm(idd, pos, None, *model.tables, model.gamma, model.beta, 1e-5, 0.1, True, PAD, BF16)
            y.float().sum().backward()
            torch.cuda.synchronize()
        return rec.calls, y.detach().cpu()

    before, y0 = plain_pass()
    _two_passes(dev, BF16, [ids], eps=0.5)
    after, y1 = plain_pass()
    assert before == after and torch.equal(y0, y1)
    assert [c[0] for c in before] == ["fcmf_embed_ln_fwd", "fcmf_dropout", "fcmf_add_ln_bwd_workspace", "fcmf_add_ln_bwd",
                                      "fcmf_embed_pos_type_bwd", "fcmf_embed_bwd"]
    assert all(c[2] == 0 for c in before if c[0] != "fcmf_add_ln_bwd_workspace")
