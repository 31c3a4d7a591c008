"""The weight EMA on the GPU: `fcmf_multi_adamw_ema` and `fcmf_multi_swap` called directly on guarded buffers (the AdamW half
bit-identical to `fcmf_multi_adamw`, the average bit-identical to the stated float32 formula, results independent of alignment,
the swap exact with its bf16 shadows), `FusedAdamW.set_ema` / `ema_weights()` with the weight-shadow cache in the loop (the
stale-shadow checks), the optimizer state round trip, and the drivers' `--ema_decay`.  Every comparison is bit for bit."""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch

import synthetic_data as synth
from helpers import _recorded, make_hf_dir

pytestmark = pytest.mark.gpu

CHUNK = 256                                      # small tensors cross chunk borders
SIZES = [1, 3, 4, 7, 255, 256, 257, 1021]
GROUP = [0, 1, 0, 1, 0, 1, 0, 1]
LR, WD = (7e-3, 3e-2), (0.01, 0.0)
PAD = 64                                         # frame elements on either side of a tensor (a whole number of 16-byte units)
SENT = {torch.float32: 12345.0, torch.bfloat16: 12352.0}


def _bits(t):
    return t.detach().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu()


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _values(n, seed, positive=False):
    """seeded normals scaled into [1e-3, 1e3] in magnitude: no intermediate of either update is subnormal"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g) * 10.0 ** float(torch.randint(-2, 3, (1,), generator=g))
    x = torch.where(x >= 0, 1.0, -1.0) * x.abs().clamp(1e-3, 1e3)
    return x.abs() if positive else x


class Slot:
    """a tensor `off` elements into the 16-byte-aligned interior of a sentinel-filled buffer; `check()`: the frame is intact"""

    def __init__(self, values, off, dev, dtype=torch.float32):
        n = values.numel()
        self.buf = torch.full((n + 2 * PAD + 4,), SENT[dtype], dtype=dtype, device=dev)
        assert self.buf.data_ptr() % 16 == 0
        self.lo, self.hi = PAD + off, PAD + off + n
        self.t = self.buf[self.lo:self.hi]
        self.t.copy_(values.to(dtype))

    def check(self):
        s = SENT[self.buf.dtype]
        assert bool((self.buf[:self.lo] == s).all()), "write before the start of a tensor"
        assert bool((self.buf[self.hi:] == s).all()), "write past the end of a tensor"

    def untouched(self):
        return bool((self.buf == SENT[self.buf.dtype]).all())


class Layout:
    """p, g, m, v, e and bf16 shadow slots of the eight tensors; off: kind -> element offset (bf16: in bf16 elements)"""

    def __init__(self, dev, off=None, seed=0):
        off = off or {}
        mk = lambda kind, base, positive=False: [Slot(_values(n, seed + base + i, positive), off.get(kind, 0), dev)
                                                 for i, n in enumerate(SIZES)]
        self.dev = dev
        self.p, self.g, self.m, self.v, self.e = mk("p", 0), mk("g", 100), mk("m", 200), mk("v", 300, True), mk("e", 400)
        self.sh = [Slot(torch.zeros(n), off.get("sh", 0), dev, torch.bfloat16) for n in SIZES]
        for s in self.sh:
            s.buf.fill_(SENT[torch.bfloat16])
        ct = [t for t, n in enumerate(SIZES) for _ in range(0, n, CHUNK)]
        co = [o for n in SIZES for o in range(0, n, CHUNK)]
        i64 = lambda xs: torch.tensor(xs, dtype=torch.int64, device=dev)
        self.sizes, self.group = i64(SIZES), torch.tensor(GROUP, dtype=torch.int32, device=dev)
        self.ct, self.co, self.nchunks = torch.tensor(ct, dtype=torch.int32, device=dev), i64(co), len(ct)
        self.sumsq = torch.zeros(1, dtype=torch.float64, device=dev)

    def table(self, slots, skip=()):
        return torch.tensor([0 if i in skip else s.t.data_ptr() for i, s in enumerate(slots)], dtype=torch.int64, device=self.dev)

    def set_grads(self, seed):
        for i, (s, n) in enumerate(zip(self.g, SIZES)):
            s.t.copy_(_values(n, seed + i))
        self.sumsq.copy_(sum(s.t.double().pow(2).sum() for s in self.g))

    def check(self):
        torch.cuda.synchronize()
        for s in self.p + self.g + self.m + self.v + self.e + self.sh:
            s.check()

    def read(self, kind):
        return [s.t.detach().cpu().clone() for s in getattr(self, kind)]


NO_SHADOW = (2, 5)       # table entries left 0 when shadows are asked for


def _adamw(L, step, max_norm, shadows, ema_decay=None):
    """one call of fcmf_multi_adamw, or with ema_decay of fcmf_multi_adamw_ema, on the layout"""
    from fcmf_framework import _hip as H
    lr = (ctypes.c_float * 8)(*(list(LR) + [0.0] * 6))
    wd = (ctypes.c_float * 8)(*(list(WD) + [0.0] * 6))
    tabs = [L.table(L.p), L.table(L.g), L.table(L.m), L.table(L.v)]
    sh = L.table(L.sh, NO_SHADOW) if shadows else None
    args = [H.ptr(t) for t in tabs] + [H.ptr(sh), H.ptr(L.sizes), H.ptr(L.group), H.ptr(L.ct), H.ptr(L.co), L.nchunks, CHUNK, lr, wd, 2,
                                       0.9, 0.999, 1e-8, step, H.ptr(L.sumsq), -1.0 if max_norm is None else max_norm, H.stream()]
    if ema_decay is None:
        rc = H.lib().fcmf_multi_adamw(*args)
    else:
        e = L.table(L.e)
        rc = H.lib().fcmf_multi_adamw_ema(*args, H.ptr(e), ema_decay)
    assert rc == 0
    L.check()


# ---- kernel level --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shadows", [False, True])
@pytest.mark.parametrize("max_norm", [None, 1.0])
def test_adamw_half_is_unchanged(dev, max_norm, shadows):
    """p, m, v and the bf16 shadows after fcmf_multi_adamw_ema are those after fcmf_multi_adamw, on the same inputs"""
    plain, ema = Layout(dev), Layout(dev)
    for step in (1, 2):
        for L in (plain, ema):
            L.set_grads(1000 * step)
        _adamw(plain, step, max_norm, shadows)
        _adamw(ema, step, max_norm, shadows, ema_decay=0.999)
        for kind in ("p", "m", "v", "sh"):
            for i, (a, b) in enumerate(zip(plain.read(kind), ema.read(kind))):
                assert _same(a, b), (kind, i, step)
        for i, s in enumerate(ema.sh):
            if not shadows or i in NO_SHADOW:
                assert s.untouched(), i                                  # no pointer, nothing written
            else:
                assert _same(s.t, ema.p[i].t.bfloat16()), i
        assert all(not _same(e0, e1) for e0, e1 in zip(plain.read("e"), ema.read("e")))      # (the plain call leaves e alone)


@pytest.mark.parametrize("d", [0.0, 0.5, 0.999, 2.0 / 11.0])
def test_ema_is_the_stated_float32_formula(dev, d):
    """e = d * e + (1 - d) * p_new with every product and the sum rounded on its own, three consecutive steps"""
    L = Layout(dev, seed=7)
    e_prev = [e.numpy() for e in L.read("e")]
    for step in (1, 2, 3):
        L.set_grads(2000 * step)
        _adamw(L, step, 1.0, True, ema_decay=d)
        p_new = [p.numpy() for p in L.read("p")]
        got = [e.numpy() for e in L.read("e")]
        for i in range(len(SIZES)):
            want = np.float32(d) * e_prev[i] + (np.float32(1) - np.float32(d)) * p_new[i]
            assert want.dtype == np.float32 and np.array_equal(got[i].view(np.int32), want.view(np.int32)), (i, step)
            if d == 0.0:
                assert np.array_equal(got[i].view(np.int32), p_new[i].view(np.int32)), (i, step)
        e_prev = got


OFFSETS = {"aligned": {}, "ema-off-by-one": {"e": 1}, "all-off-by-one": {"p": 1, "g": 1, "m": 1, "v": 1, "e": 1, "sh": 2}}


def test_adamw_ema_does_not_depend_on_alignment(dev):
    """every tensor 16-byte aligned; only the EMA tensors one float off (the vector body must be declined); everything one float
    off: the same bits"""
    runs = {}
    for name, off in OFFSETS.items():
        L = Layout(dev, off, seed=3)
        want = {k: 4 * off.get(k, 0) for k in "pgmve"}
        assert all(getattr(L, k)[i].t.data_ptr() % 16 == want[k] for k in "pgmve" for i in range(len(SIZES)))
        for step in (1, 2):
            L.set_grads(3000 * step)
            _adamw(L, step, 1.0, True, ema_decay=0.999)
        runs[name] = {k: L.read(k) for k in ("p", "m", "v", "e", "sh")}
    for name in ("ema-off-by-one", "all-off-by-one"):
        for k, tensors in runs[name].items():
            for i, (a, b) in enumerate(zip(runs["aligned"][k], tensors)):
                assert _same(a, b), (name, k, i)


def _swap(L, a, b, shadows):
    from fcmf_framework import _hip as H
    ta, tb = L.table(a), L.table(b)
    sh = L.table(L.sh, NO_SHADOW) if shadows else None
    assert H.lib().fcmf_multi_swap(H.ptr(ta), H.ptr(tb), H.ptr(sh), H.ptr(L.sizes), H.ptr(L.ct), H.ptr(L.co), L.nchunks, CHUNK,
                                   H.stream()) == 0
    L.check()


@pytest.mark.parametrize("name", list(OFFSETS))
def test_swap_exchanges_and_restores(dev, name):
    L = Layout(dev, OFFSETS[name], seed=5)
    a0, b0 = L.read("p"), L.read("e")
    _swap(L, L.p, L.e, True)
    for i, (a, b) in enumerate(zip(L.read("p"), L.read("e"))):
        assert _same(a, b0[i]) and _same(b, a0[i]), i
        if i in NO_SHADOW:
            assert L.sh[i].untouched(), i
        else:
            assert _same(L.sh[i].t.cpu(), b0[i].bfloat16()), i           # the bf16 copy of what a NOW holds
    _swap(L, L.p, L.e, True)
    for i, (a, b) in enumerate(zip(L.read("p"), L.read("e"))):
        assert _same(a, a0[i]) and _same(b, b0[i]), i
        if i not in NO_SHADOW:
            assert _same(L.sh[i].t.cpu(), a0[i].bfloat16()), i
    for s in L.sh:
        s.buf.fill_(SENT[torch.bfloat16])
    _swap(L, L.p, L.e, False)                                            # no shadow table at all
    assert all(s.untouched() for s in L.sh)
    assert all(_same(a, b0[i]) for i, a in enumerate(L.read("p")))


def test_swap_of_a_tensor_with_itself_changes_nothing(dev):
    L = Layout(dev, seed=6)
    a0 = L.read("p")
    _swap(L, L.p, L.p, True)
    for i, a in enumerate(L.read("p")):
        assert _same(a, a0[i]), i
        if i not in NO_SHADOW:
            assert _same(L.sh[i].t.cpu(), a0[i].bfloat16()), i


# ---- optimizer and cache level -------------------------------------------------------------------------------------------------
class Tiny(torch.nn.Module):
    """three `ops.linear` layers; the last weight has 70 rows: its bf16 shadow is the head of a zero-padded 96-row buffer"""

    def __init__(self, dev, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        mk = lambda *s: torch.nn.Parameter((torch.randn(*s, generator=g) * 0.2).to(dev))
        self.w1, self.b1, self.w2, self.b2, self.w3, self.b3 = mk(64, 32), mk(64), mk(64, 64), mk(64), mk(70, 64), mk(70)

    def forward(self, x):
        from fcmf_framework import ops
        return ops.linear(ops.linear(ops.linear(x, self.w1, self.b1), self.w2, self.b2), self.w3, self.b3)


def _data(dev, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(8, 32, generator=g).to(dev).bfloat16(), torch.randn(8, 70, generator=g).to(dev)


def _optimizer(model, ema=None, warmup=True):
    from fcmf_framework.optimization import FusedAdamW
    opt = FusedAdamW([dict(params=[model.w1, model.w2, model.w3], weight_decay=0.01), dict(params=[model.b1, model.b2, model.b3],
                                                                                             weight_decay=0.0)], lr=1e-2)
    if ema is not None:
        opt.set_ema(ema, warmup=warmup)
    return opt


def _train_step(model, opt, dev, seed):
    """forward, backward through the dX GEMMs (x needs its gradient: they read the transposed shadows), optimizer step -> dx"""
    x, tgt = _data(dev, seed)
    x.requires_grad_(True)
    (model(x).float() * tgt).sum().backward()
    opt.step(max_grad_norm=1.0)
    opt.zero_grad(set_to_none=True)
    return x.grad.detach().clone()


@torch.no_grad()
def _output(model, dev):
    return model(_data(dev, 99)[0]).clone()


def _state(model, opt):
    return {k: [fn(p) for p in model.parameters()] for k, fn in
            (("p", lambda p: p.detach().clone()), ("m", lambda p: opt.state[p]["exp_avg"].clone()),
             ("v", lambda p: opt.state[p]["exp_avg_sq"].clone()), ("ema", lambda p: opt.state[p]["ema"].clone() if "ema" in opt.state[p] else None))}


def _assert_state_equal(a, b, keys=("p", "m", "v", "ema")):
    for k in keys:
        for i, (x, y) in enumerate(zip(a[k], b[k])):
            assert _same(x, y), (k, i)


@pytest.fixture
def bf16():
    from fcmf_framework import ops
    ops.shadows.clear()
    ops.set_compute_dtype(torch.bfloat16)
    yield ops
    ops.set_compute_dtype(torch.float32)
    ops.shadows.clear()


def test_ema_leaves_the_trajectory_alone_and_follows_the_recurrence(dev, bf16):
    from fcmf_framework.optimization import ema_decay_at
    a, b = Tiny(dev), Tiny(dev)
    oa, ob = _optimizer(a, 0.9), _optimizer(b)
    e = [p.detach().cpu().numpy().copy() for p in a.parameters()]       # initialised to the parameter before the first averaged step
    for t in (1, 2, 3):
        _train_step(a, oa, dev, t)
        _train_step(b, ob, dev, t)
        d = np.float32(ema_decay_at(0.9, t, True))
        for i, p in enumerate(a.parameters()):
            st = oa.state[p]["ema"]
            assert st.dtype == torch.float32 and st.shape == p.shape and st.is_contiguous() and st.data_ptr() != p.data_ptr()
            e[i] = d * e[i] + (np.float32(1) - d) * p.detach().cpu().numpy()
            assert np.array_equal(st.cpu().numpy().view(np.int32), e[i].view(np.int32)), (t, i)
    _assert_state_equal(_state(a, oa), _state(b, ob), keys=("p", "m", "v"))
    assert all("ema" not in ob.state[p] for p in b.parameters())
    assert ema_decay_at(0.9, 1, True) == 2.0 / 11.0


def test_ema_weights_keeps_the_shadow_cache_consistent(dev, bf16):
    ops = bf16
    a, c = Tiny(dev), Tiny(dev)                  # c: the twin that never enters the block
    oa, oc = _optimizer(a, 0.9), _optimizer(c, 0.9)
    for t in (1, 2, 3):
        _train_step(a, oa, dev, t)
        _train_step(c, oc, dev, t)
    _assert_state_equal(_state(a, oa), _state(c, oc))
    pre = _output(a, dev)
    raw, ema = [p.detach().clone() for p in a.parameters()], [oa.state[p]["ema"].clone() for p in a.parameters()]
    assert ops.shadows.peek(a.w3) is not None and ops.shadows.padded(a.w3).shape == (96, 64)        # the padded shadow path
    with oa.ema_weights() as inside_opt:
        assert inside_opt is oa
        for p, r, e in zip(a.parameters(), raw, ema):
            assert _same(p, e) and _same(oa.state[p]["ema"], r)
        inside = _output(a, dev)
        assert not bool(ops.shadows.padded(a.w3)[70:].any())             # the zero rows behind the ragged weight's copy survive
    after = _output(a, dev)
    assert _same(after, pre) and not _same(inside, pre)
    for p, r, e in zip(a.parameters(), raw, ema):
        assert _same(p, r) and _same(oa.state[p]["ema"], e)
    # the stale-shadow check: a whole training step after the block against the twin's
    dxa, dxc = _train_step(a, oa, dev, 4), _train_step(c, oc, dev, 4)
    assert _same(dxa, dxc)
    _assert_state_equal(_state(a, oa), _state(c, oc))
    # the averaged model, built with plain copies and an emptied cache
    b = Tiny(dev, seed=1)
    with torch.no_grad():
        for p, e in zip(b.parameters(), ema):
            p.copy_(e)
    ops.shadows.clear()
    assert _same(_output(b, dev), inside)


def test_ema_weights_is_two_swap_launches(dev, bf16):
    a = Tiny(dev)
    oa = _optimizer(a, 0.9)
    for t in (1, 2):
        _train_step(a, oa, dev, t)

    def block():
        with oa.ema_weights():
            pass
    names = [c[0] for c in _recorded(block)]
    assert names == ["fcmf_multi_swap", "fcmf_multi_swap", "fcmf_multi_cast_transpose"], names
    names = [c[0] for c in _recorded(lambda: _train_step(a, oa, dev, 3))]
    assert "fcmf_multi_adamw_ema" in names and "fcmf_multi_adamw" not in names
    # parameters without an average are left alone: a frozen one that never stepped
    frozen = torch.nn.Parameter(torch.ones(5, device=dev))
    oa.add_param_group(dict(params=[frozen]))
    with oa.ema_weights():
        assert bool((frozen == 1).all()) and "ema" not in oa.state.get(frozen, {})


def test_refusals_inside_the_block(dev, bf16):
    a = Tiny(dev)
    oa = _optimizer(a, 0.9)
    _train_step(a, oa, dev, 1)
    before = _state(a, oa)
    with oa.ema_weights():
        with pytest.raises(RuntimeError, match="nest"):
            with oa.ema_weights():
                pass
        x, tgt = _data(dev, 2)
        (a(x).float() * tgt).sum().backward()
        with pytest.raises(RuntimeError, match="step"):
            oa.step(max_grad_norm=1.0)
        with pytest.raises(RuntimeError, match="set_ema"):
            oa.set_ema(0.5)
        with pytest.raises(RuntimeError, match="set_ema"):
            oa.set_ema(None)
    oa.zero_grad(set_to_none=True)
    _assert_state_equal(_state(a, oa), before)                           # the refusals left the block's exit intact
    with oa.ema_weights():                                               # and the block can be entered again
        pass
    _assert_state_equal(_state(a, oa), before)


def test_checkpoint_round_trip(dev, bf16):
    u = Tiny(dev)
    ou = _optimizer(u, 0.9)
    for t in (1, 2, 3):
        _train_step(u, ou, dev, t)
    v = Tiny(dev)
    ov = _optimizer(v, 0.9)
    for t in (1, 2):
        _train_step(v, ov, dev, t)
    sd, weights = copy.deepcopy(ov.state_dict()), copy.deepcopy(v.state_dict())
    assert all(set(s) == {"step", "exp_avg", "exp_avg_sq", "ema"} for s in sd["state"].values()) and len(sd["state"]) == 6
    w = Tiny(dev, seed=1)
    w.load_state_dict(weights)
    ow = _optimizer(w, 0.9)
    ow.load_state_dict(copy.deepcopy(sd))
    _train_step(w, ow, dev, 3)
    _assert_state_equal(_state(w, ow), _state(u, ou))
    # a state without 'ema' (the reference's AdamW checkpoint, a run that had the average off): the average starts at the parameters
    bare = copy.deepcopy(sd)
    for s in bare["state"].values():
        del s["ema"]
    x = Tiny(dev, seed=1)
    x.load_state_dict(weights)
    ox = _optimizer(x, 0.9)
    ox.load_state_dict(bare)
    for p in x.parameters():
        assert _same(ox.state[p]["ema"], p) and ox.state[p]["ema"].data_ptr() != p.data_ptr()
    # a state with 'ema' while the average is off: dropped, and step() calls the plain entry point
    y = Tiny(dev, seed=1)
    y.load_state_dict(weights)
    oy = _optimizer(y)
    oy.load_state_dict(copy.deepcopy(sd))
    assert all("ema" not in oy.state[p] for p in y.parameters())
    names = [c[0] for c in _recorded(lambda: _train_step(y, oy, dev, 3))]
    assert "fcmf_multi_adamw" in names and "fcmf_multi_adamw_ema" not in names and "fcmf_multi_swap" not in names
    _assert_state_equal(_state(y, oy), _state(u, ou), keys=("p", "m", "v"))
    # turning the average off drops the state
    ou.set_ema(None)
    assert all("ema" not in ou.state[p] for p in u.parameters())


# ---- driver level --------------------------------------------------------------------------------------------------------------
FT = ["--do_train", "--do_eval", "--num_imgs", "2", "--num_rois", "5", "--train_batch_size", "4", "--eval_batch_size", "4",
      "--gradient_accumulation_steps", "2", "--synthetic_steps", "6", "--max_seq_length", "16", "--seed", "3", "--bf16"]


def _optimizer_order_names(hf):
    """the parameter names in the order of the fine-tune driver's optimizer (the index of `optimizer_state_dict['state']`)"""
    import run_multimodal_fcmf as drv
    from fcmf_framework.fcmf_multimodal import FCMF
    model = FCMF(pretrained_path=hf, num_labels=4, num_imgs=2, num_roi=5)
    args = drv.build_parser().parse_args(["--output_dir", "o", "--pretrained_hf_model", hf])
    name_of = {id(p): n for n, p in model.named_parameters()}
    return [name_of[id(p)] for g in drv.param_groups(model, args) for p in g["params"]]


def test_finetune_driver_with_ema(tmp_path, dev):
    import run_multimodal_fcmf as drv
    from fcmf_framework import ops
    hf = make_hf_dir(synth.TINY_CFG)
    out = str(tmp_path / "ema")
    load = lambda tag: torch.load(os.path.join(out, f"seed_3_fcmf_model_{tag}.pth"), map_location="cpu", weights_only=True)
    try:
        drv.main(["--output_dir", out, "--pretrained_hf_model", hf, "--num_train_epochs", "1", "--ema_decay", "0.5", "--ema_no_warmup"] + FT)
        log = open(os.path.join(out, "training_fcmf.log")).read()
        assert "weight EMA: decay 0.5, no warmup" in log and "Dev macro-F1 per aspect" in log
        last = load("last")
        names = _optimizer_order_names(hf)
        state, raw = last["optimizer_state_dict"]["state"], last["model_state_dict"]
        assert len(state) > 20 and all("ema" in s and s["step"] == 3 for s in state.values())
        differ = [i for i, s in state.items() if not torch.equal(s["ema"], raw[names[i]])]
        assert len(differ) > len(state) // 2                              # the model side is not the average ...
        print("MEASURED best checkpoint written:", os.path.exists(os.path.join(out, "seed_3_fcmf_model_best.pth")), "best_score", last["best_score"])
        if os.path.exists(os.path.join(out, "seed_3_fcmf_model_best.pth")):
            best = load("best")
            for i, s in state.items():
                assert _same(best["model_state_dict"][names[i]], s["ema"]), names[i]      # best: the averaged weights of the same epoch
                # ... it is the raw weights: what the average's slot held while the parameters held the average
                assert _same(best["optimizer_state_dict"]["state"][i]["ema"], raw[names[i]]), names[i]
            assert any(not torch.equal(best["model_state_dict"][names[i]], raw[names[i]]) for i in state)
        res = open(os.path.join(out, "test_results_fcmf.txt")).read().splitlines()
        assert res[0] == "***** Test results *****" and res[-1].startswith("Average F1: ") and len(res) == 8
        fm = open(os.path.join(out, "test_predictions_formatted.txt"), encoding="utf-8").read()
        assert fm.startswith("TEST DETAILED PREDICTIONS\nAverage Macro F1: ") and "Sentence 0: synthetic review" in fm
        # resume continues both trajectories
        drv.main(["--output_dir", out, "--pretrained_hf_model", hf, "--num_train_epochs", "2", "--ema_decay", "0.5", "--ema_no_warmup",
                  "--resume_from_checkpoint", os.path.join(out, "seed_3_fcmf_model_last.pth")] + FT)
        again = load("last")
        assert again["epoch"] == 1
        assert all("ema" in s and s["step"] == 6 for s in again["optimizer_state_dict"]["state"].values())
        assert any(not torch.equal(again["optimizer_state_dict"]["state"][i]["ema"], s["ema"]) for i, s in state.items())
    finally:
        ops.set_compute_dtype(torch.float32)


def test_finetune_driver_without_the_flag_writes_no_ema(tmp_path, dev):
    import run_multimodal_fcmf as drv
    from fcmf_framework import ops
    hf = make_hf_dir(synth.TINY_CFG)
    out = str(tmp_path / "plain")
    try:
        drv.main(["--output_dir", out, "--pretrained_hf_model", hf, "--num_train_epochs", "1"] + FT)
    finally:
        ops.set_compute_dtype(torch.float32)
    ck = torch.load(os.path.join(out, "seed_3_fcmf_model_last.pth"), map_location="cpu", weights_only=True)
    state = ck["optimizer_state_dict"]["state"]
    assert len(state) > 20 and all(set(s) == {"step", "exp_avg", "exp_avg_sq"} for s in state.values())
    assert "weight EMA" not in open(os.path.join(out, "training_fcmf.log")).read()


def test_pretraining_driver_with_ema(tmp_path, dev, monkeypatch):
    """`*_last.pth`: the average in every stepped parameter's state -- equal to the host recurrence over the raw weights seen
    after every optimizer step -- and the raw weights, not the averaged ones, as the model"""
    import run_pretraining_fcmf as drv
    from fcmf_framework import ops
    from fcmf_framework.optimization import FusedAdamW, ema_decay_at
    seen = []

    class Spy(FusedAdamW):
        def step(self, *a, **kw):
            params = [p for g in self.param_groups for p in g["params"]]
            if not seen:
                seen.append([p.detach().cpu().clone() for p in params])
            r = super().step(*a, **kw)
            seen.append([p.detach().cpu().clone() for p in params])
            return r
    monkeypatch.setattr(drv, "FusedAdamW", Spy)
    hf = make_hf_dir(synth.TINY_CFG)
    out = str(tmp_path / "pt")
    try:
        drv.main(["--output_dir", out, "--pretrained_hf_model", hf, "--do_train", "--num_imgs", "2", "--num_rois", "5",
                  "--train_batch_size", "3", "--synthetic_steps", "3", "--synthetic_dec_len", "6", "--num_train_epochs", "1",
                  "--seed", "5", "--ema_decay", "0.5"])
    finally:
        ops.set_compute_dtype(torch.float32)
    assert len(seen) == 4
    ck = torch.load(os.path.join(out, "seed_5_iaog_model_last.pth"), map_location="cpu", weights_only=True)
    state, sd = ck["optimizer_state_dict"]["state"], ck["model_state_dict"]
    assert 20 < len(state) <= len(seen[0]) and all("ema" in s for s in state.values())
    assert "weight EMA: decay 0.5, warmup" in open(os.path.join(out, "pretraining_iaog.log")).read()
    averaged_differs = 0
    for i, s in state.items():
        e = seen[0][i].numpy()
        for t in (1, 2, 3):
            d = np.float32(ema_decay_at(0.5, t, True))
            e = d * e + (np.float32(1) - d) * seen[t][i].numpy()
        assert np.array_equal(s["ema"].numpy().view(np.int32), e.view(np.int32)), i
        final = seen[3][i]
        assert any(v.shape == final.shape and torch.equal(v, final) for v in sd.values()), i      # the model side: the raw weights
        averaged_differs += not torch.equal(s["ema"], final)
    assert averaged_differs > len(state) // 2


def test_folded_trunk_snapshot_follows_the_swap(dev):
    """resnet_eval.FoldedTrunk keeps its folded weights outside the shadow cache: it takes a new snapshot when the parameters were
    exchanged since its last one -- inside the block it is the averaged trunk, after it the raw one again"""
    from fcmf_framework import ops
    from fcmf_framework.optimization import FusedAdamW
    from fcmf_framework.resnet import ResNet
    from fcmf_framework.resnet_eval import FoldedTrunk
    ops.set_compute_dtype(torch.float32)
    ops.shadows.clear()
    layers = synth.RESNET_TINY_LAYERS
    P = synth.synth_resnet_params(synth.resnet_param_shapes(layers), 0)

    def build():
        m = ResNet(layers)
        m.load_state_dict(P, strict=False)
        return m.to(dev).eval()
    m = build()
    params = [p for n, p in m.named_parameters() if not n.startswith("fc.")]
    opt = FusedAdamW(params, lr=1e-2)
    opt.set_ema(0.5, warmup=False)
    g = torch.Generator().manual_seed(0)
    for p in params:
        p.grad = torch.randn(p.shape, generator=g).to(dev)
    opt.step()
    x = synth.synth_crops(2, 64, seed=1).to(dev)
    f = FoldedTrunk(m)
    raw = f(x).clone()
    with opt.ema_weights():
        inside = f(x).clone()
    assert torch.equal(f(x), raw) and not torch.equal(inside, raw)
    twin = build()
    with torch.no_grad():
        for q, p in zip([q for n, q in twin.named_parameters() if not n.startswith("fc.")], params):
            q.copy_(opt.state[p]["ema"])
    assert torch.equal(FoldedTrunk(twin)(x), inside)
    ops.shadows.clear()
