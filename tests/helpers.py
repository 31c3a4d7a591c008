"""shared test helpers (tests may use oracle/, the product may not)"""
import contextlib
import ctypes
import hashlib
import tempfile

import pytest
import torch

import synthetic_data as synth


def make_hf_dir(cfg):
    from fcmf_framework.roberta import RobertaConfig, RobertaModel
    d = tempfile.mkdtemp(prefix="hf_")
    RobertaModel(RobertaConfig(**cfg)).save_pretrained(d)
    return d


def build_fcmf(cfg, NI, NR, device, num_labels=4, seed=0):
    """product FCMF with the deterministic synthetic weights of oracle/synth.py"""
    from fcmf_framework.fcmf_multimodal import FCMF
    model = FCMF(make_hf_dir(cfg), num_labels=num_labels, num_imgs=NI, num_roi=NR)
    P = synth.synth_params(synth.fcmf_param_shapes(cfg, num_labels), seed)
    missing, unexpected = model.load_state_dict(P, strict=True)
    return model.to(device), P


def batch_to(batch, device):
    return {k: v.to(device) for k, v in batch.items()}


def rel_err(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


def max_err(a, b):
    return (a.detach().float().cpu() - b.detach().float().cpu()).abs().max().item()


class _CallRecorder:
    """stands in for _hip._lib: every entry point of _hip.SIGNATURES appends (name, its scalar arguments, its return code) to
    `calls` and forwards the call.  Scalar = declared as anything but c_void_p / a POINTER: addresses are left out.
    desc: the record is what the C ABI receives -- a scalar declared `float` is recorded as the float32 it is converted to, and
    a fourth element holds, for every fcmf_attn_desc argument, (its non-pointer fields, which pointer fields are non-null,
    whether v1 == k1).
    nulls: the record ends with one more element, a tuple that says for every c_void_p argument whether it was NULL ("bias given or
    not", "dx wanted or not": invisible in the scalars)."""

    def __init__(self, real, signatures, desc=False, nulls=False):
        from fcmf_framework._hip import HOST_ONLY, AttnDesc
        self._AttnDesc, self._host_only = AttnDesc, HOST_ONLY
        self._real, self.calls, self._desc, self._nulls = real, [], desc, nulls
        self._ptrs = {n: [i for i, t in enumerate(sig) if t is ctypes.c_void_p] for n, sig in signatures.items()}
        self._scalars = {n: [i for i, t in enumerate(sig) if t is not ctypes.c_void_p and not issubclass(t, ctypes._Pointer)]
                         for n, sig in signatures.items()}
        self._floats = {n: {i for i, t in enumerate(sig) if t is ctypes.c_float} for n, sig in signatures.items()}

    def __getattr__(self, name):
        fn, keep = getattr(self._real, name), self._scalars.get(name)
        if keep is None or name in self._host_only:      # (a cached planning query launches nothing: not part of a pass)
            return fn
        floats, ptrs = self._floats[name], self._ptrs[name]

        def call(*args):
            rc = fn(*args)
            if self._desc:
                scalars = tuple(ctypes.c_float(args[i]).value if i in floats else args[i] for i in keep)
                rec = (name, scalars, rc, tuple(_desc_record(a) for a in args if isinstance(a, self._AttnDesc)))
            else:
                rec = (name, tuple(args[i] for i in keep), rc)
            if self._nulls:
                rec += (tuple(not args[i] for i in ptrs),)
            self.calls.append(rec)
            return rc
        return call


def desc_fields(a):
    """-> (names of the non-pointer fields, names of the pointer fields) of a ctypes descriptor, in declaration order"""
    names = [n for n, _ in a._fields_]
    ptrs = [n for n, t in a._fields_ if t is ctypes.c_void_p]
    return [n for n in names if n not in ptrs], ptrs


def _desc_record(a):
    plain, ptrs = desc_fields(a)
    return (tuple(getattr(a, n) for n in plain), tuple(getattr(a, n) is not None for n in ptrs),
            a.v1 == a.k1)


def _calls_digest(calls):
    return hashlib.sha256(repr(calls).encode()).hexdigest()


def _recorded(fn, desc=False, nulls=False):
    """fn() with the recorder in place of the library -> its calls (desc, nulls: see _CallRecorder)"""
    from fcmf_framework import _hip as H
    H.gemm_ctx(workspace=True)                   # (the first use of a stream creates its context and workspace: not part of the pass)
    real = H.lib()
    H._lib = rec = _CallRecorder(real, H.SIGNATURES, desc, nulls)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        H._lib = real
    return rec.calls


@contextlib.contextmanager
def mfma_attention(on):
    """the MFMA / VALU switch of the attention call path set to `on` inside the block (monkeypatch: raises if there is no such switch)"""
    from fcmf_framework import attn
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(attn, "USE_MFMA_ATTENTION", on)
        yield
