"""The attention descriptor and the MFMA / VALU choice, without a GPU: fcmf_framework.attn.desc only reads shapes, strides and
addresses, so it runs on CPU tensors.
DESC / PTRS: every field of the descriptor for one case of each call site.  tools/make_attn_path_literals.py printed them at the
commit before fcmf_framework/attn.py existed, from ops._desc and (the fused cases) fused._qkv_desc, which gave the same.
All operands of a case are views of ONE buffer, so an address is recorded as its byte offset from the lowest operand address.
CHOICE: written out by hand from that commit's expressions in ops.AttentionFn.forward, ops.attention_probs and fused._use_mfma."""
import pytest
import torch

from fcmf_framework import attn, fused, ops
from helpers import desc_fields


class _Pool:
    """operands as views of one zeroed byte buffer, 64-byte aligned, in the order they are asked for"""

    def __init__(self):
        self.buf, self.used = torch.zeros(1 << 20, dtype=torch.uint8), 0

    def __call__(self, *shape, dtype=torch.float32):
        n = torch.Size(shape).numel() * torch.empty((), dtype=dtype).element_size()
        t = self.buf[self.used:self.used + n].view(dtype).view(shape)
        self.used += (n + 63) // 64 * 64
        return t


def _case(name):
    """-> the 14 arguments of attn.desc"""
    new = _Pool()
    if name == "k1-mask":
        q, k, v = new(2, 5, 32), new(2, 7, 32), new(2, 7, 32)
        return q, k, v, None, None, new(2, 7), None, 2, 1, 0.25, 0.1, 123, False, 0
    if name == "k1-k2-bias-group-div-2":
        q, k1, v1, k2, v2 = new(4, 3, 32), new(4, 6, 32), new(4, 6, 32), new(2, 3, 4, 32), new(2, 3, 4, 32)
        return q, k1, v1, k2, v2, new(4, 10), new(2, 2, 3, 10), 2, 2, 0.25, 0.0, 0, False, 0
    if name == "k2-only-expanded-q":
        q = new(4, 32).unsqueeze(1).expand(4, 3, 32)
        return q, None, None, new(4, 3, 9, 32), new(4, 3, 9, 32), None, None, 2, 1, 0.25, 0.0, 0, False, 0
    if name == "row-strided-q":
        q, k, v = new(2, 5, 40)[:, :, :32], new(2, 7, 32), new(2, 7, 32)
        return q, k, v, None, None, None, None, 2, 1, 0.25, 0.0, 0, True, 0
    if name in ("iaog-quirk-1", "iaog-quirk-0"):
        kq3 = new(3, 8, 512)
        q, k = kq3[:, :, 256:], kq3[:, :, :256]
        return q, k, k, None, None, None, None, 4, 1, 0.125, 0.0, 0, True, int(name[-1])
    if name == "chunk-44-keys":
        q, k, v = new(2, 5, 128), new(2, 300, 128), new(2, 300, 128)
        return q, k[:, 256:300], v[:, 256:300], None, None, new(2, 44), None, 2, 1, 0.125, 0.1, 2 ** 64 - 1, False, 0
    raise KeyError(name)


def _fused_case(dtype):
    """-> the arguments of fused's descriptor: the [G*T, 3H] q|k|v buffer of G = 2, T = 5, H = 128, heads = 2"""
    new = _Pool()
    return new(10, 384, dtype=dtype), new(2, 5), 2, 5, 128, 2, 0.1, 77


CASES = ["k1-mask", "k1-k2-bias-group-div-2", "k2-only-expanded-q", "row-strided-q", "iaog-quirk-1", "iaog-quirk-0", "chunk-44-keys"]
FUSED_CASES = {"fused-f32": torch.float32, "fused-bf16": torch.bfloat16}


def fields(a):
    """-> (every non-pointer field in declaration order, every pointer field as None or its offset from the lowest of them)"""
    plain, ptrs = desc_fields(a)
    addr = [getattr(a, n) for n in ptrs]
    low = min(x for x in addr if x is not None)
    return tuple(getattr(a, n) for n in plain), tuple(None if x is None else x - low for x in addr)


# dtype G heads d R T1 T2 group_div | q_sg q_sr k1_sg k1_st k2_sg k2_sr k2_st o_sg o_sr | scale dropout_p seed causal head_quirk
DESC = {
    "k1-mask": (0, 2, 2, 16, 5, 7, 0, 1, 160, 32, 224, 32, 0, 0, 0, 160, 32, 0.25, 0.10000000149011612, 123, 0, 0),
    "k1-k2-bias-group-div-2": (0, 4, 2, 16, 3, 6, 4, 2, 96, 32, 192, 32, 384, 128, 32, 96, 32, 0.25, 0.0, 0, 0, 0),
    "k2-only-expanded-q": (0, 4, 2, 16, 3, 0, 9, 1, 32, 0, 0, 0, 864, 288, 32, 96, 32, 0.25, 0.0, 0, 0, 0),
    "row-strided-q": (0, 2, 2, 16, 5, 7, 0, 1, 200, 40, 224, 32, 0, 0, 0, 160, 32, 0.25, 0.0, 0, 1, 0),
    "iaog-quirk-1": (0, 3, 4, 64, 8, 8, 0, 1, 4096, 512, 4096, 512, 0, 0, 0, 2048, 256, 0.125, 0.0, 0, 1, 1),
    "iaog-quirk-0": (0, 3, 4, 64, 8, 8, 0, 1, 4096, 512, 4096, 512, 0, 0, 0, 2048, 256, 0.125, 0.0, 0, 1, 0),
    "chunk-44-keys": (0, 2, 2, 64, 5, 44, 0, 1, 640, 128, 38400, 128, 0, 0, 0, 640, 128, 0.125, 0.10000000149011612, 18446744073709551615, 0, 0),
    "fused-f32": (0, 2, 2, 64, 5, 5, 0, 1, 1920, 384, 1920, 384, 0, 0, 0, 640, 128, 0.125, 0.10000000149011612, 77, 0, 0),
    "fused-bf16": (1, 2, 2, 64, 5, 5, 0, 1, 1920, 384, 1920, 384, 0, 0, 0, 640, 128, 0.125, 0.10000000149011612, 77, 0, 0),
}
# q k1 v1 k2 v2 mask bias
PTRS = {
    "k1-mask": (0, 1280, 3072, None, None, 4864, None),
    "k1-k2-bias-group-div-2": (0, 1536, 4608, 7680, 10752, 13824, 14016),
    "k2-only-expanded-q": (0, None, None, 512, 14336, None, None),
    "row-strided-q": (0, 1600, 3392, None, None, None, None),
    "iaog-quirk-1": (1024, 0, 0, None, None, None, None),
    "iaog-quirk-0": (1024, 0, 0, None, None, None, None),
    "chunk-44-keys": (0, 136192, 443392, None, None, 619520, None),
    "fused-f32": (0, 512, 1024, None, None, 15360, None),
    "fused-bf16": (0, 256, 512, None, None, 7680, None),
}


@pytest.mark.parametrize("name", CASES)
def test_descriptor_fields(name):
    assert fields(attn.desc(*_case(name))) == (DESC[name], PTRS[name])


@pytest.mark.parametrize("name", list(FUSED_CASES))
def test_fused_descriptor_fields(name):
    """what fused builds from its buffer, and attn.desc over the buffer's three column views"""
    qkv, mask, G, T, Hd, heads, p, seed = _fused_case(FUSED_CASES[name])
    assert fields(fused._self_desc(qkv, mask, G, T, Hd, heads, p, seed)) == (DESC[name], PTRS[name])
    x = qkv.view(G, T, 3 * Hd)
    a = attn.desc(x[:, :, :Hd], x[:, :, Hd:2 * Hd], x[:, :, 2 * Hd:], None, None, mask, None, heads, 1, 1.0 / 8, p, seed, False, 0)
    assert fields(a) == (DESC[name], PTRS[name])


# ---------------------------------------------------------------------------------------------------------------------------------
# MFMA or VALU
def _dense(dtype=torch.bfloat16, R=256, T1=256, heads=2, d=64, k1=True, k2=False, bias=False, causal=False, head_quirk=False,
           q_row_stride=None):
    """-> (descriptor, (q, k1, v1)) as ops.AttentionFn.forward builds them after its stride normalisation"""
    G, HD = 2, heads * d
    if q_row_stride is None:
        q = torch.zeros((G, R, HD), dtype=dtype)
    elif q_row_stride == 0:
        q = torch.zeros((G, HD), dtype=dtype).unsqueeze(1).expand(G, R, HD)
    else:
        q = torch.zeros((G, R, q_row_stride), dtype=dtype)[:, :, :HD]
    q = ops._query_rows(q, True)
    assert q.stride(1) == (HD if q_row_stride is None else q_row_stride)
    k = torch.zeros((G, T1, HD), dtype=dtype) if k1 else None
    kp = torch.zeros((G, R, 3, HD), dtype=dtype) if k2 else None
    b = torch.zeros((G, heads, R, T1 + (3 if k2 else 0))) if bias else None
    return attn.desc(q, k, k, kp, kp, None, b, heads, 1, 0.125, 0.0, 0, causal, head_quirk), (q, k, k)


CHOICE_DENSE = [
    (dict(), True, True),                 # bf16, d = 64, R = T1 = 256
    (dict(T1=257), True, False),
    (dict(R=257), True, False),
    (dict(heads=4, d=32), True, False),
    (dict(dtype=torch.float32), True, False),
    (dict(k2=True), True, False),
    (dict(bias=True), True, False),
    (dict(causal=True), True, False),
    (dict(head_quirk=True), True, False),
    (dict(k1=False), True, False),
    (dict(q_row_stride=128 + 8), True, False),
    (dict(q_row_stride=0), True, False),
    (dict(), False, False),               # switch off
]


@pytest.mark.parametrize("kw,switch,mfma", CHOICE_DENSE, ids=[",".join(f"{k}={v}" for k, v in kw.items()) + f"|{s}" for kw, s, _ in CHOICE_DENSE])
def test_kernel_choice_dense_operands(monkeypatch, kw, switch, mfma):
    monkeypatch.setattr(attn, "USE_MFMA_ATTENTION", switch)
    assert not hasattr(ops, "USE_MFMA_ATTENTION"), "a second switch would silently switch nothing"
    a, operands = _dense(**kw)
    assert ops._mfma_dense(a, *operands) is mfma


CHOICE_FUSED = [(torch.bfloat16, 256, True, True), (torch.bfloat16, 257, True, False), (torch.float32, 256, True, False),
                (torch.bfloat16, 256, False, False)]


@pytest.mark.parametrize("dtype,T,switch,mfma", CHOICE_FUSED)
def test_kernel_choice_fused_buffer(monkeypatch, dtype, T, switch, mfma):
    """the fused q|k|v buffer: row stride 3H, never dense, and MFMA all the same"""
    monkeypatch.setattr(attn, "USE_MFMA_ATTENTION", switch)
    G, Hd, heads = 2, 128, 2
    a = fused._self_desc(torch.zeros((G * T, 3 * Hd), dtype=dtype), None, G, T, Hd, heads, 0.0, 0)
    assert a.q_sr == 3 * Hd and attn.mfma_eligible(a) is mfma
