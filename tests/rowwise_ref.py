"""Float64 references for the row-wise, elementwise and optimizer kernels (csrc/norm.hip, csrc/misc.hip), the counter-based
dropout mask restated in numpy from the comment block of csrc/common.h, and guard-band buffers.  Plain module: no fixtures,
and nothing here calls the library -- this is the specification the kernels are held to."""
import math

import numpy as np
import torch

_M32 = np.uint64(0xFFFFFFFF)

# seeds of the GPU tests: a small one (it only permutes pairs through the XOR with the index) and one with a non-zero high word,
# as ops.next_seed() produces (the high word enters between the two multiply rounds)
SEED_LO, SEED_HI = 77, (5 << 32) | 17
EMBED_SEED = 0xC3174AA04A73B056          # what ops.next_seed() draws first after ops.manual_seed(2024)
# every (seed, n, p) a GPU test takes a mask for (test_dropout_mask_cpu.py checks the keep fraction of each)
MASK_CASES = ([(s, n, p) for s in (SEED_LO, SEED_HI) for n in (8197 * 64, 37 * 260) for p in (0.1, 0.25)] +
              [(s, n, p) for s in (SEED_LO, SEED_HI) for n in (1, 255, 257, 1048576 + 7) for p in (0.1, 0.5)] +
              [(EMBED_SEED, 15 * H, 0.1) for H in (260, 2048)] + [(99, 1000, 0.3), (123, 531476, 0.3)])


# ---- dropout mask ---------------------------------------------------------------------------------------------------------
def dropout_threshold(p):
    """uint32(p * 65536 + 0.5), evaluated in float32 as the kernels do"""
    return int(np.float32(p) * np.float32(65536.0) + np.float32(0.5))


def _hash32(seed, pair):
    """lowbias32 over (seed, pair): x = lo ^ seed_lo ^ rotl(hi, 7); two multiply rounds with seed_hi XORed in between"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    s0, s1 = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    pair = np.asarray(pair, dtype=np.uint64)
    lo, hi = pair & _M32, pair >> np.uint64(32)
    x = lo ^ s0 ^ (((hi << np.uint64(7)) | (hi >> np.uint64(25))) & _M32)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & _M32
    x ^= s1
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & _M32
    x ^= x >> np.uint64(16)
    return x


def dropout_mask(seed, start, n, p):
    """bool [n]: element `start + i` is KEPT.  One hash decides the pair idx >> 1: its low 16 bits the even element, its high
    16 bits the odd one; kept iff those bits >= the threshold."""
    idx = np.uint64(start) + np.arange(n, dtype=np.uint64)
    h = _hash32(seed, idx >> np.uint64(1))
    bits = np.where((idx & np.uint64(1)) == 1, h >> np.uint64(16), h & np.uint64(0xFFFF))
    return bits >= np.uint64(dropout_threshold(p))


def mask_tensor(seed, shape, p, start=0):
    """the mask as a float64 0/1 tensor of `shape` (row-major element index, the convention of every kernel)"""
    n = int(np.prod(shape))
    return torch.from_numpy(dropout_mask(seed, start, n, p).astype(np.float64)).reshape(shape)


def inv_keep(p):
    """float32(1 / (1 - p)) as the kernels form it, as a python float"""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p))) if p > 0 else 1.0


# ---- LayerNorm (TF style: biased variance, eps inside the sqrt) -------------------------------------------------------------
def ln_stats(z, eps):
    z = z.double()
    mean = z.mean(-1)
    var = (z - mean[:, None]).pow(2).mean(-1)
    return mean, 1.0 / torch.sqrt(var + eps)


def ln_fwd(z, gamma, beta, eps):
    """-> y, mean, rstd (float64)"""
    z = z.double()
    mean, rstd = ln_stats(z, eps)
    return (z - mean[:, None]) * rstd[:, None] * gamma.double() + beta.double(), mean, rstd


def ln_bwd(dy, z, gamma, mean, rstd):
    """explicit backward from the statistics the kernel is handed -> dz, the per-row terms of dgamma, those of dbeta"""
    dy, z, gamma = dy.double(), z.double(), gamma.double()
    mean, rstd = mean.double()[:, None], rstd.double()[:, None]
    xh = (z - mean) * rstd
    g = dy * gamma
    s1 = g.mean(-1, keepdim=True)
    s2 = (g * xh).mean(-1, keepdim=True)
    return rstd * (g - s1 - xh * s2), dy * xh, dy


# ---- activations ------------------------------------------------------------------------------------------------------------
def gelu_grad(x):
    x = x.double()
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def tanh_grad_from_output(a):
    a = a.double()
    return 1.0 - a * a


# ---- AdamW with the global-norm clip ----------------------------------------------------------------------------------------
def clip_coef(norm, max_norm):
    return 1.0 if max_norm is None or max_norm <= 0 else min(1.0, max_norm / (norm + 1e-6))


def global_norm(grads):
    return math.sqrt(sum(float(g.double().pow(2).sum()) for g in grads))


def adamw_step(p, g, m, v, step, lr, wd, coef=1.0, betas=(0.9, 0.999), eps=1e-8):
    """one decoupled-weight-decay Adam step on float64 tensors, in place"""
    b1, b2 = betas
    g = g.double() * coef
    p.mul_(1.0 - lr * wd)
    m.mul_(b1).add_(g, alpha=1.0 - b1)
    v.mul_(b2).addcmul_(g, g, value=1.0 - b2)
    denom = v.sqrt() / math.sqrt(1.0 - b2 ** step) + eps
    p.addcdiv_(m, denom, value=-lr / (1.0 - b1 ** step))


# ---- decoder head gather ----------------------------------------------------------------------------------------------------
def head_gather(slot, G, T, heads, d):
    """out[g, t, h] = sum over the slots s with (s * G + g) % heads == h of slot[g, t, s]; float64 [G, T, heads, d]"""
    slot = slot.double().reshape(G, T, heads, d)
    out = torch.zeros(G, T, heads, d, dtype=torch.float64)
    for g in range(G):
        for s in range(heads):
            out[g, :, (s * G + g) % heads] += slot[g, :, s]
    return out


# ---- guard bands ------------------------------------------------------------------------------------------------------------
_SENTINEL = {torch.float32: 12345.0, torch.bfloat16: 12352.0, torch.int64: -7777, torch.float64: 12345.0}


class Guarded:
    """`view`: a 16-byte-aligned interior of a larger sentinel-filled buffer; `check()` asserts the frame is untouched"""

    def __init__(self, shape, dtype, dev, pad=64):
        es = torch.empty((), dtype=dtype).element_size()
        pad = (pad * es + 15) // 16 * 16 // es           # the frame is a whole number of 16-byte units: the interior stays aligned
        self.n, self.pad = int(np.prod(shape)), pad
        self.buf = torch.full((self.n + 2 * pad,), _SENTINEL[dtype], dtype=dtype, device=dev)
        self.view = self.buf[pad:pad + self.n].view(shape)
        assert self.view.data_ptr() % 16 == 0

    def check(self):
        s = _SENTINEL[self.buf.dtype]
        assert bool((self.buf[:self.pad] == s).all()), "write before the start of an output"
        assert bool((self.buf[self.pad + self.n:] == s).all()), "write past the end of an output"


def guarded(shape, dtype, dev, pad=64):
    return Guarded(shape, dtype, dev, pad)


def check_all(*gs):
    for g in gs:
        if g is not None:
            g.check()
