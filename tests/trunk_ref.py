"""Float64 references for the forward streaming kernels of the ResNet trunk (csrc/conv.hip) -- patch matrix, stem packing, grouped
BatchNorm, the two pools -- and builders of inputs on which those kernels are EXACT.  Plain module: no fixtures, and nothing here
calls the library; every reference is written from the definition of its operation (include/fcmf_hip.h), not from the kernel.

The BatchNorm builder: per (group, channel) a mean m (a multiple of 1/4, |m| <= 2) and a half-width a in {1/2, 1, 2}; half of the
group's rows hold m - a, the other half m + a, in a seeded shuffled order.  Then the group's mean is m and its biased variance a^2,
every value is a multiple of 1/4 of magnitude <= 4 and every square a multiple of 1/16 <= 16, so every float32 partial sum a kernel
may form over up to 4096 rows is an integer number of sixteenths below 2^24: exact in any order.  With eps = 0, rstd = 1 / a is a power
of two; with gamma in +-{1/2, 1, 2}, beta a multiple of 1/4 (|beta| <= 2) and a residual of eighths (|res| <= 2), scale = gamma / a,
shift = beta - m * scale and y = +-gamma + beta (+ res) are multiples of 1/16 resp. 1/8 of magnitude <= 6: exact in float32 and bf16.
A group of ONE row has variance 0; eps = 1/4 then gives rstd = 2."""
import numpy as np
import torch

from gemm_ref import _gen, poisoned          # noqa: F401  (re-exported: the GPU test takes its buffers from here)
from rowwise_ref import _SENTINEL, check_all, guarded   # noqa: F401

DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f64": torch.float64}
GRID_CAP = 16384 * 256          # grid_for() of csrc/conv.hip: at most 16384 workgroups of 256 threads, then a grid-stride loop


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def grid_values(shape, seed, step=0.125, lim=2.0):
    """float64 multiples of `step` in [-lim, lim] (seeded generator on the CPU)"""
    k = int(round(lim / step))
    return torch.randint(-k, k + 1, tuple(shape), generator=_gen(seed), dtype=torch.int16).double() * step


def bn_input(groups, rows_per_group, C, seed):
    """-> x [groups * rows_per_group, C], m [groups, C], a [groups, C] (float64): see the module docstring.  rows_per_group is
    even, or 1 (then a = 0 and x = m)."""
    g = _gen(seed)
    m = torch.randint(-8, 9, (groups, C), generator=g).double() / 4
    if rows_per_group == 1:
        return m.clone(), m, torch.zeros_like(m)
    assert rows_per_group % 2 == 0
    a = 2.0 ** torch.randint(-1, 2, (groups, C), generator=g).double()
    half = rows_per_group // 2
    base = torch.cat([torch.ones(half), -torch.ones(half)]).double()
    # channel c sees the group's shuffled sign column rotated by 7 c rows: still half of each sign, and no two neighbours alike
    idx = (torch.arange(rows_per_group)[:, None] + 7 * torch.arange(C)[None, :]) % rows_per_group
    x = torch.empty(groups, rows_per_group, C, dtype=torch.float64)
    for gi in range(groups):
        col = base[torch.randperm(rows_per_group, generator=g)]
        x[gi] = m[gi] + col[idx] * a[gi]
    return x.reshape(groups * rows_per_group, C), m, a


def bn_params(C, seed):
    """dyadic gamma (+-{1/2, 1, 2}), beta and running mean (multiples of 1/4, <= 2), running variance in {1/4, 1, 4}"""
    g = _gen(seed)
    sign = torch.randint(0, 2, (C,), generator=g).double() * 2 - 1
    gamma = sign * 2.0 ** torch.randint(-1, 2, (C,), generator=g).double()
    beta = torch.randint(-8, 9, (C,), generator=g).double() / 4
    rmean = torch.randint(-8, 9, (C,), generator=g).double() / 4
    rvar = 4.0 ** torch.randint(-1, 2, (C,), generator=g).double()
    return gamma, beta, rmean, rvar


def bn_eval_input(rows, C, seed):
    """-> x, rmean, rvar for the eval form: rvar = a^2 in {1/4, 1, 4}, rmean = m + d a with d in {-1, 0, 1}, x = m +- a as above,
    so (x - rmean) / sqrt(rvar) is an integer in -2 .. 2 and y = k gamma + beta (+ res), |y| <= 8 in eighths: exact."""
    rows_even = rows + (rows & 1)
    x, m, a = bn_input(1, rows_even, C, seed)
    d = torch.randint(-1, 2, (C,), generator=_gen(seed + 1)).double()
    return x[:rows].contiguous(), m[0] + d * a[0], a[0] * a[0]


# ---- patch matrix ---------------------------------------------------------------------------------------------------------------
def conv_out(H, k, stride, pad):
    return (H + 2 * pad - k) // stride + 1


def im2col_ref(x, kh, kw, stride, pad, Kpad):
    """x [N, H, W, C] -> [N * Ho * Wo, Kpad], column k = (r * kw + s) * C + c holds x[n, ho * stride + r - pad, wo * stride + s - pad, c],
    0 where that tap lies in the padding; the columns >= kh * kw * C are 0"""
    x = x.double()
    N, H, W, C = x.shape
    Ho, Wo = conv_out(H, kh, stride, pad), conv_out(W, kw, stride, pad)
    assert Ho > 0 and Wo > 0 and Kpad >= kh * kw * C
    xp = torch.zeros(N, H + 2 * pad, W + 2 * pad, C, dtype=torch.float64)
    xp[:, pad:pad + H, pad:pad + W] = x
    out = torch.zeros(N, Ho, Wo, Kpad, dtype=torch.float64)
    for r in range(kh):
        for s in range(kw):
            k = (r * kw + s) * C
            out[..., k:k + C] = xp[:, r:r + (Ho - 1) * stride + 1:stride, s:s + (Wo - 1) * stride + 1:stride]
    return out.reshape(N * Ho * Wo, Kpad)


# ---- stem packing ---------------------------------------------------------------------------------------------------------------
def nearest_bf16(x):
    """float64 -> the nearest bf16, ties to even, as float64: ONE rounding (torch's own double -> bf16 cast rounds to float32
    first, which moves a value that lies just beyond the midpoint of two bf16 numbers onto that midpoint and then to the even side).
    From the definition: of the three bf16 numbers around torch's answer, the one closest to x; of two equally close, the even one."""
    x = x.double()
    b = x.float().bfloat16()
    bits = b.view(torch.int16).to(torch.int64) & 0xFFFF          # sign-magnitude: +-1 on the bits is the neighbour in magnitude
    cand = torch.stack([bits - 1, bits, bits + 1])
    cand = torch.where((bits & 0x7FFF) == 0, bits.expand_as(cand), cand)          # (zero has no neighbour below in magnitude)
    vals = ((cand + 0x8000) % 0x10000 - 0x8000).to(torch.int16).view(torch.bfloat16).double()
    err = (vals - x).abs()          # exact: the candidates are within two bf16 ulps of x
    best = err == err.amin(0, keepdim=True)
    pick = (best.int() * 2 + (best & ((cand & 1) == 0)).int()).argmax(0, keepdim=True)          # equal errors: the even candidate wins
    return vals.gather(0, pick)[0]


def pack_rgb0_ref(x, pad, Wp):
    """x [N, H, W, 3] (any dtype) -> (interior mask, values), both [N, H + 2 pad, Wp, 4]: the mask is True on the four channels of
    every interior pixel (rows pad .. pad + H, columns pad .. pad + W); there the values are x rounded ONCE to the nearest bf16 (a
    float64 source does not pass through float32: include/fcmf_hip.h) and 0 in channel 3.  Outside the mask nothing is written."""
    N, H, W, _ = x.shape
    assert Wp >= W + 2 * pad
    mask = torch.zeros(N, H + 2 * pad, Wp, 4, dtype=torch.bool)
    mask[:, pad:pad + H, pad:pad + W] = True
    vals = torch.zeros(N, H + 2 * pad, Wp, 4, dtype=torch.float64)
    vals[:, pad:pad + H, pad:pad + W, :3] = nearest_bf16(x)
    return mask, vals


# ---- grouped BatchNorm ----------------------------------------------------------------------------------------------------------
def bn_totals_ref(x, groups):
    """x [groups * rows_per_group, C] -> [groups, C, 2]: per (group, channel) sum and sum of squares"""
    x = x.double().reshape(groups, -1, x.shape[-1])
    return torch.stack([x.sum(1), (x * x).sum(1)], -1)


def bn_finalize_ref(totals, gamma, beta, rmean, rvar, count, momentum, eps):
    """-> dict(scale, shift, mean, rstd: [groups, C]; rmean, rvar: [C] after `groups` EMA updates in group order with the unbiased
    variance -- the biased one when count == 1).  totals None: eval, scale / shift / mean / rstd [C] from the running statistics,
    which stay as they are.  All float64."""
    gamma, beta, rmean, rvar = gamma.double(), beta.double(), rmean.double().clone(), rvar.double().clone()
    if totals is None:
        rstd = 1.0 / torch.sqrt(rvar + eps)
        scale = gamma * rstd
        return dict(scale=scale, shift=beta - rmean * scale, mean=rmean.clone(), rstd=rstd, rmean=rmean, rvar=rvar, terms=None)
    mean = totals[..., 0] / count
    var = (totals[..., 1] / count - mean * mean).clamp(min=0.0)
    rstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma * rstd
    unbiased = var * count / (count - 1) if count > 1 else var
    # the largest magnitude that enters the two EMA chains, per channel (the bound of the float32 running statistics)
    terms = torch.stack([rmean.abs(), rvar.abs(), mean.abs().amax(0), unbiased.abs().amax(0)]).amax(0)
    for g in range(totals.shape[0]):
        rmean = (1.0 - momentum) * rmean + momentum * mean[g]
        rvar = (1.0 - momentum) * rvar + momentum * unbiased[g]
    return dict(scale=scale, shift=beta - mean * scale, mean=mean, rstd=rstd, rmean=rmean, rvar=rvar, terms=terms)


def bn_apply_ref(x, res, scale, shift, rows_per_group, relu):
    """y[row] = relu?(x[row] * scale[g] + shift[g] (+ res[row])), g = row // rows_per_group; scale / shift [groups, C] or [C]"""
    x = x.double()
    rows, C = x.shape
    scale, shift = scale.double().reshape(-1, C), shift.double().reshape(-1, C)
    g = torch.arange(rows) // rows_per_group
    y = x * scale[g] + shift[g]
    if res is not None:
        y = y + res.double()
    return y.clamp(min=0.0) if relu else y


def pad_rows(N, H, W, pad):
    """row index of every interior pixel (n, h, w), in that order, inside the bordered [N, H + 2 pad, W + 2 pad] layout"""
    n, h, w = torch.meshgrid(torch.arange(N), torch.arange(H), torch.arange(W), indexing="ij")
    return (((n * (H + 2 * pad) + h + pad) * (W + 2 * pad)) + w + pad).reshape(-1)


# what bn_chunking() of csrc/conv.hip documents: enough row chunks for ~1024 workgroups, 16 .. 4096 rows each.  The library
# reports only the workspace size (and 0 for a channel count the statistics kernel refuses): test_trunk_kernels_gpu.py checks this
# restatement against it wherever it answers, and uses it to plant totals for a C the statistics kernel does not take.
def bn_chunks(rows_per_group, groups, C):
    slabs = (C + 255) // 256
    chunks = (1024 + slabs * groups - 1) // (slabs * groups)
    chunk = min(4096, max(16, (rows_per_group + chunks - 1) // chunks))
    return (rows_per_group + chunk - 1) // chunk, chunk


def bn_workspace(rows_per_group, groups, C):
    """doubles: [groups, chunks, C, 2] partials, then the totals [groups, C, 2]"""
    return (groups * bn_chunks(rows_per_group, groups, C)[0] + groups) * C * 2


def bn_stats_ok(C):
    """channel counts fcmf_bn_stats takes: a whole number of 256-channel slabs, or a divisor of 1024 that is a multiple of 4"""
    return C > 0 and C % 4 == 0 and (C % 256 == 0 if C >= 256 else 256 % (C // 4) == 0)


# ---- pools ----------------------------------------------------------------------------------------------------------------------
def maxpool_ref(x):
    """3 x 3, stride 2, pad 1 on x [N, H, W, C] -> [N, Ho, Wo, C]; a padding tap never wins (it is -inf)"""
    x = x.double()
    N, H, W, C = x.shape
    Ho, Wo = conv_out(H, 3, 2, 1), conv_out(W, 3, 2, 1)
    xp = torch.full((N, H + 2, W + 2, C), float("-inf"), dtype=torch.float64)
    xp[:, 1:1 + H, 1:1 + W] = x
    out = torch.full((N, Ho, Wo, C), float("-inf"), dtype=torch.float64)
    for r in range(3):
        for s in range(3):
            out = torch.maximum(out, xp[:, r:r + (Ho - 1) * 2 + 1:2, s:s + (Wo - 1) * 2 + 1:2])
    return out


def avg_windows(H, oh):
    """[floor(i H / oh), ceil((i + 1) H / oh)) for i in 0 .. oh - 1"""
    return [((i * H) // oh, -((-(i + 1) * H) // oh)) for i in range(oh)]


def avgpool_ref(x, oh, ow, layout):
    """adaptive average pool of x [N, H, W, C] -> (y, window size, sum of |x| over the window), each [N, C, oh, ow] (layout 0)
    or [N, oh * ow, C] (layout 1)"""
    x = x.double()
    N, H, W, C = x.shape
    y, cnt, mag = (torch.zeros(N, oh, ow, C, dtype=torch.float64) for _ in range(3))
    for i, (h0, h1) in enumerate(avg_windows(H, oh)):
        for j, (w0, w1) in enumerate(avg_windows(W, ow)):
            win = x[:, h0:h1, w0:w1]
            cnt[:, i, j] = (h1 - h0) * (w1 - w0)
            y[:, i, j] = win.sum((1, 2)) / ((h1 - h0) * (w1 - w0))
            mag[:, i, j] = win.abs().sum((1, 2))
    if layout == 0:
        return tuple(t.permute(0, 3, 1, 2).contiguous() for t in (y, cnt, mag))
    return tuple(t.reshape(N, oh * ow, C) for t in (y, cnt, mag))


def representable(t, dtype):
    """every entry of the float64 tensor survives the cast to `dtype`"""
    return bool((t.to(dtype).double() == t).all())


def is_pow2(n):
    n = np.asarray(n, dtype=np.int64)
    return (n & (n - 1)) == 0
