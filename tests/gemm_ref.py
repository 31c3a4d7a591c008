"""Operands whose GEMM is exact in every summation order, NaN-poisoned operand buffers, and float64 references for the GEMM and
convolution entry points of csrc/gemm.hip.  Plain module: no fixtures, and nothing here calls the library.

dyadic operands: entries from {-1, 0, 1} * 2^-shift.  Each is exact in bf16, float32 and e4m3, each product is exact, and every
partial sum of up to 2^24 of them is an integer multiple of 2^-(sa + sb) below 2^24: exact in float32 whatever the order -- an
MFMA chain, split-K slices, float atomics or a workspace reduce pass.  The float64 product is n * 2^-(sa + sb) with integer n, and a
bf16 output holds it exactly if and only if |n| <= 256.  A kernel that is right therefore EQUALS the reference, and one lost
contraction index, a bias from the neighbouring column or a fragment stored from the wrong lane changes the result by whole units
of the grid."""
import math

import torch

NAN_BYTE = 0x7F          # NaN in e4m3 (OCP e4m3fn: S.1111.111)
E4M3 = {0: 0x00, 1: 0x38, -1: 0xB8}


# ---- operands -----------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def dyadic(shape, seed, shift=0):
    """float64 tensor of entries drawn from {-1, 0, 1} * 2^-shift (seeded generator on the CPU)"""
    return torch.randint(-1, 2, tuple(shape), generator=_gen(seed)).double() * 2.0 ** -shift


def dyadic_ints(shape, seed, shift=0, lim=8):
    """float64 integers of [-lim, lim] * 2^-shift: bias, the aux of FCMF_EPI_ADD, the prior contents of an accumulated C"""
    return torch.randint(-lim, lim + 1, tuple(shape), generator=_gen(seed)).double() * 2.0 ** -shift


def pow2_scales(n, seed, lo=-2, hi=2):
    """float64 [n] powers of two 2^lo .. 2^hi that differ from row to row"""
    return 2.0 ** torch.randint(lo, hi + 1, (n,), generator=_gen(seed)).double()


def e4m3_bytes(t):
    """a ternary {-1, 0, 1} tensor as e4m3 bytes (uint8): 0x00, 0x38, 0xB8"""
    out = torch.zeros(t.shape, dtype=torch.uint8)
    out[t == 1] = E4M3[1]
    out[t == -1] = E4M3[-1]
    return out


class Poisoned:
    """`view`: the operand [rows, cols] as the interior of a larger NaN-filled allocation, row stride `ld`"""

    def __init__(self, t, ld, rows_extra, dev, pad=64):
        t = t if t.dim() == 2 else t.reshape(1, -1)      # (a bias, an NHWC activation: one row, poisoned outside only)
        rows, cols = t.shape
        assert ld >= cols
        es = t.element_size()
        pad = (pad * es + 15) // 16 * 16 // es           # a whole number of 16-byte units: the interior stays aligned
        nan = NAN_BYTE if t.dtype == torch.uint8 else float("nan")
        self.ld, self.pad, self.rows, self.cols = ld, pad, rows, cols
        self.buf = torch.full((2 * pad + (rows + rows_extra) * ld,), nan, dtype=t.dtype, device=dev)
        self.view = self.buf[pad:pad + rows * ld].view(rows, ld)[:, :cols]
        self.view.copy_(t.to(dev))
        assert self.view.data_ptr() % 16 == 0

    def data_ptr(self):
        return self.view.data_ptr()


def poisoned(t, ld, rows_extra, dev):
    """Everything a kernel may touch of an operand lies inside the allocation: NaN in the columns cols .. ld of every row, in
    `rows_extra` rows behind the last one and in a frame on both sides.  A kernel that lets any of it reach an accumulator it
    stores yields NaN, which is neither equal to the reference nor finite.  ld: a multiple of 8 for the MFMA paths."""
    return Poisoned(t, ld, rows_extra, dev)


# ---- float64 references -------------------------------------------------------------------------------------------------------
def product(A, B, trans_a, trans_b):
    """op(A) [M, K] op(B) [K, N]: A stored [K, M] when trans_a else [M, K]; B stored [K, N] when trans_b else [N, K]"""
    A, B = A.double(), B.double()
    return (A.t() if trans_a else A) @ (B if trans_b else B.t())


def phi(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu(x):
    return x * phi(x)


def gelu_grad(x):
    return phi(x) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def epilogue(acc, epi, bias=None, aux=None):
    """-> (C, the aux the epilogue writes or None), float64.  epi: NONE (C = acc + bias), ADD, GELU (aux <- the pre-activation),
    DGELU (aux = pre-activation), TANH, DTANH (aux = the tanh output)"""
    v = acc.double() + (0.0 if bias is None else bias.double())
    a = None if aux is None else aux.double()
    if epi == "NONE":
        return v, None
    if epi == "ADD":
        return v + a, None
    if epi == "GELU":
        return gelu(v), v
    if epi == "DGELU":
        return v * gelu_grad(a), None
    if epi == "TANH":
        return torch.tanh(v), None
    if epi == "DTANH":
        return v * (1.0 - a * a), None
    raise ValueError(epi)


def colsum(C):
    return C.double().sum(0)


def colblocks(C, col_block):
    """[M, N] -> [N / col_block, M, col_block]: block b holds the columns b * col_block .. of every row (fcmf_gemm_colblocks)"""
    M, N = C.shape
    return C.reshape(M, N // col_block, col_block).permute(1, 0, 2).contiguous()


def colstats(C, block_rows=128):
    """[ceil(M / block_rows), N, 2]: (sum, sum of squares) of every block of rows per column (fcmf_gemm_colstats)"""
    C = C.double()
    M, N = C.shape
    nb = (M + block_rows - 1) // block_rows
    out = torch.zeros(nb, N, 2, dtype=torch.float64)
    for b in range(nb):
        blk = C[b * block_rows:(b + 1) * block_rows]
        out[b, :, 0], out[b, :, 1] = blk.sum(0), (blk * blk).sum(0)
    return out


def conv_nhwc(x, w, stride, Ho, Wo):
    """direct convolution: x [n, Hp, Wp, C] (its zero border is part of it), w [Cout, kh, kw, C] -> [n * Ho * Wo, Cout],
    y[(n, oy, ox), co] = sum over (ky, kx, c) of x[n, oy * stride + ky, ox * stride + kx, c] * w[co, ky, kx, c]"""
    x, w = x.double(), w.double()
    n, Cout, kh, kw = x.shape[0], w.shape[0], w.shape[1], w.shape[2]
    y = torch.zeros(n, Ho, Wo, Cout, dtype=torch.float64)
    for ky in range(kh):
        for kx in range(kw):
            tap = x[:, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride, :]
            y += tap @ w[:, ky, kx, :].t()
    return y.reshape(n * Ho * Wo, Cout)


def conv_runs(x, w, stride, Ho, Wo):
    """fcmf_conv_gemm_runs: x [n, Hp, Wp, pix] flat per image row, w [Cout, kh, run]: for every kernel row ky one contiguous run of
    `run` elements from pixel (oy * stride + ky, ox * stride); a run may reach into the next row of the buffer (zero weights there)"""
    x, w = x.double(), w.double()
    n, Hp, Wp, pix = x.shape
    Cout, kh, run = w.shape
    flat = torch.cat([x.reshape(n * Hp * Wp * pix), torch.zeros(run, dtype=torch.float64)])
    y = torch.zeros(n, Ho, Wo, Cout, dtype=torch.float64)
    for b in range(n):
        for oy in range(Ho):
            for ox in range(Wo):
                for ky in range(kh):
                    s = ((b * Hp + oy * stride + ky) * Wp + ox * stride) * pix
                    y[b, oy, ox] += w[:, ky, :] @ flat[s:s + run]
    return y.reshape(n * Ho * Wo, Cout)


def on_grid(t, shift, limit):
    """every entry is n * 2^-shift with integer |n| <= limit"""
    n = t.double() * 2.0 ** shift
    return bool((n == n.round()).all()) and float(n.abs().max()) <= limit


def max_n(t, shift):
    return float((t.double() * 2.0 ** shift).abs().max())
