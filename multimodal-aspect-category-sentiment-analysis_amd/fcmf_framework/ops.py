"""Autograd operators of the FCMF hot path, each a thin torch.autograd.Function over the C ABI
of libfcmf_hip.so.  PyTorch supplies device memory, the stream and the autograd tape; every
FLOP and every byte of the step runs in the hand-written gfx950 kernels.

Activations are float32 (parity mode) or bfloat16 (throughput mode); master parameters and
their gradients are always float32.  bf16 copies of the weights ("shadows") are cached and
refreshed when the parameter changes.
"""
import ctypes
import math
import os

import torch

from . import _hip as H, attn
from .attn import valu_float32_key_limit      # noqa: F401  (part of this module's surface: DESIGN.md, shared_kv_attention)
from .shadows import VOCAB_PAD, shadows      # noqa: F401  (the weight-shadow cache: `ops.shadows` is the one instance)

# --------------------------------------------------------------------------------------
# global state: compute dtype, fp8 switch, dropout seeds
# --------------------------------------------------------------------------------------
_compute_dtype = torch.float32


def set_compute_dtype(dtype):
    """Activation storage type of the hot path: torch.float32 (parity) or torch.bfloat16 (MFMA)."""
    global _compute_dtype
    if dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("compute dtype must be torch.float32 or torch.bfloat16")
    _compute_dtype = dtype


def compute_dtype():
    return _compute_dtype


_fp8 = False


def set_fp8(on):
    """BASELINE configs[4]: forward and dX GEMMs of the bf16 mode on e4m3 operands (per-row scales, float32 accumulation,
    v_mfma_scale_f32_16x16x128_f8f6f4); weight gradients, attention, LayerNorm and the optimizer are unchanged"""
    global _fp8
    _fp8 = bool(on)


def fp8_enabled():
    return _fp8 and _compute_dtype == torch.bfloat16


_output_attentions = False


def set_output_attentions(on):
    """Opt-in attention-probability outputs: RobertaModel via FeatureExtractor returns one [B, heads, S, S] float32 tensor per text
    layer (`enc_attentions`), the IAOG decoder's Attention keeps and returns its [n_head*B, q_len, k_len] `attention_weights`.  The
    probabilities are recomputed from Q and K by their own kernels (fcmf_attn_probs / fcmf_attn_mfma_probs) and are the softmax
    BEFORE dropout.  Off (the default): nothing is computed and no launch is added."""
    global _output_attentions
    _output_attentions = bool(on)


def output_attentions():
    return _output_attentions


_output_fusion_attentions = False


def set_output_fusion_attentions(on):
    """Opt-in attention maps of the fusion layers, separate from set_output_attentions: FCMFEncoder.encode_aspects fills
    `encoder.fusion_attentions` (text2img, text2roi, fusion, box) and BoxMultiHeadedAttention keeps `box_attn`, all float32, the
    softmax BEFORE dropout, recomputed by attention_probs from the q / k / mask / bias each layer itself used.  Off (the default):
    the attributes are None, nothing is allocated and no launch is added."""
    global _output_fusion_attentions
    _output_fusion_attentions = bool(on)


def output_fusion_attentions():
    return _output_fusion_attentions


_ffn_dropout = False


def set_ffn_dropout(on):
    """Opt-in feed-forward dropout of torch_layers.TransformerEncoderLayer: linear2(dropout(gelu(linear1(x)))), as
    nn.TransformerEncoderLayer trains it, with the mask inside the two FFN GEMMs' epilogues (fcmf_gemm_drop: no pass of its own
    over the [M, dim_feedforward] activation, nothing saved for it).  Off (the default): linear2(gelu(linear1(x))), and no launch,
    seed draw or argument differs.  The FCMF and IAOG layers have no such dropout and do not look at the switch."""
    global _ffn_dropout
    _ffn_dropout = bool(on)


def ffn_dropout():
    return _ffn_dropout


_seed_base = 0x5DEECE66D
_seed_ctr = 0


def manual_seed(seed):
    """Seed the counter-based dropout generator (independent of torch's generator)."""
    global _seed_base, _seed_ctr
    _seed_base = (int(seed) * 0x9E3779B97F4A7C15 + 0x632BE59BD9B4E019) & 0xFFFFFFFFFFFFFFFF
    _seed_ctr = 0


def next_seed():
    global _seed_ctr
    _seed_ctr += 1
    x = (_seed_base + _seed_ctr * 0xD1342543DE82EF95) & 0xFFFFFFFFFFFFFFFF
    x ^= x >> 29
    return (x * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF


TOPK_MAX = 16    # fcmf_logsoftmax_topk's limit on k (include/fcmf_hip.h)
SAMPLE_MAX_V = 1 << 20    # fcmf_sample_token's limit on the number of columns (include/fcmf_hip.h)

# --------------------------------------------------------------------------------------
# flat gradient arena (dp.GradArena): weight-gradient buffers come out of the parameter's slice of ONE zeroed
# buffer when an arena is active, so that autograd adopts the slice as p.grad (no copy) and a step needs one memset
# --------------------------------------------------------------------------------------
_grad_arena = None


def set_grad_arena(arena):
    global _grad_arena
    _grad_arena = arena
    if arena is not None and deferred_dw.reset not in arena.on_zero:
        arena.on_zero.append(deferred_dw.reset)      # a step that died inside backward() must not leave its queue to the next one


def grad_arena():
    return _grad_arena


def grad_dest(param, shape, *, rows=None, in_place=True, temp=True, device=None):
    """where a backward writes the float32 gradient of `param` -> (buf, ret): the kernel ACCUMULATES into `buf` (zero, or holding
    what earlier producers of this pass wrote), the backward returns `ret` to autograd.  param: a Parameter viewed as `shape`, or a
    list of Parameters whose gradients lie back to back in one buffer of `shape` (fused q|k|v: the caller splits `ret`), or None.
    rows: the producer writes `rows` >= shape[0] rows (the padded vocabulary projection): `buf` is [rows, shape[1]].
    * an arena is active and the slice is unclaimed in this pass (dp.GradArena.claim): `buf` is the slice, `ret` an alias of it that
      autograd adopts as p.grad -- no fill, no copy;
    * an earlier producer of a shared weight has claimed it: `buf` is the slice again and `ret` None (accumulated in place); with
      in_place=False (the embedding tables) such a producer gets a temporary instead;
    * no arena, "not here", or not a float32 contiguous tensor of prod(shape) elements: one zero-filled temporary on `device`
      (default: the parameter's) that autograd adds -- or (None, None) with temp=False, for a caller that fills all its
      temporaries at once."""
    a = _grad_arena
    if a is not None and param is not None:
        if isinstance(param, (list, tuple)):
            ok = all(q.dtype == torch.float32 and q.is_contiguous() for q in param) and sum(q.numel() for q in param) == math.prod(shape)
        else:
            ok = param.dtype == torch.float32 and param.is_contiguous() and param.numel() == math.prod(shape)
        got = a.claim(param, rows) if ok else None
        if got is not None and (got[1] or in_place):
            buf, first = got
            if rows is None:
                buf = buf.view(shape)
                return buf, (buf if first else None)
            return buf, (a.grad_alias(param, shape) if first else None)
    if not temp:
        return None, None
    if device is None:
        device = (param[0] if isinstance(param, (list, tuple)) else param).device
    if rows is None:
        buf = torch.zeros(shape, dtype=torch.float32, device=device)
        return buf, buf
    buf = torch.zeros((rows,) + tuple(shape[1:]), dtype=torch.float32, device=device)
    return buf, buf[:shape[0]]


def as_compute(w, dtype):
    """parameter as seen by a kernel computing in `dtype`"""
    if dtype == torch.float32:
        return w.detach()
    return shadows.get(w)


def cast(x, dtype):
    """dtype conversion through fcmf_cast (float32 <-> bfloat16)"""
    if x.dtype == dtype:
        return x
    H.require_cuda(x)
    x = x.contiguous()
    y = torch.empty(x.shape, dtype=dtype, device=x.device)
    H.check(H.lib().fcmf_cast(H.ptr(x), H.ptr(y), x.numel(), H.dt(x), H.dt(y), H.stream()), "fcmf_cast")
    return y


class _CastFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, dtype):
        ctx.src = x.dtype
        return cast(x, dtype)

    @staticmethod
    def backward(ctx, dy):
        return cast(dy.contiguous(), ctx.src), None


def cast_ad(x, dtype):
    return x if x.dtype == dtype else _CastFn.apply(x, dtype)


# --------------------------------------------------------------------------------------
# raw kernel wrappers
# --------------------------------------------------------------------------------------
def _rows(x):
    """2-D view [rows, features] with unit inner stride (row stride may be arbitrary)"""
    if x.dim() != 2:
        x = x.reshape(-1, x.shape[-1])
    if x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
        x = x.contiguous()
    return x


_gemm_trace = None


def gemm_trace_begin():
    """start recording a HIP event pair (on the launch stream) around every GEMM launch"""
    global _gemm_trace
    _gemm_trace = []


def gemm_trace_end():
    """-> [(kernel name, flops, milliseconds)] for the launches since gemm_trace_begin()"""
    global _gemm_trace
    tr, _gemm_trace = _gemm_trace, None
    if not tr:
        return []
    torch.cuda.synchronize()
    return [(name, fl, e0.elapsed_time(e1) * share) for name, fl, e0, e1, share in tr]


def tracing():
    return _gemm_trace is not None


class trace_launch:
    """`with trace_launch(flops):` around a library call that multiplies on the GEMM context of the current stream (`gemm`, the
    trunk's implicit-GEMM convolutions): records (kernel name, flops, start event, end event) when a trace is open and the call
    did not raise, free otherwise.  A call that launched nothing sets `.flops = None`: nothing is recorded.  `flops` may be a list:
    the launch multiplied several groups of matrices (a weight-gradient list: one group per shape) and is recorded once per group,
    with the group's FLOPs and its share, by FLOPs, of the launch's time -- sums per kernel name are those of the launch."""

    def __init__(self, flops):
        self.flops = flops

    def __enter__(self):
        if _gemm_trace is not None:
            self.e0, self.e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *exc):
        if _gemm_trace is not None and exc[0] is None and self.flops is not None:
            self.e1.record()
            name = H.lib().fcmf_gemm_ctx_last_kernel(H.gemm_ctx()).decode()
            parts = [float(f) for f in self.flops] if isinstance(self.flops, (list, tuple)) else [float(self.flops)]
            total = sum(parts)
            for f in parts:
                _gemm_trace.append((name, f, self.e0, self.e1, f / total if total else 1.0 / len(parts)))
        return False


# ---- deferred weight gradients -------------------------------------------------------------------------------------------
# dW = dY^T X of an nn.Linear is needed only once the backward pass is over (grad clipping, the optimizer, the gradient
# exchange of its bucket), and one layer's dW is a handful of 256 x 256 tiles: alone it fills the chip only through a deep
# split of K plus a reduce pass per matrix.  During loss.backward() the weight-gradient GEMMs whose destination is a slice of the
# step's gradient arena are therefore QUEUED (operands kept alive) and multiplied together, everything that is flushed -- whatever
# its shape -- as ONE work list (fcmf_gemm_dw_list: one GEMM launch, one reduce launch): at the end of the backward pass (an
# autograd-engine callback), before a data-parallel bucket that contains queued gradients is sent (dp.GradReducer), before anything
# else reads the arena (flush_deferred_dw), or when the queue holds more than DEFER_DW_MAX_BYTES of operands.  A weight applied
# SEVERAL times (the mm layer's key / value weights: text keys, ROI keys, the fusion layer) has several producers; every one of them
# accumulates in place into the slice the first one claimed and hands autograd None (grad_dest / GradArena.claim), so they all wait
# for the flush too: the list gives a destination with several producers partial tiles only, which its reduce pass adds in a
# fixed order -- no two work items write the same tile.  The destination is remembered by address, never by tensor: autograd must
# stay the only holder of the returned slice, or AccumulateGrad clones it -- unwritten -- instead of adopting it as p.grad.
DEFER_DW = os.environ.get("FCMF_DEFER_DW", "1") == "1"
DEFER_DW_MAX_BYTES = 48 << 30


class _DeferredDW:
    def __init__(self):
        self.q, self.bytes, self.armed = [], 0, False
        self.batched_launches = self.batched_matrices = 0

    def reset(self):
        self.q, self.bytes, self.armed = [], 0, False

    def wanted(self, A, B, C, ta, tb, bias, aux, epi, colsum):
        if not (DEFER_DW and ta and tb and bias is None and aux is None and colsum is None and epi == H.EPI_NONE
                and C.dtype == torch.float32 and A.dtype == torch.bfloat16 and B.dtype == torch.bfloat16):
            return False
        arena = _grad_arena
        if not (arena is not None and C.device == arena.flat.device
                and C.untyped_storage().data_ptr() == arena.flat.untyped_storage().data_ptr()):
            return False
        # (a destination outside the arena -- the temporaries of a gradient-accumulation micro-step -- never gets here)
        return arena.uses(C.data_ptr()) >= 1

    def push(self, A, B, C, M, N, K, lda, ldb, ldc, acc):
        if not self.armed:
            try:      # (only legal while the autograd engine runs: outside of backward() the GEMM runs right away)
                torch.autograd.Variable._execution_engine.queue_callback(self.flush)
            except RuntimeError:
                return False
            self.armed = True
        # (the destination is remembered by ADDRESS: the arena owns that memory, and a second reference to the tensor object would
        #  make autograd's AccumulateGrad clone the -- not yet written -- slice instead of adopting it as p.grad)
        self.q.append((A, B, C.data_ptr(), M, N, K, lda, ldb, ldc, bool(acc)))
        self.bytes += A.numel() * A.element_size() + B.numel() * B.element_size()
        if self.bytes > DEFER_DW_MAX_BYTES:
            self.flush(final=False)
        return True

    def flush(self, final=True, lo=None, hi=None):
        """multiply the queued gradients; lo / hi: only those whose destination address lies in [lo, hi) (the arena range a
        data-parallel bucket group is about to send) -- the rest stays queued and keeps batching"""
        if lo is not None:
            q = [e for e in self.q if lo <= e[2] < hi]
            if not q:
                return
            self.q = [e for e in self.q if not (lo <= e[2] < hi)]
            self.bytes = sum(e[0].numel() * e[0].element_size() + e[1].numel() * e[1].element_size() for e in self.q)
        else:
            q, self.q, self.bytes = self.q, [], 0
        if final:
            self.armed = False
        groups = {}      # (one list per device and accumulate flag: in a training step, one)
        for e in q:
            groups.setdefault((e[0].device, e[9]), []).append(e)
        for (device, acc), es in groups.items():
            H.require_cuda(es[0][0])
            n = len(es)
            with torch.cuda.device(device):
                ctx = H.gemm_ctx(workspace=True)
                ptrs = lambda i: (ctypes.c_void_p * n)(*[e[i] if i == 2 else e[i].data_ptr() for e in es])
                ints = lambda i: (ctypes.c_int * n)(*[e[i] for e in es])
                lds = lambda i: (ctypes.c_int64 * n)(*[e[i] for e in es])
                by_shape = {}
                for e in es:
                    by_shape[e[3:6]] = by_shape.get(e[3:6], 0.0) + 2.0 * e[3] * e[4] * e[5]
                with trace_launch(list(by_shape.values())):
                    if all(e[3:9] == es[0][3:9] for e in es):      # one shape: the same list through the same-shape entry point
                        M, N, K, lda, ldb, ldc = es[0][3:9]
                        H.check(H.lib().fcmf_gemm_dw_batched(ctx, n, ptrs(0), ptrs(1), ptrs(2), M, N, K, lda, ldb, ldc, int(acc), H.stream()),
                                "fcmf_gemm_dw_batched")
                    else:
                        H.check(H.lib().fcmf_gemm_dw_list(ctx, n, ptrs(0), ptrs(1), ptrs(2), ints(3), ints(4), ints(5), lds(6), lds(7), lds(8),
                                                          int(acc), H.stream()), "fcmf_gemm_dw_list")
            self.batched_launches += 1
            self.batched_matrices += n


deferred_dw = _DeferredDW()


def flush_deferred_dw(lo=None, hi=None):
    """multiply the queued weight gradients now (anything that reads the gradient arena before backward() has returned);
    lo / hi (device addresses): only the ones whose destination lies in that range of the arena"""
    if deferred_dw.q:
        deferred_dw.flush(final=False, lo=lo, hi=hi)


_DROP_EPI = (H.EPI_GELU_DROP, H.EPI_DGELU_DROP)


def gemm(A, B, C, M, N, K, lda, ldb, ldc, ta, tb, bias=None, aux=None, epi=H.EPI_NONE, acc=False, colsum=None, drop=None):
    """drop = (p, seed) with epi = H.EPI_GELU_DROP / H.EPI_DGELU_DROP: fcmf_gemm_drop (the dropout mask over the [M, N] output in
    the epilogue); the two belong together"""
    H.require_cuda(A, B, C)
    if (drop is not None) != (epi in _DROP_EPI) or (drop is not None and acc):
        raise H.HipLibraryError("gemm: drop=(p, seed) goes with EPI_GELU_DROP / EPI_DGELU_DROP, only with them, and writes C")
    if drop is not None:
        with trace_launch(2.0 * M * N * K):
            H.check(H.lib().fcmf_gemm_drop(H.gemm_ctx(), H.ptr(A), H.ptr(B), H.ptr(C), H.ptr(bias), H.ptr(aux), H.ptr(colsum), M, N, K,
                                           lda, ldb, ldc, int(ta), int(tb), H.dt(A), H.dt(C), epi, float(drop[0]), int(drop[1]),
                                           H.stream()), "fcmf_gemm_drop")
        return
    if deferred_dw.wanted(A, B, C, ta, tb, bias, aux, epi, colsum) and deferred_dw.push(A, B, C, M, N, K, lda, ldb, ldc, acc):
        return
    ctx = H.gemm_ctx(workspace=acc or C.dtype == torch.float32)   # (weight-gradient GEMMs: the context owns the split-K scratch of this stream)
    with trace_launch(2.0 * M * N * K):
        H.check(H.lib().fcmf_gemm(ctx, H.ptr(A), H.ptr(B), H.ptr(C), H.ptr(bias), H.ptr(aux), H.ptr(colsum), M, N, K, lda, ldb, ldc,
                                  int(ta), int(tb), H.dt(A), H.dt(C), epi, int(acc), H.stream()), "fcmf_gemm")


HEAD_WGRAD_DIRECT = os.environ.get("FCMF_HEAD_WGRAD_DIRECT", "1") == "1"      # (A/B switch)


def head_weight_grad(x2, dy2, params):
    """gradient of the per-head projection weights `params` (float32 Parameters [n_head, E, d], side by side in dy2's columns) of the
    IAOG decoder's Attention, written DIRECTLY in the parameters' layout into their adjacent arena slices: dW^T [E, len * n_head * d]
    = x2^T dy2 through fcmf_gemm_colblocks (column block = d, block stride = E * d, row stride = d).  -> the tensors to hand autograd
    (the arena views), or None when it does not apply (no arena, slices not adjacent / already claimed, shape the blocked path
    refuses): the caller then multiplies into a plain [n * d, E] buffer and lets autograd permute-copy it (round 3: 96 launches
    per IAOG step)."""
    a = _grad_arena
    if a is None or dy2.dtype != torch.bfloat16 or x2.dtype != torch.bfloat16 or not HEAD_WGRAD_DIRECT:
        return None
    nh, E, d = params[0].shape
    if any(p.dtype != torch.float32 or tuple(p.shape) != (nh, E, d) for p in params) or d % 4:
        return None
    M, N = x2.shape[0], len(params) * nh * d
    if E < 256 or N < 256 or dy2.shape[1] != N or not dy2.is_contiguous():
        return None
    got = a.claim(list(params))
    if got is None or not got[1]:          # (a second producer would have to ACCUMULATE: the blocked kernel overwrites)
        return None
    with trace_launch(2.0 * E * N * M) as t:
        rc = H.lib().fcmf_gemm_colblocks(H.gemm_ctx(workspace=True), H.ptr(x2), H.ptr(dy2), H.ptr(got[0]), E, N, M, _ld(x2), N, d, 1, 1,
                                         d, E * d, 0, H.stream())
        if rc == H.ERR_UNSUPPORTED:
            t.flops = None
            a.release(params)
            return None
        H.check(rc, "fcmf_gemm_colblocks")
    return [a.grad_alias(p, (nh, E, d)) for p in params]


def _fp8_buffers(rows, K, device):
    """(q [rows, K] uint8 for e4m3 values, scale [rows] float32), uninitialised"""
    return torch.empty((rows, K), dtype=torch.uint8, device=device), torch.empty(rows, dtype=torch.float32, device=device)


def quant_fp8_rows(x, rows, K, ldx, out=None):
    """x [rows, K] (bf16 / f32 rows at stride ldx) -> (q [rows, K] uint8 e4m3, scale [rows] float32) through fcmf_quant_fp8_rows"""
    H.require_cuda(x)
    q, sc = _fp8_buffers(rows, K, x.device) if out is None else out
    H.check(H.lib().fcmf_quant_fp8_rows(H.ptr(x), ldx, H.ptr(q), K, H.ptr(sc), rows, K, H.dt(x), H.stream()), "fcmf_quant_fp8_rows")
    return q, sc


def _fp8_ok(M, N, K, ldc, *tensors):
    return (fp8_enabled() and K % 128 == 0 and N % 8 == 0 and ldc % 8 == 0 and M >= 256 and N >= 256
            and all(t is None or t.dtype == torch.bfloat16 for t in tensors))


def gemm_fp8(xq, sx, wq, sw, C, M, N, K, bias=None, aux=None, epi=H.EPI_NONE, colsum=None):
    with trace_launch(2.0 * M * N * K):
        H.check(H.lib().fcmf_gemm_fp8(H.gemm_ctx(), H.ptr(xq), H.ptr(sx), H.ptr(wq), H.ptr(sw), H.ptr(C), H.ptr(bias), H.ptr(aux), H.ptr(colsum),
                                      M, N, K, K, K, N, epi, H.stream()), "fcmf_gemm_fp8")


def gemm_nt(x, weight, w_compute, y, M, N, K, ldx, bias=None, aux=None, epi=H.EPI_NONE, colsum=None, owner=None, xq=None, drop=None):
    """y [M, N] = epilogue(x [M, K] W^T + bias), W [N, K]: the forward GEMM of nn.Linear.  `weight` = the float32 master (or a
    view of it; `owner` = its Parameter) when there is one: the fp8 mode then multiplies e4m3 copies (x quantised per row here,
    W per output row, cached); otherwise the bf16 / f32 kernel on `w_compute`.  drop = (p, seed): see gemm; such a GEMM stays on
    the bf16 / f32 kernel in fp8 mode too (the e4m3 kernel has no dropout epilogue)."""
    if _grad_arena is not None and (owner is not None or weight is not None):
        _grad_arena.note_forward((owner if owner is not None else weight).data_ptr())     # (see deferred_dw.wanted)
    if drop is not None:
        gemm(x, w_compute, y, M, N, K, ldx, K, N, 0, 0, bias=bias, aux=aux, epi=epi, colsum=colsum, drop=drop)
    elif weight is not None and weight.dtype == torch.float32 and weight.dim() == 2 and _fp8_ok(M, N, K, N, x, y, aux):
        xq, sx = quant_fp8_rows(x, M, K, ldx) if xq is None else xq       # (xq: already quantised by the producing LayerNorm)
        wq, sw = shadows.get_fp8(weight, owner)
        gemm_fp8(xq, sx, wq, sw, y, M, N, K, bias=bias, aux=aux, epi=epi, colsum=colsum)
    else:
        gemm(x, w_compute, y, M, N, K, ldx, K, N, 0, 0, bias=bias, aux=aux, epi=epi, colsum=colsum)


def colsum(X, M, N, ldx):
    out = torch.empty(N, dtype=torch.float32, device=X.device)
    H.check(H.lib().fcmf_colsum(H.ptr(X), H.ptr(out), M, N, ldx, H.dt(X), 0, H.stream()), "fcmf_colsum")
    return out


def _ld(x):
    return x.stride(0) if x.shape[0] > 1 else x.shape[1]


def gemm_dx(dy, weight, w_compute, dx, M, K_in, N_out, aux=None, epi=H.EPI_NONE, colsum=None, owner=None, dyq=None, drop=None):
    """dx [M,K_in] = dy [M,N_out] @ W [N_out,K_in] (+ epilogue).  bf16 mode multiplies by the transposed bf16 copy of the
    float32 master `weight` (an NT GEMM); f32 mode, or a weight without a master, uses `w_compute` as it lies (NN).
    drop = (p, seed): see gemm; never the e4m3 kernel."""
    if (drop is None and weight is not None and weight.dtype == torch.float32 and weight.dim() == 2 and dy.is_contiguous()
            and _fp8_ok(M, K_in, N_out, K_in, dy, dx, aux)):
        dyq, sdy = quant_fp8_rows(dy, M, N_out, N_out) if dyq is None else dyq
        wq, sw = shadows.get_fp8_t(weight, owner)                    # [K_in, N_out] e4m3, scales per input row
        gemm_fp8(dyq, sdy, wq, sw, dx, M, K_in, N_out, aux=aux, epi=epi, colsum=colsum)
    elif dy.dtype == torch.bfloat16 and weight is not None and weight.dtype == torch.float32 and weight.dim() == 2:
        wt = shadows.get_t(weight, owner)                            # [K_in, N_out]; owner: the Parameter behind a temporary view
        gemm(dy, wt, dx, M, K_in, N_out, N_out, N_out, K_in, 0, 0, aux=aux, epi=epi, colsum=colsum, drop=drop)
    else:
        gemm(dy, w_compute, dx, M, K_in, N_out, N_out, K_in, K_in, 0, 1, aux=aux, epi=epi, colsum=colsum, drop=drop)


def gemm_dx_long_k(dy, w, M, K_in, N_out, ldw):
    """dx [M,K_in] = dy [M,N_out] @ w [N_out,K_in] for a LONG contraction and a small output (the vocabulary projection:
    N_out = 64032, M x K_in = 768 x 768): a bf16 output has 9 tiles of 256x256 = 9 busy CUs; accumulating into float32 lets
    the kernel split the contraction 28 ways over the chip (workspace + reduce pass), then one cast"""
    if dy.dtype != torch.bfloat16 or N_out < 8192:
        dx = torch.empty((M, K_in), dtype=dy.dtype, device=dy.device)
        gemm(dy, w, dx, M, K_in, N_out, N_out, ldw, K_in, 0, 1)
        return dx
    dx32 = torch.zeros((M, K_in), dtype=torch.float32, device=dy.device)
    gemm(dy, w, dx32, M, K_in, N_out, N_out, ldw, K_in, 0, 1, acc=True)
    return cast(dx32, torch.bfloat16)


def _linear_fwd(x, w, bias, epi=H.EPI_NONE, aux=None, master=None):
    M, K = x.shape
    N = w.shape[0]
    y = torch.empty((M, N), dtype=x.dtype, device=x.device)
    if epi == H.EPI_TANH or master is None:
        gemm(x, w, y, M, N, K, _ld(x), K, N, 0, 0, bias=bias, aux=aux, epi=epi)
    else:
        gemm_nt(x, master, w, y, M, N, K, _ld(x), bias=bias, aux=aux, epi=epi)
    return y


def _linear_bwd(x, w, dy, need_dx=True, need_dw=True, need_db=True, dx_epi=H.EPI_NONE, dx_aux=None, master=None, bias_param=None):
    """x [M,K], w [N,K] (compute dtype), dy [M,N] -> dx [M,K], dW [N,K] f32, db [N] f32
    (master = the float32 parameter behind w, if any: bf16 mode then uses its transposed copy for dx)"""
    M, K = x.shape
    N = w.shape[0]
    dx = dw = db = None
    if need_dx:
        dx = torch.empty((M, K), dtype=dy.dtype, device=dy.device)
        gemm_dx(dy, master, w, dx, M, K, N, aux=dx_aux, epi=dx_epi)
    if need_dw:
        dwbuf, dw = grad_dest(master, (N, K), device=dy.device)   # (dw = None: accumulated in place into the slice an earlier use returned)
        gemm(dy, x, dwbuf, N, K, M, N, _ld(x), K, 1, 1, acc=True)
    if need_db:
        if bias_param is not None and bias_param.dtype == torch.float32 and tuple(bias_param.shape) == (N,):
            # straight into the parameter's (already zero) arena slice: no output tensor, no memset inside fcmf_colsum
            dbbuf, db = grad_dest(bias_param, (N,))
            H.check(H.lib().fcmf_colsum(H.ptr(dy), H.ptr(dbbuf), M, N, N, H.dt(dy), 1, H.stream()), "fcmf_colsum")
        else:
            db = colsum(dy, M, N, N)
    return dx, dw, db


class ProjectFn(torch.autograd.Function):
    """n nn.Linear on the SAME [..., K] input as one autograd node: (x, act, row0, w1, b1, w2, b2, ...) -> one output per pair.
    n = 1 is nn.Linear itself, with act = "tanh" BertPooler's (mm_modeling.py:425-431); n > 1 are q / k / v of the box attention on
    the ROI features (roi_modeling.py:170-173) and key / value of a cross attention.  With row0 (the text encoder's output [G, S, H]
    in FCMFEncoder, fcmf_pretraining.py:97-124: key and value projection of the text+ROI layer plus the [CLS] row) x[:, 0] is one
    more output.  As separate nodes the n (+ 1) gradient contributions to x are materialised and added by the engine -- for the
    row a zero-filled [G, S, H] tensor (select_backward) -- 0.5 GB of traffic per step for nothing.  Here dx = dy1 W1, then
    dx = dx + dy_i W_i in the later dX GEMMs' epilogue (FCMF_EPI_ADD), then the row's gradient added to dx[:, 0]."""

    @staticmethod
    def forward(ctx, x, act, row0, *wb):
        x2 = _rows(x)
        ws, bs = wb[0::2], wb[1::2]
        epi = H.EPI_TANH if act == "tanh" else H.EPI_NONE
        cs = (as_compute(w, x2.dtype) for w in ws)      # lazily: a stale weight shadow is cast right before its GEMM ...
        if row0:
            cs = list(cs)                               # ... but the row0 node has always cast all of them first (the first step's call order)
        ys = [_linear_fwd(x2, c, None if b is None else b.detach(), epi, master=w) for c, w, b in zip(cs, ws, bs)]
        ctx.save_for_backward(x2, *ws, *(ys if act == "tanh" else ()))
        ctx.biases = bs            # (the Parameters themselves: grad_dest looks up their arena slices by identity)
        ctx.act, ctx.row0, ctx.xshape = act, row0, x.shape
        outs = tuple(y.view(*x.shape[:-1], y.shape[1]) for y in ys)
        return outs + (x[:, 0].contiguous(),) if row0 else outs

    @staticmethod
    def backward(ctx, *dys):
        x2, *saved = ctx.saved_tensors
        n, need = len(ctx.biases), ctx.needs_input_grad
        dx, grads = None, []
        for i, (dy, w, b) in enumerate(zip(dys, saved, ctx.biases)):
            if dy is None:             # an unused output
                grads += [None, None]
                continue
            d = dy.reshape(-1, dy.shape[-1]).contiguous()
            if ctx.act == "tanh":
                dpre = torch.empty_like(d)
                H.check(H.lib().fcmf_act_bwd(H.ptr(d), H.ptr(saved[n + i]), H.ptr(dpre), d.numel(), 0, H.dt(d), H.stream()), "act_bwd")
                d = dpre
            dx, dw, db = _linear_bwd(x2, as_compute(w, x2.dtype), d, need[0], need[3 + 2 * i], b is not None and need[4 + 2 * i],
                                     dx_epi=H.EPI_NONE if dx is None else H.EPI_ADD, dx_aux=dx, master=w, bias_param=b)
            grads += [dw, db]
        if ctx.row0 and need[0]:
            if dx is None:
                dx = torch.zeros(x2.shape, dtype=x2.dtype, device=x2.device)
            if dys[n] is not None:
                dx.view(ctx.xshape)[:, 0] += dys[n]
        return (None if dx is None else dx.view(ctx.xshape), None, None, *grads)


def linear(x, weight, bias=None, act=None):
    """y = act(x W^T + b), act in {None, "tanh"}"""
    return ProjectFn.apply(x, act, False, weight, bias)[0]


def linear_multi(x, *wb):
    """(x W1^T + b1, x W2^T + b2, ...) with ONE gradient tensor for x (see ProjectFn)"""
    return ProjectFn.apply(x, None, False, *wb)


def seq_fan(seq, w1, b1, w2, b2):
    """-> (seq W1^T + b1, seq W2^T + b2, seq[:, 0]) with ONE gradient tensor for `seq` (see ProjectFn)"""
    return ProjectFn.apply(seq, None, True, w1, b1, w2, b2)


def head_layouts(ws, dtype):
    """the per-head weights `ws` (Parameters [n_head, E, d] of the IAOG decoder's Attention, side by side) for a kernel computing in
    `dtype` other than bf16 (bf16: `shadows.head_nk`) -> ([len(ws)*n_head*d, E], the nn.Linear layout in natural head order, and a
    function that builds its transpose [E, len(ws)*n_head*d], the K-contiguous operand of dx = dy W, when it is called).  Cached on
    the PARAMETER ws[0] (`shadows.derived`), never on a temporary; the addresses of all of `ws` are part of the tag."""
    nh, E, d = ws[0].shape
    tag = (dtype,) + tuple(w.data_ptr() for w in ws)

    def build(perm, shape, dim):
        parts = [w.detach().permute(*perm).reshape(shape) for w in ws]
        return cast(parts[0] if len(parts) == 1 else torch.cat(parts, dim), dtype)
    return (shadows.derived(ws[0], ("head_nk",) + tag, lambda _: build((0, 2, 1), (nh * d, E), 0)),
            lambda: shadows.derived(ws[0], ("head_kn",) + tag, lambda _: build((1, 0, 2), (E, nh * d), 1)))


def head_project(x2, ws):
    """y[:, (i*n_head + h)*d + j] = sum_e x2[:, e] * ws[i][h, e, j]: the per-head projections of the IAOG decoder `Attention`
    (w_kx / w_qx [n_head, E, d], mm_modeling.py:57-58,79-92) of one input by every weight of `ws` as ONE GEMM against the
    [len(ws)*n_head*d, E] re-layout of the parameters instead of the reference's B-fold `repeat` + bmm per weight.
    x2 [M, E] (unit inner stride, any row stride) -> y [M, len(ws)*n_head*d]"""
    ws = list(ws)
    return _linear_fwd(x2, shadows.head_nk(ws) if x2.dtype == torch.bfloat16 else head_layouts(ws, x2.dtype)[0], None)


def head_project_bwd(x2, dy2, ws, need_dx=True, need_dw=True):
    """backward of head_project: dy2 [M, len(ws)*n_head*d] dense -> (dx [M, E] or None, [dw_i in the parameters' [n_head, E, d]
    layout] or None).  ONE dX and ONE dW GEMM for all of `ws`."""
    ws = list(ws)
    nh, E, d = ws[0].shape
    M, N = dy2.shape
    dx = dws = None
    if need_dx:
        dx = torch.empty((M, E), dtype=dy2.dtype, device=dy2.device)
        if dy2.dtype == torch.bfloat16:
            gemm(dy2, shadows.head_nk(ws), dx, M, E, N, N, E, E, 0, 1)           # NN: dx = dy W with W in the forward's [N, E] layout (no second re-layout)
        else:
            gemm(dy2, head_layouts(ws, dy2.dtype)[1](), dx, M, E, N, N, N, E, 0, 0)   # NT: both operands K-contiguous
    if need_dw:
        dws = head_weight_grad(x2, dy2, ws)                                      # straight into the parameters' adjacent [n_head, E, d] arena slices
        if dws is None:
            dwl = torch.empty((N, E), dtype=torch.float32, device=dy2.device)    # (fresh buffer: written, not accumulated into)
            gemm(dy2, x2, dwl, N, E, M, N, _ld(x2), E, 1, 1)                     # [len(ws)*n_head*d, E] = dy^T x
            dws = list(dwl.view(len(ws), nh, d, E).permute(0, 1, 3, 2))          # -> the parameters' [n_head, E, d]
    return dx, dws


class HeadLinearFn(torch.autograd.Function):
    """head_project of x [..., E] by the per-head weights ws (every decoder block's cross-attention w_kx of the same encoder
    output, mm_modeling.py:601-605; one w_qx) as one node: one [..., n_head*d] output per weight, views of the one product."""

    @staticmethod
    def forward(ctx, x, *ws):
        x2 = _rows(x)
        y = head_project(x2, ws)
        ctx.save_for_backward(x2, *ws)
        ctx.xshape = x.shape
        HD = y.shape[1] // len(ws)
        y = y.view(*x.shape[:-1], len(ws) * HD)
        return tuple(y[..., i * HD:(i + 1) * HD] for i in range(len(ws)))

    @staticmethod
    def backward(ctx, *dys):
        x2, *ws = ctx.saved_tensors
        M, HD = x2.shape[0], ws[0].shape[0] * ws[0].shape[2]
        if len(dys) == 1:
            dy2 = dys[0].reshape(-1, HD).contiguous()
        else:                                  # the weights' output gradients side by side; an unused output counts as zeros
            zero = None
            parts = []
            for g in dys:
                if g is None:
                    g = zero = torch.zeros((M, HD), dtype=x2.dtype, device=x2.device) if zero is None else zero
                parts.append(g.reshape(M, HD))
            dy2 = torch.cat(parts, 1)
        dx, dws = head_project_bwd(x2, dy2, ws, ctx.needs_input_grad[0], any(ctx.needs_input_grad[1:]))
        return (None if dx is None else dx.view(ctx.xshape), *(dws or [None] * len(ws)))


def head_linear(x, *ws):
    """-> one tensor for one weight, a tuple of them for several (see HeadLinearFn)"""
    ys = HeadLinearFn.apply(x, *ws)
    return ys[0] if len(ws) == 1 else ys


def _vocab_logits(x2, weight, bias, cache_bias=False):
    """the vocabulary projection x2 [M, K] by weight [V, K] (+ bias [V]) -> (logits [M, Vp], the weight operand [Vp, K] it used).
    bf16 and a ragged vocabulary (V no multiple of VOCAB_PAD; IAOG: the tied 64001 x 768 matrix, fcmf_pretraining.py:159-166): the
    row-padded weight shadow (rows >= V zero) into column-padded logits, so that the GEMM runs on the MFMA kernels instead of
    the any-stride f32-MFMA one -- the padding logits are exactly the padding bias, zero; else Vp = V and the plain weight.
    cache_bias: the zero-padded bias is kept on the Parameter (shadows.derived: once per parameter version, the decode loop)
    instead of being built for this call."""
    V, K = weight.shape
    M = x2.shape[0]
    w = shadows.padded(weight) if x2.dtype == torch.bfloat16 and V % VOCAB_PAD != 0 else as_compute(weight, x2.dtype)
    Vp = w.shape[0]
    bp = None if bias is None else bias.detach()
    if bp is not None and Vp != V:
        pad = lambda b: torch.cat((b.float(), b.new_zeros(Vp - V, dtype=torch.float32)))
        bp = shadows.derived(bias, ("vocab_pad", Vp), pad) if cache_bias else pad(bp)
    logits = torch.empty((M, Vp), dtype=x2.dtype, device=x2.device)
    gemm(x2, w, logits, M, Vp, K, _ld(x2), K, Vp, 0, 0, bias=bp)
    return logits, w


def _vocab_bwd(d, x2, w, V, need_dx, need_db, dwp):
    """backward of _vocab_logits: d [M, Vp] the logit gradient (padding columns zero), w the weight operand the forward used ->
    (dx [M, K] or None, db [V] or None); dW = d^T x2 is ACCUMULATED into dwp [Vp, K] float32 where one is given"""
    M, Vp = d.shape
    K = x2.shape[1]
    dx = gemm_dx_long_k(d, w, M, K, Vp, K) if need_dx else None
    if dwp is not None:
        gemm(d, x2, dwp, Vp, K, M, Vp, _ld(x2), K, 1, 1, acc=True)
    return dx, (colsum(d, M, Vp, Vp)[:V] if need_db else None)


class VocabLinearFn(torch.autograd.Function):
    """logits = x W^T + b for a ragged vocabulary in bf16 mode (_vocab_logits) in the reference's shape [..., V]: one compaction
    copy of the padded logits forward, one padded re-copy of their gradient backward"""

    @staticmethod
    def forward(ctx, x, weight, bias):
        x2 = _rows(x)
        V = weight.shape[0]
        y, ctx.w = _vocab_logits(x2, weight, bias)
        ctx.save_for_backward(x2, weight)
        ctx.has_bias = bias is not None
        ctx.xshape = x.shape
        return y[:, :V].reshape(*x.shape[:-1], V)

    @staticmethod
    def backward(ctx, dy):
        x2, weight = ctx.saved_tensors
        need = ctx.needs_input_grad
        V, K = weight.shape
        M, Vp = x2.shape[0], ctx.w.shape[0]
        dyp = torch.zeros((M, Vp), dtype=x2.dtype, device=x2.device)
        dyp[:, :V] = dy.reshape(M, V)
        dwp = torch.zeros((Vp, K), dtype=torch.float32, device=x2.device) if need[1] else None
        dx, db = _vocab_bwd(dyp, x2, ctx.w, V, need[0], ctx.has_bias and need[2], dwp)
        return None if dx is None else dx.view(ctx.xshape), None if dwp is None else dwp[:V], db


def vocab_linear(x, weight, bias=None):
    """nn.Linear onto a vocabulary: the padded MFMA path for ragged vocabularies in bf16 mode, else `linear`"""
    if compute_dtype() == torch.bfloat16 and x.dtype == torch.bfloat16 and weight.shape[0] % VOCAB_PAD != 0:
        return VocabLinearFn.apply(x, weight, bias)
    return linear(x, weight, bias)


class VocabCrossEntropyFn(torch.autograd.Function):
    """loss = CrossEntropy(x W^T + b, labels; ignore_index) in ONE autograd node: the IAOG head
    (mm_modeling.py:662 logits -> run_pretraining_fcmf.py:322-324 loss).  The [rows, V] logits live only inside the
    node, in _vocab_logits' column-padded buffer (64001 -> 64032 columns); the loss kernel reads it with
    its row stride, the logit gradient overwrites it IN PLACE and feeds the dX / dW GEMMs directly -- no compaction
    copy to the reference's [B, Ld, V] shape, no padded re-copy and no zero-filled gradient buffer in the backward."""

    @staticmethod
    def forward(ctx, x, weight, bias, labels, ignore_index):
        x2 = _rows(x)
        V = weight.shape[0]
        logits, ctx.w = _vocab_logits(x2, weight, bias)
        M, Vp = logits.shape
        lb = labels.reshape(-1).contiguous()
        rows = torch.empty(M, dtype=torch.float32, device=x2.device)
        nvalid = torch.zeros(1, dtype=torch.float32, device=x2.device)
        H.check(H.lib().fcmf_xent_fwd(H.ptr(logits), Vp, H.ptr(lb), H.ptr(rows), H.ptr(nvalid), M, V, ignore_index,
                                      H.dt(logits), H.stream()), "fcmf_xent_fwd")
        ctx.save_for_backward(x2, weight, logits, lb, nvalid)
        ctx.cfg = (ignore_index, bias is not None, x.shape)
        return rows.sum() / nvalid[0]

    @staticmethod
    def backward(ctx, g):
        x2, weight, logits, lb, nvalid = ctx.saved_tensors
        ignore_index, has_bias, xshape = ctx.cfg
        need = ctx.needs_input_grad
        V, K = weight.shape
        M, Vp = logits.shape
        scale = (g.float() / nvalid[0]).reshape(1).contiguous()
        d = logits                                          # in place: the node owns the buffer
        H.check(H.lib().fcmf_xent_bwd(H.ptr(logits), Vp, H.ptr(lb), H.ptr(d), Vp, H.ptr(scale), 1.0, M, V, ignore_index,
                                      H.dt(logits), H.stream()), "fcmf_xent_bwd")
        if Vp != V:
            d[:, V:].zero_()                                # the padding logits (= bias 0) must not leak into dX / dW
        # the tied vocabulary matrix: its arena slice has zeroed slack rows up to Vp (dp.GradArena pad_rows), so the padded product
        # accumulates straight into it -- no 196 MB zero fill, and the embedding lookup's gradient (the other producer of the tied
        # matrix) adds to the same memory in place instead of through a 196 MB autograd add
        dwp, dw = grad_dest(weight, (V, K), rows=Vp, device=x2.device) if need[1] else (None, None)
        dx, db = _vocab_bwd(d, x2, ctx.w, V, need[0], has_bias and need[2], dwp)
        return None if dx is None else dx.view(xshape), dw, db, None, None


class VocabCrossEntropyExFn(torch.autograd.Function):
    """VocabCrossEntropyFn with label smoothing and / or class weights over the V real columns of the padded logits
    (fcmf_xent_fwd_ex + fcmf_xent_reduce_ex; fcmf_xent_bwd_ex in place): the rows, their weighted mean and the backward's scale
    stay on the device, with no torch arithmetic between the launches"""

    @staticmethod
    def forward(ctx, x, weight, bias, labels, ignore_index, eps, class_weight):
        x2 = _rows(x)
        V = weight.shape[0]
        cw, _ = _loss_weight(class_weight, V, 1, x2.device, "vocab_cross_entropy: class_weight")
        logits, ctx.w = _vocab_logits(x2, weight, bias)
        M, Vp = logits.shape
        lb = labels.reshape(-1).contiguous()
        rows = torch.empty((2, M), dtype=torch.float32, device=x2.device)
        out = torch.empty(2, dtype=torch.float32, device=x2.device)          # [loss, 1 / sum of the live rows' weights]
        L = H.lib()
        H.check(L.fcmf_xent_fwd_ex(H.ptr(logits), Vp, H.ptr(lb), H.ptr(cw), 0, H.ptr(rows[0]), H.ptr(rows[1]), M, V, 1, ignore_index,
                                   eps, 0.0, H.dt(logits), H.stream()), "fcmf_xent_fwd_ex")
        H.check(L.fcmf_xent_reduce_ex(H.ptr(rows[0]), H.ptr(rows[1]), M, 1, 1.0, H.ptr(out), H.ptr(out[1:]), H.stream()),
                "fcmf_xent_reduce_ex")
        ctx.save_for_backward(x2, weight, logits, lb, out, *(() if cw is None else (cw,)))
        ctx.cfg = (ignore_index, bias is not None, x.shape, eps)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        x2, weight, logits, lb, out = ctx.saved_tensors[:5]
        cw = ctx.saved_tensors[5] if len(ctx.saved_tensors) > 5 else None
        ignore_index, has_bias, xshape, eps = ctx.cfg
        need = ctx.needs_input_grad
        V, K = weight.shape
        M, Vp = logits.shape
        g = _grad_scalar(g)
        d = logits                                          # in place: the node owns the buffer
        H.check(H.lib().fcmf_xent_bwd_ex(H.ptr(logits), Vp, H.ptr(lb), H.ptr(cw), 0, H.ptr(d), Vp, H.ptr(out[1:]), H.ptr(g), M, V, 1,
                                         ignore_index, eps, 0.0, H.dt(logits), H.stream()), "fcmf_xent_bwd_ex")
        if Vp != V:
            d[:, V:].zero_()                                # the padding logits (= bias 0) must not leak into dX / dW
        dwp, dw = grad_dest(weight, (V, K), rows=Vp, device=x2.device) if need[1] else (None, None)
        dx, db = _vocab_bwd(d, x2, ctx.w, V, need[0], has_bias and need[2], dwp)
        return None if dx is None else dx.view(xshape), dw, db, None, None, None, None


class VocabCrossEntropyRDropFn(torch.autograd.Function):
    """R-Drop on the vocabulary head in ONE node that owns the padded logits [2M, Vp] of the two stacked passes (rows [0, M) and
    [M, 2M) pair up): loss = CE over all 2M rows with the labels repeated (fcmf_xent_fwd_ex + fcmf_xent_reduce_ex, so label
    smoothing and class weights apply) + alpha x the live pairs' mean symmetric KL (fcmf_symkl_fwd + the same reduce).
    Backward: the CE gradient OUT OF PLACE into a second [2M, Vp] buffer (the pair kernel still needs the logits),
    fcmf_symkl_bwd(acc=1) on top of it, padding columns zeroed, then _vocab_bwd."""

    @staticmethod
    def forward(ctx, x, weight, bias, labels, ignore_index, eps, class_weight, alpha):
        x2 = _rows(x)
        V = weight.shape[0]
        lb = labels.reshape(-1).contiguous()
        M = lb.numel()
        if x2.shape[0] != 2 * M:
            raise H.HipLibraryError(f"vocab_cross_entropy: rdrop_alpha > 0 takes the two passes stacked, 2 x {M} rows for {M} labels; "
                                    f"got {x2.shape[0]} rows")
        cw, _ = _loss_weight(class_weight, V, 1, x2.device, "vocab_cross_entropy: class_weight")
        logits, ctx.w = _vocab_logits(x2, weight, bias)
        Vp = logits.shape[1]
        lb2 = torch.cat((lb, lb))
        rows = torch.empty((4, 2 * M), dtype=torch.float32, device=x2.device)     # CE num, den [2M]; KL num, den [M]
        out = torch.empty(4, dtype=torch.float32, device=x2.device)               # [CE, 1 / D, KL term, alpha / N]
        L = H.lib()
        H.check(L.fcmf_xent_fwd_ex(H.ptr(logits), Vp, H.ptr(lb2), H.ptr(cw), 0, H.ptr(rows[0]), H.ptr(rows[1]), 2 * M, V, 1,
                                   ignore_index, eps, 0.0, H.dt(logits), H.stream()), "fcmf_xent_fwd_ex")
        H.check(L.fcmf_xent_reduce_ex(H.ptr(rows[0]), H.ptr(rows[1]), 2 * M, 1, 1.0, H.ptr(out), H.ptr(out[1:]), H.stream()),
                "fcmf_xent_reduce_ex")
        H.check(L.fcmf_symkl_fwd(H.ptr(logits), Vp, H.ptr(logits[M:]), Vp, H.ptr(lb), H.ptr(rows[2]), H.ptr(rows[3]), M, V, 1,
                                 ignore_index, H.dt(logits), H.stream()), "fcmf_symkl_fwd")
        H.check(L.fcmf_xent_reduce_ex(H.ptr(rows[2]), H.ptr(rows[3]), M, 1, alpha, H.ptr(out[2:]), H.ptr(out[3:]), H.stream()),
                "fcmf_xent_reduce_ex")
        ctx.save_for_backward(x2, weight, logits, lb2, out, *(() if cw is None else (cw,)))
        ctx.cfg = (ignore_index, bias is not None, x.shape, eps)
        return out[0] + out[2]

    @staticmethod
    def backward(ctx, g):
        x2, weight, logits, lb2, out = ctx.saved_tensors[:5]
        cw = ctx.saved_tensors[5] if len(ctx.saved_tensors) > 5 else None
        ignore_index, has_bias, xshape, eps = ctx.cfg
        need = ctx.needs_input_grad
        V, K = weight.shape
        M2, Vp = logits.shape
        M = M2 // 2
        g = _grad_scalar(g)
        d = torch.empty_like(logits)
        L = H.lib()
        H.check(L.fcmf_xent_bwd_ex(H.ptr(logits), Vp, H.ptr(lb2), H.ptr(cw), 0, H.ptr(d), Vp, H.ptr(out[1:]), H.ptr(g), M2, V, 1,
                                   ignore_index, eps, 0.0, H.dt(logits), H.stream()), "fcmf_xent_bwd_ex")
        H.check(L.fcmf_symkl_bwd(H.ptr(logits), Vp, H.ptr(logits[M:]), Vp, H.ptr(lb2), H.ptr(d), Vp, H.ptr(d[M:]), Vp, H.ptr(out[3:]),
                                 H.ptr(g), M, V, 1, ignore_index, 1, H.dt(logits), H.stream()), "fcmf_symkl_bwd")
        if Vp != V:
            d[:, V:].zero_()                                # the padding logits (= bias 0) must not leak into dX / dW
        dwp, dw = grad_dest(weight, (V, K), rows=Vp, device=x2.device) if need[1] else (None, None)
        dx, db = _vocab_bwd(d, x2, ctx.w, V, need[0], has_bias and need[2], dwp)
        return None if dx is None else dx.view(xshape), dw, db, None, None, None, None, None


def vocab_cross_entropy(x, weight, bias, labels, ignore_index=-100, *, label_smoothing=0.0, class_weight=None, rdrop_alpha=0.0):
    """mean CE of the vocabulary projection of x over the non-ignored positions (torch CrossEntropyLoss semantics, its
    `label_smoothing` and `weight` (here class_weight, float32 [V] on the device) included).  Without either it is the plain node.
    rdrop_alpha > 0: x holds two passes of the same positions stacked along its first axis (rows [0, M) and [M, 2M) of the
    flattened x pair up; `labels` has M entries) and the result is the CE over all 2M rows (= the mean of the two passes' CE) +
    rdrop_alpha x the mean over the live positions of the pairs' symmetric KL (VocabCrossEntropyRDropFn)."""
    eps, _ = check_loss_options(label_smoothing, 0.0)
    alpha = check_rdrop_alpha(rdrop_alpha, "rdrop_alpha")
    if alpha > 0.0:
        return VocabCrossEntropyRDropFn.apply(x, weight, bias, labels, int(ignore_index), eps, class_weight, alpha)
    if eps == 0.0 and class_weight is None:
        return VocabCrossEntropyFn.apply(x, weight, bias, labels, int(ignore_index))
    return VocabCrossEntropyExFn.apply(x, weight, bias, labels, int(ignore_index), eps, class_weight)


def logsoftmax_topk(logits, V, k):
    """logits [n, >= V] (unit inner stride, any row stride; columns >= V are never read) -> (log-probabilities float32 [n, k], column
    indices int32 [n, k]) of the k largest entries of every row's first V columns, by value descending, the lower column first
    among equals: log_softmax + topk in one launch (fcmf_logsoftmax_topk, include/fcmf_hip.h)"""
    H.require_cuda(logits)
    if logits.dim() != 2 or logits.stride(1) != 1 or logits.shape[1] < V:
        raise H.HipLibraryError(f"logsoftmax_topk: want [n, >= {V}] rows with unit inner stride, got {tuple(logits.shape)} / {logits.stride()}")
    n = logits.shape[0]
    ld = logits.stride(0) if n > 1 else max(logits.stride(0), V)      # (one row: its stride means nothing)
    if ld < V:
        raise H.HipLibraryError(f"logsoftmax_topk: rows overlap (row stride {ld} < {V} columns)")
    logp = torch.empty((n, k), dtype=torch.float32, device=logits.device)
    ids = torch.empty((n, k), dtype=torch.int32, device=logits.device)
    if n == 0:
        return logp, ids
    H.check(H.lib().fcmf_logsoftmax_topk(H.ptr(logits), ld, n, V, k, H.ptr(logp), H.ptr(ids), H.dt(logits),
                                         H.stream()), "fcmf_logsoftmax_topk")
    return logp, ids


CONSTRAIN_MAX_T = 512      # fcmf_logits_constrain's limit on the sequence length (include/fcmf_hip.h)
CONSTRAIN_MAX_BAN = 1024   # ... and on the number of suppressed ids


def check_constraints(repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0, suppress_tokens=()):
    """the value limits of fcmf_logits_constrain (include/fcmf_hip.h), raised as a ValueError that names the argument"""
    if not (isinstance(repetition_penalty, (int, float)) and math.isfinite(repetition_penalty) and repetition_penalty > 0):
        raise ValueError(f"repetition_penalty must be finite and > 0 (1 = off), got {repetition_penalty}")
    for name, v in (("no_repeat_ngram_size", no_repeat_ngram_size), ("min_length", min_length)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 0:
            raise ValueError(f"{name} must be an integer >= 0 (0 = off), got {v}")
    ids = list(suppress_tokens)
    if any(isinstance(v, bool) or not isinstance(v, int) or not 0 <= v < 2 ** 31 for v in ids):
        raise ValueError(f"suppress_tokens must be token ids (integers >= 0), got {ids}")
    if len(ids) > CONSTRAIN_MAX_BAN:
        raise ValueError(f"suppress_tokens holds {len(ids)} ids, the kernel takes at most {CONSTRAIN_MAX_BAN}")


def logits_constrain(logits, V, hist, repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0, sep_id=-1, ban_ids=None):
    """edits the first V columns of logits [n, >= V] (unit inner stride, any row stride) IN PLACE, before `logsoftmax_topk` /
    `sample_token`: repetition penalty once per distinct token of the row's sequence, -inf on every token that would complete an
    n-gram the sequence already holds, on sep_id while the sequence is shorter than min_length, and on ban_ids (int32 on the
    device, or None).  hist int64 [n, L] (any strides), L <= CONSTRAIN_MAX_T: row r's sequence, the start token first.  Ids outside
    [0, V) write nothing.  One launch, none when nothing is on (fcmf_logits_constrain, include/fcmf_hip.h).  Returns nothing."""
    H.require_cuda(logits, hist, ban_ids)
    check_constraints(repetition_penalty, no_repeat_ngram_size, min_length)
    if logits.dim() != 2 or logits.stride(1) != 1 or logits.shape[1] < V:
        raise H.HipLibraryError(f"logits_constrain: want [n, >= {V}] rows with unit inner stride, got {tuple(logits.shape)} / {logits.stride()}")
    n = logits.shape[0]
    ld = logits.stride(0) if n > 1 else max(logits.stride(0), V)      # (one row: its stride means nothing)
    if ld < V:
        raise H.HipLibraryError(f"logits_constrain: rows overlap (row stride {ld} < {V} columns)")
    if hist.dtype != torch.int64 or hist.dim() != 2 or hist.shape[0] != n or hist.shape[1] < 1:
        raise H.HipLibraryError(f"logits_constrain: want an int64 history [{n}, L >= 1], got {hist.dtype} {tuple(hist.shape)}")
    if hist.shape[1] > CONSTRAIN_MAX_T:
        raise H.HipLibraryError(f"logits_constrain: a sequence of {hist.shape[1]} tokens is beyond the kernel's {CONSTRAIN_MAX_T}")
    n_ban = 0
    if ban_ids is not None:
        if ban_ids.dtype != torch.int32 or ban_ids.dim() != 1 or ban_ids.shape[0] > CONSTRAIN_MAX_BAN:
            raise H.HipLibraryError(f"logits_constrain: want at most {CONSTRAIN_MAX_BAN} int32 ban_ids, got {ban_ids.dtype} {tuple(ban_ids.shape)}")
        ban_ids = ban_ids.contiguous()
        n_ban = ban_ids.shape[0]
    if n == 0:
        return
    H.check(H.lib().fcmf_logits_constrain(H.ptr(logits), ld, n, V, H.ptr(hist), hist.stride(0), hist.stride(1), hist.shape[1],
                                          float(repetition_penalty), int(no_repeat_ngram_size), int(min_length), int(sep_id),
                                          H.ptr(ban_ids) if n_ban else None, n_ban, H.dt(logits), H.stream()), "fcmf_logits_constrain")


@torch.no_grad()
def vocab_topk(x, weight, bias, k, constraints=None):
    """the k most probable tokens of every row of x [n, K] under softmax(x W^T + b), weight [V, K] -> (log-probabilities float32
    [n, k], token ids int32 [n, k]).  No autograd: the decode step.  The projection is _vocab_logits', its padded bias cached on the
    Parameter, and the kernel reads the [n, Vp] buffer with its row stride -- no compaction copy to [n, V], no log-softmax round trip.
    constraints: `logits_constrain`'s keyword arguments as a dict (hist, repetition_penalty, no_repeat_ngram_size, min_length, sep_id,
    ban_ids), applied to the [n, Vp] buffer before the tail: the log-probabilities are those of the constrained logits."""
    logits = _vocab_logits(_rows(x), weight, bias, cache_bias=True)[0]
    if constraints is not None:
        logits_constrain(logits, weight.shape[0], **constraints)
    return logsoftmax_topk(logits, weight.shape[0], k)


def check_sampler(temperature=1.0, top_k=0, top_p=1.0):
    """the value limits of fcmf_sample_token (include/fcmf_hip.h), raised as a ValueError that names the argument"""
    if not (math.isfinite(temperature) and temperature > 0):
        raise ValueError(f"temperature must be finite and > 0, got {temperature}")
    if int(top_k) != top_k or top_k < 0:
        raise ValueError(f"top_k must be an integer >= 0 (0 = off), got {top_k}")
    if not 0 < top_p <= 1:
        raise ValueError(f"top_p must be in (0, 1] (1 = off), got {top_p}")


def sample_token(logits, V, ctr, seed, temperature=1.0, top_k=0, top_p=1.0):
    """logits [n, >= V] (unit inner stride, any row stride; columns >= V are never read), ctr int64 [n] on the device -> (token ids
    int32 [n], log-probabilities float32 [n]): one token per row drawn from softmax(logits / temperature) restricted to the top_k
    largest entries (0 = off; ties kept) and then to the nucleus of mass top_p (1 = off), by Gumbel-max over the counter-based hash
    of (seed, ctr[r], column); the log-probability is the drawn token's under the unfiltered distribution at temperature 1.  One
    launch (fcmf_sample_token, include/fcmf_hip.h)"""
    H.require_cuda(logits, ctr)
    check_sampler(temperature, top_k, top_p)
    if logits.dim() != 2 or logits.stride(1) != 1 or logits.shape[1] < V:
        raise H.HipLibraryError(f"sample_token: want [n, >= {V}] rows with unit inner stride, got {tuple(logits.shape)} / {logits.stride()}")
    n = logits.shape[0]
    ld = logits.stride(0) if n > 1 else max(logits.stride(0), V)      # (one row: its stride means nothing)
    if ld < V:
        raise H.HipLibraryError(f"sample_token: rows overlap (row stride {ld} < {V} columns)")
    if ctr.dtype != torch.int64 or ctr.shape != (n,):
        raise H.HipLibraryError(f"sample_token: want one int64 counter per row, got {ctr.dtype} {tuple(ctr.shape)}")
    ctr = ctr.contiguous()
    ids = torch.empty((n,), dtype=torch.int32, device=logits.device)
    logp = torch.empty((n,), dtype=torch.float32, device=logits.device)
    if n == 0:
        return ids, logp
    H.check(H.lib().fcmf_sample_token(H.ptr(logits), ld, n, V, float(temperature), int(top_k), float(top_p),
                                      int(seed) & 0xFFFFFFFFFFFFFFFF, H.ptr(ctr), H.ptr(ids), H.ptr(logp), H.dt(logits),
                                      H.stream()), "fcmf_sample_token")
    return ids, logp


@torch.no_grad()
def vocab_sample(x, weight, bias, ctr, seed, temperature=1.0, top_k=0, top_p=1.0, constraints=None):
    """one sampled token for every row of x [n, K] under softmax(x W^T + b), weight [V, K] -> (token ids int32 [n], log-probabilities
    float32 [n]) (`sample_token`).  No autograd: the sampling decode step, on the projection and the [n, Vp] buffer of `vocab_topk`;
    constraints as there: the draw and its log-probability are those of the constrained logits."""
    logits = _vocab_logits(_rows(x), weight, bias, cache_bias=True)[0]
    if constraints is not None:
        logits_constrain(logits, weight.shape[0], **constraints)
    return sample_token(logits, weight.shape[0], ctr, seed, temperature, top_k, top_p)


DECODE_ATTN_MAX_T = 512    # fcmf_attn_decode's limit on the number of keys (include/fcmf_hip.h)


@torch.no_grad()
def decode_attention(q, keys, idx, heads, T, live, pos_dim=0, k_new=None, append_at=None, scale=None):
    """one query row per sequence against keys read through an index (fcmf_attn_decode, include/fcmf_hip.h): values are the keys,
    plain slot -> head pairing, scores of the positions live .. T-1 filled with -1e4.  No autograd: the decode step.
    q [n, heads*d] (unit inner stride, any row stride); keys 3-D with heads*d innermost, `pos_dim` (0 or 1) its position axis and
    the other leading axis the indexed one: a cache [Tmax, rows, heads*d] with idx int64 [n, >= T] (the ancestor table; any
    strides), or hoisted encoder keys [samples, Tk, heads*d] (pos_dim=1) with idx int64 [n] (the sample of every row).
    k_new [n, heads*d] with append_at: row r's own key at that position, also stored to the cache row r.  -> out [n, heads*d]"""
    H.require_cuda(q, keys, idx, k_new)
    n, HD = q.shape
    d = HD // heads
    ok = (q.dim() == 2 and keys.dim() == 3 and pos_dim in (0, 1) and keys.shape[2] == HD == heads * d and keys.dtype == q.dtype and
          q.stride(1) == 1 and keys.stride(2) == 1 and 1 <= T <= keys.shape[pos_dim] and idx.dtype == torch.int64 and idx.shape[0] == n and
          (idx.dim() == 1 or (idx.dim() == 2 and (idx.shape[1] >= T or (k_new is not None and idx.shape[1] >= T - 1 == append_at)))))
    if k_new is not None:
        ok = ok and k_new.shape == q.shape and k_new.dtype == q.dtype and k_new.stride(1) == 1 and append_at is not None
    if not ok:
        raise H.HipLibraryError(f"decode_attention: q {tuple(q.shape)} {q.dtype}, keys {tuple(keys.shape)} {keys.dtype} (positions on axis "
                                f"{pos_dim}), idx {tuple(idx.shape)} {idx.dtype}, T {T}, append_at {append_at} do not fit together")
    out = torch.empty((n, HD), dtype=q.dtype, device=q.device)
    if n == 0:
        return out
    idx_sp = idx.stride(1) if idx.dim() == 2 else 0
    H.check(H.lib().fcmf_attn_decode(H.ptr(q), q.stride(0), H.ptr(keys), keys.stride(pos_dim), keys.stride(1 - pos_dim),
                                     H.ptr(idx) if idx.numel() else None, idx.stride(0), idx_sp, keys.shape[1 - pos_dim],
                                     H.ptr(k_new), 0 if k_new is None else k_new.stride(0), int(append_at or 0), H.ptr(out), HD,
                                     n, heads, d, T, live, 1.0 / math.sqrt(d) if scale is None else float(scale), H.dt(q),
                                     H.stream()), "fcmf_attn_decode")
    return out


ADVANCE_MAX_W = 8          # fcmf_beam_advance / fcmf_chain_advance: beams or chains per sample (include/fcmf_hip.h)
ADVANCE_MAX_T = 512        # ... and max_len + 1, the limit of the constraint and decode-attention kernels
SLOT_EMPTY, SLOT_LIVE, SLOT_ENDED = 0, 1, 2


def check_advance(width, max_len, what="beam_size"):
    """the limits of fcmf_beam_advance / fcmf_chain_advance (include/fcmf_hip.h), raised as a ValueError that names the argument"""
    if isinstance(width, bool) or not isinstance(width, int) or not 1 <= width <= ADVANCE_MAX_W:
        raise ValueError(f"{what} must be an integer in 1 .. {ADVANCE_MAX_W} for the device loop, got {width}")
    if isinstance(max_len, bool) or not isinstance(max_len, int) or not 1 <= max_len < ADVANCE_MAX_T:
        raise ValueError(f"max_len must be an integer in 1 .. {ADVANCE_MAX_T - 1} for the device loop, got {max_len}")


def advance_state(num_samples, width, max_len, start_id, device, chains=False):
    """the device-resident state of a decode call as fcmf_beam_advance / fcmf_chain_advance define it (include/fcmf_hip.h), a dict:
    seq int64 [max_len + 1, R] and anc int64 [max_len, R] (position-major), score float64 [R], state int32 [R], done int32 [B] and
    -- beams -- the finished lists fin_score / fin_len / fin_seq / fin_count, or -- chains -- len int32 [R].  R = num_samples * width.
    Beams start with slot 0 of every sample live and the rest empty, chains all live; every slot holds the start token.  No
    host-to-device copy: fills only."""
    check_advance(width, max_len, "num_chains" if chains else "beam_size")
    B, W, S = int(num_samples), int(width), int(max_len) + 1
    R = B * W
    st = dict(B=B, W=W, max_len=int(max_len),
              seq=torch.full((S, R), int(start_id), dtype=torch.int64, device=device),
              anc=torch.zeros((S - 1, R), dtype=torch.int64, device=device),
              score=torch.zeros((R,), dtype=torch.float64, device=device),
              done=torch.zeros((B,), dtype=torch.int32, device=device))
    if chains:
        st["state"] = torch.full((R,), SLOT_LIVE, dtype=torch.int32, device=device)
        st["len"] = torch.ones((R,), dtype=torch.int32, device=device)
    else:
        st["state"] = torch.zeros((B, W), dtype=torch.int32, device=device)
        st["state"][:, 0] = SLOT_LIVE
        st["state"] = st["state"].view(R)
        cap = W * S
        st["fin_score"] = torch.zeros((B, cap), dtype=torch.float64, device=device)
        st["fin_len"] = torch.zeros((B, cap), dtype=torch.int32, device=device)
        st["fin_seq"] = torch.zeros((B, cap, S), dtype=torch.int64, device=device)
        st["fin_count"] = torch.zeros((B,), dtype=torch.int32, device=device)
    return st


def _advance_inputs(name, logp, ids, st, t, shape):
    H.require_cuda(logp, ids, st["seq"])
    if logp.dtype != torch.float32 or ids.dtype != torch.int32 or tuple(logp.shape) != shape or tuple(ids.shape) != shape:
        raise H.HipLibraryError(f"{name}: want float32 log-probabilities and int32 ids of shape {shape}, got {logp.dtype} "
                                f"{tuple(logp.shape)} / {ids.dtype} {tuple(ids.shape)}")
    if not 0 <= t < st["max_len"]:
        raise H.HipLibraryError(f"{name}: round {t} is outside a state of {st['max_len']} rounds")


@torch.no_grad()
def beam_advance(logp, ids, st, t, sep_id):
    """round t of the beam search on the device, in place on `st` (= advance_state(...)): logp float32 / ids int32 [R, k >= W], the
    step's `logsoftmax_topk` outputs on st["seq"][t].  `decoding._advance` and the finishing rules of `decoding.beam_rounds` for
    every sample that is not done, float64 scores, stable ties.  One launch, no host read (fcmf_beam_advance, include/fcmf_hip.h)."""
    B, W = st["B"], st["W"]
    if logp.dim() != 2 or logp.shape[1] < W:
        raise H.HipLibraryError(f"beam_advance: want [{B * W}, >= {W}] step outputs, got {tuple(logp.shape)}")
    _advance_inputs("beam_advance", logp, ids, st, t, (B * W, logp.shape[1]))
    logp, ids = logp.contiguous(), ids.contiguous()
    H.check(H.lib().fcmf_beam_advance(H.ptr(logp), H.ptr(ids), logp.shape[1], B, W, int(t), st["max_len"], int(sep_id),
                                      H.ptr(st["seq"]), H.ptr(st["anc"]), H.ptr(st["score"]), H.ptr(st["state"]),
                                      H.ptr(st["fin_score"]), H.ptr(st["fin_seq"]), H.ptr(st["fin_len"]), H.ptr(st["fin_count"]),
                                      H.ptr(st["done"]), H.stream()), "fcmf_beam_advance")


@torch.no_grad()
def chain_advance(logp, ids, st, t, sep_id):
    """round t of the sampling chains on the device, in place on `st` (= advance_state(..., chains=True)): logp float32 / ids int32
    [R] (or [R, 1]), the step's `sample_token` outputs on st["seq"][t].  One launch, no host read (fcmf_chain_advance)."""
    B, W = st["B"], st["W"]
    logp, ids = logp.reshape(-1), ids.reshape(-1)
    _advance_inputs("chain_advance", logp, ids, st, t, (B * W,))
    H.check(H.lib().fcmf_chain_advance(H.ptr(logp), H.ptr(ids), B, W, int(t), st["max_len"], int(sep_id), H.ptr(st["seq"]),
                                       H.ptr(st["anc"]), H.ptr(st["score"]), H.ptr(st["state"]), H.ptr(st["len"]), H.ptr(st["done"]),
                                       H.stream()), "fcmf_chain_advance")


class FFNFn(torch.autograd.Function):
    """y = gelu_erf(x W1^T + b1) W2^T + b2   (BertIntermediate + BertOutput.dense,
    mm_modeling.py:305-314,320; decoder PositionWiseFFN :558-565).  GELU is the epilogue of the
    first GEMM; in the backward gelu' is the epilogue of the dA GEMM."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2):
        x2 = _rows(x)
        c1, c2 = as_compute(w1, x2.dtype), as_compute(w2, x2.dtype)
        M = x2.shape[0]
        u = torch.empty((M, w1.shape[0]), dtype=x2.dtype, device=x2.device)
        a = _linear_fwd(x2, c1, b1.detach(), H.EPI_GELU, aux=u, master=w1)
        y = _linear_fwd(a, c2, b2.detach(), master=w2)
        ctx.save_for_backward(x2, w1, w2, u, a)
        ctx.xshape = x.shape
        return y.view(*x.shape[:-1], w2.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2, w1, w2, u, a = ctx.saved_tensors
        dy2 = dy.reshape(-1, dy.shape[-1]).contiguous()
        c1, c2 = as_compute(w1, x2.dtype), as_compute(w2, x2.dtype)
        du, dw2, db2 = _linear_bwd(a, c2, dy2, True, True, True, dx_epi=H.EPI_DGELU, dx_aux=u, master=w2)
        dx, dw1, db1 = _linear_bwd(x2, c1, du, ctx.needs_input_grad[0], True, True, master=w1)
        return (None if dx is None else dx.view(ctx.xshape)), dw1, db1, dw2, db2


def ffn(x, w1, b1, w2, b2):
    return FFNFn.apply(x, w1, b1, w2, b2)


# --------------------------------------------------------------------------------------
# residual + dropout + LayerNorm
# --------------------------------------------------------------------------------------
def ln_fwd(x, res, res_ld, gamma, beta, eps, p, seed, z, quant=False):
    """y = LN(z), z = dropout(x; p, seed) + res, x [rows, H] dense, res rows at stride res_ld (or None, 0) -> (y, mean, rstd, yq).
    z: the tensor that receives the pre-LN sum the backward needs (x itself: in place).  quant: the kernel also emits
    yq = (e4m3 y, row scales), what the fp8 GEMM that consumes y would otherwise quantise in a pass of its own; else yq is None"""
    rows, Hd = x.shape
    y = torch.empty_like(x)
    mean, rstd = (torch.empty(rows, dtype=torch.float32, device=x.device) for _ in range(2))
    name, yq = ("fcmf_add_ln_fwd_fp8", _fp8_buffers(rows, Hd, x.device)) if quant else ("fcmf_add_ln_fwd", None)
    H.check(getattr(H.lib(), name)(H.ptr(x), H.ptr(res), res_ld, H.ptr(gamma), H.ptr(beta), H.ptr(y), H.ptr(z), H.ptr(mean),
                                   H.ptr(rstd), rows, Hd, eps, p, seed, H.dt(x), *map(H.ptr, yq or ()), H.stream()), name)
    return y, mean, rstd, yq


def ln_bwd(dy, z, gamma, mean, rstd, p, seed, dg, db, dxsum=None, quant=False):
    """backward of ln_fwd -> (dz: the gradient of the sum = of the residual, dx: of the dropout's input -- dz itself when p == 0,
    dxq: (e4m3 dx, row scales) when `quant`, else None).  The float32 [H] gradients of gamma and beta are ACCUMULATED into dg and
    db, the column sums of dx (the bias gradient of the Linear that produced x) into dxsum where one is given."""
    rows, Hd = z.shape
    dz = torch.empty_like(z)
    dx = torch.empty_like(z) if p > 0 else None
    L = H.lib()
    # scratch for the per-workgroup partial column sums (stream-ordered reuse is safe: every call fully rewrites the part it reads)
    ws = torch.empty(L.fcmf_add_ln_bwd_workspace(rows, Hd), dtype=torch.float32, device=z.device)
    name, dxq = ("fcmf_add_ln_bwd_fp8", _fp8_buffers(rows, Hd, z.device)) if quant else ("fcmf_add_ln_bwd", None)
    H.check(getattr(L, name)(H.ptr(dy), H.ptr(z), H.ptr(gamma), H.ptr(mean), H.ptr(rstd), H.ptr(dz), H.ptr(dx), H.ptr(dg), H.ptr(db),
                             H.ptr(dxsum), H.ptr(ws), rows, Hd, p, seed, H.dt(z), *map(H.ptr, dxq or ()), H.stream()), name)
    return dz, (dz if dx is None else dx), dxq


class AddLNFn(torch.autograd.Function):
    """LN(dropout(x) + res): BertSelfOutput / BertOutput / AddNorm (mm_modeling.py:276-280,
    324-328, 570-573) with FCMFLayerNorm (:167-171) or nn.LayerNorm (HF, eps 1e-5)."""

    @staticmethod
    def forward(ctx, x, res, gamma, beta, eps, p, seed):
        x2 = _rows(x).contiguous()
        r2 = None if res is None else _rows(res)
        z = torch.empty_like(x2)
        H.require_cuda(x2)
        y, mean, rstd, _ = ln_fwd(x2, r2, 0 if r2 is None else _ld(r2), gamma, beta, eps, p, seed, z)
        ctx.save_for_backward(z, gamma, mean, rstd, beta)
        ctx.p, ctx.seed, ctx.xshape = p, seed, x.shape
        ctx.res_shape = None if res is None else res.shape
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        z, gamma, mean, rstd, beta = ctx.saved_tensors
        dgbuf, dg = grad_dest(gamma, (z.shape[1],))      # the arena slices (already zero) where an arena is active: no fill launches
        dbbuf, db = grad_dest(beta, (z.shape[1],))       # (dg / db = None: a later use of shared parameters, accumulated in place)
        dz, dx, _ = ln_bwd(dy.reshape(z.shape).contiguous(), z, gamma, mean, rstd, ctx.p, ctx.seed, dgbuf, dbbuf)
        return dx.view(ctx.xshape), (None if ctx.res_shape is None else dz.view(ctx.res_shape)), dg, db, None, None, None


def add_layer_norm(x, res, gamma, beta, eps, p=0.0, training=False):
    p = float(p) if training else 0.0
    return AddLNFn.apply(x, res, gamma, beta, float(eps), p, next_seed() if p > 0 else 0)


class DropoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p, seed):
        x2 = x.contiguous()
        y = torch.empty_like(x2)
        H.require_cuda(x2)
        H.check(H.lib().fcmf_dropout(H.ptr(x2), H.ptr(y), x2.numel(), p, seed, H.dt(x2), H.stream()), "fcmf_dropout")
        ctx.p, ctx.seed = p, seed
        return y

    @staticmethod
    def backward(ctx, dy):
        d = dy.contiguous()
        o = torch.empty_like(d)
        H.check(H.lib().fcmf_dropout(H.ptr(d), H.ptr(o), d.numel(), ctx.p, ctx.seed, H.dt(d), H.stream()), "fcmf_dropout")
        return o, None, None


def dropout(x, p, training):
    if not training or p <= 0:
        return x
    return DropoutFn.apply(x, float(p), next_seed())


# --------------------------------------------------------------------------------------
# RoBERTa embeddings
# --------------------------------------------------------------------------------------
def position_ids(input_ids, pad_id):
    """HF create_position_ids_from_input_ids"""
    ids = input_ids.contiguous()
    H.require_cuda(ids)
    pos = torch.empty_like(ids)
    H.check(H.lib().fcmf_position_ids(H.ptr(ids), H.ptr(pos), ids.shape[0], ids.shape[1], pad_id, H.stream()),
            "fcmf_position_ids")
    return pos


class EmbedLNFn(torch.autograd.Function):
    """RobertaEmbeddings: LN(word[ids] + type[tt] + pos[pos]) then dropout"""

    @staticmethod
    def forward(ctx, ids, pos, tt, word, ptab, ttab, gamma, beta, eps, p, seed, pad_id, out_dtype, g=None, scale=None):
        ids, pos = ids.contiguous(), pos.contiguous()
        tt = None if tt is None else tt.contiguous()
        ntok, Hd = ids.numel(), word.shape[1]
        y = torch.empty((ntok, Hd), dtype=out_dtype, device=word.device)
        z = torch.empty_like(y)
        mean = torch.empty(ntok, dtype=torch.float32, device=word.device)
        rstd = torch.empty(ntok, dtype=torch.float32, device=word.device)
        H.require_cuda(ids, word)
        if g is None:
            H.check(H.lib().fcmf_embed_ln_fwd(H.ptr(ids), H.ptr(pos), H.ptr(tt), H.ptr(word), H.ptr(ptab), H.ptr(ttab),
                                              H.ptr(gamma), H.ptr(beta), H.ptr(y), H.ptr(z), H.ptr(mean), H.ptr(rstd),
                                              ntok, Hd, eps, p, seed, H.dt(y), H.stream()), "fcmf_embed_ln_fwd")
        else:      # (EmbedLNAdvFn: the sum plus scale[sequence] * g at the tokens that are not pad)
            H.check(H.lib().fcmf_embed_ln_adv_fwd(H.ptr(ids), H.ptr(pos), H.ptr(tt), H.ptr(word), H.ptr(ptab), H.ptr(ttab),
                                                  H.ptr(gamma), H.ptr(beta), H.ptr(y), H.ptr(z), H.ptr(mean), H.ptr(rstd),
                                                  ntok, Hd, eps, p, seed, H.dt(y), H.stream(), H.ptr(g), H.ptr(scale),
                                                  ids.shape[-1], pad_id), "fcmf_embed_ln_adv_fwd")
        ctx.save_for_backward(ids, pos, tt, z, gamma, mean, rstd)
        ctx.p, ctx.seed, ctx.pad_id = p, seed, pad_id
        ctx.params = (word, ptab, ttab, gamma, beta)       # (the Parameters: grad_dest looks up their arena slices)
        return y.view(*ids.shape, Hd)

    @staticmethod
    def backward(ctx, dy):
        ids, pos, tt, z, gamma, mean, rstd = ctx.saved_tensors
        ntok, Hd = z.shape
        d = dy.reshape(ntok, Hd).contiguous()
        L = H.lib()
        if ctx.p > 0:
            o = torch.empty_like(d)
            H.check(L.fcmf_dropout(H.ptr(d), H.ptr(o), d.numel(), ctx.p, ctx.seed, H.dt(d), H.stream()), "fcmf_dropout")
            d = o
        word, ptab, ttab, gpar, bpar = ctx.params
        # (arena slices: already zero, no fill launches.  Only the word table accumulates in place -- dword = None: the tied
        #  matrix's slice was claimed by the vocabulary projection; the others get a temporary that autograd adds)
        dg, _ = grad_dest(gpar, (Hd,), in_place=False, device=z.device)
        db, _ = grad_dest(bpar, (Hd,), in_place=False, device=z.device)
        dz = ln_bwd(d, z, gamma, mean, rstd, 0.0, 0, dg, db)[0]      # (the dropout, applied AFTER the LayerNorm here, is undone above)
        rec = getattr(ctx, "adv_record", None)
        if rec is not None:      # (EmbeddingAdversary.record: dz IS the gradient w.r.t. the token embeddings; kept, not copied)
            rec[0][rec[1]] = (dz, ids)
        dwordbuf, dword = grad_dest(word, word.shape, device=z.device)
        dpos, _ = grad_dest(ptab, ptab.shape, in_place=False, device=z.device)
        dtt, _ = grad_dest(ttab, ttab.shape, in_place=False, device=z.device)
        two_d = ids.dim() == 2 and pos.is_contiguous()
        fused = False
        if two_d and (tt is None or tt.is_contiguous()):
            # [sequences, S] layout: position rows are shared by the offsets of all sequences; position and type gradients in ONE pass
            rc = L.fcmf_embed_pos_type_bwd(H.ptr(dz), H.ptr(pos), H.ptr(tt), H.ptr(dpos), H.ptr(dtt), ids.shape[0], ids.shape[1], Hd,
                                           ctx.pad_id, H.dt(dz), H.stream())
            fused = rc == 0
            if rc not in (0, H.ERR_UNSUPPORTED):
                H.check(rc, "fcmf_embed_pos_type_bwd")
        H.check(L.fcmf_embed_bwd(H.ptr(dz), H.ptr(ids), H.ptr(pos), H.ptr(tt), H.ptr(dwordbuf), None if two_d else H.ptr(dpos),
                                 None if fused else H.ptr(dtt), ntok, Hd, ctx.pad_id, H.dt(dz), H.stream()), "fcmf_embed_bwd")
        if two_d and not fused:
            H.check(L.fcmf_embed_pos_bwd(H.ptr(dz), H.ptr(pos), H.ptr(dpos), ids.shape[0], ids.shape[1], Hd, ctx.pad_id,
                                         H.dt(dz), H.stream()), "fcmf_embed_pos_bwd")
        return None, None, None, dword, dpos, dtt, dg, db, None, None, None, None, None


class EmbedLNAdvFn(EmbedLNFn):
    """EmbedLNFn on the perturbed sum (EmbeddingAdversary.attack).  g and scale are constants: the backward is EmbedLNFn's"""

    @staticmethod
    def backward(ctx, dy):
        return EmbedLNFn.backward(ctx, dy) + (None, None)


_adversary = None      # the EmbeddingAdversary whose record() or attack() block is running


class EmbeddingAdversary:
    """FGM on the text embeddings (Miyato et al., "Adversarial Training Methods for Semi-Supervised Text Classification"), in two
    passes over the same batch:

        with adv.record():  loss = model(batch)        # clean pass: every embed_layer_norm call registers, in forward order
        loss.backward()                                # ... and its backward deposits (dz, ids): the gradient at the embeddings
        with adv.attack():  loss_adv = model(batch)    # call k adds epsilon * dz_k / ||dz_k|| (per sequence, pad tokens excluded)
        loss_adv.backward()                            # accumulates onto the first pass: the step's gradient is the sum

    Only calls made in training mode, with grad enabled and a word table that requires grad take part; all others run the plain
    kernel in either block.  The perturbation is never materialised: fcmf_adv_scale turns the kept dz into one float per sequence
    and fcmf_embed_ln_adv_fwd reads dz and that scale.  Nothing flows back through either.  The records (one dz per call: the
    cost in memory) are released when attack() exits.  ids of any rank: the last axis is the sequence."""

    def __init__(self, epsilon):
        epsilon = float(epsilon)
        if not (math.isfinite(epsilon) and epsilon >= 0.0):
            raise ValueError(f"the adversary's epsilon must be finite and >= 0, got {epsilon}")
        self.epsilon = epsilon
        self._records, self._mode, self._next = [], None, 0

    def _enter(self, mode):
        global _adversary
        if _adversary is not None:
            raise RuntimeError("an EmbeddingAdversary block is already running: record() and attack() do not nest")
        _adversary, self._mode, self._next = self, mode, 0

    def _leave(self):
        global _adversary
        _adversary, self._mode = None, None

    def record(self):
        return _AdversaryBlock(self, "record")

    def attack(self):
        return _AdversaryBlock(self, "attack")

    def recorded(self):
        """embed_layer_norm calls registered by the last record() and not yet released"""
        return len(self._records)

    def _embed(self, args, takes_part):
        ids, word, pad_id, out_dtype = args[0], args[3], args[11], args[12]
        if not takes_part:
            return EmbedLNFn.apply(*args)
        if self._mode == "record":
            y = EmbedLNFn.apply(*args)
            self._records.append(None)
            y.grad_fn.adv_record = (self._records, len(self._records) - 1)      # (grad_fn is the node's ctx)
            return y
        k, self._next = self._next, self._next + 1
        if k >= len(self._records):
            raise ValueError(f"the adversarial pass makes more embedding calls than the clean pass recorded ({len(self._records)})")
        if self._records[k] is None:
            raise ValueError(f"embedding call {k} of the clean pass has no gradient: run backward() between record() and attack()")
        dz, rids = self._records[k]
        if rids.shape != ids.shape or dz.shape[-1] != word.shape[1] or dz.dtype != out_dtype:
            raise ValueError(f"embedding call {k}: the clean pass saw ids {tuple(rids.shape)} and a {dz.dtype} gradient of width "
                             f"{dz.shape[-1]}, the adversarial pass ids {tuple(ids.shape)}, {out_dtype} and width {word.shape[1]}")
        S = ids.shape[-1]
        nseq = ids.numel() // S if S else 0
        scale = torch.empty(nseq, dtype=torch.float32, device=dz.device)
        H.check(H.lib().fcmf_adv_scale(H.ptr(dz), H.ptr(rids), H.ptr(scale), nseq, S, dz.shape[-1], pad_id, self.epsilon, H.dt(dz),
                                       H.stream()), "fcmf_adv_scale")
        return EmbedLNAdvFn.apply(*args, dz, scale)


class _AdversaryBlock:
    def __init__(self, adv, mode):
        self.adv, self.mode = adv, mode

    def __enter__(self):
        a = self.adv
        if self.mode == "attack" and not a._records:
            raise ValueError("attack() with nothing recorded: the text embeddings must be trainable (a word table that requires "
                             "grad, in training mode, with grad enabled) during record()")
        a._enter(self.mode)
        if self.mode == "record":
            a._records = []      # (a new list: a backward of an older pass still deposits into its own)
        return a

    def __exit__(self, *exc):
        a = self.adv
        a._leave()
        if self.mode == "attack":
            used, n = a._next, len(a._records)
            a._records = []
            if exc[0] is None and used != n:
                raise ValueError(f"the adversarial pass made {used} embedding calls, the clean pass recorded {n}")
        return False


def embed_layer_norm(ids, pos, tt, word, ptab, ttab, gamma, beta, eps, p, training, pad_id, out_dtype):
    p = float(p) if training else 0.0
    if _adversary is not None:
        return _adversary._embed((ids, pos, tt, word, ptab, ttab, gamma, beta, float(eps), p, next_seed() if p > 0 else 0,
                                  int(pad_id), out_dtype), bool(training) and torch.is_grad_enabled() and word.requires_grad)
    return EmbedLNFn.apply(ids, pos, tt, word, ptab, ttab, gamma, beta, float(eps), p, next_seed() if p > 0 else 0,
                           int(pad_id), out_dtype)


# --------------------------------------------------------------------------------------
# attention
# --------------------------------------------------------------------------------------
def _query_rows(q, row0):
    """q [G,R,HD] as the kernels read it in place: unit inner stride, rows that do not overlap.  row0: or ONE row expanded over the
    R rows, row stride 0 (the [CLS] query against every image's keys)"""
    ok = q.stride(2) == 1 and (q.stride(1) >= q.shape[2] or (row0 and q.stride(1) == 0))
    return q if ok else q.contiguous()


def _kv_pair(k, v):
    """K and V of a segment with a unit inner stride and the SAME strides (the descriptor carries K's only)"""
    if k is None:
        return None, None
    k = k if k.stride(-1) == 1 else k.contiguous()
    v = v if v.stride() == k.stride() else v.contiguous()
    if v.stride() != k.stride():
        k = k.contiguous()
    return k, v


def _mfma_dense(a, *operands):
    """attn.mfma_eligible for operands that are tensors of their own: the MFMA kernels take one row stride per operand, so q / k1
    / v1 must be dense -- which keeps a stride-0 expanded query row, and any row-strided view, on the VALU kernel"""
    return attn.mfma_eligible(a) and all(t.is_contiguous() for t in operands)


class AttentionFn(torch.autograd.Function):
    """Two-segment multi-head attention (see fcmf_attn_desc in include/fcmf_hip.h).
      q  [G,R,heads*d]; k1/v1 [G,T1,heads*d] shared by the R rows of a group;
      k2/v2 [G/group_div,R,T2,heads*d] private per row; mask [G,T1+T2] additive float32;
      bias [G/group_div,heads,R,T1+T2] additive float32.  Returns [G,R,heads*d]."""

    @staticmethod
    def forward(ctx, q, k1, v1, k2, v2, mask, bias, heads, group_div, scale, p, seed, causal):
        H.require_cuda(q)
        q = _query_rows(q, True)
        k1, v1 = _kv_pair(k1, v1)
        k2, v2 = _kv_pair(k2, v2)
        mask = None if mask is None else mask.contiguous().float()
        bias = None if bias is None else bias.contiguous()
        G, R, HD = q.shape
        out = torch.empty((G, R, HD), dtype=q.dtype, device=q.device)
        lse = torch.empty((G, heads, R), dtype=torch.float32, device=q.device)
        a = attn.desc(q, k1, v1, k2, v2, mask, bias, heads, group_div, scale, p, seed, causal, 0)
        ctx.mfma = _mfma_dense(a, q, k1, v1)
        attn.forward(a, out, lse, ctx.mfma)
        ctx.save_for_backward(q, k1, v1, k2, v2, mask, bias, out, lse)
        ctx.cfg = (heads, group_div, scale, p, seed, causal)
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k1, v1, k2, v2, mask, bias, out, lse = ctx.saved_tensors
        heads, group_div, scale, p, seed, causal = ctx.cfg
        G, R, HD = q.shape
        dout = dout.contiguous()
        a = attn.desc(q, k1, v1, k2, v2, mask, bias, heads, group_div, scale, p, seed, causal, 0)
        if ctx.mfma:
            dq, dk, dv = torch.empty_like(q), torch.empty_like(k1), torch.empty_like(v1)
            attn.mfma_backward(a, out, dout, lse, H.ptr(dq), H.ptr(dk), H.ptr(dv))
            return dq, dk, dv, None, None, None, None, None, None, None, None, None, None
        new = lambda like, *shape: torch.empty(shape, dtype=like.dtype, device=q.device)
        dk1 = dv1 = dk2 = dv2 = dbias = scratch = None
        if k1 is not None:
            dk1, dv1 = new(k1, G, a.T1, HD), new(k1, G, a.T1, HD)
        # private keys shared by `group_div` groups: the library sums their gradients over the group (no per-group rows)
        grouped = k2 is not None and group_div <= 8 and G % group_div == 0
        if k2 is not None:
            G2 = G // group_div if grouped else G
            dk2, dv2 = new(q, G2, R, a.T2, HD), new(q, G2, R, a.T2, HD)
        if bias is not None and ctx.needs_input_grad[6]:
            dbias = torch.empty((G, heads, R, a.T1 + a.T2), dtype=torch.float32, device=q.device)
        if grouped:
            scratch = torch.empty(2 * G * heads * R * a.T2, dtype=torch.float32, device=q.device)
        dq = attn.small_backward(a, out, dout, lse, q, dk1, dv1, dk2, dv2, dbias, scratch)
        if group_div > 1:
            if dk2 is not None and not grouped:
                dk2, dv2 = attn.sum_groups(dk2, group_div), attn.sum_groups(dv2, group_div)
            if dbias is not None:
                dbias = attn.sum_groups(dbias, group_div)
        return dq, dk1, dv1, dk2, dv2, None, dbias, None, None, None, None, None, None


def attention(q, k1=None, v1=None, k2=None, v2=None, mask=None, bias=None, heads=12, group_div=1, scale=None,
              p=0.0, training=False, causal=False):
    d = q.shape[-1] // heads
    scale = 1.0 / math.sqrt(d) if scale is None else scale
    p = float(p) if training else 0.0
    return AttentionFn.apply(q, k1, v1, k2, v2, mask, bias, heads, group_div, float(scale), p,
                             next_seed() if p > 0 else 0, causal)


class SharedKVAttentionFn(torch.autograd.Function):
    """MFMA attention over any number of keys, one key/value set per `kv_share` consecutive query groups
    (fcmf_attn_mfma_long_fwd / _bwd): q [G,Tq,heads*64], k / v [G/kv_share,Tk,heads*64], mask [G,Tk] additive float32."""

    @staticmethod
    def forward(ctx, q, k, v, mask, heads, kv_share, scale, p, seed):
        H.require_cuda(q, k, v)
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        mask = None if mask is None else mask.contiguous().float()
        G, Tq, HD = q.shape
        out = torch.empty_like(q)
        lse = torch.empty((G, heads, Tq), dtype=torch.float32, device=q.device)
        attn.long_forward(q, k, v, mask, out, lse, heads, kv_share, scale, p, seed)
        ctx.save_for_backward(q, k, v, mask, out, lse)
        ctx.cfg = (heads, kv_share, scale, p, seed)
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, mask, out, lse = ctx.saved_tensors
        heads, kv_share, scale, p, seed = ctx.cfg
        dout = dout.contiguous()
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        attn.long_backward(q, k, v, mask, out, dout, lse, dq, dk, dv, heads, kv_share, scale, p, seed)
        return dq, dk, dv, None, None, None, None, None, None


class ChunkedF32AttentionFn(torch.autograd.Function):
    """float32 parity mode of shared_kv_attention for more shared keys than the VALU kernels hold in LDS: the keys go through
    fcmf_attn_small_fwd in chunks, each with its own logsumexp, and the chunk outputs are merged with the weights
    exp(lse_chunk - lse) (a few element-wise torch operations on [chunks, G, heads, Tq]: this mode exists to be compared with,
    not to be fast).  The backward runs fcmf_attn_small_bwd per chunk with the MERGED output and logsumexp, from which the
    kernel recomputes exactly the global probabilities of the chunk's keys.  q may be a strided view (one sharing member).
    Not covered: a group without any live key (its chunks would be weighted equally, not by their sizes)."""

    @staticmethod
    def forward(ctx, q, k, v, mask, heads, scale, p, seed, chunk):
        H.require_cuda(q, k, v)
        q = _query_rows(q, False)
        k, v = k.contiguous(), v.contiguous()
        G, R, HD = q.shape
        T = k.shape[1]
        bounds = [(c, min(c + chunk, T)) for c in range(0, T, chunk)]
        masks = [None if mask is None else mask[:, a:b].contiguous().float() for a, b in bounds]
        outs = torch.empty((len(bounds), G, R, HD), dtype=q.dtype, device=q.device)
        lses = torch.empty((len(bounds), G, heads, R), dtype=torch.float32, device=q.device)
        for i, (a, b) in enumerate(bounds):
            d = attn.desc(q, k[:, a:b], v[:, a:b], None, None, masks[i], None, heads, 1, scale, p, (seed + i) & 0xFFFFFFFFFFFFFFFF, False, 0)
            attn.forward(d, outs[i], lses[i], False)
        lse = torch.logsumexp(lses, 0)
        w = torch.exp(lses - lse).transpose(2, 3).unsqueeze(-1)                       # [chunks, G, R, heads, 1]
        out = (outs.view(len(bounds), G, R, heads, HD // heads) * w).sum(0).view(G, R, HD)
        ctx.save_for_backward(q, k, v, out, lse, *[m for m in masks if m is not None])
        ctx.cfg = (heads, scale, p, seed, bounds, mask is not None)
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse, *masks = ctx.saved_tensors
        heads, scale, p, seed, bounds, has_mask = ctx.cfg
        G, R, HD = q.shape
        dout = dout.contiguous()
        dq = torch.zeros((G, R, HD), dtype=q.dtype, device=q.device)
        dk, dv = torch.empty_like(k), torch.empty_like(v)
        for i, (a, b) in enumerate(bounds):
            d = attn.desc(q, k[:, a:b], v[:, a:b], None, None, masks[i] if has_mask else None, None, heads, 1, scale, p,
                          (seed + i) & 0xFFFFFFFFFFFFFFFF, False, 0)
            dkc, dvc = (torch.empty((G, b - a, HD), dtype=q.dtype, device=q.device) for _ in range(2))
            dq += attn.small_backward(d, out, dout, lse, q, dkc, dvc)
            dk[:, a:b], dv[:, a:b] = dkc, dvc
        return dq, dk, dv, None, None, None, None, None, None


def shared_kv_attention(q, k, v, mask=None, heads=12, kv_share=1, scale=None, p=0.0, training=False):
    """softmax(scale q k^T + mask) v where group g of q [G,Tq,HD] reads key set g // kv_share of k / v [G/kv_share,Tk,HD]
    (the aspect prompts of a review share its visual tokens); mask [G,Tk] additive.  bf16 with head dim 64: the long-key
    MFMA kernel, any Tk.  float32 (the parity mode): the VALU kernels, one `attention` call per sharing member on a
    strided view of q; autograd sums the members' key gradients in float32.  Up to valu_float32_key_limit(d) keys (285 at
    head dim 64: the float32 K / V images of a head must fit in LDS) the keys go in one piece, beyond that in chunks of 256
    merged by their logsumexps (ChunkedF32AttentionFn)."""
    G, Tq, HD = q.shape
    d = HD // heads
    scale = 1.0 / math.sqrt(d) if scale is None else scale
    p = float(p) if training else 0.0
    if (kv_share < 1 or G % kv_share or k.shape != v.shape or k.shape[0] * kv_share != G or k.shape[2] != HD
            or k.dtype != q.dtype or v.dtype != q.dtype or (mask is not None and tuple(mask.shape) != (G, k.shape[1]))):
        raise H.HipLibraryError(f"shared_kv_attention: q {tuple(q.shape)} / k {tuple(k.shape)} / v {tuple(v.shape)} do not "
                                f"form {kv_share} query groups per key set")
    if q.dtype == torch.bfloat16 and d * heads == HD and d == 64:
        return SharedKVAttentionFn.apply(q, k, v, mask, heads, kv_share, float(scale), p, next_seed() if p > 0 else 0)
    if q.dtype == torch.float32 and d <= 128:
        # one call per sharing member on a strided view of q; the keys in one piece while the VALU kernels hold them in LDS,
        # else in chunks of 256 merged by their logsumexps
        seeds = [next_seed() if p > 0 else 0 for _ in range(kv_share)]
        view = lambda m: (q[m::kv_share], k, v, None if mask is None else mask[m::kv_share])
        if k.shape[1] <= valu_float32_key_limit(d):
            outs = [AttentionFn.apply(*view(m)[:3], None, None, view(m)[3], None, heads, 1, float(scale), p, seeds[m], False)
                    for m in range(kv_share)]
        else:
            outs = [ChunkedF32AttentionFn.apply(*view(m), heads, float(scale), p, seeds[m], min(256, valu_float32_key_limit(d)))
                    for m in range(kv_share)]
        return torch.stack(outs, 1).reshape(G, Tq, HD)
    raise H.HipLibraryError(f"shared_kv_attention: unsupported configuration ({q.dtype}, head dim {d}): bf16 with head dim 64, "
                            "or float32 with head dim <= 128")


def shared_kv_attention_probs(q, k, mask=None, heads=12, kv_share=1, scale=None, average_heads=False, out=None):
    """softmax(scale q k^T + mask) of `shared_kv_attention` as float32, before dropout, recomputed from q and k (no values, no
    logsumexp of a forward): [G, heads, Tq, Tk], or with average_heads the mean over the heads [G, Tq, Tk] (what
    torch.nn.MultiheadAttention returns by default).  Operands and refusals as shared_kv_attention.  bf16 with head dim 64:
    fcmf_attn_mfma_long_probs, any Tk; the head mean is formed inside the kernel (float32, ascending head order, every
    element stored once: deterministic, and no per-head tensor exists).  float32 (the parity mode): fcmf_attn_probs once per
    sharing member, up to its 512 keys, the head mean a torch reduction.  Detached; there is no backward.  out: a contiguous
    float32 tensor of the result's shape to fill instead of a new one."""
    H.require_cuda(q, k)
    G, Tq, HD = q.shape
    d = HD // heads
    scale = 1.0 / math.sqrt(d) if scale is None else float(scale)
    if (kv_share < 1 or G % kv_share or k.dim() != 3 or k.shape[0] * kv_share != G or k.shape[2] != HD or k.dtype != q.dtype
            or (mask is not None and tuple(mask.shape) != (G, k.shape[1]))):
        raise H.HipLibraryError(f"shared_kv_attention_probs: q {tuple(q.shape)} / k {tuple(k.shape)} do not form {kv_share} "
                                f"query groups per key set")
    Tk = k.shape[1]
    bf16 = q.dtype == torch.bfloat16 and d * heads == HD and d == 64
    if not bf16 and not (q.dtype == torch.float32 and d * heads == HD and d <= 128):
        raise H.HipLibraryError(f"shared_kv_attention_probs: unsupported configuration ({q.dtype}, head dim {d}): bf16 with "
                                "head dim 64, or float32 with head dim <= 128")
    if not bf16 and Tk > 512:
        raise H.HipLibraryError(f"shared_kv_attention_probs: unsupported configuration (float32 with {Tk} keys: the parity "
                                "mode takes up to 512)")
    shape = (G, Tq, Tk) if average_heads else (G, heads, Tq, Tk)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=q.device)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != q.device:
        raise H.HipLibraryError(f"shared_kv_attention_probs: out must be a contiguous float32 {shape} tensor on {q.device}")
    q, k = q.detach().contiguous(), k.detach().contiguous()
    mask = None if mask is None else mask.detach().contiguous().float()
    if bf16:
        attn.long_probs(q, k, mask, out, heads, kv_share, scale, average_heads)
        return out
    per_head = torch.empty((G, heads, Tq, Tk), dtype=torch.float32, device=q.device) if average_heads or kv_share > 1 else out
    for m in range(kv_share):
        qm = _query_rows(q[m::kv_share], False)
        mm = None if mask is None else mask[m::kv_share].contiguous()
        pm = per_head if kv_share == 1 else torch.empty((G // kv_share, heads, Tq, Tk), dtype=torch.float32, device=q.device)
        a = attn.desc(qm, k, None, None, None, mm, None, heads, 1, scale, 0.0, 0, False, False)
        attn.probs(a, pm, heads * Tq * Tk, Tq * Tk, False)
        if kv_share > 1:
            per_head[m::kv_share] = pm
    if average_heads:
        torch.mean(per_head, 1, out=out)
    elif per_head is not out:
        out.copy_(per_head)
    return out


def attention_probs(q, k1=None, k2=None, mask=None, bias=None, heads=12, group_div=1, scale=None, causal=False,
                    head_quirk=False, slot_major=False, out=None):
    """softmax(score) of `attention` / fcmf_attn_desc as float32, before dropout, recomputed from q and the keys (no values, no
    logsumexp of a forward): [G, heads, R, T1+T2], or with slot_major [heads*G, R, T1+T2] where index h*G + g is output slot h of
    group g (with head_quirk, the order of the reference Attention's `score`, mm_modeling.py:126-132).  Same operand layouts, stride
    normalisation and MFMA / VALU choice as AttentionFn.forward (_query_rows, _mfma_dense over attn.mfma_eligible).  Detached;
    there is no backward.  out: a float32 tensor of that shape to fill instead of a new one."""
    H.require_cuda(q)
    q = _query_rows(q.detach(), True)
    k1 = None if k1 is None else (k1.detach() if k1.stride(2) == 1 else k1.detach().contiguous())
    k2 = None if k2 is None else (k2.detach() if k2.stride(3) == 1 else k2.detach().contiguous())
    mask = None if mask is None else mask.detach().contiguous().float()
    bias = None if bias is None else bias.detach().contiguous()
    G, R, HD = q.shape
    T = (0 if k1 is None else k1.shape[1]) + (0 if k2 is None else k2.shape[2])
    scale = 1.0 / math.sqrt(HD // heads) if scale is None else float(scale)
    shape = (heads * G, R, T) if slot_major else (G, heads, R, T)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=q.device)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != q.device:
        raise H.HipLibraryError(f"attention_probs: out must be a contiguous float32 {shape} tensor on {q.device}")
    p_sg, p_sh = (R * T, G * R * T) if slot_major else (heads * R * T, R * T)
    a = attn.desc(q, k1, None, k2, None, mask, bias, heads, group_div, scale, 0.0, 0, causal, head_quirk)
    attn.probs(a, out, p_sg, p_sh, _mfma_dense(a, q, k1))
    return out


def bertscore(cand, ref, cand_len, ref_len, cand_w=None, ref_w=None):
    """BERTScore greedy matching of N (candidate, reference) pairs in one launch (fcmf_bertscore, include/fcmf_hip.h): cand
    [N, Lc, H] and ref [N, Lr, H] token embeddings (float32 or bf16, same dtype), cand_len / ref_len integer [N] valid rows of each
    pair (rows beyond them are never read), cand_w / ref_w optional float32 [N, L] per-token weights (None = 1 per valid token)
    -> float32 [N, 3] = P, R, F.  Detached; there is no backward.  Strides are normalised as attention_probs does: a unit
    innermost stride is kept with whatever row / pair strides come with it, anything else is made contiguous."""
    H.require_cuda(cand, ref, cand_len, ref_len, cand_w, ref_w)
    if cand.dim() != 3 or ref.dim() != 3 or cand.shape[0] != ref.shape[0] or cand.shape[2] != ref.shape[2] or cand.dtype != ref.dtype:
        raise H.HipLibraryError(f"bertscore: cand {tuple(cand.shape)} {cand.dtype} and ref {tuple(ref.shape)} {ref.dtype} must be "
                                f"[N, L, H] of one N, H and dtype")
    N, Lc, Hd = cand.shape
    Lr = ref.shape[1]

    def rows(x):
        x = x.detach()
        V = 16 // x.element_size()                  # (a view whose rows are not 16-byte aligned is copied, not refused)
        keep = (x.stride(2) == 1 and x.stride(1) >= x.shape[2] and x.stride(1) % V == 0 and x.stride(0) % V == 0
                and x.data_ptr() % 16 == 0)
        return x if keep else x.contiguous()

    def lens(l):
        if tuple(l.shape) != (N,) or l.dtype.is_floating_point:
            raise H.HipLibraryError(f"bertscore: lengths must be integer [{N}] tensors")
        return l.detach().to(torch.int32).contiguous()

    def weights(wt, L):
        if wt is None:
            return None
        if tuple(wt.shape) != (N, L):
            raise H.HipLibraryError(f"bertscore: weights must be [{N}, {L}], got {tuple(wt.shape)}")
        return wt.detach().float().contiguous()
    cand, ref = rows(cand), rows(ref)
    cand_len, ref_len = lens(cand_len), lens(ref_len)
    cand_w, ref_w = weights(cand_w, Lc), weights(ref_w, Lr)
    out = torch.empty((N, 3), dtype=torch.float32, device=cand.device)
    H.check(H.lib().fcmf_bertscore(H.ptr(cand), H.ptr(ref), H.ptr(cand_len), H.ptr(ref_len), H.ptr(cand_w), H.ptr(ref_w),
                                   H.ptr(out), N, Lc, Lr, Hd, cand.stride(1), cand.stride(0), ref.stride(1), ref.stride(0),
                                   H.dt(cand), H.stream()), "fcmf_bertscore")
    return out


# --------------------------------------------------------------------------------------
# box geometry
# --------------------------------------------------------------------------------------
_dim_mat_cache = {}


def box_dim_mat(device):
    """1/1000^(k/8), k=0..7, rounded exactly as roi_modeling.py:123-125 does (float32)"""
    key = str(device)
    if key not in _dim_mat_cache:
        feat_range = torch.arange(64 / 8)
        dm = 1.0 / torch.pow(1000, feat_range / (64 / 8))
        _dim_mat_cache[key] = dm.float().to(device)
    return _dim_mat_cache[key]


class BoxBiasFn(torch.autograd.Function):
    """log(clamp(relu(WG(emb(boxes))), 1e-6)) -> [G,heads,N,N] float32 (roi_modeling.py:148-163,40)"""

    @staticmethod
    def forward(ctx, coords, wg_w, wg_b, fast_trig=False):
        c = coords.contiguous()
        H.require_cuda(c, wg_w)
        G, N, _ = c.shape
        heads = wg_w.shape[0]
        ww, wb = wg_w.detach().contiguous().float(), wg_b.detach().contiguous().float()
        bias = torch.empty((G, heads, N, N), dtype=torch.float32, device=c.device)
        ctx.cdt = H.dt(c) | (H.BOX_FAST_TRIG if fast_trig and c.dtype == torch.float32 else 0)
        H.check(H.lib().fcmf_box_bias_fwd(H.ptr(c), ctx.cdt, H.ptr(box_dim_mat(c.device)), H.ptr(ww), H.ptr(wb),
                                          H.ptr(bias), G, N, heads, H.stream()), "fcmf_box_bias_fwd")
        ctx.save_for_backward(c, ww, wb)
        return bias

    @staticmethod
    def backward(ctx, dbias):
        c, ww, wb = ctx.saved_tensors
        G, N, _ = c.shape
        heads = ww.shape[0]
        buf = torch.zeros(ww.numel() + wb.numel(), dtype=torch.float32, device=ww.device)       # (one fill for both)
        dw, db = buf[:ww.numel()].view_as(ww), buf[ww.numel():].view_as(wb)
        d = dbias.contiguous().float()
        H.check(H.lib().fcmf_box_bias_bwd(H.ptr(c), ctx.cdt, H.ptr(box_dim_mat(c.device)), H.ptr(ww), H.ptr(wb), H.ptr(d),
                                          H.ptr(dw), H.ptr(db), G, N, heads, H.stream()), "fcmf_box_bias_bwd")
        return None, dw, db, None


def box_bias(coords, wg_w, wg_b):
    # The reference does the geometry in the dtype of the coordinates (float64 from the data loader,
    # roi_modeling.py:79-138) and rounds to float32 (:150).  The parity (fp32) mode keeps that; the bf16 mode
    # runs the float32 instantiation of the same kernels (sincosf instead of f64 sincos: 5x faster, error ~1e-5
    # on a bias that is consumed in bf16).
    # ... and the hardware's sine / cosine (FCMF_BOX_FAST_TRIG: the 64 sincosf calls per box pair were two thirds of both kernels;
    # argument error <= 1e-4 on a bias whose bf16 rounding is 3e-2).
    bf16_mode = compute_dtype() == torch.bfloat16
    if bf16_mode and coords.dtype == torch.float64:
        coords = coords.float()
    return BoxBiasFn.apply(coords, wg_w, wg_b, bf16_mode)


def box_embedding(coords):
    c = coords.contiguous()
    H.require_cuda(c)
    G, N, _ = c.shape
    emb = torch.empty((G, N, N, 64), dtype=torch.float32, device=c.device)
    H.check(H.lib().fcmf_box_embedding(H.ptr(c), H.dt(c), H.ptr(box_dim_mat(c.device)), H.ptr(emb), G, N, H.stream()),
            "fcmf_box_embedding")
    return emb


# --------------------------------------------------------------------------------------
# cross entropy
# --------------------------------------------------------------------------------------
class XentFn(torch.autograd.Function):
    """mean cross entropy over the non-ignored rows (torch.nn.CrossEntropyLoss semantics) x `mult`: rows, their mean and the
    backward's scale in two launches, no torch arithmetic (fcmf_xent_fwd + fcmf_xent_mean)"""

    @staticmethod
    def forward(ctx, logits, labels, ignore_index, mult):
        lg = logits if logits.stride(-1) == 1 else logits.contiguous()
        lg = lg.reshape(-1, lg.shape[-1]) if lg.dim() != 2 else lg
        lb = labels.reshape(-1).contiguous()
        H.require_cuda(lg, lb)
        n, C = lg.shape
        rows = torch.empty(n, dtype=torch.float32, device=lg.device)
        out2 = torch.empty(2, dtype=torch.float32, device=lg.device)       # [loss, mult / nvalid]
        L = H.lib()
        H.check(L.fcmf_xent_fwd(H.ptr(lg), lg.stride(0), H.ptr(lb), H.ptr(rows), None, n, C, ignore_index, H.dt(lg), H.stream()),
                "fcmf_xent_fwd")
        H.check(L.fcmf_xent_mean(H.ptr(rows), H.ptr(lb), n, ignore_index, float(mult), H.ptr(out2), H.stream()), "fcmf_xent_mean")
        ctx.save_for_backward(lg, lb, out2)
        ctx.ignore_index = ignore_index
        ctx.lshape = logits.shape
        return out2[0]

    @staticmethod
    def backward(ctx, g):
        lg, lb, out2 = ctx.saved_tensors
        n, C = lg.shape
        d = torch.empty((n, C), dtype=lg.dtype, device=lg.device)
        scale = (g.float() * out2[1]).reshape(1)
        H.check(H.lib().fcmf_xent_bwd(H.ptr(lg), lg.stride(0), H.ptr(lb), H.ptr(d), C, H.ptr(scale), 1.0, n, C,
                                      ctx.ignore_index, H.dt(lg), H.stream()), "fcmf_xent_bwd")
        return d.view(ctx.lshape), None, None, None


def additive_mask(m, value):
    """(m - 1) * (-value) as float32 for a 0 / 1 int64 mask [G, L] (row stride free): fcmf_additive_mask"""
    G, Lc = m.shape
    out = torch.empty((G, Lc), dtype=torch.float32, device=m.device)
    H.check(H.lib().fcmf_additive_mask(H.ptr(m), m.stride(0), H.ptr(out), G, Lc, float(value), H.stream()), "fcmf_additive_mask")
    return out


def check_loss_options(label_smoothing=0.0, focal_gamma=0.0):
    """the value limits of fcmf_xent_*_ex (include/fcmf_hip.h), raised as a ValueError that names the argument -> (eps, gamma)"""
    for name, v in (("label_smoothing", label_smoothing), ("focal_gamma", focal_gamma)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
            raise ValueError(f"{name} must be a finite number, got {v!r}")
    if not 0.0 <= label_smoothing < 1.0:
        raise ValueError(f"label_smoothing must lie in [0, 1), got {label_smoothing}")
    if focal_gamma < 0.0:
        raise ValueError(f"focal_gamma must be >= 0 (0 = off), got {focal_gamma}")
    if label_smoothing > 0.0 and focal_gamma > 0.0:
        raise ValueError(f"focal_gamma ({focal_gamma}) and label_smoothing ({label_smoothing}) cannot both be set")
    return float(label_smoothing), float(focal_gamma)


def _loss_weight(weight, C, segments, device, what):
    """class weights of a loss -> (contiguous float32 tensor or None, fcmf_xent_*_ex's wstride: 0 = [C] shared, C = [segments, C])"""
    if weight is None:
        return None, 0
    if not torch.is_tensor(weight):
        raise H.HipLibraryError(f"{what} must be a tensor, got {type(weight).__name__}")
    if weight.device != device:
        raise H.HipLibraryError(f"{what} is on {weight.device}, the logits are on {device}")
    if weight.dtype != torch.float32:
        raise H.HipLibraryError(f"{what} must be float32, got {weight.dtype}")
    if tuple(weight.shape) == (C,):
        return weight.contiguous(), 0
    if tuple(weight.shape) == (segments, C):
        return weight.contiguous(), C
    raise H.HipLibraryError(f"{what} must have shape [{C}] or [{segments}, {C}] (segments, classes), got {tuple(weight.shape)}")


def _grad_scalar(g):
    """the upstream gradient of a scalar loss as the device float32 [1] that fcmf_xent_bwd_ex reads"""
    g = g.reshape(1)
    return g if g.dtype == torch.float32 else g.float()


class XentExFn(torch.autograd.Function):
    """cross entropy with class weights, label smoothing or a focal factor, each segment (row r -> segment r % segments) divided
    by its own live weight sum, x `mult`: fcmf_xent_fwd_ex + fcmf_xent_reduce_ex forward, fcmf_xent_bwd_ex backward, no torch
    arithmetic between them (include/fcmf_hip.h states the function)"""

    @staticmethod
    def forward(ctx, logits, labels, weight, ignore_index, mult, eps, gamma, segments):
        lg = _rows2d(logits)
        lb = labels.reshape(-1).contiguous()
        H.require_cuda(lg, lb)
        n, C = lg.shape
        if segments < 1 or n % segments != 0:
            raise H.HipLibraryError(f"cross_entropy: {n} rows do not divide into {segments} segments")
        if lb.numel() != n:
            raise H.HipLibraryError(f"cross_entropy: {n} rows of logits but {lb.numel()} labels")
        w, wstride = _loss_weight(weight, C, segments, lg.device, "cross_entropy: weight")
        ld = lg.stride(0) if n > 1 else max(lg.stride(0), C)              # (one row: its stride means nothing)
        rows = torch.empty((2, n), dtype=torch.float32, device=lg.device)
        out = torch.empty(1 + segments, dtype=torch.float32, device=lg.device)      # [loss, mult / D_s ...]
        L = H.lib()
        H.check(L.fcmf_xent_fwd_ex(H.ptr(lg), ld, H.ptr(lb), H.ptr(w), wstride, H.ptr(rows[0]), H.ptr(rows[1]), n, C, segments,
                                   ignore_index, eps, gamma, H.dt(lg), H.stream()), "fcmf_xent_fwd_ex")
        H.check(L.fcmf_xent_reduce_ex(H.ptr(rows[0]), H.ptr(rows[1]), n, segments, mult, H.ptr(out), H.ptr(out[1:]), H.stream()),
                "fcmf_xent_reduce_ex")
        ctx.save_for_backward(lg, lb, out, *(() if w is None else (w,)))
        ctx.cfg = (ignore_index, eps, gamma, segments, wstride, ld, logits.shape)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        lg, lb, out = ctx.saved_tensors[:3]
        w = ctx.saved_tensors[3] if len(ctx.saved_tensors) > 3 else None
        ignore_index, eps, gamma, segments, wstride, ld, lshape = ctx.cfg
        n, C = lg.shape
        d = torch.empty((n, C), dtype=lg.dtype, device=lg.device)
        g = _grad_scalar(g)
        H.check(H.lib().fcmf_xent_bwd_ex(H.ptr(lg), ld, H.ptr(lb), H.ptr(w), wstride, H.ptr(d), C, H.ptr(out[1:]), H.ptr(g), n, C,
                                         segments, ignore_index, eps, gamma, H.dt(lg), H.stream()), "fcmf_xent_bwd_ex")
        return d.view(lshape), None, None, None, None, None, None, None


def cross_entropy(logits, labels, ignore_index=-100, mult=1.0, *, weight=None, label_smoothing=0.0, focal_gamma=0.0, segments=1):
    """torch.nn.CrossEntropyLoss semantics x `mult`.  Options (any of them selects XentExFn; none leaves the plain XentFn):
    `weight` float32 [C] or [segments, C] on the device, `label_smoothing` in [0, 1), `focal_gamma` >= 0 (not with smoothing),
    `segments`: row r of the flattened logits belongs to segment r % segments, and the result is the SUM over the segments of each
    segment's own weighted mean (logits [B, A, C]: segments=A is the drivers' sum over aspects of per-aspect batch means)."""
    eps, gamma = check_loss_options(label_smoothing, focal_gamma)
    if isinstance(segments, bool) or not isinstance(segments, int) or segments < 1:
        raise ValueError(f"segments must be a positive integer, got {segments!r}")
    if weight is None and eps == 0.0 and gamma == 0.0 and segments == 1:
        return XentFn.apply(logits, labels, int(ignore_index), float(mult))
    return XentExFn.apply(logits, labels, weight, int(ignore_index), float(mult), eps, gamma, segments)


def _rows2d(logits):
    lg = logits if logits.stride(-1) == 1 else logits.contiguous()
    return lg.reshape(-1, lg.shape[-1]) if lg.dim() != 2 else lg


def check_rdrop_alpha(alpha, name="alpha"):
    """the weight of the symmetric-KL term: a finite number >= 0 (0 = off), else a ValueError that names the argument -> float"""
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float)) or not math.isfinite(alpha) or alpha < 0.0:
        raise ValueError(f"{name} must be a finite number >= 0 (0 = off), got {alpha!r}")
    return float(alpha)


class SymmetricKLFn(torch.autograd.Function):
    """alpha x sum over segments of the live pairs' mean 1/2 [KL(p||q) + KL(q||p)], p / q = softmax of a pair of rows of a / b
    (include/fcmf_hip.h states the function): fcmf_symkl_fwd + fcmf_xent_reduce_ex forward, fcmf_symkl_bwd backward"""

    @staticmethod
    def forward(ctx, a, b, labels, ignore_index, alpha, segments):
        a2, b2 = _rows2d(a), _rows2d(b)
        lb = None if labels is None else labels.reshape(-1).contiguous()
        n, C = a2.shape
        a2, b2 = (t.contiguous() if n > 1 and t.stride(0) < C else t for t in (a2, b2))      # (an expanded row)
        lda, ldb = (t.stride(0) if n > 1 else C for t in (a2, b2))               # (one row: its stride means nothing)
        rows = torch.empty((2, n), dtype=torch.float32, device=a2.device)
        out = torch.empty(1 + segments, dtype=torch.float32, device=a2.device)     # [loss, alpha / N_s ...]
        L = H.lib()
        H.check(L.fcmf_symkl_fwd(H.ptr(a2), lda, H.ptr(b2), ldb, H.ptr(lb), H.ptr(rows[0]), H.ptr(rows[1]), n, C, segments,
                                 ignore_index, H.dt(a2), H.stream()), "fcmf_symkl_fwd")
        H.check(L.fcmf_xent_reduce_ex(H.ptr(rows[0]), H.ptr(rows[1]), n, segments, alpha, H.ptr(out), H.ptr(out[1:]), H.stream()),
                "fcmf_xent_reduce_ex")
        ctx.save_for_backward(a2, b2, out, *(() if lb is None else (lb,)))
        ctx.cfg = (ignore_index, segments, lda, ldb, a.shape, b.shape)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        a2, b2, out = ctx.saved_tensors[:3]
        lb = ctx.saved_tensors[3] if len(ctx.saved_tensors) > 3 else None
        ignore_index, segments, lda, ldb, ashape, bshape = ctx.cfg
        n, C = a2.shape
        d = torch.empty((2, n, C), dtype=a2.dtype, device=a2.device)
        g = _grad_scalar(g)
        H.check(H.lib().fcmf_symkl_bwd(H.ptr(a2), lda, H.ptr(b2), ldb, H.ptr(lb), H.ptr(d[0]), C, H.ptr(d[1]), C, H.ptr(out[1:]),
                                       H.ptr(g), n, C, segments, ignore_index, 0, H.dt(a2), H.stream()), "fcmf_symkl_bwd")
        need = ctx.needs_input_grad
        return d[0].view(ashape) if need[0] else None, d[1].view(bshape) if need[1] else None, None, None, None, None


def symmetric_kl(a, b, labels=None, ignore_index=-100, *, alpha=1.0, segments=1):
    """the R-Drop consistency term of two logit tensors of one shape [..., C]: alpha x the SUM over segments (pair r of the
    flattened rows -> segment r % segments) of the MEAN over the segment's live pairs of 1/2 [KL(softmax a || softmax b) +
    KL(softmax b || softmax a)].  `labels` (int64, one per pair, optional) only decides liveness: a pair whose label is
    ignore_index contributes nothing.  Gradients go to whichever of a, b needs one."""
    alpha = check_rdrop_alpha(alpha)
    if isinstance(segments, bool) or not isinstance(segments, int) or segments < 1:
        raise ValueError(f"segments must be a positive integer, got {segments!r}")
    if not torch.is_tensor(a) or not torch.is_tensor(b):
        raise H.HipLibraryError("symmetric_kl: a and b must be tensors")
    H.require_cuda(a, b, labels)
    if a.shape != b.shape or a.dim() < 1:
        raise H.HipLibraryError(f"symmetric_kl: a {tuple(a.shape)} and b {tuple(b.shape)} must have one shape [..., C]")
    if a.dtype != b.dtype or a.dtype not in (torch.float32, torch.bfloat16):
        raise H.HipLibraryError(f"symmetric_kl: a and b must both be float32 or both bfloat16, got {a.dtype} and {b.dtype}")
    if a.device != b.device or (labels is not None and labels.device != a.device):
        raise H.HipLibraryError("symmetric_kl: a, b and labels must be on one device")
    n = a.numel() // a.shape[-1] if a.shape[-1] else 0
    if a.shape[-1] < 1 or n % segments != 0:
        raise H.HipLibraryError(f"symmetric_kl: {n} pairs of {a.shape[-1]} columns do not divide into {segments} segments")
    if labels is not None and (labels.dtype != torch.int64 or labels.numel() != n):
        raise H.HipLibraryError(f"symmetric_kl: labels must be int64 with {n} entries, got {labels.dtype} with {labels.numel()}")
    return SymmetricKLFn.apply(a, b, labels, int(ignore_index), alpha, segments)


def rdrop_pairs(logits, labels, rdrop_alpha):
    """what the R-Drop form of a model's loss_aspects adds: logits [2B, A, C] (copy i and copy i + B of review i), labels [B, A]
    -> (the labels repeated for the cross entropy over all 2B rows, rdrop_alpha x symmetric_kl of the two halves with the
    aspects as its segments)"""
    alpha = check_rdrop_alpha(rdrop_alpha, "rdrop_alpha")
    B = labels.shape[0]
    if logits.dim() != 3 or logits.shape[0] != 2 * B:
        raise H.HipLibraryError(f"loss_aspects: rdrop_alpha > 0 takes the logits of two passes, [2 x {B}, A, C] for labels "
                                f"{tuple(labels.shape)}; got {tuple(logits.shape)}")
    return torch.cat((labels, labels), dim=0), symmetric_kl(logits[:B], logits[B:], segments=logits.shape[1], alpha=alpha)


class BCELogitsFn(torch.autograd.Function):
    """torch.nn.BCEWithLogitsLoss() (mean over every element) of logits [N, C] against float targets: fcmf_bce_logits, one
    launch forward (the loss) and one backward ((sigmoid - target) * g / (N C)), no torch arithmetic"""

    @staticmethod
    def forward(ctx, logits, target):
        lg = _rows2d(logits)
        tg = target.reshape(lg.shape).float().contiguous()
        H.require_cuda(lg, tg)
        n, C = lg.shape
        loss = torch.empty((), dtype=torch.float32, device=lg.device)
        H.check(H.lib().fcmf_bce_logits(H.ptr(lg), lg.stride(0), H.ptr(tg), C, n, C, None, H.ptr(loss), None, C, None, H.dt(lg),
                                        H.stream()), "fcmf_bce_logits")
        ctx.save_for_backward(lg, tg)
        ctx.lshape = logits.shape
        return loss

    @staticmethod
    def backward(ctx, g):
        lg, tg = ctx.saved_tensors
        n, C = lg.shape
        d = torch.empty((n, C), dtype=lg.dtype, device=lg.device)
        gs = g.float().contiguous()
        H.check(H.lib().fcmf_bce_logits(H.ptr(lg), lg.stride(0), H.ptr(tg), C, n, C, H.ptr(gs), None, H.ptr(d), C, None, H.dt(lg),
                                        H.stream()), "fcmf_bce_logits")
        return d.view(ctx.lshape), None


def bce_with_logits(logits, target):
    return BCELogitsFn.apply(logits, target)


def sigmoid(logits):
    """float32 sigmoid of [N, C] logits (evaluating a multi-label head): the `probs` output of fcmf_bce_logits"""
    lg = _rows2d(logits.detach())
    H.require_cuda(lg)
    n, C = lg.shape
    probs = torch.empty((n, C), dtype=torch.float32, device=lg.device)
    H.check(H.lib().fcmf_bce_logits(H.ptr(lg), lg.stride(0), None, C, n, C, None, None, None, C, H.ptr(probs), H.dt(lg),
                                    H.stream()), "fcmf_bce_logits")
    return probs.view(logits.shape)
