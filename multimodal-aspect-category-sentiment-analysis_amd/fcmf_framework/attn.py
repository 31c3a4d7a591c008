"""The one way from attention operands to a launch: a descriptor (fcmf_attn_desc, include/fcmf_hip.h), the MFMA / VALU choice
made from the descriptor's own fields, and one function per kernel pair.  ops, fused and iaog_modeling normalise their
operands, build a descriptor here and call these; nothing else in the package launches an fcmf_attn_small / _mfma / _probs
kernel or fills an AttnDesc.  The long kernels (long_forward / long_backward / long_probs: fcmf_attn_mfma_long_fwd / _bwd /
_probs, any number of keys, one key/value set per `kv_share` consecutive query groups) take dense tensors instead of a
descriptor: their key sets are not the descriptor's per-group keys."""
import ctypes
import functools

import torch

from . import _hip as H

USE_MFMA_ATTENTION = True   # the single switch: tests and tools turn it off to compare the MFMA kernels with the VALU kernels


def desc(q, k1, v1, k2, v2, mask, bias, heads, group_div, scale, p, seed, causal, head_quirk):
    """q [G,R,heads*d]; k1 / v1 [G,T1,heads*d] shared by the R rows of a group; k2 / v2 [G/group_div,R,T2,heads*d] private per
    row (V is read with K's strides); mask, bias contiguous float32.  Shapes, strides and addresses only: nothing is launched."""
    G, R, HD = q.shape
    d = HD // heads
    T1 = 0 if k1 is None else k1.shape[1]
    T2 = 0 if k2 is None else k2.shape[2]
    a = H.AttnDesc()
    a.dtype, a.G, a.heads, a.d, a.R, a.T1, a.T2, a.group_div = H.dt(q), G, heads, d, R, T1, T2, group_div
    a.q_sg, a.q_sr = q.stride(0), q.stride(1)
    if k1 is not None:
        a.k1_sg, a.k1_st = k1.stride(0), k1.stride(1)
    if k2 is not None:
        a.k2_sg, a.k2_sr, a.k2_st = k2.stride(0), k2.stride(1), k2.stride(2)
    a.o_sg, a.o_sr = R * HD, HD
    a.q, a.k1, a.v1, a.k2, a.v2, a.mask, a.bias = H.ptr(q), H.ptr(k1), H.ptr(v1), H.ptr(k2), H.ptr(v2), H.ptr(mask), H.ptr(bias)
    a.scale, a.dropout_p, a.seed, a.causal, a.head_quirk = scale, p, seed, int(causal), int(head_quirk)
    return a


def mfma_eligible(a):
    """the text-encoder shape (bf16, head dim 64, <= 256 queries and shared keys, plain mask) goes to the MFMA kernels.  They
    address row t of group g at (g*T + t)*ld: callers whose operands are not column blocks of [G*T, ld] buffers demand dense ones."""
    return (USE_MFMA_ATTENTION and a.dtype == H.BF16 and a.d == 64 and a.T2 == 0 and a.k1 is not None and a.bias is None
            and not a.causal and not a.head_quirk and a.T1 <= 256 and a.R <= 256)


def _ld(a):
    """-> ldq, ldk of the MFMA kernels: the row strides; a group of ONE row has none of its own ((g*1 + 0)*ld: its group stride)"""
    return (a.q_sr if a.R > 1 else a.q_sg), (a.k1_st if a.T1 > 1 else a.k1_sg)


def forward(a, out, lse, mfma):
    if mfma:
        H.check(H.lib().fcmf_attn_mfma_fwd(a.q, a.k1, a.v1, a.mask, H.ptr(out), H.ptr(lse), a.G, a.heads, a.R, a.T1, *_ld(a),
                                           a.o_sr, a.scale, a.dropout_p, a.seed, H.stream()), "fcmf_attn_mfma_fwd")
    else:
        H.check(H.lib().fcmf_attn_small_fwd(a, H.ptr(out), H.ptr(lse), H.stream()), "fcmf_attn_small_fwd")


def probs(a, out, p_sg, p_sh, mfma):
    """the pre-dropout softmax as float32: element (g, slot h, r, t) at out + g*p_sg + h*p_sh + r*(T1+T2) + t"""
    if mfma:
        H.check(H.lib().fcmf_attn_mfma_probs(a.q, a.k1, a.mask, H.ptr(out), a.G, a.heads, a.R, a.T1, *_ld(a), p_sg, p_sh,
                                             a.scale, H.stream()), "fcmf_attn_mfma_probs")
    else:
        H.check(H.lib().fcmf_attn_probs(a, H.ptr(out), p_sg, p_sh, H.stream()), "fcmf_attn_probs")


def small_backward(a, out, dout, lse, like_q, dk1, dv1, dk2=None, dv2=None, dbias=None, scratch=None):
    """the VALU backward -> dq (shaped like like_q, a [G,R,heads*d] tensor).  The kernel writes one dq partial per 128 SHARED
    keys, summed here.  scratch (float32, 2*G*heads*R*T2): the grouped backward, dk2 / dv2 already summed over group_div."""
    nch = max(1, (a.T1 + 127) // 128)
    dq = torch.empty((nch,) + tuple(like_q.shape), dtype=like_q.dtype, device=like_q.device)
    if scratch is not None:
        H.check(H.lib().fcmf_attn_small_bwd_grouped(a, H.ptr(out), H.ptr(dout), H.ptr(lse), H.ptr(dq), H.ptr(dk1), H.ptr(dv1),
                                                    H.ptr(dk2), H.ptr(dv2), H.ptr(dbias), H.ptr(scratch), scratch.numel() * 4,
                                                    H.stream()), "fcmf_attn_small_bwd_grouped")
    else:
        H.check(H.lib().fcmf_attn_small_bwd(a, H.ptr(out), H.ptr(dout), H.ptr(lse), H.ptr(dq), H.ptr(dk1), H.ptr(dv1),
                                            H.ptr(dk2), H.ptr(dv2), H.ptr(dbias), H.stream()), "fcmf_attn_small_bwd")
    return sum_leading(dq)


def mfma_backward(a, out, dout, lse, dq, dk, dv, colsum_part=None):
    """dq / dk / dv: ADDRESSES, written with the row strides of q / k1 (columns of one dqkv buffer, or tensors laid out like
    q / k1 / v1).  colsum_part (float32 [G, 3*heads*64]): also receives each sequence's column sums of dq | dk | dv."""
    H.check(H.lib().fcmf_attn_mfma_bwd(a.q, a.k1, a.v1, a.mask, H.ptr(out), H.ptr(dout), H.ptr(lse), dq, dk, dv, a.G, a.heads,
                                       a.R, a.T1, *_ld(a), a.o_sr, a.scale, a.dropout_p, a.seed, H.ptr(colsum_part), H.stream()),
            "fcmf_attn_mfma_bwd")


def long_forward(q, k, v, mask, out, lse, heads, kv_share, scale, p, seed):
    """q / out [G,Tq,heads*64], k / v [G/kv_share,Tk,heads*64], all dense bf16; mask [G,Tk] float32 or None; lse [G,heads,Tq]"""
    G, Tq, HD = q.shape
    H.check(H.lib().fcmf_attn_mfma_long_fwd(H.ptr(q), H.ptr(k), H.ptr(v), H.ptr(mask), H.ptr(out), H.ptr(lse), G, heads, Tq,
                                            k.shape[1], kv_share, HD, HD, HD, scale, p, seed, H.stream()), "fcmf_attn_mfma_long_fwd")


def long_backward(q, k, v, mask, out, dout, lse, dq, dk, dv, heads, kv_share, scale, p, seed):
    """dq / dk / dv: dense tensors like q / k / v"""
    G, Tq, HD = q.shape
    # running float32 sums of dk | dv over the sharing groups (written before they are read: no fill)
    ws = torch.empty(2 * k.numel(), dtype=torch.float32, device=q.device) if kv_share > 1 else None
    H.check(H.lib().fcmf_attn_mfma_long_bwd(H.ptr(q), H.ptr(k), H.ptr(v), H.ptr(mask), H.ptr(out), H.ptr(dout), H.ptr(lse),
                                            H.ptr(dq), H.ptr(dk), H.ptr(dv), G, heads, Tq, k.shape[1], kv_share, HD, HD, HD, scale,
                                            p, seed, H.ptr(ws), 0 if ws is None else ws.numel() * 4, H.stream()),
            "fcmf_attn_mfma_long_bwd")


def long_probs(q, k, mask, out, heads, kv_share, scale, head_mean):
    """the pre-dropout softmax of long_forward as float32: out [G,heads,Tq,Tk], or with head_mean [G,Tq,Tk] = the mean over
    the heads, formed inside the kernel.  q / k dense bf16 as long_forward's; every element of out is written"""
    G, Tq, HD = q.shape
    H.check(H.lib().fcmf_attn_mfma_long_probs(H.ptr(q), H.ptr(k), H.ptr(mask), H.ptr(out), G, heads, Tq, k.shape[1], kv_share,
                                              HD, HD, scale, int(head_mean), H.stream()), "fcmf_attn_mfma_long_probs")


def sum_leading(x):
    """[n, ...] -> [...] summing the leading axis (attention dq chunk partials)"""
    return x[0] if x.shape[0] == 1 else sum_groups(x, x.shape[0])[0]


def sum_groups(x, reps):
    """[G, ...] -> [G/reps, ...] summing consecutive groups"""
    G = x.shape[0]
    inner = x[0].numel()
    out = torch.empty((G // reps,) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
    H.check(H.lib().fcmf_sum_axis(H.ptr(x), H.ptr(out), G // reps, reps, inner, H.dt(x), H.stream()), "fcmf_sum_axis")
    return out


def small_plan(a, backward=False, grouped=False, has_dbias=False, has_dv1=True, ptrs_aligned=True):
    """what fcmf_attn_small_fwd / _bwd / _bwd_grouped would launch for the descriptor (host only, nothing is launched) ->
    (return code, info[11] as fcmf_attn_small_plan documents it, (kernel name, name of the follow-up kernel or None))"""
    info = (ctypes.c_int32 * 11)()
    names = (ctypes.c_char_p * 2)()
    rc = H.lib().fcmf_attn_small_plan(a, int(backward), int(grouped), int(has_dbias), int(has_dv1), int(ptrs_aligned), info, names)
    return rc, list(info), tuple(None if n is None else n.decode() for n in names)


@functools.lru_cache(maxsize=None)
def valu_float32_key_limit(d):
    """most shared keys the float32 VALU attention takes at head dim d: the largest T whose forward plan the library accepts
    (its K and V images, the waves' score rows and one query row must fit the LDS; never more than its 512-key limit)"""
    a = H.AttnDesc()
    a.dtype, a.G, a.heads, a.d, a.R, a.group_div = H.F32, 1, 1, d, 1, 1
    a.q = a.k1 = a.v1 = 16              # presence and alignment are all the plan reads of an address
    for T in range(512, 0, -1):
        a.T1 = T
        if small_plan(a)[0] == 0:
            return T
    return 0
