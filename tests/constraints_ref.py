"""The executable statement of fcmf_logits_constrain's contract (include/fcmf_hip.h) in numpy, on ONE row and its sequence: the
arithmetic in float32 (one multiply or one correctly rounded divide -- numpy's float32 operators are IEEE), then one rounding to
nearest-even into the storage type.  Plain module: no fixtures, and nothing here calls the library.

For a row x (its first V columns), its sequence h (start token first, the token the step ran on last; L = len(h) >= 1):
  1. repetition penalty theta: for every DISTINCT v in h with 0 <= v < V: x[v] <- x[v] * theta if x[v] < 0 else x[v] / theta;
  2. no_repeat_ngram_size n >= 1: for every i in 0 .. L-n with h[i : i+n-1] == h[L-n+1 :]: x[h[i+n-1]] <- -inf;
  3. min_length m: if L < m: x[sep_id] <- -inf;
  4. x[v] <- -inf for v in ban_ids.
Ids outside [0, V) write nothing; a ban wins over a penalty.

`constrained_step` wraps a step function seq -> logits into the constrained one, so that oracle.beam_search_ids (through a
log-softmax) and sampling_ref.sample_chains run constrained decodes unchanged."""
import numpy as np
import torch


def to_bf16_bits(x32):
    """float32 array -> uint16 bf16 bit patterns, round to nearest-even (NaN stays NaN)"""
    u = np.asarray(x32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)
    nan = np.isnan(np.asarray(x32, dtype=np.float32))
    return np.where(nan, np.uint16(0x7FC0), r)


def from_bf16_bits(b):
    return (np.asarray(b, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def round_storage(x32, bf16):
    """float32 values rounded once into the storage type, returned as float32"""
    return from_bf16_bits(to_bf16_bits(x32)) if bf16 else np.asarray(x32, dtype=np.float32)


def banned(h, V, no_repeat_ngram_size=0, min_length=0, sep_id=-1, ban_ids=()):
    """the set of columns in [0, V) that rules 2 - 4 set to -inf for the sequence h"""
    h = [int(v) for v in h]
    L, n = len(h), int(no_repeat_ngram_size)
    out = set()
    if n >= 1 and L >= n:
        suffix = h[L - n + 1:]
        for i in range(L - n + 1):
            if h[i:i + n - 1] == suffix:
                out.add(h[i + n - 1])
    if min_length > 0 and L < min_length:
        out.add(int(sep_id))
    out.update(int(v) for v in ban_ids)
    return {v for v in out if 0 <= v < V}


def constrain_row(x, h, V=None, repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0, sep_id=-1, ban_ids=(), bf16=False):
    """x: the stored values of one row as float32 (exactly representable in the storage type) -> the row after the call, float32
    holding storage-type values; columns >= V are returned as they came"""
    x = np.array(x, dtype=np.float32, copy=True)
    V = x.shape[0] if V is None else V
    theta = np.float32(repetition_penalty)
    if theta != np.float32(1.0):
        for v in sorted({int(v) for v in h if 0 <= int(v) < V}):
            with np.errstate(all="ignore"):
                y = x[v] * theta if x[v] < 0 else x[v] / theta
            x[v] = round_storage(np.float32(y), bf16)
    for v in banned(h, V, no_repeat_ngram_size, min_length, sep_id, ban_ids):
        x[v] = -np.inf
    return x


def constrain_rows(X, hist, V=None, bf16=False, **settings):
    """X [rows, >= V] float32, hist [rows, L] -> the rows after the call"""
    return np.stack([constrain_row(x, h, V, bf16=bf16, **settings) for x, h in zip(np.asarray(X, dtype=np.float32), np.asarray(hist))])


def constrained_step(step_logits, sep_id, repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0, suppress_tokens=(), bf16=False,
                     as_logprobs=False):
    """step_logits(seq) -> logits [V] (numpy or torch, float32 values)  ==>  seq -> the constrained logits as float64 numpy, or --
    as_logprobs -- their log-softmax as a float32 torch tensor (what oracle.beam_search_ids takes): banned tokens at -inf, the
    mass renormalised over the rest"""
    def step(seq):
        x = step_logits(seq)
        x = x.detach().float().numpy() if isinstance(x, torch.Tensor) else np.asarray(x, dtype=np.float32)
        y = constrain_row(x, seq, None, repetition_penalty, no_repeat_ngram_size, min_length, sep_id, suppress_tokens, bf16)
        if as_logprobs:
            return torch.log_softmax(torch.from_numpy(y).float(), dim=-1)
        return y.astype(np.float64)
    return step


def has_repeated_ngram(seq, n):
    grams = [tuple(seq[i:i + n]) for i in range(len(seq) - n + 1)]
    return len(grams) != len(set(grams))
