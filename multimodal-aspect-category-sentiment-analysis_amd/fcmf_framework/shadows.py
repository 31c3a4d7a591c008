"""Weight shadows: every GEMM operand that is derived from a float32 master parameter -- its bf16 copy, the transposed copy
the dX GEMM reads, the e4m3 copies, the zero-padded vocabulary matrix, the per-head and other re-layouts.

ONE dict, keyed (kind, address, shape, tag); ONE entry type; ONE rule for serving an entry (`Entry.serves`).  Addresses are
recycled -- a freed model's for the next model's parameters of the same shape and version -- so an entry belongs to a tensor,
its OWNER, not to an address: it holds a weak reference to the owner and is served to nobody else.  The owner of `w` is the
explicit `owner=` argument, else `w` itself, and in both cases the tensor that one is a view of (`_base`): successive view
objects `W[:E]` of a packed parameter are temporaries, `W` is what persists."""
import weakref

import torch

from . import _hip as H

VOCAB_PAD = 32   # row padding of ragged 2-D weights (one MFMA k-tile)


def _owner(w, owner, addr):
    """-> (the owner of `w`, which lies at `addr`; how many bytes into the owner that is)"""
    o = w if owner is None else owner
    if o._base is not None:
        o = o._base
    return (o, 0) if o is w else (o, addr - o.data_ptr())


class Entry:
    """`payload` was built from the bytes at `owner()`'s address + `offset` when the owner's version was `version`.
    dense: that source is a contiguous [R, C] matrix (`refresh_transposed` re-reads it in place).  full: the bf16 copy of a
    ragged 2-D weight is the head of this zero-padded buffer."""
    __slots__ = ("payload", "version", "stale", "owner", "offset", "dense", "full")

    def __init__(self, payload, version, owner, offset, dense=True, stale=False):
        self.payload, self.version, self.stale, self.owner, self.offset, self.dense = payload, version, stale, owner, offset, dense
        self.full = None

    def serves(self, w, owner, addr, fresh=True):
        """THE rule.  This entry, keyed at `addr`, is `w`'s: its owner is alive, is the owner of `w` (`_owner`) and still lies
        where it lay -- and, unless any age will do (fresh=False), is of the owner's version and not marked stale.
        (A tensor that owns an entry is no view: when it asks for itself there is nothing to resolve.)"""
        o = self.owner()
        if o is not w or owner is not None:
            ow, offset = _owner(w, owner, addr)
            if o is not ow or self.offset != offset:
                return False
        return not fresh or (self.version == o._version and not self.stale)


class Shadows:
    def __init__(self):
        self._d = {}
        self._owners = {}      # id(owner) -> (weak reference, its address when its first entry was made): what `_prune` walks
        self._mt_tables = None
        self.swaps = 0         # how often FusedAdamW.ema_weights() exchanged the parameters' contents (never reset)

    def __len__(self):
        return len(self._d)

    def lookup(self, kind, w, tag=None, owner=None):
        """read-only: `w`'s entry of `kind` ("bf16", "t", "fp8", "fp8_t", "derived", "heads"), fresh or not, or None"""
        addr = w.data_ptr()
        e = self._d.get((kind, addr, w.shape, tag))
        return e if e is not None and e.serves(w, owner, addr, fresh=False) else None

    def _put(self, key, payload, o, offset, dense=True, stale=False):
        e = self._d[key] = Entry(payload, o._version, weakref.ref(o), offset, dense, stale)
        self._owners.setdefault(id(o), (e.owner, key[1] - offset))
        return e

    def get(self, w, owner=None):
        """the fresh bf16 copy of a float32 weight"""
        key = ("bf16", w.data_ptr(), w.shape, None)
        e = self._d.get(key)
        if e is not None and e.serves(w, owner, key[1]):
            return e.payload
        o, off = _owner(w, owner, key[1])
        full = None
        if e is not None and e.owner() is o:      # (the owner's own buffer, out of date: rebuilt in place; another tensor's is left alone)
            sh, full = e.payload, e.full
        elif w.dim() == 2 and w.shape[0] % VOCAB_PAD != 0:
            # 2-D weights with a ragged row count (the 64001-row tied vocabulary matrix) get ZERO rows up to the next
            # multiple of 32 behind the copy: `padded(w)` hands the MFMA kernels a regular [rows32, K] operand
            rows = (w.shape[0] + VOCAB_PAD - 1) // VOCAB_PAD * VOCAB_PAD
            full = torch.zeros((rows, w.shape[1]), dtype=torch.bfloat16, device=w.device)
            sh = full[:w.shape[0]]
        else:
            sh = torch.empty(w.shape, dtype=torch.bfloat16, device=w.device)
        src = w.detach()
        if not src.is_contiguous():
            src = src.contiguous()
        H.check(H.lib().fcmf_cast(H.ptr(src), H.ptr(sh), src.numel(), H.F32, H.BF16, H.stream()), "fcmf_cast")
        self._put(key, sh, o, off).full = full
        return sh

    def padded(self, w):
        """the fresh bf16 copy of a 2-D weight including its zero rows up to a multiple of 32"""
        sh = self.get(w)
        full = self._d[("bf16", w.data_ptr(), w.shape, None)].full
        return sh if full is None else full

    def get_t(self, w, owner=None):
        """bf16 TRANSPOSE [K, N] of a float32 [N, K] weight: dX = dY W then reads W^T as a K-contiguous operand
        (ds_read_b128 instead of transposed LDS reads: the NT kernels run 10-25 % faster than the NN ones).
        Rebuilt by `refresh_transposed` after an optimizer step, or lazily (one small kernel per weight)."""
        key = ("t", w.data_ptr(), w.shape, None)
        e = self._d.get(key)
        if e is not None and e.serves(w, owner, key[1]):
            return e.payload
        o, off = _owner(w, owner, key[1])
        sh = e.payload if e is not None and e.owner() is o else \
            torch.empty((w.shape[1], w.shape[0]), dtype=torch.bfloat16, device=w.device)
        src = w.detach()
        if not src.is_contiguous():
            src = src.contiguous()
        H.check(H.lib().fcmf_cast_transpose(H.ptr(src), H.ptr(sh), w.shape[0], w.shape[1], H.stream()), "fcmf_cast_transpose")
        self._put(key, sh, o, off, dense=w.is_contiguous())
        return sh

    def _fp8(self, kind, w, owner, source):
        key = (kind, w.data_ptr(), w.shape, None)
        e = self._d.get(key)
        if e is not None and e.serves(w, owner, key[1]):
            return e.payload
        o, off = _owner(w, owner, key[1])
        src = source()                                  # [rows, K] bf16, fresh
        rows, K = src.shape
        q, sc = e.payload if e is not None and e.owner() is o else \
            (torch.empty((rows, K), dtype=torch.uint8, device=src.device), torch.empty(rows, dtype=torch.float32, device=src.device))
        H.check(H.lib().fcmf_quant_fp8_rows(H.ptr(src), K, H.ptr(q), K, H.ptr(sc), rows, K, H.dt(src), H.stream()), "fcmf_quant_fp8_rows")
        return self._put(key, (q, sc), o, off).payload

    def get_fp8(self, w, owner=None):
        """(q [N, K] e4m3 bytes, scale [N] float32) of a float32 [N, K] weight, quantised per output row (from the bf16 copy:
        half the bytes to read); rebuilt lazily after the parameter changed"""
        return self._fp8("fp8", w, owner, lambda: self.get(w, owner) if w.is_contiguous() else w.detach().contiguous())

    def get_fp8_t(self, w, owner=None):
        """(q [K, N] e4m3, scale [K]) of the TRANSPOSE of a float32 [N, K] weight, quantised per input row: the B operand
        of dX = dY W on the fp8 kernel (contraction over N)"""
        return self._fp8("fp8_t", w, owner, lambda: self.get_t(w, owner))

    def derived(self, w, tag, build):
        """a tensor derived from the parameter `w` (a re-layout and / or cast), cached per tag and rebuilt by
        `build(w.detach())` when the parameter has changed"""
        key = ("derived", w.data_ptr(), w.shape, tag)
        e = self._d.get(key)
        if e is not None and e.serves(w, None, key[1]):
            return e.payload
        o, off = _owner(w, None, key[1])
        return self._put(key, build(w.detach()), o, off).payload

    def head_nk(self, ws):
        """bf16 [len(ws) * n_head * d, E] re-layout ("nn.Linear layout", natural head order) of the per-head weights `ws` (float32
        Parameters [n_head, E, d] of the IAOG decoder's Attention): row (i * n_head + h) * d + j = ws[i][h, :, j].  Every [d, E]
        row block is the transpose of the dense [E, d] slice ws[i][h] and is REGISTERED as one of the transposed copies, so
        `refresh_transposed` rebuilds all of them -- every block of the decoder -- in the optimizer's one launch.  With another
        optimizer the first use after an update refreshes everything, also in one launch."""
        nh, E, d = ws[0].shape
        key = ("heads", ws[0].data_ptr(), ws[0].shape, tuple(w.data_ptr() for w in ws))
        g = self._d.get(key)
        if g is not None and g.serves(ws[0], None, key[1], fresh=False):
            # (one parameter's pieces are registered, refreshed, marked stale and pruned together: its first stands for all)
            buf, firsts = g.payload
            fresh = lambda: all(e is not None and e.serves(w, None, k2[1]) for w, k2 in zip(ws, firsts) for e in (self._d.get(k2),))
            if fresh():
                return buf
            self.refresh_transposed()      # merely stale: one launch for all of them
            if fresh():
                return buf                 # (else a piece was pruned, its parameter has moved, or is another tensor's: start over)
        buf = torch.empty((len(ws) * nh * d, E), dtype=torch.bfloat16, device=ws[0].device)
        pieces = []
        for i, w in enumerate(ws):
            if w.dtype != torch.float32 or not w.is_contiguous() or tuple(w.shape) != (nh, E, d):
                raise H.HipLibraryError("head_nk: dense float32 [n_head, E, d] parameters expected")
            for h in range(nh):
                src = w.detach()[h]
                # (the GROUP is part of the key: the same parameter may sit in two groupings -- [w_kx] alone and [w_kx, w_qx] --
                #  and each grouping's buffer must keep its own registered pieces, or the loser would serve stale weights)
                k2 = ("t", src.data_ptr(), (E, d), key[1:])
                self._put(k2, buf[(i * nh + h) * d:(i * nh + h + 1) * d], w, src.data_ptr() - w.data_ptr(), stale=True)
                pieces.append(k2)
        self._mt_tables = None
        self._put(key, (buf, pieces[::nh]), ws[0], 0)
        self.refresh_transposed()
        return buf

    def peek(self, w):
        """`w`'s own bf16 copy, fresh or not (FusedAdamW writes it in its update kernel), or None"""
        e = self.lookup("bf16", w)
        return None if e is None else e.payload

    def mark_fresh(self, w):
        e = self.lookup("bf16", w)
        if e is not None:
            e.version, e.stale = e.owner()._version, False

    def _prune(self):
        """drop the entries whose owner is gone (a freed model: its storage may have been returned to the driver, or recycled
        for something else) or has moved (`.to()`, re-fused q|k|v storage).  Nothing to do while every owner is where it was."""
        if all(o is not None and o.data_ptr() == a for r, a in self._owners.values() for o in (r(),)):
            return
        dead = [k for k, e in self._d.items() for o in (e.owner(),) if o is None or o.data_ptr() + e.offset != k[1]]
        for k in dead:
            del self._d[k]
        if any(k[0] == "t" for k in dead):
            self._mt_tables = None
        self._owners = {id(e.owner()): (e.owner, k[1] - e.offset) for k, e in self._d.items()}

    def mark_all_stale(self):
        """the parameters were rewritten behind autograd's back (the fused optimizers' update kernels)"""
        self._prune()
        for e in self._d.values():
            e.stale = True

    def refresh_transposed(self):
        """rebuild EVERY cached transposed copy of a LIVE weight in one launch (called by the fused optimizers right after
        their update: all of them are stale at that point, and rebuilding them lazily costs one small launch per weight)"""
        self._prune()
        items = [(k, e) for k, e in self._d.items() if k[0] == "t" and e.dense]      # (sources read in place must be dense [R, C])
        if not items:
            return
        sig = tuple((k[1], e.payload.data_ptr()) for k, e in items)
        if self._mt_tables is None or self._mt_tables[0] != sig:
            dev = items[0][1].payload.device
            desc = []
            for t, (k, _) in enumerate(items):
                R, C = k[2]
                desc += [(t, r, c) for r in range((R + 63) // 64) for c in range((C + 63) // 64)]
            self._mt_tables = (sig,
                               torch.tensor([k[1] for k, _ in items], dtype=torch.int64, device=dev),
                               torch.tensor([e.payload.data_ptr() for _, e in items], dtype=torch.int64, device=dev),
                               torch.tensor([list(k[2]) for k, _ in items], dtype=torch.int32, device=dev),
                               torch.tensor(desc, dtype=torch.int32, device=dev), len(desc))
        _, src, dst, dims, desc, n = self._mt_tables
        H.check(H.lib().fcmf_multi_cast_transpose(H.ptr(src), H.ptr(dst), H.ptr(dims), H.ptr(desc), n, H.stream()),
                "fcmf_multi_cast_transpose")
        for _, e in items:
            e.version, e.stale = e.owner()._version, False

    def clear(self):
        self._d.clear()
        self._owners.clear()
        self._mt_tables = None


shadows = Shadows()
