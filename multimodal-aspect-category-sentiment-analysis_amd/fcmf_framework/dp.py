"""Single-node data parallelism for the FCMF step: one process per GPU, replicated parameters, the minibatch
sharded across ranks, ONE exchange per optimizer step -- the gradient mean.

The reference wraps the model in torch DDP with find_unused_parameters=True over NCCL
(run_multimodal_fcmf.py:237-240).  Here the exchange is explicit and sized for xGMI:

* `GradArena`: every parameter's gradient is a view of ONE flat float32 buffer, laid out in the order backward
  produces gradients (reverse registration order; q/k/v weights of a fused attention block adjacent so that their
  [3H, H] weight-gradient GEMM writes one slice).  The backward kernels write straight into the slices
  (`ops.grad_dest`): one memset per step replaces the per-tensor zero fills, autograd adopts the slices as
  `p.grad` without copying, and a bucket of gradients is a contiguous range of the buffer.
* `GradReducer`: all-reduces (RCCL, `torch.distributed` backend "nccl" on ROCm; gloo in the CPU tests) each bucket
  IN PLACE -- no concatenation, no copy-back -- on a side stream as soon as the last gradient of the bucket has been
  accumulated, so the collective overlaps the rest of backward; divides by the world size on that stream; reports how
  long the main stream actually waited for communication (`stats()`).  Parameters that never receive a gradient (the
  text encoder's pooler, dead at fcmf_pretraining.py:41) are left out of the arena instead of searched for every step
  (DDP's find_unused_parameters).
"""
import torch
import torch.distributed as dist

ALIGN = 64      # elements: every slice starts on a 256-byte boundary (16-byte vector accesses, clean bucket edges)


class GradArena:
    def __init__(self, params, blocks=(), pad_rows=32):
        """params: the parameters that receive gradients, in registration order.  blocks: lists of parameters that
        must sit next to each other, in the given order (fused q|k|v weight / bias gradients).  pad_rows: a large 2-D parameter
        whose row count is no multiple of this (the 64001-row tied vocabulary matrix) gets zeroed SLACK rows behind its slice, so
        that the MFMA weight-gradient GEMM -- which writes whole 32-row groups -- can accumulate straight into it (`claim(p, rows=...)`)."""
        params = [p for p in params if p.requires_grad]
        seen, uniq = set(), []
        for p in params:                      # tied parameters (decoder.dense.weight) appear once
            if id(p) not in seen:
                seen.add(id(p))
                uniq.append(p)
        self.params = uniq
        in_block = {id(p): bi for bi, b in enumerate(blocks) for p in b}
        order, done = [], set()
        for p in reversed(self.params):       # the order backward produces them
            if id(p) in done:
                continue
            group = blocks[in_block[id(p)]] if id(p) in in_block else [p]
            for q in group:
                if id(q) in seen and id(q) not in done:
                    done.add(id(q))
                    order.append(q)
        self.order = order
        self.offset, off = {}, 0
        self.slack = {}                       # parameter -> zeroed elements behind its slice (see pad_rows)
        self.packed = set()                   # parameters packed tight behind their block head (no alignment gap before them)
        for p in order:
            adj = id(p) in in_block and blocks[in_block[id(p)]][0] is not p      # packed tight behind its block head
            if not adj:
                off = (off + ALIGN - 1) // ALIGN * ALIGN
            else:
                self.packed.add(id(p))
            self.offset[id(p)] = off
            off += p.numel()
            if pad_rows and p.dim() == 2 and p.shape[0] >= 8192 and p.shape[0] % pad_rows:
                self.slack[id(p)] = (pad_rows - p.shape[0] % pad_rows) * p.shape[1]
                off += self.slack[id(p)]
        self.total = (off + ALIGN - 1) // ALIGN * ALIGN
        dev = self.params[0].device
        self.flat = torch.zeros(self.total, dtype=torch.float32, device=dev)
        self.view = {id(p): self.flat[self.offset[id(p)]:self.offset[id(p)] + p.numel()].view_as(p) for p in order}
        self._by_ptr = {p.data_ptr(): p for p in order}
        self._slice_param = {self.view[id(p)].data_ptr(): p for p in order}     # arena address -> the parameter whose slice starts there
        self.fwd_uses = {}                    # parameter address -> forward GEMMs that used it since zero() (ops.gemm_nt)
        self._taken = set()
        self.on_zero = []                     # callbacks (the reducer resets its bucket state here)
        self.activate()

    @classmethod
    def for_model(cls, model, skip=lambda name: "bert.cell.pooler" in name, extra=()):
        """arena over the model's live parameters; q|k|v parameters of every fused attention block adjacent.
        extra: parameters of modules that run BEFORE the model in the step (the ResNet-152 extractors under
        --fine_tune_cnn): their gradients are produced last in backward, so their slices follow the model's."""
        from .fused import QKVStorageMixin
        blocks = []
        for m in model.modules():
            if isinstance(m, QKVStorageMixin):
                blocks.append([m.query.weight, m.key.weight, m.value.weight])
                blocks.append([m.query.bias, m.key.bias, m.value.bias])
        # IAOG decoder: the per-head projection weights whose gradients ONE column-blocked GEMM writes (ops.head_project_bwd ->
        # ops.head_weight_grad) -- [w_kx | w_qx] of every self attention, and the w_kx of ALL blocks' cross attention (ONE
        # ops.head_linear projects the encoder output by all of them: IAOGDecoder.project_encoder)
        for m in model.modules():
            blks = getattr(m, "blks", None)
            if blks is not None and all(hasattr(b, "attention1") and hasattr(b, "attention2") for b in blks):
                for b in blks:
                    blocks.append([b.attention1.w_kx, b.attention1.w_qx])
                blocks.append([b.attention2.w_kx for b in blks])
        return cls(list(extra) + [p for n, p in model.named_parameters() if not skip(n)], blocks)

    # ---- step protocol -------------------------------------------------------------------------
    def activate(self):
        from . import ops
        ops.set_grad_arena(self)

    def deactivate(self):
        from . import ops
        if ops.grad_arena() is self:
            ops.set_grad_arena(None)

    def zero(self):
        """start of an optimizer step: ONE memset; gradients are detached so that the first producer's slice is
        adopted by autograd as p.grad without a copy.  (With gradient accumulation call this once per optimizer
        step, not per micro-step.)"""
        self.flat.zero_()
        self._taken.clear()
        self.fwd_uses.clear()
        for p in self.order:
            p.grad = None
        for cb in self.on_zero:
            cb()

    def note_forward(self, ptr):
        self.fwd_uses[ptr] = self.fwd_uses.get(ptr, 0) + 1

    def used_once(self, slice_ptr):
        """True if the arena slice starting at `slice_ptr` belongs to a parameter that exactly ONE forward GEMM has used since
        zero(): its weight gradient then has a single producer in this backward pass (ops.deferred_dw may delay it; with two
        producers autograd ADDS their results the moment each Function returns)"""
        return self.uses(slice_ptr) == 1

    def uses(self, slice_ptr):
        """forward GEMMs that have used the parameter whose arena slice starts at `slice_ptr` since zero() (0: no such slice, or a
        parameter whose producers are unknown)"""
        p = self._slice_param.get(slice_ptr)
        return 0 if p is None else self.fwd_uses.get(p.data_ptr(), 0)

    def _resolve(self, param):
        """the arena's parameter behind `param`, or None ("not here").  Matched by address AND element count: a [3H, H] view of
        the fused q|k|v block shares the query weight's pointer.  Not across micro-steps of a gradient accumulation: once p.grad
        is set, every producer of a pass must return a tensor (a temporary that autograd adds), or the post-accumulate hook that
        drives the bucket exchange would not fire."""
        p = self._by_ptr.get(param.data_ptr())
        if p is None or p.numel() != param.numel() or p.grad is not None:
            return None
        return p

    def claim(self, params, rows=None):
        """-> None ("not here": the caller uses a zero-filled temporary that autograd adds) or (buf, first).
        params: one parameter -> buf is its slice; with `rows` (a producer that writes rows >= shape[0] rows of a 2-D parameter:
        the padded vocabulary projection) the [rows, cols] buffer that starts at the slice and runs into its zeroed slack, None if
        the slack does not cover it.  A list of parameters -> ONE flat buffer covering their slices, which must be adjacent in
        the given order (fused q|k|v, the IAOG decoder's per-head weights) and all in the same state.
        first: this call claimed the slice(s) -- the caller hands autograd aliases of them (`grad_alias`, or views of buf).  Not
        first: an EARLIER producer of this backward pass has claimed them (a weight applied several times in the forward: the
        fusion layer runs 7 + 1 times, the tied vocabulary matrix): the caller accumulates into buf IN PLACE and hands autograd
        `None` for this use -- the first producer's tensor, which autograd holds until every use has reported, is this very
        memory.  (Round 3 gave later producers a zero-filled temporary that autograd then added: a fill and an add launch per
        parameter and use.)"""
        if isinstance(params, (list, tuple)):
            ps = [self._resolve(q) for q in params]
            if any(p is None for p in ps):
                return None
            first = id(ps[0]) not in self._taken
            off = end = self.offset[id(ps[0])]
            for p in ps:
                if self.offset[id(p)] != end or (id(p) not in self._taken) != first:
                    return None
                end += p.numel()
            buf = self.flat[off:end]
        else:
            p = self._resolve(params)
            if p is None:
                return None
            ps = (p,)
            first = id(p) not in self._taken
            if rows is None:
                buf = self.view[id(p)]
            else:
                if p.dim() != 2 or rows < p.shape[0] or (rows - p.shape[0]) * p.shape[1] > self.slack.get(id(p), 0):
                    return None
                off = self.offset[id(p)]
                buf = self.flat[off:off + rows * p.shape[1]].view(rows, p.shape[1])
        if first:
            self._taken.update(id(p) for p in ps)
        return buf, first

    def release(self, params):
        """give back claimed slices that nothing was written to (a kernel refused the shape)"""
        for q in params:
            p = self._by_ptr.get(q.data_ptr())
            if p is not None:
                self._taken.discard(id(p))

    def grad_alias(self, param, shape=None):
        """a FRESH tensor object over the slice of `param` to hand autograd: it adopts a gradient as p.grad without a copy only
        when it is the sole holder of the tensor object -- the arena's own view objects would be cloned"""
        v = self.view[id(self._by_ptr[param.data_ptr()])]
        return v.view(v.shape if shape is None else shape)

    def adopt(self, p):
        """make p.grad the arena slice (copying a gradient that was produced elsewhere into it)"""
        v = self.view.get(id(p))
        if v is None or p.grad is None or p.grad.data_ptr() == v.data_ptr():
            return
        v.copy_(p.grad)
        p.grad = v

    def adopt_all(self):
        for p in self.order:
            self.adopt(p)


class GradReducer:
    """bucketed in-place gradient mean over the ranks, overlapped with backward.

    bucket_mb : target bucket size.  32 MB by default: xGMI is point to point (7 links x ~150 GB/s per GPU), a ring
                all-reduce is bound by one link, and a bucket must be large enough to amortise the collective's launch +
                synchronisation (~20-30 us) yet small enough that the first collective starts early in backward and the
                LAST one -- the only one nothing can hide -- is short.  FCMF-base: 626 MB of float32 gradients = 20 buckets.
    exchange  : "fp32" -- all-reduce of the float32 slices in place (bit-comparable with DDP);
                "bf16" -- half the bytes on the links with float32 ACCUMULATION on arrival: each rank sends shard j of its
                bucket, rounded to bf16, to rank j (all-to-all), rank j sums the `world` shards in float32, rounds the sum to
                bf16 once and all-gathers it.  (A bf16 all-reduce would round the running sum at every ring step.)  Every
                rank ends up with the same bits, so replicas cannot drift.
    native    : all-reduce through the C ABI (`fcmf_dp_allreduce_bucket`: RCCL bound by libfcmf_hip.so itself) instead of
                `torch.distributed.all_reduce`; fp32 exchange, CUDA tensors, one GPU per process.
    group_mb  : launch granularity.  Buckets are SENT in groups of consecutive ready buckets of at least this many MB (160 by
                default = four to five encoder layers): the weight-gradient GEMMs of a group's parameters are queued by
                `ops.deferred_dw` until the group goes out and are multiplied together as one work list (`fcmf_gemm_dw_list`), and
                only the queue entries whose destination lies in the group's arena range are flushed -- later layers keep
                batching.  (Round 3 flushed the whole queue before every 32 MB bucket: one matrix per shape per flush, i.e. the
                batched kernel never ran under data parallelism.)  The collectives stay one per bucket, back to back.
    recheck_every: how often (in optimizer steps) the set of parameters that receive no gradient on any rank is
                re-verified -- a parameter that turns live on SOME rank later raises on EVERY rank instead of
                silently diverging replicas (round-2 advisor finding).
    single_rank: run the whole machinery (hooks, buckets, collectives, mean) in a group of ONE rank as well instead of
                short-circuiting it -- the RCCL path rehearsed on a one-GPU box (tests/test_dp_gpu.py)."""

    def __init__(self, arena, bucket_mb=32, process_group=None, overlap=True, exchange="fp32", native=False, recheck_every=50,
                 group_mb=160, single_rank=False):
        if not isinstance(arena, GradArena):                      # list of parameters (round-1 signature)
            arena = GradArena(list(arena))
        if exchange not in ("fp32", "bf16"):
            raise ValueError("exchange must be 'fp32' or 'bf16'")
        self.arena = arena
        self.group = process_group
        self.world = dist.get_world_size(process_group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(process_group) if dist.is_initialized() else 0
        self.live = self.world > 1 or (single_rank and dist.is_initialized())
        self.params = arena.order
        self.overlap = overlap
        self.exchange = exchange
        self.recheck_every = recheck_every
        cap = int(bucket_mb * 1024 * 1024 / 4)
        self.group_elems = int(group_mb * 1024 * 1024 / 4)
        self.buckets = []                     # (lo, hi, [params]) contiguous ranges of arena.flat, backward order
        cur, lo = [], 0
        order = arena.order
        for i, p in enumerate(order):
            cur.append(p)
            hi = arena.offset[id(p)] + p.numel()
            nxt = order[i + 1] if i + 1 < len(order) else None
            # a bucket may only end where the next slice starts on its own ALIGN boundary: never inside a tightly packed
            # q|k|v block (its members' sizes need not be multiples of ALIGN: a rounded-up edge would cut into the next one)
            if hi - lo >= cap and nxt is not None and id(nxt) not in arena.packed:
                edge = arena.offset[id(nxt)]
                self.buckets.append((lo, edge, cur))
                cur, lo = [], edge
        if cur:
            self.buckets.append((lo, arena.total, cur))
        self._check_partition()
        self._bucket_of = {id(p): bi for bi, (_, _, ps) in enumerate(self.buckets) for p in ps}
        self._hooks = []
        self._stream = None
        self.enabled = True        # set False on non-boundary micro-steps of gradient accumulation
        self._exposed_ms, self._steps, self._events = 0.0, 0, []
        self._dead = None
        self._stage = {}
        self.launch_log = []       # bucket indices in launch order of the current step (tests, diagnostics)
        self.group_log = []        # (first bucket, last bucket, parameters still without a local gradient) per group sent
        self._n_dead = [0] * len(self.buckets)
        self._native = None
        if native and self.live:
            self._native = _NativeComm(self.world, self.rank, self.group, arena.flat.device)
        if self.live:
            for p in self.params:
                self._hooks.append(p.register_post_accumulate_grad_hook(self._on_grad))
        arena.on_zero.append(self.reset)
        self.reset()

    def _check_partition(self):
        """the buckets tile [0, total) and every parameter's slice lies inside ITS bucket"""
        pos = 0
        for lo, hi, ps in self.buckets:
            assert lo == pos and hi > lo and lo % ALIGN == 0, (lo, hi, pos)
            for p in ps:
                o = self.arena.offset[id(p)]
                assert lo <= o and o + p.numel() <= hi, "gradient slice crosses a bucket edge"
            pos = hi
        assert pos == self.arena.total

    def reset(self):
        self._ready = [set() for _ in self.buckets]
        self._launched = [False] * len(self.buckets)
        self._work = []
        self.launch_log = []
        self.group_log = []
        self._next = 0

    # -- called by autograd right after p.grad has been accumulated ------------------------------
    def _on_grad(self, p):
        if not self.enabled:
            return
        self.arena.adopt(p)
        bi = self._bucket_of[id(p)]
        if self._dead is None or id(p) not in self._dead:      # (a "dead" parameter that turns live is caught by the recheck, on every rank at once)
            self._ready[bi].add(id(p))
        if self.overlap:
            self._launch_in_order()

    def _complete(self, bi):
        """every parameter of bucket bi has its gradient -- or never gets one: parameters that received no gradient on ANY
        rank in the first step (`_dead`, the same set on every rank) count as ready, or one of them would hold its bucket and
        every later one back until finish()"""
        return len(self._ready[bi]) + self._n_dead[bi] >= len(self.buckets[bi][2])

    def _launch_in_order(self, flush=False):
        """collectives must be issued in the SAME order on every rank: buckets go out strictly in arena (= backward) order,
        bucket k only once buckets 0..k-1 have gone.  A bucket that is complete before its predecessor (a parameter without a
        gradient on this rank, a gradient produced out of order) waits for it -- at the latest until finish().  Consecutive
        complete buckets are sent as a GROUP once they add up to `group_mb` (or the arena ends): see the class docstring."""
        nb = len(self.buckets)
        while self._next < nb:
            end, size = self._next, 0
            while end < nb and (flush or self._complete(end)):
                size += self.buckets[end][1] - self.buckets[end][0]
                end += 1
                if size >= self.group_elems and not flush:
                    break
            # (everything but the LAST bucket complete: nothing is left to batch with -- FCMF's last bucket is the 196 MB word-embedding
            #  gradient, produced by the final backward kernel; the layers in front of it must not wait for it)
            if end == self._next or not (flush or size >= self.group_elems or end >= nb - 1):
                return
            self._flush_range(self._next, end)
            self.group_log.append((self._next, end - 1, sum(len(self.buckets[b][2]) - len(self._ready[b]) for b in range(self._next, end))))
            for bi in range(self._next, end):
                self._launch(bi)
            self._next = end

    def _flush_range(self, b0, b1):
        """queued weight-gradient GEMMs (ops.deferred_dw) whose destination lies in buckets b0 .. b1-1 are issued now, as one
        batch per shape; the others stay queued"""
        from . import ops
        flat = self.arena.flat
        if flat.is_cuda:
            base = flat.data_ptr()
            ops.flush_deferred_dw(base + 4 * self.buckets[b0][0], base + 4 * self.buckets[b1 - 1][1])

    def _side(self, buf):
        if self._stream is None:
            self._stream = torch.cuda.Stream(device=buf.device)
        return self._stream

    def _launch(self, bi):
        if self._launched[bi]:
            return
        self._launched[bi] = True
        self.launch_log.append(bi)
        lo, hi, ps = self.buckets[bi]
        for p in ps:                          # gradients that arrived while disabled (accumulation) or not at all
            self.arena.adopt(p)
        buf = self.arena.flat[lo:hi]
        if self.exchange == "bf16":
            return self._launch_bf16(bi, buf)
        if buf.is_cuda:
            side = self._side(buf)
            side.wait_stream(torch.cuda.current_stream(buf.device))
            with torch.cuda.stream(side):
                if self._native is not None:
                    self._native.allreduce_mean(buf, side)
                    w = None
                else:
                    w = dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=self.group, async_op=True)
        else:
            w = dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=self.group, async_op=True)
        self._work.append((w, buf))

    # -- bf16 on the links, float32 accumulation on arrival ---------------------------------------
    def _launch_bf16(self, bi, buf):
        n, W = buf.numel(), self.world
        shard = ((n + W - 1) // W + ALIGN - 1) // ALIGN * ALIGN
        st = self._stage.get(bi)
        if st is None:
            mk = lambda k: torch.zeros(k, dtype=torch.bfloat16, device=buf.device)
            st = self._stage[bi] = (mk(W * shard), mk(W * shard), mk(shard))       # send, receive / gathered, my reduced shard
        send, recv, mine = st

        def run():
            _cast(buf, send[:n])                                   # float32 slice -> bf16 (the tail of `send` stays zero)
            dist.all_to_all_single(recv, send, group=self.group)   # recv[j*shard:(j+1)*shard] = rank j's shard `rank`
            _sum_rows(recv.view(W, shard), mine)                   # float32 accumulation, ONE rounding to bf16
            dist.all_gather_into_tensor(recv, mine, group=self.group)
            _cast(recv[:n], buf, scale=1.0 / W)                    # mean, back in the float32 arena
        if buf.is_cuda:
            side = self._side(buf)
            side.wait_stream(torch.cuda.current_stream(buf.device))
            with torch.cuda.stream(side):
                run()                        # (RCCL collectives called on `side`: stream-ordered, the host does not wait)
        else:
            run()
        self._work.append((None, None))

    def finish(self):
        """after backward: flush buckets whose gradients never all arrived, wait for the collectives and leave the
        MEAN in the arena (p.grad of every parameter that received a gradient on ANY rank is its arena slice)."""
        if not self.live:
            return
        self._launch_in_order(flush=True)
        cuda = self.arena.flat.is_cuda
        if cuda:
            main = torch.cuda.current_stream(self.arena.flat.device)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(main)
        for w, buf in self._work:
            if w is None:                     # bf16 exchange / native RCCL: already the mean, ordered on the side stream
                continue
            if cuda:
                with torch.cuda.stream(self._stream):
                    w.wait()                  # (RCCL: makes the SIDE stream wait for the collective, not the host)
                    buf.div_(self.world)
            else:
                w.wait()
                buf.div_(self.world)
        if cuda:
            main.wait_stream(self._stream)
            e1.record(main)
            self._events.append((e0, e1))
        if self._dead is None or (self.recheck_every and self._steps % self.recheck_every == 0):
            # which parameters received a gradient on NO rank (statically dead ones that were not left out of the
            # arena): decided on the first step -- they keep p.grad = None so that the optimizer skips them exactly as
            # it does in a single process (DDP's find_unused_parameters, made static) -- and re-verified now and then:
            # the reduced bitmap is the same on every rank, so a change raises everywhere at once
            have = torch.tensor([0.0 if p.grad is None else 1.0 for p in self.params], device=self.arena.flat.device)
            dist.all_reduce(have, op=dist.ReduceOp.SUM, group=self.group)
            dead = {id(p) for p, h in zip(self.params, have.tolist()) if h == 0.0}
            if self._dead is not None and not self._dead <= dead:
                raise RuntimeError("GradReducer: a parameter that received no gradient on any rank in the first step "
                                   "now receives one on some rank; exclude statically dead parameters with "
                                   "GradArena.for_model(skip=...) or build the reducer after the graph is final")
            if self._dead is None:
                self._dead = dead
                self._n_dead = [sum(id(p) in dead for p in ps) for _, _, ps in self.buckets]
        for p in self.params:                 # a parameter without a LOCAL gradient still takes part in the mean
            if p.grad is None and id(p) not in self._dead:
                p.grad = self.arena.view[id(p)]
        self._steps += 1
        self._work = []

    def stats(self):
        """exposed (not overlapped) communication: how long the main stream sat in finish() per step"""
        ms = [a.elapsed_time(b) for a, b in self._events]
        self._events = []
        return dict(world=self.world, buckets=len(self.buckets), bytes_per_step=self.arena.total * (2 if self.exchange == "bf16" else 4),
                    launch_groups=len(self.group_log) or None, group_mb=round(self.group_elems * 4 / 2 ** 20, 1), bucket_mb=[round((hi - lo) * 4 / 2 ** 20, 1) for lo, hi, _ in self.buckets],
                    arena_mb=round(self.arena.total * 4 / 2 ** 20, 1), exchange=self.exchange, native_rccl=self._native is not None,
                    exposed_comm_ms_per_step=round(sum(ms) / max(1, len(ms)), 3) if ms else None, steps=self._steps)

    def broadcast_parameters(self, src=0):
        """replicate rank `src`'s parameters (what DDP does at wrap time)"""
        if not self.live:
            return
        for p in self.params:
            dist.broadcast(p.data, src=src, group=self.group)

    def close(self):
        if self._native is not None:
            self._native.close()
            self._native = None


def _cast(src, dst, scale=None):
    """dst <- src converted to dst's dtype (x scale): the library's cast kernel on the GPU; torch on CPU tensors (gloo tests)"""
    if src.is_cuda:
        from . import _hip as H
        H.check(H.lib().fcmf_cast(H.ptr(src), H.ptr(dst), src.numel(), H.dt(src), H.dt(dst), H.stream()), "fcmf_cast")
        if scale is not None:
            dst.mul_(scale)
    else:
        dst.copy_(src if scale is None else src.float() * scale)


def _sum_rows(x, out):
    """out[j] = sum_i x[i, j], accumulated in float32, rounded to out's dtype once"""
    if x.is_cuda:
        from . import _hip as H
        H.check(H.lib().fcmf_sum_axis(H.ptr(x), H.ptr(out), 1, x.shape[0], x.shape[1], H.dt(x), H.stream()), "fcmf_sum_axis")
    else:
        out.copy_(x.float().sum(0))


class _NativeComm:
    """RCCL communicator owned by libfcmf_hip.so (C ABI `fcmf_dp_*`); the 128-byte unique id travels over the existing
    torch.distributed group (any backend), the collectives themselves never touch torch.distributed"""

    def __init__(self, world, rank, group, device):
        import ctypes
        from . import _hip as H
        L = H.lib()
        uid = (ctypes.c_char * 128)()
        if rank == 0:
            H.check(L.fcmf_dp_unique_id(ctypes.cast(uid, ctypes.c_void_p)), "fcmf_dp_unique_id")
        box = [bytes(uid)]
        dist.broadcast_object_list(box, src=0, group=group)
        uid = (ctypes.c_char * 128).from_buffer_copy(box[0])
        self._h = ctypes.c_void_p()
        torch.cuda.set_device(device)
        H.check(L.fcmf_dp_comm_create(ctypes.byref(self._h), ctypes.cast(uid, ctypes.c_void_p), world, rank), "fcmf_dp_comm_create")

    def allreduce_mean(self, buf, stream):
        from . import _hip as H
        H.check(H.lib().fcmf_dp_allreduce_bucket(self._h, H.ptr(buf), buf.numel(), H.dt(buf), 1, stream.cuda_stream),
                "fcmf_dp_allreduce_bucket")

    def close(self):
        from . import _hip as H
        if self._h:
            H.lib().fcmf_dp_comm_destroy(self._h)
            self._h = None
