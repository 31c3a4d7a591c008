"""IAOG decode: the beam search the reference keeps beside FCMFSeq2Seq (fcmf_pretraining.py:383-517, commented out there,
as are its call sites run_pretraining_fcmf.py:405-414,523-533) with the same signature, semantics and return value.

What the reference's loop does, and what this module does with it on the GPU:
  * the encoder runs ONCE per sample (:404-418); here also the per-block cross-attention key projections of its output
    (`w_kx` of all decoder blocks, one GEMM -- `IAOGDecoder.project_encoder`) run once per sample instead of once per beam
    and step;
  * every step feeds ONLY the last token of a beam to the decoder ([1, 1], :452,470) and the decoder's per-block cache
    is never filled (mm_modeling.py:584-588 write state[2][i] only when it already holds a tensor; the reference's
    deep copies :461-465 copy Nones), so a step sees the last token at position 0 and the encoder output -- nothing else.
    The step's log-probabilities are therefore a function of (sample, last token): they are computed once per distinct
    token and kept (a beam search of width k and length L costs at most 1 + k (L - 1) decoder steps, usually far fewer),
    top-k on the device, one host read per new token;
  * scores are Python floats summed in the reference's order; candidates are sorted by score, descending and stable (:493).
Batch size 1 per decoder call, as in the reference: the decoder `Attention`'s slot -> head pairing depends on the batch
size (mm_modeling.py:79-85), so stacking beams into one call would change the arithmetic.

`beam_search_batch` / `beam_search_ids_batch` advance a whole eval batch one beam round per decoder call instead.  At batch size
1 the pairing is the plain one (slot s reads head s), so the (sample, last token) rows of every sample's live beams that the memo
does not hold yet go through ONE `IAOGDecoder.decode_step` with the plain pairing per row -- the batch-1 result of each row, one
vocabulary GEMM with M = rows, log-softmax + top-k in one HIP kernel (csrc/topk.hip: no eager log_softmax / topk), one host read per
round.  The beam rules per sample are `beam_search_ids`'s, unchanged: `beam_rounds` is that loop over many samples with the
device step behind a callable.

context="prefix" (every entry point; the default "last" is the reference's loop above, unchanged): a step is conditioned on the
beam's whole prefix instead -- the function the decoder is trained as (is_train=True: token p at position p, causal self
attention, the tril rule on the cross attention), at batch size 1 and in eval mode.  The step's logits for seq = [start .. tok_t]
are row t of the teacher-forced decoder call on tensor([seq]).  There is no (sample, token) memo: every live beam is a row of its
round, all rows of round t have length t + 1, and `IAOGDecoder.decode_step_prefix` runs them in one pass over a per-block KEY cache
[max_len, B * beam, n_head * d] (values are the keys: no value cache).  The host carries per beam the ANCESTOR TABLE -- which row
of round p held position p of this beam -- and uploads it with the tokens and sample indices in the round's one host-to-device
tensor; csrc/attn_decode.hip reads the cache through it and appends the round's keys, so beams that share or reorder history copy
nothing on the device.  One host read per round, as in "last" mode; the beam rules are the same code (`_advance`).

length_penalty (every entry point, default 0): the FINAL choice among the finished hypotheses (or, when none finished, among the
live beams) ranks by score / max(len(seq) - 1, 1) ** length_penalty instead of the raw log-likelihood sum, which always prefers the
shortest.  The per-round pruning and every returned score stay the raw sum; 0 takes the reference's code path, with no division.

Sampling (`sample_rounds`, `sample_ids_batch`, `sample_batch`): instead of a beam, every sample runs `num_chains` independent
chains; per round every unfinished chain is one row of the batched step of either context and draws ONE token from the step's
distribution after temperature / top-k / nucleus filtering (csrc/sample.hip: no eager softmax / sort / cumsum / multinomial).  The
draw of (sample, chain, round) is a function of the sampler's seed and the counter ((sample_offset + b) * num_chains + c) * max_len + t
alone, so a sample's text does not depend on the eval batch it is decoded in.  A chain's score is the sum of its tokens'
log-probabilities under the model's own distribution, the quantity a beam's score is.

Constraints (every entry point, `constraints=` a dict of `make_constraints`' settings, default None): repetition_penalty,
no_repeat_ngram_size, min_length and suppress_tokens, by the rules of Hugging Face's logits processors, applied to the step's LOGITS
on the device (csrc/constrain.hip, between the vocabulary GEMM and either tail) -- the constrained logits are the step's
distribution, so every returned log-probability, beam and chain score is under it, in both strategies alike.  A constrained step is
a function of the row's whole sequence: the rows handed to the step carry the beam's or chain's `seq` (the host has it), the step
puts it into the round's one upload tensor and the kernel takes the [n, L] view by strides; beam search in context "last" loses its
(sample, last token) memo and runs every live beam as a row of its round, as sampling does.  Still one upload and one host read per
round; the suppressed ids are uploaded once per call.  None, or all settings off, takes the paths above unchanged: the step
callables receive exactly the same tuples and no new code runs.

loop="device" (the batched entry points and, through them, `beam_search_ids` / `beam_search`; default "host": everything above,
untouched): the search itself moves to the device.  The state -- sequences and ancestor table position-major, float64 scores, slot
states, per sample a finished list and a done flag -- is allocated once per call in fixed shape, R = samples * beams (or chains)
slots; a round runs the step on ALL R rows (tokens = seq[t], the ancestor table and the rows' own sequences as strided views of the
state: the kernels already take them) and then ONE launch of csrc/beam.hip, which applies `_advance` and the finishing rules of
`beam_rounds` (or the chain rules of `sample_rounds`) in place.  Nothing is uploaded and nothing is read per round; every
`poll_every` rounds the B done flags are read so that a batch whose samples have all finished stops early (0 = never), and the
result does not depend on that.  A fixed number of reads at the end brings the state back and `rebuild_beams` / `rebuild_chains`
apply the final rules (`fin = final or beams`, `_best`) on the host.  The price is that rows of finished samples, ended beams and
the empty slots of round 0 still run (their outputs are ignored), and that context "last" has no (sample, token) memo: for
unconstrained "last" the memoised host loop stays the cheaper choice.  Beam size / chain count <= 8 and max_len <= 511 (ValueError
before any launch otherwise).  Scores are float64 sums in the host's order, ties break as the host's stable sort does: on equal step
outputs the results are equal; the step's GEMMs see other row counts than the host loop's, so on a real model scores may differ in
the last bits.
"""
import torch
import torch.nn.functional as F

from . import ops

__all__ = ["beam_search", "beam_search_ids", "beam_search_batch", "beam_search_ids_batch", "beam_rounds",
           "sample_rounds", "sample_ids_batch", "sample_batch", "make_sampler", "make_constraints", "beam_rounds_device",
           "sample_rounds_device", "rebuild_beams", "rebuild_chains"]

CONTEXTS = ("last", "prefix")


def _check_context(context):
    if context not in CONTEXTS:
        raise ValueError(f"context must be one of {CONTEXTS}, got {context!r}")


def _best(fin, length_penalty=0.0):
    """the final choice among [(score, seq)]: the highest score, the first among equals; with a length penalty the score is
    divided by (tokens after the start token) ** length_penalty first"""
    if length_penalty == 0:
        return sorted(fin, key=lambda c: c[0], reverse=True)[0]
    return sorted(fin, key=lambda c: c[0] / max(len(c[1]) - 1, 1) ** length_penalty, reverse=True)[0]


@torch.no_grad()
def beam_search_ids(model, start_id, sep_id, enc_ids, enc_mask, enc_type, add_mask, vis_embeds, roi_embeds, roi_coors,
                    beam_size=3, max_len=20, context="last", length_penalty=0.0, constraints=None, loop="host", poll_every=4):
    """-> (token ids of the best sequence incl. the start token, its log-likelihood, [(score, ids)] of the finished beams)
    context="prefix", constraints on, or loop="device": the batched path with this one sample (see the module header)"""
    _check_context(context)
    _check_loop(loop, beam_size, max_len)
    constraints = make_constraints(constraints)
    model.eval()
    if enc_ids.dim() == 1:                                    # one sample without a batch axis (:395-402)
        enc_ids, enc_mask, enc_type, add_mask = (t.unsqueeze(0) for t in (enc_ids, enc_mask, enc_type, add_mask))
        vis_embeds, roi_embeds, roi_coors = (t.unsqueeze(0) for t in (vis_embeds, roi_embeds, roi_coors))
    if context == "prefix" or constraints is not None or loop == "device":
        return beam_search_ids_batch(model, start_id, sep_id, enc_ids[:1], enc_mask[:1], enc_type[:1], add_mask[:1], vis_embeds[:1],
                                     roi_embeds[:1], roi_coors[:1], beam_size=beam_size, max_len=max_len, context=context,
                                     length_penalty=length_penalty, constraints=constraints, **_loop_kw(loop, poll_every))[0]
    enc = model.encoder(enc_ids, vis_embeds, roi_embeds, roi_coors, enc_type, enc_mask, add_mask)
    enc = enc[0] if isinstance(enc, tuple) else enc
    dec = model.decoder
    keys = dec.project_encoder(enc)                           # the blocks' cross-attention keys of this sample, once
    device = enc.device
    memo = {}

    def step(tok):
        """(top-k log-probabilities, top-k ids) after `tok`, as Python lists"""
        if tok not in memo:
            state = dec.init_state(enc, None)                 # (:436; valid lens None: no mask on either attention)
            logits = dec(torch.tensor([[tok]], device=device, dtype=torch.long), state, is_train=False, hoisted=keys)
            lp = F.log_softmax(logits[0, -1, :].float(), dim=-1)
            s, i = torch.topk(lp, beam_size)
            memo[tok] = (s.tolist(), i.tolist())
        return memo[tok]

    beams = [(0.0, [int(start_id)])]
    final = []
    for _ in range(max_len):
        cands = []
        for score, seq in beams:
            if seq[-1] == sep_id:                             # finished beams leave the search (:444-447)
                final.append((score, seq))
                continue
            top_s, top_i = step(seq[-1])
            for k in range(beam_size):
                cands.append((score + top_s[k], seq + [top_i[k]]))
        if not cands:
            break
        beams = sorted(cands, key=lambda c: c[0], reverse=True)[:beam_size]
        if all(seq[-1] == sep_id for _, seq in beams):        # (:500-502)
            final.extend(beams)
            break
    if not final:                                             # nothing finished within max_len (:505-506)
        final = list(beams)
    best_score, best_seq = _best(final, length_penalty)
    return best_seq, best_score, final


def beam_search(model, tokenizer, enc_ids, enc_mask, enc_type, add_mask, vis_embeds, roi_embeds, roi_coors,
                beam_size=3, num_preds=1, max_len=20, device='cuda', context="last", length_penalty=0.0, constraints=None,
                loop="host", poll_every=4):
    """the reference's signature and result: [decoded text of the best sequence] (fcmf_pretraining.py:383-517)"""
    start = tokenizer.bos_token_id if tokenizer.bos_token_id is not None else tokenizer.cls_token_id
    ids, _, _ = beam_search_ids(model, start, tokenizer.sep_token_id, enc_ids, enc_mask, enc_type, add_mask, vis_embeds,
                                roi_embeds, roi_coors, beam_size=beam_size, max_len=max_len, context=context,
                                length_penalty=length_penalty, constraints=constraints, **_loop_kw(loop, poll_every))
    return [tokenizer.decode(torch.tensor(ids), skip_special_tokens=True).strip()]


def _advance(beams, final, tops, sep_id, beam_size):
    """one round of one sample by `beam_search_ids`'s rules: finished beams move to `final` (:444-447), every other beam j is
    expanded by tops(j, seq) -> (top log-probabilities, top ids), the candidates are sorted by score, descending and stable (:493).
    -> None when no beam was live, else (the surviving beams [(score, seq)], for each the position j of its parent in `beams`)"""
    cands = []
    for j, (score, seq) in enumerate(beams):
        if seq[-1] == sep_id:                                 # finished beams leave the search (:444-447)
            final.append((score, seq))
            continue
        top_s, top_i = tops(j, seq)
        for k in range(beam_size):
            cands.append((score + top_s[k], seq + [top_i[k]], j))
    if not cands:
        return None
    best = sorted(cands, key=lambda c: c[0], reverse=True)[:beam_size]
    return [(score, seq) for score, seq, _ in best], [j for _, _, j in best]


def beam_rounds(step_many, num_samples, start_id, sep_id, beam_size=3, max_len=20, context="last", length_penalty=0.0,
                constraints=None):
    """the loop of `beam_search_ids` for `num_samples` samples side by side, on the host alone.  Per round: the (sample, last token)
    pairs of every live beam of every unfinished sample that the memo does not hold are collected (each once, in order of first
    appearance) and handed to ONE call step_many(pairs) -> {pair: (top log-probabilities, top ids)} (Python lists of at least
    beam_size entries); then every sample advances by exactly `beam_search_ids`'s rules: the same candidate order, the same stable
    sort, the same finishing rules, Python-float sums in the same order.  A sample whose beams are finished drops out.
    context="prefix": no memo.  Round t hands every live beam of every unfinished sample, in (sample, beam) order, to ONE call
    step_many(rows, t) -> [(top log-probabilities, top ids)] in row order, rows = [(sample, token at position t, ancestors)]:
    ancestors[p] is the index that the beam's position p had among the rows of round p (p < t) -- the step keeps what it needs of a
    row under (round, row index) and finds a beam's history there.  At most num_samples * beam_size rows per round.
    constraints not None (only whether it is None is read here): a step is a function of the beam's whole sequence, so there is no
    memo in either context -- every live beam is a row, in (sample, beam) order -- and every row carries the beam's own `seq` (all of
    length t + 1 in round t) as one more, last entry: "last" rows = [(sample, last token, seq)] with step_many(rows) -> a list in
    row order, "prefix" rows = [(sample, token, ancestors, seq)].
    -> [(ids of the best sequence incl. the start token, its score, the finished list [(score, ids)])], one entry per sample"""
    _check_context(context)
    prefix = context == "prefix"
    on = constraints is not None
    by_row = prefix or on                                     # every live beam is a row of its round: no memo
    memo = {}
    beams = [[(0.0, [int(start_id)])] for _ in range(num_samples)]
    anc = [[[]] for _ in range(num_samples)]                  # prefix mode: per beam, the rows that held its earlier positions
    final = [[] for _ in range(num_samples)]
    live = list(range(num_samples))
    for t in range(max_len):
        if not live:
            break
        if by_row:
            rows, row_of = [], {}
            for b in live:
                for j, (_, seq) in enumerate(beams[b]):
                    if seq[-1] != sep_id:
                        row_of[(b, j)] = len(rows)
                        rows.append((b, seq[-1]) + ((anc[b][j],) if prefix else ()) + ((seq,) if on else ()))
            tops_all = (step_many(rows, t) if prefix else step_many(rows)) if rows else []
        else:
            need = []
            for b in live:
                for _, seq in beams[b]:
                    pair = (b, seq[-1])
                    if seq[-1] != sep_id and pair not in memo and pair not in need:
                        need.append(pair)
            if need:
                memo.update(step_many(need))
        still = []
        for b in live:
            if by_row:
                adv = _advance(beams[b], final[b], lambda j, seq: tops_all[row_of[(b, j)]], sep_id, beam_size)
            else:
                adv = _advance(beams[b], final[b], lambda j, seq: memo[(b, seq[-1])], sep_id, beam_size)
            if adv is None:
                continue
            beams[b], parents = adv
            if all(seq[-1] == sep_id for _, seq in beams[b]):  # (:500-502)
                final[b].extend(beams[b])
                continue
            if prefix:
                anc[b] = [anc[b][j] + [row_of[(b, j)]] for j in parents]
            still.append(b)
        live = still
    out = []
    for b in range(num_samples):
        fin = final[b] if final[b] else list(beams[b])        # nothing finished within max_len (:505-506)
        best_score, best_seq = _best(fin, length_penalty)
        out.append((best_seq, best_score, fin))
    return out


def sample_rounds(step_many, num_samples, start_id, sep_id, num_chains=1, max_len=20, context="last", sample_offset=0,
                  length_penalty=0.0, constraints=None):
    """the sampling loop for `num_samples` samples side by side, on the host alone: every sample runs `num_chains` independent chains
    from [start_id]; round t hands every unfinished chain, in (sample, chain) order, to ONE call of the step and appends the token it
    draws; a chain ends at sep_id or after max_len draws.  A row carries its counter ((sample_offset + b) * num_chains + c) * max_len
    + t (sample_offset: the running index of sample 0 in the eval set), on which -- with the sampler's seed -- the draw depends.
    context="last":   step_many(rows) -> [(log-probability, token)] in row order, rows = [(sample, last token, counter)]; no memo, a
                      draw is no function of (sample, token).
    context="prefix": step_many(rows, t), rows = [(sample, token at position t, ancestors, counter)], ancestors[p] the index the
                      chain had among the rows of round p (as in `beam_rounds`; chains never branch).  At most num_samples *
                      num_chains rows per round.
    constraints not None (only whether it is None is read here): every row carries a copy of the chain's whole sequence as one
    more, last entry -- (sample, last token, counter, seq) / (sample, token, ancestors, counter, seq).
    A chain's score is the Python-float sum of the returned log-probabilities, in order.
    -> [(ids of the best chain incl. the start token, its score, [(score, ids)] of all chains in chain order)], one entry per sample;
    best = `_best` (the highest score, or the highest length-penalised one; the first chain among equals)"""
    _check_context(context)
    prefix = context == "prefix"
    seqs = [[[int(start_id)] for _ in range(num_chains)] for _ in range(num_samples)]
    scores = [[0.0] * num_chains for _ in range(num_samples)]
    anc = [[[] for _ in range(num_chains)] for _ in range(num_samples)]
    live = [(b, c) for b in range(num_samples) for c in range(num_chains)]
    for t in range(max_len):
        if not live:
            break
        ctr = [((sample_offset + b) * num_chains + c) * max_len + t for b, c in live]
        own = (lambda b, c: (list(seqs[b][c]),)) if constraints is not None else (lambda b, c: ())
        if prefix:
            res = step_many([(b, seqs[b][c][-1], anc[b][c], n) + own(b, c) for (b, c), n in zip(live, ctr)], t)
        else:
            res = step_many([(b, seqs[b][c][-1], n) + own(b, c) for (b, c), n in zip(live, ctr)])
        still = []
        for i, ((b, c), (lp, tok)) in enumerate(zip(live, res)):
            scores[b][c] += lp
            seqs[b][c].append(int(tok))
            anc[b][c].append(i)
            if tok != sep_id:
                still.append((b, c))
        live = still
    out = []
    for b in range(num_samples):
        chains = [(scores[b][c], seqs[b][c]) for c in range(num_chains)]
        best_score, best_seq = _best(chains, length_penalty)
        out.append((best_seq, best_score, chains))
    return out


LOOPS = ("host", "device")


def _check_loop(loop, width, max_len, what="beam_size"):
    if loop not in LOOPS:
        raise ValueError(f"loop must be one of {LOOPS}, got {loop!r}")
    if loop == "device":
        ops.check_advance(width, max_len, what)


def _loop_kw(loop, poll_every):
    """the keywords a wrapper hands on: none for the host loop, so that its callee is called with exactly the arguments it always got"""
    return {} if loop == "host" else dict(loop=loop, poll_every=poll_every)


def _run_device_rounds(st, round_fn, poll_every):
    """rounds 0 .. max_len-1 of a device loop; every `poll_every` rounds (0 = never) ONE read of `done` ([B] int32) ends the loop
    once every sample is done -- the rounds it saves change no slot and no finished list.  -> the rounds run"""
    if isinstance(poll_every, bool) or not isinstance(poll_every, int) or poll_every < 0:
        raise ValueError(f"poll_every must be an integer >= 0 (0 = never poll), got {poll_every}")
    for t in range(st["max_len"]):
        if poll_every and t and t % poll_every == 0 and bool(st["done"].all().item()):
            return t
        round_fn(t)
    return st["max_len"]


def rebuild_beams(score, state, seq, fin_count, fin_score, fin_len, fin_seq, beam_size, length_penalty=0.0):
    """`beam_rounds`' result from the final device state of `beam_rounds_device`, read back as host lists (`.tolist()` of the
    tensors of ops.advance_state: score / state [R], seq [max_len + 1][R], fin_count [B], fin_score / fin_len [B][>= count],
    fin_seq [B][>= count][max_len + 1]), by the host loop's rules:
      fin = final if final else beams -- the finished list in append order; a sample that finished nothing within max_len returns
      its beams in slot order, all max_len + 1 tokens long.  Beams that ended in the last round are in `fin` only in that second case:
      when `final` is non-empty they never reached it (slot state 2, not appended), as in the host loop;
      best = `_best` (first among equals, length penalty on request).
    -> [(best_seq, best_score, fin)], one entry per sample"""
    W = int(beam_size)
    out = []
    for b in range(len(fin_count)):
        n = fin_count[b]
        if n:
            fin = [(fin_score[b][e], list(fin_seq[b][e][:fin_len[b][e]])) for e in range(n)]
        else:
            # nothing finished: the sample ran every round, so every slot is filled (live or ended in the last round)
            fin = [(score[r], [row[r] for row in seq]) for r in range(b * W, b * W + W) if state[r] != ops.SLOT_EMPTY]
        best_score, best_seq = _best(fin, length_penalty)
        out.append((best_seq, best_score, fin))
    return out


def rebuild_chains(score, length, seq, num_chains, length_penalty=0.0):
    """`sample_rounds`' result from the final device state of `sample_rounds_device` as host lists (score / length [R], seq
    [max_len + 1][R]): per sample all chains in chain order, each its first `length` tokens, and `_best` among them"""
    W = int(num_chains)
    out = []
    for b in range(len(score) // W):
        chains = [(score[r], [seq[p][r] for p in range(length[r])]) for r in range(b * W, b * W + W)]
        best_score, best_seq = _best(chains, length_penalty)
        out.append((best_seq, best_score, chains))
    return out


@torch.no_grad()
def beam_rounds_device(step_rows, num_samples, start_id, sep_id, beam_size=3, max_len=20, context="last", length_penalty=0.0,
                       constraints=None, device=None, poll_every=4, return_state=False):
    """`beam_rounds` with the search state on the device from the start token to the final hypotheses (ops.advance_state,
    include/fcmf_hip.h fcmf_beam_advance): R = num_samples * beam_size fixed slots, slot b * beam_size + j beam j of sample b.
    Round t calls step_rows(tokens, t, anc, hist) -> (log-probabilities float32 [R, >= beam_size], ids int32 alike) on ALL R rows
    -- tokens = seq[t] (int64 [R], contiguous), anc the strided [R, t] ancestor view (slot indices: the key cache has R rows),
    hist the strided [R, t + 1] view of every slot's own sequence; all device tensors -- and then ONE launch of the advance
    kernel.  Rows of done samples, empty slots and ended beams run on valid tokens and their outputs are ignored.  Nothing is
    uploaded and nothing is read per round, except the poll: every `poll_every` rounds `done` ([B] int32) is read and the loop ends
    when all are set (0: never, run max_len rounds); the result does not depend on it.  `context` and `constraints` are checked and
    otherwise left to the step.  At the end a fixed number of reads, whatever max_len, bring back the slots and the finished lists,
    and `rebuild_beams` applies the host loop's final rules.  -> `beam_rounds`' result; with return_state also the state dict"""
    _check_context(context)
    st = ops.advance_state(num_samples, beam_size, max_len, start_id, device)
    seq, anc = st["seq"], st["anc"]

    def one_round(t):
        logp, ids = step_rows(seq[t], t, anc[:t].t(), seq[:t + 1].t())
        ops.beam_advance(logp, ids, st, t, sep_id)

    _run_device_rounds(st, one_round, poll_every)
    counts = st["fin_count"].cpu()
    n = max(int(counts.max()) if counts.numel() else 0, 1)
    res = rebuild_beams(st["score"].cpu().tolist(), st["state"].cpu().tolist(), seq.cpu().tolist(), counts.tolist(),
                        st["fin_score"][:, :n].cpu().tolist(), st["fin_len"][:, :n].cpu().tolist(),
                        st["fin_seq"][:, :n].cpu().tolist(), beam_size, length_penalty)
    return (res, st) if return_state else res


@torch.no_grad()
def sample_rounds_device(step_rows, num_samples, start_id, sep_id, num_chains=1, max_len=20, context="last", sample_offset=0,
                         length_penalty=0.0, constraints=None, device=None, poll_every=4, return_state=False):
    """`sample_rounds` with the chains on the device (fcmf_chain_advance), as `beam_rounds_device`: R = num_samples * num_chains
    slots, every round all R rows.  step_rows(tokens, t, anc, hist, ctr) -> (log-probability float32, id int32) of [R] or [R, 1]:
    ctr int64 [R] is row t of the counter table ((sample_offset + b) * num_chains + c) * max_len + t, formed ONCE per call as
    [max_len, R].  A chain that has ended keeps its score and length; its row still runs and is ignored."""
    _check_context(context)
    st = ops.advance_state(num_samples, num_chains, max_len, start_id, device, chains=True)
    seq, anc = st["seq"], st["anc"]
    R = st["B"] * st["W"]
    ctr = ((int(sample_offset) * num_chains + torch.arange(R, dtype=torch.int64)).view(1, R) * max_len +
           torch.arange(max_len, dtype=torch.int64).view(max_len, 1)).to(device)      # the ONE upload of the call

    def one_round(t):
        logp, ids = step_rows(seq[t], t, anc[:t].t(), seq[:t + 1].t(), ctr[t])
        ops.chain_advance(logp, ids, st, t, sep_id)

    _run_device_rounds(st, one_round, poll_every)
    res = rebuild_chains(st["score"].cpu().tolist(), st["len"].cpu().tolist(), seq.cpu().tolist(), num_chains, length_penalty)
    return (res, st) if return_state else res


@torch.no_grad()
def beam_search_ids_batch(model, start_id, sep_id, enc_ids, enc_mask, enc_type, add_mask, vis_embeds, roi_embeds, roi_coors,
                          beam_size=3, max_len=20, context="last", length_penalty=0.0, constraints=None, loop="host", poll_every=4):
    """`beam_search_ids` of every sample of a batch ([B, ...] tensors), one decoder call per beam round for all of them: the encoder
    and `project_encoder` run once for the batch.  context="prefix": every step sees its beam's whole prefix (module header); the
    key cache is allocated here, once per batch.  constraints: `make_constraints`' settings (module header): the rows' sequences
    ride in the round's one upload.  loop="device": the search state lives on the device (`beam_rounds_device`; beam_size <= 8),
    every round runs all B * beam_size rows and nothing is uploaded or read per round but the poll every `poll_every` rounds; in
    context "last" that is `decode_step` on every row with no memo, as the constrained path -- for unconstrained "last" the memoised
    host loop remains the cheaper choice.  -> [(ids, score, final)], one entry per sample"""
    _check_context(context)
    _check_loop(loop, beam_size, max_len)
    constraints = make_constraints(constraints)
    _check_room(constraints, model.decoder.dense.weight.shape[0], max_len, beam_size)
    model.eval()
    enc = model.encoder(enc_ids, vis_embeds, roi_embeds, roi_coors, enc_type, enc_mask, add_mask)
    enc = enc[0] if isinstance(enc, tuple) else enc
    dec = model.decoder
    keys = dec.project_encoder(enc)
    device = enc.device
    cons = _device_constraints(constraints, sep_id, device)   # the suppressed ids: ONE upload per call

    if loop == "device":
        rows = enc_ids.shape[0] * beam_size
        sample_idx = torch.arange(rows, device=device) // beam_size          # constant over the rounds, formed on the device
        cache = dec.init_cache(max_len, rows, device) if context == "prefix" else None

        def step_dev(tokens, t, anc, hist):
            own = None if cons is None else dict(cons, hist=hist)
            if cache is None:
                return dec.decode_step(tokens, sample_idx, enc, keys, beam_size, constraints=own)
            return dec.decode_step_prefix(tokens, sample_idx, anc, t, cache, enc, keys, beam_size, constraints=own)

        return beam_rounds_device(step_dev, enc_ids.shape[0], start_id, sep_id, beam_size, max_len, context, length_penalty,
                                  constraints, device, poll_every)

    def read(logp, ids):
        both = torch.cat((logp, ids.view(torch.float32)), dim=1).cpu()      # ONE host read: the ids ride along as their bits
        return list(zip(both[:, :beam_size].tolist(), both[:, beam_size:].contiguous().view(torch.int32).tolist()))

    def step_many(pairs):
        idx = torch.tensor(pairs, device=device, dtype=torch.long)          # [n, 2]: (sample, token)
        logp, ids = dec.decode_step(idx[:, 1].contiguous(), idx[:, 0].contiguous(), enc, keys, beam_size)
        both = torch.cat((logp, ids.view(torch.float32)), dim=1).cpu()      # ONE host read: the ids ride along as their bits
        top_s, top_i = both[:, :beam_size].tolist(), both[:, beam_size:].contiguous().view(torch.int32).tolist()
        return {p: (s, i) for p, s, i in zip(pairs, top_s, top_i)}

    if context == "prefix":
        cache = dec.init_cache(max_len, enc_ids.shape[0] * beam_size, device)

        def step_rows(rows, t):
            # ONE upload, [2 + t, n]: the samples, the tokens, then the ancestor table position by position (its transpose is the
            # kernel's [n, t] view: it takes any strides)
            buf = torch.tensor([[r[0] for r in rows], [r[1] for r in rows]] + [[r[2][p] for r in rows] for p in range(t)],
                               device=device, dtype=torch.long)
            logp, ids = dec.decode_step_prefix(buf[1], buf[0], buf[2:].t(), t, cache, enc, keys, beam_size)
            both = torch.cat((logp, ids.view(torch.float32)), dim=1).cpu()      # ONE host read, as above
            return list(zip(both[:, :beam_size].tolist(), both[:, beam_size:].contiguous().view(torch.int32).tolist()))

        def step_rows_seq(rows, t):
            # ONE upload, [2 + t + (t + 1), n]: as above, then the rows' own sequences position by position (the kernel's [n, t + 1] view)
            buf = torch.tensor([[r[0] for r in rows], [r[1] for r in rows]] + [[r[2][p] for r in rows] for p in range(t)] +
                               [[r[3][p] for r in rows] for p in range(t + 1)], device=device, dtype=torch.long)
            return read(*dec.decode_step_prefix(buf[1], buf[0], buf[2:2 + t].t(), t, cache, enc, keys, beam_size,
                                                constraints=dict(cons, hist=buf[2 + t:].t())))

        return beam_rounds(step_rows if cons is None else step_rows_seq, enc_ids.shape[0], start_id, sep_id, beam_size, max_len, context,
                           length_penalty, constraints)

    def step_seq(rows):
        # ONE upload, [2 + L, n]: the samples, the tokens, then the rows' own sequences position by position
        buf = torch.tensor([[r[0] for r in rows], [r[1] for r in rows]] + [[r[2][p] for r in rows] for p in range(len(rows[0][2]))],
                           device=device, dtype=torch.long)
        return read(*dec.decode_step(buf[1], buf[0], enc, keys, beam_size, constraints=dict(cons, hist=buf[2:].t())))

    return beam_rounds(step_many if cons is None else step_seq, enc_ids.shape[0], start_id, sep_id, beam_size, max_len,
                       length_penalty=length_penalty, constraints=constraints)


def beam_search_batch(model, tokenizer, enc_ids, enc_mask, enc_type, add_mask, vis_embeds, roi_embeds, roi_coors,
                      beam_size=3, max_len=20, context="last", length_penalty=0.0, constraints=None, loop="host", poll_every=4):
    """-> [decoded text of the best sequence], one per sample of the batch (what `beam_search` returns per sample, [0])"""
    start = tokenizer.bos_token_id if tokenizer.bos_token_id is not None else tokenizer.cls_token_id
    res = beam_search_ids_batch(model, start, tokenizer.sep_token_id, enc_ids, enc_mask, enc_type, add_mask, vis_embeds,
                                roi_embeds, roi_coors, beam_size=beam_size, max_len=max_len, context=context,
                                length_penalty=length_penalty, constraints=constraints, **_loop_kw(loop, poll_every))
    return [tokenizer.decode(torch.tensor(ids), skip_special_tokens=True).strip() for ids, _, _ in res]


def make_constraints(constraints=None, **settings):
    """the constraint settings of every entry point as a checked dict -- repetition_penalty (1 = off), no_repeat_ngram_size (0 = off),
    min_length (0 = off), suppress_tokens (a tuple of ids, () = off) -- from a dict and / or keywords; None when all are off"""
    out = dict(repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0, suppress_tokens=())
    given = dict(constraints or {}, **settings)
    extra = set(given) - set(out)
    if extra:
        raise ValueError(f"constraints: unknown settings {sorted(extra)} (known: {sorted(out)})")
    out.update(given)
    if isinstance(out["suppress_tokens"], (str, bytes)) or not hasattr(out["suppress_tokens"], "__iter__"):
        raise ValueError(f"suppress_tokens must be a sequence of token ids, got {out['suppress_tokens']!r}")
    out["suppress_tokens"] = tuple(out["suppress_tokens"])
    ops.check_constraints(**out)
    if out["repetition_penalty"] == 1 and not out["no_repeat_ngram_size"] and not out["min_length"] and not out["suppress_tokens"]:
        return None
    return out


def _check_room(constraints, V, max_len, width):
    """constraints on: a round's sequence must fit the kernel, and `width` columns must stay unbanned whatever is decoded -- at most
    max_len n-gram bans, the separator and the suppressed ids can be -inf"""
    if constraints is None:
        return
    if max_len > ops.CONSTRAIN_MAX_T:
        raise ValueError(f"constraints: max_len {max_len} is beyond the constraint kernel's {ops.CONSTRAIN_MAX_T} tokens")
    n_ban = len(constraints["suppress_tokens"])
    if V < max_len + 1 + n_ban + width:
        raise ValueError(f"constraints: a vocabulary of {V} cannot keep {width} tokens unbanned beside up to {max_len} n-gram bans, the "
                         f"separator and {n_ban} suppressed ids (needs >= {max_len + 1 + n_ban + width})")


def _device_constraints(constraints, sep_id, device):
    """`make_constraints`' dict as ops.logits_constrain's keyword arguments but `hist`: the suppressed ids go to the device here, once"""
    if constraints is None:
        return None
    ban = constraints["suppress_tokens"]
    return dict(repetition_penalty=constraints["repetition_penalty"], no_repeat_ngram_size=constraints["no_repeat_ngram_size"],
                min_length=constraints["min_length"], sep_id=int(sep_id),
                ban_ids=torch.tensor(ban, device=device, dtype=torch.int32) if ban else None)


def make_sampler(sampler=None):
    """the sampler settings of the sampling entry points as a checked dict: seed (0), temperature (1), top_k (0 = off), top_p (1 = off)"""
    out = dict(seed=0, temperature=1.0, top_k=0, top_p=1.0)
    extra = set(sampler or ()) - set(out)
    if extra:
        raise ValueError(f"sampler: unknown settings {sorted(extra)} (known: {sorted(out)})")
    out.update(sampler or {})
    ops.check_sampler(out["temperature"], out["top_k"], out["top_p"])
    return out


@torch.no_grad()
def sample_ids_batch(model, start_id, sep_id, enc_ids, enc_mask, enc_type, add_mask, vis_embeds, roi_embeds, roi_coors,
                     num_chains=1, max_len=20, context="last", sampler=None, sample_offset=0, length_penalty=0.0, constraints=None,
                     loop="host", poll_every=4):
    """`sample_rounds` of every sample of a batch ([B, ...] tensors) over the batched decode steps: the encoder and `project_encoder`
    run once for the batch, every round is ONE upload (samples, tokens, counters and, in prefix mode, the ancestor table), one decoder
    call ending in csrc/sample.hip and ONE host read.  sampler: `make_sampler`'s settings; sample_offset: the running index of the
    batch's first sample in the eval set; constraints: `make_constraints`' settings (module header).  loop="device": the chains
    live on the device (`sample_rounds_device`; num_chains <= 8): all B * num_chains rows run every round, the counters are uploaded
    once per call, nothing is read per round but the poll.  -> [(ids of the best chain, its score, [(score, ids)] of all chains)], one entry per sample"""
    _check_context(context)
    if num_chains < 1:
        raise ValueError(f"num_chains must be >= 1, got {num_chains}")
    _check_loop(loop, num_chains, max_len, "num_chains")
    cfg = make_sampler(sampler)
    constraints = make_constraints(constraints)
    _check_room(constraints, model.decoder.dense.weight.shape[0], max_len, 1)
    model.eval()
    enc = model.encoder(enc_ids, vis_embeds, roi_embeds, roi_coors, enc_type, enc_mask, add_mask)
    enc = enc[0] if isinstance(enc, tuple) else enc
    dec = model.decoder
    keys = dec.project_encoder(enc)
    device = enc.device
    cons = _device_constraints(constraints, sep_id, device)   # the suppressed ids: ONE upload per call

    if loop == "device":
        rows = enc_ids.shape[0] * num_chains
        sample_idx = torch.arange(rows, device=device) // num_chains         # constant over the rounds, formed on the device
        cache = dec.init_cache(max_len, rows, device) if context == "prefix" else None

        def step_dev(tokens, t, anc, hist, ctr):
            own = None if cons is None else dict(cons, hist=hist)
            if cache is None:
                return dec.decode_step(tokens, sample_idx, enc, keys, 1, sampler=dict(cfg, ctr=ctr), constraints=own)
            return dec.decode_step_prefix(tokens, sample_idx, anc, t, cache, enc, keys, 1, sampler=dict(cfg, ctr=ctr), constraints=own)

        return sample_rounds_device(step_dev, enc_ids.shape[0], start_id, sep_id, num_chains, max_len, context, sample_offset,
                                    length_penalty, constraints, device, poll_every)

    def read(logp, ids):
        both = torch.cat((logp, ids.view(torch.float32)), dim=1).cpu()      # ONE host read: the ids ride along as their bits
        return list(zip(both[:, 0].tolist(), both[:, 1].contiguous().view(torch.int32).tolist()))

    if context == "prefix":
        cache = dec.init_cache(max_len, enc_ids.shape[0] * num_chains, device)

        def step_rows(rows, t):
            # ONE upload, [3 + t, n]: the samples, the tokens, the counters, then the ancestor table position by position
            buf = torch.tensor([[r[0] for r in rows], [r[1] for r in rows], [r[3] for r in rows]] + [[r[2][p] for r in rows] for p in range(t)],
                               device=device, dtype=torch.long)
            return read(*dec.decode_step_prefix(buf[1], buf[0], buf[3:].t(), t, cache, enc, keys, 1, sampler=dict(cfg, ctr=buf[2])))

        def step_rows_seq(rows, t):
            # ONE upload, [3 + t + (t + 1), n]: as above, then the chains' own sequences position by position
            buf = torch.tensor([[r[0] for r in rows], [r[1] for r in rows], [r[3] for r in rows]] + [[r[2][p] for r in rows] for p in range(t)] +
                               [[r[4][p] for r in rows] for p in range(t + 1)], device=device, dtype=torch.long)
            return read(*dec.decode_step_prefix(buf[1], buf[0], buf[3:3 + t].t(), t, cache, enc, keys, 1, sampler=dict(cfg, ctr=buf[2]),
                                                constraints=dict(cons, hist=buf[3 + t:].t())))

        return sample_rounds(step_rows if cons is None else step_rows_seq, enc_ids.shape[0], start_id, sep_id, num_chains, max_len, context,
                             sample_offset, length_penalty, constraints)

    def step_many(rows):
        buf = torch.tensor(rows, device=device, dtype=torch.long).t().contiguous()      # ONE upload, [3, n]: samples, tokens, counters
        return read(*dec.decode_step(buf[1], buf[0], enc, keys, 1, sampler=dict(cfg, ctr=buf[2])))

    def step_seq(rows):
        # ONE upload, [3 + L, n]: samples, tokens, counters, then the chains' own sequences position by position
        buf = torch.tensor([[r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]] +
                           [[r[3][p] for r in rows] for p in range(len(rows[0][3]))], device=device, dtype=torch.long)
        return read(*dec.decode_step(buf[1], buf[0], enc, keys, 1, sampler=dict(cfg, ctr=buf[2]), constraints=dict(cons, hist=buf[3:].t())))

    return sample_rounds(step_many if cons is None else step_seq, enc_ids.shape[0], start_id, sep_id, num_chains, max_len, context,
                         sample_offset, length_penalty, constraints)


def sample_batch(model, tokenizer, enc_ids, enc_mask, enc_type, add_mask, vis_embeds, roi_embeds, roi_coors,
                 num_chains=1, max_len=20, context="last", sampler=None, sample_offset=0, length_penalty=0.0, constraints=None,
                 loop="host", poll_every=4):
    """-> [decoded text of the best chain], one per sample of the batch: `beam_search_batch`'s result from `sample_ids_batch`"""
    start = tokenizer.bos_token_id if tokenizer.bos_token_id is not None else tokenizer.cls_token_id
    res = sample_ids_batch(model, start, tokenizer.sep_token_id, enc_ids, enc_mask, enc_type, add_mask, vis_embeds, roi_embeds,
                           roi_coors, num_chains=num_chains, max_len=max_len, context=context, sampler=sampler,
                           sample_offset=sample_offset, length_penalty=length_penalty, constraints=constraints,
                           **_loop_kw(loop, poll_every))
    return [tokenizer.decode(torch.tensor(ids), skip_special_tokens=True).strip() for ids, _, _ in res]
