// Beam and chain bookkeeping of the IAOG decode on the device (see include/fcmf_hip.h, fcmf_beam_advance / fcmf_chain_advance):
// round t of `decoding._advance` and the rules around it in `decoding.beam_rounds` / `sample_rounds`, for every sample in one
// launch, on state that never leaves the device.  The work is a few KB per sample and latency bound: ONE wave per sample.
//   beam round, the wave of sample b (slots b*W .. b*W + W-1 of the R = B*W rows):
//     1. ended beams go to the sample's finished list in beam order (a ballot gives every ended beam its place); their
//        sequences are copied lanes-across-positions;
//     2. lane c = j*W + k holds candidate (beam j, k-th top token): score[j] + (double)logp[j, k], valid when beam j is live.
//        Lane order IS the host's candidate order (j ascending, k ascending);
//     3. rank by counting over the <= 64 candidates in LDS: the number of valid candidates that are larger, or equal and
//        earlier -- the position a stable descending sort gives.  Ranks 0 .. W-1 survive;
//     4. the history moves in place.  Children are written into the slots their parents are read from, and parents may
//        permute or repeat.  A lane owns whole POSITIONS: it loads the W parent entries of its position into registers, then
//        stores the W children, and touches no other position -- no lane ever reads what another lane writes;
//     5. the new token, the parent's slot as the ancestor of position t, score and state; if every new beam ended they are
//        appended to the finished list (their history comes from the registers of step 4) and the sample is done.
//   Rows of a done sample, and a sample that has no candidates, get seq[t+1] = seq[t] and anc[t] = their own slot: the step can
//   run all R rows every round on valid tokens and indices.
// One workgroup owns a sample's finished list and done[b]; no atomics; the order of every store is fixed: two launches give the
// same bits.  Plain vector stores only.
#include <math.h>

#include "common.h"

constexpr int BEAM_MAX_W = 8, BEAM_MAX_T = 512;
constexpr int SLOT_EMPTY = 0, SLOT_LIVE = 1, SLOT_ENDED = 2;

struct BeamK {
  const float* logp;
  const int32_t* ids;
  int64_t ld;
  int B, W, t, max_len, sep;
  int64_t* seq;
  int64_t* anc;
  double* score;
  int32_t* state;
  double* fin_score;
  int64_t* fin_seq;
  int32_t* fin_len;
  int32_t* fin_count;
  int32_t* done;
};

// the rows of a sample that does not advance: a valid token and ancestor for the next step
__device__ __forceinline__ void hold_rows(int64_t* seq, int64_t* anc, int64_t R, int r0, int W, int t, int lane) {
  if (lane < W) {
    seq[(int64_t)(t + 1) * R + r0 + lane] = seq[(int64_t)t * R + r0 + lane];
    anc[(int64_t)t * R + r0 + lane] = r0 + lane;
  }
}

// grid = B, 64 threads (one wave)
__global__ __launch_bounds__(64) void beam_advance_kernel(BeamK P) {
  __shared__ double c_score[64];
  __shared__ int c_ok[64];
  __shared__ double n_score[BEAM_MAX_W];
  __shared__ int n_par[BEAM_MAX_W], n_id[BEAM_MAX_W];
  const int lane = threadIdx.x, b = blockIdx.x, W = P.W, t = P.t;
  const int64_t R = (int64_t)P.B * W;
  const int r0 = b * W, S = P.max_len + 1;
  const int64_t cap = (int64_t)W * S;
  if (P.done[b]) {
    hold_rows(P.seq, P.anc, R, r0, W, t, lane);
    return;
  }

  // ---- 1. ended beams leave for the finished list, in beam order
  const int st = lane < W ? P.state[r0 + lane] : SLOT_EMPTY;
  const unsigned long long ended = __ballot(st == SLOT_ENDED);
  int count = P.fin_count[b];
  if (ended) {
    if (st == SLOT_ENDED) {
      const int64_t e = count + __popcll(ended & ((1ull << lane) - 1));
      if (e < cap) {
        P.fin_score[b * cap + e] = P.score[r0 + lane];
        P.fin_len[b * cap + e] = t + 1;
      }
    }
    int e = count;
    for (int j = 0; j < W; ++j) {
      if (!((ended >> j) & 1)) continue;
      if (e < cap)
        for (int p = lane; p <= t; p += 64) P.fin_seq[(b * cap + e) * S + p] = P.seq[(int64_t)p * R + r0 + j];
      ++e;
    }
    count = e < cap ? e : (int)cap;
  }

  // ---- 2. the candidates, one per lane, in the host's order
  const int cj = lane / W, ck = lane - cj * W;
  bool ok = false;
  double sc = 0.0;
  int id = 0;
  if (cj < W) {
    ok = P.state[r0 + cj] == SLOT_LIVE;
    sc = P.score[r0 + cj] + (double)P.logp[(int64_t)(r0 + cj) * P.ld + ck];
    id = P.ids[(int64_t)(r0 + cj) * P.ld + ck];
  }
  if (!__ballot(ok)) {                                        // no beam was live: the sample is done, its beams stay
    if (lane == 0) { P.fin_count[b] = count; P.done[b] = 1; }
    hold_rows(P.seq, P.anc, R, r0, W, t, lane);
    return;
  }
  c_score[lane] = sc;
  c_ok[lane] = ok;
  __syncthreads();

  // ---- 3. rank by counting: stable, descending
  int rank = 0;
  for (int c = 0; c < 64; ++c) {
    const double o = c_score[c];
    rank += c_ok[c] && (o > sc || (o == sc && c < lane));
  }
  if (ok && rank < W) { n_score[rank] = sc; n_par[rank] = cj; n_id[rank] = id; }
  __syncthreads();

  bool all_ended = true;
  for (int i = 0; i < W; ++i) all_ended &= n_id[i] == P.sep;
  const bool room = count + W <= cap;                         // always, by the bound of the header; guards the stores all the same

  // ---- 4. history in place: a lane owns its positions, reads the W parents of one, then writes the W children
  for (int p = lane; p <= t; p += 64) {
    int64_t* sp = P.seq + (int64_t)p * R + r0;
    int64_t* ap = P.anc + (int64_t)p * R + r0;
    int64_t v[BEAM_MAX_W], a[BEAM_MAX_W];
#pragma unroll
    for (int i = 0; i < BEAM_MAX_W; ++i) {
      v[i] = 0; a[i] = 0;
      if (i < W) {
        v[i] = sp[n_par[i]];
        if (p < t) a[i] = ap[n_par[i]];
      }
    }
#pragma unroll
    for (int i = 0; i < BEAM_MAX_W; ++i) {
      if (i < W) {
        sp[i] = v[i];
        if (p < t) ap[i] = a[i];
        if (all_ended && room) P.fin_seq[(b * cap + count + i) * S + p] = v[i];
      }
    }
  }

  // ---- 5. the new position, score and state
  if (lane < W) {
    const int nid = n_id[lane];
    P.seq[(int64_t)(t + 1) * R + r0 + lane] = nid;
    P.anc[(int64_t)t * R + r0 + lane] = r0 + n_par[lane];
    P.score[r0 + lane] = n_score[lane];
    P.state[r0 + lane] = nid == P.sep ? SLOT_ENDED : SLOT_LIVE;
    if (all_ended && room) {
      P.fin_seq[(b * cap + count + lane) * S + t + 1] = nid;
      P.fin_score[b * cap + count + lane] = n_score[lane];
      P.fin_len[b * cap + count + lane] = t + 2;
    }
  }
  if (lane == 0) {
    P.fin_count[b] = count + (all_ended && room ? W : 0);
    if (all_ended) P.done[b] = 1;
  }
}

struct ChainK {
  const float* logp;
  const int32_t* ids;
  int B, W, t, sep;
  int64_t* seq;
  int64_t* anc;
  double* score;
  int32_t* state;
  int32_t* len;
  int32_t* done;
};

// grid = B, 64 threads (one wave): lane c is chain c of the sample
__global__ __launch_bounds__(64) void chain_advance_kernel(ChainK P) {
  const int lane = threadIdx.x, b = blockIdx.x, W = P.W, t = P.t;
  const int64_t R = (int64_t)P.B * W;
  const int r = b * W + lane;
  bool open = false;                                          // still live after this round
  if (lane < W) {
    int64_t tok = P.seq[(int64_t)t * R + r];                  // an ended chain repeats its last token: valid for the step
    if (P.state[r] == SLOT_LIVE) {
      tok = P.ids[r];
      P.score[r] += (double)P.logp[r];
      P.len[r] = t + 2;
      open = tok != P.sep;
      if (!open) P.state[r] = SLOT_ENDED;
    }
    P.seq[(int64_t)(t + 1) * R + r] = tok;
    P.anc[(int64_t)t * R + r] = r;
  }
  const unsigned long long any_open = __ballot(open);
  if (lane == 0 && !any_open) P.done[b] = 1;
}

static int advance_args(int B, int W, int t, int max_len) {
  if (B < 0 || W < 0 || t < 0 || max_len < 0) return FCMF_ERR_ARG;
  if (W < 1 || W > BEAM_MAX_W || max_len < 1 || max_len + 1 > BEAM_MAX_T) return FCMF_ERR_UNSUPPORTED;
  if (t >= max_len) return FCMF_ERR_ARG;
  return FCMF_OK;
}

extern "C" int fcmf_beam_advance(const float* logp, const int32_t* ids, int64_t ld, int B, int W, int t, int max_len, int sep_id,
                                 int64_t* seq, int64_t* anc, double* score, int32_t* state, double* fin_score, int64_t* fin_seq,
                                 int32_t* fin_len, int32_t* fin_count, int32_t* done, void* stream) {
  if (!logp || !ids || !seq || !anc || !score || !state || !fin_score || !fin_seq || !fin_len || !fin_count || !done)
    return FCMF_ERR_ARG;
  const int rc = advance_args(B, W, t, max_len);
  if (rc != FCMF_OK) return rc;
  if (ld < W) return FCMF_ERR_ARG;
  if (B == 0) return FCMF_OK;
  BeamK P{};
  P.logp = logp; P.ids = ids; P.ld = ld; P.B = B; P.W = W; P.t = t; P.max_len = max_len; P.sep = sep_id;
  P.seq = seq; P.anc = anc; P.score = score; P.state = state;
  P.fin_score = fin_score; P.fin_seq = fin_seq; P.fin_len = fin_len; P.fin_count = fin_count; P.done = done;
  return fcmf_launch(beam_advance_kernel, dim3(B), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), P);
}

extern "C" int fcmf_chain_advance(const float* logp, const int32_t* ids, int B, int W, int t, int max_len, int sep_id, int64_t* seq,
                                  int64_t* anc, double* score, int32_t* state, int32_t* len, int32_t* done, void* stream) {
  if (!logp || !ids || !seq || !anc || !score || !state || !len || !done) return FCMF_ERR_ARG;
  const int rc = advance_args(B, W, t, max_len);
  if (rc != FCMF_OK) return rc;
  if (B == 0) return FCMF_OK;
  ChainK P{};
  P.logp = logp; P.ids = ids; P.B = B; P.W = W; P.t = t; P.sep = sep_id;
  P.seq = seq; P.anc = anc; P.score = score; P.state = state; P.len = len; P.done = done;
  return fcmf_launch(chain_advance_kernel, dim3(B), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), P);
}
