// MFMA attention for the text-encoder layers: bf16, head dim 64, up to 256 queries / keys per (sequence, head)
// (128: FCMF-base; 256: FCMF-large, in the <2,2> / 256-key instantiations further down).
//   forward : one workgroup per (sequence, head, 128-query tile); K and V tiles staged once in LDS;
//             each of the 4 waves owns 32 query rows: S^T = K Q^T on v_mfma_f32_16x16x32_bf16 with the
//             key index in the accumulator registers (row max / sum = 32 in-lane values + 2 shuffles);
//             the normalised, dropped-out P^T accumulators ARE the operand of O^T = V^T P^T (keys taken in
//             the order the accumulator registers hold them; V is consumed through ds_read_b64_tr_b16 in
//             that same order straight from its row-major image): 32 KiB of LDS, four workgroups per CU.
//   backward: one workgroup per (sequence, head), Tq <= 128: P is recomputed from the saved logsumexp.
//             The keys go by in chunks of 32: phase 1 (wave = 32 query rows) builds Pdrop^T and dS^T
//             [key][query] of the chunk in LDS, phase 2 adds the chunk to dQ (wave = 32 queries, accumulators
//             live across chunks) and finishes dV / dK of the chunk's keys (wave = 16 head-dim columns, the
//             transposed dO / Q operands stay in registers).  80 KiB of LDS: two workgroups per CU overlap
//             each other's loads, barriers and stores; no atomics.  Every global read of a workgroup (tiles, O rows,
//             lse, mask row) is requested in one batch up front and the chunk loop holds no load and no wait on the
//             vector-memory counter, so its stores drain under the next chunk; dq / dk / dv leave as whole 128-byte
//             rows, put together in LDS that is dead by then.
// One LDS image per tile serves both row reads (ds_read_b128) and transposed reads
// (ds_read_b64_tr_b16); swizzles verified conflict-free with tools/lds_conflicts.py.
#include "attn_tiles.h"
#include <cstdlib>

// =========================================================================================
// NKT = 128-key tiles per (sequence, head): 1 (Tk <= 128: 32 KiB of LDS, three workgroups per CU) or 2 (Tk <= 256: the
// FCMF-large text encoder, 64 KiB, two per CU).  The images of the second tile lie right behind the first (row r of the
// 256-row image = row r - 128 of the second tile: the swizzle keys only use row bits 1..3).

// one (sequence, head, 128-query tile) from the staged K / V images: scores, softmax, dropout, P V, store
// (mask_lds != NULL: the additive key mask of the tile was staged in LDS with K / V -- the persistent kernel must not issue a
// global load inside the tile: the counter of vector-memory operations retires in order, so waiting for it would also wait
// for the next tile's operands that are in flight behind it)
// The tile in two halves, arithmetic and stores, so that the persistent kernel can put the wait for the NEXT tile's operands
// between them: oc = O^T accumulators, lv[f] = logsumexp of query q0 + 16 f + (lane & 15), stored by the first half unless
// LSE_LATE (the one-tile kernels, which have no such wait, keep their registers: fwd256 fits three workgroups per CU only so).
template <int NKT, bool LSE_LATE>
__device__ __forceinline__ void attn_mfma_fwd_tile_compute(const AttnMfmaParams& P, int g, int h, int q0, int lane, const bf16x8 (&qf)[2][2],
                                                           const char* Ks, const char* Vs, const float* mask_lds, f32x4 (&oc)[4][2],
                                                           float (&lv)[2]) {
  constexpr int NKF = 8 * NKT;       // 16-key fragments
  const float* mrow = P.mask ? P.mask + (int64_t)g * P.Tk : nullptr;
  // trailing keys under the "hard" additive mask (<= -1e30: HF's finfo.min padding mask) get probabilities that are EXACTLY
  // zero: their 16-key fragments (scores, softmax terms, P V steps) are skipped with bit-identical results.
  // nvalid = index of the last key that is not hard-masked, + 1 (wave-uniform).
  int nvalid = P.Tk;
  if (mask_lds || mrow) {
    const int last = last_live_key<2 * NKT>([&](int, int key) { return mask_lds ? mask_lds[key] : mrow[key]; }, P.Tk, lane);
    nvalid = last >= 0 ? last + 1 : P.Tk;    // no live key at all: nothing may be skipped (softmax over finfo.min scores is uniform over ALL keys)
  }
  // S^T[key][q]: NKF key fragments x 2 query fragments
  f32x4 sc[NKF][2];
  fwd_score_frags<NKF>([&](int x0, int s) { return frag_row64(Ks, x0, s, lane); }, qf, nvalid, sc);
  // lane holds, for query q0+16f+(lane&15), keys 16kf + 4(lane>>4) + r
  const float inv_keep = P.p > 0.f ? 1.0f / (1.0f - P.p) : 1.0f;
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    const int q = q0 + 16 * f + (lane & 15);
    float m = -INFINITY;
#pragma unroll
    for (int kf = 0; kf < NKF; ++kf) {
      if (16 * kf >= nvalid) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = 16 * kf + 4 * (lane >> 4) + r;
        float s = -INFINITY;
        if (key < P.Tk) s = sc[kf][f][r] * P.scale + (mask_lds ? mask_lds[key] : (mrow ? mrow[key] : 0.f));
        sc[kf][f][r] = s;
        m = fmaxf(m, s);
      }
    }
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    float sum = 0.f;
#pragma unroll
    for (int kf = 0; kf < NKF; ++kf) {
      if (16 * kf >= nvalid) continue;         // (sc of a skipped fragment stays 0 = its probabilities)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float e = __expf(sc[kf][f][r] - m);
        sc[kf][f][r] = e;
        sum += e;
      }
    }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    const float inv = 1.0f / sum;
    lv[f] = m + __logf(sum);
    if (!LSE_LATE && q < P.Tq && (lane >> 4) == 0 && P.lse) P.lse[((int64_t)g * P.heads + h) * P.Tq + q] = lv[f];
#pragma unroll
    for (int kf = 0; kf < NKF; ++kf) {
      if (16 * kf >= nvalid) continue;
      float dm[4] = {1.f, 1.f, 1.f, 1.f};
      if (P.p > 0.f)
        dropout_mult4(P.seed, ((uint64_t)g * P.heads + h) * P.Tq * P.Tk + (__umul24((unsigned)q, (unsigned)P.Tk) + (unsigned)(16 * kf + 4 * (lane >> 4))),
                      P.p, inv_keep, dm);
#pragma unroll
      for (int r = 0; r < 4; ++r) sc[kf][f][r] = sc[kf][f][r] * inv * dm[r];
    }
  }
  // O^T[d][q] = sum_key V[key][d] P[q][key]
#pragma unroll
  for (int df = 0; df < 4; ++df)
#pragma unroll
    for (int f = 0; f < 2; ++f) oc[df][f] = f32x4{0.f, 0.f, 0.f, 0.f};
  fwd_pv_step<NKF>(Vs, sc, nvalid, lane, oc);
}
template <bool LSE_LATE>
__device__ __forceinline__ void attn_mfma_fwd_tile_store(const AttnMfmaParams& P, int g, int h, int q0, int lane, const f32x4 (&oc)[4][2],
                                                         const float (&lv)[2]) {
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    const int q = q0 + 16 * f + (lane & 15);
    if (q < P.Tq) {
      if (LSE_LATE && (lane >> 4) == 0 && P.lse) P.lse[((int64_t)g * P.heads + h) * P.Tq + q] = lv[f];
      bf16_t* orow = P.out + ((int64_t)g * P.Tq + q) * P.ldo + h * AD + 4 * (lane >> 4);
#pragma unroll
      for (int df = 0; df < 4; ++df) store4(orow + 16 * df, oc[df][f]);
    }
  }
}
template <int NKT>
__device__ __forceinline__ void attn_mfma_fwd_tile(const AttnMfmaParams& P, int g, int h, int q0, int lane, const bf16x8 (&qf)[2][2],
                                                   const char* Ks, const char* Vs, const float* mask_lds = nullptr) {
  f32x4 oc[4][2];
  float lv[2];
  attn_mfma_fwd_tile_compute<NKT, false>(P, g, h, q0, lane, qf, Ks, Vs, mask_lds, oc, lv);
  attn_mfma_fwd_tile_store<false>(P, g, h, q0, lane, oc, lv);
}

template <int NKT>
__device__ __forceinline__ void attn_mfma_fwd_body(const AttnMfmaParams& P) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Ks = smem;
  char* Vs = smem + NKT * TILE_B;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int g = blockIdx.x / P.heads, h = blockIdx.x % P.heads;
  const int q0 = blockIdx.y * AT + w * 32;
  const bf16_t* kbase_p = P.k + (int64_t)g * P.Tk * P.ldk + h * AD;
  const bf16_t* vbase_p = P.v + (int64_t)g * P.Tk * P.ldk + h * AD;
  const TileRegs kt = load_tile(kbase_p, P.ldk, P.Tk, tid);
  const TileRegs vt = load_tile(vbase_p, P.ldk, P.Tk, tid);
  bf16x8 qf[2][2];
  load_q_frags(P.q, P.ldq, P.Tq, g, h, q0, lane, qf);
  store_tile<false>(Ks, kt, tid);      // (all of K, V and Q were requested before the first LDS write)
  store_tile<true>(Vs, vt, tid);
  if constexpr (NKT == 2) {
    const TileRegs kt2 = load_tile(kbase_p + (int64_t)AT * P.ldk, P.ldk, P.Tk - AT, tid);
    const TileRegs vt2 = load_tile(vbase_p + (int64_t)AT * P.ldk, P.ldk, P.Tk - AT, tid);
    store_tile<false>(Ks + TILE_B, kt2, tid);
    store_tile<true>(Vs + TILE_B, vt2, tid);
  }
  __syncthreads();
  attn_mfma_fwd_tile<NKT>(P, g, h, q0, lane, qf, Ks, Vs);
}

// Persistent form for Tk <= 128 (the FCMF-base text encoder: 4608 (sequence, head) tiles per layer): a workgroup walks
// tiles blockIdx.x, + gridDim.x, ...; the K / V / Q loads of the NEXT tile are put in flight (into registers) before the
// current tile is computed and land in the other half of a double-buffered LDS image afterwards, so the global-load
// latency -- 58 % of a wave's lifetime in the one-tile-per-workgroup kernel (SQ_WAIT_ANY) -- hides under the softmax.
// Per tile: prefetch, arithmetic, wait for the prefetch (nothing but loads outstanding), LDS writes, THEN the tile's global
// stores, barrier: no wait for loads ever stands behind younger stores.  64 KiB of LDS, two workgroups per CU.
__global__ __launch_bounds__(256, 2) void attn_mfma_fwd_persist_kernel(AttnMfmaParams P, int ntiles, int qtiles) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  auto where = [&](int tile, int& g, int& h, int& q0) {
    const int gh = tile / qtiles;
    g = gh / P.heads; h = gh - g * P.heads; q0 = (tile - gh * qtiles) * AT + w * 32;
  };
  constexpr int BUF = 2 * TILE_B + 512;      // K image, V image, 128 mask floats
  int tile = blockIdx.x;
  if (tile >= ntiles) return;
  int g, h, q0;
  where(tile, g, h, q0);
  bf16x8 qf[2][2];
  // (every load of a tile's operands is unconditional -- indices past the end are clamped, the values cleared or never read --
  // so that the compiler keeps them one batch and counts its waits; mask entries of keys >= Tk are never read)
  auto mask_of = [&](int gg) { return P.mask ? P.mask[(int64_t)gg * P.Tk + min(tid, P.Tk - 1)] : 0.f; };
  {
    TileRegs kt = load_tile_clamped(P.k + (int64_t)g * P.Tk * P.ldk + h * AD, P.ldk, P.Tk, tid);
    TileRegs vt = load_tile_clamped(P.v + (int64_t)g * P.Tk * P.ldk + h * AD, P.ldk, P.Tk, tid);
    const float mv = mask_of(g);
    load_q_frags_clamped(P, g, h, q0, lane, qf);
    zero_tail(kt, P.Tk, tid);
    zero_tail(vt, P.Tk, tid);
    zero_q_tail(P, q0, lane, qf);
    store_tile<false>(smem, kt, tid);
    store_tile<true>(smem + TILE_B, vt, tid);
    if (tid < AT) reinterpret_cast<float*>(smem + 2 * TILE_B)[tid] = mv;
  }
  __syncthreads();
  int cur = 0;
  // The loop body is a tile that HAS a successor; the last tile of the walk is computed behind the loop.  (With both in one
  // body the path that skips the prefetch joins the back edge, and the compiler then waits at the loop top, where it
  // redefines the prefetch registers, for most of the previous tile's stores.)
  for (int nxt = tile + gridDim.x; nxt < ntiles; nxt += gridDim.x) {
    int g2, h2, q2;
    bf16x8 qn[2][2];
    where(nxt, g2, h2, q2);                  // next tile's operands: in flight under this tile's arithmetic
    TileRegs kt = load_tile_clamped(P.k + (int64_t)g2 * P.Tk * P.ldk + h2 * AD, P.ldk, P.Tk, tid);
    TileRegs vt = load_tile_clamped(P.v + (int64_t)g2 * P.Tk * P.ldk + h2 * AD, P.ldk, P.Tk, tid);
    const float mv = mask_of(g2);
    load_q_frags_clamped(P, g2, h2, q2, lane, qn);
    const char* buf = smem + cur * BUF;
    f32x4 oc[4][2];
    float lv[2];
    attn_mfma_fwd_tile_compute<1, true>(P, g, h, q0, lane, qf, buf, buf + TILE_B, reinterpret_cast<const float*>(buf + 2 * TILE_B), oc, lv);
    // The next tile's operands go to LDS BEFORE this tile's results are stored: loads and stores retire through one in-order
    // counter, so a wait for the operands placed behind the stores would also wait for the stores' acknowledgement.
    cur ^= 1;                                // (the other buffer was last read before the previous barrier)
    zero_tail(kt, P.Tk, tid);
    zero_tail(vt, P.Tk, tid);
    store_tile<false>(smem + cur * BUF, kt, tid);
    store_tile<true>(smem + cur * BUF + TILE_B, vt, tid);
    if (tid < AT) reinterpret_cast<float*>(smem + cur * BUF + 2 * TILE_B)[tid] = mv;
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) qf[f][s2] = qn[f][s2];
    zero_q_tail(P, q2, lane, qf);
    // (pinned: the compiler otherwise sinks this last use of the loaded fragments below the stores, and its wait with it)
    asm volatile("" : "+v"(qf[0][0]), "+v"(qf[0][1]), "+v"(qf[1][0]), "+v"(qf[1][1]) : : "memory");
    attn_mfma_fwd_tile_store<true>(P, g, h, q0, lane, oc, lv);
    g = g2; h = h2; q0 = q2;
    __syncthreads();
  }
  const char* buf = smem + cur * BUF;
  attn_mfma_fwd_tile<1>(P, g, h, q0, lane, qf, buf, buf + TILE_B, reinterpret_cast<const float*>(buf + 2 * TILE_B));
}

__global__ __launch_bounds__(256, 3) void attn_mfma_fwd_kernel(AttnMfmaParams P) { attn_mfma_fwd_body<1>(P); }
__global__ __launch_bounds__(256, 2) void attn_mfma_fwd256_kernel(AttnMfmaParams P) { attn_mfma_fwd_body<2>(P); }

// =========================================================================================
// backward.  NQT = 128-query tiles, NKT = 128-key tiles handled by ONE workgroup per (sequence, head):
//   <1,1>  Tq, Tk <= 128 : 80 KiB of LDS, two workgroups per CU (the FCMF-base text encoder);
//   <2,2>  Tq, Tk <= 256 : 144 KiB, one workgroup per CU = one wave per SIMD with the whole register file (the
//          FCMF-large text encoder, S = 256): the fragments of BOTH query tiles stay in registers, the key chunks go by
//          once, and for every chunk the two query tiles take turns in the two chunk images, so that dK / dV of the chunk
//          accumulate over all 256 queries in registers and are stored once -- no partial buffers, no atomics.
template <int NQT, int NKT>
__device__ __forceinline__ void attn_mfma_bwd_body(const AttnMfmaParams& P) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Qs = smem;                               // NQT tiles
  char* dOs = Qs + NQT * TILE_B;                 // NQT tiles
  char* Ks = dOs + NQT * TILE_B;                 // NKT tiles
  char* Vs = Ks + NKT * TILE_B;                  // NKT tiles
  char* PdT = Vs + NKT * TILE_B;                 // [32 keys][128 q] bf16 of the current (key chunk, query tile), 8 KiB
  char* dST = PdT + TILE_B / 2;                  // 8 KiB
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int g = blockIdx.x / P.heads, h = blockIdx.x % P.heads;
  const int64_t qbase = (int64_t)g * P.Tq, kbase = (int64_t)g * P.Tk;
  // delta[q] = sum_d dO[q][d] O[q][d] for the wave's 32 query rows of every query tile: two lanes per row, then every
  // lane picks the values of the rows its accumulator registers hold
  // ALL global reads of the workgroup -- the Q / dO / K / V tiles, the O rows of delta, lse and the mask row -- are requested
  // here in one batch, none of them under a branch (indices past the end are clamped, the values cleared afterwards), and
  // waited for once: one round trip to memory, and none in the chunk loop below.
  float dl4[NQT][2][4], lse4[NQT][2][4];
  float mreg[2 * NKT];       // additive mask of key 64 i + lane (0 without a mask and past Tk)
  {
    TileRegs tq[NQT], td[NQT], tk[NKT], tv[NKT];
    uint4 og[NQT][4];        // O[q][32 half + 8 i ..], q = the wave's row lane >> 1, half = lane & 1
#pragma unroll
    for (int qt = 0; qt < NQT; ++qt) {
      tq[qt] = load_tile_clamped(P.q + (qbase + qt * AT) * P.ldq + h * AD, P.ldq, P.Tq - qt * AT, tid);
      td[qt] = load_tile_clamped(P.dout + (qbase + qt * AT) * P.ldo + h * AD, P.ldo, P.Tq - qt * AT, tid);
    }
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
      tk[kt] = load_tile_clamped(P.k + (kbase + kt * AT) * P.ldk + h * AD, P.ldk, P.Tk - kt * AT, tid);
      tv[kt] = load_tile_clamped(P.v + (kbase + kt * AT) * P.ldk + h * AD, P.ldk, P.Tk - kt * AT, tid);
    }
#pragma unroll
    for (int qt = 0; qt < NQT; ++qt) {
      const int q = min(qt * AT + 32 * w + (lane >> 1), P.Tq - 1);
      const bf16_t* b = P.o + (qbase + q) * P.ldo + h * AD + 32 * (lane & 1);
#pragma unroll
      for (int i = 0; i < 4; ++i) og[qt][i] = *reinterpret_cast<const uint4*>(b + 8 * i);
#pragma unroll
      for (int f = 0; f < 2; ++f)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int q2 = qt * AT + 32 * w + 16 * f + 4 * (lane >> 4) + r;
          lse4[qt][f][r] = P.lse[((int64_t)g * P.heads + h) * P.Tq + min(q2, P.Tq - 1)];
        }
    }
#pragma unroll
    for (int i = 0; i < 2 * NKT; ++i) mreg[i] = P.mask ? P.mask[kbase + min(64 * i + lane, P.Tk - 1)] : 0.f;
#pragma unroll
    for (int qt = 0; qt < NQT; ++qt) {
      zero_tail(tq[qt], P.Tq - qt * AT, tid);
      zero_tail(td[qt], P.Tq - qt * AT, tid);
      store_tile<false>(Qs + qt * TILE_B, tq[qt], tid);
      store_tile<false>(dOs + qt * TILE_B, td[qt], tid);
    }
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
      zero_tail(tk[kt], P.Tk - kt * AT, tid);
      zero_tail(tv[kt], P.Tk - kt * AT, tid);
      store_tile<false>(Ks + kt * TILE_B, tk[kt], tid);
      store_tile<false>(Vs + kt * TILE_B, tv[kt], tid);
    }
    __syncthreads();
    // delta[q] = sum_d dO[q][d] O[q][d]: dO from its LDS image (not a second time from memory), O from the registers
#pragma unroll
    for (int qt = 0; qt < NQT; ++qt) {
      const int ql = 32 * w + (lane >> 1), half = lane & 1;
      float sd = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bf16x8 x = *reinterpret_cast<const bf16x8*>(dOs + qt * TILE_B + off64(ql, 4 * half + i));
        const bf16x8 y = *reinterpret_cast<const bf16x8*>(&og[qt][i]);
#pragma unroll
        for (int j = 0; j < 8; ++j) sd += (float)x[j] * (float)y[j];
      }
      if (qt * AT + ql >= P.Tq) sd = 0.f;
      sd += __shfl_xor(sd, 1, 64);
#pragma unroll
      for (int f = 0; f < 2; ++f)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int qr = 16 * f + 4 * (lane >> 4) + r;          // row inside the wave's 32
          dl4[qt][f][r] = __shfl(sd, 2 * qr, 64);
          if (qt * AT + 32 * w + qr >= P.Tq) lse4[qt][f][r] = 0.f;
        }
    }
  }

  bool masked = P.mask != nullptr;
  float score_scale = P.scale;            // (0 for a sequence whose every key is hard-masked: see below)
  // operands that stay in registers, per query tile
  bf16x8 qa[NQT][2][2], da[NQT][2][2], oT[NQT][4], qT[NQT][4];
  f32x4 aQ[NQT][4][2] = {};
#pragma unroll
  for (int qt = 0; qt < NQT; ++qt)
    bwd_resident_frags(Qs + qt * TILE_B, dOs + qt * TILE_B, w, lane, qa[qt], da[qt], oT[qt], qT[qt]);

  // ---- key chunks of 32; per chunk the query tiles take turns: phase 1 (wave = 32 query rows) builds Pdrop^T and dS^T
  // [key][q] of (chunk, query tile) in LDS, phase 2 adds them to dQ of that tile (wave = 32 queries) and to dV / dK of
  // the chunk's 32 keys (wave = 16 columns), which are stored after the last query tile
  const int nchunks_all = (P.Tk + 31) >> 5;
  // trailing keys whose additive mask is the "hard" value (<= -1e30: HF's finfo.min padding mask) have probabilities that
  // are EXACTLY zero (exp underflows), so whole 32-key chunks of them contribute nothing to dQ and get dK = dV = 0: they
  // are skipped, with bit-identical results.  nvalid = index of the last key that is not hard-masked, + 1 (wave-uniform).
  int nvalid = P.Tk;
  if (masked) {
    const int last = last_live_key<2 * NKT>([&](int i, int) { return mreg[i]; }, P.Tk, lane);
#pragma unroll
    for (int i = 0; i < 2 * NKT; ++i)
      if (64 * i + lane >= P.Tk) mreg[i] = 0.f;
    nvalid = last >= 0 ? last + 1 : P.Tk;    // no live key at all: nothing may be skipped (softmax over finfo.min scores is uniform over ALL keys)
    if (uniform_if_no_live_key(last >= 0, P.Tk, score_scale, lse4)) masked = false;
  }
  const int nchunks = (nvalid + 31) >> 5;
  const BwdDropout D = bwd_dropout_state(P, g, h, lane, 0xFFFFu);      // (pair offsets stay below 2^15: Tq, Tk <= 256)
  f32x4 cV = f32x4{0.f, 0.f, 0.f, 0.f}, cK = f32x4{0.f, 0.f, 0.f, 0.f};   // column sums of dV / dK over the keys (this lane's keys)
  // dk / dv leave in whole 128-byte rows too: wave w owns 16 of a row's 64 columns, so the chunk's [32 keys][64 d] blocks
  // are put together in LDS -- in the K / V rows of the chunk itself, dead once the chunk is done (16-byte piece XOR
  // ((key >> 1) & 7), as for dq below) -- and go out 16 bytes per lane behind the NEXT barrier the loop has anyway.
  auto flush_dkv = [&](int cc) {
    const int r = tid >> 3, ch = tid & 7, key = 32 * cc + r;
    const int o = cc * (TILE_B / 4) + r * 128 + ((ch ^ ((r >> 1) & 7)) << 4);
    const uint4 dvv = *reinterpret_cast<const uint4*>(Vs + o), dkk = *reinterpret_cast<const uint4*>(Ks + o);
    if (key < P.Tk) {
      *reinterpret_cast<uint4*>(P.dv + (kbase + key) * P.ldk + h * AD + 8 * ch) = dvv;
      *reinterpret_cast<uint4*>(P.dk + (kbase + key) * P.ldk + h * AD + 8 * ch) = dkk;
    }
  };
  for (int c = 0; c < nchunks; ++c) {
    f32x4 aV[2], aK[2];
#pragma unroll
    for (int kf = 0; kf < 2; ++kf) { aV[kf] = f32x4{0.f, 0.f, 0.f, 0.f}; aK[kf] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    // mask of the chunk's keys 32 c + 16 k4 + (lane & 15) from the lanes that loaded them: no global load in this loop, so no
    // wait that the dk / dv stores of the previous chunk (same in-order counter) could hold up
    float mk2[2] = {0.f, 0.f};
    if (masked) {
      float mc = mreg[0];
#pragma unroll
      for (int i = 1; i < 2 * NKT; ++i) mc = (c >> 1) == i ? mreg[i] : mc;
#pragma unroll
      for (int k4 = 0; k4 < 2; ++k4) mk2[k4] = __shfl(mc, 32 * (c & 1) + 16 * k4 + (lane & 15), 64);
    }
#pragma unroll
    for (int qt = 0; qt < NQT; ++qt) {
      bwd_chunk_phase1(P, D, Ks, Vs, PdT, dST, c, 32 * c, qt * AT, mk2, score_scale, qa[qt], da[qt], lse4[qt], dl4[qt], w, lane);
      __syncthreads();
      if (qt == 0 && c > 0) flush_dkv(c - 1);      // (staged by all four waves before the barrier just passed)
      bwd_chunk_phase2(Ks, PdT, dST, c, oT[qt], qT[qt], aQ[qt], aV, aK, w, lane);
      __syncthreads();   // the chunk images are rewritten by the next query tile / chunk
    }
    cV += aV[0] + aV[1];        // (keys past Tk carry zero probabilities: no mask needed)
    cK += aK[0] + aK[1];
    // staged over the chunk's own K / V rows, which nobody reads again (every wave has passed the closing barrier above)
#pragma unroll
    for (int kf = 0; kf < 2; ++kf) {
      const int kl = 16 * kf + (lane & 15);
      const int o = c * (TILE_B / 4) + kl * 128 + (((2 * w + (lane >> 5)) ^ ((kl >> 1) & 7)) << 4) + ((lane >> 4) & 1) * 8;
      store4(reinterpret_cast<bf16_t*>(Vs + o), aV[kf]);
      f32x4 t = aK[kf];
      t[0] *= P.scale; t[1] *= P.scale; t[2] *= P.scale; t[3] *= P.scale;
      store4(reinterpret_cast<bf16_t*>(Ks + o), t);
    }
  }
  __syncthreads();
  flush_dkv(nchunks - 1);
  for (int c = nchunks; c < nchunks_all; ++c) {      // the skipped (fully hard-masked) chunks: dK = dV = 0
    const int key = 32 * c + (tid >> 3);
    if (key < P.Tk) {
      *reinterpret_cast<uint4*>(P.dv + (kbase + key) * P.ldk + h * AD + 8 * (tid & 7)) = make_uint4(0, 0, 0, 0);
      *reinterpret_cast<uint4*>(P.dk + (kbase + key) * P.ldk + h * AD + 8 * (tid & 7)) = make_uint4(0, 0, 0, 0);
    }
  }
  // dq leaves in whole 128-byte rows: the wave turns its 64 x 32 block of dQ^T into [q][d] through its own quarter of the
  // two chunk images (free now: every wave has passed the last chunk's closing barrier; wave-private, so no barrier here)
  // and stores 16 bytes per lane, 8 rows per instruction.  16-byte piece XOR ((q >> 1) & 7): conflict free both ways.
  char* stg = PdT + w * (TILE_B / 4);
#pragma unroll
  for (int qt = 0; qt < NQT; ++qt) {
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      const int ql = 16 * f + (lane & 15);
#pragma unroll
      for (int df = 0; df < 4; ++df) {
        f32x4 t = aQ[qt][df][f];
        t[0] *= P.scale; t[1] *= P.scale; t[2] *= P.scale; t[3] *= P.scale;
        store4(reinterpret_cast<bf16_t*>(stg + ql * 128 + (((2 * df + (lane >> 5)) ^ ((ql >> 1) & 7)) << 4) + ((lane >> 4) & 1) * 8), t);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int ql = 8 * i + (lane >> 3), ch = lane & 7, x = qt * AT + 32 * w + ql;
      const uint4 v = *reinterpret_cast<const uint4*>(stg + ql * 128 + ((ch ^ ((ql >> 1) & 7)) << 4));
      if (x < P.Tq) *reinterpret_cast<uint4*>(P.dq + (qbase + x) * P.ldq + h * AD + 8 * ch) = v;
    }
  }
  // ---- optional: column sums of this (sequence, head)'s dq | dk | dv (f32 accumulators, before the bf16 rounding): the
  // bias gradient of the fused q|k|v projection is their sum over the sequences -- saves a pass over dqkv
  if (P.colsum) {
    const int HD = P.heads * AD;
    float* row = P.colsum + (int64_t)g * 3 * HD + h * AD;
#pragma unroll
    for (int r = 0; r < 4; ++r) { cV[r] = row16_sum(cV[r]); cK[r] = row16_sum(cK[r]); }
    if ((lane & 15) == 0) {      // d = 16 w + 4 (lane >> 4) + r: the workgroup owns these 64 columns of row g
      const int d0 = 16 * w + 4 * (lane >> 4);
#pragma unroll
      for (int r = 0; r < 4; ++r) { row[2 * HD + d0 + r] = cV[r]; row[HD + d0 + r] = cK[r] * P.scale; }
    }
    // dq: rows q = .. + (lane & 15) over the fragments, query tiles and the four waves (through LDS: 64 floats at the start of
    // each wave's own dq staging quarter, which only that wave has read)
    constexpr int RW = TILE_B / 4 / 4;             // floats between the waves' rows
    float* red = reinterpret_cast<float*>(PdT);    // [4 waves][RW], 64 d used
#pragma unroll
    for (int df = 0; df < 4; ++df) {
      f32x4 t = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int qt = 0; qt < NQT; ++qt)
#pragma unroll
        for (int f = 0; f < 2; ++f) t += aQ[qt][df][f];
#pragma unroll
      for (int r = 0; r < 4; ++r) t[r] = row16_sum(t[r]);
      if ((lane & 15) == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) red[w * RW + 16 * df + 4 * (lane >> 4) + r] = t[r];
      }
    }
    __syncthreads();
    if (tid < 64) row[tid] = (red[tid] + red[RW + tid] + red[2 * RW + tid] + red[3 * RW + tid]) * P.scale;
  }
}

__global__ __launch_bounds__(256, 2) void attn_mfma_bwd_kernel(AttnMfmaParams P) { attn_mfma_bwd_body<1, 1>(P); }
__global__ __launch_bounds__(256, 1) void attn_mfma_bwd256_kernel(AttnMfmaParams P) { attn_mfma_bwd_body<2, 2>(P); }

// =========================================================================================
extern "C" int fcmf_attn_mfma_fwd(const void* q, const void* k, const void* v, const float* mask, void* out, float* lse,
                                  int G, int heads, int Tq, int Tk, int64_t ldq, int64_t ldk, int64_t ldo, float scale,
                                  float dropout_p, uint64_t seed, void* stream) {
  if (!q || !k || !v || !out || G <= 0 || heads <= 0 || Tq <= 0 || Tk <= 0) return FCMF_ERR_ARG;
  if (Tk > 2 * AT || ldq % 8 || ldk % 8 || ldo % 4 || !al16(q) || !al16(k) || !al16(v) || !al16(out)) return FCMF_ERR_UNSUPPORTED;
  const AttnMfmaParams P = attn_mfma_params(q, k, v, mask, out, lse, G, heads, Tq, Tk, ldq, ldk, ldo, scale, dropout_p, seed);
  const dim3 grid(G * heads, (Tq + AT - 1) / AT);
  if (Tk > AT) {
    const int smem = 4 * TILE_B;
    static bool attr2 = false;      // (this kernel's dynamic LDS is one constant: its limit is raised once)
    return fcmf_launch_flagged(&attr2, attn_mfma_fwd256_kernel, grid, dim3(256), smem, reinterpret_cast<hipStream_t>(stream), P);
  }
  const int ntiles = (int)(grid.x * grid.y);
  static const bool no_persist = getenv("FCMF_ATTN_NO_PERSIST") != nullptr;      // A/B switch for benchmarks
  if (ntiles >= 4 * 512 && !no_persist) {       // enough tiles for every resident workgroup (2 per CU) to walk several
    const int smem = 2 * (2 * TILE_B + 512);
    static bool attr3 = false;      // (this kernel's dynamic LDS is one constant: its limit is raised once)
    return fcmf_launch_flagged(&attr3, attn_mfma_fwd_persist_kernel, dim3(512), dim3(256), smem, reinterpret_cast<hipStream_t>(stream), P, ntiles, (int)grid.y);
  }
  const int smem = 2 * TILE_B;
  static bool attr = false;      // (this kernel's dynamic LDS is one constant: its limit is raised once)
  return fcmf_launch_flagged(&attr, attn_mfma_fwd_kernel, grid, dim3(256), smem, reinterpret_cast<hipStream_t>(stream), P);
}

extern "C" int fcmf_attn_mfma_bwd(const void* q, const void* k, const void* v, const float* mask, const void* out,
                                  const void* dout, const float* lse, void* dq, void* dk, void* dv, int G, int heads,
                                  int Tq, int Tk, int64_t ldq, int64_t ldk, int64_t ldo, float scale, float dropout_p,
                                  uint64_t seed, float* colsum, void* stream) {
  if (!q || !k || !v || !out || !dout || !lse || !dq || !dk || !dv || G <= 0 || heads <= 0 || Tq <= 0 || Tk <= 0) return FCMF_ERR_ARG;
  if (Tk > 2 * AT || Tq > 2 * AT || ldq % 8 || ldk % 8 || ldo % 8 || !al16(q) || !al16(k) || !al16(v) || !al16(out) || !al16(dout) ||
      !al16(dq) || !al16(dk) || !al16(dv))
    return FCMF_ERR_UNSUPPORTED;
  const AttnMfmaParams P = attn_mfma_params(q, k, v, mask, nullptr, const_cast<float*>(lse), G, heads, Tq, Tk, ldq, ldk, ldo, scale,
                                            dropout_p, seed, out, dout, dq, dk, dv, colsum);
  if (Tk > AT || Tq > AT) {
    const int smem = 9 * TILE_B;   // 2 x (Q, dO) + 2 x (K, V) tiles + the two 8 KiB chunk images = 144 KiB: one workgroup per CU
    static bool attr2 = false;      // (this kernel's dynamic LDS is one constant: its limit is raised once)
    return fcmf_launch_flagged(&attr2, attn_mfma_bwd256_kernel, dim3(G * heads), dim3(256), smem, reinterpret_cast<hipStream_t>(stream), P);
  }
  const int smem = 5 * TILE_B;   // Q, K, V, dO tiles + the two 8 KiB chunk images = 80 KiB: two workgroups per CU
  static bool attr = false;      // (this kernel's dynamic LDS is one constant: its limit is raised once)
  return fcmf_launch_flagged(&attr, attn_mfma_bwd_kernel, dim3(G * heads), dim3(256), smem, reinterpret_cast<hipStream_t>(stream), P);
}
