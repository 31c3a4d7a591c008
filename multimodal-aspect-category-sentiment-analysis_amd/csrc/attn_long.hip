// MFMA attention with any number of keys and a key/value set shared by consecutive query groups: bf16, head dim 64,
// up to 256 queries per group.  The cross-attention of the comparison baselines: the text queries of the `kv_share`
// aspect prompts of a review attend to all of the review's visual tokens (371 or 595 keys), which are projected and stored
// once per review -- group g reads key set g / kv_share.
//   forward : one workgroup per (group, head, 128-query tile).  The keys go by in 128-key tiles: the next tile's K / V rows
//             are in flight (in registers) while the current tile is computed from its LDS images, exactly as one tile of
//             attn_mfma.hip is (S^T accumulators with the key index in the registers, P never leaves them), under a
//             running row maximum and sum that rescale the O accumulators.  Dropout multiplies the unnormalised
//             probabilities, the row sum is taken before it, and O is divided by the sum at the end.  32 KiB of LDS.
//   backward: one workgroup per (key set, head) walks the `kv_share` groups that read the set.  Per group, Q, dO, the
//             logsumexp and the row dot-products stay resident (Tq <= 256) and the 32-key chunk loop of attn_mfma.hip runs
//             inside the loop over 128-key tiles: dQ accumulates across tiles in registers, dK / dV of a chunk are
//             finished when the chunk leaves.  Every dK / dV element belongs to ONE lane for all groups, so their sum over
//             the groups is a private float32 read-modify-write in a workspace, rounded to bf16 once by the last group:
//             no atomics, no partial buffers, deterministic.  80 KiB (Tq <= 128) or 112 KiB of LDS.
// Tiles (forward) and chunks (backward) whose keys all carry the hard mask (<= -1e30, HF's finfo.min) are skipped with
// bit-identical results unless the group has no live key at all (then softmax is uniform over ALL keys).
#include "attn_tiles.h"

struct AttnLongParams {
  AttnMfmaParams a;      // (G = number of query groups; k / v / dk / dv hold G / kv_share key sets)
  int kv_share;
  float* ws;             // backward, kv_share > 1: [2][G / kv_share][Tk][heads * 64] f32 running sums of dK | dV
};

// does the group have any key that is not hard-masked?  (wave-uniform)
__device__ __forceinline__ bool any_live_key(const float* mrow, int Tk, int lane) {
  for (int k0 = 0; k0 < Tk; k0 += 64) {
    const int key = k0 + lane;
    if (__ballot(key < Tk && mrow[key] > -1e30f)) return true;
  }
  return false;
}
// ... and among keys k0 .. k0 + n - 1 (n <= 128)?
__device__ __forceinline__ bool any_live_in(const float* mrow, int Tk, int k0, int n, int lane) {
  const int a = k0 + lane, b = k0 + 64 + lane;
  const bool la = lane < n && a < Tk && mrow[a] > -1e30f;
  const bool lb = 64 + lane < n && b < Tk && mrow[b] > -1e30f;
  return __ballot(la || lb) != 0;
}

// =========================================================================================
__global__ __launch_bounds__(256, 2) void attn_long_fwd_kernel(AttnLongParams L) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const AttnMfmaParams& P = L.a;
  char* Ks = smem;
  char* Vs = smem + TILE_B;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int g = blockIdx.x / P.heads, h = blockIdx.x % P.heads;
  const int q0 = blockIdx.y * AT + w * 32;
  const int64_t kbase = (int64_t)(g / L.kv_share) * P.Tk;
  const bf16_t* kp = P.k + kbase * P.ldk + h * AD;
  const bf16_t* vp = P.v + kbase * P.ldk + h * AD;
  const float* mrow = P.mask ? P.mask + (int64_t)g * P.Tk : nullptr;
  const int ntiles = (P.Tk + AT - 1) / AT;
  const bool skip_dead = mrow && any_live_key(mrow, P.Tk, lane);
  auto next_live = [&](int t) {      // first tile >= t with a live key (the same in every wave: barriers stay matched)
    while (skip_dead && t < ntiles && !any_live_in(mrow, P.Tk, t * AT, AT, lane)) ++t;
    return t;
  };
  int t = next_live(0);
  bf16x8 qf[2][2];
  {
    const TileRegs kt = load_tile(kp + (int64_t)t * AT * P.ldk, P.ldk, P.Tk - t * AT, tid);
    const TileRegs vt = load_tile(vp + (int64_t)t * AT * P.ldk, P.ldk, P.Tk - t * AT, tid);
    load_q_frags(P.q, P.ldq, P.Tq, g, h, q0, lane, qf);
    store_tile<false>(Ks, kt, tid);
    store_tile<true>(Vs, vt, tid);
  }
  __syncthreads();
  const float inv_keep = P.p > 0.f ? 1.0f / (1.0f - P.p) : 1.0f;
  const uint64_t drop_base = ((uint64_t)g * P.heads + h) * P.Tq * P.Tk;
  float m_run[2] = {-INFINITY, -INFINITY}, l_run[2] = {0.f, 0.f};
  f32x4 oc[4][2];
#pragma unroll
  for (int df = 0; df < 4; ++df)
#pragma unroll
    for (int f = 0; f < 2; ++f) oc[df][f] = f32x4{0.f, 0.f, 0.f, 0.f};

  while (t < ntiles) {
    const int tn = next_live(t + 1);
    TileRegs kt, vt;
    if (tn < ntiles) {                        // next tile's rows: in flight under this tile's arithmetic
      kt = load_tile(kp + (int64_t)tn * AT * P.ldk, P.ldk, P.Tk - tn * AT, tid);
      vt = load_tile(vp + (int64_t)tn * AT * P.ldk, P.ldk, P.Tk - tn * AT, tid);
    }
    const int k0 = t * AT;
    const int rows = min(AT, P.Tk - k0);      // keys of this tile; 16-key fragments past them are skipped
    // S^T[key][q]: 8 key fragments x 2 query fragments
    f32x4 sc[8][2];
    fwd_score_frags<8>([&](int x0, int s) { return frag_row64(Ks, x0, s, lane); }, qf, rows, sc);
    // lane holds, for query q0+16f+(lane&15), keys k0 + 16kf + 4(lane>>4) + r
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      const int q = q0 + 16 * f + (lane & 15);
      float m = -INFINITY;
#pragma unroll
      for (int kf = 0; kf < 8; ++kf) {
        if (16 * kf >= rows) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = k0 + 16 * kf + 4 * (lane >> 4) + r;
          float s = -INFINITY;
          if (key < P.Tk) s = sc[kf][f][r] * P.scale + (mrow ? mrow[key] : 0.f);
          sc[kf][f][r] = s;
          m = fmaxf(m, s);
        }
      }
      m = fmaxf(m, __shfl_xor(m, 16, 64));
      m = fmaxf(m, __shfl_xor(m, 32, 64));
      const float m_new = fmaxf(m_run[f], m);            // (finite: every tile has a key below Tk)
      const float alpha = __expf(m_run[f] - m_new);      // 0 at the first tile, and after tiles that held only hard-masked keys
      float sum = 0.f;
#pragma unroll
      for (int kf = 0; kf < 8; ++kf) {
        if (16 * kf >= rows) continue;         // (sc of a skipped fragment stays 0 = its probabilities)
        float dm[4] = {1.f, 1.f, 1.f, 1.f};
        if (P.p > 0.f)
          dropout_mult4(P.seed, drop_base + (__umul24((unsigned)q, (unsigned)P.Tk) + (unsigned)(k0 + 16 * kf + 4 * (lane >> 4))),
                        P.p, inv_keep, dm);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float e = __expf(sc[kf][f][r] - m_new);
          sum += e;
          sc[kf][f][r] = e * dm[r];
        }
      }
      sum += __shfl_xor(sum, 16, 64);
      sum += __shfl_xor(sum, 32, 64);
      l_run[f] = l_run[f] * alpha + sum;
      m_run[f] = m_new;
#pragma unroll
      for (int df = 0; df < 4; ++df) oc[df][f] *= alpha;
    }
    fwd_pv_step<8>(Vs, sc, rows, lane, oc);      // O^T[d][q] += sum_key V[key][d] P[q][key]
    __syncthreads();                          // every wave is done with the images
    if (tn < ntiles) {
      store_tile<false>(Ks, kt, tid);
      store_tile<true>(Vs, vt, tid);
    }
    __syncthreads();
    t = tn;
  }
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    const int q = q0 + 16 * f + (lane & 15);
    if (q < P.Tq) {
      const float inv = 1.0f / l_run[f];
      if ((lane >> 4) == 0 && P.lse) P.lse[((int64_t)g * P.heads + h) * P.Tq + q] = m_run[f] + __logf(l_run[f]);
      bf16_t* orow = P.out + ((int64_t)g * P.Tq + q) * P.ldo + h * AD + 4 * (lane >> 4);
#pragma unroll
      for (int df = 0; df < 4; ++df) store4(orow + 16 * df, oc[df][f] * inv);
    }
  }
}

// =========================================================================================
// dK / dV of 32-key chunk `cg` (global chunk index) after group `sm` of the key set: add the running float32 sums of the
// earlier groups, then either keep the sum (more groups follow) or round it to bf16 (last group).  `contrib` = false: the
// chunk was skipped for this group (all its keys hard-masked), aV / aK are not read.
__device__ __forceinline__ void finish_chunk(const AttnLongParams& L, int64_t kbase, int h, int w, int lane, int cg, int sm,
                                             bool contrib, const f32x4 (&aV)[2], const f32x4 (&aK)[2]) {
  const AttnMfmaParams& P = L.a;
  const bool first = sm == 0, last = sm == L.kv_share - 1;
  if (!contrib && !first && !last) return;       // the running sums stand as they are
  const int dcol = h * AD + 16 * w + 4 * (lane >> 4);
  const int64_t HD = (int64_t)P.heads * AD;
  const int64_t dv_off = (int64_t)(P.G / L.kv_share) * P.Tk * HD;      // the dV half of the workspace
#pragma unroll
  for (int kf = 0; kf < 2; ++kf) {
    const int key = 32 * cg + 16 * kf + (lane & 15);
    if (key >= P.Tk) continue;
    f32x4 tv = f32x4{0.f, 0.f, 0.f, 0.f}, tk = f32x4{0.f, 0.f, 0.f, 0.f};
    if (contrib) { tv = aV[kf]; tk = aK[kf] * P.scale; }
    float* wk = L.ws + (kbase + key) * HD + dcol;      // (not dereferenced when kv_share == 1: first and last)
    if (!first) {
      tk += *reinterpret_cast<const f32x4*>(wk);
      tv += *reinterpret_cast<const f32x4*>(wk + dv_off);
    }
    if (!last) {
      *reinterpret_cast<f32x4*>(wk) = tk;
      *reinterpret_cast<f32x4*>(wk + dv_off) = tv;
    } else {
      store4(P.dv + (kbase + key) * P.ldk + dcol, tv);
      store4(P.dk + (kbase + key) * P.ldk + dcol, tk);
    }
  }
}

template <int NQT>
__device__ __forceinline__ void attn_long_bwd_body(const AttnLongParams& L) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const AttnMfmaParams& P = L.a;
  char* Qs = smem;                               // NQT tiles
  char* dOs = Qs + NQT * TILE_B;                 // NQT tiles
  char* Ks = dOs + NQT * TILE_B;                 // the current 128-key tile
  char* Vs = Ks + TILE_B;
  char* PdT = Vs + TILE_B;                       // [32 keys][128 q] bf16 of the current (key chunk, query tile), 8 KiB
  char* dST = PdT + TILE_B / 2;                  // 8 KiB
  const int ks = blockIdx.x / P.heads, h = blockIdx.x % P.heads;
  const int64_t kbase = (int64_t)ks * P.Tk;
  const bf16_t* kp = P.k + kbase * P.ldk + h * AD;
  const bf16_t* vp = P.v + kbase * P.ldk + h * AD;
  const int ntiles = (P.Tk + AT - 1) / AT;
  // One workgroup per CU (NQT = 2) has the registers to hold the next tile while it computes; two per CU (NQT = 1, 256
  // registers each) overlap each other's loads instead.
  constexpr bool PREFETCH = NQT == 2;
  const f32x4 zero4[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};

#pragma unroll 1
  for (int sm = 0; sm < L.kv_share; ++sm) {
    // (the thread index is made opaque per group: otherwise every lane-dependent address and dropout term of the chunk loop is
    //  hoisted out of THIS loop too and stays live across the prologue, which costs ~100 spilled registers)
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63, w = tid >> 6;
    const int g = ks * L.kv_share + sm;
    const int64_t qbase = (int64_t)g * P.Tq;
    const float* mrow = P.mask ? P.mask + (int64_t)g * P.Tk : nullptr;
    float score_scale = P.scale;          // (0 for a group whose every key is hard-masked: see below)
    const bool live_any = !mrow || any_live_key(mrow, P.Tk, lane);
    const bool skip_dead = mrow && live_any;
    auto next_live = [&](int t) {
      while (skip_dead && t < ntiles && !any_live_in(mrow, P.Tk, t * AT, AT, lane)) ++t;
      return t;
    };
    int t = next_live(0);
    // ---- prologue of the group: Q and dO tiles, delta[q] = sum_d dO[q][d] O[q][d] and the logsumexp of the rows whose
    // values this lane's accumulator registers hold, the first live K / V tile
    float dl4[NQT][2][4], lse4[NQT][2][4];
    {
      TileRegs tq[NQT], td[NQT];
#pragma unroll
      for (int qt = 0; qt < NQT; ++qt) {
        tq[qt] = load_tile(P.q + (qbase + qt * AT) * P.ldq + h * AD, P.ldq, P.Tq - qt * AT, tid);
        td[qt] = load_tile(P.dout + (qbase + qt * AT) * P.ldo + h * AD, P.ldo, P.Tq - qt * AT, tid);
      }
      const TileRegs tk = load_tile(kp + (int64_t)t * AT * P.ldk, P.ldk, P.Tk - t * AT, tid);
      const TileRegs tv = load_tile(vp + (int64_t)t * AT * P.ldk, P.ldk, P.Tk - t * AT, tid);
#pragma unroll
      for (int qt = 0; qt < NQT; ++qt) {
        const int q = qt * AT + 32 * w + (lane >> 1), half = lane & 1;
        float sd = 0.f;
        if (q < P.Tq) {
          const bf16_t* a = P.dout + (qbase + q) * P.ldo + h * AD + 32 * half;
          const bf16_t* b = P.o + (qbase + q) * P.ldo + h * AD + 32 * half;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const bf16x8 x = *reinterpret_cast<const bf16x8*>(a + 8 * i);
            const bf16x8 y = *reinterpret_cast<const bf16x8*>(b + 8 * i);
#pragma unroll
            for (int j = 0; j < 8; ++j) sd += (float)x[j] * (float)y[j];
          }
        }
        sd += __shfl_xor(sd, 1, 64);
#pragma unroll
        for (int f = 0; f < 2; ++f)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int ql = 16 * f + 4 * (lane >> 4) + r;          // row inside the wave's 32
            dl4[qt][f][r] = __shfl(sd, 2 * ql, 64);
            const int q2 = qt * AT + 32 * w + ql;
            lse4[qt][f][r] = q2 < P.Tq ? P.lse[((int64_t)g * P.heads + h) * P.Tq + q2] : 0.f;
          }
      }
      __syncthreads();                     // the previous group is done with every image
#pragma unroll
      for (int qt = 0; qt < NQT; ++qt) {
        store_tile<false>(Qs + qt * TILE_B, tq[qt], tid);
        store_tile<false>(dOs + qt * TILE_B, td[qt], tid);
      }
      store_tile<false>(Ks, tk, tid);
      store_tile<false>(Vs, tv, tid);
    }
    __syncthreads();
    if (uniform_if_no_live_key(live_any, P.Tk, score_scale, lse4)) mrow = nullptr;
    bf16x8 qa[NQT][2][2], da[NQT][2][2], oT[NQT][4], qT[NQT][4];
    f32x4 aQ[NQT][4][2] = {};
#pragma unroll
    for (int qt = 0; qt < NQT; ++qt)
      bwd_resident_frags(Qs + qt * TILE_B, dOs + qt * TILE_B, w, lane, qa[qt], da[qt], oT[qt], qT[qt]);
    // (pair offsets: a query row below 2 AT + 2 times Tk / 2, plus a key)
    const BwdDropout D = bwd_dropout_state(P, g, h, lane, (uint64_t)(2 * AT + 2) * (uint64_t)(P.Tk >> 1) + (uint64_t)P.Tk + 1);

    // dead tiles before the first live one
#pragma unroll 1
    for (int cg = 0; cg < 4 * min(t, ntiles); ++cg) finish_chunk(L, kbase, h, w, lane, cg, sm, false, zero4, zero4);
#pragma unroll 1
    while (t < ntiles) {
      const int tn = next_live(t + 1);
      TileRegs nk, nv;
      if (PREFETCH && tn < ntiles) {          // next live tile's rows: in flight under this tile's arithmetic
        nk = load_tile(kp + (int64_t)tn * AT * P.ldk, P.ldk, P.Tk - tn * AT, tid);
        nv = load_tile(vp + (int64_t)tn * AT * P.ldk, P.ldk, P.Tk - tn * AT, tid);
      }
      const int rows = min(AT, P.Tk - t * AT);
#pragma unroll 1
      for (int c = 0; 32 * c < rows; ++c) {
        const int cg = 4 * t + c;               // global chunk index
        if (skip_dead && !any_live_in(mrow, P.Tk, 32 * cg, 32, lane)) {      // probabilities exactly 0: nothing for dQ, dK = dV = 0
          finish_chunk(L, kbase, h, w, lane, cg, sm, false, zero4, zero4);
          continue;
        }
        f32x4 aV[2], aK[2];
#pragma unroll
        for (int kf = 0; kf < 2; ++kf) { aV[kf] = f32x4{0.f, 0.f, 0.f, 0.f}; aK[kf] = f32x4{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
        for (int qt = 0; qt < NQT; ++qt) {
          float mk2[2];
#pragma unroll
          for (int k4 = 0; k4 < 2; ++k4) {
            const int key = 32 * cg + 16 * k4 + (lane & 15);
            mk2[k4] = (mrow && key < P.Tk) ? mrow[key] : 0.f;
          }
          bwd_chunk_phase1(P, D, Ks, Vs, PdT, dST, c, 32 * cg, qt * AT, mk2, score_scale, qa[qt], da[qt], lse4[qt], dl4[qt], w, lane);
          __syncthreads();
          bwd_chunk_phase2(Ks, PdT, dST, c, oT[qt], qT[qt], aQ[qt], aV, aK, w, lane);
          __syncthreads();   // the chunk images are rewritten by the next query tile / chunk
        }
        finish_chunk(L, kbase, h, w, lane, cg, sm, true, aV, aK);
      }
      // dead tiles between this one and the next live one
#pragma unroll 1
      for (int cg = 4 * (t + 1); cg < 4 * min(tn, ntiles); ++cg) finish_chunk(L, kbase, h, w, lane, cg, sm, false, zero4, zero4);
      if (tn < ntiles) {                      // (every wave passed the barrier that ends the tile's last chunk)
        if (!PREFETCH) {
          nk = load_tile(kp + (int64_t)tn * AT * P.ldk, P.ldk, P.Tk - tn * AT, tid);
          nv = load_tile(vp + (int64_t)tn * AT * P.ldk, P.ldk, P.Tk - tn * AT, tid);
        }
        store_tile<false>(Ks, nk, tid);
        store_tile<false>(Vs, nv, tid);
      }
      __syncthreads();
      t = tn;
    }
#pragma unroll
    for (int qt = 0; qt < NQT; ++qt)
#pragma unroll
      for (int f = 0; f < 2; ++f) {
        const int x = qt * AT + 32 * w + 16 * f + (lane & 15);
        if (x < P.Tq) {
          const int dcol = h * AD + 4 * (lane >> 4);
#pragma unroll
          for (int df = 0; df < 4; ++df) store4(P.dq + (qbase + x) * P.ldq + dcol + 16 * df, aQ[qt][df][f] * P.scale);
        }
      }
  }
}

__global__ __launch_bounds__(256, 2) void attn_long_bwd_kernel(AttnLongParams L) { attn_long_bwd_body<1>(L); }
__global__ __launch_bounds__(256, 1) void attn_long_bwd256_kernel(AttnLongParams L) { attn_long_bwd_body<2>(L); }

// =========================================================================================
// Probabilities of the long kernels: P = softmax(scale Q K^T + mask) as float32, before dropout, with the score and mask
// semantics of attn_long_fwd_kernel, per head [G, heads, Tq, Tk] or as the head mean [G, Tq, Tk].  No V, no logsumexp of a
// forward: a first pass over the keys leaves each row's maximum and 1 / sum (the running pair of the forward) in LDS, a second
// pass recomputes the scores, normalises and stores.  One workgroup owns a 128-query tile of `nh` heads of a group: one head
// (per-head mode, grid.x = G * heads) or all of them (head mean, grid.x = G).  In the second pass the heads are the INNER
// loop: the float32 sum over the heads, in ascending order, stays in the accumulator registers of the lane that stores the
// element -- once, with no per-head tensor in memory and no atomics, so two launches agree bit for bit.  Q K^T is computed
// twice; the kernel is bound by its writes.  Tiles whose keys are all hard-masked are not multiplied (unless the group has no
// live key at all), but their zeros are stored: the output is not initialised by the caller.
// Dynamic LDS: the K tile, the tile's 128 additive mask values, (maximum, 1 / sum) per (head, query of the tile).
struct AttnLongProbsParams {
  const bf16_t *q, *k;
  const float* mask;
  float* probs;
  int G, heads, Tq, Tk, kv_share, head_mean;
  int64_t ldq, ldk;
  float scale;
  int vec;      // every 4-key group of a row is 16-byte aligned: one 16-byte store per accumulator
};

// four consecutive keys of one output row (prow = the row's element of key `key`); keys at or past Tk are not written
__device__ __forceinline__ void store_probs4(float* prow, f32x4 v, int key, int Tk, bool vec) {
  if (vec) {      // Tk % 4 == 0: a group that starts inside the row ends inside it
    if (key < Tk) __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(prow));
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (key + r < Tk) prow[r] = v[r];
  }
}

__global__ __launch_bounds__(256, 2) void attn_long_probs_kernel(AttnLongProbsParams P) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Ks = smem;
  float* Ms = reinterpret_cast<float*>(smem + TILE_B);                    // [128] additive mask of the tile's keys, -inf past Tk
  float2* St = reinterpret_cast<float2*>(smem + TILE_B + AT * 4);         // [nh][128] (maximum, 1 / sum)
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int nh = P.head_mean ? P.heads : 1;
  const int g = P.head_mean ? blockIdx.x : blockIdx.x / P.heads;
  const int h0 = P.head_mean ? 0 : blockIdx.x % P.heads;
  const int q0 = blockIdx.y * AT + w * 32;
  const bool active = q0 < P.Tq;      // (wave-uniform: an idle wave only stages tiles and keeps the barriers matched)
  const bf16_t* kp = P.k + (int64_t)(g / P.kv_share) * P.Tk * P.ldk;
  const float* mrow = P.mask ? P.mask + (int64_t)g * P.Tk : nullptr;
  float* out = P.probs + (int64_t)(P.head_mean ? g : g * P.heads + h0) * P.Tq * P.Tk;
  const int ntiles = (P.Tk + AT - 1) / AT;
  const bool skip_dead = mrow && any_live_key(mrow, P.Tk, lane);
  auto next_live = [&](int t) {      // first tile >= t with a live key (the same in every wave: barriers stay matched)
    while (skip_dead && t < ntiles && !any_live_in(mrow, P.Tk, t * AT, AT, lane)) ++t;
    return t;
  };
  const int t_first = next_live(0);      // (< ntiles: tiles are skipped only when some key is live)
  // what one (head, tile) step reads, loaded a step ahead: the K tile, the tile's mask values, the head's Q fragments
  struct Step { TileRegs kt; float mk; bf16x8 qf[2][2]; };
  auto load_step = [&](int h, int t, Step& s) {
    s.kt = load_tile(kp + (int64_t)t * AT * P.ldk + (h0 + h) * AD, P.ldk, P.Tk - t * AT, tid);
    const int key = t * AT + tid;
    s.mk = (tid < AT && key < P.Tk) ? (mrow ? mrow[key] : 0.f) : -INFINITY;
    load_q_frags(P.q, P.ldq, P.Tq, g, h0 + h, q0, lane, s.qf);
  };
  auto stage_step = [&](const Step& s) {
    store_tile<false>(Ks, s.kt, tid);
    if (tid < AT) Ms[tid] = s.mk;
  };
  // scores of the staged tile: lane holds, for query q0 + 16 f + (lane & 15), keys k0 + 16 kf + 4 (lane >> 4) + r
  auto scores = [&](const bf16x8 (&qf)[2][2], int rows, f32x4 (&sc)[8][2]) {
    fwd_score_frags<8>([&](int x0, int s) { return frag_row64(Ks, x0, s, lane); }, qf, rows, sc);
#pragma unroll
    for (int kf = 0; kf < 8; ++kf) {
      if (16 * kf >= rows) continue;
      const f32x4 mk = *reinterpret_cast<const f32x4*>(Ms + 16 * kf + 4 * (lane >> 4));
#pragma unroll
      for (int f = 0; f < 2; ++f)
#pragma unroll
        for (int r = 0; r < 4; ++r) sc[kf][f][r] = sc[kf][f][r] * P.scale + mk[r];      // (-inf past Tk)
    }
  };

  // ---- zeros of the skipped tiles
  if (skip_dead && active) {
    const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int t = 0; t < ntiles; ++t) {
      if (any_live_in(mrow, P.Tk, t * AT, AT, lane)) continue;
      const int k0 = t * AT, rows = min(AT, P.Tk - k0);
#pragma unroll
      for (int f = 0; f < 2; ++f) {
        const int q = q0 + 16 * f + (lane & 15);
        if (q >= P.Tq) continue;
#pragma unroll
        for (int kf = 0; kf < 8; ++kf) {
          const int key = k0 + 16 * kf + 4 * (lane >> 4);
          if (16 * kf < rows) store_probs4(out + (int64_t)q * P.Tk + key, zero, key, P.Tk, P.vec);
        }
      }
    }
  }

  Step cur, nxt;
  // ---- pass 1: heads outside, live tiles inside: the running maximum and sum of every (head, row)
  {
    float m_run[2] = {-INFINITY, -INFINITY}, l_run[2] = {0.f, 0.f};
    int h = 0, t = t_first;
    load_step(h, t, cur);
#pragma unroll 1
    while (h < nh) {
      stage_step(cur);
      __syncthreads();
      int hn = h, tn = next_live(t + 1);
      if (tn >= ntiles) { hn = h + 1; tn = t_first; }
      if (hn < nh) load_step(hn, tn, nxt);      // in flight under this step's arithmetic
      if (active) {
        const int rows = min(AT, P.Tk - t * AT);
        f32x4 sc[8][2];
        scores(cur.qf, rows, sc);
#pragma unroll
        for (int f = 0; f < 2; ++f) {
          float m = -INFINITY;
#pragma unroll
          for (int kf = 0; kf < 8; ++kf) {
            if (16 * kf >= rows) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) m = fmaxf(m, sc[kf][f][r]);
          }
          m = fmaxf(m, __shfl_xor(m, 16, 64));
          m = fmaxf(m, __shfl_xor(m, 32, 64));
          const float m_new = fmaxf(m_run[f], m);            // (finite: every tile has a key below Tk)
          float sum = 0.f;
#pragma unroll
          for (int kf = 0; kf < 8; ++kf) {
            if (16 * kf >= rows) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) sum += __expf(sc[kf][f][r] - m_new);
          }
          sum += __shfl_xor(sum, 16, 64);
          sum += __shfl_xor(sum, 32, 64);
          l_run[f] = l_run[f] * __expf(m_run[f] - m_new) + sum;      // (factor 0 at the first tile)
          m_run[f] = m_new;
        }
        if (hn != h) {      // the head's last tile
#pragma unroll
          for (int f = 0; f < 2; ++f) {
            if ((lane >> 4) == 0) St[h * AT + 32 * w + 16 * f + lane] = make_float2(m_run[f], 1.0f / l_run[f]);
            m_run[f] = -INFINITY;
            l_run[f] = 0.f;
          }
        }
      }
      __syncthreads();                          // every wave is done with the images
      cur = nxt;
      h = hn; t = tn;
    }
  }
  // ---- pass 2: live tiles outside, heads inside: normalise, sum over the heads in registers, store each tile once
  {
    const float inv_heads = 1.0f / (float)nh;
    int t = t_first, h = 0;
    load_step(h, t, cur);
    f32x4 acc[8][2] = {};
#pragma unroll 1
    while (t < ntiles) {
      stage_step(cur);
      __syncthreads();                          // (also: the statistics of pass 1 are visible)
      int hn = h + 1, tn = t;
      if (hn == nh) { hn = 0; tn = next_live(t + 1); }
      if (tn < ntiles) load_step(hn, tn, nxt);
      if (active) {
        const int k0 = t * AT, rows = min(AT, P.Tk - k0);
        f32x4 sc[8][2];
        scores(cur.qf, rows, sc);
#pragma unroll
        for (int f = 0; f < 2; ++f) {
          const float2 st = St[h * AT + 32 * w + 16 * f + (lane & 15)];
#pragma unroll
          for (int kf = 0; kf < 8; ++kf) {
            if (16 * kf >= rows) continue;
            f32x4 p;
#pragma unroll
            for (int r = 0; r < 4; ++r) p[r] = __expf(sc[kf][f][r] - st.x) * st.y;
            acc[kf][f] = h == 0 ? p : acc[kf][f] + p;
          }
        }
        if (hn == 0) {      // the tile's last head
#pragma unroll
          for (int f = 0; f < 2; ++f) {
            const int q = q0 + 16 * f + (lane & 15);
            if (q >= P.Tq) continue;
#pragma unroll
            for (int kf = 0; kf < 8; ++kf) {
              const int key = k0 + 16 * kf + 4 * (lane >> 4);
              if (16 * kf < rows) store_probs4(out + (int64_t)q * P.Tk + key, acc[kf][f] * inv_heads, key, P.Tk, P.vec);
            }
          }
        }
      }
      __syncthreads();
      cur = nxt;
      h = hn; t = tn;
    }
  }
}

// =========================================================================================
constexpr int LONG_MAX_TK = 1 << 20;     // (q * Tk of the dropout counter is a 24-bit multiply; far above any visual token count)

extern "C" int fcmf_attn_mfma_long_fwd(const void* q, const void* k, const void* v, const float* mask, void* out, float* lse,
                                       int G, int heads, int Tq, int Tk, int kv_share, int64_t ldq, int64_t ldk, int64_t ldo,
                                       float scale, float dropout_p, uint64_t seed, void* stream) {
  if (!q || !k || !v || !out || G <= 0 || heads <= 0 || Tq <= 0 || Tk <= 0 || kv_share <= 0 || G % kv_share) return FCMF_ERR_ARG;
  if (Tq > 2 * AT || Tk > LONG_MAX_TK || ldq % 8 || ldk % 8 || ldo % 4 || !al16(q) || !al16(k) || !al16(v) || !al16(out))
    return FCMF_ERR_UNSUPPORTED;
  const AttnLongParams L{attn_mfma_params(q, k, v, mask, out, lse, G, heads, Tq, Tk, ldq, ldk, ldo, scale, dropout_p, seed), kv_share, nullptr};
  const dim3 grid(G * heads, (Tq + AT - 1) / AT);
  static bool attr = false;      // (this kernel's dynamic LDS is one constant: its limit is raised once)
  return fcmf_launch_flagged(&attr, attn_long_fwd_kernel, grid, dim3(256), 2 * TILE_B, reinterpret_cast<hipStream_t>(stream), L);
}

// bytes of the backward's float32 workspace: running sums of dK | dV, one row per key of every key set
static int64_t long_bwd_workspace(int G, int heads, int Tk, int kv_share) {
  return kv_share > 1 ? 2 * (int64_t)(G / kv_share) * Tk * heads * AD * (int64_t)sizeof(float) : 0;
}

extern "C" int fcmf_attn_mfma_long_bwd(const void* q, const void* k, const void* v, const float* mask, const void* out,
                                       const void* dout, const float* lse, void* dq, void* dk, void* dv, int G, int heads,
                                       int Tq, int Tk, int kv_share, int64_t ldq, int64_t ldk, int64_t ldo, float scale,
                                       float dropout_p, uint64_t seed, float* workspace, int64_t workspace_bytes, void* stream) {
  if (!q || !k || !v || !out || !dout || !lse || !dq || !dk || !dv || G <= 0 || heads <= 0 || Tq <= 0 || Tk <= 0 ||
      kv_share <= 0 || G % kv_share)
    return FCMF_ERR_ARG;
  if (kv_share > 1 && (!workspace || workspace_bytes < long_bwd_workspace(G, heads, Tk, kv_share))) return FCMF_ERR_ARG;
  if (Tq > 2 * AT || Tk > LONG_MAX_TK || ldq % 8 || ldk % 8 || ldo % 8 || !al16(q) || !al16(k) || !al16(v) || !al16(out) ||
      !al16(dout) || !al16(dq) || !al16(dk) || !al16(dv) || !al16(workspace))
    return FCMF_ERR_UNSUPPORTED;
  const AttnLongParams L{attn_mfma_params(q, k, v, mask, nullptr, const_cast<float*>(lse), G, heads, Tq, Tk, ldq, ldk, ldo, scale, dropout_p,
                                          seed, out, dout, dq, dk, dv),
                         kv_share, workspace};
  const dim3 grid((G / kv_share) * heads);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (Tq > AT) {
    static bool attr2 = false;      // (this kernel's dynamic LDS is one constant: its limit is raised once)
    return fcmf_launch_flagged(&attr2, attn_long_bwd256_kernel, grid, dim3(256), 7 * TILE_B, st, L);      // 112 KiB: one workgroup per CU
  }
  static bool attr = false;
  return fcmf_launch_flagged(&attr, attn_long_bwd_kernel, grid, dim3(256), 5 * TILE_B, st, L);          // 80 KiB: two per CU
}

// LDS of attn_long_probs_kernel for `nh` heads per workgroup
static size_t long_probs_lds(int nh) { return TILE_B + AT * sizeof(float) + (size_t)nh * AT * sizeof(float2); }

extern "C" int fcmf_attn_mfma_long_probs(const void* q, const void* k, const float* mask, float* probs, int G, int heads, int Tq,
                                         int Tk, int kv_share, int64_t ldq, int64_t ldk, float scale, int head_mean, void* stream) {
  if (!q || !k || !probs || G <= 0 || heads <= 0 || Tq <= 0 || Tk <= 0 || kv_share <= 0 || G % kv_share) return FCMF_ERR_ARG;
  if (Tq > 2 * AT || Tk > LONG_MAX_TK || ldq % 8 || ldk % 8 || !al16(q) || !al16(k) || (head_mean && heads > 32))
    return FCMF_ERR_UNSUPPORTED;      // (32 heads: 48.5 KiB of LDS, below the default dynamic limit)
  AttnLongProbsParams P{};
  P.q = (const bf16_t*)q; P.k = (const bf16_t*)k; P.mask = mask; P.probs = probs;
  P.G = G; P.heads = heads; P.Tq = Tq; P.Tk = Tk; P.kv_share = kv_share; P.head_mean = head_mean != 0;
  P.ldq = ldq; P.ldk = ldk; P.scale = scale;
  P.vec = Tk % 4 == 0 && al16(probs);
  const dim3 grid(head_mean ? G : G * heads, (Tq + AT - 1) / AT);
  return fcmf_launch(attn_long_probs_kernel, grid, dim3(256), long_probs_lds(head_mean ? heads : 1), reinterpret_cast<hipStream_t>(stream), P);
}
