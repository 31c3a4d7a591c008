// Tile images, MFMA operand fragments, the parameter block and the steps shared by the MFMA attention kernels (attn_mfma.hip:
// up to 256 keys resident in LDS; attn_long.hip: any number of keys streamed through it; attn_probs.hip: the probabilities of
// up to 256 keys).  bf16, head dim 64, 256-thread workgroups.
#pragma once
#include "common.h"

constexpr int AD = 64;             // head dim
constexpr int AT = 128;            // tile rows (queries / keys)
constexpr int TILE_B = AT * AD * 2;  // 16 KiB

// [rows][64 bf16] tile, 128-B rows: 32-B pair index XOR ((r>>1)&1 | ((r>>3)&1)<<1)
__device__ __forceinline__ int vkey(int r) { return ((r >> 1) & 1) | (((r >> 3) & 1) << 1); }
__device__ __forceinline__ int off64(int r, int c8) { return r * 128 + ((((c8 >> 1) ^ vkey(r))) << 5) + ((c8 & 1) << 4); }
// [32 keys][128 q bf16] chunk images of the backward (Pdrop^T, dS^T), 256-B rows: 16-B chunk XOR key16(row & 15), a GF(2)-linear key
// (bit columns 2, 4, 8, 9) under which BOTH read patterns are conflict free -- the ds_read_b128 operand reads of phase 2 (row = lane & 15,
// chunk = 4 s + (lane >> 4)) and the ds_read_b64_tr_b16 reads of dS^T (tools/lds_conflicts.py searches the 4 x 4 bit matrices; the
// ds_write_b64 of phase 1 puts 16 rows of one column into a 128-B bank window and is 2-way under any key).  The round-3 key
// ((r & 3) << 2 | (r >> 2) & 3) left every operand read 2-way: 30 % of the kernel's LDS cycles were bank conflicts (r03_attn_pmc.txt).
__device__ __forceinline__ int key16(int r) { return ((r & 7) << 1) ^ (((r >> 3) & 1) * 9); }
__device__ __forceinline__ int off128(int r, int ch) { return r * 256 + ((ch ^ key16(r)) << 4); }
// per-wave P tile of the forward [32][128 bf16]: chunk XOR (row & 15)
__device__ __forceinline__ int offp(int r, int ch) { return r * 256 + ((ch ^ (r & 15)) << 4); }

// forward-only V image: 32-B pair index XOR ((r>>1)&3), conflict free for the KEY-PERMUTED transposed reads
// (k-slot j of k-step s = key 32s + 4*(lane>>4) + (j&3) + 16*(j>>2): the order in which the S^T accumulator
// registers of two adjacent key fragments line up as an MFMA operand, so P never leaves the registers)
__device__ __forceinline__ int off64p(int r, int c8) { return r * 128 + ((((c8 >> 1) ^ ((r >> 1) & 3))) << 5) + ((c8 & 1) << 4); }

typedef bf16x4 __attribute__((address_space(3))) * lds_v4_t;

// A[row = tile column c0 + (lane&15)][k = keys in the permuted order above] from the off64p image
__device__ __forceinline__ bf16x8 frag_tr64p(const char* lds, int c0, int s, int lane) {
  const int g4 = lane >> 4, i16 = lane & 15, q4 = i16 >> 2, p = i16 & 3;
  const int r = 32 * s + 4 * g4 + q4, c8 = (c0 >> 3) + (p >> 1);
  bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_v4_t)(lds + off64p(r, c8) + (p & 1) * 8));
  bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_v4_t)(lds + off64p(r + 16, c8) + (p & 1) * 8));
  bf16x8 o;
  o[0] = lo[0]; o[1] = lo[1]; o[2] = lo[2]; o[3] = lo[3]; o[4] = hi[0]; o[5] = hi[1]; o[6] = hi[2]; o[7] = hi[3];
  return o;
}
// staging of a [rows<=128][64] bf16 tile (row stride ld elements, zero-filled) in two halves, load and store, so that a kernel
// can put ALL its tile loads in flight before the first LDS write (a fused form exposes one global round trip per tile)
struct TileRegs { uint4 v[4]; };
__device__ __forceinline__ TileRegs load_tile(const bf16_t* __restrict__ src, int64_t ld, int rows, int tid) {
  TileRegs t;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = tid + 256 * i, r = c >> 3, c8 = c & 7;
    t.v[i] = make_uint4(0, 0, 0, 0);
    if (r < rows) t.v[i] = *reinterpret_cast<const uint4*>(src + (int64_t)r * ld + c8 * 8);
  }
  return t;
}
// load_tile without a branch per piece: a row past the end reads the last valid row of the matrix instead (src[(rows - 1) * ld]
// must exist; rows may be <= 0 for a tile that starts past the end, as long as the matrix has a row before it) and zero_tail()
// clears it before store_tile.  hipcc turns every conditional piece of load_tile into a branch and gives up counting across them:
// it drains the loads in flight (vmcnt(0)) in the middle of a batch.  Unconditional loads stay one batch with one wait.
__device__ __forceinline__ TileRegs load_tile_clamped(const bf16_t* __restrict__ src, int64_t ld, int rows, int tid) {
  TileRegs t;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = tid + 256 * i, r = c >> 3, c8 = c & 7;
    t.v[i] = *reinterpret_cast<const uint4*>(src + (int64_t)min(r, rows - 1) * ld + c8 * 8);
  }
  return t;
}
__device__ __forceinline__ void zero_tail(TileRegs& t, int rows, int tid) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (((tid + 256 * i) >> 3) >= rows) t.v[i] = make_uint4(0, 0, 0, 0);
}
template <bool PERMUTED>
__device__ __forceinline__ void store_tile(char* lds, const TileRegs& t, int tid) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = tid + 256 * i, r = c >> 3, c8 = c & 7;
    *reinterpret_cast<uint4*>(lds + (PERMUTED ? off64p(r, c8) : off64(r, c8))) = t.v[i];
  }
}
// MFMA operand (rows x0..x0+15, k-step s over the 64 columns) by row read
__device__ __forceinline__ bf16x8 frag_row64(const char* lds, int x0, int s, int lane) {
  return *reinterpret_cast<const bf16x8*>(lds + off64(x0 + (lane & 15), 4 * s + (lane >> 4)));
}
// MFMA operand whose "row" index is the tile COLUMN (c0..c0+15) and whose k index is the tile ROW
// (32*s .. 32*s+31): transposed read of the row-major image
__device__ __forceinline__ bf16x8 frag_tr64(const char* lds, int c0, int s, int lane) {
  const int g4 = lane >> 4, i16 = lane & 15, q4 = i16 >> 2, p = i16 & 3;
  const int r = 32 * s + 8 * g4 + q4, c8 = (c0 >> 3) + (p >> 1);
  bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_v4_t)(lds + off64(r, c8) + (p & 1) * 8));
  bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_v4_t)(lds + off64(r + 4, c8) + (p & 1) * 8));
  bf16x8 o;
  o[0] = lo[0]; o[1] = lo[1]; o[2] = lo[2]; o[3] = lo[3]; o[4] = hi[0]; o[5] = hi[1]; o[6] = hi[2]; o[7] = hi[3];
  return o;
}
__device__ __forceinline__ bf16x8 frag_row128(const char* lds, int x0, int s, int lane) {
  return *reinterpret_cast<const bf16x8*>(lds + off128(x0 + (lane & 15), 4 * s + (lane >> 4)));
}
__device__ __forceinline__ bf16x8 frag_tr128(const char* lds, int c0, int s, int lane) {
  const int g4 = lane >> 4, i16 = lane & 15, q4 = i16 >> 2, p = i16 & 3;
  const int r = 32 * s + 8 * g4 + q4, ch = (c0 >> 3) + (p >> 1);
  bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_v4_t)(lds + off128(r, ch) + (p & 1) * 8));
  bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_v4_t)(lds + off128(r + 4, ch) + (p & 1) * 8));
  bf16x8 o;
  o[0] = lo[0]; o[1] = lo[1]; o[2] = lo[2]; o[3] = lo[3]; o[4] = hi[0]; o[5] = hi[1]; o[6] = hi[2]; o[7] = hi[3];
  return o;
}
__device__ __forceinline__ void store4(bf16_t* p, f32x4 v) {
  bf16x4 o;
  o[0] = (bf16_t)v[0]; o[1] = (bf16_t)v[1]; o[2] = (bf16_t)v[2]; o[3] = (bf16_t)v[3];
  *reinterpret_cast<bf16x4*>(p) = o;
}

// sum over the 16 lanes of a DPP row (lanes 16i .. 16i+15), result in every lane: four row rotations as DPP operands of
// the adds -- no LDS crossbar traffic (ds_bpermute), which a __shfl_xor butterfly would cost
__device__ __forceinline__ float row16_sum(float x) {
#define FCMF_ROR_ADD(n) x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x120 + (n), 0xf, 0xf, true))
  FCMF_ROR_ADD(8); FCMF_ROR_ADD(4); FCMF_ROR_ADD(2); FCMF_ROR_ADD(1);
#undef FCMF_ROR_ADD
  return x;
}

struct AttnMfmaParams {
  const bf16_t *q, *k, *v, *o, *dout;
  const float* mask;
  bf16_t *out, *dq, *dk, *dv;
  float* lse;
  float* colsum;       // backward, optional: [G][3 * heads * 64] f32, row g = column sums of dq | dk | dv of sequence g
  int G, heads, Tq, Tk;
  int64_t ldq, ldk, ldo;
  float scale, p;
  uint64_t seed;
};

// host side of the MFMA attention entry points (attn_mfma.hip, attn_long.hip, attn_probs.hip)
static inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
// the C arguments of an entry point as the parameter block: the forwards pass out / lse and stop at the seed, the backwards
// pass out = nullptr and the forward's output as o
static inline AttnMfmaParams attn_mfma_params(const void* q, const void* k, const void* v, const float* mask, void* out, float* lse, int G,
                                              int heads, int Tq, int Tk, int64_t ldq, int64_t ldk, int64_t ldo, float scale, float p,
                                              uint64_t seed, const void* o = nullptr, const void* dout = nullptr, void* dq = nullptr,
                                              void* dk = nullptr, void* dv = nullptr, float* colsum = nullptr) {
  AttnMfmaParams P{};
  P.q = (const bf16_t*)q; P.k = (const bf16_t*)k; P.v = (const bf16_t*)v; P.mask = mask; P.out = (bf16_t*)out; P.lse = lse;
  P.o = (const bf16_t*)o; P.dout = (const bf16_t*)dout; P.dq = (bf16_t*)dq; P.dk = (bf16_t*)dk; P.dv = (bf16_t*)dv; P.colsum = colsum;
  P.G = G; P.heads = heads; P.Tq = Tq; P.Tk = Tk; P.ldq = ldq; P.ldk = ldk; P.ldo = ldo;
  P.scale = scale; P.p = p; P.seed = seed;
  return P;
}

// Q fragments of the wave's 32 query rows straight from global memory in operand layout (16 B per lane)
__device__ __forceinline__ void load_q_frags(const bf16_t* q, int64_t ldq, int Tq, int g, int h, int q0, int lane,
                                             bf16x8 (&qf)[2][2]) {
#pragma unroll
  for (int f = 0; f < 2; ++f)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int row = q0 + 16 * f + (lane & 15);
      uint4 v = make_uint4(0, 0, 0, 0);
      if (row < Tq) v = *reinterpret_cast<const uint4*>(q + ((int64_t)g * Tq + row) * ldq + h * AD + 32 * s + 8 * (lane >> 4));
      qf[f][s] = *reinterpret_cast<bf16x8*>(&v);
    }
}
// the same without a branch per fragment (see load_tile_clamped): rows past Tq read row Tq - 1; zero_q_tail() clears them
__device__ __forceinline__ void load_q_frags_clamped(const AttnMfmaParams& P, int g, int h, int q0, int lane, bf16x8 (&qf)[2][2]) {
#pragma unroll
  for (int f = 0; f < 2; ++f)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int row = min(q0 + 16 * f + (lane & 15), P.Tq - 1);
      const uint4 v = *reinterpret_cast<const uint4*>(P.q + ((int64_t)g * P.Tq + row) * P.ldq + h * AD + 32 * s + 8 * (lane >> 4));
      qf[f][s] = *reinterpret_cast<const bf16x8*>(&v);
    }
}
__device__ __forceinline__ void zero_q_tail(const AttnMfmaParams& P, int q0, int lane, bf16x8 (&qf)[2][2]) {
#pragma unroll
  for (int f = 0; f < 2; ++f)
    if (q0 + 16 * f + (lane & 15) >= P.Tq) {
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j) qf[f][s][j] = (bf16_t)0.f;
    }
}

// =========================================================================================
// Steps shared by the kernels.  Forward (attn_mfma.hip, attn_long.hip): the score step and the P V step of one tile of NKF
// 16-key fragments.  Backward (attn_mfma.hip, attn_long.hip): the two phases of one (32-key chunk, query
// tile) step and what they need around them.

// index of the last key among 0 .. 64 N - 1 that is below Tk and not hard-masked (mask > -1e30), -1 if there is none
// (wave-uniform); mask_of(i, key) = the additive mask of key = 64 i + lane, read only for keys below Tk
template <int N, class MaskOf>
__device__ __forceinline__ int last_live_key(MaskOf mask_of, int Tk, int lane) {
  int last = -1;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const int key = 64 * i + lane;
    const unsigned long long b = __ballot(key < Tk && mask_of(i, key) > -1e30f);
    if (b) last = 64 * i + 63 - __builtin_clzll(b);
  }
  return last;
}

// Score step: S^T[key][q] = K Q^T of the tile (kfrag(x0, s) = operand of key rows x0 .. x0 + 15, k-step s, from the
// caller's K image); fragments that start at or past `nkeys` are skipped (their sc stays 0).  The lane holds, for query
// q0 + 16 f + (lane & 15), keys 16 kf + 4 (lane >> 4) + r.  (Scale + mask + row maximum stay in the kernels, and
// attn_probs_mfma_kernel keeps its own loop: as functions here they cost the forwards up to 4 % and that kernel 2 - 16 % --
// the compiler then keeps more saved exec masks than it has scalar registers; profiles/r15_attn_shared_steps.txt.)
template <int NKF, class KFrag>
__device__ __forceinline__ void fwd_score_frags(KFrag kfrag, const bf16x8 (&qf)[2][2], int nkeys, f32x4 (&sc)[NKF][2]) {
#pragma unroll
  for (int kf = 0; kf < NKF; ++kf)
#pragma unroll
    for (int f = 0; f < 2; ++f) sc[kf][f] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int kf = 0; kf < NKF; ++kf) {
      if (16 * kf >= nkeys) continue;
      const bf16x8 ka = kfrag(16 * kf, s);
#pragma unroll
      for (int f = 0; f < 2; ++f) sc[kf][f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ka, qf[f][s], sc[kf][f], 0, 0, 0);
    }
}
// P V step: O^T[d][q] += sum_key V[key][d] P[q][key], the P^T operand of k-step s straight from the accumulators of key
// fragments 2s and 2s+1, V from its off64p image
template <int NKF>
__device__ __forceinline__ void fwd_pv_step(const char* Vs, const f32x4 (&sc)[NKF][2], int nkeys, int lane, f32x4 (&oc)[4][2]) {
#pragma unroll
  for (int s = 0; s < NKF / 2; ++s) {
    if (32 * s >= nkeys) continue;
    bf16x8 pb[2];
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
      for (int r = 0; r < 4; ++r) { pb[f][r] = (bf16_t)sc[2 * s][f][r]; pb[f][4 + r] = (bf16_t)sc[2 * s + 1][f][r]; }
#pragma unroll
    for (int df = 0; df < 4; ++df) {
      const bf16x8 va = frag_tr64p(Vs, 16 * df, s, lane);
#pragma unroll
      for (int f = 0; f < 2; ++f) oc[df][f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(va, pb[f], oc[df][f], 0, 0, 0);
    }
  }
}

// ---- backward
// operands of one query tile that stay in registers: the wave's 32 query rows of Q and dO (phase 1), the transposed
// 16-column slices dO^T / Q^T [d = 16w ..][q] that dV / dK of every key chunk multiply (phase 2).  (The dQ accumulators are
// zeroed where the callers declare them: zeroed through a reference here, attn_long_bwd_kernel spills 128 bytes per lane more.)
__device__ __forceinline__ void bwd_resident_frags(const char* Qs, const char* dOs, int w, int lane, bf16x8 (&qa)[2][2], bf16x8 (&da)[2][2],
                                                   bf16x8 (&oT)[4], bf16x8 (&qT)[4]) {
#pragma unroll
  for (int f = 0; f < 2; ++f)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      qa[f][s] = frag_row64(Qs, 32 * w + 16 * f, s, lane);
      da[f][s] = frag_row64(dOs, 32 * w + 16 * f, s, lane);
    }
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    oT[s] = frag_tr64(dOs, 16 * w, s, lane);     // A[row = d][k = q]
    qT[s] = frag_tr64(Qs, 16 * w, s, lane);
  }
}
// A sequence with no live key: softmax is uniform over ALL keys, and the forward's logsumexp is finfo.min itself (log Tk is
// absorbed), from which exp(s + mask - lse) would recompute probabilities of 1 instead of 1 / Tk.  Wave-uniform substitution,
// no per-element work: zero the score scale and take lse = log Tk; returns true when the caller must drop its mask as well.
template <int NQT>
__device__ __forceinline__ bool uniform_if_no_live_key(bool live_any, int Tk, float& score_scale, float (&lse4)[NQT][2][4]) {
  if (live_any) return false;
  score_scale = 0.f;
  const float ltk = __logf((float)Tk);
#pragma unroll
  for (int qt = 0; qt < NQT; ++qt)
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
      for (int r = 0; r < 4; ++r) lse4[qt][f][r] = ltk;
  return true;
}

// Dropout of one (sequence, head) in the backward, with the mask shared between neighbouring lanes.  One hash decides the element
// PAIR (q, key & ~1), (q, key | 1); in phase 1 the two elements sit in lanes l and l ^ 1 (key = .. + (lane & 15)), each holding rows
// q0 .. q0+3 -- computed per element, both lanes would evaluate the same four hashes (two 32-bit multiplies each, quarter rate: two
// thirds of the backward's vector instructions).  Even lanes hash rows q0, q0+1, odd lanes q0+2, q0+3, and a quad-permute DPP
// move swaps them: two hashes per four elements.  Needs an even Tk (then every row starts on a pair boundary); the high word of
// the 64-bit pair index is wave-uniform unless the low word wraps inside this (sequence, head): pair_span = a bound of the
// caller's pair offsets; if the low word could wrap within it, the per-element form is used.
struct BwdDropout {
  bool share_hash;
  uint32_t pb_lo, hash_k0, hash_s1, thr;
  float inv_keep;
  uint64_t drop_base;      // dropout counter of (query 0, key 0)
  int odd;                 // lane & 1
};
__device__ __forceinline__ BwdDropout bwd_dropout_state(const AttnMfmaParams& P, int g, int h, int lane, uint64_t pair_span) {
  BwdDropout D;
  D.inv_keep = P.p > 0.f ? 1.0f / (1.0f - P.p) : 1.0f;
  D.drop_base = ((uint64_t)g * P.heads + h) * P.Tq * P.Tk;
  const uint64_t pair_base = D.drop_base >> 1;
  const uint32_t pb_hi = (uint32_t)(pair_base >> 32);
  D.pb_lo = (uint32_t)pair_base;
  D.share_hash = P.p > 0.f && (P.Tk & 1) == 0 && (uint64_t)D.pb_lo + pair_span <= 0xFFFFFFFFull;
  D.hash_k0 = (uint32_t)P.seed ^ ((pb_hi << 7) | (pb_hi >> 25));
  D.hash_s1 = (uint32_t)(P.seed >> 32);
  D.thr = dropout_threshold(P.p);
  D.odd = lane & 1;
  return D;
}
// multipliers of (q0 + r, key), r = 0..3, under share_hash (key & 1 == lane & 1)
__device__ __forceinline__ void pair_dropout_mult4(const BwdDropout& D, unsigned q0, int key, int Tk, float (&mult4)[4]) {
  const int odd = D.odd;
  const uint32_t o0 = D.pb_lo + __umul24(q0 + 2 * odd, (unsigned)Tk >> 1) + ((unsigned)key >> 1);
  const uint32_t hA = fcmf_hash32_rounds(o0 ^ D.hash_k0, D.hash_s1);
  const uint32_t hB = fcmf_hash32_rounds((o0 + ((unsigned)Tk >> 1)) ^ D.hash_k0, D.hash_s1);
  const uint32_t nA = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)hA, 0xB1, 0xf, 0xf, true);   // quad_perm [1,0,3,2]: lane ^ 1
  const uint32_t nB = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)hB, 0xB1, 0xf, 0xf, true);
  const uint32_t hr[4] = {odd ? nA : hA, odd ? nB : hB, odd ? hA : nA, odd ? hB : nB};
#pragma unroll
  for (int r = 0; r < 4; ++r) mult4[r] = ((hr[r] >> (16 * odd)) & 0xFFFFu) >= D.thr ? D.inv_keep : 0.f;
}

// One (32-key chunk, 128-query tile) step of the backward, in two phases with a barrier of the caller's between them and
// another behind them (the chunk images are rewritten by the next step).  Ks / Vs: images that hold the chunk's keys in rows
// 32 c .. 32 c + 31; key0 = the first of them in the sequence; qt0 = first query of the tile; mk2[k4] = additive mask of key
// key0 + 16 k4 + (lane & 15); qa / da / oT / qT / lse4 / dl4 / aQ: the tile's (bwd_resident_frags).
// Phase 1 (wave = 32 query rows): Pdrop^T and dS^T [key][q] of (chunk, tile) into the two chunk images, P recomputed from
// the logsumexp.
__device__ __forceinline__ void bwd_chunk_phase1(const AttnMfmaParams& P, const BwdDropout& D, const char* Ks, const char* Vs, char* PdT,
                                                 char* dST, int c, int key0, int qt0, const float (&mk2)[2], float score_scale,
                                                 const bf16x8 (&qa)[2][2], const bf16x8 (&da)[2][2], const float (&lse4)[2][4],
                                                 const float (&dl4)[2][4], int w, int lane) {
  f32x4 sS[2][2], sP[2][2];
#pragma unroll
  for (int k4 = 0; k4 < 2; ++k4)
#pragma unroll
    for (int f = 0; f < 2; ++f) { sS[k4][f] = f32x4{0.f, 0.f, 0.f, 0.f}; sP[k4][f] = f32x4{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int k4 = 0; k4 < 2; ++k4) {
      const bf16x8 kb = frag_row64(Ks, 32 * c + 16 * k4, s, lane);
      const bf16x8 vb = frag_row64(Vs, 32 * c + 16 * k4, s, lane);
#pragma unroll
      for (int f = 0; f < 2; ++f) {
        sS[k4][f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa[f][s], kb, sS[k4][f], 0, 0, 0);   // D[q][key]
        sP[k4][f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(da[f][s], vb, sP[k4][f], 0, 0, 0);
      }
    }
#pragma unroll
  for (int k4 = 0; k4 < 2; ++k4) {
    const int kl = 16 * k4 + (lane & 15), key = key0 + kl;
    const float mk = mk2[k4];
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      f32x4 pdv, dsv;
      float mult4[4] = {1.0f, 1.0f, 1.0f, 1.0f};
      if (D.share_hash) pair_dropout_mult4(D, qt0 + 32 * w + 16 * f + 4 * (lane >> 4), key, P.Tk, mult4);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int q = qt0 + 32 * w + 16 * f + 4 * (lane >> 4) + r;
        float pr = 0.f, mult = mult4[r];
        if (key < P.Tk && q < P.Tq) pr = __expf(sS[k4][f][r] * score_scale + mk - lse4[f][r]);
        // element index ((g heads + h) Tq + q) Tk + key = a wave-uniform 64-bit base + a small 24-bit product: no
        // 64-bit vector multiply per element (integer multiplies are quarter rate; the kernel is VALU-bound)
        if (P.p > 0.f && !D.share_hash)
          mult = dropout_mult(P.seed, D.drop_base + (__umul24((unsigned)q, (unsigned)P.Tk) + (unsigned)key), P.p, D.inv_keep);
        pdv[r] = pr * mult;
        dsv[r] = pr * (sP[k4][f][r] * mult - dl4[f][r]);
      }
      const int ch = 4 * w + 2 * f + (lane >> 5);
      const int o = off128(kl, ch) + ((lane >> 4) & 1) * 8;
      store4(reinterpret_cast<bf16_t*>(PdT + o), pdv);
      store4(reinterpret_cast<bf16_t*>(dST + o), dsv);
    }
  }
}
// Phase 2: dQ^T[d][q] += K^T[d][keys of the chunk] dS^T[keys][q] (wave = 32 queries), then
// dV^T / dK^T [d = 16w..][key of the chunk] += dO^T / Q^T [d][q of this tile] x Pdrop / dS [q][key] (wave = 16 columns)
__device__ __forceinline__ void bwd_chunk_phase2(const char* Ks, const char* PdT, const char* dST, int c, const bf16x8 (&oT)[4],
                                                 const bf16x8 (&qT)[4], f32x4 (&aQ)[4][2], f32x4 (&aV)[2], f32x4 (&aK)[2], int w, int lane) {
  bf16x8 tb[2];
#pragma unroll
  for (int f = 0; f < 2; ++f) tb[f] = frag_tr128(dST, 32 * w + 16 * f, 0, lane);    // B[k = key][col = q]
#pragma unroll
  for (int df = 0; df < 4; ++df) {
    const bf16x8 ka2 = frag_tr64(Ks, 16 * df, c, lane);                              // A[row = d][k = key]
#pragma unroll
    for (int f = 0; f < 2; ++f) aQ[df][f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ka2, tb[f], aQ[df][f], 0, 0, 0);
  }
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int kf = 0; kf < 2; ++kf) {
      const bf16x8 pb = frag_row128(PdT, 16 * kf, s, lane);   // B[k = q][col = key]
      const bf16x8 sb = frag_row128(dST, 16 * kf, s, lane);
      aV[kf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(oT[s], pb, aV[kf], 0, 0, 0);
      aK[kf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qT[s], sb, aK[kf], 0, 0, 0);
    }
}
