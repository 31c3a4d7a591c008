// Two-segment multi-head attention, forward and backward, VALU f32 math, any activation dtype.
// One workgroup = one (group g, head h).  The T1 shared keys/values and a block of query rows (with dO in
// the backward) are staged once in LDS; one WAVE owns one query row at a time: its scores over the shared
// keys run one key per lane out of LDS, its T2 private keys are scored one key per lane (the lane walks its key's
// row with 16-byte loads) and their values / keys are accumulated 8 keys x 64 dims per wave instruction (head
// dim 64) or one key per step with the head dimension across the lanes (other head dims).  The
// backward is two passes per row block: pass A (wave = row) builds the dropped probabilities and score
// gradients [row][key] in LDS and finishes dq / dbias (and dk2 / dv2 rows, unless the private keys are shared by a
// group of sequences: then attn_private_grad_kernel sums them over the group), pass B (wave = shared key) reduces
// them over the rows into dk1 / dv1 -- two workgroup barriers per row block, no per-row global round trips.
// Used for every attention on the path in fp32 (parity) mode and, in bf16 mode, for the dead-row-pruned
// fusion layers (1 live query row per image), the 15-token fusion layer, the geometry-biased ROI attention
// and the IAOG decoder; the bf16 text-encoder attention runs on attn_mfma.hip instead.
// Three kernel families (ATTN_SMALL_KERNELS lists every instantiation): the general two-segment kernels below, the all-in-LDS
// "dense" kernels (tiny: one shared segment of <= 128 keys on the matrix cores; rows_flat: <= 16 query rows) built from the
// phases of the second part, and attn_private_grad_kernel.  The host side is attn_small_plan (descriptor -> kernel, grid, LDS:
// no HIP call) and run_plan (the only place that launches).
#include "attn_tiles.h"   // al16

constexpr int AS_MAXT = 512;   // T1 + T2 <= 512 (forward: KPL = 4 or 8 keys per lane; FCMF-large fuses 256 text + 100 ROI keys)
constexpr int AS_MAXD = 128;   // head dim <= 128 (two elements per lane)

struct AttnK {
  fcmf_attn_desc a;
  void* out; float* lse;
  const void* dout; const void* o_in;
  void *dq, *dk1, *dv1, *dk2, *dv2; float* dbias;
  float *pd2, *ds2;            // backward, grouped private keys: [G][heads][R][T2] dropped probabilities / score gradients
  int RB;                      // query rows staged per block (host: what fits the LDS budget)
  int TLP;                     // pitch of the per-row key arrays of the backward (max keys a block sees)
  int KVF;                     // floats occupied by the staged shared K and V images
};

// stage n rows of a (.., t, h, :) tensor into an f32 LDS image with row pitch `pitch`.  Aligned rows go 16 bytes
// per lane, several rows per wave instruction, four instructions in flight per wave; otherwise lanes run across
// the head dimension (coalesced) one row at a time.
template <typename TT, typename TD>   // TD = float (converted) or TT (raw copy: shared keys/values stay in the activation dtype)
__device__ __forceinline__ void stage_rows(TD* dst, int pitch, const TT* src, int64_t row_stride, int n, int d, int w, int lane,
                                           int nw = 4) {
  constexpr int V = 16 / sizeof(TT);
  const bool vec = d % V == 0 && row_stride % V == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0;
  if (vec) {
    const int lpr = d / V, rpi = 64 / lpr;            // lanes per row, rows per wave instruction
    const int rl = lane / lpr, ch = lane - rl * lpr;
    const bool on = rl < rpi;
    for (int t0 = w * rpi; t0 < n; t0 += 4 * nw * rpi) {   // nw waves x 4 instructions per round
      uint4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int t = t0 + u * nw * rpi + rl;
        v[u] = make_uint4(0, 0, 0, 0);
        if (on && t < n) v[u] = *reinterpret_cast<const uint4*>(src + (int64_t)t * row_stride + ch * V);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int t = t0 + u * nw * rpi + rl;
        if (on && t < n) {
          TD* o = dst + t * pitch + ch * V;
          if constexpr (sizeof(TD) == sizeof(TT)) {
            *reinterpret_cast<uint4*>(o) = v[u];
          } else if constexpr (sizeof(TT) == 2) {
            const bf16x8 x = *reinterpret_cast<const bf16x8*>(&v[u]);
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = (float)x[j];
          } else {
            const float4 x = *reinterpret_cast<const float4*>(&v[u]);
            o[0] = x.x; o[1] = x.y; o[2] = x.z; o[3] = x.w;
          }
        }
      }
    }
  } else {
    for (int t = w; t < n; t += nw) {
      const TT* sr = src + (int64_t)t * row_stride;
      for (int c = lane; c < d; c += 64) {
        if constexpr (sizeof(TD) == sizeof(TT)) dst[t * pitch + c] = sr[c];
        else dst[t * pitch + c] = to_f32<TT>(sr[c]);
      }
    }
  }
}

// <x, row> out of LDS (x f32, a broadcast; row in the activation dtype): rows with a 16-byte aligned pitch are
// read 16 bytes at a time
template <typename TT>
__device__ __forceinline__ float lds_dot(const float* __restrict__ x, const TT* __restrict__ row, int d, bool v16) {
  float s = 0.f;
  constexpr int V = 16 / sizeof(TT);
  if (v16) {
    for (int c = 0; c < d; c += V) {
      if constexpr (sizeof(TT) == 2) {
        const bf16x8 b = *reinterpret_cast<const bf16x8*>(row + c);
        const float4 a0 = *reinterpret_cast<const float4*>(x + c), a1 = *reinterpret_cast<const float4*>(x + c + 4);
        s += a0.x * (float)b[0] + a0.y * (float)b[1] + a0.z * (float)b[2] + a0.w * (float)b[3] +
             a1.x * (float)b[4] + a1.y * (float)b[5] + a1.z * (float)b[6] + a1.w * (float)b[7];
      } else {
        const float4 a = *reinterpret_cast<const float4*>(x + c), b = *reinterpret_cast<const float4*>(row + c);
        s += a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
      }
    }
  } else {
    for (int c = 0; c < d; ++c) s += x[c] * to_f32<TT>(row[c]);
  }
  return s;
}

// <q, row> and <q2, row2> for one private key held by this lane: the lane walks its own global row with 16-byte
// loads (all of them independent, so they are in flight together; q comes from LDS as a broadcast)
template <typename TT>
__device__ __forceinline__ void dot2_row(const float* __restrict__ qa, const TT* __restrict__ ra, const float* __restrict__ qb,
                                         const TT* __restrict__ rb, int d, bool vec, float& sa, float& sb) {
  sa = 0.f; sb = 0.f;
  constexpr int V = 16 / sizeof(TT);
  if (vec) {
    for (int c = 0; c < d; c += V) {
      if constexpr (sizeof(TT) == 2) {
        const bf16x8 x = *reinterpret_cast<const bf16x8*>(ra + c);
#pragma unroll
        for (int j = 0; j < 8; ++j) sa += qa[c + j] * (float)x[j];
        if (rb) {
          const bf16x8 y = *reinterpret_cast<const bf16x8*>(rb + c);
#pragma unroll
          for (int j = 0; j < 8; ++j) sb += qb[c + j] * (float)y[j];
        }
      } else {
        const float4 x = *reinterpret_cast<const float4*>(ra + c);
        sa += qa[c] * x.x + qa[c + 1] * x.y + qa[c + 2] * x.z + qa[c + 3] * x.w;
        if (rb) {
          const float4 y = *reinterpret_cast<const float4*>(rb + c);
          sb += qb[c] * y.x + qb[c + 1] * y.y + qb[c + 2] * y.z + qb[c + 3] * y.w;
        }
      }
    }
  } else {
    for (int c = 0; c < d; ++c) {
      sa += qa[c] * to_f32<TT>(ra[c]);
      if (rb) sb += qb[c] * to_f32<TT>(rb[c]);
    }
  }
}
template <typename TT>
__device__ __forceinline__ bool private_rows_vectorisable(const fcmf_attn_desc& a) {
  constexpr int V = 16 / sizeof(TT);
  return a.T2 > 0 && a.d % V == 0 && a.k2_sg % V == 0 && a.k2_sr % V == 0 && a.k2_st % V == 0 &&
         (reinterpret_cast<uintptr_t>(a.k2) & 15) == 0 && (reinterpret_cast<uintptr_t>(a.v2) & 15) == 0;
}

// One wave's softmax with dropout over row r of (g, h), KPL keys per lane: sc[n] = score of key lane + 64 n (-inf past T).  The
// dropped probabilities go to dst[t], the row's logsumexp to P.lse.  Used by every forward of this file.  DIV: p = e / sum (the
// tiny kernels) instead of e * (1 / sum) -- the two round differently, and each family keeps the bits it has always produced.
template <int KPL, bool DIV>
__device__ __forceinline__ void softmax_dropout_row(float (&sc)[KPL], int T, int lane, const AttnK& P, int g, int h, int r, float inv_keep,
                                                    float* dst) {
  const fcmf_attn_desc& a = P.a;
  float m = -INFINITY;
#pragma unroll
  for (int n = 0; n < KPL; ++n) m = fmaxf(m, sc[n]);
  m = wave_max(m);
  float sum = 0.f;
#pragma unroll
  for (int n = 0; n < KPL; ++n) {
    sc[n] = lane + 64 * n < T ? __expf(sc[n] - m) : 0.f;
    sum += sc[n];
  }
  sum = wave_sum(sum);
  const float inv = 1.0f / sum;
#pragma unroll
  for (int n = 0; n < KPL; ++n) {
    const int t = lane + 64 * n;
    if (t < T) {
      float pv = DIV ? sc[n] / sum : sc[n] * inv;
      if (a.dropout_p > 0.f) pv *= dropout_mult(a.seed, (((uint64_t)g * a.heads + h) * a.R + r) * T + t, a.dropout_p, inv_keep);
      dst[t] = pv;
    }
  }
  if (lane == 0 && P.lse) P.lse[((int64_t)g * a.heads + h) * a.R + r] = m + __logf(sum);
}

// DC = head dimension when it is 64 (the text / fusion layers of FCMF: loops unroll, the 16-byte loads of a private key
// row are all in flight together; 274 -> 120 us on the step's two fusion attentions), 0 = taken from the descriptor.
// (Eight waves per workgroup -- one per query row of the 7-row fusion layers -- were measured slower than four.)
template <typename TT, int KPL, int DC>
__global__ __launch_bounds__(256) void attn_small_fwd_kernel(AttnK P) {
  constexpr int NW = 4;
  constexpr int PMAX = 64 * KPL;          // keys a wave's probability row can hold
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const fcmf_attn_desc& a = P.a;
  const int d = DC ? DC : a.d;
  const int T1 = a.T1, T2 = a.T2, T = T1 + T2, RB = P.RB;
  constexpr int V16 = 16 / sizeof(TT);
  const bool v4 = d % V16 == 0;         // 16-byte LDS accesses throughout
  const int dp = v4 ? d + V16 : d + 1;  // K/V row pitch (elements): +16 B keeps 16-byte reads of 16 lanes on distinct banks; else odd
  TT* K1s = reinterpret_cast<TT*>(sm);
  TT* V1s = K1s + T1 * dp;
  float* Qs = sm + P.KVF;               // [RB][d] (KVF = floats taken by the two K/V images)
  float* ps = Qs + RB * d;              // [NW][PMAX] probability row of each wave
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int g = blockIdx.x / a.heads, h = blockIdx.x % a.heads;
  const int hin = a.head_quirk ? (int)(((int64_t)h * a.G + g) % a.heads) : h;
  const int g2 = g / a.group_div;
  const TT* Q = reinterpret_cast<const TT*>(a.q);
  const TT* K2 = reinterpret_cast<const TT*>(a.k2);
  const TT* V2 = reinterpret_cast<const TT*>(a.v2);
  TT* O = reinterpret_cast<TT*>(P.out);
  if (T1 > 0) {
    stage_rows<TT, TT>(K1s, dp, reinterpret_cast<const TT*>(a.k1) + (int64_t)g * a.k1_sg + hin * d, a.k1_st, T1, d, w, lane, NW);
    stage_rows<TT, TT>(V1s, dp, reinterpret_cast<const TT*>(a.v1) + (int64_t)g * a.k1_sg + hin * d, a.k1_st, T1, d, w, lane, NW);
  }
  const float inv_keep = a.dropout_p > 0.f ? 1.0f / (1.0f - a.dropout_p) : 1.0f;
  float* p = ps + w * PMAX;
  const bool vec2 = private_rows_vectorisable<TT>(a);
  for (int rb0 = 0; rb0 < a.R; rb0 += RB) {
    const int nr = min(RB, a.R - rb0);
    stage_rows<TT, float>(Qs, d, Q + (int64_t)g * a.q_sg + (int64_t)rb0 * a.q_sr + hin * d, a.q_sr, nr, d, w, lane, NW);
    __syncthreads();
    for (int rl = w; rl < nr; rl += NW) {
      const int r = rb0 + rl;
      const float* q = Qs + rl * d;
      float sc[KPL];
#pragma unroll
      for (int n = 0; n < KPL; ++n) {
        const int t = lane + 64 * n;
        float accv = 0.f;
        if (t < T1) {
          accv = lds_dot<TT>(q, K1s + t * dp, d, v4);
        } else if (t < T) {   // private key: this lane walks its own row
          float dummy;
          dot2_row<TT>(q, K2 + (int64_t)g2 * a.k2_sg + (int64_t)r * a.k2_sr + (int64_t)(t - T1) * a.k2_st + hin * d, nullptr,
                       (const TT*)nullptr, d, vec2, accv, dummy);
        }
        sc[n] = accv;
      }
#pragma unroll
      for (int n = 0; n < KPL; ++n) {
        const int t = lane + 64 * n;
        float s = -INFINITY;
        if (t < T) {
          s = sc[n] * a.scale;
          if (a.mask) s += a.mask[(int64_t)g * T + t];
          if (a.bias) s += a.bias[(((int64_t)g2 * a.heads + h) * a.R + r) * T + t];
          if (a.causal && t > r) s = -1e4f;
        }
        sc[n] = s;
      }
      softmax_dropout_row<KPL, false>(sc, T, lane, P, g, h, r, inv_keep, p);
      // out[c] = sum_t p[t] v[t][c]: lanes across the head dimension (p is read back by the wave that wrote it)
      float o0 = 0.f, o1 = 0.f;
      {
        int t = 0;
        for (; v4 && t + 4 <= T1; t += 4) {
          const float4 pv = *reinterpret_cast<const float4*>(p + t);
          const TT* vr = V1s + t * dp;
          auto f = [&](int i) { return to_f32<TT>(vr[i]); };
          if (lane < d) o0 += pv.x * f(lane) + pv.y * f(dp + lane) + pv.z * f(2 * dp + lane) + pv.w * f(3 * dp + lane);
          if (lane + 64 < d) o1 += pv.x * f(lane + 64) + pv.y * f(dp + lane + 64) + pv.z * f(2 * dp + lane + 64) + pv.w * f(3 * dp + lane + 64);
        }
        for (; t < T1; ++t) {
          const float pv = p[t];
          if (lane < d) o0 += pv * to_f32<TT>(V1s[t * dp + lane]);
          if (lane + 64 < d) o1 += pv * to_f32<TT>(V1s[t * dp + lane + 64]);
        }
      }
      if (T2 > 0 && DC == 64 && sizeof(TT) == 2 && vec2) {
        // private values, 16 bytes per lane: lane = (key t2 % 8, 8-dim slice): one wave instruction covers 8 keys x 64
        // dims, every instruction of the row is in flight before the first use; the 8 key groups are then summed across
        // lanes (lanes that share lane & 7 hold the same dims)
        const TT* vb = V2 + (int64_t)g2 * a.k2_sg + (int64_t)r * a.k2_sr + hin * d + (lane & 7) * 8;
        const int kg = lane >> 3;
        float acc8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int t0 = 0; t0 < T2; t0 += 32) {
          bf16x8 x[4];
          float pw[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int t2 = t0 + 8 * u + kg;
            pw[u] = 0.f;
            x[u] = bf16x8{};
            if (t2 < T2) { x[u] = *reinterpret_cast<const bf16x8*>(vb + (int64_t)t2 * a.k2_st); pw[u] = p[T1 + t2]; }
          }
#pragma unroll
          for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc8[j] += pw[u] * (float)x[u][j];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float t = acc8[j];
          t += __shfl_xor(t, 8, 64); t += __shfl_xor(t, 16, 64); t += __shfl_xor(t, 32, 64);
          acc8[j] = t;
        }
        // lane l < 64 owns dim l: it sits in slice l >> 3, element l & 7 -- held by every lane with (lane & 7) == l >> 3
        float mine = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float t = __shfl(acc8[j], lane >> 3, 64);     // from lane (l >> 3): its slice is l >> 3
          if ((lane & 7) == j) mine = t;
        }
        o0 += mine;
      } else if (T2 > 0) {
        const TT* vb = V2 + (int64_t)g2 * a.k2_sg + (int64_t)r * a.k2_sr + hin * d;
#pragma unroll 8
        for (int t2 = 0; t2 < T2; ++t2) {
          const float pv = p[T1 + t2];
          const TT* vr = vb + (int64_t)t2 * a.k2_st;
          if (lane < d) o0 += pv * to_f32<TT>(vr[lane]);
          if (lane + 64 < d) o1 += pv * to_f32<TT>(vr[lane + 64]);
        }
      }
      TT* orow = O + (int64_t)g * a.o_sg + (int64_t)r * a.o_sr + h * d;
      if (lane < d) orow[lane] = from_f32<TT>(o0);
      if (lane + 64 < d) orow[lane + 64] = from_f32<TT>(o1);
    }
    __syncthreads();   // the row block is restaged
  }
}

// Backward.  grid = (G*heads, ceil(T1/128)): block (.., c) owns the shared keys [128c, 128c+128) (their
// dK1/dV1 accumulate in registers across the row blocks, so no atomics are needed) and, for c == 0, the
// private keys.  Each chunk writes its partial dq to dq[c] (dense [chunks,G,R,heads*d]); the host sums the
// chunks.  dk1/dv1 are dense [G,T1,heads*d].
// ONE_BLOCK: all R rows fit one staged block (the usual case): dk1/dv1 are final after pass B and go straight
// to memory; otherwise they accumulate in registers across the row blocks.
// Grouped private keys (P.pd2 != nullptr): rows of `group_div` consecutive groups share their private keys (the six
// aspects of a review), so dk2 / dv2 are sums over the group.  Pass A then only stores the private keys' dropped
// probabilities and score gradients (a few KB per workgroup) and attn_private_grad_kernel forms the sums -- instead of
// one dk2 / dv2 row pair per (group, row, key) written here and summed by another pass (6x the bytes, twice).
// (Four waves and a run-time head dimension: eight waves per workgroup and a compile-time d = 64 were both measured
// SLOWER here -- 180 VGPRs instead of 88 halve the resident waves.)
template <typename TT, bool ONE_BLOCK, bool GROUPED>
__global__ __launch_bounds__(256) void attn_small_bwd_kernel(AttnK P) {
  constexpr int NW = 4;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const fcmf_attn_desc& a = P.a;
  const int d = a.d, T1 = a.T1, T2 = a.T2, T = T1 + T2, RB = P.RB;
  constexpr int V16 = 16 / sizeof(TT);
  const bool v4 = d % V16 == 0;
  const int dp = v4 ? d + V16 : d + 1;
  const int chunk = blockIdx.y, kc0 = chunk * 128;
  const int T1c = min(128, T1 - kc0);                 // shared keys of this chunk (may be <= 0 if T1 == 0)
  const int T2c = chunk == 0 ? T2 : 0;                // private keys are handled by chunk 0
  const int nsh = T1c > 0 ? T1c : 0;
  const int TL = nsh + T2c;                           // keys this block sees: local index tl
  TT* K1s = reinterpret_cast<TT*>(sm);
  TT* V1s = K1s + nsh * dp;
  float* Qs = sm + P.KVF;            // [RB][d]
  float* dOs = Qs + RB * d;          // [RB][d]
  const int TLP = P.TLP;
  float* PD = dOs + RB * d;          // [RB][TLP] dropped probabilities
  float* DS = PD + RB * TLP;         // [RB][TLP] score gradients
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int g = blockIdx.x / a.heads, h = blockIdx.x % a.heads;
  const int hin = a.head_quirk ? (int)(((int64_t)h * a.G + g) % a.heads) : h;
  const int g2 = g / a.group_div;
  const int64_t HD = (int64_t)a.heads * d;
  const TT* Q = reinterpret_cast<const TT*>(a.q);
  const TT* K2 = reinterpret_cast<const TT*>(a.k2);
  const TT* V2 = reinterpret_cast<const TT*>(a.v2);
  const TT* O = reinterpret_cast<const TT*>(P.o_in);
  const TT* dO = reinterpret_cast<const TT*>(P.dout);
  TT* dQ = reinterpret_cast<TT*>(P.dq) + (int64_t)chunk * a.G * a.R * HD;
  TT* dK1 = reinterpret_cast<TT*>(P.dk1);
  TT* dV1 = reinterpret_cast<TT*>(P.dv1);
  TT* dK2 = reinterpret_cast<TT*>(P.dk2);
  TT* dV2 = reinterpret_cast<TT*>(P.dv2);
  if (nsh > 0) {
    stage_rows<TT, TT>(K1s, dp, reinterpret_cast<const TT*>(a.k1) + (int64_t)g * a.k1_sg + (int64_t)kc0 * a.k1_st + hin * d, a.k1_st, nsh, d, w, lane, NW);
    stage_rows<TT, TT>(V1s, dp, reinterpret_cast<const TT*>(a.v1) + (int64_t)g * a.k1_sg + (int64_t)kc0 * a.k1_st + hin * d, a.k1_st, nsh, d, w, lane, NW);
  }
  constexpr int NACC = ONE_BLOCK ? 1 : 128 / NW;      // shared keys of a chunk per wave: w + NW n
  float accK[NACC][2], accV[NACC][2];
#pragma unroll
  for (int n = 0; n < NACC; ++n) { accK[n][0] = accK[n][1] = accV[n][0] = accV[n][1] = 0.f; }
  const bool kv_same = (P.dv1 == nullptr);
  const float inv_keep = a.dropout_p > 0.f ? 1.0f / (1.0f - a.dropout_p) : 1.0f;
  const bool vec2 = private_rows_vectorisable<TT>(a);

  for (int rb0 = 0; rb0 < a.R; rb0 += RB) {
    const int nr = min(RB, a.R - rb0);
    stage_rows<TT, float>(Qs, d, Q + (int64_t)g * a.q_sg + (int64_t)rb0 * a.q_sr + hin * d, a.q_sr, nr, d, w, lane, NW);
    stage_rows<TT, float>(dOs, d, dO + (int64_t)g * a.o_sg + (int64_t)rb0 * a.o_sr + h * d, a.o_sr, nr, d, w, lane, NW);
    __syncthreads();
    // ---- pass A: wave = query row ---------------------------------------------------------------
    for (int rl = w; rl < nr; rl += NW) {
      const int r = rb0 + rl;
      const float* q = Qs + rl * d;
      const float* dov = dOs + rl * d;
      float* pd = PD + rl * TLP;
      float* ds = DS + rl * TLP;
      const float q0 = lane < d ? q[lane] : 0.f, q1 = lane + 64 < d ? q[lane + 64] : 0.f;
      const float o0 = lane < d ? dov[lane] : 0.f, o1 = lane + 64 < d ? dov[lane + 64] : 0.f;
      float delta;
      {
        const TT* orow = O + (int64_t)g * a.o_sg + (int64_t)r * a.o_sr + h * d;
        float part = 0.f;
        if (lane < d) part = o0 * to_f32<TT>(orow[lane]);
        if (lane + 64 < d) part += o1 * to_f32<TT>(orow[lane + 64]);
        delta = wave_sum(part);
      }
      // raw scores and dO.v per key: local key tl = lane + 64 n  (shared chunk keys first, then private)
      float sv[4], dv[4];
      const int64_t p2 = (int64_t)g2 * a.k2_sg + (int64_t)r * a.k2_sr + hin * d;
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        const int tl = lane + 64 * n;
        float s = 0.f, dpd = 0.f;
        if (tl < nsh) {
          s = lds_dot<TT>(q, K1s + tl * dp, d, v4);
          dpd = lds_dot<TT>(dov, V1s + tl * dp, d, v4);
        } else if (tl < TL) {   // private key: this lane walks its own rows of K2 and V2
          const int64_t o2 = p2 + (int64_t)(tl - nsh) * a.k2_st;
          dot2_row<TT>(q, K2 + o2, dov, V2 + o2, d, vec2, s, dpd);
        }
        sv[n] = s; dv[n] = dpd;
      }
      const float lse_r = P.lse[((int64_t)g * a.heads + h) * a.R + r];
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        const int tl = lane + 64 * n;
        if (tl < TL) {
          const int t = tl < nsh ? kc0 + tl : T1 + (tl - nsh);   // global key index
          float s = sv[n] * a.scale;
          if (a.mask) s += a.mask[(int64_t)g * T + t];
          if (a.bias) s += a.bias[(((int64_t)g2 * a.heads + h) * a.R + r) * T + t];
          const bool filled = a.causal && t > r;
          if (filled) s = -1e4f;
          // (a row whose every key carries the hard finfo.min mask: its logsumexp IS finfo.min -- log T is absorbed -- and the
          //  probabilities are uniform, as torch's softmax gives them)
          const float pr = lse_r <= -1e30f ? 1.0f / (float)T : __expf(s - lse_r);
          float mult = 1.0f;
          if (a.dropout_p > 0.f)
            mult = dropout_mult(a.seed, (((uint64_t)g * a.heads + h) * a.R + r) * T + t, a.dropout_p, inv_keep);
          const float dsv = filled ? 0.f : pr * (dv[n] * mult - delta);
          pd[tl] = pr * mult;
          ds[tl] = dsv;
          if (P.dbias) P.dbias[(((int64_t)g * a.heads + h) * a.R + r) * T + t] = dsv;
          if (GROUPED && tl >= nsh) {
            const int64_t i2 = (((int64_t)g * a.heads + h) * a.R + r) * T2 + (tl - nsh);
            P.pd2[i2] = pr * mult;
            P.ds2[i2] = dsv;
          }
        }
      }
      // dq[c] = scale * sum_t ds[t] k[t][c]; private keys also get their dk2 / dv2 rows (outer products)
      float dq0 = 0.f, dq1 = 0.f;
      {
        int tl = 0;
        for (; v4 && tl + 4 <= nsh; tl += 4) {
          const float4 dsv = *reinterpret_cast<const float4*>(ds + tl);
          const TT* kr = K1s + tl * dp;
          auto f = [&](int i) { return to_f32<TT>(kr[i]); };
          if (lane < d) dq0 += dsv.x * f(lane) + dsv.y * f(dp + lane) + dsv.z * f(2 * dp + lane) + dsv.w * f(3 * dp + lane);
          if (lane + 64 < d) dq1 += dsv.x * f(lane + 64) + dsv.y * f(dp + lane + 64) + dsv.z * f(2 * dp + lane + 64) + dsv.w * f(3 * dp + lane + 64);
        }
        for (; tl < nsh; ++tl) {
          const float dsv = ds[tl];
          if (lane < d) dq0 += dsv * to_f32<TT>(K1s[tl * dp + lane]);
          if (lane + 64 < d) dq1 += dsv * to_f32<TT>(K1s[tl * dp + lane + 64]);
        }
      }
      if (GROUPED && T2c > 0 && d == 64 && sizeof(TT) == 2 && vec2) {
        // grouped private keys: only dq needs them here.  16 bytes per lane, lane = (key t2 % 8, 8-dim slice): every load
        // of the row is in flight before the first use; the 8 key groups are summed across lanes afterwards
        const TT* kb = K2 + p2 + (lane & 7) * 8;
        const int kg = lane >> 3;
        float acc8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int t0 = 0; t0 < T2c; t0 += 32) {
          bf16x8 x[4];
          float wgt[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int t2 = t0 + 8 * u + kg;
            wgt[u] = 0.f;
            x[u] = bf16x8{};
            if (t2 < T2c) { x[u] = *reinterpret_cast<const bf16x8*>(kb + (int64_t)t2 * a.k2_st); wgt[u] = ds[nsh + t2]; }
          }
#pragma unroll
          for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc8[j] += wgt[u] * (float)x[u][j];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float t = acc8[j];
          t += __shfl_xor(t, 8, 64); t += __shfl_xor(t, 16, 64); t += __shfl_xor(t, 32, 64);
          acc8[j] = t;
        }
        float mine = 0.f;          // lane l owns dim l = slice l >> 3, element l & 7
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float t = __shfl(acc8[j], lane >> 3, 64);
          if ((lane & 7) == j) mine = t;
        }
        dq0 += mine;
      } else if (GROUPED) {
#pragma unroll 4
        for (int t2 = 0; t2 < T2c; ++t2) {
          const float dsv = ds[nsh + t2];
          const TT* kr = K2 + p2 + (int64_t)t2 * a.k2_st;
          if (lane < d) dq0 += dsv * to_f32<TT>(kr[lane]);
          if (lane + 64 < d) dq1 += dsv * to_f32<TT>(kr[lane + 64]);
        }
      } else
#pragma unroll 4
      for (int t2 = 0; t2 < T2c; ++t2) {
        const float dsv = ds[nsh + t2], pv = pd[nsh + t2];
        const TT* kr = K2 + p2 + (int64_t)t2 * a.k2_st;
        const int64_t dst = (((int64_t)g * a.R + r) * T2 + t2) * HD + h * d;
        if (lane < d) {
          dq0 += dsv * to_f32<TT>(kr[lane]);
          dK2[dst + lane] = from_f32<TT>(dsv * a.scale * q0);
          dV2[dst + lane] = from_f32<TT>(pv * o0);
        }
        if (lane + 64 < d) {
          dq1 += dsv * to_f32<TT>(kr[lane + 64]);
          dK2[dst + lane + 64] = from_f32<TT>(dsv * a.scale * q1);
          dV2[dst + lane + 64] = from_f32<TT>(pv * o1);
        }
      }
      TT* dqrow = dQ + ((int64_t)g * a.R + r) * HD + h * d;
      if (lane < d) dqrow[lane] = from_f32<TT>(dq0 * a.scale);
      if (lane + 64 < d) dqrow[lane + 64] = from_f32<TT>(dq1 * a.scale);
    }
    __syncthreads();
    // ---- pass B: wave = shared key (w + 4n): reduce over the rows of the block -----------------------
    auto key_sums = [&](int tl, float& k0, float& k1, float& v0, float& v1) {
      k0 = k1 = v0 = v1 = 0.f;
      for (int rl = 0; rl < nr; ++rl) {
        const float dsv = DS[rl * TLP + tl], pv = PD[rl * TLP + tl];
        if (lane < d) { k0 += dsv * Qs[rl * d + lane]; v0 += pv * dOs[rl * d + lane]; }
        if (lane + 64 < d) { k1 += dsv * Qs[rl * d + lane + 64]; v1 += pv * dOs[rl * d + lane + 64]; }
      }
      k0 *= a.scale; k1 *= a.scale;
    };
    auto write_key = [&](int tl, float k0, float k1, float v0, float v1) {
      const int64_t off = ((int64_t)g * T1 + kc0 + tl) * HD + h * d;
      if (lane < d) {
        dK1[off + lane] = from_f32<TT>(kv_same ? k0 + v0 : k0);
        if (!kv_same) dV1[off + lane] = from_f32<TT>(v0);
      }
      if (lane + 64 < d) {
        dK1[off + lane + 64] = from_f32<TT>(kv_same ? k1 + v1 : k1);
        if (!kv_same) dV1[off + lane + 64] = from_f32<TT>(v1);
      }
    };
    if constexpr (ONE_BLOCK) {
      for (int tl = w; tl < nsh; tl += NW) {
        float k0, k1, v0, v1;
        key_sums(tl, k0, k1, v0, v1);
        write_key(tl, k0, k1, v0, v1);
      }
    } else {
#pragma unroll
      for (int n = 0; n < NACC; ++n) {
        const int tl = w + NW * n;
        if (tl < nsh) {
          float k0, k1, v0, v1;
          key_sums(tl, k0, k1, v0, v1);
          accK[n][0] += k0; accK[n][1] += k1; accV[n][0] += v0; accV[n][1] += v1;
        }
      }
      __syncthreads();   // the row block is restaged
      if (rb0 + RB >= a.R) {
#pragma unroll
        for (int n = 0; n < NACC; ++n) {
          const int tl = w + NW * n;
          if (tl < nsh) write_key(tl, accK[n][0], accK[n][1], accV[n][0], accV[n][1]);
        }
      }
    }
  }
}

// dk2 / dv2 of grouped private keys: block = (g2, r) = one set of T2 private keys; thread = output column c (head c / d):
//   dk2[g2][r][t2][c] = scale * sum_a ds2[g2*gd + a][head][r][t2] * q[g2*gd + a][r][c]
//   dv2[g2][r][t2][c] =         sum_a pd2[...]                     * dO[g2*gd + a][r][c]
// (pd2 / ds2 of the group staged in LDS as [a][head][t2]; every output row is one coalesced store)
template <typename TT>
__global__ __launch_bounds__(256) void attn_private_grad_kernel(AttnK P) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const fcmf_attn_desc& a = P.a;
  const int d = a.d, T2 = a.T2, gd = a.group_div, heads = a.heads, HD = heads * d;
  const int g2 = blockIdx.x / a.R, r = blockIdx.x % a.R;
  const int tb = (T2 + gridDim.y - 1) / gridDim.y, t_lo = blockIdx.y * tb, t_hi = min(T2, t_lo + tb);   // this block's keys
  const int nt = t_hi - t_lo;              // this block's keys only (every block staged all T2 keys of the group: 4x the gather)
  float* PD = sm;                          // [gd][heads][nt]
  float* DS = sm + gd * heads * tb;
  for (int i = threadIdx.x; i < gd * heads * nt; i += 256) {
    const int tl = i % nt, ah = i / nt, hh = ah % heads, aa = ah / heads;
    const int64_t src = ((((int64_t)g2 * gd + aa) * heads + hh) * a.R + r) * T2 + t_lo + tl;
    PD[i] = P.pd2[src];
    DS[i] = P.ds2[src];
  }
  __syncthreads();
  const TT* Q = reinterpret_cast<const TT*>(a.q);
  const TT* dO = reinterpret_cast<const TT*>(P.dout);
  TT* dK2 = reinterpret_cast<TT*>(P.dk2);
  TT* dV2 = reinterpret_cast<TT*>(P.dv2);
  for (int c = threadIdx.x; c < HD; c += 256) {
    const int hh = c / d;
    float qv[8], ov[8];
#pragma unroll
    for (int aa = 0; aa < 8; ++aa) {
      qv[aa] = ov[aa] = 0.f;
      if (aa < gd) {
        const int64_t g = (int64_t)g2 * gd + aa;
        qv[aa] = to_f32<TT>(Q[g * a.q_sg + (int64_t)r * a.q_sr + c]) * a.scale;
        ov[aa] = to_f32<TT>(dO[g * a.o_sg + (int64_t)r * a.o_sr + c]);
      }
    }
    const int64_t out0 = (((int64_t)g2 * a.R + r) * T2) * HD + c;
    for (int t2 = t_lo; t2 < t_hi; ++t2) {
      float kacc = 0.f, vacc = 0.f;
#pragma unroll
      for (int aa = 0; aa < 8; ++aa)
        if (aa < gd) {
          kacc += DS[(aa * heads + hh) * nt + t2 - t_lo] * qv[aa];
          vacc += PD[(aa * heads + hh) * nt + t2 - t_lo] * ov[aa];
        }
      dK2[out0 + (int64_t)t2 * HD] = from_f32<TT>(kacc);
      dV2[out0 + (int64_t)t2 * HD] = from_f32<TT>(vacc);
    }
  }
}

// =========================================================================================================================
// The dense kernels: bf16, no causal fill, every operand of one (group, head) in LDS, a few flat, fully parallel loops instead
// of the general kernels' wave-per-row rounds of dependent LDS / reduction latencies.  Same arithmetic, same dropout counters,
// same outputs as the general kernels.  Two families share one LDS layout and the phases below:
//   tiny       one shared key segment, <= 128 rows x 128 keys (the geometry-biased ROI attention: 36 x 36, 8 heads of 96; 4 us of
//              arithmetic per (group, head)): thread = (row, key) scores -- on the matrix cores when d % 32 == 0 --, wave = row
//              softmax, thread = (row, 8 columns) outputs, thread = (key, 8 columns) dK / dV;
//   rows_flat  <= 16 query rows against <= 128 shared keys and / or each row's private keys, no bias (the step's two fusion
//              attentions: 7 [CLS] rows, one per image): the private keys' K2 / V2 rows come straight from global memory and
//              thread = (row, 8 columns, quarter of the keys) forms the outputs / dq; the private keys of grouped sequences
//              leave through the pd2 / ds2 scratch exactly as in the general kernel.
// =========================================================================================================================
constexpr int TINY_MAX = 64;        // rows / keys of the one-block kernels
constexpr int TINY_WIDE_MAX = 128;  // ... of the wide forward / row-blocked backward (LDS permitting)
constexpr size_t TINY_LDS = 160 * 1024, FLAT_LDS = 64 * 1024;

// The LDS layout of the dense kernels, for the host (bytes = the launch's dynamic LDS) and for the kernels (their pointers):
//   bf16 images, row pitch dp = d + 8:   Q [R][dp] | dO [R][dp] (backward only) | K [T1][dp] | V [T1][dp]
//   f32 arrays, row pitch TP = T1+T2+1:  PD [rows][TP] (forward: the scores, then the dropped probabilities)
//                                        | DS [rows][TP] score offsets, then score gradients | delta [R]      (backward only)
// rows = R, or the row block of attn_tiny_bwd_blocked_kernel.  frag_pad (the tiny kernels): frag_xyT reads 16 rows at a time,
// so up to 15 rows (15 dp bf16) past the end of the last image it is given -- K in the forward, where V and the scores follow, V
// in the backward, where the f32 arrays follow (counted at min(R, 16) rows: no launch has fewer).  Where that is less than the
// 15 rows, a pad at the end of the allocation makes up the difference.
struct AttnDenseLds {
  int q, dout, k, v;     // in bf16 elements from the start of the dynamic LDS
  int pd, ds, delta;     // in floats
  size_t row_bytes;      // one more row of the f32 arrays
  size_t bytes;          // everything, pad included
};
__host__ __device__ inline AttnDenseLds attn_dense_lds(int R, int rows, int T1, int T2, int d, bool backward, bool frag_pad) {
  const int dp = d + 8, TP = T1 + T2 + 1;
  AttnDenseLds L;
  L.q = 0;
  L.dout = R * dp;
  L.k = backward ? 2 * R * dp : R * dp;
  L.v = L.k + T1 * dp;
  L.pd = (L.v + T1 * dp) / 2;
  L.ds = L.pd + rows * TP;
  L.delta = backward ? L.ds + rows * TP : L.ds;
  L.row_bytes = sizeof(float) * (backward ? 2 : 1) * (size_t)TP;
  L.bytes = sizeof(float) * (size_t)(backward ? L.delta + R : L.ds);
  const size_t over = (size_t)15 * dp * 2;
  const size_t behind = backward ? sizeof(float) * ((size_t)2 * (R < 16 ? R : 16) * TP + R) : (size_t)T1 * dp * 2 + sizeof(float) * (size_t)R * TP;
  if (frag_pad && behind < over) L.bytes += over - behind;
  return L;
}

// <a, b> over d bf16 (d % 8 == 0, 16-byte aligned rows; a in LDS, b in LDS or global memory).  v_dot2c_f32_bf16: two bf16
// products added to an f32 accumulator per instruction, no conversions (two interleaved accumulation chains)
__device__ __forceinline__ float dot_bf16(const bf16_t* a, const bf16_t* __restrict__ b, int d) {
  typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
  float s0 = 0.f, s1 = 0.f;
  for (int c = 0; c < d; c += 8) {
    const bf16x8 x = *reinterpret_cast<const bf16x8*>(a + c), y = *reinterpret_cast<const bf16x8*>(b + c);
    s0 = __builtin_amdgcn_fdot2_f32_bf16(bf16x2_t{x[0], x[1]}, bf16x2_t{y[0], y[1]}, s0, false);
    s1 = __builtin_amdgcn_fdot2_f32_bf16(bf16x2_t{x[2], x[3]}, bf16x2_t{y[2], y[3]}, s1, false);
    s0 = __builtin_amdgcn_fdot2_f32_bf16(bf16x2_t{x[4], x[5]}, bf16x2_t{y[4], y[5]}, s0, false);
    s1 = __builtin_amdgcn_fdot2_f32_bf16(bf16x2_t{x[6], x[7]}, bf16x2_t{y[6], y[7]}, s1, false);
  }
  return s0 + s1;
}

// one 16 x 16 fragment of X Y^T out of two row-major LDS images (rows of d bf16, pitch dp, d % 32 == 0) on the matrix cores:
// v_mfma_f32_16x16x32_bf16 wants 8 consecutive k per lane for row (lane & 15) of either operand at k offset 8 (lane >> 4) --
// the same 16-byte read for both (pitch 2 (d + 8) bytes: the 16 rows of a quarter wave start in distinct bank groups).  The lane
// ends up with rows x0 + 4 (lane >> 4) + i, i = 0..3, of column y0 + (lane & 15).  Rows past the end of an operand read whatever
// follows it inside the workgroup's LDS allocation (attn_dense_lds) and only reach outputs that are never stored.
__device__ __forceinline__ f32x4 frag_xyT(const bf16_t* X, const bf16_t* Y, int dp, int d, int x0, int y0, int lane) {
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  const bf16_t* xr = X + (x0 + (lane & 15)) * dp + (lane >> 4) * 8;
  const bf16_t* yr = Y + (y0 + (lane & 15)) * dp + (lane >> 4) * 8;
  for (int k0 = 0; k0 < d; k0 += 32)
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8*>(xr + k0), *reinterpret_cast<const bf16x8*>(yr + k0), acc, 0, 0, 0);
  return acc;
}

// ---- the phases ----------------------------------------------------------------------------------------------------------
// the images of head h of group g: Q (and dO), shared K and V
__device__ __forceinline__ void stage_head(bf16_t* img, const AttnDenseLds& L, const AttnK& P, int g, int h, int w, int lane, bool backward) {
  const fcmf_attn_desc& a = P.a;
  const int d = a.d, dp = d + 8;
  stage_rows<bf16_t, bf16_t>(img + L.q, dp, reinterpret_cast<const bf16_t*>(a.q) + (int64_t)g * a.q_sg + h * d, a.q_sr, a.R, d, w, lane);
  if (backward)
    stage_rows<bf16_t, bf16_t>(img + L.dout, dp, reinterpret_cast<const bf16_t*>(P.dout) + (int64_t)g * a.o_sg + h * d, a.o_sr, a.R, d, w, lane);
  if (a.T1 > 0) {
    stage_rows<bf16_t, bf16_t>(img + L.k, dp, reinterpret_cast<const bf16_t*>(a.k1) + (int64_t)g * a.k1_sg + h * d, a.k1_st, a.T1, d, w, lane);
    stage_rows<bf16_t, bf16_t>(img + L.v, dp, reinterpret_cast<const bf16_t*>(a.v1) + (int64_t)g * a.k1_sg + h * d, a.k1_st, a.T1, d, w, lane);
  }
}

// delta[r] = <dO[r], O[r]> straight from global memory: wave = row
__device__ __forceinline__ void delta_rows(float* dl, const AttnK& P, int g, int h, int w, int lane) {
  const fcmf_attn_desc& a = P.a;
  for (int r = w; r < a.R; r += 4) {
    const int64_t row = (int64_t)g * a.o_sg + (int64_t)r * a.o_sr + h * a.d;
    const bf16_t* orow = reinterpret_cast<const bf16_t*>(P.o_in) + row;
    const bf16_t* drow = reinterpret_cast<const bf16_t*>(P.dout) + row;
    float part = 0.f;
    for (int c = lane; c < a.d; c += 64) part += (float)drow[c] * (float)orow[c];
    part = wave_sum(part);
    if (lane == 0) dl[r] = part;
  }
}

// score offsets of the rows [r0, r0 + rb) into DS: + mask + bias - logsumexp, one coalesced pass with all loads in flight
// together (a global load per score inside the element loop serialises on its latency).  +inf marks a row whose every key
// carries the hard finfo.min mask: its logsumexp IS finfo.min -- log T is absorbed -- and its probabilities are uniform, as in
// the general kernel.
__device__ __forceinline__ void score_offsets(float* DS, int TP, int T, const AttnK& P, int g, int g2, int h, int r0, int rb, int tid) {
  const fcmf_attn_desc& a = P.a;
  const int64_t bias0 = (((int64_t)g2 * a.heads + h) * a.R + r0) * T;      // (the block's rows are contiguous in the bias tile)
  for (int idx = tid; idx < rb * T; idx += 256) {
    const int rl = idx / T, t = idx - rl * T;
    float add = a.mask ? a.mask[(int64_t)g * T + t] : 0.f;
    if (a.bias) add += a.bias[bias0 + idx];
    const float lse_r = P.lse[((int64_t)g * a.heads + h) * a.R + r0 + rl];
    DS[rl * TP + t] = lse_r <= -1e30f ? INFINITY : add - lse_r;
  }
}

// dropped probability and score gradient of (row r = block row rl, key t) from s = q.k and dpd = dO.v; DS holds the element's
// score offset on entry.  FLAT: no dbias; a private key's pair also goes to the pd2 / ds2 scratch of the grouped backward.
template <bool FLAT>
__device__ __forceinline__ void bwd_element(float* PD, float* DS, const float* dl, int TP, int T, const AttnK& P, int g, int h, int r, int rl,
                                            int t, float s, float dpd, float inv_keep) {
  const fcmf_attn_desc& a = P.a;
  const float off = DS[rl * TP + t];
  const float pr = off == INFINITY ? 1.0f / (float)T : __expf(s * a.scale + off);
  float mult = 1.0f;
  if (a.dropout_p > 0.f) mult = dropout_mult(a.seed, (((uint64_t)g * a.heads + h) * a.R + r) * T + t, a.dropout_p, inv_keep);
  const float dsv = pr * (dpd * mult - dl[r]);
  PD[rl * TP + t] = pr * mult;
  DS[rl * TP + t] = dsv;
  if (!FLAT && P.dbias) P.dbias[(((int64_t)g * a.heads + h) * a.R + r) * T + t] = dsv;
  if (FLAT && t >= a.T1 && P.pd2) {
    const int64_t i2 = (((int64_t)g * a.heads + h) * a.R + r) * a.T2 + (t - a.T1);
    P.pd2[i2] = pr * mult;
    P.ds2[i2] = dsv;
  }
}

// out[rl][c .. c+8) = mul * sum_t W[rl][t] * X[t][c .. c+8) for rb rows: thread = (row, 8 columns), one 16-byte read of X per key
// (the tiny forward's outputs from the probabilities and V; the tiny backwards' dQ rows from the score gradients and K)
__device__ __forceinline__ void row_sums8(const float* W, int TP, const bf16_t* X, int dp, int T, int rb, int d8, float mul, bf16_t* out,
                                          int64_t out_sr, int tid) {
  for (int idx = tid; idx < rb * d8; idx += 256) {
    const int rl = idx / d8, c = (idx - rl * d8) * 8;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int t = 0; t < T; ++t) {
      const float wv = W[rl * TP + t];
      const bf16x8 x = *reinterpret_cast<const bf16x8*>(X + t * dp + c);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += wv * (float)x[j];
    }
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (bf16_t)(acc[j] * mul);
    *reinterpret_cast<bf16x8*>(out + rl * out_sr + c) = o;
  }
}

// the same sums for few rows, shared and private keys: thread = (row, 8 columns, quarter of the keys), the four quarters in
// neighbouring lanes and summed across them.  X2 = the private rows of (g2, head h): row r, key t2 at X2 + r k2_sr + t2 k2_st.
__device__ __forceinline__ void row_sums8_quarters(const float* W, int TP, const bf16_t* X1, int dp, const bf16_t* X2, const fcmf_attn_desc& a,
                                                   float mul, bf16_t* out, int64_t out_sr, int tid) {
  const int d8 = a.d >> 3;
  for (int item = tid >> 2; item < a.R * d8; item += 64) {
    const int r = item / d8, c = (item - r * d8) * 8, qt = tid & 3;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int t = qt; t < a.T1; t += 4) {
      const float wv = W[r * TP + t];
      const bf16x8 x = *reinterpret_cast<const bf16x8*>(X1 + t * dp + c);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += wv * (float)x[j];
    }
    for (int t2 = qt; t2 < a.T2; t2 += 4) {
      const float wv = W[r * TP + a.T1 + t2];
      const bf16x8 x = *reinterpret_cast<const bf16x8*>(X2 + (int64_t)r * a.k2_sr + c + (int64_t)t2 * a.k2_st);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += wv * (float)x[j];
    }
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float v = acc[j];
      v += __shfl_xor(v, 1, 64);
      v += __shfl_xor(v, 2, 64);
      o[j] = (bf16_t)(v * mul);
    }
    if (qt == 0) *reinterpret_cast<bf16x8*>(out + r * out_sr + c) = o;
  }
}

// dK / dV of (key t, columns c .. c+8): k += sum_rl DS[rl][t] Q[rl][c ..], v += sum_rl PD[rl][t] dO[rl][c ..] over rb rows (Qs / dOs
// = the first of them), and the store of the finished sums at element `off` of the dense [G, T1, heads*d] gradients
__device__ __forceinline__ void dkv_accumulate(float (&k)[8], float (&v)[8], const float* DS, const float* PD, int TP, const bf16_t* Qs,
                                               const bf16_t* dOs, int dp, int t, int c, int rb) {
  for (int rl = 0; rl < rb; ++rl) {
    const float dsv = DS[rl * TP + t], pv = PD[rl * TP + t];
    const bf16x8 qq = *reinterpret_cast<const bf16x8*>(Qs + rl * dp + c), gg = *reinterpret_cast<const bf16x8*>(dOs + rl * dp + c);
#pragma unroll
    for (int j = 0; j < 8; ++j) { k[j] += dsv * (float)qq[j]; v[j] += pv * (float)gg[j]; }
  }
}
__device__ __forceinline__ void dkv_store(const float (&k)[8], const float (&v)[8], const AttnK& P, int64_t off) {
  bf16x8 ok, ov;
#pragma unroll
  for (int j = 0; j < 8; ++j) { ok[j] = (bf16_t)(k[j] * P.a.scale); ov[j] = (bf16_t)v[j]; }
  *reinterpret_cast<bf16x8*>(reinterpret_cast<bf16_t*>(P.dk1) + off) = ok;
  *reinterpret_cast<bf16x8*>(reinterpret_cast<bf16_t*>(P.dv1) + off) = ov;
}
// ... for every shared key, all R rows at once: thread = (key, 8 columns)
__device__ __forceinline__ void dkv_keys(const float* DS, const float* PD, int TP, const bf16_t* Qs, const bf16_t* dOs, int dp, const AttnK& P,
                                         int g, int h, int tid) {
  const fcmf_attn_desc& a = P.a;
  const int d8 = a.d >> 3;
  for (int idx = tid; idx < a.T1 * d8; idx += 256) {
    const int t = idx / d8, c = (idx - t * d8) * 8;
    float k[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    dkv_accumulate(k, v, DS, PD, TP, Qs, dOs, dp, t, c, a.R);
    dkv_store(k, v, P, ((int64_t)g * a.T1 + t) * a.heads * a.d + h * a.d + c);
  }
}

// ---- the tiny kernels ------------------------------------------------------------------------------------------------------
template <bool WIDE>      // WIDE: 65..128 keys, two per lane in the softmax
__global__ __launch_bounds__(256) void attn_tiny_fwd_kernel(AttnK P) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const fcmf_attn_desc& a = P.a;
  const int d = a.d, T = a.T1, R = a.R, dp = d + 8, TP = T + 1;
  const AttnDenseLds L = attn_dense_lds(R, R, T, 0, d, false, true);
  bf16_t* img = reinterpret_cast<bf16_t*>(sm);
  bf16_t *Qs = img + L.q, *Ks = img + L.k, *Vs = img + L.v;
  float* Ss = sm + L.pd;                                  // [R][TP]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int g = blockIdx.x / a.heads, h = blockIdx.x % a.heads, g2 = g / a.group_div;
  stage_head(img, L, P, g, h, w, lane, false);
  // additive terms (bias tile + key mask) staged with the operands: one coalesced pass, all loads in flight together
  for (int idx = tid; idx < R * T; idx += 256) {
    const int r = idx / T, t = idx - r * T;
    float add = 0.f;
    if (a.mask) add = a.mask[(int64_t)g * T + t];
    if (a.bias) add += a.bias[(((int64_t)g2 * a.heads + h) * R) * T + idx];
    Ss[r * TP + t] = add;
  }
  __syncthreads();
  if ((d & 31) == 0) {                                   // scores on the matrix cores: wave = 16 x 16 fragments w, w + 4, ...
    const int nfc = (T + 15) >> 4, nf = ((R + 15) >> 4) * nfc;
    for (int f = w; f < nf; f += 4) {
      const int r0 = (f / nfc) * 16, t0 = (f % nfc) * 16;
      const f32x4 acc = frag_xyT(Qs, Ks, dp, d, r0, t0, lane);
      const int t = t0 + (lane & 15);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = r0 + 4 * (lane >> 4) + i;
        if (r < R && t < T) Ss[r * TP + t] += acc[i] * a.scale;
      }
    }
  } else {
    for (int idx = tid; idx < R * T; idx += 256) {
      const int r = idx / T, t = idx - r * T;
      Ss[r * TP + t] += dot_bf16(Qs + r * dp, Ks + t * dp, d) * a.scale;
    }
  }
  __syncthreads();
  const float inv_keep = a.dropout_p > 0.f ? 1.0f / (1.0f - a.dropout_p) : 1.0f;
  constexpr int KPL = WIDE ? 2 : 1;
  for (int r = w; r < R; r += 4) {
    float sc[KPL];
#pragma unroll
    for (int n = 0; n < KPL; ++n) sc[n] = lane + 64 * n < T ? Ss[r * TP + lane + 64 * n] : -INFINITY;
    softmax_dropout_row<KPL, true>(sc, T, lane, P, g, h, r, inv_keep, Ss + r * TP);
  }
  __syncthreads();
  row_sums8(Ss, TP, Vs, dp, T, R, d >> 3, 1.0f, reinterpret_cast<bf16_t*>(P.out) + (int64_t)g * a.o_sg + h * d, a.o_sr, tid);
}

// probabilities and score gradients of the rows [r0, r0 + rb) of a tiny backward: Q K^T and dO V^T on the matrix cores (see
// frag_xyT) when d % 32 == 0, else thread = (row, key) -- the thread that staged the element's offset
__device__ __forceinline__ void tiny_bwd_elements(float* PD, float* DS, const float* dl, int TP, const bf16_t* img, const AttnDenseLds& L,
                                                  const AttnK& P, int g, int h, int r0, int rb, float inv_keep, int tid) {
  const fcmf_attn_desc& a = P.a;
  const int d = a.d, T = a.T1, dp = d + 8, lane = tid & 63, w = tid >> 6;
  const bf16_t *Qs = img + L.q, *dOs = img + L.dout, *Ks = img + L.k, *Vs = img + L.v;
  if ((d & 31) == 0) {
    const int nfc = (T + 15) >> 4, nf = ((rb + 15) >> 4) * nfc;
    for (int f = w; f < nf; f += 4) {
      const int rl0 = (f / nfc) * 16, t0 = (f % nfc) * 16;
      const f32x4 sv = frag_xyT(Qs, Ks, dp, d, r0 + rl0, t0, lane), dv = frag_xyT(dOs, Vs, dp, d, r0 + rl0, t0, lane);
      const int t = t0 + (lane & 15);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int rl = rl0 + 4 * (lane >> 4) + i;
        if (rl < rb && t < T) bwd_element<false>(PD, DS, dl, TP, T, P, g, h, r0 + rl, rl, t, sv[i], dv[i], inv_keep);
      }
    }
  } else {
    for (int idx = tid; idx < rb * T; idx += 256) {
      const int rl = idx / T, t = idx - rl * T;
      bwd_element<false>(PD, DS, dl, TP, T, P, g, h, r0 + rl, rl, t, dot_bf16(Qs + (r0 + rl) * dp, Ks + t * dp, d),
                         dot_bf16(dOs + (r0 + rl) * dp, Vs + t * dp, d), inv_keep);
    }
  }
}

__global__ __launch_bounds__(256) void attn_tiny_bwd_kernel(AttnK P) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const fcmf_attn_desc& a = P.a;
  const int d = a.d, T = a.T1, R = a.R, dp = d + 8, TP = T + 1;
  const AttnDenseLds L = attn_dense_lds(R, R, T, 0, d, true, true);
  bf16_t* img = reinterpret_cast<bf16_t*>(sm);
  float *PD = sm + L.pd, *DS = sm + L.ds, *dl = sm + L.delta;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int g = blockIdx.x / a.heads, h = blockIdx.x % a.heads, g2 = g / a.group_div;
  stage_head(img, L, P, g, h, w, lane, true);
  score_offsets(DS, TP, T, P, g, g2, h, 0, R, tid);
  delta_rows(dl, P, g, h, w, lane);
  __syncthreads();
  const float inv_keep = a.dropout_p > 0.f ? 1.0f / (1.0f - a.dropout_p) : 1.0f;
  tiny_bwd_elements(PD, DS, dl, TP, img, L, P, g, h, 0, R, inv_keep, tid);
  __syncthreads();
  row_sums8(DS, TP, img + L.k, dp, T, R, d >> 3, a.scale, reinterpret_cast<bf16_t*>(P.dq) + (int64_t)g * R * a.heads * d + h * d,
            (int64_t)a.heads * d, tid);
  dkv_keys(DS, PD, TP, img + L.q, img + L.dout, dp, P, g, h, tid);
}

// The same backward for geometries whose two [R][T] f32 arrays no longer fit beside the operands (FCMF-large's ROI box
// attention: 100 x 100, heads of 128 -> 190 KB): the query rows go through the score / dQ phases in blocks of RBK rows, and
// each thread keeps its (key, 8 columns) dK / dV sums in registers across the blocks (NI = 8 items of 16 floats: T * d / 8
// <= 2048 items over 256 threads).  Rows in ascending order inside and across blocks: the sums are the ones the
// one-block kernel forms.
__global__ __launch_bounds__(256) void attn_tiny_bwd_blocked_kernel(AttnK P) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  constexpr int NI = 8;
  const fcmf_attn_desc& a = P.a;
  const int d = a.d, T = a.T1, R = a.R, dp = d + 8, TP = T + 1, RBK = P.RB;
  const AttnDenseLds L = attn_dense_lds(R, RBK, T, 0, d, true, true);
  bf16_t* img = reinterpret_cast<bf16_t*>(sm);
  float *PD = sm + L.pd, *DS = sm + L.ds, *dl = sm + L.delta;   // PD / DS: [RBK][TP], of the current row block
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int g = blockIdx.x / a.heads, h = blockIdx.x % a.heads, g2 = g / a.group_div;
  const int64_t HD = (int64_t)a.heads * d;
  stage_head(img, L, P, g, h, w, lane, true);
  delta_rows(dl, P, g, h, w, lane);
  const float inv_keep = a.dropout_p > 0.f ? 1.0f / (1.0f - a.dropout_p) : 1.0f;
  const int d8 = d >> 3, nkv = T * d8;
  float kacc[NI][8], vacc[NI][8];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) { kacc[i][j] = 0.f; vacc[i][j] = 0.f; }
  for (int r0 = 0; r0 < R; r0 += RBK) {
    const int rb = R - r0 < RBK ? R - r0 : RBK;
    __syncthreads();                                     // operands + delta staged / the previous block's arrays read
    score_offsets(DS, TP, T, P, g, g2, h, r0, rb, tid);
    if ((d & 31) == 0) __syncthreads();                  // (the fragments' elements were staged by other threads)
    tiny_bwd_elements(PD, DS, dl, TP, img, L, P, g, h, r0, rb, inv_keep, tid);
    __syncthreads();
    row_sums8(DS, TP, img + L.k, dp, T, rb, d8, a.scale, reinterpret_cast<bf16_t*>(P.dq) + ((int64_t)g * R + r0) * HD + h * d, HD, tid);
#pragma unroll
    for (int i = 0; i < NI; ++i) {                       // dK / dV partial sums: thread = (key, 8 columns), in registers
      const int idx = tid + 256 * i;
      if (idx < nkv) dkv_accumulate(kacc[i], vacc[i], DS, PD, TP, img + L.q + r0 * dp, img + L.dout + r0 * dp, dp, idx / d8, (idx % d8) * 8, rb);
    }
  }
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int idx = tid + 256 * i;
    if (idx < nkv) dkv_store(kacc[i], vacc[i], P, ((int64_t)g * T + idx / d8) * HD + h * d + (idx % d8) * 8);
  }
}

// ---- the rows_flat kernels ---------------------------------------------------------------------------------------------------
// Nothing in the backward needs a reduction -- the probabilities come from the saved logsumexp -- so the work is flat.  (The
// general kernel gives a wave a row -- 7 rows on 4 waves: two rounds, the second three quarters full -- and then a shared key: 32
// keys per wave one after the other, 7-long dependent sums, 128-byte stores.)
__global__ __launch_bounds__(256) void attn_rows_flat_bwd_kernel(AttnK P) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const fcmf_attn_desc& a = P.a;
  const int d = a.d, T1 = a.T1, T = T1 + a.T2, R = a.R, dp = d + 8, TP = T + 1;
  const AttnDenseLds L = attn_dense_lds(R, R, T1, a.T2, d, true, false);
  bf16_t* img = reinterpret_cast<bf16_t*>(sm);
  bf16_t *Qs = img + L.q, *dOs = img + L.dout, *Ks = img + L.k, *Vs = img + L.v;
  float *PD = sm + L.pd, *DS = sm + L.ds, *dl = sm + L.delta;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int g = blockIdx.x / a.heads, h = blockIdx.x % a.heads, g2 = g / a.group_div;
  const bf16_t* K2 = reinterpret_cast<const bf16_t*>(a.k2) + (int64_t)g2 * a.k2_sg + h * d;
  const bf16_t* V2 = reinterpret_cast<const bf16_t*>(a.v2) + (int64_t)g2 * a.k2_sg + h * d;
  stage_head(img, L, P, g, h, w, lane, true);
  score_offsets(DS, TP, T, P, g, g2, h, 0, R, tid);
  delta_rows(dl, P, g, h, w, lane);
  __syncthreads();
  const float inv_keep = a.dropout_p > 0.f ? 1.0f / (1.0f - a.dropout_p) : 1.0f;
  for (int idx = tid; idx < R * T; idx += 256) {         // thread = (row, key): the thread that staged the element's offset
    const int r = idx / T, t = idx - r * T;
    float s, dpd;
    if (t < T1) {
      s = dot_bf16(Qs + r * dp, Ks + t * dp, d);
      dpd = dot_bf16(dOs + r * dp, Vs + t * dp, d);
    } else {                                             // private key: its K2 / V2 rows straight from global memory
      const int64_t o2 = (int64_t)r * a.k2_sr + (int64_t)(t - T1) * a.k2_st;
      s = dot_bf16(Qs + r * dp, K2 + o2, d);
      dpd = dot_bf16(dOs + r * dp, V2 + o2, d);
    }
    bwd_element<true>(PD, DS, dl, TP, T, P, g, h, r, r, t, s, dpd, inv_keep);
  }
  __syncthreads();
  row_sums8_quarters(DS, TP, Ks, dp, K2, a, a.scale, reinterpret_cast<bf16_t*>(P.dq) + (int64_t)g * R * a.heads * d + h * d,
                     (int64_t)a.heads * d, tid);
  dkv_keys(DS, PD, TP, Qs, dOs, dp, P, g, h, tid);
}

// the forward of the same geometry: thread = (row, key) scores, wave = row softmax (T <= 384 keys: up to 6 per lane), thread =
// (row, 8 columns, quarter of the keys) outputs
__global__ __launch_bounds__(256) void attn_rows_flat_fwd_kernel(AttnK P) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const fcmf_attn_desc& a = P.a;
  const int d = a.d, T1 = a.T1, T = T1 + a.T2, R = a.R, dp = d + 8, TP = T + 1;
  const AttnDenseLds L = attn_dense_lds(R, R, T1, a.T2, d, false, false);
  bf16_t* img = reinterpret_cast<bf16_t*>(sm);
  bf16_t *Qs = img + L.q, *Ks = img + L.k, *Vs = img + L.v;
  float* Ss = sm + L.pd;                                  // [R][TP] scores, then dropped probabilities
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int g = blockIdx.x / a.heads, h = blockIdx.x % a.heads, g2 = g / a.group_div;
  const bf16_t* K2 = reinterpret_cast<const bf16_t*>(a.k2) + (int64_t)g2 * a.k2_sg + h * d;
  const bf16_t* V2 = reinterpret_cast<const bf16_t*>(a.v2) + (int64_t)g2 * a.k2_sg + h * d;
  stage_head(img, L, P, g, h, w, lane, false);
  __syncthreads();
  for (int idx = tid; idx < R * T; idx += 256) {         // thread = (row, key)
    const int r = idx / T, t = idx - r * T;
    float s;
    if (t < T1) s = dot_bf16(Qs + r * dp, Ks + t * dp, d);
    else s = dot_bf16(Qs + r * dp, K2 + (int64_t)r * a.k2_sr + (int64_t)(t - T1) * a.k2_st, d);
    s *= a.scale;
    if (a.mask) s += a.mask[(int64_t)g * T + t];
    Ss[r * TP + t] = s;
  }
  __syncthreads();
  const float inv_keep = a.dropout_p > 0.f ? 1.0f / (1.0f - a.dropout_p) : 1.0f;
  for (int r = w; r < R; r += 4) {
    float sc[6];
#pragma unroll
    for (int n = 0; n < 6; ++n) sc[n] = lane + 64 * n < T ? Ss[r * TP + lane + 64 * n] : -INFINITY;
    softmax_dropout_row<6, false>(sc, T, lane, P, g, h, r, inv_keep, Ss + r * TP);
  }
  __syncthreads();
  row_sums8_quarters(Ss, TP, Vs, dp, V2, a, 1.0f, reinterpret_cast<bf16_t*>(P.out) + (int64_t)g * a.o_sg + h * d, a.o_sr, tid);
}

// =========================================================================================================================
// Host: descriptor -> plan -> launch
// =========================================================================================================================
// Every kernel instantiation of this file, once: the enum, the name table and run_plan's switch are all made from this list.
// (attn_small_plan counts on the order inside the two general families: K4, K4_D64, K8, K8_D64 and plain, GROUPED, ONE, ONE_GROUPED.)
#define ATTN_SMALL_KERNELS(X)                                        \
  X(AK_FWD_F32_K4, attn_small_fwd_kernel<float, 4, 0>)               \
  X(AK_FWD_F32_K4_D64, attn_small_fwd_kernel<float, 4, 64>)          \
  X(AK_FWD_F32_K8, attn_small_fwd_kernel<float, 8, 0>)               \
  X(AK_FWD_F32_K8_D64, attn_small_fwd_kernel<float, 8, 64>)          \
  X(AK_FWD_BF16_K4, attn_small_fwd_kernel<bf16_t, 4, 0>)             \
  X(AK_FWD_BF16_K4_D64, attn_small_fwd_kernel<bf16_t, 4, 64>)        \
  X(AK_FWD_BF16_K8, attn_small_fwd_kernel<bf16_t, 8, 0>)             \
  X(AK_FWD_BF16_K8_D64, attn_small_fwd_kernel<bf16_t, 8, 64>)        \
  X(AK_TINY_FWD, attn_tiny_fwd_kernel<false>)                        \
  X(AK_TINY_FWD_WIDE, attn_tiny_fwd_kernel<true>)                    \
  X(AK_ROWS_FLAT_FWD, attn_rows_flat_fwd_kernel)                     \
  X(AK_BWD_F32, attn_small_bwd_kernel<float, false, false>)          \
  X(AK_BWD_F32_GROUPED, attn_small_bwd_kernel<float, false, true>)   \
  X(AK_BWD_F32_ONE, attn_small_bwd_kernel<float, true, false>)       \
  X(AK_BWD_F32_ONE_GROUPED, attn_small_bwd_kernel<float, true, true>) \
  X(AK_BWD_BF16, attn_small_bwd_kernel<bf16_t, false, false>)        \
  X(AK_BWD_BF16_GROUPED, attn_small_bwd_kernel<bf16_t, false, true>) \
  X(AK_BWD_BF16_ONE, attn_small_bwd_kernel<bf16_t, true, false>)     \
  X(AK_BWD_BF16_ONE_GROUPED, attn_small_bwd_kernel<bf16_t, true, true>) \
  X(AK_TINY_BWD, attn_tiny_bwd_kernel)                               \
  X(AK_TINY_BWD_BLOCKED, attn_tiny_bwd_blocked_kernel)               \
  X(AK_ROWS_FLAT_BWD, attn_rows_flat_bwd_kernel)                     \
  X(AK_PRIVATE_GRAD_F32, attn_private_grad_kernel<float>)            \
  X(AK_PRIVATE_GRAD_BF16, attn_private_grad_kernel<bf16_t>)
#define X(id, ...) id,
enum AttnSmallKernel { AK_NONE = -1, ATTN_SMALL_KERNELS(X) AK_COUNT };
#undef X
#define X(id, ...) #__VA_ARGS__,
static const char* const ATTN_SMALL_KERNEL_NAMES[AK_COUNT] = {ATTN_SMALL_KERNELS(X)};
#undef X

struct AttnSmallPlan {
  int rc;                      // FCMF_OK, or why nothing is launched
  bool desc_ok;                // the descriptor itself passed (rc then speaks of what this file supports)
  int kernel, grid_x, grid_y;  // AttnSmallKernel; 256 threads per workgroup throughout
  size_t smem;
  int RB, TLP, KVF;            // -> AttnK
  int kernel2, grid2_x, grid2_y;   // attn_private_grad_kernel behind a grouped backward, or AK_NONE
  size_t smem2;
};

static int check_desc(const fcmf_attn_desc* a) {
  if (!a || !a->q) return FCMF_ERR_ARG;
  if (a->dtype != FCMF_F32 && a->dtype != FCMF_BF16) return FCMF_ERR_UNSUPPORTED;
  if (a->G <= 0 || a->heads <= 0 || a->R <= 0 || a->d <= 0 || a->d > AS_MAXD) return FCMF_ERR_ARG;
  if (a->T1 < 0 || a->T2 < 0 || a->T1 + a->T2 <= 0 || a->T1 + a->T2 > AS_MAXT || a->T2 > 128) return FCMF_ERR_ARG;
  if (a->T1 > 0 && (!a->k1 || !a->v1)) return FCMF_ERR_ARG;
  if (a->T2 > 0 && (!a->k2 || !a->v2)) return FCMF_ERR_ARG;
  if (a->group_div <= 0) return FCMF_ERR_ARG;
  return FCMF_OK;
}

// what both dense families ask of the inputs: bf16, no causal fill, no head quirk, 16-byte rows
static bool dense_inputs_ok(const fcmf_attn_desc* a) {
  if (!(a->dtype == FCMF_BF16 && !a->causal && !a->head_quirk && a->d % 8 == 0 && a->q_sr % 8 == 0 && a->q_sg % 8 == 0 && a->o_sr % 8 == 0 &&
        a->o_sg % 8 == 0 && al16(a->q)))
    return false;
  if (a->T1 > 0 && !(a->k1_st % 8 == 0 && a->k1_sg % 8 == 0 && al16(a->k1) && al16(a->v1))) return false;
  if (a->T2 > 0 && !(a->k2_sg % 8 == 0 && a->k2_sr % 8 == 0 && a->k2_st % 8 == 0 && al16(a->k2) && al16(a->v2))) return false;
  return true;
}
static bool tiny_ok(const fcmf_attn_desc* a) {
  return dense_inputs_ok(a) && a->T2 == 0 && a->T1 > 0 && a->T1 <= TINY_WIDE_MAX && a->R <= TINY_WIDE_MAX;
}
static bool rows_flat_ok(const fcmf_attn_desc* a) { return dense_inputs_ok(a) && !a->bias && a->R <= 16 && a->T1 <= 128; }

// query rows per staged block of the general kernels: all R if the workgroup then stays within 80 KiB of LDS (two or more
// workgroups per CU); else blocks of >= 8 rows within 80 KiB if they fit; else as many rows as fit in 160 KiB
static int rows_per_block(int R, size_t base_bytes, size_t per_row_bytes) {
  const size_t soft = 80 * 1024, hard = 160 * 1024;
  if (base_bytes + (size_t)R * per_row_bytes <= soft) return R;
  if (base_bytes + 8 * per_row_bytes <= soft) return (int)((soft - base_bytes) / per_row_bytes);
  if (base_bytes + per_row_bytes > hard) return 0;
  const size_t rb = (hard - base_bytes) / per_row_bytes;
  return (int)(rb > (size_t)R ? R : rb);
}

// The plan: which kernel runs a descriptor, and with what grid and LDS.  Pure: no HIP call, and of the pointers only their
// presence and alignment.  io_al16 = the output / gradient pointers of the call (out; out, dout, dq, dk1, dv1) are 16-byte aligned.
static AttnSmallPlan attn_small_plan(const fcmf_attn_desc* a, bool backward, bool grouped, bool has_dbias, bool has_dv1, bool io_al16) {
  AttnSmallPlan p{};
  p.kernel = p.kernel2 = AK_NONE;
  p.rc = check_desc(a);
  if (p.rc) return p;
  p.desc_ok = true;
  p.rc = FCMF_ERR_UNSUPPORTED;
  const int R = a->R, T1 = a->T1, T2 = a->T2, d = a->d;
  const bool f32 = a->dtype == FCMF_F32;
  p.grid_x = a->G * a->heads; p.grid_y = 1;
  auto found = [&p](int kernel, size_t smem) { p.kernel = kernel; p.smem = smem; p.rc = FCMF_OK; return p; };
  if (backward && grouped) {
    // dk2 / dv2 summed over the group by attn_private_grad_kernel: 4 key ranges per (review, row), ~1800 workgroups on the step
    p.smem2 = sizeof(float) * 2 * (size_t)a->group_div * a->heads * T2;
    if (T2 <= 0 || a->group_div > 8 || a->G % a->group_div || a->head_quirk || p.smem2 > 150 * 1024) return p;
    p.kernel2 = f32 ? AK_PRIVATE_GRAD_F32 : AK_PRIVATE_GRAD_BF16;
    p.grid2_x = (a->G / a->group_div) * R; p.grid2_y = 4;
  }
  // the general kernels' LDS: the K and V images of the shared keys (of one 128-key chunk in the backward; rows of d + 16 bytes,
  // together rounded to 16 bytes, KVF floats), then per staged query row d floats (forward; + 4 waves' probability rows of
  // 64 KPL floats in all) or 2 d + 2 TLP floats (backward: Q, dO and the row's probabilities and score gradients)
  const size_t esz = f32 ? 4 : 2;
  const int nsh = backward && T1 > 128 ? 128 : T1;
  const int KVF = (int)((2 * (size_t)nsh * (d + 16 / esz) * esz + 15) / 16 * 4);
  if (!backward) {
    if (tiny_ok(a) && io_al16) {
      const AttnDenseLds L = attn_dense_lds(R, R, T1, 0, d, false, true);
      if (L.bytes <= TINY_LDS) return found(T1 > 64 ? AK_TINY_FWD_WIDE : AK_TINY_FWD, L.bytes);
    }
    if (rows_flat_ok(a) && T1 + T2 <= 384 && io_al16) {
      const AttnDenseLds L = attn_dense_lds(R, R, T1, T2, d, false, false);
      if (L.bytes <= FLAT_LDS) return found(AK_ROWS_FLAT_FWD, L.bytes);
    }
    const int kpl = T1 + T2 <= 256 ? 4 : 8;              // keys per lane
    const size_t base = sizeof(float) * ((size_t)KVF + 4 * 64 * kpl), per_row = sizeof(float) * (size_t)d;
    p.RB = rows_per_block(R, base, per_row);
    if (p.RB <= 0) return p;
    p.KVF = KVF;
    return found((f32 ? AK_FWD_F32_K4 : AK_FWD_BF16_K4) + (kpl == 8 ? 2 : 0) + (d == 64 ? 1 : 0), base + p.RB * per_row);
  }
  if (!grouped && has_dv1 && tiny_ok(a) && io_al16) {
    const AttnDenseLds L = attn_dense_lds(R, 0, T1, 0, d, true, true);      // without the [rows][T + 1] arrays
    if (R <= TINY_MAX && T1 <= TINY_MAX && L.bytes + R * L.row_bytes <= TINY_LDS) return found(AK_TINY_BWD, L.bytes + R * L.row_bytes);
    if (L.bytes + 16 * L.row_bytes <= TINY_LDS) {        // row blocks of >= 16 rows, as even as the LDS allows
      const int fit = (int)((TINY_LDS - L.bytes) / L.row_bytes), nblk = (R + fit - 1) / fit;
      p.RB = (R + nblk - 1) / nblk;
      return found(AK_TINY_BWD_BLOCKED, L.bytes + p.RB * L.row_bytes);
    }
  }
  if (rows_flat_ok(a) && !has_dbias && (T2 == 0 || grouped) && (T1 == 0 || has_dv1) && io_al16) {
    const AttnDenseLds L = attn_dense_lds(R, R, T1, T2, d, true, false);
    if (L.bytes <= FLAT_LDS) return found(AK_ROWS_FLAT_BWD, L.bytes);
  }
  p.TLP = (nsh + T2 + 3) & ~3;         // multiple of 4: rows of the key arrays stay 16-byte aligned
  const size_t base = sizeof(float) * (size_t)KVF, per_row = sizeof(float) * (2 * (size_t)d + 2 * (size_t)p.TLP);
  p.RB = rows_per_block(R, base, per_row);
  if (p.RB <= 0) return p;             // (cannot happen: <= 132 KiB of images + 3 KiB per row)
  p.KVF = KVF;
  p.grid_y = T1 > 0 ? (T1 + 127) / 128 : 1;
  return found((f32 ? AK_BWD_F32 : AK_BWD_BF16) + (p.RB >= R ? 2 : 0) + (grouped ? 1 : 0), base + p.RB * per_row);
}

// The only place that names kernel instantiations.  The rows_flat kernels stay below the 64 KiB every kernel may take
// and are launched as they are; every other launch first raises its kernel's dynamic-LDS limit (fcmf_launch).
static int launch_kernel(int kernel, dim3 grid, size_t smem, hipStream_t st, const AttnK& P) {
  bool attr_set = kernel == AK_ROWS_FLAT_FWD || kernel == AK_ROWS_FLAT_BWD;
  switch (kernel) {
#define X(id, ...) case id: return fcmf_launch_flagged(&attr_set, __VA_ARGS__, grid, dim3(256), smem, st, P);
    ATTN_SMALL_KERNELS(X)
#undef X
  }
  return FCMF_ERR_ARG;
}
static int run_plan(const AttnSmallPlan& pl, AttnK& P, void* stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  P.RB = pl.RB; P.TLP = pl.TLP; P.KVF = pl.KVF;
  const int rc = launch_kernel(pl.kernel, dim3(pl.grid_x, pl.grid_y), pl.smem, st, P);
  if (rc != FCMF_OK || pl.kernel2 == AK_NONE) return rc;
  return launch_kernel(pl.kernel2, dim3(pl.grid2_x, pl.grid2_y), pl.smem2, st, P);
}

extern "C" int fcmf_attn_small_plan(const fcmf_attn_desc* desc, int backward, int grouped, int has_dbias, int has_dv1, int ptrs_aligned,
                                    int32_t* info, const char** kernels) {
  if (!info) return FCMF_ERR_ARG;
  const AttnSmallPlan pl = attn_small_plan(desc, backward != 0, grouped != 0, has_dbias != 0, has_dv1 != 0, ptrs_aligned != 0);
  const bool ok = pl.rc == FCMF_OK;
  const int32_t v[11] = {pl.kernel, pl.grid_x, pl.grid_y, (int32_t)pl.smem, pl.RB, pl.TLP, pl.KVF,
                         ok ? pl.kernel2 : AK_NONE, pl.grid2_x, pl.grid2_y, (int32_t)pl.smem2};
  for (int i = 0; i < 11; ++i) info[i] = ok || i == 0 || i == 7 ? v[i] : 0;
  if (kernels) {
    kernels[0] = ok ? ATTN_SMALL_KERNEL_NAMES[pl.kernel] : nullptr;
    kernels[1] = ok && pl.kernel2 != AK_NONE ? ATTN_SMALL_KERNEL_NAMES[pl.kernel2] : nullptr;
  }
  return pl.rc;
}

extern "C" int fcmf_attn_small_fwd(const fcmf_attn_desc* desc, void* out, float* lse, void* stream) {
  const AttnSmallPlan pl = attn_small_plan(desc, false, false, false, false, al16(out));
  if (!pl.desc_ok) return pl.rc;
  if (!out) return FCMF_ERR_ARG;
  if (pl.rc) return pl.rc;
  AttnK P{};
  P.a = *desc; P.out = out; P.lse = lse;
  return run_plan(pl, P, stream);
}

static int attn_small_bwd_impl(const fcmf_attn_desc* desc, const void* out, const void* dout, const float* lse,
                               void* dq, void* dk1, void* dv1, void* dk2, void* dv2, float* dbias,
                               float* scratch, int64_t scratch_bytes, void* stream) {
  const bool grouped = scratch != nullptr;
  const AttnSmallPlan pl = attn_small_plan(desc, true, grouped, dbias != nullptr, dv1 != nullptr,
                                           al16(out) && al16(dout) && al16(dq) && al16(dk1) && al16(dv1));
  if (!pl.desc_ok) return pl.rc;
  if (!out || !dout || !lse || !dq) return FCMF_ERR_ARG;
  if (desc->T1 > 0 && !dk1) return FCMF_ERR_ARG;
  if (desc->T1 > 0 && !dv1 && desc->v1 != desc->k1) return FCMF_ERR_ARG;
  if (desc->T2 > 0 && (!dk2 || !dv2)) return FCMF_ERR_ARG;
  if (pl.rc) return pl.rc;
  AttnK P{};
  P.a = *desc; P.o_in = out; P.dout = dout; P.lse = const_cast<float*>(lse);
  P.dq = dq; P.dk1 = dk1; P.dv1 = dv1; P.dk2 = dk2; P.dv2 = dv2; P.dbias = dbias;
  if (grouped) {
    const int64_t n2 = (int64_t)desc->G * desc->heads * desc->R * desc->T2;
    if (scratch_bytes < 2 * n2 * (int64_t)sizeof(float)) return FCMF_ERR_ARG;
    P.pd2 = scratch; P.ds2 = scratch + n2;
  }
  return run_plan(pl, P, stream);
}

extern "C" int fcmf_attn_small_bwd(const fcmf_attn_desc* desc, const void* out, const void* dout, const float* lse,
                                   void* dq, void* dk1, void* dv1, void* dk2, void* dv2, float* dbias,
                                   void* stream) {
  return attn_small_bwd_impl(desc, out, dout, lse, dq, dk1, dv1, dk2, dv2, dbias, nullptr, 0, stream);
}

extern "C" int fcmf_attn_small_bwd_grouped(const fcmf_attn_desc* desc, const void* out, const void* dout, const float* lse,
                                           void* dq, void* dk1, void* dv1, void* dk2, void* dv2, float* dbias,
                                           float* scratch, int64_t scratch_bytes, void* stream) {
  if (!scratch) return FCMF_ERR_ARG;
  return attn_small_bwd_impl(desc, out, dout, lse, dq, dk1, dv1, dk2, dv2, dbias, scratch, scratch_bytes, stream);
}
