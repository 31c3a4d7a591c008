// Attention probabilities on request: P = softmax(score) as float32, before dropout, recomputed from Q and K with the score
// definition of fcmf_attn_desc (include/fcmf_hip.h).  The forward kernels never materialise P; these two do, for the callers that
// hand probabilities out (RobertaModel(output_attentions=True), the IAOG decoder's Attention.attention_weights).  Both find the row
// maximum and sum themselves -- no logsumexp from a forward is needed -- and both are bound by their writes (G*heads*R*T*4 bytes
// out against the Q / K rows in), so neither stages more than it must:
//   attn_probs_kernel     : VALU, f32 / bf16, every descriptor feature (two key segments, group_div, mask, bias, causal, head_quirk,
//                           arbitrary row strides, query row stride 0).  One wave per query row, one key per lane and 64-key step:
//                           the lane walks its key's row in global memory against the query row broadcast from LDS; the store of a
//                           step is 256 contiguous bytes of the row.
//   attn_probs_mfma_kernel: bf16, head dim 64, Tq, Tk <= 256 (the text-encoder layers).  One workgroup per (sequence, head, 128-query
//                           tile); K staged once in LDS, S^T = K Q^T on v_mfma_f32_16x16x32_bf16 -- the orientation of the forward
//                           (attn_mfma.hip): the accumulator registers of a lane then hold FOUR CONSECUTIVE KEYS of one query, so the
//                           row maximum / sum are in-lane plus two shuffles and every lane stores 16 contiguous bytes along the key axis.
// Output element (g, slot h, r, t) at probs + g*p_sg + h*p_sh + r*T + t: [G, heads, R, T] (p_sg = heads*R*T, p_sh = R*T) or the decoder's
// slot-major [heads*G, R, T] (p_sg = R*T, p_sh = G*R*T: index h*G + g, the order of the reference's torch.split(output, mb_size, dim=0)).
#include "attn_tiles.h"

constexpr int AP_MAXT = 512;   // T1 + T2 (limits of fcmf_attn_small_bwd)
constexpr int AP_MAXD = 128;
constexpr int AP_KPL = AP_MAXT / 64;   // 64-key steps of a row

struct AttnProbsK {
  fcmf_attn_desc a;
  float* probs;
  int64_t p_sg, p_sh;
  int vec1, vec2;      // the rows of the shared / private key segment can be read 16 bytes at a time
};

// <q, row>: q f32 in LDS (a broadcast), row in global memory in the activation dtype
template <typename TT>
__device__ __forceinline__ float probs_dot(const float* __restrict__ q, const TT* __restrict__ row, int d, bool vec) {
  float s = 0.f;
  constexpr int V = 16 / sizeof(TT);
  if (vec) {
    for (int c = 0; c < d; c += V) {
      if constexpr (sizeof(TT) == 2) {
        const bf16x8 x = *reinterpret_cast<const bf16x8*>(row + c);
#pragma unroll
        for (int j = 0; j < 8; ++j) s += q[c + j] * (float)x[j];
      } else {
        const float4 x = *reinterpret_cast<const float4*>(row + c);
        s += q[c] * x.x + q[c + 1] * x.y + q[c + 2] * x.z + q[c + 3] * x.w;
      }
    }
  } else {
    for (int c = 0; c < d; ++c) s += q[c] * to_f32<TT>(row[c]);
  }
  return s;
}

// grid = (G*heads, ceil(R / 4)); wave w of a workgroup owns query row 4*blockIdx.y + w
template <typename TT>
__global__ __launch_bounds__(256) void attn_probs_kernel(AttnProbsK P) {
  __shared__ float Qs[4][AP_MAXD];
  const fcmf_attn_desc& a = P.a;
  const int d = a.d, T1 = a.T1, T = a.T1 + a.T2;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int g = blockIdx.x / a.heads, h = blockIdx.x % a.heads;
  const int hin = a.head_quirk ? (int)(((int64_t)h * a.G + g) % a.heads) : h;
  const int g2 = g / a.group_div;
  const int r = blockIdx.y * 4 + w;
  const bool live = r < a.R;
  if (live) {
    const TT* qrow = reinterpret_cast<const TT*>(a.q) + (int64_t)g * a.q_sg + (int64_t)r * a.q_sr + hin * d;
    for (int c = lane; c < d; c += 64) Qs[w][c] = to_f32<TT>(qrow[c]);
  }
  __syncthreads();
  if (!live) return;
  const float* q = Qs[w];
  const TT* k1 = reinterpret_cast<const TT*>(a.k1) + (int64_t)g * a.k1_sg + hin * d;
  const TT* k2 = reinterpret_cast<const TT*>(a.k2) + (int64_t)g2 * a.k2_sg + (int64_t)r * a.k2_sr + hin * d;
  const float* mrow = a.mask ? a.mask + (int64_t)g * T : nullptr;
  const float* brow = a.bias ? a.bias + (((int64_t)g2 * a.heads + h) * a.R + r) * T : nullptr;
  float sc[AP_KPL];
  float m = -INFINITY;
#pragma unroll
  for (int n = 0; n < AP_KPL; ++n) {
    const int t = lane + 64 * n;
    float s = -INFINITY;
    if (t < T) {
      s = (t < T1 ? probs_dot<TT>(q, k1 + (int64_t)t * a.k1_st, d, P.vec1) : probs_dot<TT>(q, k2 + (int64_t)(t - T1) * a.k2_st, d, P.vec2)) * a.scale;
      if (mrow) s += mrow[t];
      if (brow) s += brow[t];
      if (a.causal && t > r) s = -1e4f;
    }
    sc[n] = s;
    m = fmaxf(m, s);
  }
  m = wave_max(m);
  float sum = 0.f;
#pragma unroll
  for (int n = 0; n < AP_KPL; ++n) {
    const float e = lane + 64 * n < T ? __expf(sc[n] - m) : 0.f;     // (a fully finfo.min-masked row: every term is exp(0) -> uniform 1/T)
    sc[n] = e;
    sum += e;
  }
  sum = wave_sum(sum);
  const float inv = 1.0f / sum;
  float* prow = P.probs + (int64_t)g * P.p_sg + (int64_t)h * P.p_sh + (int64_t)r * T;
#pragma unroll
  for (int n = 0; n < AP_KPL; ++n) {
    const int t = lane + 64 * n;
    if (t < T) prow[t] = sc[n] * inv;
  }
}

extern "C" int fcmf_attn_probs(const fcmf_attn_desc* desc, float* probs, int64_t p_sg, int64_t p_sh, void* stream) {
  const fcmf_attn_desc* a = desc;
  if (!a || !a->q || !probs) return FCMF_ERR_ARG;
  if (a->dtype != FCMF_F32 && a->dtype != FCMF_BF16) return FCMF_ERR_UNSUPPORTED;
  if (a->G <= 0 || a->heads <= 0 || a->R <= 0 || a->d <= 0 || a->T1 < 0 || a->T2 < 0 || a->T1 + a->T2 <= 0 || a->group_div <= 0) return FCMF_ERR_ARG;
  if (a->T1 > 0 && !a->k1) return FCMF_ERR_ARG;
  if (a->T2 > 0 && !a->k2) return FCMF_ERR_ARG;
  if (a->T1 + a->T2 > AP_MAXT || a->T2 > 128 || a->d > AP_MAXD) return FCMF_ERR_UNSUPPORTED;
  AttnProbsK P{};
  P.a = *a; P.probs = probs; P.p_sg = p_sg; P.p_sh = p_sh;
  const int V = a->dtype == FCMF_F32 ? 4 : 8;
  P.vec1 = a->T1 > 0 && a->d % V == 0 && a->k1_sg % V == 0 && a->k1_st % V == 0 && al16(a->k1);
  P.vec2 = a->T2 > 0 && a->d % V == 0 && a->k2_sg % V == 0 && a->k2_sr % V == 0 && a->k2_st % V == 0 && al16(a->k2);
  const dim3 grid(a->G * a->heads, (a->R + 3) / 4);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  return a->dtype == FCMF_F32 ? fcmf_launch(attn_probs_kernel<float>, grid, dim3(256), 0, st, P)
                              : fcmf_launch(attn_probs_kernel<bf16_t>, grid, dim3(256), 0, st, P);
}

// =========================================================================================
// MFMA kernel
constexpr int PD = 64;     // head dim
constexpr int PT = 128;    // query rows per workgroup / key rows per LDS tile

// K image [keys][64 bf16], 128-byte rows: 16-byte chunk XOR ((row >> 1) & 7) -- conflict free for the ds_read_b128 operand read
// (row = lane & 15, chunk = 4 s + (lane >> 4)): the pattern tools/lds_conflicts.py checks for the GEMM's 64-deep k-tiles
__device__ __forceinline__ int probs_koff(int r, int c8) { return r * 128 + ((c8 ^ ((r >> 1) & 7)) << 4); }

struct AttnProbsMfmaK {
  const bf16_t *q, *k;
  const float* mask;
  float* probs;
  int G, heads, Tq, Tk;
  int64_t ldq, ldk, p_sg, p_sh;
  float scale;
  int vec;      // every 4-key group of a row is 16-byte aligned: one 16-byte store per accumulator
};

template <int NKT>     // 128-key tiles: 1 (Tk <= 128) or 2 (Tk <= 256)
__global__ __launch_bounds__(256, 2) void attn_probs_mfma_kernel(AttnProbsMfmaK P) {
  constexpr int NKF = 8 * NKT;       // 16-key fragments
  __shared__ __attribute__((aligned(16))) char Ks[NKT * PT * PD * 2];
  __shared__ float Ms[NKT * PT];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int g = blockIdx.x / P.heads, h = blockIdx.x % P.heads;
  const int q0 = blockIdx.y * PT + w * 32;
  // stage K (zero rows past Tk) and the additive key mask
  const bf16_t* kbase = P.k + (int64_t)g * P.Tk * P.ldk + h * PD;
#pragma unroll
  for (int i = 0; i < 4 * NKT; ++i) {
    const int c = tid + 256 * i, r = c >> 3, c8 = c & 7;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (r < P.Tk) v = *reinterpret_cast<const uint4*>(kbase + (int64_t)r * P.ldk + c8 * 8);
    *reinterpret_cast<uint4*>(Ks + probs_koff(r, c8)) = v;
  }
  if (tid < NKT * PT) Ms[tid] = (P.mask && tid < P.Tk) ? P.mask[(int64_t)g * P.Tk + tid] : 0.f;
  bf16x8 qf[2][2];
  load_q_frags(P.q, P.ldq, P.Tq, g, h, q0, lane, qf);
  __syncthreads();
  if (q0 >= P.Tq) return;      // (wave-uniform; after the only barrier)
  const int nkf = (P.Tk + 15) >> 4;      // key fragments that hold a key
  // S^T[key][query]: lane holds, for query q0 + 16 f + (lane & 15), keys 16 kf + 4 (lane >> 4) + r
  f32x4 sc[NKF][2];
#pragma unroll
  for (int kf = 0; kf < NKF; ++kf)
#pragma unroll
    for (int f = 0; f < 2; ++f) sc[kf][f] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int kf = 0; kf < NKF; ++kf) {
      if (kf >= nkf) continue;
      const bf16x8 ka = *reinterpret_cast<const bf16x8*>(Ks + probs_koff(16 * kf + (lane & 15), 4 * s + (lane >> 4)));
#pragma unroll
      for (int f = 0; f < 2; ++f) sc[kf][f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ka, qf[f][s], sc[kf][f], 0, 0, 0);
    }
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    const int q = q0 + 16 * f + (lane & 15);
    float m = -INFINITY;
#pragma unroll
    for (int kf = 0; kf < NKF; ++kf) {
      if (kf >= nkf) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = 16 * kf + 4 * (lane >> 4) + r;
        const float s = key < P.Tk ? sc[kf][f][r] * P.scale + Ms[key] : -INFINITY;
        sc[kf][f][r] = s;
        m = fmaxf(m, s);
      }
    }
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    float sum = 0.f;
#pragma unroll
    for (int kf = 0; kf < NKF; ++kf) {
      if (kf >= nkf) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float e = __expf(sc[kf][f][r] - m);      // (keys past Tk: exp(-inf) = 0; a fully finfo.min-masked row: exp(0) everywhere)
        sc[kf][f][r] = e;
        sum += e;
      }
    }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    const float inv = 1.0f / sum;
    if (q < P.Tq) {
      float* prow = P.probs + (int64_t)g * P.p_sg + (int64_t)h * P.p_sh + (int64_t)q * P.Tk + 4 * (lane >> 4);
#pragma unroll
      for (int kf = 0; kf < NKF; ++kf) {
        if (kf >= nkf) continue;
        const int key = 16 * kf + 4 * (lane >> 4);
        if (P.vec) {      // Tk % 4 == 0: a group that starts inside the row ends inside it
          if (key < P.Tk) __builtin_nontemporal_store(sc[kf][f] * inv, reinterpret_cast<f32x4*>(prow + 16 * kf));
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (key + r < P.Tk) prow[16 * kf + r] = sc[kf][f][r] * inv;
        }
      }
    }
  }
}

extern "C" int fcmf_attn_mfma_probs(const void* q, const void* k, const float* mask, float* probs, int G, int heads, int Tq, int Tk,
                                    int64_t ldq, int64_t ldk, int64_t p_sg, int64_t p_sh, float scale, void* stream) {
  if (!q || !k || !probs || G <= 0 || heads <= 0 || Tq <= 0 || Tk <= 0) return FCMF_ERR_ARG;
  if (Tk > 2 * PT || Tq > 2 * PT || ldq % 8 || ldk % 8 || !al16(q) || !al16(k)) return FCMF_ERR_UNSUPPORTED;
  AttnProbsMfmaK P{};
  P.q = (const bf16_t*)q; P.k = (const bf16_t*)k; P.mask = mask; P.probs = probs;
  P.G = G; P.heads = heads; P.Tq = Tq; P.Tk = Tk; P.ldq = ldq; P.ldk = ldk; P.p_sg = p_sg; P.p_sh = p_sh; P.scale = scale;
  P.vec = Tk % 4 == 0 && p_sg % 4 == 0 && p_sh % 4 == 0 && al16(probs);
  const dim3 grid(G * heads, (Tq + PT - 1) / PT);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  return Tk > PT ? fcmf_launch(attn_probs_mfma_kernel<2>, grid, dim3(256), 0, st, P)
                 : fcmf_launch(attn_probs_mfma_kernel<1>, grid, dim3(256), 0, st, P);
}
