// BERTScore greedy matching (Zhang et al. 2020, idf = False, rescale_with_baseline = False), batched: one workgroup scores one
// (candidate, reference) pair from the two sentences' token embeddings,
//   s[i][j] = <c_i, r_j> / (|c_i| |r_j|)   P = sum_i wc[i] max_j s[i][j] / sum wc   R = sum_j wr[j] max_i s[i][j] / sum wr   F = 2PR / (P+R)
// over the valid rows only (see include/fcmf_hip.h).  Three phases, two barriers:
//   1. norms: a wave per row, 16 bytes per lane and step, f32 sum of squares, 1 / sqrt into LDS;
//   2. similarities, never stored: wave w owns the candidate rows of its row blocks and walks ALL reference columns, so a row
//      maximum is complete inside the wave; its column maxima go to the wave's OWN slice colpart[w][*], which no other wave touches.
//        bf16: 16 x 16 tiles of C R^T on v_mfma_f32_16x16x32_bf16, operands straight from global memory in operand layout (lane:
//              row lane & 15, 8 bf16 at k = 32 s + 8 (lane >> 4)) -- the STORED values, products exact in f32; the accumulator is
//              divided by the f32 norms afterwards.  A candidate fragment is fed to BS_JB column blocks per load.
//        f32 : VALU, the walk of attn_probs_kernel: one reference row per lane and 64-column step against the candidate row that
//              every lane reads at the same address (a broadcast);
//   3. wave 0: the weighted sums, lane-strided in a fixed order plus the xor butterfly of wave_sum.
// No atomics and a fixed wave -> row assignment: two launches on the same inputs give the same bits.  Rows at or beyond a pair's
// length are never loaded (their fragments are zeros, their similarities -inf), so they may hold anything, NaN included.
#include "common.h"

constexpr int BS_MAXL = 512;   // the encoder's position limit
constexpr int BS_JB = 2;       // reference column blocks per candidate fragment load

struct BertScoreK {
  const void *cand, *ref;
  const int *cand_len, *ref_len;
  const float *cand_w, *ref_w;
  float* out;
  int Lc_max, Lr_max, H;
  int64_t ldc, sc, ldr, sr;
};

// sum of squares of one row (H % 8 == 0, 16-byte aligned), the same value in every lane
template <typename TT>
__device__ __forceinline__ float bs_row_sumsq(const TT* __restrict__ row, int H, int lane) {
  float ss = 0.f;
  for (int c = lane * 8; c < H; c += 512) {
    if constexpr (sizeof(TT) == 2) {
      const bf16x8 x = *reinterpret_cast<const bf16x8*>(row + c);
#pragma unroll
      for (int j = 0; j < 8; ++j) { const float v = (float)x[j]; ss += v * v; }
    } else {
      const float4 a = *reinterpret_cast<const float4*>(row + c), b = *reinterpret_cast<const float4*>(row + c + 4);
      ss += a.x * a.x + a.y * a.y + a.z * a.z + a.w * a.w;
      ss += b.x * b.x + b.y * b.y + b.z * b.z + b.w * b.w;
    }
  }
  return wave_sum(ss);
}

// grid = N, 256 threads
template <typename TT>
__global__ __launch_bounds__(256) void bertscore_kernel(BertScoreK P) {
  __shared__ float icn[BS_MAXL], irn[BS_MAXL];      // 1 / |c_i|, 1 / |r_j| (0 for an all-zero row: its similarities are 0, not NaN)
  __shared__ float rowmax[BS_MAXL];                 // max_j s[i][j]
  __shared__ float colpart[4][BS_MAXL];             // wave w's max over ITS candidate rows of s[i][j]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t n = blockIdx.x;
  const int H = P.H;
  // the lengths live in device memory, so the host cannot have checked them: clamp
  const int Lc = min(max(P.cand_len[n], 0), P.Lc_max), Lr = min(max(P.ref_len[n], 0), P.Lr_max);
  float* o = P.out + 3 * n;
  if (Lc == 0 || Lr == 0) {      // (uniform over the workgroup, before any barrier)
    if (tid < 3) o[tid] = 0.f;
    return;
  }
  const TT* C = reinterpret_cast<const TT*>(P.cand) + n * P.sc;
  const TT* R = reinterpret_cast<const TT*>(P.ref) + n * P.sr;

  // ---- 1. norms
  for (int row = w; row < Lc + Lr; row += 4) {
    const bool isc = row < Lc;
    const float ss = bs_row_sumsq<TT>(isc ? C + (int64_t)row * P.ldc : R + (int64_t)(row - Lc) * P.ldr, H, lane);
    if (lane == 0) (isc ? icn[row] : irn[row - Lc]) = ss > 0.f ? 1.0f / sqrtf(ss) : 0.f;
  }
  for (int j = lane; j < Lr; j += 64) colpart[w][j] = -INFINITY;
  __syncthreads();

  // ---- 2. similarities -> row maxima, per-wave column maxima
  if constexpr (sizeof(TT) == 2) {
    const int nib = (Lc + 15) >> 4, njb = (Lr + 15) >> 4, nks = (H + 31) >> 5;
    const int fr = lane & 15, fq = lane >> 4;
    const bool kin = H % 32 == 0;      // every 8-wide chunk of every 32-deep step lies inside the row
    for (int ib = w; ib < nib; ib += 4) {
      const int ai = 16 * ib + fr;
      const bool av = ai < Lc;
      const bf16_t* arow = C + (int64_t)ai * P.ldc + 8 * fq;      // (dereferenced under `av` only)
      float rmax[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
      for (int jb0 = 0; jb0 < njb; jb0 += BS_JB) {
        f32x4 acc[BS_JB];
        const bf16_t* brow[BS_JB];
        bool bv[BS_JB];
#pragma unroll
        for (int t = 0; t < BS_JB; ++t) {
          const int bj = 16 * (jb0 + t) + fr;
          acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
          bv[t] = bj < Lr;
          brow[t] = R + (int64_t)bj * P.ldr + 8 * fq;
        }
        for (int s = 0; s < nks; ++s) {
          const int k = 32 * s;
          const bool kv = kin || k + 8 * fq < H;
          uint4 a = make_uint4(0, 0, 0, 0);
          if (av && kv) a = *reinterpret_cast<const uint4*>(arow + k);
#pragma unroll
          for (int t = 0; t < BS_JB; ++t) {
            uint4 b = make_uint4(0, 0, 0, 0);
            if (bv[t] && kv) b = *reinterpret_cast<const uint4*>(brow[t] + k);
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<bf16x8*>(&a), *reinterpret_cast<bf16x8*>(&b), acc[t], 0, 0, 0);
          }
        }
        // lane holds s[16 ib + 4 fq + r][16 (jb0 + t) + fr]
#pragma unroll
        for (int t = 0; t < BS_JB; ++t) {
          const int j = 16 * (jb0 + t) + fr;
          const bool jv = j < Lr;
          const float jn = jv ? irn[j] : 0.f;
          float cm = -INFINITY;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int i = 16 * ib + 4 * fq + r;
            const float s = (jv && i < Lc) ? acc[t][r] * icn[i] * jn : -INFINITY;
            rmax[r] = fmaxf(rmax[r], s);
            cm = fmaxf(cm, s);
          }
          cm = fmaxf(cm, __shfl_xor(cm, 16, 64));
          cm = fmaxf(cm, __shfl_xor(cm, 32, 64));
          if (fq == 0 && jv) colpart[w][j] = fmaxf(colpart[w][j], cm);
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float m = rmax[r];
        m = fmaxf(m, __shfl_xor(m, 1, 64));
        m = fmaxf(m, __shfl_xor(m, 2, 64));
        m = fmaxf(m, __shfl_xor(m, 4, 64));
        m = fmaxf(m, __shfl_xor(m, 8, 64));
        const int i = 16 * ib + 4 * fq + r;
        if (fr == 0 && i < Lc) rowmax[i] = m;
      }
    }
  } else {
    for (int i = w; i < Lc; i += 4) {
      const float* crow = C + (int64_t)i * P.ldc;
      const float ci = icn[i];
      float m = -INFINITY;
      for (int j = lane; j < Lr; j += 64) {
        const float* rrow = R + (int64_t)j * P.ldr;
        float d = 0.f;
        for (int c = 0; c < H; c += 4) {
          const float4 x = *reinterpret_cast<const float4*>(crow + c), y = *reinterpret_cast<const float4*>(rrow + c);
          d += x.x * y.x + x.y * y.y + x.z * y.z + x.w * y.w;
        }
        const float s = d * ci * irn[j];
        m = fmaxf(m, s);
        colpart[w][j] = fmaxf(colpart[w][j], s);
      }
      m = wave_max(m);
      if (lane == 0) rowmax[i] = m;
    }
  }
  __syncthreads();

  // ---- 3. weighted sums
  if (w != 0) return;
  const float* cw = P.cand_w ? P.cand_w + n * P.Lc_max : nullptr;
  const float* rw = P.ref_w ? P.ref_w + n * P.Lr_max : nullptr;
  float pn = 0.f, pd = 0.f, rn = 0.f, rd = 0.f;
  for (int i = lane; i < Lc; i += 64) {
    const float wt = cw ? cw[i] : 1.f;
    pn += wt * rowmax[i];
    pd += wt;
  }
  for (int j = lane; j < Lr; j += 64) {
    const float wt = rw ? rw[j] : 1.f;
    rn += wt * fmaxf(fmaxf(colpart[0][j], colpart[1][j]), fmaxf(colpart[2][j], colpart[3][j]));
    rd += wt;
  }
  pn = wave_sum(pn); pd = wave_sum(pd); rn = wave_sum(rn); rd = wave_sum(rd);
  if (lane == 0) {
    float p = 0.f, r = 0.f, f = 0.f;
    if (pd != 0.f && rd != 0.f) {
      p = pn / pd;
      r = rn / rd;
      f = p + r != 0.f ? 2.f * p * r / (p + r) : 0.f;
    }
    o[0] = p; o[1] = r; o[2] = f;
  }
}

extern "C" int fcmf_bertscore(const void* cand, const void* ref, const int* cand_len, const int* ref_len, const float* cand_w,
                              const float* ref_w, float* out, int N, int Lc_max, int Lr_max, int H, int64_t ldc, int64_t sc,
                              int64_t ldr, int64_t sr, int dtype, void* stream) {
  if (!cand || !ref || !cand_len || !ref_len || !out) return FCMF_ERR_ARG;
  if (N < 0 || Lc_max < 0 || Lr_max < 0 || H <= 0 || ldc < 0 || sc < 0 || ldr < 0 || sr < 0) return FCMF_ERR_ARG;
  if (dtype != FCMF_F32 && dtype != FCMF_BF16) return FCMF_ERR_UNSUPPORTED;
  if (Lc_max > BS_MAXL || Lr_max > BS_MAXL || H % 8) return FCMF_ERR_UNSUPPORTED;
  const int V = dtype == FCMF_F32 ? 4 : 8;      // elements of 16 bytes
  auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  if (ldc % V || sc % V || ldr % V || sr % V || !al16(cand) || !al16(ref)) return FCMF_ERR_UNSUPPORTED;
  if (N == 0) return FCMF_OK;
  BertScoreK P{};
  P.cand = cand; P.ref = ref; P.cand_len = cand_len; P.ref_len = ref_len; P.cand_w = cand_w; P.ref_w = ref_w; P.out = out;
  P.Lc_max = Lc_max; P.Lr_max = Lr_max; P.H = H; P.ldc = ldc; P.sc = sc; P.ldr = ldr; P.sr = sr;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  return dtype == FCMF_F32 ? fcmf_launch(bertscore_kernel<float>, dim3(N), dim3(256), 0, st, P)
                           : fcmf_launch(bertscore_kernel<bf16_t>, dim3(N), dim3(256), 0, st, P);
}
