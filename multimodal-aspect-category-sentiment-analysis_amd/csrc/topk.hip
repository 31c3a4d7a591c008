// log-softmax + top-k of the rows of a logits matrix in one pass (see include/fcmf_hip.h): the tail of an IAOG decode step, the
// k best next tokens of every (sample, last token) row and their log-probabilities, without a [rows, V] log-softmax round trip.
// One 256-thread workgroup per row.  A thread walks its columns once and keeps
//   * a running (max, sum of exp(x - max)) -- the online softmax denominator, rescaled once per 16-byte chunk, and
//   * its own K best (value, column) pairs, sorted, in registers: K is a template parameter and every index into the list is a
//     compile-time constant after unrolling (a runtime-indexed list would live in scratch; the Makefile fails the build when a
//     kernel of this file needs any).
// The order is total: the larger stored value first, the lower column first among equal values -- what a stable descending sort
// of the row gives.  Selection compares stored values only, so it carries no rounding; lse enters the k results at the very end.
// Merges: over the wave by an xor butterfly (both lanes of a pair form the same merged list: bitonic merge of two sorted lists,
// best(A[j], B[K-1-j]) then log2 K compare-exchange stages), over the four waves through LDS by wave 0.  Fixed order, no atomics:
// two launches give the same bits.  Columns at or beyond V are never loaded.
#include <limits.h>

#include "common.h"

struct TopkK {
  const void* x;
  int64_t ld;
  int V, k, vec;      // vec: rows are 16-byte aligned -> 16-byte loads, else one element per load
  float* logp;
  int* ids;
};

template <int K>
struct TopList {
  float v[K];
  int i[K];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int j = 0; j < K; ++j) { v[j] = -INFINITY; i[j] = INT_MAX; }      // (a real -inf entry has a column < INT_MAX: it beats an empty slot)
  }
};

__device__ __forceinline__ bool tk_better(float av, int ai, float bv, int bi) { return (av > bv) | ((av == bv) & (ai < bi)); }

// (v[a], i[a]) <- the better of the two, (v[b], i[b]) <- the other; a < b are compile-time constants at every call
template <int K>
__device__ __forceinline__ void tk_cmpx(TopList<K>& L, int a, int b) {
  const bool sw = tk_better(L.v[b], L.i[b], L.v[a], L.i[a]);
  const float hv = sw ? L.v[b] : L.v[a], lv = sw ? L.v[a] : L.v[b];
  const int hi = sw ? L.i[b] : L.i[a], li = sw ? L.i[a] : L.i[b];
  L.v[a] = hv; L.i[a] = hi; L.v[b] = lv; L.i[b] = li;
}

template <int K>
__device__ __forceinline__ void tk_insert(TopList<K>& L, float x, int col) {
  if (tk_better(x, col, L.v[K - 1], L.i[K - 1])) {
    L.v[K - 1] = x; L.i[K - 1] = col;
#pragma unroll
    for (int j = K - 1; j > 0; --j) tk_cmpx<K>(L, j - 1, j);
  }
}

// L <- the K best of L and the sorted list (bv, bi)
template <int K>
__device__ __forceinline__ void tk_merge(TopList<K>& L, const float (&bv)[K], const int (&bi)[K]) {
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const bool sw = tk_better(bv[K - 1 - j], bi[K - 1 - j], L.v[j], L.i[j]);
    L.v[j] = sw ? bv[K - 1 - j] : L.v[j];
    L.i[j] = sw ? bi[K - 1 - j] : L.i[j];
  }
#pragma unroll
  for (int s = K / 2; s >= 1; s >>= 1) {
#pragma unroll
    for (int j = 0; j < K; ++j)
      if ((j & s) == 0) tk_cmpx<K>(L, j, j + s);
  }
}

// (m, s) <- (m, s) joined with (m2, s2): s counts exp(x - m)
__device__ __forceinline__ void tk_join(float& m, float& s, float m2, float s2) {
  const float M = fmaxf(m, m2);
  const float a = m == M ? 1.f : __expf(m - M), b = m2 == M ? 1.f : __expf(m2 - M);      // (-inf joined with -inf: no inf - inf)
  s = s * a + s2 * b;
  m = M;
}

template <int K, int N>
__device__ __forceinline__ void tk_consume(TopList<K>& L, float& m, float& s, const float (&x)[N], int col0) {
  float cm = x[0];
#pragma unroll
  for (int e = 1; e < N; ++e) cm = fmaxf(cm, x[e]);
  if (cm > m) {
    s *= __expf(m - cm);      // (m = -inf: s is 0 and stays 0)
    m = cm;
  }
  if (m != -INFINITY) {
#pragma unroll
    for (int e = 0; e < N; ++e) s += __expf(x[e] - m);
  }
#pragma unroll
  for (int e = 0; e < N; ++e) tk_insert<K>(L, x[e], col0 + e);
}

// grid = rows, 256 threads
template <typename TT, int K>
__global__ __launch_bounds__(256) void logsoftmax_topk_kernel(TopkK P) {
  constexpr int VEC = 16 / sizeof(TT);
  __shared__ float wv[4][K], wm[4], ws[4];
  __shared__ int wi[4][K];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int V = P.V;
  const TT* row = reinterpret_cast<const TT*>(P.x) + (int64_t)blockIdx.x * P.ld;
  TopList<K> L;
  L.clear();
  float m = -INFINITY, s = 0.f;

  if (P.vec) {
    const int nfull = V / VEC;      // whole 16-byte chunks inside the row; the < VEC columns after them go one by one
    for (int c = tid; c < nfull; c += 256) {
      float x[VEC];
      if constexpr (sizeof(TT) == 2) {
        const bf16x8 r = *reinterpret_cast<const bf16x8*>(row + c * VEC);
#pragma unroll
        for (int e = 0; e < VEC; ++e) x[e] = (float)r[e];
      } else {
        const float4 r = *reinterpret_cast<const float4*>(row + c * VEC);
        x[0] = r.x; x[1] = r.y; x[2] = r.z; x[3] = r.w;
      }
      tk_consume<K, VEC>(L, m, s, x, c * VEC);
    }
    const int col = nfull * VEC + tid;
    if (col < V) {
      const float x[1] = {to_f32<TT>(row[col])};
      tk_consume<K, 1>(L, m, s, x, col);
    }
  } else {
    for (int col = tid; col < V; col += 256) {
      const float x[1] = {to_f32<TT>(row[col])};
      tk_consume<K, 1>(L, m, s, x, col);
    }
  }

  // ---- the wave: xor butterfly, every lane ends with the wave's list and (m, s)
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    float bv[K];
    int bi[K];
#pragma unroll
    for (int j = 0; j < K; ++j) { bv[j] = __shfl_xor(L.v[j], o, 64); bi[j] = __shfl_xor(L.i[j], o, 64); }
    tk_merge<K>(L, bv, bi);
    tk_join(m, s, __shfl_xor(m, o, 64), __shfl_xor(s, o, 64));
  }
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < K; ++j) { wv[w][j] = L.v[j]; wi[w][j] = L.i[j]; }
    wm[w] = m; ws[w] = s;
  }
  __syncthreads();
  if (w != 0) return;

  // ---- the four waves (wave 0, every lane the same work on the same LDS words)
#pragma unroll
  for (int u = 1; u < 4; ++u) {
    float bv[K];
    int bi[K];
#pragma unroll
    for (int j = 0; j < K; ++j) { bv[j] = wv[u][j]; bi[j] = wi[u][j]; }
    tk_merge<K>(L, bv, bi);
    tk_join(m, s, wm[u], ws[u]);
  }
  if (lane != 0) return;
  // log p = x - lse with lse = m + log s, formed as (x - m) - log s: x - m is exact for the values near the maximum
  const float ls = logf(s);
  float* lo = P.logp + (int64_t)blockIdx.x * P.k;
  int* io = P.ids + (int64_t)blockIdx.x * P.k;
#pragma unroll
  for (int j = 0; j < K; ++j)
    if (j < P.k) { lo[j] = (L.v[j] - m) - ls; io[j] = L.i[j]; }
}

template <typename TT>
static int topk_launch(const TopkK& P, int rows, hipStream_t st) {
  const dim3 g(rows), b(256);
  if (P.k <= 1) return fcmf_launch(logsoftmax_topk_kernel<TT, 1>, g, b, 0, st, P);
  if (P.k <= 2) return fcmf_launch(logsoftmax_topk_kernel<TT, 2>, g, b, 0, st, P);
  if (P.k <= 4) return fcmf_launch(logsoftmax_topk_kernel<TT, 4>, g, b, 0, st, P);
  if (P.k <= 8) return fcmf_launch(logsoftmax_topk_kernel<TT, 8>, g, b, 0, st, P);
  return fcmf_launch(logsoftmax_topk_kernel<TT, 16>, g, b, 0, st, P);
}

extern "C" int fcmf_logsoftmax_topk(const void* logits, int64_t ld, int rows, int V, int k, float* logp, int32_t* ids, int dtype,
                                    void* stream) {
  if (!logits || !logp || !ids || rows < 0) return FCMF_ERR_ARG;
  if (dtype != FCMF_F32 && dtype != FCMF_BF16) return FCMF_ERR_UNSUPPORTED;
  if (V < 1 || k < 1 || k > 16 || k > V) return FCMF_ERR_UNSUPPORTED;
  if (ld < V) return FCMF_ERR_ARG;
  if (rows == 0) return FCMF_OK;
  const int64_t esz = dtype == FCMF_F32 ? 4 : 2;
  TopkK P{};
  P.x = logits; P.ld = ld; P.V = V; P.k = k; P.logp = logp; P.ids = ids;
  P.vec = (reinterpret_cast<uintptr_t>(logits) & 15) == 0 && (ld * esz) % 16 == 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  return dtype == FCMF_F32 ? topk_launch<float>(P, rows, st) : topk_launch<bf16_t>(P, rows, st);
}
