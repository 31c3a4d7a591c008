// One sampled token per row of a logits matrix (see include/fcmf_hip.h, fcmf_sample_token): temperature, top-k and nucleus
// filtering and a Gumbel-max draw, the sampling tail of an IAOG decode step beside csrc/topk.hip's beam tail.  One 256-thread
// workgroup per row; the row (128 KB of bf16 at V = 64001) is read from L2 once per phase, 16 bytes per lane on aligned rows:
//   1. statistics: the row maximum m and s = sum exp(x - m) (online, per thread; joined in a fixed order) -- the lse of logp;
//   2. top-k threshold (0 < top_k < V): the top_k-th largest ORDER KEY of the row, an exact radix selection.  The key is the
//      order-preserving bit pattern of the stored value (16 bits for bf16, 32 for float; -0 counts as +0), so nothing is rounded
//      and ties at the threshold are all kept;
//   3. nucleus threshold (top_p < 1): the smallest key whose mass strictly above it is below top_p, a radix walk over the same
//      key space among the keys that passed 2.  A column's mass is exp((x - m) / T) as a 24.40 fixed-point INTEGER, so the
//      per-digit sums are integer LDS atomics: exact, independent of the order in which lanes arrive, no floating-point atomic.
//      The fixed point rounds each term by < 2^-40 of the largest one: the mass of a set is off by < 2^-20 * 2^-20 relative
//      to the total, far inside the float32 rounding of exp itself (1e-6);
//   4. the draw: argmax over the kept columns of x / T + Gumbel(hash(seed, ctr, column)), the lower column on an exact tie,
//      by an xor butterfly and then LDS across the four waves.
// Both radix walks are `radix_walk`: digits of 12 bits from the top (bf16: 12 + 4, float: 12 + 12 + 8), per digit one pass that
// adds every participating column's weight (1, or its mass) into a 4096-bin LDS histogram, a suffix scan (a thread owns 16
// adjacent bins) and the one bin where the running sum from the top crosses the target.  Phases 2 and 3 are skipped when off.
// Fixed order or integer sums everywhere: two launches give the same bits.  Columns at or beyond V are never loaded.
#include <limits.h>
#include <math.h>

#include "common.h"

struct SampleK {
  const void* x;
  int64_t ld;
  int V, top_k, vec;      // top_k: 0 = off; vec: rows are 16-byte aligned -> 16-byte loads, else one element per load
  float temperature, top_p;
  uint64_t seed;
  const int64_t* ctr;
  int* ids;
  float* logp;
};

typedef unsigned long long u64;
constexpr int SM_BINS = 4096, SM_PER_THREAD = SM_BINS / 256;

// f(x as float, column) for every column < V of the row, this thread's share: 16-byte chunks c = tid, tid + 256, ... four loads in
// flight, then the < VEC columns after the last whole chunk one by one
template <typename TT, typename F>
__device__ __forceinline__ void sm_for_each(const TT* row, int V, int vec, int tid, F&& f) {
  constexpr int VEC = 16 / sizeof(TT);
  typedef TT raw_t __attribute__((ext_vector_type(VEC)));
  if (vec) {
    const int nfull = V / VEC;
    int c = tid;
    for (; c + 3 * 256 < nfull; c += 4 * 256) {
      raw_t r[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) r[u] = *reinterpret_cast<const raw_t*>(row + (int64_t)(c + u * 256) * VEC);
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int e = 0; e < VEC; ++e) f((float)r[u][e], (c + u * 256) * VEC + e);
    }
    for (; c < nfull; c += 256) {
      const raw_t r = *reinterpret_cast<const raw_t*>(row + (int64_t)c * VEC);
#pragma unroll
      for (int e = 0; e < VEC; ++e) f((float)r[e], c * VEC + e);
    }
    const int col = nfull * VEC + tid;
    if (col < V) f(to_f32<TT>(row[col]), col);
  } else {
    for (int col = tid; col < V; col += 256) f(to_f32<TT>(row[col]), col);
  }
}

// the order key of a stored value in KB bits: a > b as values <=> key(a) > key(b); -0 and +0 share one key
template <int KB>
__device__ __forceinline__ uint32_t sm_key(float x) {
  const uint32_t b = __float_as_uint(x == 0.f ? 0.f : x);
  const uint32_t k = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return k >> (32 - KB);
}

// (m, s) <- (m, s) joined with (m2, s2): s counts exp(x - m)
__device__ __forceinline__ void sm_join(float& m, float& s, float m2, float s2) {
  const float M = fmaxf(m, m2);
  const float a = m == M ? 1.f : __expf(m - M), b = m2 == M ? 1.f : __expf(m2 - M);      // (-inf joined with -inf: no inf - inf)
  s = s * a + s2 * b;
  m = M;
}

// mass of a column as a 24.40 fixed-point integer: exp((x - m) / T) in (0, 1] -> 0 .. 2^40 (V <= 2^20 terms: the sum fits 2^60)
__device__ __forceinline__ u64 sm_mass(float x, float m, float inv_t) {
  return (u64)(__expf((x - m) * inv_t) * 1099511627776.f);      // (x = -inf: 0)
}

// The key at which the running sum of weights, taken from the largest key down, crosses `target`: the key v with
// W(keys > v) < target <= W(keys >= v), over the columns whose key is >= lo_key.
//   MASS = false: weight 1, target = the rank k -> the k-th largest key;
//   MASS = true:  weight = sm_mass, target = ceil(top_p * total weight) -> the smallest key with the mass above it < top_p.
// Every thread returns the same key.  hist [SM_BINS], scan [256], bc [2]: LDS.
template <typename TT, bool MASS>
__device__ __forceinline__ uint32_t radix_walk(const TT* row, const SampleK& P, uint32_t lo_key, u64 target, float m, float inv_t,
                                               u64* hist, u64* scan, u64* bc) {
  constexpr int KB = 8 * sizeof(TT);
  constexpr int NLEV = KB == 16 ? 2 : 3;
  const int tid = threadIdx.x;
  uint32_t found = 0;      // the digits chosen so far, in place
  u64 carry = 0;           // weight above the chosen prefix
#pragma unroll
  for (int lev = 0; lev < NLEV; ++lev) {
    const int shift = KB == 16 ? (lev == 0 ? 4 : 0) : (lev == 0 ? 20 : (lev == 1 ? 8 : 0));      // the digit's lowest bit
    const int width = (lev == 0 ? KB : (KB == 16 ? 4 : (lev == 1 ? 20 : 8))) - shift;          // 12, 12 (4), 8
#pragma unroll
    for (int i = 0; i < SM_PER_THREAD; ++i) hist[tid + 256 * i] = 0;
    __syncthreads();
    sm_for_each<TT>(row, P.V, P.vec, tid, [&](float x, int) {
      const uint32_t key = sm_key<KB>(x);
      bool in = key >= lo_key;
      if (lev > 0) in = in && ((key ^ found) >> (shift + width)) == 0;
      if (in) {
        const u64 w = MASS ? sm_mass(x, m, inv_t) : 1ull;
        if (w) atomicAdd(&hist[(key >> shift) & ((1u << width) - 1)], w);
      }
    });
    __syncthreads();
    u64 c[SM_PER_THREAD], tot = 0;
#pragma unroll
    for (int i = 0; i < SM_PER_THREAD; ++i) { c[i] = hist[tid * SM_PER_THREAD + i]; tot += c[i]; }
    scan[tid] = tot;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {      // inclusive suffix sums: scan[t] = the weight of the bins of threads >= t
      const u64 v = tid + o < 256 ? scan[tid + o] : 0;
      __syncthreads();
      scan[tid] += v;
      __syncthreads();
    }
    if (MASS && lev == 0) {
      const u64 total = scan[0];
      const double want = ceil((double)P.top_p * (double)total);      // integer A: A < top_p * total <=> A < ceil(top_p * total)
      target = want < 1.0 ? 1ull : (u64)want;
      if (target > total) target = total;
    }
    u64 A = carry + (scan[tid] - tot);
#pragma unroll
    for (int i = SM_PER_THREAD - 1; i >= 0; --i) {
      if (c[i] > 0 && A < target && A + c[i] >= target) { bc[0] = (u64)(tid * SM_PER_THREAD + i); bc[1] = A; }      // one bin in all
      A += c[i];
    }
    __syncthreads();
    found |= (uint32_t)bc[0] << shift;
    carry = bc[1];
    __syncthreads();
  }
  return found;
}

__device__ __forceinline__ bool sm_better(float av, int ai, float bv, int bi) { return (av > bv) | ((av == bv) & (ai < bi)); }

// grid = rows, 256 threads
template <typename TT>
__global__ __launch_bounds__(256) void sample_token_kernel(SampleK P) {
  constexpr int KB = 8 * sizeof(TT);
  __shared__ __attribute__((aligned(16))) u64 hist[SM_BINS];
  __shared__ u64 scan[256], bc[2];
  __shared__ float wm[4], ws[4], wv[4], wx[4];
  __shared__ int wi[4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int V = P.V;
  const TT* row = reinterpret_cast<const TT*>(P.x) + (int64_t)blockIdx.x * P.ld;

  // ---- 1. m, s of the whole row
  float m = -INFINITY, s = 0.f;
  sm_for_each<TT>(row, V, P.vec, tid, [&](float x, int) {
    if (x > m) {
      s = s * __expf(m - x) + 1.f;      // (m = -inf: s is 0 and stays 0 before the 1)
      m = x;
    } else if (x != -INFINITY) {
      s += __expf(x - m);
    }
  });
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) sm_join(m, s, __shfl_xor(m, o, 64), __shfl_xor(s, o, 64));
  if (lane == 0) { wm[w] = m; ws[w] = s; }
  __syncthreads();
  m = wm[0]; s = ws[0];
#pragma unroll
  for (int u = 1; u < 4; ++u) sm_join(m, s, wm[u], ws[u]);      // every thread the same order: the same bits

  // ---- 2, 3. the kept set is { key >= thr }
  const float inv_t = 1.f / P.temperature;
  uint32_t thr = 0;
  if (P.top_k > 0) thr = radix_walk<TT, false>(row, P, 0u, (u64)P.top_k, m, inv_t, hist, scan, bc);
  if (P.top_p < 1.f) thr = radix_walk<TT, true>(row, P, thr, 0ull, m, inv_t, hist, scan, bc);

  // ---- 4. Gumbel-max over the kept columns
  const uint64_t chi = ((uint64_t)P.ctr[blockIdx.x] & ((1ull << 44) - 1)) << 20;
  float bv = -INFINITY, bx = 0.f;
  int bi = INT_MAX;
  sm_for_each<TT>(row, V, P.vec, tid, [&](float x, int col) {
    if (sm_key<KB>(x) >= thr && x != -INFINITY) {
      const uint32_t h = fcmf_hash32(P.seed, chi | (uint64_t)col);
      const float u = ((float)(h >> 9) + 0.5f) * 1.1920928955078125e-07f;      // 2^-23: exact, in (0, 1)
      const float v = x / P.temperature - logf(-logf(u));
      if (sm_better(v, col, bv, bi)) { bv = v; bi = col; bx = x; }
    }
  });
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float ov = __shfl_xor(bv, o, 64), ox = __shfl_xor(bx, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (sm_better(ov, oi, bv, bi)) { bv = ov; bi = oi; bx = ox; }
  }
  if (lane == 0) { wv[w] = bv; wx[w] = bx; wi[w] = bi; }
  __syncthreads();
  if (tid != 0) return;
#pragma unroll
  for (int u = 1; u < 4; ++u)
    if (sm_better(wv[u], wi[u], bv, bi)) { bv = wv[u]; bi = wi[u]; bx = wx[u]; }
  P.ids[blockIdx.x] = bi;
  P.logp[blockIdx.x] = (bx - m) - logf(s);      // x - lse with lse = m + log s, as csrc/topk.hip forms it
}

extern "C" int fcmf_sample_token(const void* logits, int64_t ld, int rows, int V, float temperature, int top_k, float top_p,
                                 uint64_t seed, const int64_t* ctr, int32_t* ids, float* logp, int dtype, void* stream) {
  if (!logits || !ctr || !ids || !logp || rows < 0) return FCMF_ERR_ARG;
  if (dtype != FCMF_F32 && dtype != FCMF_BF16) return FCMF_ERR_UNSUPPORTED;
  if (V < 1 || V > (1 << 20)) return FCMF_ERR_UNSUPPORTED;
  if (!isfinite(temperature) || !(temperature > 0.f) || top_k < 0 || !(top_p > 0.f) || !(top_p <= 1.f)) return FCMF_ERR_ARG;
  if (ld < V) return FCMF_ERR_ARG;
  if (rows == 0) return FCMF_OK;
  const int64_t esz = dtype == FCMF_F32 ? 4 : 2;
  SampleK P{};
  P.x = logits; P.ld = ld; P.V = V; P.top_k = top_k >= V ? 0 : top_k;
  P.temperature = temperature; P.top_p = top_p; P.seed = seed; P.ctr = ctr; P.ids = ids; P.logp = logp;
  P.vec = (reinterpret_cast<uintptr_t>(logits) & 15) == 0 && (ld * esz) % 16 == 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 g(rows), b(256);
  return dtype == FCMF_F32 ? fcmf_launch(sample_token_kernel<float>, g, b, 0, st, P)
                           : fcmf_launch(sample_token_kernel<bf16_t>, g, b, 0, st, P);
}
