// Single-query attention with indexed keys (see include/fcmf_hip.h): the two attentions of an IAOG prefix-decode step.  Values
// are the keys (mm_modeling.py:129), the pairing is the plain one (slot s reads head s), so per (row r, head h):
//   score_p = scale * <q[r, h], key_p[h]> for p < live, exactly -1e4 for live <= p < T (the reference's masked_fill: the key
//   still takes part in the softmax and in the sum), out[r, h] = sum_p softmax(score)_p * key_p[h].
// key_p of row r lives at keys + p*k_sp + idx[r*idx_sr + p*idx_sp]*k_si + h*d: the self-attention cache [Tmax, rows, heads*d]
// read through the row's ancestor table, or the hoisted encoder keys [samples, Tk, heads*d] read through the sample index.
//
// Memory- and latency-bound: one wave per (row, head), keys straight to registers, 16 bytes per lane.  A key of d elements is
// d / VEC 16-byte chunks (VEC = 4 float / 8 bf16); G = the next power of two lanes hold one key, so a wave instruction reads
// 64 / G keys, U of them in flight (the index loads first, then the key loads).  A lane keeps an online softmax of the keys
// of its lane group -- running maximum m, denominator l and VEC accumulators, float32 -- the dot product is summed over the
// group by xor shuffles, and the 64 / G groups are joined by an xor butterfly at the end.  No LDS, no atomics, a fixed order:
// two launches give the same bits.
//
// Append: with k_new, row r's own key (position append_at) is taken from k_new[r] -- the cache is not read there, idx neither --
// and stored to keys + append_at*k_sp + r*k_si.  Every OTHER position is only read.  The stores of a launch touch position
// append_at alone and its loads never do, so no wave reads what another wave of the same launch writes: there is no hazard
// inside a launch, whatever the ancestor tables hold.
// An index outside [0, idx_n) reads nothing and makes the row's output NaN (as fcmf_embed_scale_fwd does for a bad id).
#include "common.h"

struct DecodeK {
  const void* q;
  void* keys;
  const int64_t* idx;
  const void* k_new;
  void* out;
  int64_t q_sr, k_sp, k_si, idx_sr, idx_sp, idx_n, kn_sr, o_sr;
  int pairs, heads, d, T, live, append_at, G, lg;      // G = 1 << lg lanes per key
  float scale;
};

constexpr int DEC_U = 4;      // keys in flight per lane

template <typename R, int VEC>
__device__ __forceinline__ void dec_cvt(const R& r, float (&x)[VEC]) {
#pragma unroll
  for (int e = 0; e < VEC; ++e) x[e] = (float)r[e];
}

// (m, l, acc) <- joined with (m2, l2, acc2); an empty side has m = -inf, l = 0
template <int VEC>
__device__ __forceinline__ void dec_join(float& m, float& l, float (&acc)[VEC], float m2, float l2, const float (&acc2)[VEC]) {
  const float M = fmaxf(m, m2);
  const float a = m == M ? 1.f : __expf(m - M), b = m2 == M ? 1.f : __expf(m2 - M);      // (-inf with -inf: no inf - inf)
  l = l * a + l2 * b;
#pragma unroll
  for (int e = 0; e < VEC; ++e) acc[e] = acc[e] * a + acc2[e] * b;
  m = M;
}

// grid = ceil(rows * heads / 4), 256 threads: wave w of block b serves pair 4 b + w = row * heads + head
template <typename TT>
__global__ __launch_bounds__(256) void attn_decode_kernel(DecodeK P) {
  constexpr int VEC = 16 / sizeof(TT);
  typedef TT raw_t __attribute__((ext_vector_type(VEC)));
  const int lane = threadIdx.x & 63;
  const int pair = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pair >= P.pairs) return;                               // (a whole wave: the shuffles below see all 64 lanes)
  const int r = pair / P.heads, h = pair - r * P.heads;
  const int c = lane & (P.G - 1), sub = lane >> P.lg, KP = 64 >> P.lg;
  const bool act = c * VEC < P.d;                            // lanes beyond the key's last chunk (d / VEC no power of two) idle
  const int64_t col = (int64_t)h * P.d + c * VEC;
  const TT* keys = reinterpret_cast<const TT*>(P.keys);
  const bool append = P.k_new != nullptr;

  float qv[VEC], own[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) { qv[e] = 0.f; own[e] = 0.f; }
  if (act) {
    const raw_t qr = *reinterpret_cast<const raw_t*>(reinterpret_cast<const TT*>(P.q) + r * P.q_sr + col);
    dec_cvt<raw_t, VEC>(qr, qv);
    if (append) {
      const raw_t kr = *reinterpret_cast<const raw_t*>(reinterpret_cast<const TT*>(P.k_new) + r * P.kn_sr + col);
      dec_cvt<raw_t, VEC>(kr, own);
      if (sub == 0) *reinterpret_cast<raw_t*>(reinterpret_cast<TT*>(P.keys) + P.append_at * P.k_sp + r * P.k_si + col) = kr;
    }
  }

  float m = -INFINITY, l = 0.f, acc[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) acc[e] = 0.f;
  bool bad = false;
  const int64_t* ix = P.idx + r * P.idx_sr;

  for (int p0 = 0; p0 < P.T; p0 += KP * DEC_U) {
    int64_t at[DEC_U];
    raw_t kr[DEC_U];
#pragma unroll
    for (int u = 0; u < DEC_U; ++u) {                        // the indices of this lane's next U keys
      const int p = p0 + u * KP + sub;
      at[u] = -1;
      if (p < P.T && !(append && p == P.append_at)) {
        const int64_t i = ix[p * P.idx_sp];
        if (i >= 0 && i < P.idx_n) at[u] = p * P.k_sp + i * P.k_si + col;
        else bad = true;
      }
    }
#pragma unroll
    for (int u = 0; u < DEC_U; ++u) {                        // their keys, all in flight
      kr[u] = raw_t{};
      if (act && at[u] >= 0) kr[u] = *reinterpret_cast<const raw_t*>(keys + at[u]);
    }
#pragma unroll
    for (int u = 0; u < DEC_U; ++u) {
      const int p = p0 + u * KP + sub;
      float kv[VEC];
      dec_cvt<raw_t, VEC>(kr[u], kv);
      if (append && p == P.append_at) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) kv[e] = own[e];
      }
      float s = 0.f;
#pragma unroll
      for (int e = 0; e < VEC; ++e) s += qv[e] * kv[e];
      for (int o = 1; o < P.G; o <<= 1) s += __shfl_xor(s, o, 64);      // (every lane of the wave runs this: G is uniform)
      s = p < P.live ? s * P.scale : -10000.0f;
      if (p < P.T) {
        const float mn = fmaxf(m, s);
        const float a = __expf(m - mn), pr = __expf(s - mn);            // (m = -inf: a = 0)
        l = l * a + pr;
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[e] = acc[e] * a + pr * kv[e];
        m = mn;
      }
    }
  }

  for (int o = P.G; o < 64; o <<= 1) {                       // the lane groups: every lane ends with the sums over all keys
    float acc2[VEC];
    const float m2 = __shfl_xor(m, o, 64), l2 = __shfl_xor(l, o, 64);
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc2[e] = __shfl_xor(acc[e], o, 64);
    dec_join<VEC>(m, l, acc, m2, l2, acc2);
  }
  bad = __any(bad);
  if (act && sub == 0) {
    const float inv = bad ? __builtin_nanf("") : 1.f / l;
    raw_t o;
#pragma unroll
    for (int e = 0; e < VEC; ++e) o[e] = (TT)(acc[e] * inv);
    *reinterpret_cast<raw_t*>(reinterpret_cast<TT*>(P.out) + r * P.o_sr + col) = o;
  }
}

static bool dec_aligned(const void* p, int64_t stride_bytes) {
  return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && stride_bytes % 16 == 0;
}

extern "C" int fcmf_attn_decode(const void* q, int64_t q_sr, void* keys, int64_t k_sp, int64_t k_si, const int64_t* idx,
                                int64_t idx_sr, int64_t idx_sp, int64_t idx_n, const void* k_new, int64_t kn_sr, int append_at,
                                void* out, int64_t o_sr, int n, int heads, int d, int T, int live, float scale, int dtype,
                                void* stream) {
  if (!q || !keys || !out || n < 0 || heads < 1 || idx_n < 1) return FCMF_ERR_ARG;
  if (dtype != FCMF_F32 && dtype != FCMF_BF16) return FCMF_ERR_UNSUPPORTED;
  if (d < 8 || d > 128 || d % 8 != 0 || T < 1 || T > 512) return FCMF_ERR_UNSUPPORTED;
  if (live < 0 || live > T) return FCMF_ERR_ARG;
  if (k_new && (append_at < 0 || append_at >= T || n > idx_n)) return FCMF_ERR_ARG;
  if (!idx && !(k_new && T == 1)) return FCMF_ERR_ARG;       // (only a lone appended key needs no index)
  if (q_sr < 0 || k_sp < 0 || k_si < 0 || idx_sr < 0 || idx_sp < 0 || kn_sr < 0 || o_sr < 0) return FCMF_ERR_ARG;
  const int64_t esz = dtype == FCMF_F32 ? 4 : 2;
  if (!dec_aligned(q, q_sr * esz) || !dec_aligned(keys, k_sp * esz) || k_si * esz % 16 != 0 || !dec_aligned(out, o_sr * esz) ||
      (k_new && !dec_aligned(k_new, kn_sr * esz)))
    return FCMF_ERR_ARG;
  const int64_t pairs = (int64_t)n * heads;
  if (pairs > INT32_MAX) return FCMF_ERR_UNSUPPORTED;
  if (n == 0) return FCMF_OK;
  DecodeK P{};
  P.q = q; P.keys = keys; P.idx = idx; P.k_new = k_new; P.out = out;
  P.q_sr = q_sr; P.k_sp = k_sp; P.k_si = k_si; P.idx_sr = idx_sr; P.idx_sp = idx_sp; P.idx_n = idx_n; P.kn_sr = kn_sr; P.o_sr = o_sr;
  P.pairs = (int)pairs; P.heads = heads; P.d = d; P.T = T; P.live = live; P.append_at = append_at; P.scale = scale;
  const int chunks = d / (int)(16 / esz);
  while ((1 << P.lg) < chunks) ++P.lg;
  P.G = 1 << P.lg;
  const dim3 g((unsigned)((pairs + 3) / 4)), b(256);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  return dtype == FCMF_F32 ? fcmf_launch(attn_decode_kernel<float>, g, b, 0, st, P)
                           : fcmf_launch(attn_decode_kernel<bf16_t>, g, b, 0, st, P);
}
