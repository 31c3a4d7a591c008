// Cross entropy with class weights, label smoothing and a focal factor, per SEGMENT (row r belongs to segment r % segments):
//   l_n  = (1 - eps) w_y (1 - p_y)^gamma (-log p_y) + (eps / C) sum_c w_c (-log p_c)
//   loss = mult * sum_s [ sum_{n in s, live} l_n / sum_{n in s, live} w_{y_n} ]
// Forward rows, a one-workgroup reduction and the backward, in the two shapes of misc.hip's plain cross entropy: one wave per
// row below 1024 classes, one workgroup per row with 16-byte accesses from there on.  HBM-bound streaming kernels.
//
// What keeps the numbers honest:
//   * the row sum of exponentials is gathered WITHOUT the label's term (s_o), so 1 - p_y = s_o / (s_o + e_y) has no
//     subtraction in it: the focal factor matters exactly where 1.0f - p_y would have cancelled;
//   * log p_y = (x_y - m) - log s, and log s = log1p(s_o) when the label holds the row maximum (e_y = 1): a confident row's
//     loss of 1e-6 keeps its digits;
//   * the label's gradient is (A - B) p_y - B (1 - p_y) - w_y c (see row_coeffs), again without p_y - 1;
//   * the smoothing sum is W log s - sum_c w_c (x_c - m); the wide kernel, which learns m only at the end of its one pass,
//     gathers sum w_c (x_c - r_t) around a per-thread reference r_t (its first element) and shifts by (r_t - m) W_t afterwards,
//     so a common offset of the logits never meets the sum.
// Below them: the symmetric KL divergence of row pairs (the R-Drop consistency term), in the same two shapes.
// MODE: 0 = no smoothing (the weight is read at the label only), 1 = smoothing with unit weights, 2 = smoothing with weights.
#include "common.h"

// what a row's loss and gradient need beside the sums: q = 1 - p_y, p_y, log p_y and log s (s = the whole row's sum of exp(x - m))
struct RowTerms { float q, py, lp, logs; };
__device__ __forceinline__ RowTerms row_terms(float xy, float m, float so) {
  RowTerms t;
  const float ey = expf(xy - m), s = so + ey;
  t.q = so / s;
  t.py = ey / s;
  t.logs = xy == m ? log1pf(so) : logf(s);
  t.lp = (xy - m) - t.logs;
  return t;
}

__device__ __forceinline__ float row_loss(const RowTerms& t, float wy, float W, float A, float eps, float gamma, int C) {
  const float focal = gamma > 0.f ? powf(t.q, gamma) : 1.0f;
  float l = (1.0f - eps) * wy * focal * (-t.lp);
  if (eps > 0.f) l += (eps / (float)C) * (W * t.logs - A);
  return l;
}

// the row's gradient is  d_j = p_j a - [j == y] b - w_j c  (c = 0 without smoothing); at the label it is written as
// amb p_y - b q - w_y c with amb = a - b.  sc = mult / D_s times the upstream gradient.
struct RowCoeffs { float a, b, amb, c; };
__device__ __forceinline__ RowCoeffs row_coeffs(const RowTerms& t, float wy, float W, float eps, float gamma, int C, float sc) {
  RowCoeffs k;
  if (gamma > 0.f) {
    const float f = t.q > 0.f ? wy * (powf(t.q, gamma) - gamma * t.py * powf(t.q, gamma - 1.0f) * t.lp) : 0.f;
    k.a = k.b = f * sc; k.amb = 0.f; k.c = 0.f;
  } else {
    k.b = sc * (1.0f - eps) * wy;
    k.amb = sc * (eps / (float)C) * W;
    k.a = k.b + k.amb;
    k.c = sc * (eps / (float)C);
  }
  return k;
}

// ---- one wave per row (C < 1024) -------------------------------------------------------------------------------------------
// wave-wide (max, sum_{c != lab} exp(x - max), sum w, sum w (x - max)) of lr[0..C): every lane returns the same values
template <typename T, int MODE, bool WX>
__device__ __forceinline__ void wave_row_stats(const T* __restrict__ lr, const float* __restrict__ wr, int C, int lab, float& m_out,
                                               float& so_out, float& W_out, float& A_out) {
  const int lane = threadIdx.x & 63;
  float m = -INFINITY;
  for (int c = lane; c < C; c += 64) m = fmaxf(m, to_f32<T>(lr[c]));
  m = wave_max(m);
  float so = 0.f, W = 0.f, A = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float d = to_f32<T>(lr[c]) - m;
    if (c != lab) so += __expf(d);
    if (MODE == 2) { const float w = wr[c]; W += w; if (WX) A += w * d; }
    else if (MODE == 1 && WX) A += d;
  }
  m_out = m;
  so_out = wave_sum(so);
  W_out = MODE == 2 ? wave_sum(W) : (float)C;
  A_out = (MODE != 0 && WX) ? wave_sum(A) : 0.f;
}

template <typename T, int MODE>
__global__ __launch_bounds__(256) void xent_ex_fwd_kernel(const T* __restrict__ logits, int64_t ld, const int64_t* __restrict__ labels,
                                                          const float* __restrict__ weight, int64_t wstride, float* __restrict__ num,
                                                          float* __restrict__ den, int n, int C, int segments, int64_t ignore_index,
                                                          float eps, float gamma) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  const int64_t lab = labels[row];
  if (lab == ignore_index || lab < 0 || lab >= C) {      // a label outside [0, C) that is not ignore_index poisons the loss, reads nothing
    if (lane == 0) { num[row] = lab == ignore_index ? 0.f : NAN; den[row] = 0.f; }
    return;
  }
  const T* lr = logits + (int64_t)row * ld;
  const float* wr = weight ? weight + (int64_t)(row % segments) * wstride : nullptr;
  float m, so, W, A;
  wave_row_stats<T, MODE, true>(lr, wr, C, (int)lab, m, so, W, A);
  if (lane == 0) {
    const float wy = wr ? wr[lab] : 1.0f;
    const RowTerms t = row_terms(to_f32<T>(lr[lab]), m, so);
    num[row] = row_loss(t, wy, W, A, eps, gamma, C);
    den[row] = wy;
  }
}

template <typename T, int MODE>
__global__ __launch_bounds__(256) void xent_ex_bwd_kernel(const T* __restrict__ logits, int64_t ld, const int64_t* __restrict__ labels,
                                                          const float* __restrict__ weight, int64_t wstride, T* __restrict__ dlogits,
                                                          int64_t ldd, const float* __restrict__ scales, const float* __restrict__ gptr,
                                                          int n, int C, int segments, int64_t ignore_index, float eps, float gamma) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  const int64_t lab = labels[row];
  T* dr = dlogits + (int64_t)row * ldd;
  const int seg = row % segments;
  const float sc = scales[seg] * (gptr ? *gptr : 1.0f);
  if (lab == ignore_index || lab < 0 || lab >= C || sc == 0.f) {      // sc == 0: a segment without live weight
    for (int c = lane; c < C; c += 64) dr[c] = from_f32<T>(0.f);
    return;
  }
  const T* lr = logits + (int64_t)row * ld;
  const float* wr = weight ? weight + (int64_t)seg * wstride : nullptr;
  float m, so, W, A;
  wave_row_stats<T, MODE, false>(lr, wr, C, (int)lab, m, so, W, A);
  const float wy = wr ? wr[lab] : 1.0f;
  const RowTerms t = row_terms(to_f32<T>(lr[lab]), m, so);
  const RowCoeffs k = row_coeffs(t, wy, W, eps, gamma, C, sc);
  const float inv = k.a / (so + expf(to_f32<T>(lr[lab]) - m));
  for (int c = lane; c < C; c += 64) {
    const float wc = MODE == 2 ? wr[c] : 1.0f;
    float g = __expf(to_f32<T>(lr[c]) - m) * inv - wc * k.c;
    if (c == lab) g = k.amb * t.py - k.b * t.q - wc * k.c;
    dr[c] = from_f32<T>(g);
  }
}

// ---- one workgroup per row (C >= 1024) -------------------------------------------------------------------------------------
// block-wide statistics of lr[0..C) in ONE pass over the row: m = max, so = sum_{c != lab} exp(x - m), W = sum w, and with WX
// A = sum w (x - m).  Every thread returns the same values.  `vec`: the row (and the weight row) is aligned for 16-byte loads.
template <typename T, int MODE, bool WX>
__device__ __forceinline__ void block_row_stats(const T* lr, const float* __restrict__ wr, int C, int lab, bool vec, float& m_out,
                                                float& so_out, float& W_out, float& A_out) {
  constexpr int VN = XVec<T>::N;
  typedef typename XVec<T>::type vec_t;
  constexpr bool SUMS = MODE == 2 || (MODE == 1 && WX);      // a thread's sum of weights is needed (MODE 1: only for the shift)
  __shared__ float red[4][4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  float m = -INFINITY, so = 0.f, Wt = 0.f, At = 0.f, r = 0.f;
  const int Cv = vec ? (C / VN) * VN : 0;
  if (MODE != 0 && WX) {                                     // the thread's reference: its first element
    const int c0 = tid * VN < Cv ? tid * VN : Cv + tid;
    if (c0 < C) r = to_f32<T>(lr[c0]);
  }
  for (int c = tid * VN; c < Cv; c += 256 * VN) {
    const vec_t v = *reinterpret_cast<const vec_t*>(lr + c);
    float x[VN], mx = -INFINITY;
#pragma unroll
    for (int e = 0; e < VN; ++e) { x[e] = (float)v[e]; mx = fmaxf(mx, x[e]); }
    const float mn = fmaxf(m, mx);
    float acc = 0.f;
    if ((unsigned)(lab - c) < (unsigned)VN) {                // the label's chunk: its term stays out of the sum
#pragma unroll
      for (int e = 0; e < VN; ++e) acc += (c + e) == lab ? 0.f : __expf(x[e] - mn);
    } else {
#pragma unroll
      for (int e = 0; e < VN; ++e) acc += __expf(x[e] - mn);
    }
    so = (m == -INFINITY ? 0.f : so * __expf(m - mn)) + acc;
    m = mn;
    if (MODE == 2) {
#pragma unroll
      for (int e = 0; e < VN; e += 4) {
        const f32x4 wv = *reinterpret_cast<const f32x4*>(wr + c + e);
#pragma unroll
        for (int j = 0; j < 4; ++j) { Wt += wv[j]; if (WX) At += wv[j] * (x[e + j] - r); }
      }
    } else if (MODE == 1 && WX) {
#pragma unroll
      for (int e = 0; e < VN; ++e) At += x[e] - r;
      Wt += (float)VN;
    }
  }
  for (int c = Cv + tid; c < C; c += 256) {
    const float x = to_f32<T>(lr[c]);
    if (c == lab) online_merge(m, so, x, 0.f); else online_merge(m, so, x, 1.f);
    if (MODE == 2) { const float wc = wr[c]; Wt += wc; if (WX) At += wc * (x - r); }
    else if (MODE == 1 && WX) { At += x - r; Wt += 1.0f; }
  }
  float Ws = Wt;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    online_merge(m, so, __shfl_xor(m, o, 64), __shfl_xor(so, o, 64));
    if (MODE == 2) Ws += __shfl_xor(Ws, o, 64);
  }
  if (lane == 0) { red[0][w] = m; red[1][w] = so; red[2][w] = Ws; }
  __syncthreads();
  m = red[0][0]; so = red[1][0];
#pragma unroll
  for (int k = 1; k < 4; ++k) online_merge(m, so, red[0][k], red[1][k]);
  m_out = m; so_out = so;
  W_out = MODE == 2 ? (red[2][0] + red[2][1]) + (red[2][2] + red[2][3]) : (float)C;
  A_out = 0.f;
  if (SUMS && WX) {
    const float a = wave_sum(At + (r - m) * Wt);             // (a thread without elements has At = Wt = r = 0)
    if (lane == 0) red[3][w] = a;
    __syncthreads();
    A_out = (red[3][0] + red[3][1]) + (red[3][2] + red[3][3]);
  }
}

template <typename T, int MODE>
__global__ __launch_bounds__(256) void xent_ex_fwd_wide_kernel(const T* __restrict__ logits, int64_t ld,
                                                               const int64_t* __restrict__ labels, const float* __restrict__ weight,
                                                               int64_t wstride, float* __restrict__ num, float* __restrict__ den, int C,
                                                               int segments, int64_t ignore_index, float eps, float gamma, int vec) {
  const int row = blockIdx.x;
  const int64_t lab = labels[row];
  if (lab == ignore_index || lab < 0 || lab >= C) {
    if (threadIdx.x == 0) { num[row] = lab == ignore_index ? 0.f : NAN; den[row] = 0.f; }
    return;
  }
  const T* lr = logits + (int64_t)row * ld;
  const float* wr = weight ? weight + (int64_t)(row % segments) * wstride : nullptr;
  float m, so, W, A;
  block_row_stats<T, MODE, true>(lr, wr, C, (int)lab, vec != 0, m, so, W, A);
  if (threadIdx.x == 0) {
    const float wy = wr ? wr[lab] : 1.0f;
    const RowTerms t = row_terms(to_f32<T>(lr[lab]), m, so);
    num[row] = row_loss(t, wy, W, A, eps, gamma, C);
    den[row] = wy;
  }
}

// may run IN PLACE (dlogits == logits): the label's logit is read before the statistics pass, whose barrier every read of the
// row precedes; after it each element is read and written by the same thread.  Columns at or past C are never touched.
template <typename T, int MODE>
__global__ __launch_bounds__(256) void xent_ex_bwd_wide_kernel(const T* logits, int64_t ld, const int64_t* __restrict__ labels,
                                                               const float* __restrict__ weight, int64_t wstride, T* dlogits,
                                                               int64_t ldd, const float* __restrict__ scales,
                                                               const float* __restrict__ gptr, int C, int segments,
                                                               int64_t ignore_index, float eps, float gamma, int vec) {
  constexpr int VN = XVec<T>::N;
  typedef typename XVec<T>::type vec_t;
  const int row = blockIdx.x, tid = threadIdx.x;
  const int64_t lab64 = labels[row];
  T* dr = dlogits + (int64_t)row * ldd;
  const int Cv = vec ? (C / VN) * VN : 0;
  const int seg = row % segments;
  const float sc = scales[seg] * (gptr ? *gptr : 1.0f);
  if (lab64 == ignore_index || lab64 < 0 || lab64 >= C || sc == 0.f) {
    vec_t z;
#pragma unroll
    for (int e = 0; e < VN; ++e) z[e] = from_f32<T>(0.f);
    for (int c = tid * VN; c < Cv; c += 256 * VN) *reinterpret_cast<vec_t*>(dr + c) = z;
    for (int c = Cv + tid; c < C; c += 256) dr[c] = from_f32<T>(0.f);
    return;
  }
  const int lab = (int)lab64;
  const T* lr = logits + (int64_t)row * ld;
  const float* wr = weight ? weight + (int64_t)seg * wstride : nullptr;
  const float xy = to_f32<T>(lr[lab]);
  float m, so, W, A;
  block_row_stats<T, MODE, false>(lr, wr, C, lab, vec != 0, m, so, W, A);
  const float wy = wr ? wr[lab] : 1.0f;
  const RowTerms t = row_terms(xy, m, so);
  const RowCoeffs k = row_coeffs(t, wy, W, eps, gamma, C, sc);
  const float inv = k.a / (so + expf(xy - m));
  const float gy = k.amb * t.py - k.b * t.q - wy * k.c;
  for (int c = tid * VN; c < Cv; c += 256 * VN) {
    const vec_t v = *reinterpret_cast<const vec_t*>(lr + c);
    float g[VN];
#pragma unroll
    for (int e = 0; e < VN; ++e) g[e] = __expf((float)v[e] - m) * inv;
    if (MODE == 2) {
#pragma unroll
      for (int e = 0; e < VN; e += 4) {
        const f32x4 wv = *reinterpret_cast<const f32x4*>(wr + c + e);
#pragma unroll
        for (int j = 0; j < 4; ++j) g[e + j] -= wv[j] * k.c;
      }
    } else if (MODE == 1) {
#pragma unroll
      for (int e = 0; e < VN; ++e) g[e] -= k.c;
    }
    if ((unsigned)(lab - c) < (unsigned)VN) {
#pragma unroll
      for (int e = 0; e < VN; ++e) g[e] = (c + e) == lab ? gy : g[e];
    }
    vec_t o;
#pragma unroll
    for (int e = 0; e < VN; ++e) o[e] = from_f32<T>(g[e]);
    *reinterpret_cast<vec_t*>(dr + c) = o;
  }
  for (int c = Cv + tid; c < C; c += 256) {
    const float wc = MODE == 2 ? wr[c] : 1.0f;
    const float g = __expf(to_f32<T>(lr[c]) - m) * inv - wc * k.c;
    dr[c] = from_f32<T>(c == lab ? gy : g);
  }
}

// ---- symmetric KL of row pairs (R-Drop): k = 1/2 [KL(p||q) + KL(q||p)] = 1/2 sum_c (p_c - q_c) d_c, d = a - b ---------------------
// A constant added to d changes neither k nor its gradients, so d is taken around max a - max b: d'_c = (a_c - max a) -
// (b_c - max b).  With S_a = sum exp(a - max a), T_a = sum exp(a - max a) d' (S_b, T_b likewise):
//   k       = 1/2 (T_a / S_a - T_b / S_b)
//   dk/da_j =  1/2 [p_j (d'_j - T_a / S_a) + p_j - q_j],   dk/db_j = -1/2 [q_j (d'_j - T_b / S_b) + p_j - q_j]
// Both sides run through the same inlined code, so bitwise-equal rows give S_a == S_b, T_a == T_b == 0, p_j == q_j: k and both
// gradients are exactly zero.  No log anywhere.  Finite logits are assumed (a -inf column has no d).
struct PairStats { float ma, mb, ia, ib, Ea, Eb; };      // the maxima, 1 / S and T / S of the two rows

__device__ __forceinline__ PairStats pair_stats(float ma, float mb, float sa, float sb, float ta, float tb) {
  PairStats p;
  p.ma = ma; p.mb = mb;
  p.ia = 1.0f / sa; p.ib = 1.0f / sb;
  p.Ea = ta / sa; p.Eb = tb / sb;
  return p;
}

// one side's share of an element: s += e, t += e * d with e = exp(x - m)
__device__ __forceinline__ void pair_side(float x, float m, float d, float& s, float& t) {
  const float e = __expf(x - m);
  s += e;
  t += e * d;
}

// the two gradients of one column: xa, xb the logits, h = 1/2 * scale.  No contraction here: p - q fused into fma(e_a, 1 / S_a, -q)
// would subtract a rounded q from an unrounded p and leave ~1e-10 where equal rows must give an exact zero.
__device__ __forceinline__ void pair_grads(const PairStats& st, float xa, float xb, float h, float& ga, float& gb) {
#pragma clang fp contract(off)
  const float da = xa - st.ma, db = xb - st.mb, d = da - db;
  const float p = __expf(da) * st.ia, q = __expf(db) * st.ib, pq = p - q;
  ga = h * (p * (d - st.Ea) + pq);
  gb = -h * (q * (d - st.Eb) + pq);
}

__device__ __forceinline__ bool pair_live(const int64_t* __restrict__ labels, int r, int64_t ignore_index) {
  return !labels || labels[r] != ignore_index;
}

// one wave per pair (C < 1024): a pass for the maxima, a pass for the sums; every lane returns the same values
template <typename T>
__device__ __forceinline__ PairStats wave_pair_stats(const T* __restrict__ ar, const T* __restrict__ br, int C) {
  const int lane = threadIdx.x & 63;
  float ma = -INFINITY, mb = -INFINITY;
  for (int c = lane; c < C; c += 64) { ma = fmaxf(ma, to_f32<T>(ar[c])); mb = fmaxf(mb, to_f32<T>(br[c])); }
  ma = wave_max(ma); mb = wave_max(mb);
  float sa = 0.f, sb = 0.f, ta = 0.f, tb = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float xa = to_f32<T>(ar[c]), xb = to_f32<T>(br[c]);
    const float d = (xa - ma) - (xb - mb);
    pair_side(xa, ma, d, sa, ta);
    pair_side(xb, mb, d, sb, tb);
  }
  return pair_stats(ma, mb, wave_sum(sa), wave_sum(sb), wave_sum(ta), wave_sum(tb));
}

template <typename T>
__global__ __launch_bounds__(256) void symkl_fwd_kernel(const T* __restrict__ a, int64_t lda, const T* __restrict__ b, int64_t ldb,
                                                        const int64_t* __restrict__ labels, float* __restrict__ num,
                                                        float* __restrict__ den, int n, int C, int64_t ignore_index) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n) return;
  if (!pair_live(labels, r, ignore_index)) {
    if (lane == 0) { num[r] = 0.f; den[r] = 0.f; }
    return;
  }
  const PairStats st = wave_pair_stats<T>(a + (int64_t)r * lda, b + (int64_t)r * ldb, C);
  if (lane == 0) { num[r] = 0.5f * (st.Ea - st.Eb); den[r] = 1.0f; }
}

template <typename T, bool ACC>
__global__ __launch_bounds__(256) void symkl_bwd_kernel(const T* __restrict__ a, int64_t lda, const T* __restrict__ b, int64_t ldb,
                                                        const int64_t* __restrict__ labels, T* __restrict__ da, int64_t ldda,
                                                        T* __restrict__ db, int64_t lddb, const float* __restrict__ scales,
                                                        const float* __restrict__ gptr, int n, int C, int segments,
                                                        int64_t ignore_index) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n) return;
  T* dar = da + (int64_t)r * ldda;
  T* dbr = db + (int64_t)r * lddb;
  const float sc = scales[r % segments] * (gptr ? *gptr : 1.0f);
  if (!pair_live(labels, r, ignore_index) || sc == 0.f) {      // sc == 0: a segment without a live pair
    if (!ACC)
      for (int c = lane; c < C; c += 64) { dar[c] = from_f32<T>(0.f); dbr[c] = from_f32<T>(0.f); }
    return;
  }
  const T* ar = a + (int64_t)r * lda;
  const T* br = b + (int64_t)r * ldb;
  const PairStats st = wave_pair_stats<T>(ar, br, C);
  const float h = 0.5f * sc;
  for (int c = lane; c < C; c += 64) {
    float ga, gb;
    pair_grads(st, to_f32<T>(ar[c]), to_f32<T>(br[c]), h, ga, gb);
    if (ACC) { ga += to_f32<T>(dar[c]); gb += to_f32<T>(dbr[c]); }
    dar[c] = from_f32<T>(ga);
    dbr[c] = from_f32<T>(gb);
  }
}

// one workgroup per pair (C >= 1024), ONE pass over the two rows: a thread learns the maxima only at the end, so it gathers
// exp(x - running max) d around its own reference rho_t = a_first - b_first (the idea of block_row_stats' smoothing sum) and
// shifts by (rho_t - (max a - max b)) S_t once the block's maxima are known.  Every thread returns the same values.
template <typename T>
__device__ __forceinline__ PairStats block_pair_stats(const T* ar, const T* br, int C, bool vec) {
  constexpr int VN = XVec<T>::N;
  typedef typename XVec<T>::type vec_t;
  __shared__ float red[6][4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int Cv = vec ? (C / VN) * VN : 0;
  float ma = -INFINITY, mb = -INFINITY, sa = 0.f, sb = 0.f, ta = 0.f, tb = 0.f, ra = 0.f, rb = 0.f;
  {
    const int c0 = tid * VN < Cv ? tid * VN : Cv + tid;
    if (c0 < C) { ra = to_f32<T>(ar[c0]); rb = to_f32<T>(br[c0]); }
  }
  for (int c = tid * VN; c < Cv; c += 256 * VN) {
    const vec_t va = *reinterpret_cast<const vec_t*>(ar + c);
    const vec_t vb = *reinterpret_cast<const vec_t*>(br + c);
    float xa[VN], xb[VN], na = ma, nb = mb;
#pragma unroll
    for (int e = 0; e < VN; ++e) { xa[e] = (float)va[e]; xb[e] = (float)vb[e]; na = fmaxf(na, xa[e]); nb = fmaxf(nb, xb[e]); }
    const float fa = ma == -INFINITY ? 0.f : __expf(ma - na), fb = mb == -INFINITY ? 0.f : __expf(mb - nb);
    sa *= fa; ta *= fa; sb *= fb; tb *= fb;
    ma = na; mb = nb;
#pragma unroll
    for (int e = 0; e < VN; ++e) {
      const float d = (xa[e] - ra) - (xb[e] - rb);
      pair_side(xa[e], ma, d, sa, ta);
      pair_side(xb[e], mb, d, sb, tb);
    }
  }
  for (int c = Cv + tid; c < C; c += 256) {
    const float xa = to_f32<T>(ar[c]), xb = to_f32<T>(br[c]);
    const float na = fmaxf(ma, xa), nb = fmaxf(mb, xb);
    const float fa = ma == -INFINITY ? 0.f : __expf(ma - na), fb = mb == -INFINITY ? 0.f : __expf(mb - nb);
    sa *= fa; ta *= fa; sb *= fb; tb *= fb;
    ma = na; mb = nb;
    const float d = (xa - ra) - (xb - rb);
    pair_side(xa, ma, d, sa, ta);
    pair_side(xb, mb, d, sb, tb);
  }
  const float wa = wave_max(ma), wb = wave_max(mb);
  if (lane == 0) { red[0][w] = wa; red[1][w] = wb; }
  __syncthreads();
  const float Ma = fmaxf(fmaxf(red[0][0], red[0][1]), fmaxf(red[0][2], red[0][3]));
  const float Mb = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
  // to the block's maxima and the block's centre (a thread without elements has s = t = 0 and a factor of 0)
  const float fa = ma == -INFINITY ? 0.f : __expf(ma - Ma), fb = mb == -INFINITY ? 0.f : __expf(mb - Mb);
  const float shift = (ra - rb) - (Ma - Mb);
  ta = (ta + shift * sa) * fa; sa *= fa;
  tb = (tb + shift * sb) * fb; sb *= fb;
  sa = wave_sum(sa); sb = wave_sum(sb); ta = wave_sum(ta); tb = wave_sum(tb);
  if (lane == 0) { red[2][w] = sa; red[3][w] = sb; red[4][w] = ta; red[5][w] = tb; }
  __syncthreads();
  return pair_stats(Ma, Mb, (red[2][0] + red[2][1]) + (red[2][2] + red[2][3]), (red[3][0] + red[3][1]) + (red[3][2] + red[3][3]),
                    (red[4][0] + red[4][1]) + (red[4][2] + red[4][3]), (red[5][0] + red[5][1]) + (red[5][2] + red[5][3]));
}

template <typename T>
__global__ __launch_bounds__(256) void symkl_fwd_wide_kernel(const T* __restrict__ a, int64_t lda, const T* __restrict__ b, int64_t ldb,
                                                             const int64_t* __restrict__ labels, float* __restrict__ num,
                                                             float* __restrict__ den, int C, int64_t ignore_index, int vec) {
  const int r = blockIdx.x;
  if (!pair_live(labels, r, ignore_index)) {
    if (threadIdx.x == 0) { num[r] = 0.f; den[r] = 0.f; }
    return;
  }
  const PairStats st = block_pair_stats<T>(a + (int64_t)r * lda, b + (int64_t)r * ldb, C, vec != 0);
  if (threadIdx.x == 0) { num[r] = 0.5f * (st.Ea - st.Eb); den[r] = 1.0f; }
}

// the second pass re-reads the two rows (L2) and, with ACC, the destinations: each element is read and written by the same thread
template <typename T, bool ACC>
__global__ __launch_bounds__(256) void symkl_bwd_wide_kernel(const T* __restrict__ a, int64_t lda, const T* __restrict__ b, int64_t ldb,
                                                             const int64_t* __restrict__ labels, T* __restrict__ da, int64_t ldda,
                                                             T* __restrict__ db, int64_t lddb, const float* __restrict__ scales,
                                                             const float* __restrict__ gptr, int C, int segments,
                                                             int64_t ignore_index, int vec) {
  constexpr int VN = XVec<T>::N;
  typedef typename XVec<T>::type vec_t;
  const int r = blockIdx.x, tid = threadIdx.x;
  T* dar = da + (int64_t)r * ldda;
  T* dbr = db + (int64_t)r * lddb;
  const int Cv = vec ? (C / VN) * VN : 0;
  const float sc = scales[r % segments] * (gptr ? *gptr : 1.0f);
  if (!pair_live(labels, r, ignore_index) || sc == 0.f) {
    if (!ACC) {
      vec_t z;
#pragma unroll
      for (int e = 0; e < VN; ++e) z[e] = from_f32<T>(0.f);
      for (int c = tid * VN; c < Cv; c += 256 * VN) { *reinterpret_cast<vec_t*>(dar + c) = z; *reinterpret_cast<vec_t*>(dbr + c) = z; }
      for (int c = Cv + tid; c < C; c += 256) { dar[c] = from_f32<T>(0.f); dbr[c] = from_f32<T>(0.f); }
    }
    return;
  }
  const T* ar = a + (int64_t)r * lda;
  const T* br = b + (int64_t)r * ldb;
  const PairStats st = block_pair_stats<T>(ar, br, C, vec != 0);
  const float h = 0.5f * sc;
  for (int c = tid * VN; c < Cv; c += 256 * VN) {
    const vec_t va = *reinterpret_cast<const vec_t*>(ar + c);
    const vec_t vb = *reinterpret_cast<const vec_t*>(br + c);
    float ga[VN], gb[VN];
#pragma unroll
    for (int e = 0; e < VN; ++e) pair_grads(st, (float)va[e], (float)vb[e], h, ga[e], gb[e]);
    if (ACC) {
      const vec_t pa = *reinterpret_cast<const vec_t*>(dar + c);
      const vec_t pb = *reinterpret_cast<const vec_t*>(dbr + c);
#pragma unroll
      for (int e = 0; e < VN; ++e) { ga[e] += (float)pa[e]; gb[e] += (float)pb[e]; }
    }
    vec_t oa, ob;
#pragma unroll
    for (int e = 0; e < VN; ++e) { oa[e] = from_f32<T>(ga[e]); ob[e] = from_f32<T>(gb[e]); }
    *reinterpret_cast<vec_t*>(dar + c) = oa;
    *reinterpret_cast<vec_t*>(dbr + c) = ob;
  }
  for (int c = Cv + tid; c < C; c += 256) {
    float ga, gb;
    pair_grads(st, to_f32<T>(ar[c]), to_f32<T>(br[c]), h, ga, gb);
    if (ACC) { ga += to_f32<T>(dar[c]); gb += to_f32<T>(dbr[c]); }
    dar[c] = from_f32<T>(ga);
    dbr[c] = from_f32<T>(gb);
  }
}

// ---- reduction: ONE workgroup, fixed order, float64 partial sums -------------------------------------------------------------
// The segments are taken one after the other; thread t sums the segment's rows s + t segments, s + (t + 256) segments, ...,
// the waves meet in a fixed butterfly and their four partial sums are added in wave order.  loss[0] = mult * sum_s N_s / D_s
// (0 / 0 = NaN, as torch), scales[s] = mult / D_s, 0 where D_s is not positive.
__global__ __launch_bounds__(256) void xent_ex_reduce_kernel(const float* __restrict__ num, const float* __restrict__ den, int n,
                                                             int segments, float mult, float* __restrict__ loss,
                                                             float* __restrict__ scales) {
  __shared__ double part[2][2][4];                         // [parity of the segment][num, den][wave]: one barrier per segment
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double tot = 0.0;
  for (int s = 0; s < segments; ++s) {
    double a = 0.0, b = 0.0;
#pragma unroll 4
    for (int64_t r = s + (int64_t)threadIdx.x * segments; r < n; r += (int64_t)256 * segments) { a += (double)num[r]; b += (double)den[r]; }
    a = wave_sum_d(a); b = wave_sum_d(b);
    if (lane == 0) { part[s & 1][0][w] = a; part[s & 1][1][w] = b; }
    __syncthreads();
    a = (part[s & 1][0][0] + part[s & 1][0][1]) + (part[s & 1][0][2] + part[s & 1][0][3]);
    b = (part[s & 1][1][0] + part[s & 1][1][1]) + (part[s & 1][1][2] + part[s & 1][1][3]);
    tot += a / b;
    if (threadIdx.x == 0) scales[s] = b > 0.0 ? (float)((double)mult / b) : 0.f;
  }
  if (threadIdx.x == 0) loss[0] = (float)((double)mult * tot);
}

// ---- host ------------------------------------------------------------------------------------------------------------------
static int xent_ex_args(const void* logits, const int64_t* labels, const float* weight, int64_t wstride, int64_t ld, int n, int C,
                        int segments, float eps, float gamma, int dtype) {
  if (!logits || !labels || n < 0 || C <= 0 || ld < C || segments < 1 || n % segments != 0) return FCMF_ERR_ARG;
  if (!(eps >= 0.f && eps < 1.f) || !(gamma >= 0.f) || gamma > 3.0e38f) return FCMF_ERR_ARG;
  if (weight && wstride != 0 && wstride < C) return FCMF_ERR_ARG;
  if (eps > 0.f && gamma > 0.f) return FCMF_ERR_UNSUPPORTED;
  if (dtype != FCMF_F32 && dtype != FCMF_BF16) return FCMF_ERR_UNSUPPORTED;
  return FCMF_OK;
}

static int xent_ex_vec(const void* a, int64_t lda, const void* b, int64_t ldb, const float* weight, int64_t wstride, int segments,
                       int dtype) {
  const int es = dtype == FCMF_F32 ? 4 : 2;
  uintptr_t bits = reinterpret_cast<uintptr_t>(a) | (uintptr_t)(lda * es);
  if (b) bits |= reinterpret_cast<uintptr_t>(b) | (uintptr_t)(ldb * es);
  if (weight) bits |= reinterpret_cast<uintptr_t>(weight) | (segments > 1 ? (uintptr_t)(wstride * 4) : 0);
  return (bits & 15) == 0;
}

// kernel<T, MODE> by the runtime mode
#define XENT_EX_BY_MODE(KERNEL, GRID, ...)                                                              \
  do {                                                                                                  \
    if (mode == 0) hipLaunchKernelGGL((KERNEL<T, 0>), GRID, dim3(256), 0, st, __VA_ARGS__);             \
    else if (mode == 1) hipLaunchKernelGGL((KERNEL<T, 1>), GRID, dim3(256), 0, st, __VA_ARGS__);        \
    else hipLaunchKernelGGL((KERNEL<T, 2>), GRID, dim3(256), 0, st, __VA_ARGS__);                       \
  } while (0)

template <typename T>
static void xent_ex_fwd_launch(hipStream_t st, int mode, int vec, const T* logits, int64_t ld, const int64_t* labels, const float* weight,
                               int64_t wstride, float* num, float* den, int n, int C, int segments, int64_t ignore_index, float eps,
                               float gamma) {
  if (C >= 1024)      // wide class axis: one workgroup per row
    XENT_EX_BY_MODE(xent_ex_fwd_wide_kernel, dim3(n), logits, ld, labels, weight, wstride, num, den, C, segments, ignore_index, eps, gamma, vec);
  else
    XENT_EX_BY_MODE(xent_ex_fwd_kernel, dim3((n + 3) / 4), logits, ld, labels, weight, wstride, num, den, n, C, segments, ignore_index, eps, gamma);
}

template <typename T>
static void xent_ex_bwd_launch(hipStream_t st, int mode, int vec, const T* logits, int64_t ld, const int64_t* labels, const float* weight,
                               int64_t wstride, T* dlogits, int64_t ldd, const float* scales, const float* grad, int n, int C,
                               int segments, int64_t ignore_index, float eps, float gamma) {
  if (C >= 1024)
    XENT_EX_BY_MODE(xent_ex_bwd_wide_kernel, dim3(n), logits, ld, labels, weight, wstride, dlogits, ldd, scales, grad, C, segments, ignore_index, eps, gamma, vec);
  else
    XENT_EX_BY_MODE(xent_ex_bwd_kernel, dim3((n + 3) / 4), logits, ld, labels, weight, wstride, dlogits, ldd, scales, grad, n, C, segments, ignore_index, eps, gamma);
}

extern "C" int fcmf_xent_fwd_ex(const void* logits, int64_t ld, const int64_t* labels, const float* weight, int64_t wstride,
                                float* num, float* den, int n, int C, int segments, int64_t ignore_index, float eps, float gamma,
                                int dtype, void* stream) {
  if (!num || !den) return FCMF_ERR_ARG;
  const int rc = xent_ex_args(logits, labels, weight, wstride, ld, n, C, segments, eps, gamma, dtype);
  if (rc != FCMF_OK) return rc;
  if (n == 0) return FCMF_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int mode = eps > 0.f ? (weight ? 2 : 1) : 0;
  const int vec = xent_ex_vec(logits, ld, nullptr, 0, weight, wstride, segments, dtype);
  if (dtype == FCMF_F32)
    xent_ex_fwd_launch<float>(st, mode, vec, (const float*)logits, ld, labels, weight, wstride, num, den, n, C, segments, ignore_index, eps, gamma);
  else
    xent_ex_fwd_launch<bf16_t>(st, mode, vec, (const bf16_t*)logits, ld, labels, weight, wstride, num, den, n, C, segments, ignore_index, eps, gamma);
  FCMF_CHECK_LAUNCH();
  return FCMF_OK;
}

extern "C" int fcmf_xent_reduce_ex(const float* num, const float* den, int n, int segments, float mult, float* loss, float* scales,
                                   void* stream) {
  if (!num || !den || !loss || !scales || n < 0 || segments < 1 || n % segments != 0) return FCMF_ERR_ARG;
  hipLaunchKernelGGL(xent_ex_reduce_kernel, dim3(1), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), num, den, n, segments, mult,
                     loss, scales);
  FCMF_CHECK_LAUNCH();
  return FCMF_OK;
}

extern "C" int fcmf_xent_bwd_ex(const void* logits, int64_t ld, const int64_t* labels, const float* weight, int64_t wstride,
                                void* dlogits, int64_t ldd, const float* scales, const float* grad, int n, int C, int segments,
                                int64_t ignore_index, float eps, float gamma, int dtype, void* stream) {
  if (!dlogits || !scales || ldd < C) return FCMF_ERR_ARG;
  const int rc = xent_ex_args(logits, labels, weight, wstride, ld, n, C, segments, eps, gamma, dtype);
  if (rc != FCMF_OK) return rc;
  if (n == 0) return FCMF_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int mode = eps > 0.f ? (weight ? 2 : 1) : 0;
  const int vec = xent_ex_vec(logits, ld, dlogits, ldd, weight, wstride, segments, dtype);
  if (dtype == FCMF_F32)
    xent_ex_bwd_launch<float>(st, mode, vec, (const float*)logits, ld, labels, weight, wstride, (float*)dlogits, ldd, scales, grad, n, C, segments, ignore_index, eps, gamma);
  else
    xent_ex_bwd_launch<bf16_t>(st, mode, vec, (const bf16_t*)logits, ld, labels, weight, wstride, (bf16_t*)dlogits, ldd, scales, grad, n, C, segments, ignore_index, eps, gamma);
  FCMF_CHECK_LAUNCH();
  return FCMF_OK;
}

// ---- symmetric KL: host ----------------------------------------------------------------------------------------------------
static int symkl_args(const void* a, int64_t lda, const void* b, int64_t ldb, int n, int C, int segments, int dtype) {
  if (!a || !b || n < 0 || C <= 0 || lda < C || ldb < C || segments < 1 || n % segments != 0) return FCMF_ERR_ARG;
  if (dtype != FCMF_F32 && dtype != FCMF_BF16) return FCMF_ERR_UNSUPPORTED;
  return FCMF_OK;
}

// do the n rows of C elements behind p (stride ld) and behind q (stride ldq) share a byte?
static bool symkl_overlap(const void* p, int64_t ld, const void* q, int64_t ldq, int n, int C, int es) {
  const uintptr_t p0 = reinterpret_cast<uintptr_t>(p), q0 = reinterpret_cast<uintptr_t>(q);
  const uintptr_t p1 = p0 + (uintptr_t)(((int64_t)(n - 1) * ld + C) * es), q1 = q0 + (uintptr_t)(((int64_t)(n - 1) * ldq + C) * es);
  return p0 < q1 && q0 < p1;
}

template <typename T>
static void symkl_fwd_launch(hipStream_t st, int vec, const T* a, int64_t lda, const T* b, int64_t ldb, const int64_t* labels, float* num,
                             float* den, int n, int C, int64_t ignore_index) {
  if (C >= 1024)
    hipLaunchKernelGGL((symkl_fwd_wide_kernel<T>), dim3(n), dim3(256), 0, st, a, lda, b, ldb, labels, num, den, C, ignore_index, vec);
  else
    hipLaunchKernelGGL((symkl_fwd_kernel<T>), dim3((n + 3) / 4), dim3(256), 0, st, a, lda, b, ldb, labels, num, den, n, C, ignore_index);
}

template <typename T, bool ACC>
static void symkl_bwd_launch(hipStream_t st, int vec, const T* a, int64_t lda, const T* b, int64_t ldb, const int64_t* labels, T* da,
                             int64_t ldda, T* db, int64_t lddb, const float* scales, const float* grad, int n, int C, int segments,
                             int64_t ignore_index) {
  if (C >= 1024)
    hipLaunchKernelGGL((symkl_bwd_wide_kernel<T, ACC>), dim3(n), dim3(256), 0, st, a, lda, b, ldb, labels, da, ldda, db, lddb, scales,
                       grad, C, segments, ignore_index, vec);
  else
    hipLaunchKernelGGL((symkl_bwd_kernel<T, ACC>), dim3((n + 3) / 4), dim3(256), 0, st, a, lda, b, ldb, labels, da, ldda, db, lddb,
                       scales, grad, n, C, segments, ignore_index);
}

extern "C" int fcmf_symkl_fwd(const void* a, int64_t lda, const void* b, int64_t ldb, const int64_t* labels, float* num, float* den,
                              int n, int C, int segments, int64_t ignore_index, int dtype, void* stream) {
  if (!num || !den) return FCMF_ERR_ARG;
  const int rc = symkl_args(a, lda, b, ldb, n, C, segments, dtype);
  if (rc != FCMF_OK) return rc;
  if (n == 0) return FCMF_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int vec = xent_ex_vec(a, lda, b, ldb, nullptr, 0, 1, dtype);
  if (dtype == FCMF_F32)
    symkl_fwd_launch<float>(st, vec, (const float*)a, lda, (const float*)b, ldb, labels, num, den, n, C, ignore_index);
  else
    symkl_fwd_launch<bf16_t>(st, vec, (const bf16_t*)a, lda, (const bf16_t*)b, ldb, labels, num, den, n, C, ignore_index);
  FCMF_CHECK_LAUNCH();
  return FCMF_OK;
}

extern "C" int fcmf_symkl_bwd(const void* a, int64_t lda, const void* b, int64_t ldb, const int64_t* labels, void* da, int64_t ldda,
                              void* db, int64_t lddb, const float* scales, const float* grad, int n, int C, int segments,
                              int64_t ignore_index, int acc, int dtype, void* stream) {
  if (!da || !db || !scales || ldda < C || lddb < C || (acc != 0 && acc != 1)) return FCMF_ERR_ARG;
  const int rc = symkl_args(a, lda, b, ldb, n, C, segments, dtype);
  if (rc != FCMF_OK) return rc;
  if (n == 0) return FCMF_OK;
  const int es = dtype == FCMF_F32 ? 4 : 2;
  if (symkl_overlap(da, ldda, a, lda, n, C, es) || symkl_overlap(da, ldda, b, ldb, n, C, es) ||
      symkl_overlap(db, lddb, a, lda, n, C, es) || symkl_overlap(db, lddb, b, ldb, n, C, es) ||
      symkl_overlap(da, ldda, db, lddb, n, C, es))
    return FCMF_ERR_ARG;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int vec = xent_ex_vec(a, lda, b, ldb, nullptr, 0, 1, dtype) && xent_ex_vec(da, ldda, db, lddb, nullptr, 0, 1, dtype);
#define SYMKL_BWD(T, ACC)                                                                                                     \
  symkl_bwd_launch<T, ACC>(st, vec, (const T*)a, lda, (const T*)b, ldb, labels, (T*)da, ldda, (T*)db, lddb, scales, grad, n, C, \
                           segments, ignore_index)
  if (dtype == FCMF_F32) { if (acc) SYMKL_BWD(float, true); else SYMKL_BWD(float, false); }
  else { if (acc) SYMKL_BWD(bf16_t, true); else SYMKL_BWD(bf16_t, false); }
#undef SYMKL_BWD
  FCMF_CHECK_LAUNCH();
  return FCMF_OK;
}
