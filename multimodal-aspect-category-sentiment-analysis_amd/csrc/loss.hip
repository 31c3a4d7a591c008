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
