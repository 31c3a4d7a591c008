// Shared device helpers for the FCMF gfx950 kernels (wave64, CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/fcmf_hip.h"

typedef __bf16 bf16_t;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#define FCMF_CHECK_LAUNCH()                                            \
  do {                                                                 \
    hipError_t e__ = hipGetLastError();                                \
    if (e__ != hipSuccess) return FCMF_ERR_LAUNCH;                     \
  } while (0)

// Launches k(args...) and returns FCMF_OK / FCMF_ERR_LAUNCH.  A launch with dynamic LDS first raises the kernel's
// dynamic-LDS limit to `smem` (above 64 KiB the default limit refuses the launch) -- before EVERY such launch, or, with
// `attr_set`, at the first launch through that flag only (kernels whose dynamic LDS is one constant: attn_mfma.hip).
template <class... P, class... A>
static int fcmf_launch_flagged(bool* attr_set, void (*k)(P...), dim3 grid, dim3 block, size_t smem, hipStream_t st, A&&... args) {
  if (smem && !(attr_set && *attr_set)) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    if (attr_set) *attr_set = true;
  }
  hipLaunchKernelGGL(k, grid, block, smem, st, static_cast<P>(args)...);
  FCMF_CHECK_LAUNCH();
  return FCMF_OK;
}
template <class... P, class... A>
static int fcmf_launch(void (*k)(P...), dim3 grid, dim3 block, size_t smem, hipStream_t st, A&&... args) {
  return fcmf_launch_flagged(nullptr, k, grid, block, smem, st, args...);
}

// ---- scalar conversions ----------------------------------------------------------------
template <typename T> __device__ __forceinline__ float to_f32(T x);
template <> __device__ __forceinline__ float to_f32<float>(float x) { return x; }
template <> __device__ __forceinline__ float to_f32<bf16_t>(bf16_t x) { return (float)x; }
template <typename T> __device__ __forceinline__ T from_f32(float x);
template <> __device__ __forceinline__ float from_f32<float>(float x) { return x; }
template <> __device__ __forceinline__ bf16_t from_f32<bf16_t>(float x) { return (bf16_t)x; }

// 4-wide vector load/store of T as float4 (T = float: 16 B, T = bf16: 8 B)
template <typename T> struct Vec4;
template <> struct Vec4<float> {
  typedef float4 raw;      // as loaded, before conversion (software-pipelined loops hold the next row in this form)
  static __device__ __forceinline__ raw load_raw(const float* p) { return *reinterpret_cast<const float4*>(p); }
  static __device__ __forceinline__ float4 cvt(raw v) { return v; }
  static __device__ __forceinline__ float4 load(const float* p) { return *reinterpret_cast<const float4*>(p); }
  static __device__ __forceinline__ void store(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
};
template <> struct Vec4<bf16_t> {
  typedef bf16x4 raw;
  static __device__ __forceinline__ raw load_raw(const bf16_t* p) { return *reinterpret_cast<const bf16x4*>(p); }
  static __device__ __forceinline__ float4 cvt(raw v) { return make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]); }
  static __device__ __forceinline__ float4 load(const bf16_t* p) {
    bf16x4 v = *reinterpret_cast<const bf16x4*>(p);
    return make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
  }
  static __device__ __forceinline__ void store(bf16_t* p, float4 v) {
    bf16x4 o;
    o[0] = (bf16_t)v.x; o[1] = (bf16_t)v.y; o[2] = (bf16_t)v.z; o[3] = (bf16_t)v.w;
    *reinterpret_cast<bf16x4*>(p) = o;
  }
};

// ---- wave / block reductions (wave = 64 lanes) --------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- wide class axes (the cross-entropy kernels of misc.hip and loss.hip): 16 bytes of a row per lane, online softmax sums ----
template <typename T> struct XVec;
template <> struct XVec<float> { static constexpr int N = 4; typedef f32x4 type; };
template <> struct XVec<bf16_t> { static constexpr int N = 8; typedef bf16x8 type; };

// (m, s) <- the (max, sum of exp(x - max)) of two parts that hold (m, s) and (m2, s2)
__device__ __forceinline__ void online_merge(float& m, float& s, float m2, float s2) {
  const float mn = fmaxf(m, m2);
  s = (m == -INFINITY ? 0.f : s * __expf(m - mn)) + (m2 == -INFINITY ? 0.f : s2 * __expf(m2 - mn));
  m = mn;
}

// ---- column sums of a row-major matrix (fcmf_colsum, the LayerNorm backward's reduce pass) -----------------------------------
// out[c] += sum_r X[r, c] for the rows [blockIdx.y * rows_per_block, +rows_per_block) of the 256-column block blockIdx.x, by one
// workgroup of COLSUM_WAVES waves.  A lane owns V adjacent columns, so one wave instruction reads 256 contiguous columns of
// 64 * V / 256 rows (16 bytes per lane for float with V = 4 and bf16 with V = 8); a wave keeps COLSUM_INFLIGHT such
// instructions in flight (8 KB), a workgroup 128 KB: one workgroup per CU streams.  The parallelism is inside the workgroup, not
// in the number of row blocks, because every row block ends with one float atomic per column into the SAME addresses, which
// the memory side serialises.  `vec` = the rows are aligned for V-wide loads; without it, and for a lane whose V columns
// straddle N, the lane reads element by element.
constexpr int COLSUM_WAVES = 16, COLSUM_INFLIGHT = 8, COLSUM_MAX_ROWS = 2048;

template <typename T, int V>
__device__ __forceinline__ void colsum_block(const T* __restrict__ X, float* __restrict__ out, int M, int N, int64_t ldx,
                                             int rows_per_block, int vec) {
  typedef T raw_t __attribute__((ext_vector_type(V)));
  constexpr int LPR = 256 / V, RPI = 64 / LPR;             // lanes per row, rows per wave instruction
  constexpr int STEP = RPI * COLSUM_WAVES, U = COLSUM_INFLIGHT;
  static_assert(V % 4 == 0 && 256 % V == 0 && LPR <= 64 && U == 8, "colsum_block: lane layout");
  __shared__ __attribute__((aligned(16))) float red[COLSUM_WAVES][RPI * 256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane / LPR, cl = (lane % LPR) * V;
  const int col = blockIdx.x * 256 + cl;
  const int r0 = blockIdx.y * rows_per_block;
  const int r1 = min(M, r0 + rows_per_block);
  float s[V];
#pragma unroll
  for (int j = 0; j < V; ++j) s[j] = 0.f;
  int r = r0 + RPI * wave + sub;                            // this lane's rows: r, r + STEP, r + 2 STEP, ...
  if (vec && col + V - 1 < N) {
    raw_t v[U];
    auto add = [&]() {
#pragma unroll
      for (int j = 0; j < V; ++j)
        s[j] += (((float)v[0][j] + (float)v[1][j]) + ((float)v[2][j] + (float)v[3][j])) +
                (((float)v[4][j] + (float)v[5][j]) + ((float)v[6][j] + (float)v[7][j]));
    };
    for (; r + (U - 1) * STEP < r1; r += U * STEP) {
      const T* p = X + (int64_t)r * ldx + col;
#pragma unroll
      for (int u = 0; u < U; ++u) v[u] = *reinterpret_cast<const raw_t*>(p + (int64_t)u * STEP * ldx);
      add();
    }
    if (r < r1) {                                           // the last, partial batch: the same loads, each behind its row test
      const T* p = X + (int64_t)r * ldx + col;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        v[u] = raw_t{};
        if (r + u * STEP < r1) v[u] = *reinterpret_cast<const raw_t*>(p + (int64_t)u * STEP * ldx);
      }
      add();
    }
  } else if (col < N) {
    for (; r < r1; r += STEP) {
      const T* p = X + (int64_t)r * ldx + col;
#pragma unroll
      for (int j = 0; j < V; ++j)
        if (col + j < N) s[j] += to_f32<T>(p[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < V; j += 4)
    *reinterpret_cast<float4*>(&red[wave][sub * 256 + cl + j]) = make_float4(s[j], s[j + 1], s[j + 2], s[j + 3]);
  __syncthreads();
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (threadIdx.x < 256 && c < N) {                         // thread t finishes column t: 256 contiguous atomics per wave
    float a = 0.f, b = 0.f;
#pragma unroll
    for (int w = 0; w < COLSUM_WAVES; w += 2)
#pragma unroll
      for (int h = 0; h < RPI; ++h) { a += red[w][h * 256 + threadIdx.x]; b += red[w + 1][h * 256 + threadIdx.x]; }
    atomicAdd(out + c, a + b);
  }
}

// rows per workgroup for `colblocks` column blocks in all: about one workgroup per CU (256), a whole number of the
// workgroup's row groups (`rpi` = rows per wave instruction), at most COLSUM_MAX_ROWS (a lane's chain of additions stays short;
// beyond it the row blocks, and with them the atomics per column, grow instead)
static inline int colsum_rows_per_block(int M, int64_t colblocks, int rpi) {
  const int64_t unit = COLSUM_WAVES * rpi;
  int64_t rpb = ((int64_t)M * colblocks + 255) / 256;
  rpb = (rpb + unit - 1) / unit * unit;
  return (int)(rpb < unit ? unit : (rpb > COLSUM_MAX_ROWS ? COLSUM_MAX_ROWS : rpb));
}

// ---- counter-based dropout RNG --------------------------------------------------------------
// Stateless hash of (seed, element index): forward and backward regenerate the same mask without storing
// it.  One 32-bit hash (the "lowbias32" integer finaliser: two 32-bit multiplies -- integer multiplies are
// quarter rate on CDNA, so they are what a mask costs) decides TWO consecutive elements, 16 bits each: an
// element is dropped when its 16 bits fall below p * 65536 (p is honoured to 1.5e-5).
// (the two multiply rounds, given x = lo ^ seed_lo ^ rotl(hi, 7): kernels whose `hi` and seed are wave-uniform fold that part
//  into one scalar and call this directly)
__device__ __forceinline__ uint32_t fcmf_hash32_rounds(uint32_t x, uint32_t s1) {
  x ^= x >> 16; x *= 0x7feb352du;
  x ^= s1;
  x ^= x >> 15; x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}
__device__ __forceinline__ uint32_t fcmf_hash32(uint64_t seed, uint64_t pair) {
  const uint32_t s0 = (uint32_t)seed, s1 = (uint32_t)(seed >> 32);
  const uint32_t lo = (uint32_t)pair, hi = (uint32_t)(pair >> 32);
  return fcmf_hash32_rounds(lo ^ s0 ^ ((hi << 7) | (hi >> 25)), s1);
}
__device__ __forceinline__ uint32_t dropout_threshold(float p) { return (uint32_t)(p * 65536.0f + 0.5f); }
// returns the multiplier applied to the element: 0 (dropped) or 1/(1-p) (kept)
__device__ __forceinline__ float dropout_mult(uint64_t seed, uint64_t idx, float p, float inv_keep) {
  const uint32_t h = fcmf_hash32(seed, idx >> 1);
  const uint32_t bits = (idx & 1) ? (h >> 16) : (h & 0xFFFFu);
  return bits >= dropout_threshold(p) ? inv_keep : 0.0f;
}
// multipliers of the 4 consecutive elements base .. base+3 (same values as four dropout_mult calls):
// two hashes when base is even, three otherwise
__device__ __forceinline__ void dropout_mult4(uint64_t seed, uint64_t base, float p, float inv_keep, float (&m)[4]) {
  const uint32_t thr = dropout_threshold(p);
  const uint64_t k0 = base >> 1;
  const uint32_t h0 = fcmf_hash32(seed, k0), h1 = fcmf_hash32(seed, k0 + 1);
  if ((base & 1) == 0) {
    m[0] = (h0 & 0xFFFFu) >= thr ? inv_keep : 0.f; m[1] = (h0 >> 16) >= thr ? inv_keep : 0.f;
    m[2] = (h1 & 0xFFFFu) >= thr ? inv_keep : 0.f; m[3] = (h1 >> 16) >= thr ? inv_keep : 0.f;
  } else {
    const uint32_t h2 = fcmf_hash32(seed, k0 + 2);
    m[0] = (h0 >> 16) >= thr ? inv_keep : 0.f;     m[1] = (h1 & 0xFFFFu) >= thr ? inv_keep : 0.f;
    m[2] = (h1 >> 16) >= thr ? inv_keep : 0.f;     m[3] = (h2 & 0xFFFFu) >= thr ? inv_keep : 0.f;
  }
}

// exact-erf GELU and its derivative (mm_modeling.py:10-15)
__device__ __forceinline__ float gelu_f(float x) { return x * 0.5f * (1.0f + erff(x * 0.70710678118654752440f)); }
__device__ __forceinline__ float dgelu_f(float x) {
  float cdf = 0.5f * (1.0f + erff(x * 0.70710678118654752440f));
  float pdf = 0.39894228040143267794f * __expf(-0.5f * x * x);
  return cdf + x * pdf;
}
