// Photo / ROI preprocessing of the category classifiers (reference image_processing/run_image_categories.py:35-41,79-85,
// run_roi_categories.py:34-45,81-89: v2.Resize((224,224), antialias=True) -> RandomHorizontalFlip -> ConvertImageDtype ->
// Normalize), restated as review_batches.to_crop computes it: F.interpolate(bilinear, antialias, align_corners=False) on the
// float values, round half to even, clamp to [0, 255], / 255, (x - mean) / std.
//
// PyTorch's antialiased bilinear resize is separable: a triangle filter whose support grows with the downscale factor, weights
// normalised per output index (so the borders renormalise), the horizontal pass first, then the vertical one.  Two launches:
//   pass 1: every crop row -> S horizontally resampled values (float scratch [n][3][max_rows][S]);
//   pass 2: the vertical taps over the scratch -> rint / clamp / normalise -> out [n][3][S][S], flipped at the output index.
// Both are memory-bound streams; the weights are recomputed per thread in the arithmetic order of ATen's CPU kernel
// (UpSampleKernel.cpp _compute_indices_min_size_weights_aa: float weights, its mixed float / double index arithmetic).
#include "common.h"

namespace {

struct Taps {
  int xmin, xsize;
  float center, invscale;
};

// ATen: scale = in / out (float), support = scale >= 1 ? scale : 1, center = scale * (i + 0.5),
// taps [xmin, xmin + xsize) clipped to the input, xsize <= ceil(support) * 2 + 1
__device__ __forceinline__ Taps aa_taps(int i, int in_size, int out_size) {
  const float scale = (float)in_size / (float)out_size;
  const float support = scale >= 1.0f ? scale : 1.0f;
  const int max_taps = (int)ceilf(support) * 2 + 1;
  Taps t;
  t.center = (float)((double)scale * ((double)i + 0.5));
  t.invscale = scale >= 1.0f ? (float)(1.0 / (double)scale) : 1.0f;
  const int64_t lo = (int64_t)((double)(t.center - support) + 0.5);
  const int64_t hi = (int64_t)((double)(t.center + support) + 0.5);
  t.xmin = (int)(lo > 0 ? lo : 0);
  const int64_t xs = (hi < in_size ? hi : in_size) - t.xmin;
  t.xsize = (int)(xs < 0 ? 0 : (xs > max_taps ? max_taps : xs));
  return t;
}

// unnormalised triangle weight of tap j: aa_filter(((j + xmin) - center + 0.5) * invscale)
__device__ __forceinline__ float aa_w(const Taps& t, int j) {
  const float d = (float)(j + t.xmin) - t.center;
  const float x = fabsf((float)(((double)d + 0.5) * (double)t.invscale));
  return x < 1.0f ? (float)(1.0 - (double)x) : 0.0f;
}

__device__ __forceinline__ float aa_total(const Taps& t) {
  float s = 0.f;
  for (int j = 0; j < t.xsize; ++j) s += aa_w(t, j);
  return s;
}

// the crop box clipped as a Python slice; false when it is empty or reaches outside the `src_bytes` of the source buffer
__device__ __forceinline__ bool crop_extent(const fcmf_crop_desc& d, int64_t src_bytes, int& hc, int& wc) {
  const int r1 = d.r1 < d.H ? d.r1 : d.H, c1 = d.c1 < d.W ? d.c1 : d.W;
  hc = r1 - d.r0; wc = c1 - d.c0;
  if (d.r0 < 0 || d.c0 < 0 || hc <= 0 || wc <= 0 || d.sC < 0 || d.sH < 0 || d.sW < 0 || d.offset < 0) return false;
  const int64_t last = d.offset + 2 * d.sC + (int64_t)(r1 - 1) * d.sH + (int64_t)(c1 - 1) * d.sW;
  return last < src_bytes;
}

struct Norm3 { float mean[3], std[3]; };

__global__ __launch_bounds__(256) void crop_resize_h_kernel(const uint8_t* __restrict__ src, int64_t src_bytes,
                                                            const fcmf_crop_desc* __restrict__ descs, int max_rows, int S,
                                                            float* __restrict__ scratch) {
  const int n = blockIdx.y;
  const fcmf_crop_desc d = descs[n];
  int hc, wc;
  if (!crop_extent(d, src_bytes, hc, wc) || hc > max_rows) return;          // pass 2 writes NaN for this crop
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int ox = (int)(idx % S);
  const int64_t t = idx / S;
  const int row = (int)(t % max_rows), c = (int)(t / max_rows);
  if (c >= 3 || row >= hc) return;
  const Taps tp = aa_taps(ox, wc, S);
  const float total = aa_total(tp);
  const uint8_t* p = src + d.offset + c * d.sC + (int64_t)(d.r0 + row) * d.sH + (int64_t)(d.c0 + tp.xmin) * d.sW;
  float acc = 0.f;
  for (int j = 0; j < tp.xsize; ++j) {
    const float w = total != 0.f ? aa_w(tp, j) / total : aa_w(tp, j);
    acc += (float)p[(int64_t)j * d.sW] * w;
  }
  scratch[(((int64_t)n * 3 + c) * max_rows + row) * S + ox] = acc;
}

template <typename T>
__global__ __launch_bounds__(256) void crop_resize_v_kernel(const float* __restrict__ scratch, int64_t src_bytes,
                                                            const fcmf_crop_desc* __restrict__ descs, int max_rows, int S,
                                                            Norm3 nm, T* __restrict__ out) {
  const int n = blockIdx.y;
  const fcmf_crop_desc d = descs[n];
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int ox = (int)(idx % S);
  const int64_t t = idx / S;
  const int oy = (int)(t % S), c = (int)(t / S);
  if (c >= 3) return;
  T* o = out + (((int64_t)n * 3 + c) * S + oy) * S + (d.flip ? S - 1 - ox : ox);
  int hc, wc;
  if (!crop_extent(d, src_bytes, hc, wc) || hc > max_rows) { *o = from_f32<T>(__builtin_nanf("")); return; }
  const Taps tp = aa_taps(oy, hc, S);
  const float total = aa_total(tp);
  const float* p = scratch + (((int64_t)n * 3 + c) * max_rows + tp.xmin) * S + ox;
  float acc = 0.f;
  for (int j = 0; j < tp.xsize; ++j) {
    const float w = total != 0.f ? aa_w(tp, j) / total : aa_w(tp, j);
    acc += p[(int64_t)j * S] * w;
  }
  const float v = fminf(fmaxf(rintf(acc), 0.f), 255.f) / 255.0f;
  *o = from_f32<T>((v - nm.mean[c]) / nm.std[c]);
}

}  // namespace

extern "C" int fcmf_crop_resize_normalize(const uint8_t* src, int64_t src_bytes, const fcmf_crop_desc* descs, int n, int max_rows,
                                          int S, const float* mean, const float* std, float* scratch, int64_t scratch_bytes,
                                          void* out, int dtype, void* stream) {
  if (!src || !descs || !mean || !std || !scratch || !out || n < 0 || n > 65535 || max_rows <= 0 || S <= 0 || src_bytes <= 0)
    return FCMF_ERR_ARG;
  if (dtype != FCMF_F32 && dtype != FCMF_BF16) return FCMF_ERR_UNSUPPORTED;
  if (scratch_bytes < (int64_t)n * 3 * max_rows * S * (int64_t)sizeof(float)) return FCMF_ERR_ARG;
  if (n == 0) return FCMF_OK;
  Norm3 nm;
  for (int c = 0; c < 3; ++c) {
    if (!(std[c] != 0.f)) return FCMF_ERR_ARG;
    nm.mean[c] = mean[c]; nm.std[c] = std[c];
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int64_t hx = ((int64_t)3 * max_rows * S + 255) / 256, vx = ((int64_t)3 * S * S + 255) / 256;
  if (hx > INT32_MAX || vx > INT32_MAX) return FCMF_ERR_ARG;
  hipLaunchKernelGGL(crop_resize_h_kernel, dim3((unsigned)hx, n), dim3(256), 0, st, src, src_bytes, descs, max_rows, S, scratch);
  FCMF_CHECK_LAUNCH();
  if (dtype == FCMF_F32)
    hipLaunchKernelGGL((crop_resize_v_kernel<float>), dim3((unsigned)vx, n), dim3(256), 0, st, scratch, src_bytes, descs, max_rows, S,
                       nm, (float*)out);
  else
    hipLaunchKernelGGL((crop_resize_v_kernel<bf16_t>), dim3((unsigned)vx, n), dim3(256), 0, st, scratch, src_bytes, descs, max_rows,
                       S, nm, (bf16_t*)out);
  FCMF_CHECK_LAUNCH();
  return FCMF_OK;
}
