// Generation constraints on the logits of a decode step, in place (see include/fcmf_hip.h, fcmf_logits_constrain): repetition
// penalty, no-repeat n-gram bans, a minimum length and a list of always-suppressed ids, between the vocabulary GEMM and the
// tails csrc/topk.hip / csrc/sample.hip.  The work is O(L^2) integer compares and at most 2L + 1 + n_ban scattered element
// accesses per row -- never a pass over the V columns.  One 256-thread workgroup per row:
//   0. the row's sequence is staged once in LDS as int, through the two strides of `hist` (a value that does not fit an int
//      becomes INT_MIN: out of range for every store, and equal only to other such values in the n-gram compares);
//   1. repetition penalty: position p OWNS its token when no q < p holds the same one, and only the owner does the
//      read-modify-write of that column.  Distinct owners touch distinct addresses, so no atomic and no token penalised twice;
//   -- every store of phase 1 is complete (device-scope release) before the workgroup barrier: a ban below may hit a column
//      another thread has just penalised, and the ban must land later;
//   2. no-repeat n-gram: start i compares n - 1 tokens with the suffix, out of LDS, and stores -inf to the column of the token
//      that followed.  Several threads may store the same -inf to one address, which is benign;
//   3. the separator below the minimum length, and the suppressed ids: -inf stores.
// Stores are one element wide (2 bytes for bf16): a neighbouring column is never read or rewritten.  Two launches give the
// same bits: the only arithmetic is one float32 multiply or correctly rounded divide and one rounding to the storage type.
#include <limits.h>
#include <math.h>

#include "common.h"

constexpr int CONSTRAIN_MAX_T = 512, CONSTRAIN_MAX_BAN = 1024;

struct ConstrainK {
  void* x;
  int64_t ld;
  int V, L;
  const int64_t* hist;
  int64_t sr, sp;
  float theta;
  int ngram, ban_sep, sep, n_ban;      // ngram: 0 = off; ban_sep: L < min_length
  const int* ban;
};

// grid = rows, 256 threads
template <typename TT>
__global__ __launch_bounds__(256) void logits_constrain_kernel(ConstrainK P) {
  __shared__ int h[CONSTRAIN_MAX_T];
  const int tid = threadIdx.x, V = P.V, L = P.L;
  TT* row = reinterpret_cast<TT*>(P.x) + (int64_t)blockIdx.x * P.ld;
  const int64_t* hp = P.hist + (int64_t)blockIdx.x * P.sr;
  const TT ninf = from_f32<TT>(-INFINITY);

  for (int p = tid; p < L; p += 256) {
    const int64_t v = hp[(int64_t)p * P.sp];
    h[p] = (v < INT_MIN || v > INT_MAX) ? INT_MIN : (int)v;
  }
  __syncthreads();

  // ---- 1. repetition penalty, once per distinct token
  if (P.theta != 1.f) {
    for (int p = tid; p < L; p += 256) {
      const int v = h[p];
      if (v < 0 || v >= V) continue;
      bool own = true;
      for (int q = 0; q < p; ++q) own &= h[q] != v;
      if (!own) continue;
      const float x = to_f32<TT>(row[v]);
      row[v] = from_f32<TT>(x < 0.f ? x * P.theta : __fdiv_rn(x, P.theta));
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");      // the penalised columns are written before any ban below is issued
    __syncthreads();
  }

  // ---- 2. no-repeat n-gram: h[i .. i+n-2] == h[L-n+1 .. L-1] bans h[i+n-1]
  const int n = P.ngram;
  if (n >= 1 && L >= n) {
    const int* suf = h + (L - n + 1);
    for (int i = tid; i <= L - n; i += 256) {
      bool eq = true;
      for (int k = 0; k < n - 1 && eq; ++k) eq = h[i + k] == suf[k];
      const int v = h[i + n - 1];
      if (eq && v >= 0 && v < V) row[v] = ninf;
    }
  }

  // ---- 3. the separator below the minimum length, the suppressed ids
  if (tid == 0 && P.ban_sep && P.sep >= 0 && P.sep < V) row[P.sep] = ninf;
  for (int j = tid; j < P.n_ban; j += 256) {
    const int v = P.ban[j];
    if (v >= 0 && v < V) row[v] = ninf;
  }
}

extern "C" int fcmf_logits_constrain(void* logits, int64_t ld, int rows, int V, const int64_t* hist, int64_t hist_sr,
                                     int64_t hist_sp, int hist_len, float repetition_penalty, int no_repeat_ngram, int min_length,
                                     int sep_id, const int32_t* ban_ids, int n_ban, int dtype, void* stream) {
  if (!logits || !hist || rows < 0 || V < 1 || ld < V || hist_len < 1) return FCMF_ERR_ARG;
  if (!isfinite(repetition_penalty) || !(repetition_penalty > 0.f)) return FCMF_ERR_ARG;
  if (no_repeat_ngram < 0 || min_length < 0 || n_ban < 0 || (n_ban > 0 && !ban_ids)) return FCMF_ERR_ARG;
  if (dtype != FCMF_F32 && dtype != FCMF_BF16) return FCMF_ERR_UNSUPPORTED;
  if (hist_len > CONSTRAIN_MAX_T || n_ban > CONSTRAIN_MAX_BAN) return FCMF_ERR_UNSUPPORTED;
  const int ban_sep = min_length > 0 && hist_len < min_length;
  if (rows == 0 || (repetition_penalty == 1.f && no_repeat_ngram == 0 && !ban_sep && n_ban == 0)) return FCMF_OK;
  ConstrainK P{};
  P.x = logits; P.ld = ld; P.V = V; P.L = hist_len; P.hist = hist; P.sr = hist_sr; P.sp = hist_sp;
  P.theta = repetition_penalty; P.ngram = no_repeat_ngram; P.ban_sep = ban_sep; P.sep = sep_id; P.n_ban = n_ban; P.ban = ban_ids;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 g(rows), b(256);
  return dtype == FCMF_F32 ? fcmf_launch(logits_constrain_kernel<float>, g, b, 0, st, P)
                           : fcmf_launch(logits_constrain_kernel<bf16_t>, g, b, 0, st, P);
}
