/* fcmf_hip.h -- C ABI of libfcmf_hip.so: the MI355X (gfx950) kernels underneath the
 * `fcmf_framework` Python module surface.
 *
 * The reference (sonbui25/Multimodal-Aspect-Category-Sentiment-Analysis) has no FFI layer:
 * its operators are whatever torch dispatches from fcmf_framework/{mm_modeling,roi_modeling,
 * fcmf_pretraining,fcmf_multimodal,optimization}.py.  Each entry point below names the
 * reference code (file:line under /root/reference) whose arithmetic it replaces.
 *
 * Conventions
 *  - plain pointers + sizes only; every pointer is a DEVICE pointer unless stated otherwise;
 *  - `stream` is a hipStream_t passed as void*; all work is enqueued on it, nothing
 *    synchronises, nothing allocates (workspaces are caller-provided);
 *  - return value: 0 = FCMF_OK, negative = error (no exceptions cross the ABI);
 *  - dtype codes select the ACTIVATION storage type; master parameters, optimizer state,
 *    LayerNorm statistics, logsumexp and gradients of parameters are always float32.
 */
#ifndef FCMF_HIP_H
#define FCMF_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FCMF_OK 0
#define FCMF_ERR_ARG (-1)
#define FCMF_ERR_LAUNCH (-2)
#define FCMF_ERR_UNSUPPORTED (-3)
#define FCMF_ERR_COMM (-4)        /* RCCL unavailable or a collective call failed */

#define FCMF_F32 0
#define FCMF_BF16 1
#define FCMF_F64 2

/* GEMM epilogues */
#define FCMF_EPI_NONE 0   /* C = acc + bias                                            */
#define FCMF_EPI_GELU 1   /* C = gelu_erf(acc + bias); aux (if non-NULL) <- acc + bias  */
#define FCMF_EPI_TANH 2   /* C = tanh(acc + bias)                                       */
#define FCMF_EPI_DGELU 3  /* C = acc * gelu'(aux)      (aux = saved pre-activation)     */
#define FCMF_EPI_DTANH 4  /* C = acc * (1 - aux^2)     (aux = saved tanh output)        */
#define FCMF_EPI_ADD 5    /* C = acc + bias + aux      (residual-gradient accumulation)  */
/* the two below through fcmf_gemm_drop only; m(idx) = 1/(1-p) or 0: the counter-based dropout mask of fcmf_dropout */
#define FCMF_EPI_GELU_DROP 6   /* C = gelu_erf(acc + bias) * m(i*N + j); aux (if non-NULL) <- acc + bias, unmasked */
#define FCMF_EPI_DGELU_DROP 7  /* C = acc * gelu'(aux) * m(i*N + j)                                                */
/* eval-mode BatchNorm folded into a convolution: its scale lives in the weights, its shift is the bias (fcmf_gemm, fcmf_conv_gemm_epi;
 * fcmf_gemm_fp8 and fcmf_gemm_drop answer FCMF_ERR_UNSUPPORTED) */
#define FCMF_EPI_RELU 8        /* C = max(acc + bias, 0)                                      */
#define FCMF_EPI_ADD_RELU 9    /* C = max(acc + bias + aux, 0)  (aux = the block's identity)   */

int fcmf_abi_version(void);
/* human-readable "gfx950 ..." build string (host pointer, static storage) */
const char* fcmf_build_info(void);

/* ---------------------------------------------------------------------------------------
 * GEMM context: everything fcmf_gemm uses beyond its arguments.  The library keeps NO mutable process-global state; a
 * context is owned by the caller and used by one host thread / one stream at a time (the Python layer keeps one per
 * (device, stream)).  NULL is a valid context: defaults, no split-K workspace.
 *   set_workspace: caller-owned DEVICE scratch for the k-split partial tiles of weight-gradient GEMMs (accumulate != 0):
 *                  with at least ksplit*M*N*4 bytes the partials are written with plain stores and summed by a reduce
 *                  pass (5x cheaper than 65 536 float atomics per CU); without it, or when it is too small, float
 *                  atomics.  The buffer must stay valid until the stream has drained.  ptr = NULL unregisters.
 *   tune         : benchmark / test knobs; a negative value keeps the current setting.
 *                  force_tile 0 = built-in heuristic, 128 = 128x128 kernel, 256 / 192 = persistent 256x256 / 192x256 kernel
 *                  wherever its preconditions hold; kb 32 / 64 = depth of the k-tiles of the K-contiguous persistent kernels
 *                  (both depths issue the same MFMAs in the same order: bit-identical results); num_cus = workgroups of
 *                  the persistent kernels (8..256; leaves CUs to kernels that run beside them, e.g. RCCL);
 *                  nt_min_bytes = bf16 outputs of at least this size leave with nontemporal stores (default 0 = all).
 *   last_kernel  : name of the kernel the context's last fcmf_gemm dispatched, e.g.
 *                  "gemm_bf16_tile256_kernel<0,1,bf16,GELU>" (benchmarks attribute launch time by it; host string owned
 *                  by the context). */
typedef struct fcmf_gemm_ctx fcmf_gemm_ctx;
int fcmf_gemm_ctx_create(fcmf_gemm_ctx** ctx);
int fcmf_gemm_ctx_destroy(fcmf_gemm_ctx* ctx);
int fcmf_gemm_ctx_set_workspace(fcmf_gemm_ctx* ctx, void* ptr, int64_t bytes);
int fcmf_gemm_ctx_tune(fcmf_gemm_ctx* ctx, int force_tile, int kb, int num_cus, int64_t nt_min_bytes);
const char* fcmf_gemm_ctx_last_kernel(const fcmf_gemm_ctx* ctx);

/* ---------------------------------------------------------------------------------------
 * GEMM:  C[M,N] (+)= epilogue( op(A)[M,K] * op(B)[K,N] + bias[N] )
 *   ctx: GEMM context (above) or NULL.
 *   trans_a = 0: A stored [M,K] (row stride lda)      trans_a = 1: A stored [K,M]
 *   trans_b = 0: B stored [N,K] (nn.Linear weight)    trans_b = 1: B stored [K,N]
 *   in_dtype: dtype of A and B; out_dtype: dtype of C and aux; bias is float32 or NULL.
 *   accumulate != 0 (out_dtype must be F32): C += result (k-split partials go through the context's workspace, or are
 *   added with float atomics when there is none -- C must be initialised either way).
 *   colsum (float32 [N], may be NULL; not with accumulate): colsum[n] += sum_m C[m,n] -- the bias
 *   gradient of the layer that produced the operand, fused into the epilogue.
 * Replaces nn.Linear forward/backward everywhere on the path: mm_modeling.py:182-184,
 * 229-231,272,308,320,422 ; fcmf_pretraining.py:25-26 ; roi_modeling.py:73 ;
 * fcmf_multimodal.py:18 and their autograd (dX = dY*W, dW = dY^T*X).
 * bf16 inputs whose contiguous dimensions are multiples of 8 elements with 16-byte aligned
 * bases run on the MFMA bf16 kernel; everything else runs on the generic f32-MFMA kernel. */
int fcmf_gemm(fcmf_gemm_ctx* ctx, const void* A, const void* B, void* C, const float* bias, void* aux, float* colsum,
              int M, int N, int K, int64_t lda, int64_t ldb, int64_t ldc,
              int trans_a, int trans_b, int in_dtype, int out_dtype,
              int epilogue, int accumulate, void* stream);

/* ---------------------------------------------------------------------------------------
 * GEMM with the feed-forward dropout of nn.TransformerEncoderLayer in its epilogue: linear2(dropout(gelu(linear1(x)))) and its
 * backward without a pass of their own over the [M, N] activation.  Arguments as fcmf_gemm (no `accumulate`: C is written);
 * epilogue is FCMF_EPI_GELU_DROP (forward) or FCMF_EPI_DGELU_DROP (backward: aux = the pre-activation the forward wrote,
 * required), anything else is FCMF_ERR_ARG, as is dropout_p outside (0, 1).
 *   mask: element (i, j) of the LOGICAL [M, N] output (row-major index i*N + j, 64-bit, whatever ldc is) is multiplied by
 *         dropout_mult(seed, i*N + j, p, 1/(1-p)) -- the mask fcmf_dropout applies to a contiguous [M, N] tensor with the same
 *         seed -- so both epilogues of one layer regenerate the same mask from (seed, p) and nothing is stored for it.  A dropped
 *         element is an exact zero; a kept bf16 value is rounded once, after the scaling.
 *   aux of GELU_DROP is the unmasked pre-activation (gelu' needs it); colsum sums the values as stored, after the mask.
 * Kernels: the generic f32-MFMA kernel (exact erf forms), the 128x128 bf16 kernel and the persistent 256 / 192-row bf16
 * kernels at both k-tile depths (transposed A: the 128x128 kernel); never the 64x64 kernel.  fcmf_gemm_fp8 answers
 * FCMF_ERR_UNSUPPORTED for the two epilogues: in fp8 mode these two GEMMs stay bf16. */
int fcmf_gemm_drop(fcmf_gemm_ctx* ctx, const void* A, const void* B, void* C, const float* bias, void* aux, float* colsum,
                   int M, int N, int K, int64_t lda, int64_t ldb, int64_t ldc,
                   int trans_a, int trans_b, int in_dtype, int out_dtype,
                   int epilogue, float dropout_p, uint64_t seed, void* stream);

/* ---------------------------------------------------------------------------------------
 * FP8 (OCP e4m3fn) path of BASELINE configs[4] (FCMF-large): forward and dX GEMMs on the block-scaled matrix instruction
 * v_mfma_scale_f32_16x16x128_f8f6f4 (2x the bf16 MFMA rate), float32 accumulation; weight gradients stay bf16.
 * The only "large" hook of the reference is the constant block of mm_modeling.py:21-30; the arithmetic replaced is the
 * same nn.Linear forward / dX as fcmf_gemm.
 *   fcmf_quant_fp8_rows: x [rows, K] (FCMF_BF16 / FCMF_F32, row stride ldx elements) -> q [rows, K] e4m3 bytes (row stride
 *       ldq bytes) with one dequantisation scale per row: scale[r] = max|x[r, :]| / 448 (1 for a zero row),
 *       q = rne(x / scale[r]).  K, ldx, ldq multiples of 8.
 *   fcmf_gemm_fp8: C[M,N] bf16 = epilogue( (A_q[M,K] * B_q[N,K]^T) * sa[m] * sb[n] + bias[n] ); both operands K-contiguous
 *       e4m3 with their row scales (A: activations / output gradients quantised per token; B: the weight quantised per output
 *       row -- or its transposed copy per input row for dX).  Epilogues NONE / GELU / DGELU / ADD, aux and colsum as in
 *       fcmf_gemm.  K % 128 == 0, lda / ldb % 16 == 0 (bytes), N and ldc % 8 == 0, M, N >= 256: otherwise
 *       FCMF_ERR_UNSUPPORTED (the caller keeps the bf16 path). */
int fcmf_quant_fp8_rows(const void* x, int64_t ldx, void* q, int64_t ldq, float* scale, int rows, int K, int dtype, void* stream);
int fcmf_gemm_fp8(fcmf_gemm_ctx* ctx, const void* A, const float* sa, const void* B, const float* sb, void* C,
                  const float* bias, void* aux, float* colsum, int M, int N, int K, int64_t lda, int64_t ldb, int64_t ldc,
                  int epilogue, void* stream);

/* column sums: out[n] (+)= sum_m X[m,n]  (bias gradients).  X dtype = dtype, out float32. */
int fcmf_colsum(const void* X, float* out, int M, int N, int64_t ldx, int dtype,
                int accumulate, void* stream);

/* ---------------------------------------------------------------------------------------
 * Two-segment multi-head attention (VALU, any dtype).  One "group" g has R query rows; every
 * row attends to T1 keys shared by the group (K1/V1) followed by T2 keys private to the row
 * (K2/V2, indexed by g / group_div so that several groups can share the private segment).
 *   score[t] = scale * <q, k_t> + mask[g, t] + bias[g / group_div, h, r, t]
 *   causal != 0: score[t] = -1e4 where t > r   (IAOG `Attention`, mm_modeling.py:115-124)
 *   p = dropout(softmax(score)); out = sum_t p[t] v_t ; lse[g,h,r] = logsumexp(score)
 * Dropout (dropout_p > 0) is a stateless function of (seed, counter), so the backward regenerates the forward's mask.  The
 * counter of probability (g, h, r, t) is its row-major element index in the [G, heads, R, T1+T2] probability tensor,
 *   idx = ((g*heads + h)*R + r)*(T1+T2) + t            (t counts the shared keys first, then the private ones)
 * and in the MFMA kernels below idx = ((g*heads + h)*Tq + q)*Tk + key with g the QUERY group (also under kv_share > 1).
 * One 32-bit hash of (seed, idx >> 1) decides a pair of elements: its low 16 bits the even one, its high 16 bits the odd
 * one; an element is kept iff its 16 bits >= (uint32_t)(dropout_p * 65536 + 0.5) (float32 arithmetic), and kept
 * probabilities are multiplied by the float32 1 / (1 - dropout_p).  The hash is fcmf_hash32 of csrc/common.h;
 * tests/rowwise_ref.py (dropout_mask, mask_tensor, inv_keep) is the executable statement of all of this, and
 * tests/attn_ref.py the attention under it.
 * Layouts (elements): Q  (g,r,h,:) at q  + g*q_sg  + r*q_sr  + h*d
 *                     K1 (g,t,h,:) at k1 + g*k1_sg + t*k1_st + h*d          (V1 same strides)
 *                     K2 (g2,r,t,h,:) at k2 + g2*k2_sg + r*k2_sr + t*k2_st + h*d  (V2 same)
 *                     O  (g,r,h,:) at o  + g*o_sg  + r*o_sr  + h*d          (dO same)
 * head_quirk != 0 reproduces mm_modeling.py:79-85: output slot h of group g READS Q/K/V head
 * (h*G + g) % heads; the backward WRITES dq/dk/dv at slot h (several slots may read one head, so
 * the caller scatter-adds slots back to heads).
 * Replaces BertSelfAttention/BertCoAttention (mm_modeling.py:193-219,240-266), HF
 * eager_attention_forward, box_attention (roi_modeling.py:14-47) and Attention
 * (mm_modeling.py:66-132). */
typedef struct {
  int dtype, G, heads, d, R, T1, T2, group_div;
  int64_t q_sg, q_sr, k1_sg, k1_st, k2_sg, k2_sr, k2_st, o_sg, o_sr;
  const void *q, *k1, *v1, *k2, *v2;
  const float* mask;   /* [G, T1+T2] additive or NULL */
  const float* bias;   /* [G/group_div, heads, R, T1+T2] additive or NULL */
  float scale, dropout_p;
  uint64_t seed;
  int causal, head_quirk;
} fcmf_attn_desc;

int fcmf_attn_small_fwd(const fcmf_attn_desc* desc /*host*/, void* out, float* lse, void* stream);
/* Gradients are written DENSE (independent of the input strides) and fully overwritten:
 *   dq  [ceil(T1/128) or 1, G, R, heads*d] -- one partial per 128-key chunk of the shared segment;
 *       the caller sums the leading axis (fcmf_sum_axis);
 *   dk1/dv1 [G, T1, heads*d];   dk2/dv2 [G, R, T2, heads*d] (indexed by g, NOT g/group_div: the
 *       caller sums groups that share a private segment);
 *   dbias (float32, may be NULL) [G, heads, R, T1+T2].
 * When v1 == k1 (IAOG) pass dv1 = NULL: dk1 receives both terms.  Limits: T1+T2 <= 512, T2 <= 128,
 * d <= 128 (FCMF-large: 256 text keys + 100 ROI keys in the shared mm_attention layer). */
int fcmf_attn_small_bwd(const fcmf_attn_desc* desc /*host*/, const void* out, const void* dout,
                        const float* lse, void* dq, void* dk1, void* dv1, void* dk2, void* dv2,
                        float* dbias, void* stream);
/* The same backward where the `group_div` consecutive groups that share private keys (the six aspects of a review:
 * fcmf_multimodal.py:84-124 under aspect batching) also share their gradients: dk2 / dv2 are
 * [G/group_div, R, T2, heads*d], already summed over the group.  scratch: caller-owned device memory,
 * >= 2*G*heads*R*T2*4 bytes (the private keys' probabilities and score gradients between the two kernels).
 * group_div <= 8, G % group_div == 0, no head_quirk; FCMF_ERR_UNSUPPORTED otherwise (use fcmf_attn_small_bwd and sum). */
int fcmf_attn_small_bwd_grouped(const fcmf_attn_desc* desc, const void* out, const void* dout,
                                const float* lse, void* dq, void* dk1, void* dv1, void* dk2, void* dv2,
                                float* dbias, float* scratch, int64_t scratch_bytes, void* stream);
/* What the three entry points above would launch for a descriptor, without a device (host only: nothing is launched, no
 * pointer is read; tests, tools and the Python layer's key limit).  backward / grouped select the entry point; has_dbias /
 * has_dv1: dbias / dv1 non-NULL; ptrs_aligned: the call's output and gradient pointers (out; out, dout, dq, dk1, dv1) are all
 * 16-byte aligned.  Returns what the entry point would (its NULL-argument and scratch-size checks aside).  info[11] = kernel id,
 * grid x, grid y, dynamic LDS bytes, RB (query rows staged per block), TLP, KVF (floats: pitch of the backward's key arrays,
 * size of the shared K + V images), then the attn_private_grad_kernel launch behind a grouped backward: kernel id (-1 = none),
 * grid x, grid y, dynamic LDS bytes; kernel id -1 and zeros unless FCMF_OK.  Every launch has 256 threads per workgroup.
 * kernels (host, may be NULL): [2] names of the two kernels (static storage; NULL where there is none). */
int fcmf_attn_small_plan(const fcmf_attn_desc* desc /*host*/, int backward, int grouped, int has_dbias, int has_dv1, int ptrs_aligned,
                         int32_t* info /*host*/, const char** kernels /*host*/);

/* ---------------------------------------------------------------------------------------
 * MFMA self/cross attention for bf16, head dim 64, Tq, Tk <= 256 (the text-encoder layers: 128 tokens in FCMF-base,
 * 256 in FCMF-large; the backward handles every query of a (sequence, head) in one workgroup, so Tq <= 256 there too):
 *   Q [G,Tq,heads*64], K/V [G,Tk,heads*64] (row strides ldq/ldk elements), mask [G,Tk] additive.
 * Replaces HF RobertaSelfAttention + eager_attention_forward and mm_modeling.py:193-219. */
int fcmf_attn_mfma_fwd(const void* q, const void* k, const void* v, const float* mask,
                       void* out, float* lse, int G, int heads, int Tq, int Tk,
                       int64_t ldq, int64_t ldk, int64_t ldo, float scale,
                       float dropout_p, uint64_t seed, void* stream);
int fcmf_attn_mfma_bwd(const void* q, const void* k, const void* v, const float* mask,
                       const void* out, const void* dout, const float* lse,
                       void* dq, void* dk, void* dv, int G, int heads, int Tq, int Tk,
                       int64_t ldq, int64_t ldk, int64_t ldo, float scale,
                       float dropout_p, uint64_t seed, float* colsum, void* stream);
/* colsum (may be NULL): float32 [G][3*heads*64]; row g receives the column sums of sequence g's dq | dk | dv (taken from
 * the f32 accumulators).  Their sum over g is the bias gradient of a fused q|k|v projection (the autograd of
 * mm_modeling.py:182-184 / HF RobertaSelfAttention's three nn.Linear biases) without another pass over dqkv. */

/* ---------------------------------------------------------------------------------------
 * MFMA attention with any number of keys and a key/value set shared by consecutive query groups: bf16, head dim 64,
 * Tq <= 256, 1 <= Tk <= 2^20 (FCMF_ERR_UNSUPPORTED beyond).  The cross-attention of the comparison baselines (mRoBERTa,
 * TomBERT): the text queries of the `kv_share` aspect prompts of a review attend to all of its visual tokens.
 *   Q [G,Tq,heads*64]; K/V [G/kv_share,Tk,heads*64], group g reads key set g / kv_share (G % kv_share == 0);
 *   mask [G,Tk] additive float32 or NULL; out [G,Tq,heads*64]; lse [G,heads,Tq].
 * Semantics, row strides and alignment rules are those of fcmf_attn_mfma_fwd / _bwd: softmax(scale QK^T + mask) with the
 * mask added in float32 (a finfo.min key gets probability exactly 0; a row whose every key is masked is uniform over all
 * Tk keys), dropout on the probabilities with the same counter function of (seed, group, head, query, key) (stated at fcmf_attn_desc), then V.
 * Backward: dq [G,Tq,.]; dk / dv [G/kv_share,Tk,.] are the sums over the sharing groups, accumulated in float32 and rounded
 * to bf16 once.  kv_share > 1 needs `workspace`: caller-owned device memory of at least
 * 2 * (G/kv_share) * Tk * heads*64 * 4 bytes, 16-byte aligned (contents need not be initialised; FCMF_ERR_ARG if too small). */
int fcmf_attn_mfma_long_fwd(const void* q, const void* k, const void* v, const float* mask,
                            void* out, float* lse, int G, int heads, int Tq, int Tk, int kv_share,
                            int64_t ldq, int64_t ldk, int64_t ldo, float scale,
                            float dropout_p, uint64_t seed, void* stream);
int fcmf_attn_mfma_long_bwd(const void* q, const void* k, const void* v, const float* mask,
                            const void* out, const void* dout, const float* lse,
                            void* dq, void* dk, void* dv, int G, int heads, int Tq, int Tk, int kv_share,
                            int64_t ldq, int64_t ldk, int64_t ldo, float scale,
                            float dropout_p, uint64_t seed, float* workspace, int64_t workspace_bytes, void* stream);
/* The probabilities of that attention as float32, BEFORE dropout: softmax(scale QK^T + mask) with exactly the score and
 * mask semantics above (a finfo.min key gets probability exactly 0; a group without a live key is uniform over all Tk keys).
 * Same operands and limits as fcmf_attn_mfma_long_fwd without V (bf16, head dim 64, Tq <= 256, 1 <= Tk <= 2^20, ldq / ldk
 * multiples of 8, 16-byte aligned q / k); no logsumexp of a forward is needed, the kernel finds each row's maximum and sum.
 *   head_mean == 0: probs [G, heads, Tq, Tk];
 *   head_mean != 0: probs [G, Tq, Tk] = (1/heads) * sum_h P_h (torch's average_attn_weights), heads <= 32.  The heads are
 *                   summed in float32 in ascending order inside the kernel: no per-head tensor exists in memory, there are no
 *                   atomics, every element is stored exactly once -- two launches on the same operands agree bit for bit.
 * probs is dense and need not be initialised: every element is written, those of skipped (all hard-masked) key tiles too. */
int fcmf_attn_mfma_long_probs(const void* q, const void* k, const float* mask, float* probs, int G, int heads,
                              int Tq, int Tk, int kv_share, int64_t ldq, int64_t ldk, float scale, int head_mean,
                              void* stream);

/* ---------------------------------------------------------------------------------------
 * Attention probabilities on request: P = softmax(score) as float32, BEFORE dropout, recomputed from Q and K with exactly the
 * score definition of fcmf_attn_desc above (the forward kernels never materialise P).  Both entry points find the row maximum
 * and sum themselves (no lse of a forward is needed); a row whose every key carries the finfo(float32).min mask comes out
 * uniform, 1/T, as in the forward kernels and in torch.
 * Output element (g, slot h, r, t) at probs + g*p_sg + h*p_sh + r*T + t (elements), so one kernel writes either layout:
 *   [G, heads, R, T]: p_sg = heads*R*T, p_sh = R*T   (HF `output_attentions`: one [B, heads, S, S] tensor per text-encoder layer,
 *                     mm_modeling.py:440-446 -> fcmf_pretraining.py:41);
 *   [heads*G, R, T] : p_sg = R*T, p_sh = G*R*T       (index h*G + g: the `score` the IAOG `Attention` returns and keeps as
 *                     attention_weights, mm_modeling.py:126-132, in the order of its torch.split(output, mb_size, dim=0)).
 * fcmf_attn_probs: VALU, FCMF_F32 / FCMF_BF16; reads desc->q / k1 / k2 with their strides (a query row stride of 0 included),
 *   mask, bias, group_div, causal and head_quirk; IGNORES v1, v2, dropout_p, seed and the o_* strides.  Limits as
 *   fcmf_attn_small_bwd: T1+T2 <= 512, T2 <= 128, d <= 128, FCMF_ERR_UNSUPPORTED outside them.
 * fcmf_attn_mfma_probs: bf16, head dim 64, Tq, Tk <= 256; q / k rows as fcmf_attn_mfma_fwd reads them (row strides ldq / ldk:
 *   the fused layers' [rows, 3*H] q|k|v buffer is read in place), mask [G, Tk] additive or NULL.  Same alignment rules as
 *   fcmf_attn_mfma_fwd (ldq, ldk multiples of 8, 16-byte aligned q / k), FCMF_ERR_UNSUPPORTED otherwise. */
int fcmf_attn_probs(const fcmf_attn_desc* desc /*host*/, float* probs, int64_t p_sg, int64_t p_sh, void* stream);
int fcmf_attn_mfma_probs(const void* q, const void* k, const float* mask, float* probs, int G, int heads,
                         int Tq, int Tk, int64_t ldq, int64_t ldk, int64_t p_sg, int64_t p_sh,
                         float scale, void* stream);

/* ---------------------------------------------------------------------------------------
 * BERTScore greedy matching (Zhang et al. 2020 with idf = False, rescale_with_baseline = False: what the reference's
 * `bert_score.score(preds, refs, ...)` computes from the scorer model's token embeddings, run_pretraining_fcmf.py:434,575).
 * One launch scores N (candidate, reference) pairs:
 *   s[i][j] = <c_i, r_j> / (|c_i| |r_j|)                      over the valid rows i < cand_len[n], j < ref_len[n] only
 *   P = sum_i wc[i] max_j s[i][j] / sum_i wc[i]     R = sum_j wr[j] max_i s[i][j] / sum_j wr[j]     F = 2 P R / (P + R)
 *   cand [N, Lc_max, H], ref [N, Lr_max, H] in `dtype` (FCMF_F32 / FCMF_BF16): row i of pair n at cand + n*sc + i*ldc (elements);
 *   cand_len, ref_len int32 [N] in DEVICE memory (the host cannot see them: the kernel clamps each to [0, L*_max]); rows at or
 *   beyond a pair's length are never read and may hold anything;
 *   cand_w, ref_w float32 [N, L*_max] dense per-token weights, or NULL = 1 for every valid token.  A token of weight 0 (<s>, </s>)
 *   still is a match target of the other side;   out float32 [N, 3] = P, R, F.
 * P = R = F = 0 (never NaN / inf) when either length is 0 or either weight sum is 0; F = 0 when P + R = 0.  An all-zero row has
 * similarity 0 to everything.
 * Dot products and norms accumulate in float32; bf16 rows go to the MFMA as stored (products exact) and the accumulator is divided
 * by the float32 norms afterwards; FCMF_F32 takes a VALU path.  Fixed-order reductions, no atomics: two launches on the same inputs
 * give the same bits.
 * Limits: Lc_max, Lr_max <= 512; H % 8 == 0; 16-byte aligned cand / ref and strides that keep every row 16-byte aligned --
 * FCMF_ERR_UNSUPPORTED otherwise; negative sizes / strides and NULL cand, ref, lengths or out are FCMF_ERR_ARG. */
int fcmf_bertscore(const void* cand, const void* ref, const int* cand_len, const int* ref_len, const float* cand_w,
                   const float* ref_w, float* out, int N, int Lc_max, int Lr_max, int H, int64_t ldc, int64_t sc,
                   int64_t ldr, int64_t sr, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------
 * log-softmax + top-k of the rows of a logits matrix, one launch: the tail of an IAOG decode step (the reference's
 * `log_softmax(logits)` + `topk(beam_size)`, fcmf_pretraining.py:476-480), for `rows` independent rows at once.
 *   logits [rows, ld] in `dtype` (FCMF_F32 / FCMF_BF16), row r at logits + r*ld (elements); only columns 0 .. V-1 are ever
 *   loaded (ld >= V: the column padding 64001 -> 64032 of the bf16 vocabulary projection may hold anything, NaN included);
 *   lse[r] = log sum_{j<V} exp(x[r,j]), float32, the row maximum subtracted;
 *   ids  int32   [rows, k]: the columns of the k largest entries of the row, by stored value descending, the LOWER column first
 *                among equal values (= a stable descending sort of the row).  The selection compares stored values, so it
 *                carries no rounding;
 *   logp float32 [rows, k]: x[r, ids] - lse[r].  An entry -inf has log-probability -inf and sorts last.
 * A row of only -inf, or one holding NaN, is undefined (as for torch).  Fixed-order reductions, no atomics: two launches give
 * the same bits.  Rows that are 16-byte aligned (logits and ld * element size multiples of 16) are read 16 bytes per lane,
 * any other layout one element per lane.
 * Limits: 1 <= k <= 16, k <= V, dtype FCMF_F32 / FCMF_BF16 -- FCMF_ERR_UNSUPPORTED otherwise; NULL pointers, rows < 0 or ld < V
 * are FCMF_ERR_ARG; rows == 0 succeeds without a launch. */
int fcmf_logsoftmax_topk(const void* logits, int64_t ld, int rows, int V, int k, float* logp, int32_t* ids, int dtype,
                         void* stream);

/* ---------------------------------------------------------------------------------------
 * One sampled token per row of a logits matrix, one launch: the sampling tail of an IAOG decode step, beside the beam tail above
 * (temperature, top-k and nucleus filtering in the order and with the tie rules of Hugging Face's TopKLogitsWarper /
 * TopPLogitsWarper, then a Gumbel-max draw), for `rows` independent rows at once.
 *   logits [rows, ld] in `dtype` (FCMF_F32 / FCMF_BF16), row r at logits + r*ld (elements); only columns 0 .. V-1 are ever
 *   loaded (the column padding and any guard band may hold anything, NaN included).  For a row r, x_j its stored values:
 *   K  (top-k)   every column when top_k == 0 or top_k >= V; else { j : x_j >= v }, v the top_k-th largest stored value of the
 *                row: ties at v are ALL kept.  The comparison is on stored values and carries no rounding (-0 equals +0);
 *   z_j = x_j / temperature for j in K, p = softmax of z over K;
 *   N  (nucleus) j in N iff M(x_j) < top_p, M(v) = sum of p_i over the i in K with x_i > v, the mass STRICTLY above the value:
 *                ties stand or fall together, the row maximum is always kept, top_p == 1 keeps all of K;
 *   ids  int32   [rows]: argmax over j in N of z_j + g_j, the LOWER column on an exact tie; g_j = -log(-log(u_j)),
 *                u_j = ((h_j >> 9) + 0.5) * 2^-23 (exact in float32, never 0 or 1), h_j = fcmf_hash32(seed, ((ctr[r] & (2^44 - 1))
 *                << 20) | j), the hash of csrc/common.h.  A column holding -inf is never drawn;
 *   logp float32 [rows]: x[r, ids[r]] - lse[r], lse[r] = log sum_{j<V} exp(x[r,j]): the draw's log-probability under the model's
 *                own distribution (temperature 1, unfiltered) -- fcmf_logsoftmax_topk's definition, so that the score of a sampled
 *                chain is comparable with a beam's.  The log-probability under the filtered distribution is not returned.
 * ctr int64 [rows] on the device: a row's draw depends on (seed, ctr[r]) and its logits only -- not on its row index nor on the
 * other rows of the launch.  A row of only -inf, or one holding NaN inside V, is undefined.  No floating-point atomics,
 * fixed-order reductions (the nucleus masses are integer sums): two launches give the same bits.  Rows that are 16-byte aligned
 * are read 16 bytes per lane, any other layout one element per lane.
 * Limits: 1 <= V <= 2^20, dtype FCMF_F32 / FCMF_BF16 -- FCMF_ERR_UNSUPPORTED otherwise; temperature finite and > 0, top_k >= 0,
 * 0 < top_p <= 1, no NULL pointer, rows >= 0, ld >= V -- FCMF_ERR_ARG otherwise; rows == 0 succeeds without a launch. */
int fcmf_sample_token(const void* logits, int64_t ld, int rows, int V, float temperature, int top_k, float top_p, uint64_t seed,
                      const int64_t* ctr, int32_t* ids, float* logp, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------
 * Generation constraints on the logits of a decode step, in place, one launch for `rows` independent rows: repetition penalty,
 * no-repeat n-gram bans, a minimum length and always-suppressed ids (the rules of Hugging Face's RepetitionPenaltyLogitsProcessor,
 * NoRepeatNGramLogitsProcessor, MinLengthLogitsProcessor and SuppressTokensLogitsProcessor).
 * The edit is made on the LOGITS, before fcmf_logsoftmax_topk / fcmf_sample_token: the constrained logits ARE the step's
 * distribution.  The log-probabilities those return, beam and chain scores, temperature, top-k and top-p all see them; a banned
 * token has log-probability -inf and the mass is renormalised over the rest.  (Hugging Face's beam search applies its processors
 * after the log-softmax instead; one definition for both strategies keeps a chain's score and a beam's the same quantity.)
 *   logits [rows, ld] in `dtype` (FCMF_F32 / FCMF_BF16), row r at logits + r*ld (elements); only columns 0 .. V-1 are touched.
 *   hist   int64 on the device: the sequence of row r is h[p] = hist[r*hist_sr + p*hist_sp], p = 0 .. L-1, L = hist_len: the start
 *          token first, the token the step was run on last.  All rows of a call have the same L.  Entries are vocabulary ids and
 *          are held as int: a value beyond int is out of range like any other and equals only other such values.
 * Per row, x its stored values, in this order:
 *   1. repetition penalty theta (finite, > 0; 1 = off): for every DISTINCT v among h[0 .. L-1] with 0 <= v < V,
 *      x[v] <- x[v] < 0 ? x[v] * theta : x[v] / theta, in float32 with a correctly rounded divide, rounded once to nearest-even
 *      into the storage type.  A token that occurs five times is penalised once;
 *   2. no_repeat_ngram n (0 = off): for every i in 0 .. L-n with h[i .. i+n-2] == h[L-n+1 .. L-1]: x[h[i+n-1]] <- -inf.  n = 1 bans
 *      every token of the sequence, L < n bans nothing;
 *   3. min_length m (0 = off): if L < m, x[sep_id] <- -inf (L is the length penalty's len(seq) - 1 of the resulting sequence);
 *   4. x[ban_ids[j]] <- -inf for j < n_ban; ban_ids int32 on the device, or NULL with n_ban == 0.
 * A ban wins over a penalty on the same column.  An id outside [0, V) -- from hist, sep_id or ban_ids -- writes nothing.  Every
 * other column, every column >= V and every byte outside the rows keep their bits (bf16 columns are 2-byte stores).  No atomics,
 * one rounding: two launches give the same bits.
 * Limits: hist_len <= 512, n_ban <= 1024, dtype FCMF_F32 / FCMF_BF16 -- FCMF_ERR_UNSUPPORTED otherwise; logits and hist not
 * NULL, rows >= 0, 1 <= V <= ld, hist_len >= 1, theta finite and > 0, no_repeat_ngram / min_length / n_ban >= 0, ban_ids not NULL when n_ban > 0
 * -- FCMF_ERR_ARG otherwise; rows == 0, or nothing to do (theta == 1, n == 0, L >= m, n_ban == 0), succeeds without a launch. */
int fcmf_logits_constrain(void* logits, int64_t ld, int rows, int V, const int64_t* hist, int64_t hist_sr, int64_t hist_sp,
                          int hist_len, float repetition_penalty, int no_repeat_ngram, int min_length, int sep_id,
                          const int32_t* ban_ids, int n_ban, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------
 * Single-query attention with indexed keys, one launch for n rows x `heads` slots: the two attentions of an IAOG decode step
 * that sees its whole prefix (the decoder `Attention` of mm_modeling.py:66-132 for ONE query row per sequence: values are the
 * projected keys :129, plain slot -> head pairing, which is the reference's at batch size 1).  All strides in elements.
 *   q     [n, heads*d] in `dtype`, row r at q + r*q_sr (q_sr may exceed heads*d: the query half of a [kx | qx] buffer);
 *   keys  the key of position p for row r is the heads*d elements at keys + p*k_sp + idx[r*idx_sr + p*idx_sp]*k_si, int64 idx:
 *           - a self-attention cache [Tmax, rows, heads*d] (k_sp, k_si = its strides) with idx the row's ancestor table
 *             [n, >= T]: which cache row held position p of this row's sequence;
 *           - hoisted encoder keys [samples, Tk, heads*d] (k_si, k_sp = its strides) with idx the row's sample index and
 *             idx_sp = 0 -- no [n, Tk, heads*d] gather per block and step;
 *         idx_n = the extent of the indexed axis: an index outside [0, idx_n) reads nothing and makes that row's output NaN;
 *   score_p = scale * <q[r, h], key_p[h]> for p < live and EXACTLY -1e4 for live <= p < T -- the reference's masked_fill
 *         (:115-124): a filled key still takes part in the softmax and in the sum, it is not excluded;
 *   out[r, h*d + j] = sum_{p < T} softmax(score)_p * key_p[h*d + j], row r at out + r*o_sr, in `dtype`; float32 accumulation.
 *   Append (k_new != NULL): row r's own key, position append_at, is k_new + r*kn_sr.  The kernel uses it from there -- neither
 *         the cache nor idx is read at position append_at -- and stores it to keys + append_at*k_sp + r*k_si.  No other element
 *         of `keys` is written, and the launch never loads position append_at, so there is no hazard inside a launch whatever
 *         the ancestor tables hold.  idx may be NULL when T == 1 (the appended key is the only one).
 * One wave per (row, slot), keys straight to registers with 16-byte loads, in-wave shuffles, no LDS, no atomics: two launches
 * give the same bits.
 * Limits: d a multiple of 8 in 8 .. 128, 1 <= T <= 512, FCMF_F32 / FCMF_BF16 -- FCMF_ERR_UNSUPPORTED otherwise.  q, keys, k_new,
 * out and every stride of theirs must be multiples of 16 bytes; 0 <= live <= T; with k_new 0 <= append_at < T and n <= idx_n --
 * FCMF_ERR_ARG otherwise.  n == 0 succeeds without a launch.  The caller guarantees that T positions exist behind `keys`. */
int fcmf_attn_decode(const void* q, int64_t q_sr, void* keys, int64_t k_sp, int64_t k_si, const int64_t* idx, int64_t idx_sr,
                     int64_t idx_sp, int64_t idx_n, const void* k_new, int64_t kn_sr, int append_at, void* out, int64_t o_sr,
                     int n, int heads, int d, int T, int live, float scale, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------
 * Beam bookkeeping of an IAOG decode on the device: round t of the beam search (decoding._advance and the rules of
 * decoding.beam_rounds around it) for B samples in one launch, on state that stays on the device from the start token to the
 * final hypotheses.  R = B * W rows; slot r = b*W + j is beam j of sample b, W = the beam size.
 * State (all on the device, allocated and initialised by the caller: see decoding.beam_rounds_device):
 *   seq    int64 [max_len + 1, R], position-major: seq[p*R + r] is token p of slot r.  seq + t*R is the contiguous token vector of
 *          round t; (seq, row stride 1, position stride R) is the [R, t + 1] history fcmf_logits_constrain takes.  Initially
 *          seq[0, :] = the start token in EVERY slot;
 *   anc    int64 [max_len, R], position-major: anc[p*R + r] is the slot that ran position p of slot r's sequence in round p -- the
 *          [R, t] ancestor table of fcmf_attn_decode (idx_sr = 1, idx_sp = R, idx_n = R) over a key cache of R rows;
 *   score  float64 [R], initially 0;
 *   state  int32 [R]: 0 empty, 1 live, 2 ended (the last token is sep_id and the slot is still among the beams).  Initially slot
 *          b*W is live and the other W - 1 slots of the sample are empty;
 *   fin_*  the finished list of sample b, entries e = 0 .. fin_count[b] - 1 in the host's append order: fin_score float64
 *          [B, cap], fin_len int32 [B, cap] (tokens, the start token included), fin_seq int64 [B, cap, max_len + 1] (the first
 *          fin_len entries), fin_count int32 [B] initially 0.  cap = W * (max_len + 1): a round appends at most the W ended beams
 *          of its input, the round that finishes the sample at most W more, and there are at most max_len rounds -- so
 *          beam_rounds' `final` never holds more than W * max_len + W entries;
 *   done   int32 [B], initially 0.
 * Inputs: logp float32 / ids int32 [R, >= W], row r at logp + r*ld / ids + r*ld (elements): fcmf_logsoftmax_topk's outputs of
 * the step run on seq[t] (k >= W).  Per sample b with done[b] == 0, in this order:
 *   1. every ended beam is appended to the finished list, in beam order, with its score and length t + 1, and gives no
 *      candidates;
 *   2. the candidates are, for every live beam j ascending and k = 0 .. W-1 ascending, (score[j] + (double)logp[j, k], ids[j, k]);
 *   3. no candidates: done[b] = 1, score / state / history of the slots stay as they are;
 *   4. the W best candidates by score descending, STABLE: among equal scores the earlier candidate wins (a live beam gives W
 *      candidates, so there are always W).  -inf compares as doubles do; NaN is undefined, as in fcmf_logsoftmax_topk;
 *   5. candidate i of that order becomes slot b*W + i: seq[0 .. t] and anc[0 .. t-1] of its parent slot, seq[t + 1] = its id,
 *      anc[t] = the parent's slot, score = the candidate's, state = ended when id == sep_id, else live;
 *   6. if all W new beams are ended they are appended to the finished list in slot order with length t + 2, and done[b] = 1.
 * The sum is one float64 addition per round, so scores are bit-equal to the host loop's Python-float sums.
 * Rows that do not advance -- every slot of a done sample, and of a sample that became done by rule 3 -- get seq[t + 1] = seq[t]
 * and anc[t] = their own slot; an ended beam keeps sep_id as its token and is replaced in the next round: the step can run all
 * R rows every round on valid tokens and ancestor indices.  Their step outputs are never read.
 * Children are written into the slots their parents are read from, and parents may permute or repeat: one wave owns a sample,
 * a lane owns whole positions, loads the W parent entries of a position into registers and only then stores the W children.
 * No atomics; one workgroup owns a sample's finished list and done[b]; fixed order: two launches give the same bits.
 * Limits: 1 <= W <= 8 (the W*W candidates are one per lane of a wave), 1 <= max_len and max_len + 1 <= 512 --
 * FCMF_ERR_UNSUPPORTED otherwise; a NULL pointer, a negative size, ld < W or t outside [0, max_len) -- FCMF_ERR_ARG; B == 0
 * succeeds without a launch.  The checks are made in this order: negative sizes, limits, t and ld. */
int fcmf_beam_advance(const float* logp, const int32_t* ids, int64_t ld, int B, int W, int t, int max_len, int sep_id,
                      int64_t* seq, int64_t* anc, double* score, int32_t* state, double* fin_score, int64_t* fin_seq,
                      int32_t* fin_len, int32_t* fin_count, int32_t* done, void* stream);

/* ---------------------------------------------------------------------------------------
 * The sampling counterpart (decoding.sample_rounds): round t of B samples x W independent chains, slot r = b*W + c.  seq, anc,
 * score, state and done as in fcmf_beam_advance, every slot live initially; len int32 [R], initially 1: the tokens of the chain,
 * the start token included.  logp float32 [R] and ids int32 [R]: fcmf_sample_token's outputs of the step run on seq[t].
 *   live chain r:  score[r] += (double)logp[r]; seq[t + 1, r] = ids[r]; anc[t, r] = r; len[r] = t + 2; state = ended when
 *                  ids[r] == sep_id.  Chains never branch;
 *   ended chain r: seq[t + 1, r] = seq[t, r], anc[t, r] = r (a valid row for the step, its outputs unread); score, len stay;
 *   done[b] = 1 once no chain of sample b is live.
 * No atomics, fixed order.  Limits and error codes as for fcmf_beam_advance (1 <= W <= 8, max_len + 1 <= 512). */
int fcmf_chain_advance(const float* logp, const int32_t* ids, int B, int W, int t, int max_len, int sep_id, int64_t* seq,
                       int64_t* anc, double* score, int32_t* state, int32_t* len, int32_t* done, void* stream);

/* ---------------------------------------------------------------------------------------
 * y = LayerNorm(dropout(x) + res) * gamma + beta   (eps inside the sqrt, biased variance)
 * Replaces BertSelfOutput/BertOutput/AddNorm + FCMFLayerNorm (mm_modeling.py:158-171,
 * 276-280,324-328,566-573) and HF nn.LayerNorm(eps=1e-5).
 *   x [rows,H] dense; res row r at res + r*res_stride (NULL = no residual);
 *   z (optional, may alias x) <- dropout(x)+res ; mean/rstd float32 [rows]. */
int fcmf_add_ln_fwd(const void* x, const void* res, int64_t res_stride, const float* gamma,
                    const float* beta, void* y, void* z, float* mean, float* rstd,
                    int rows, int H, float eps, float dropout_p, uint64_t seed, int dtype,
                    void* stream);
/* dz [rows,H] <- grad wrt (dropout(x)+res); dx (NULL when dropout_p==0: dx == dz) <- grad wrt x;
 * dgamma/dbeta float32 [H] are ACCUMULATED (atomics); dxsum (float32 [H], may be NULL) accumulates
 * the column sums of dx = the bias gradient of the Linear that produced x. */
int fcmf_add_ln_bwd(const void* dy, const void* z, const float* gamma, const float* mean,
                    const float* rstd, void* dz, void* dx, float* dgamma, float* dbeta, float* dxsum,
                    float* workspace, int rows, int H, float dropout_p, uint64_t seed, int dtype,
                    void* stream);
/* fcmf_add_ln_fwd / fcmf_add_ln_bwd that ALSO emit the e4m3 copy (q8 [rows, H] bytes + qscale [rows], as fcmf_quant_fp8_rows
 * would produce them from the stored values) of the tensor the next fp8 GEMM consumes: y for the forward, the gradient that
 * flows into the producing Linear (dx with dropout, else dz) for the backward -- no separate quantisation pass over it. */
int fcmf_add_ln_fwd_fp8(const void* x, const void* res, int64_t res_stride, const float* gamma, const float* beta, void* y,
                        void* z, float* mean, float* rstd, int rows, int H, float eps, float dropout_p, uint64_t seed,
                        int dtype, void* q8, float* qscale, void* stream);
int fcmf_add_ln_bwd_fp8(const void* dy, const void* z, const float* gamma, const float* mean, const float* rstd, void* dz,
                        void* dx, float* dgamma, float* dbeta, float* dxsum, float* workspace, int rows, int H,
                        float dropout_p, uint64_t seed, int dtype, void* q8, float* qscale, void* stream);
/* floats of scratch `workspace` must hold (per-workgroup partial column sums, reduced by a second
 * kernel without atomics); workspace == NULL falls back to float atomics. */
int64_t fcmf_add_ln_bwd_workspace(int rows, int H);

/* ---------------------------------------------------------------------------------------
 * RoBERTa embeddings (HF RobertaEmbeddings via mm_modeling.py:440-446).
 * position ids = cumsum(ids != pad) * (ids != pad) + pad, one sequence per wave. */
int fcmf_position_ids(const int64_t* ids, int64_t* pos, int nseq, int S, int pad_id, void* stream);
/* z = word[ids] + pos_table[pos] + type[type_ids] (tables float32), then LayerNorm as above. */
int fcmf_embed_ln_fwd(const int64_t* ids, const int64_t* pos, const int64_t* type_ids,
                      const float* word, const float* pos_table, const float* type_table,
                      const float* gamma, const float* beta, void* y, void* z, float* mean,
                      float* rstd, int ntok, int H, float eps, float dropout_p, uint64_t seed,
                      int dtype, void* stream);
/* Adversarial training on the token embeddings (FGM: Miyato et al., "Adversarial Training Methods for Semi-Supervised Text
 * Classification"), one step per micro-batch: (1) a clean forward and backward; g = dz of fcmf_add_ln_bwd in the embedding's
 * backward, the gradient at the pre-LayerNorm sum, [nseq, S, H] in `dtype`; (2) fcmf_adv_scale: scale[s] = epsilon /
 * ||g[s, t, :] over the tokens t with ids[s, t] != pad_id||_2, and 0 where that norm is 0 (every token pad, a zero gradient);
 * (3) fcmf_embed_ln_adv_fwd: a second forward on z = ((word + type) + pos) + scale[s] * g[s, t, :] at the tokens that are not pad
 * -- pad tokens get exactly the plain sum -- then LayerNorm and dropout as fcmf_embed_ln_fwd; (4) its backward is the plain
 * one (the perturbation is a constant) and accumulates onto the first.  The perturbation is never materialised.
 *
 * fcmf_adv_scale: one workgroup per sequence, float32 accumulation, no atomics (the same bits every run); rows whose id is
 * pad_id are not read.  The squares are taken of the values divided by the power of two of the sequence's largest magnitude,
 * so no gradient scale leaves float32, and dz * 2^k gives scale * 2^-k bit for bit while both stay normal numbers.  scale is
 * float32 [nseq].  A NaN among the values that are read gives scale 0.
 * fcmf_embed_ln_adv_fwd: the arguments of fcmf_embed_ln_fwd, then g [ntok, H] in `dtype`, scale [ntok / S] float32, S and
 * pad_id; row r belongs to sequence r / S.  With every scale 0 and finite g the outputs are fcmf_embed_ln_fwd's.
 * Both, before any launch: FCMF_ERR_ARG for a NULL required pointer (type_ids and z may be NULL as in fcmf_embed_ln_fwd),
 * S <= 0, a negative count, ntok no multiple of S, epsilon negative or not finite; FCMF_ERR_UNSUPPORTED for H % 4 != 0, H
 * above the LayerNorm limit of 2048 (the forward), another dtype than FCMF_F32 / FCMF_BF16, dz / g not aligned to four
 * elements; FCMF_OK and nothing done for nseq == 0 / ntok == 0. */
int fcmf_adv_scale(const void* dz, const int64_t* ids, float* scale, int nseq, int S, int H, int pad_id, float epsilon,
                   int dtype, void* stream);
int fcmf_embed_ln_adv_fwd(const int64_t* ids, const int64_t* pos, const int64_t* type_ids,
                          const float* word, const float* pos_table, const float* type_table,
                          const float* gamma, const float* beta, void* y, void* z, float* mean,
                          float* rstd, int ntok, int H, float eps, float dropout_p, uint64_t seed,
                          int dtype, void* stream, const void* g, const float* scale, int S, int pad_id);
/* scatter-add dz into the float32 table gradients (pad rows of word/pos receive nothing).  dpos may be NULL when
 * the position table is handled by fcmf_embed_pos_bwd. */
int fcmf_embed_bwd(const void* dz, const int64_t* ids, const int64_t* pos, const int64_t* type_ids,
                   float* dword, float* dpos, float* dtype_table, int ntok, int H, int pad_id,
                   int dtype, void* stream);
/* position-table gradient for tokens laid out [nseq, S]: same result as the dpos part of fcmf_embed_bwd (ACCUMULATED
 * into dpos), summed per sequence offset in registers first -- the offsets of all sequences share position rows. */
int fcmf_embed_pos_bwd(const void* dz, const int64_t* pos, float* dpos, int nseq, int S, int H, int pad_id,
                       int dtype, void* stream);
/* the position-table AND the type-table gradient (both ACCUMULATED) of tokens laid out [nseq, S] in one pass over dz; call
 * fcmf_embed_bwd with dpos = dtype_table = NULL beside it.  FCMF_ERR_UNSUPPORTED (H not a multiple of 16 bytes of columns or
 * more than 256 such groups, unaligned dz): use fcmf_embed_bwd's type-table path + fcmf_embed_pos_bwd. */
int fcmf_embed_pos_type_bwd(const void* dz, const int64_t* pos, const int64_t* type_ids, float* dpos,
                            float* dtype_table, int nseq, int S, int H, int pad_id, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------
 * Box geometry (roi_modeling.py:79-138,161-163 and the log-clamp of :40), fused:
 *   bias[g,h,i,j] = log(max(relu(<WG_h, emb(box_i, box_j)> + b_h), 1e-6))
 * coords [G,N,4] = (x_min,x_max,y_min,y_max) in float64 or float32 (coord_dtype);
 * wg_w [heads,64], wg_b [heads] float32 (heads <= 8); bias float32 [G,heads,N,N];
 * dim_mat: device float32[8] = 1/1000^(k/8) as the reference rounds it (roi_modeling.py:123-125).
 * coord_dtype = FCMF_F32 | FCMF_BOX_FAST_TRIG: the 64 sines / cosines of a box pair on the hardware's v_sin_f32 / v_cos_f32
 * (arguments up to ~110 revolutions: absolute error <= 1e-4, against 1e-7 of sincosf) -- for a bias that is consumed in bf16. */
#define FCMF_BOX_FAST_TRIG 0x100
int fcmf_box_bias_fwd(const void* coords, int coord_dtype, const float* dim_mat, const float* wg_w,
                      const float* wg_b, float* bias, int G, int N, int heads, void* stream);
/* dwg_w/dwg_b are ACCUMULATED. */
int fcmf_box_bias_bwd(const void* coords, int coord_dtype, const float* dim_mat, const float* wg_w,
                      const float* wg_b, const float* dbias, float* dwg_w, float* dwg_b, int G, int N,
                      int heads, void* stream);
/* the raw 64-d relational embedding [G,N,N,64] float32 (tests / API parity of
 * BoxMultiHeadedAttention.BoxRelationalEmbedding). */
int fcmf_box_embedding(const void* coords, int coord_dtype, const float* dim_mat, float* emb, int G,
                       int N, void* stream);

/* ---------------------------------------------------------------------------------------
 * Cross entropy over C classes (run_multimodal_fcmf.py:290,474; ignore_index for IAOG
 * run_pretraining_fcmf.py:322-324).  loss_rows[n] = -log softmax(logits[n])[label] (0 if ignored);
 * nvalid <- number of non-ignored rows (float). */
int fcmf_xent_fwd(const void* logits, int64_t ld, const int64_t* labels, float* loss_rows,
                  float* nvalid, int n, int C, int64_t ignore_index, int dtype, void* stream);
/* dlogits[n,c] = (softmax - onehot) * (*scale_ptr) * extra_scale  (0 for ignored rows) */
int fcmf_xent_bwd(const void* logits, int64_t ld, const int64_t* labels, void* dlogits,
                  int64_t ldd, const float* scale_ptr, float extra_scale, int n, int C,
                  int64_t ignore_index, int dtype, void* stream);

/* The reduction of CrossEntropyLoss(reduction="mean") (run_multimodal_fcmf.py:290,474) over fcmf_xent_fwd's rows, times
 * `mult` (the driver sums the 6 aspects' batch means, :463-475 = mean over all rows x 6), in one fixed-order pass:
 * out2[0] = mult * sum(loss_rows) / #(labels != ignore_index), out2[1] = mult / #(...) -- the scale of fcmf_xent_bwd. */
int fcmf_xent_mean(const float* loss_rows, const int64_t* labels, int n, int64_t ignore_index,
                   float mult, float* out2, void* stream);

/* ---------------------------------------------------------------------------------------
 * Cross entropy with class weights, label smoothing and a focal factor, normalised per SEGMENT (csrc/loss.hip; the plain
 * entry points above are untouched and stay the path of a loss without options).  Row r of the n rows belongs to segment
 * r % segments (logits [B, A, C] flattened: the segment is the aspect).  For a live row (label != ignore_index) of
 * segment s, with p = softmax over the first C columns and w = the segment's weights (ones when weight is NULL):
 *   l_n  = (1 - eps) w_y (1 - p_y)^gamma (-log p_y) + (eps / C) sum_c w_c (-log p_c)
 *   loss = mult * sum_s [ sum_{n in s, live} l_n / sum_{n in s, live} w_{y_n} ]
 * With gamma = 0 a segment's term is torch's F.cross_entropy(x_s, y_s, weight, label_smoothing=eps, ignore_index).
 *   logits [n, >= C] of `dtype` (FCMF_F32 / FCMF_BF16), row stride ld >= C elements; labels int64 [n];
 *   weight float32 or NULL: [C] shared by all segments (wstride = 0) or one row per segment, wstride >= C elements apart;
 *   eps in [0, 1), gamma >= 0 and finite, not both positive.
 * Every entry point returns before any launch: FCMF_ERR_ARG for a null pointer, segments < 1, n % segments != 0, a
 * stride below C, eps outside [0, 1) or gamma < 0 / not finite; FCMF_ERR_UNSUPPORTED for eps > 0 together with gamma > 0
 * and for another dtype.  C < 1024: one wave per row; C >= 1024: one workgroup per row in one pass, 16-byte accesses when
 * logits (dlogits, weight) and their strides are 16-byte aligned, element accesses otherwise.  1 - p_y is formed from the
 * other classes' exponentials and log p_y as x_y - lse, never as 1.0f - p_y or log(p_y).
 *
 * fcmf_xent_fwd_ex: num[r] = l_r, den[r] = w_{y_r}; both 0 for an ignored row.  A label outside [0, C) that is not
 * ignore_index reads nothing and gives num = NaN, den = 0 (the loss turns NaN instead of reading out of bounds). */
int fcmf_xent_fwd_ex(const void* logits, int64_t ld, const int64_t* labels, const float* weight, int64_t wstride,
                     float* num, float* den, int n, int C, int segments, int64_t ignore_index, float eps, float gamma,
                     int dtype, void* stream);
/* The reduction over fcmf_xent_fwd_ex's rows by ONE workgroup in a fixed order with float64 partial sums (no atomics, no
 * host read): loss[0] = mult * sum_s N_s / D_s with N_s, D_s the segment's sums of num and den (0 / 0 = NaN when a segment
 * has no live weight, as torch); scales[s] (float32 [segments]) = mult / D_s, the scale of fcmf_xent_bwd_ex -- 0 where
 * D_s is not positive, so that such a segment's rows get zero gradients. */
int fcmf_xent_reduce_ex(const float* num, const float* den, int n, int segments, float mult, float* loss, float* scales,
                        void* stream);
/* dlogits[r, j] = sc * [(1 - eps) w_y (p_j - [j == y]) + (eps / C) (p_j sum_c w_c - w_j)] for gamma = 0 and
 *                 sc * w_y [gamma p_y (1 - p_y)^(gamma - 1) log p_y - (1 - p_y)^gamma] ([j == y] - p_j) for gamma > 0,
 * sc = scales[r % segments] * (grad ? *grad : 1) (grad: device float32 [1], the upstream gradient); zeros for ignored rows,
 * rows with a label outside [0, C) and rows whose sc is 0.  dlogits has `dtype` and row stride ldd >= C.  For C >= 1024 it
 * may be the logits themselves (dlogits == logits, ldd == ld: every element is read and written by the same thread).
 * Columns at or past C are neither read nor written. */
int fcmf_xent_bwd_ex(const void* logits, int64_t ld, const int64_t* labels, const float* weight, int64_t wstride,
                     void* dlogits, int64_t ldd, const float* scales, const float* grad, int n, int C, int segments,
                     int64_t ignore_index, float eps, float gamma, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------
 * Symmetric KL divergence of row pairs: the consistency term of R-Drop (Liang et al., 2021; csrc/loss.hip).  For a pair of
 * logit rows a, b of C columns, with p = softmax(a), q = softmax(b), d_c = a_c - b_c:
 *   k        = 1/2 [KL(p||q) + KL(q||p)] = 1/2 sum_c (p_c - q_c) d_c      (log p_c - log q_c = d_c - (lse a - lse b), sum(p - q) = 0)
 *   dk/da_j  =  1/2 [p_j (d_j - E_p d) + p_j - q_j]
 *   dk/db_j  = -1/2 [q_j (d_j - E_q d) + p_j - q_j]
 *   loss     = alpha * sum_s [ sum_{r in s, live} k_r / #live pairs of s ]
 * A constant added to d changes none of the three; the kernels take d around max a - max b (float32: 1/2 (E_p d - E_q d) of the
 * raw d loses the digits of k to a common offset of the rows).  No log is taken.  Bitwise-equal rows give k == 0 and all-zero
 * gradients exactly.  Pair r belongs to segment r % segments, as in fcmf_xent_*_ex.  `labels` (int64 [n], may be NULL = all
 * live) only decides liveness: a pair whose label equals ignore_index is dead.
 *   a, b [n, >= C] of `dtype` (FCMF_F32 / FCMF_BF16), row strides lda, ldb >= C elements; finite logits.
 * C < 1024: one wave per pair; C >= 1024: one workgroup per pair in one pass over the rows, 16-byte accesses when both rows (and,
 * backward, both destinations) and their strides are 16-byte aligned, element accesses otherwise.  float32 arithmetic, no
 * atomics, a fixed order.  FCMF_ERR_ARG before any launch for a null pointer (labels and grad excepted), n < 0, C < 1,
 * segments < 1, n % segments != 0 or a stride below C; FCMF_ERR_UNSUPPORTED for another dtype; n == 0 succeeds without a launch.
 *
 * fcmf_symkl_fwd: num[r] = k_r, den[r] = 1 for a live pair, both 0 for a dead one.  fcmf_xent_reduce_ex(num, den, n, segments,
 * mult = alpha) then yields the loss and scales[s] = alpha / #live pairs of s. */
int fcmf_symkl_fwd(const void* a, int64_t lda, const void* b, int64_t ldb, const int64_t* labels, float* num, float* den, int n,
                   int C, int segments, int64_t ignore_index, int dtype, void* stream);
/* da[r, j] = sc dk/da_j, db[r, j] = sc dk/db_j, sc = scales[r % segments] * (grad ? *grad : 1) (grad: device float32 [1], the
 * upstream gradient).  acc = 0 writes; acc = 1 adds to what da / db hold (each element is read and written by the same thread).
 * A dead pair, or one whose sc is 0, gets zeros with acc = 0 and is left alone with acc = 1.  da, db have `dtype` and row strides
 * ldda, lddb >= C; columns at or past C are never touched.  FCMF_ERR_ARG also for acc outside {0, 1} and when the rows of da or
 * db overlap those of a or b, or each other. */
int fcmf_symkl_bwd(const void* a, int64_t lda, const void* b, int64_t ldb, const int64_t* labels, void* da, int64_t ldda, void* db,
                   int64_t lddb, const float* scales, const float* grad, int n, int C, int segments, int64_t ignore_index, int acc,
                   int dtype, void* stream);

/* torch.nn.BCEWithLogitsLoss() (mean over n x C) of the multi-label photo-category head (image_processing/
 * run_image_categories.py:175,186), in one launch of one workgroup (classifier heads: n x C of a few thousand):
 *   logits [n, C] of `dtype` (row stride ld elements), target float32 [n, C] (row stride ldt; may be NULL when only probs
 *   is asked for);
 *   loss (float32 [1], may be NULL) <- mean of max(x,0) - x*y + log1p(exp(-|x|)), summed in a fixed order in float64;
 *   dlogits (may be NULL, `dtype`, row stride ldd) <- (sigmoid(x) - y) * (dloss ? *dloss : 1) / (n*C);
 *   probs (float32 [n, C] dense, may be NULL) <- sigmoid(x). */
int fcmf_bce_logits(const void* logits, int64_t ld, const float* target, int64_t ldt, int n, int C, const float* dloss,
                    float* loss, void* dlogits, int64_t ldd, float* probs, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------
 * Additive attention mask of a 0 / 1 int64 mask [rows, >= cols] with row stride ld (elements):
 * out[r][c] = (1 - mask[r][c]) * value as float32 [rows, cols]  (fcmf_pretraining.py:53-56,97-100,133-136: value = -10000;
 * HF get_extended_attention_mask for the text encoder: value = finfo(float32).min). */
int fcmf_additive_mask(const int64_t* mask, int64_t ld, float* out, int rows, int cols, float value,
                       void* stream);

/* ---------------------------------------------------------------------------------------
 * elementwise helpers */
/* dst[i] = (dst_dtype) src[i], float32 <-> bfloat16 (round to nearest even).  4 elements per lane when src is 16-byte and dst
 * 8-byte aligned; any other element-aligned pair (a contiguous view inside a packed buffer) goes one element per lane. */
int fcmf_cast(const void* src, void* dst, int64_t n, int src_dtype, int dst_dtype, void* stream);
/* dst (bfloat16 [cols, rows]) = transpose(src float32 [rows, cols]): transposed weight copies for the dX GEMMs */
int fcmf_cast_transpose(const float* src, void* dst, int rows, int cols, void* stream);
/* the same for many weights in ONE launch (all transposed copies go stale together at the optimizer step):
 * src_ptrs / dst_ptrs: device int64 arrays of device addresses (float32 [rows_t, cols_t] -> bfloat16 [cols_t, rows_t]);
 * dims: device int32 [ntensors][2] = (rows, cols); tile_desc: device int32 [ntiles][3] = (tensor, tile row, tile column),
 * one 64x64 tile per workgroup. */
int fcmf_multi_cast_transpose(const int64_t* src_ptrs, const int64_t* dst_ptrs, const int32_t* dims,
                              const int32_t* tile_desc, int ntiles, void* stream);
/* y = x * dropout_mask(seed) / (1-p) ; used for the classifier-head dropout
 * (fcmf_multimodal.py:49) and its backward (same call on dy). */
int fcmf_dropout(const void* x, void* y, int64_t n, float p, uint64_t seed, int dtype, void* stream);
/* out = dy * act'(aux): kind 0 = tanh (aux = tanh OUTPUT, BertPooler mm_modeling.py:430),
 * kind 1 = erf-GELU (aux = PRE-activation, mm_modeling.py:15). */
int fcmf_act_bwd(const void* dy, const void* aux, void* out, int64_t n, int kind, int dtype,
                 void* stream);
/* out[i] (+)= sum over the `reps` copies: in is [outer, reps, inner] -> out [outer, inner] */
int fcmf_sum_axis(const void* in, void* out, int64_t outer, int reps, int64_t inner, int dtype,
                  void* stream);

/* IAOG decoder glue (FCMFSeq2Seq / IAOGDecoder):
 *  fcmf_embed_scale_fwd: out[row] = weight[ids[row]] * scale + pos_table[row % S]  -- `self.embedding(X) * sqrt(H)` followed by
 *      PositionalEncoding's `X + P[:, :T]` (mm_modeling.py:650 and :619-633; pos_table may be NULL); weight / pos_table float32,
 *      out in `dtype`; V = rows of `weight`: an id outside [0, V) reads nothing and makes its output row NaN (torch's gather
 *      raises a device assert there; a NaN loss is the stream-ordered way of being as loud);
 *  fcmf_embed_scale_bwd: dweight[ids[row]] += dy[row] * scale (the embedding gradient; dweight float32 [V, H], zero-initialised by the
 *      caller); rows with an id outside [0, V) are skipped -- dweight is a slice of the flat gradient arena, its neighbour is another
 *      parameter's gradient -- and counted in *oob_count (device int32, may be NULL);
 *  fcmf_head_gather: the decoder `Attention` pairs output slot s of batch element g with head (s*G + g) % heads
 *      (mm_modeling.py:79-85).  slot [G, T, heads*d] dense (gradients per slot, as fcmf_attn_small_bwd with head_quirk writes
 *      them) -> out[g, t, h*d + j] = sum of the slots that read head h; out rows have stride ldo elements (so that dk | dq of a
 *      fused projection land side by side). */
int fcmf_embed_scale_fwd(const int64_t* ids, const float* weight, const float* pos_table, void* out, int n, int H, int S,
                         int64_t V, float scale, int dtype, void* stream);
int fcmf_embed_scale_bwd(const void* dy, const int64_t* ids, float* dweight, int n, int H, int64_t V, int32_t* oob_count,
                         float scale, int dtype, void* stream);
int fcmf_head_gather(const void* slot, void* out, int64_t ldo, int G, int T, int heads, int d, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------
 * Optimizer (run_multimodal_fcmf.py:485-488: clip_grad_norm_ + torch.optim.AdamW, 4 groups).
 * Tensors are described by device tables: ptr tables are int64 device arrays of device
 * addresses; `chunk_tensor[c]`/`chunk_offset[c]` assign chunk c (chunk_size elements) to a
 * tensor and a start offset. */
int fcmf_multi_sumsq(const int64_t* g_ptrs, const int64_t* sizes, const int32_t* chunk_tensor,
                     const int64_t* chunk_offset, int nchunks, int chunk_size,
                     double* sumsq /* [1], accumulated */, double* per_tensor /* [ntensors] or NULL */,
                     void* stream);
/* AdamW with decoupled weight decay, bias correction, eps outside sqrt(v_hat) (torch
 * semantics).  The clip coefficient min(1, max_norm/(sqrt(*sumsq)+1e-6)) is computed on
 * device (max_norm <= 0 disables).  group_of[t] selects lr[]/wd[] (host arrays, <= 8 groups).
 * bf16_ptrs (may be NULL; entries may be 0): shadow bf16 copies refreshed after the update. */
int fcmf_multi_adamw(const int64_t* p_ptrs, const int64_t* g_ptrs, const int64_t* m_ptrs,
                     const int64_t* v_ptrs, const int64_t* bf16_ptrs, const int64_t* sizes,
                     const int32_t* group_of, const int32_t* chunk_tensor,
                     const int64_t* chunk_offset, int nchunks, int chunk_size,
                     const float* lr /*host[8]*/, const float* wd /*host[8]*/, int ngroups,
                     float beta1, float beta2, float eps, int step, const double* sumsq,
                     float max_norm, void* stream);
/* fcmf_multi_adamw that also keeps an exponential moving average of the weights.  Every argument of fcmf_multi_adamw in
 * the same order, then ema_ptrs (device table of float32 addresses, one per tensor, none zero) and ema_decay in [0, 1).
 * p, m, v and the bf16 shadows come out bit-identical to fcmf_multi_adamw; then, per element, with the updated parameter
 * p_new,
 *     e = ema_decay * e + (1.0f - ema_decay) * p_new
 * in float32, every product and the sum rounded on its own (no fused multiply-add; ema_decay == 0 gives e == p_new).  The
 * result does not depend on the alignment of any tensor.  FCMF_ERR_ARG before any launch for ema_ptrs == NULL, an
 * ema_decay that is not finite or lies outside [0, 1), and whatever fcmf_multi_adamw refuses. */
int fcmf_multi_adamw_ema(const int64_t* p_ptrs, const int64_t* g_ptrs, const int64_t* m_ptrs,
                         const int64_t* v_ptrs, const int64_t* bf16_ptrs, const int64_t* sizes,
                         const int32_t* group_of, const int32_t* chunk_tensor,
                         const int64_t* chunk_offset, int nchunks, int chunk_size,
                         const float* lr /*host[8]*/, const float* wd /*host[8]*/, int ngroups,
                         float beta1, float beta2, float eps, int step, const double* sumsq,
                         float max_norm, void* stream, const int64_t* ema_ptrs, float ema_decay);
/* Exchange the contents of the float32 tensors a[t] and b[t] of every tensor in one launch (the averaged weights in for
 * evaluation, and back out).  Where bf16_ptrs is not NULL and bf16_ptrs[t] is not 0 the bf16 copy (round to nearest even)
 * of what a[t] NOW holds is written there: the shadow convention of fcmf_multi_adamw.  Each element is read from both
 * sides before either is written, by the lane that writes them, so a[t] == b[t] leaves the data as it is. */
int fcmf_multi_swap(const int64_t* a_ptrs, const int64_t* b_ptrs, const int64_t* bf16_ptrs,
                    const int64_t* sizes, const int32_t* chunk_tensor, const int64_t* chunk_offset,
                    int nchunks, int chunk_size, void* stream);
/* BertAdam.step for one tensor (optimization.py:94-162): per-parameter clip, no bias
 * correction, weight decay added to the update; `lr_scheduled` is computed by the host
 * from the warmup schedule. `scratch` is a device double[1]. */
int fcmf_bertadam(float* p, const float* g, float* m, float* v, int64_t n, float lr_scheduled,
                  float beta1, float beta2, float eps, float weight_decay, float max_grad_norm,
                  double* scratch, void* stream);

/* ---------------------------------------------------------------------------------------
 * ResNet-152 trunk (fcmf_framework/resnet_utils.py:13-30,39-56 driving torchvision's resnet152:
 * conv1/bn1/relu/maxpool/layer1..4, then adaptive_avg_pool2d / global mean).  Activations are NHWC
 * ([N*H*W, C] row-major) so every convolution is an fcmf_gemm: 1x1 stride-1 convolutions directly on the
 * activation matrix, all others on the patch matrix written by fcmf_conv_im2col; weights are passed as
 * [Cout, kh*kw*Cin] with k = (r, s, c).
 *
 * fcmf_conv_im2col: dst[row, (r*kw + s)*C + c] = src(n, ho*stride + r - pad, wo*stride + s - pad, c) or 0,
 * row = (n*Ho + ho)*Wo + wo, Ho = (H + 2*pad - kh)/stride + 1; columns kh*kw*C .. Kpad-1 are zero (the stem's
 * K = 147 is padded to a multiple of 32).  src element (n,h,w,c) at n*sn + h*sh + w*sw + c*sc: NCHW float32
 * crops and NHWC activations alike.  FCMF_ERR_ARG when the kernel is larger than the padded input (no output row or column).
 * (nn.Conv2d's input gather, torchvision Bottleneck conv2 / downsample.0 / conv1) */
int fcmf_conv_im2col(const void* src, int src_dtype, void* dst, int dst_dtype, int N, int H, int W, int C,
                     int64_t sn, int64_t sh, int64_t sw, int64_t sc, int kh, int kw, int stride, int pad,
                     int Kpad, void* stream);
/* GROUPED BatchNorm2d batch statistics.  The reference calls the trunk once per image index / per (image, ROI)
 * with B crops each (run_multimodal_fcmf.py:449-457) in train() mode (:431): rows are packed group-major, group g
 * = rows [g*rows_per_group, (g+1)*rows_per_group), and every group gets ITS OWN statistics.
 * sums: double workspace of fcmf_bn_stats_workspace(rows_per_group, groups, C) elements, fully overwritten with
 * per-(group, row chunk, channel) partial (sum, sum of squares) pairs -- no atomics -- followed by their per-(group,
 * channel) totals (a second, tree-reduction kernel); fcmf_bn_finalize reads the totals. */
int64_t fcmf_bn_stats_workspace(int64_t rows_per_group, int groups, int C);
int fcmf_bn_stats(const void* x, double* sums, int64_t rows_per_group, int groups, int C, int dtype, void* stream);
/* sums != NULL (training; as written by fcmf_bn_stats with rows_per_group == count): scale/shift [groups, C] from
 * each group's batch mean and biased variance (y = x*scale + shift == (x-mean)/sqrt(var+eps)*gamma + beta);
 * running_mean / running_var receive one momentum update per group in group order with the unbiased variance
 * (nn.BatchNorm2d over `groups` calls).  sums == NULL (eval): scale/shift [C] from the running statistics.
 * mean_out / rstd_out (both or neither; [groups, C], eval: [C]): the statistics the backward needs. */
int fcmf_bn_finalize(const double* sums, const float* gamma, const float* beta, float* running_mean,
                     float* running_var, float* scale, float* shift, float* mean_out, float* rstd_out, int C,
                     int groups, int64_t count, float momentum, float eps, void* stream);
/* y = relu?(x * scale[g] + shift[g] (+ res)), g = row / rows_per_group (eval: rows_per_group = rows); y may alias x.
 * (bn -> relu, and the bottleneck's bn3 -> += identity -> relu) */
int fcmf_bn_apply(const void* x, const void* res, void* y, const float* scale, const float* shift, int64_t rows,
                  int C, int64_t rows_per_group, int relu, int dtype, void* stream);
/* the same with y an NHWC tensor that carries a zero border of `pad` pixels ([n, H + 2 pad, W + 2 pad, C], border zeroed once by
 * its owner; rows = n * H * W): the input of an implicit-GEMM 3x3 convolution, produced without a padding pass */
int fcmf_bn_apply_pad(const void* x, const void* res, void* y_padded, const float* scale, const float* shift,
                      int64_t rows, int C, int64_t rows_per_group, int relu, int H, int W, int pad, int dtype, void* stream);
/* fcmf_bn_finalize + fcmf_bn_apply / fcmf_bn_apply_pad in ONE launch: every workgroup derives the scale / shift of its channels
 * from the totals in `sums` itself (sums == NULL: eval, running statistics), the first workgroup of a group leaves mean / rstd
 * [groups, C] (both or neither) for the backward, workgroup 0 applies the `groups` running-statistics updates in group order.
 * rows = groups * rows_per_group; pad = 0: y [rows, C] (may alias x); pad > 0: y the zero-bordered NHWC buffer (rows = n * H * W).
 * FCMF_ERR_UNSUPPORTED unless C / (16 / sizeof(T)) is a power of two <= 256 and x / y / res are 16-byte aligned (the caller then
 * takes the two separate entry points). */
int fcmf_bn_finalize_apply(const void* x, const void* res, void* y, const double* sums, const float* gamma, const float* beta,
                           float* running_mean, float* running_var, float* mean_out, float* rstd_out, int C, int groups,
                           int64_t rows_per_group, float momentum, float eps, int relu, int H, int W, int pad, int dtype, void* stream);
/* Implicit-GEMM convolution (no patch matrix): y[(n, oy, ox), co] = sum_{ky,kx,c} x[n, oy*stride + ky, ox*stride + kx, c] * w[co, (ky,kx,c)]
 * on the bf16 MFMA GEMM kernels -- the LDS-DMA of a k-tile reads tap (ky, kx) of every output pixel's receptive field straight
 * from the NHWC activation x [n, Hp, Wp, C], which INCLUDES the zero border where the convolution pads (Hp = H + 2 pad).
 * ResNet-152 trunk: every 3x3 convolution and the strided 1x1 shortcuts (resnet_utils.py:13-24 driving torchvision's Bottleneck);
 * bf16, C a power of two >= 64, w [Cout, kh*kw*C] row-major in (ky, kx, c) order, y [n*Ho*Wo, Cout]. */
int fcmf_conv_gemm(fcmf_gemm_ctx* ctx, const void* x, const void* w, void* y, int n, int Hp, int Wp, int C, int Ho, int Wo,
                   int kh, int kw, int stride, int Cout, void* stream);
/* fcmf_conv_gemm with an epilogue: y = epi(conv(x, w) + bias[co] (+ aux[(n, oy, ox), co])), bias float32 [Cout] (required), aux bf16
 * [n*Ho*Wo, Cout] (required by the two ADD epilogues, ignored otherwise), epilogue one of FCMF_EPI_NONE / _RELU / _ADD / _ADD_RELU
 * (anything else: FCMF_ERR_ARG).  The convolutions of an eval-mode trunk whose BatchNorm is folded into w and bias. */
int fcmf_conv_gemm_epi(fcmf_gemm_ctx* ctx, const void* x, const void* w, void* y, const float* bias, void* aux, int epilogue,
                       int n, int Hp, int Wp, int C, int Ho, int Wo, int kh, int kw, int stride, int Cout, void* stream);
/* f32 C (+)= op(A) op(B) of bf16 operands with a COLUMN-BLOCKED output: element (i, j) is stored at
 *   C + (j / col_block) * col_block_stride + i * ldc + j % col_block          (col_block % 4 == 0, N % col_block == 0).
 * The per-head projection weights of the IAOG decoder's Attention are [n_head, E, d] tensors (mm_modeling.py:57-58); their gradient
 * dW^T [E, n_head * d] = x^T dY written with col_block = d, col_block_stride = E * d, ldc = d lands in exactly that layout (the
 * autograd of the reference's repeat + bmm, mm_modeling.py:79-92, without a permute copy per parameter).  Split-K through the
 * context's workspace only (the reduce pass writes the blocked layout): FCMF_ERR_UNSUPPORTED otherwise -- callers fall back to
 * fcmf_gemm into a plain buffer. */
int fcmf_gemm_colblocks(fcmf_gemm_ctx* ctx, const void* A, const void* B, float* C, int M, int N, int K, int64_t lda,
                        int64_t ldb, int64_t ldc, int trans_a, int trans_b, int col_block, int64_t col_block_stride,
                        int accumulate, void* stream);

/* The weight gradients of a whole backward pass in one launch: C_i [M_i, N_i] float32 (+)= A_i^T B_i for `count` problems of ANY
 * shapes, A_i = dY_i [K_i, M_i], B_i = X_i [K_i, N_i] (bf16, K_i = tokens) -- nn.Linear's weight gradient (loss.backward(),
 * run_multimodal_fcmf.py:466), which the host queues during the backward pass.  The 256 x 256 tiles of all matrices form ONE work
 * list for the persistent kernel: whole rounds of equal-depth tiles run unsplit and write C themselves, the rest is cut into
 * near-equal pieces of K whose partial tiles one reduce launch sums in a fixed order (bit-identical from run to run).  Several
 * problems may name the SAME C (a weight applied more than once): C (+)= the sum of all of them.  A / B / C: host arrays of `count`
 * device pointers; M / N / K / lda / ldb / ldc: host arrays of `count`.  accumulate as fcmf_gemm.  The tables travel through the
 * head of the context's workspace.  Problems the tile kernel does not take (M or N < 256, unaligned), a list of fewer than two
 * that it takes, and every problem when there is no workspace run as fcmf_gemm calls inside: same results. */
int fcmf_gemm_dw_list(fcmf_gemm_ctx* ctx, int count, const void* const* A, const void* const* B, void* const* C, const int* M,
                      const int* N, const int* K, const int64_t* lda, const int64_t* ldb, const int64_t* ldc, int accumulate,
                      void* stream);
/* The work list fcmf_gemm_dw_list builds, without a device: from the shapes, dest[i] (index of the first problem that shares problem
 * i's C; i itself otherwise), the workgroup count and the workspace size.  items [max_items][6] = problem, tile row, tile column,
 * first k-tile (32 deep), k-tiles, workspace slot (-1: the item writes C) in launch order (item i runs on workgroup i % num_cus);
 * reduce [max_reduce][5] = first slot, slots, problem, tile row, tile column; either may be NULL.  info[6] = items, reduce entries,
 * slots, bytes of tables at the head of the workspace, workspace bytes needed in all, planned efficiency (mean / max k-tiles per
 * workgroup) in millionths.  FCMF_ERR_UNSUPPORTED: the workspace is too small for the partial tiles of the shared destinations. */
int fcmf_gemm_dw_list_plan(int count, const int* M, const int* N, const int* K, const int* dest, int num_cus, int64_t ws_bytes,
                           int* items, int max_items, int* reduce, int max_reduce, int64_t* info);
/* `count` same-shape problems: fcmf_gemm_dw_list with one shape. */
int fcmf_gemm_dw_batched(fcmf_gemm_ctx* ctx, int count, const void* const* A, const void* const* B, void* const* C, int M, int N, int K,
                         int64_t lda, int64_t ldb, int64_t ldc, int accumulate, void* stream);
/* Implicit-GEMM convolution for inputs with few channels -- the trunk's stem, conv1 = 7x7 / stride 2 / pad 3 on RGB crops
 * (torchvision resnet152.conv1 driven by resnet_utils.py:13-24), whose patch matrix was 1.8 GB per 448 crops: x is NHWC bf16 with
 * `pix` elements per pixel (a power of two: 4 = RGB0, written by fcmf_pack_rgb0) and its zero border; for every kernel row ky the
 * contraction walks ONE contiguous run of `run` elements (a power of two >= 32, >= kw * pix: 32 = 8 pixels for kw = 7) starting at
 * pixel (oy*stride + ky, ox*stride).  K = kh * run; w [Cout, kh * run] bf16 holds zeros where the run exceeds the kernel (kx >= kw,
 * the padding channel).  stride * pix must be a multiple of 8 (16-byte DMA).  y [n*Ho*Wo, Cout] bf16.  stats (optional, may be
 * NULL): the block statistics of y as fcmf_gemm_colstats writes them (same restriction: FCMF_ERR_UNSUPPORTED for Cout < 256). */
int fcmf_conv_gemm_runs(fcmf_gemm_ctx* ctx, const void* x, const void* w, void* y, float* stats, int n, int Hp, int Wp, int pix, int run,
                        int Ho, int Wo, int kh, int stride, int Cout, void* stream);
/* crops in any layout (element strides of n, h, w, c; float32 / float64 / bf16; 3 channels) -> the interior of dst
 * [N, H + 2 pad, Wp, 4] bf16, Wp >= W + 2 pad (channel 3 = 0; the border is NOT written: zero it once).  Every value is rounded
 * once, to the nearest bf16 with ties to even (a float64 source does not pass through float32). */
int fcmf_pack_rgb0(const void* src, int src_dtype, void* dst, int N, int H, int W, int64_t sn, int64_t sh, int64_t sw, int64_t sc,
                   int pad, int Wp, void* stream);
/* The 1x1 (plain GEMM: A [M, K] = the NHWC activation, W [N, K]) and implicit-GEMM convolutions with the statistics of the
 * train-mode BatchNorm that follows EVERY convolution of the trunk (torchvision Bottleneck: conv -> bn, resnet_utils.py:13-24) as a
 * by-product of the epilogue: stats [ceil(M / R)][N][2] float32 <- (sum, sum of squares) of each block of R output rows per
 * output channel, of the values as stored (bf16-rounded); plain stores, deterministic.  bf16 only.  R =
 * fcmf_gemm_colstats_block_rows(ctx, M, N, K): 128 for the 256-column tiles, 256 for the narrow layouts (32 <= N <= 128 with
 * M >= 8192 and K % 64 == 0), 0 where no kernel emits statistics.  FCMF_ERR_UNSUPPORTED where
 * the shape does not run on the 256-row persistent kernel (M or N < 256, unaligned): run fcmf_gemm / fcmf_conv_gemm +
 * fcmf_bn_stats instead.  fcmf_bn_stats_blocks: those blocks -> the per-group totals inside `sums` (a fcmf_bn_stats_workspace
 * buffer) that fcmf_bn_finalize reads; rows_per_group must be a multiple of block_rows (else FCMF_ERR_UNSUPPORTED). */
int fcmf_gemm_colstats(fcmf_gemm_ctx* ctx, const void* A, const void* B, void* C, float* stats, int M, int N, int K, int64_t lda,
                       int64_t ldb, int64_t ldc, void* stream);
int fcmf_conv_gemm_colstats(fcmf_gemm_ctx* ctx, const void* x, const void* w, void* y, float* stats, int n, int Hp, int Wp, int C,
                            int Ho, int Wo, int kh, int kw, int stride, int Cout, void* stream);
int fcmf_gemm_colstats_block_rows(const fcmf_gemm_ctx* ctx, int M, int N, int K);
int fcmf_bn_stats_blocks(const float* blockstats, double* sums, int64_t rows_per_group, int groups, int C, int block_rows, void* stream);
/* nn.MaxPool2d(kernel_size=3, stride=2, padding=1) on NHWC: [N,H,W,C] -> [N,(H-1)/2+1,(W-1)/2+1,C] */
int fcmf_maxpool3x3s2(const void* x, void* y, int N, int H, int W, int C, int dtype, void* stream);
/* F.adaptive_avg_pool2d(x, [oh, ow]) of an NHWC activation, float32 output: layout 0 = [N, C, oh, ow] (what
 * myResNetImg returns, resnet_utils.py:24), layout 1 = [N, oh*ow, C] (the [B, 49, 2048] token layout the driver
 * builds with view/permute, run_multimodal_fcmf.py:451).  oh = ow = 1 is myResNetRoI's x.mean(3).mean(2) (:48). */
int fcmf_adaptive_avgpool(const void* x, float* y, int N, int H, int W, int C, int oh, int ow, int layout,
                          int dtype, void* stream);

/* ---- backward of the trunk (fine-tuning the CNN: resnet_utils.py if_fine_tune=True, --fine_tune_cnn) ----
 * BatchNorm2d (+ the ReLU behind it) backward, grouped like the forward.  g: gradient wrt the block output z; z: that
 * output (ReLU mask z > 0; NULL = no ReLU); y: the convolution output the forward normalised; mean/rstd from
 * fcmf_bn_finalize.  dy <- gradient wrt y: gamma*rstd*(gm - mean_rows(gm) - xhat*mean_rows(gm*xhat)) with gm = g*[z>0]
 * (training != 0) or gamma*rstd*gm (eval); gres (may be NULL) <- gm, the gradient of the identity branch that was added
 * before the ReLU; dgamma / dbeta float32 [C] are ACCUMULATED.  dy / gres may alias g.
 * sums: double workspace of fcmf_bn_stats_workspace(rows_per_group, groups, C) elements. */
int fcmf_bn_bwd(const void* g, const void* z, const void* y, const float* mean, const float* rstd, const float* gamma,
                double* sums, void* dy, void* gres, float* dgamma, float* dbeta, int64_t rows_per_group, int groups,
                int C, int training, int dtype, void* stream);
/* transpose of fcmf_conv_im2col (NHWC, same dtype both sides): dX[n,h,w,c] = sum of dA over the windows covering the
 * pixel, gathered per input pixel (no atomics).  dA [N*Ho*Wo, Kpad] = dY * W is the patch-matrix gradient. */
int fcmf_conv_col2im(const void* dA, void* dX, int N, int H, int W, int C, int kh, int kw, int stride, int pad,
                     int Kpad, int dtype, void* stream);
/* nn.MaxPool2d(3, 2, 1) backward: dX gets dY of every window whose first maximum (scan order) the pixel is */
int fcmf_maxpool3x3s2_bwd(const void* x, const void* dy, void* dx, int N, int H, int W, int C, int dtype, void* stream);
/* F.adaptive_avg_pool2d backward: dy float32 in the forward's output layout (0 = [N,C,oh,ow], 1 = [N,oh*ow,C]) */
int fcmf_adaptive_avgpool_bwd(const float* dy, void* dx, int N, int H, int W, int C, int oh, int ow, int layout,
                              int dtype, void* stream);

/* ---------------------------------------------------------------------------------------
 * Crop + antialiased resize + flip + normalise of uint8 photos (the category classifiers' preprocessing,
 * image_processing/run_image_categories.py:35-41 and run_roi_categories.py:34-45: v2.Resize((S,S), antialias=True),
 * RandomHorizontalFlip, ConvertImageDtype, Normalize), for a batch of crops of different photos and sizes in one call.
 * Photos are packed into one DEVICE byte buffer `src` of `src_bytes` bytes; crop i is described by descs[i] (DEVICE array):
 *   offset      byte offset of its photo in src;  H, W its size;  sC, sH, sW element (= byte) strides of channel, row and
 *               column (CHW: W*H, W, 1; HWC as PIL decodes it: 1, 3*W, 3);
 *   r0:r1, c0:c1 the crop box as the reference slices it (image[:, x1:x2, y1:y2]: the first index is rows); ends past the photo
 *               are clipped as in a Python slice;
 *   flip        != 0: out[..., x] = resized[..., S-1-x].
 * out [n, 3, S, S] contiguous, float32 or bfloat16 (`dtype`) = (rint(resize(crop)) clamped to [0, 255] / 255 - mean[c]) / std[c]
 * with resize = F.interpolate(mode="bilinear", antialias=True, align_corners=False) on the float values (review_batches.to_crop).
 * mean / std: HOST float[3].  scratch: caller-owned DEVICE float32 of >= n * 3 * max_rows * S elements (the horizontally resampled
 * rows); max_rows >= the clipped height of every crop.  A crop that is empty, starts below 0 or reaches past src_bytes, or is
 * taller than max_rows, yields NaN (host wrappers reject those before the launch). */
typedef struct {
  int64_t offset;
  int H, W;
  int64_t sC, sH, sW;
  int r0, r1, c0, c1;
  int flip, reserved;
} fcmf_crop_desc;

int fcmf_crop_resize_normalize(const uint8_t* src, int64_t src_bytes, const fcmf_crop_desc* descs, int n, int max_rows, int S,
                               const float* mean, const float* std, float* scratch, int64_t scratch_bytes, void* out,
                               int dtype, void* stream);

/* ---------------------------------------------------------------------------------------
 * Data-parallel gradient exchange (reference: torch.distributed.init_process_group("nccl") + DistributedDataParallel,
 * run_multimodal_fcmf.py:169,237-240; run_pretraining_fcmf.py:196-199).  One communicator per process (= per GPU, the HIP
 * device current at creation time); the flat gradient arena is all-reduced bucket by bucket IN PLACE on `stream`
 * (RCCL over xGMI), so the collective of one bucket overlaps the backward kernels that are still producing the next.
 * RCCL is bound at run time (the process's own copy if it has one, e.g. PyTorch's): FCMF_ERR_COMM when it is absent.
 *   fcmf_dp_unique_id   : rank 0 fills a HOST buffer of FCMF_DP_UNIQUE_ID_BYTES and hands it to the other ranks out of band
 *                         (the drivers use their torch.distributed store);
 *   fcmf_dp_comm_create : collective over the `nranks` processes holding that id; *comm receives an opaque handle;
 *   fcmf_dp_allreduce_bucket: buf[count] of `dtype` (FCMF_F32 / FCMF_BF16) <- sum (average = 0) or mean (average != 0, formed
 *                         inside the collective) over the ranks; enqueued on `stream`, returns at once. */
#define FCMF_DP_UNIQUE_ID_BYTES 128
int fcmf_dp_unique_id(void* out_host);
int fcmf_dp_comm_create(void** comm, const void* unique_id_host, int nranks, int rank);
int fcmf_dp_comm_destroy(void* comm);
int fcmf_dp_allreduce_bucket(void* comm, void* buf, int64_t count, int dtype, int average, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FCMF_HIP_H */
