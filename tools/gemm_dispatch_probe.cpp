// CPU-only probe of the GEMM host dispatch (csrc/gemm.hip): calls the extern "C" entry points with fake device addresses and
// prints, for every call, the return code, the last_kernel string and every launch the call made -- host stub, grid, block,
// dynamic LDS, the dynamic-LDS limit set for that kernel, and every field of the parameter struct by name.  The HIP launch
// calls are defined in hip_launch_stubs.h (definitions in the executable take precedence over the runtime's), so nothing reaches
// a device and no address is dereferenced.  Two builds of gemm.hip dispatch alike exactly when their dumps are byte-identical.
//
// Build and run (no GPU needed), from csrc/ after `make gemm.o`:
//   clang++ -std=c++17 -O1 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -I../../include -I../../tools -c ../../tools/gemm_dispatch_probe.cpp -o probe.o
//   hipcc --offload-arch=gfx950 -rdynamic probe.o gemm.o -ldl -o gemm_dispatch_probe
//   ./gemm_dispatch_probe | sha256sum        # the dump; the summary (counts per stub / last_kernel / return code) goes to stderr
// GemmParams / GenericParams / DwList below mirror gemm.hip: keep them in step with it.
#include "fcmf_hip.h"

struct GemmParams {
  const void* A; const void* B; void* C; const float* bias; void* aux;
  int M, N, K;
  int64_t lda, ldb, ldc;
  int epilogue, accumulate, ksplit, ktiles_per_split;
  unsigned a_bytes, b_bytes, c_bytes;
  float* colsum;
  int tiles, total_items;
  float* ws;
  int nt_out;
  const float* sa; const float* sb;
  int cv_C, cv_logC, cv_Hp, cv_Wp, cv_Ho, cv_Wo, cv_kw, cv_inv_kw, cv_stride;
  float* colstats;
  int cv_logP;
};
struct DwList { const void* mats; const void* items; };
struct GenericParams {
  const void* A; const void* B; void* C; const float* bias; void* aux;
  int M, N, K;
  int64_t a_si, a_sk, b_sj, b_sk, ldc;
  int epilogue, accumulate;
  float* colsum;
  int kchunk;
};

#include "hip_launch_stubs.h"
#define I(a, i) (*(int*)(a)[i])
#define L(a, i) ((long long)*(int64_t*)(a)[i])
#define P(a, i) (*(void**)(a)[i])

static void print_launch_params(const std::string& name, void** a) {
  if (name.find("splitk_reduce_list") != std::string::npos) {
    printf("   ws=%p red=%p mats=%p entries=%d accumulate=%d", P(a, 0), P(a, 1), P(a, 2), I(a, 3), I(a, 4));
  } else if (name.find("splitk_reduce_frag") != std::string::npos) {
    printf("   ws=%p C=%p M=%d N=%d ldc=%lld ksplit=%d tiles=%d tiles_n=%d accumulate=%d cblk=%d cblk_stride=%lld", P(a, 0), P(a, 1), I(a, 2), I(a, 3), L(a, 4), I(a, 5), I(a, 6), I(a, 7), I(a, 8), I(a, 9), L(a, 10));
  } else if (name.find("splitk_reduce") != std::string::npos) {
    printf("   ws=%p C=%p M=%d N=%d ldc=%lld ksplit=%d accumulate=%d", P(a, 0), P(a, 1), I(a, 2), I(a, 3), L(a, 4), I(a, 5), I(a, 6));
  } else if (name.find("gemm_generic") != std::string::npos) {
    const GenericParams& p = *(GenericParams*)a[0];
    printf("   A=%p B=%p C=%p bias=%p aux=%p M=%d N=%d K=%d a_si=%lld a_sk=%lld b_sj=%lld b_sk=%lld ldc=%lld epilogue=%d accumulate=%d colsum=%p kchunk=%d",
           p.A, p.B, p.C, (void*)p.bias, p.aux, p.M, p.N, p.K, (long long)p.a_si, (long long)p.a_sk, (long long)p.b_sj, (long long)p.b_sk, (long long)p.ldc, p.epilogue, p.accumulate, (void*)p.colsum, p.kchunk);
  } else {
    const GemmParams& p = *(GemmParams*)a[0];
    printf("   A=%p B=%p C=%p bias=%p aux=%p M=%d N=%d K=%d lda=%lld ldb=%lld ldc=%lld epilogue=%d accumulate=%d ksplit=%d ktiles_per_split=%d a_bytes=%u b_bytes=%u c_bytes=%u"
           " colsum=%p tiles=%d total_items=%d ws=%p nt_out=%d sa=%p sb=%p cv=%d,%d,%d,%d,%d,%d,%d,%d,%d colstats=%p cv_logP=%d",
           p.A, p.B, p.C, (void*)p.bias, p.aux, p.M, p.N, p.K, (long long)p.lda, (long long)p.ldb, (long long)p.ldc, p.epilogue, p.accumulate, p.ksplit, p.ktiles_per_split, p.a_bytes, p.b_bytes, p.c_bytes,
           (void*)p.colsum, p.tiles, p.total_items, (void*)p.ws, p.nt_out, (void*)p.sa, (void*)p.sb, p.cv_C, p.cv_logC, p.cv_Hp, p.cv_Wp, p.cv_Ho, p.cv_Wo, p.cv_kw, p.cv_inv_kw, p.cv_stride,
           (void*)p.colstats, p.cv_logP);
    if (name.find("dw_batched") != std::string::npos) { const DwList& l = *(DwList*)a[1]; printf(" mats=%p items=%p", l.mats, l.items); }
  }
}

// ---- the sweep ---------------------------------------------------------------------------------------------------------------
static char* const A0 = (char*)0x10000000, * const B0 = (char*)0x20000000, * const C0 = (char*)0x30000000;
static float* const BIAS = (float*)0x40000000, * const COLSUM = (float*)0x60000000, * const STATS = (float*)0x68000000;
static void* const AUX = (void*)0x50000000, * const WS = (void*)0x70000000, * const STREAM = (void*)0x1000;
static const int Ms[] = {1, 36, 64, 100, 128, 255, 256, 384, 512, 768, 2048, 8192, 24576, 49152};
static const int Ns[] = {4, 8, 36, 64, 128, 256, 768, 1024, 3072, 4096, 64008};
static const int Ks[] = {32, 64, 96, 128, 768, 1024, 3072, 49152};
struct Ctx { fcmf_gemm_ctx* c; char tag[48]; };
static Ctx g_ctx[24]; static int g_nctx = 0;

static void done(const Ctx& c, const char* what, int rc) {
  const char* k = fcmf_gemm_ctx_last_kernel(c.c);
  printf("%s [%s] rc=%d last=%s\n", what, c.tag, rc, k);
  ++g_count["rc " + std::to_string(rc)];
  if (rc == FCMF_OK && c.c) ++g_count["last_kernel " + std::string(k)];
}
static void add_ctx(const char* tag, bool make, int64_t ws_bytes, int tile = -1, int kb = -1, int cus = -1) {
  Ctx& c = g_ctx[g_nctx++];
  c.c = nullptr;
  snprintf(c.tag, sizeof c.tag, "%s", tag);
  if (!make) return;
  fcmf_gemm_ctx_create(&c.c);
  if (ws_bytes) fcmf_gemm_ctx_set_workspace(c.c, WS, ws_bytes);
  if (tile >= 0) fcmf_gemm_ctx_tune(c.c, tile, kb, cus, -1);
}
// variant 0: aligned operands, natural leading dimensions; 1: A misaligned by 2 bytes; 2: odd lda
static void sweep_gemm(const Ctx& c, int variant) {
  char what[160];
  for (int M : Ms) for (int N : Ns) for (int K : Ks) for (int ta = 0; ta < 2; ++ta) for (int tb = 0; tb < 2; ++tb)
    for (int din = 0; din < 2; ++din) for (int dout = 0; dout < 2; ++dout) for (int epi = 0; epi < 6; ++epi) for (int acc = 0; acc < 2; ++acc)
      for (int opt = 0; opt < 8; ++opt) {
        const int64_t lda = (ta ? M : K) + (variant == 2), ldb = tb ? N : K;
        snprintf(what, sizeof what, "gemm v%d %dx%dx%d t%d%d d%d%d e%d a%d o%d", variant, M, N, K, ta, tb, din, dout, epi, acc, opt);
        done(c, what, fcmf_gemm(c.c, A0 + 2 * (variant == 1), B0, C0, opt & 1 ? BIAS : nullptr, opt & 2 ? AUX : nullptr, opt & 4 ? COLSUM : nullptr, M, N, K,
                                lda, ldb, N, ta, tb, din, dout, epi, acc, STREAM));
      }
}
struct Conv { int Hp, Wp, C, Ho, Wo, k, stride, Cout; };
// ResNet-152 at 224 x 224: every distinct convolution after the stem (1x1 reduce / 3x3 / 1x1 expand / downsample of each stage)
static const Conv convs[] = {
  {56, 56, 64, 56, 56, 1, 1, 64}, {58, 58, 64, 56, 56, 3, 1, 64}, {56, 56, 64, 56, 56, 1, 1, 256}, {56, 56, 256, 56, 56, 1, 1, 64},
  {56, 56, 256, 56, 56, 1, 1, 128}, {58, 58, 128, 28, 28, 3, 2, 128}, {28, 28, 128, 28, 28, 1, 1, 512}, {56, 56, 256, 28, 28, 1, 2, 512},
  {28, 28, 512, 28, 28, 1, 1, 128}, {30, 30, 128, 28, 28, 3, 1, 128}, {28, 28, 512, 28, 28, 1, 1, 256}, {30, 30, 256, 14, 14, 3, 2, 256},
  {14, 14, 256, 14, 14, 1, 1, 1024}, {28, 28, 512, 14, 14, 1, 2, 1024}, {14, 14, 1024, 14, 14, 1, 1, 256}, {16, 16, 256, 14, 14, 3, 1, 256},
  {14, 14, 1024, 14, 14, 1, 1, 512}, {16, 16, 512, 7, 7, 3, 2, 512}, {7, 7, 512, 7, 7, 1, 1, 2048}, {14, 14, 1024, 7, 7, 1, 2, 2048},
  {7, 7, 2048, 7, 7, 1, 1, 512}, {9, 9, 512, 7, 7, 3, 1, 512}, {58, 58, 32, 56, 56, 3, 1, 64} /* unsupported: C < 64 */};
static void sweep_rest(const Ctx& c) {
  char what[160];
  const int n = 448;                                   // bench.py's crop batch: 7 images x 64 reviews
  for (const Conv& v : convs) {
    snprintf(what, sizeof what, "conv %d,%d,%d->%d,%d k%d s%d co%d", v.Hp, v.Wp, v.C, v.Ho, v.Wo, v.k, v.stride, v.Cout);
    done(c, what, fcmf_conv_gemm(c.c, A0, B0, C0, n, v.Hp, v.Wp, v.C, v.Ho, v.Wo, v.k, v.k, v.stride, v.Cout, STREAM));
    done(c, what, fcmf_conv_gemm_colstats(c.c, A0, B0, C0, STATS, n, v.Hp, v.Wp, v.C, v.Ho, v.Wo, v.k, v.k, v.stride, v.Cout, STREAM));
  }
  done(c, "stem runs", fcmf_conv_gemm_runs(c.c, A0, B0, C0, nullptr, n, 230, 232, 4, 32, 112, 112, 7, 2, 64, STREAM));
  done(c, "stem runs+stats", fcmf_conv_gemm_runs(c.c, A0, B0, C0, STATS, n, 230, 232, 4, 32, 112, 112, 7, 2, 64, STREAM));
  done(c, "stem runs bad pix", fcmf_conv_gemm_runs(c.c, A0, B0, C0, STATS, n, 230, 232, 3, 32, 112, 112, 7, 2, 64, STREAM));
  // IAOG decoder heads: dW^T [E, heads * d] = x^T dY into the parameters' [heads, E, d] layout; then geometries the path refuses
  for (int acc = 0; acc < 2; ++acc) {
    done(c, "colblocks iaog", fcmf_gemm_colblocks(c.c, A0, B0, (float*)C0, 768, 768, 2048, 768, 768, 64, 1, 1, 64, 768 * 64, acc, STREAM));
    done(c, "colblocks small", fcmf_gemm_colblocks(c.c, A0, B0, (float*)C0, 128, 768, 2048, 128, 768, 64, 1, 1, 64, 128 * 64, acc, STREAM));
    done(c, "colblocks block 100", fcmf_gemm_colblocks(c.c, A0, B0, (float*)C0, 768, 768, 2048, 768, 768, 100, 1, 1, 100, 768 * 100, acc, STREAM));
    done(c, "colblocks ldc < block", fcmf_gemm_colblocks(c.c, A0, B0, (float*)C0, 768, 768, 2048, 768, 768, 32, 1, 1, 64, 768 * 64, acc, STREAM));
  }
  for (int M : Ms) for (int N : Ns) for (int K : Ks) {
    snprintf(what, sizeof what, "colstats %dx%dx%d", M, N, K);
    done(c, what, fcmf_gemm_colstats(c.c, A0, B0, C0, STATS, M, N, K, K, K, N, STREAM));
    printf("block_rows %dx%dx%d [%s] -> %d\n", M, N, K, c.tag, fcmf_gemm_colstats_block_rows(c.c, M, N, K));
  }
  done(c, "colstats no stats", fcmf_gemm_colstats(c.c, A0, B0, C0, nullptr, 512, 512, 512, 512, 512, 512, STREAM));
  static const int counts[] = {0, 1, 2, 12, 33, 40};
  static const int shapes[][3] = {{768, 768, 8192}, {768, 3072, 8192}, {768, 128, 8192} /* falls back: N < 256 */};
  const void* pa[40]; const void* pb[40]; void* pc[40];
  // (outputs 16 MiB apart: destinations that overlap without being the same matrix stay out of a list)
  for (int i = 0; i < 40; ++i) { pa[i] = A0 + i * 0x100000; pb[i] = B0 + i * 0x100000; pc[i] = C0 + (size_t)i * 0x1000000; }
  for (int cnt : counts) for (const auto& s : shapes) for (int acc = 0; acc < 2; ++acc) {
    snprintf(what, sizeof what, "dw_batched n%d %dx%dx%d a%d", cnt, s[0], s[1], s[2], acc);
    done(c, what, fcmf_gemm_dw_batched(c.c, cnt, pa, pb, pc, s[0], s[1], s[2], s[0], s[1], s[1], acc, STREAM));
  }
  static const int fp8_epi[] = {FCMF_EPI_NONE, FCMF_EPI_GELU, FCMF_EPI_DGELU, FCMF_EPI_ADD, FCMF_EPI_TANH, FCMF_EPI_DTANH};
  for (int epi : fp8_epi) for (int aux = 0; aux < 2; ++aux) {
    snprintf(what, sizeof what, "fp8 e%d aux%d", epi, aux);
    done(c, what, fcmf_gemm_fp8(c.c, A0, BIAS, B0, BIAS, C0, BIAS, aux ? AUX : nullptr, COLSUM, 8192, 3072, 768, 768, 768, 3072, epi, STREAM));
  }
  done(c, "fp8 no scale", fcmf_gemm_fp8(c.c, A0, nullptr, B0, BIAS, C0, nullptr, nullptr, nullptr, 8192, 3072, 768, 768, 768, 3072, 0, STREAM));
  done(c, "fp8 K % 128", fcmf_gemm_fp8(c.c, A0, BIAS, B0, BIAS, C0, nullptr, nullptr, nullptr, 8192, 3072, 832, 832, 832, 3072, 0, STREAM));
  done(c, "fp8 lda % 16", fcmf_gemm_fp8(c.c, A0, BIAS, B0, BIAS, C0, nullptr, nullptr, nullptr, 8192, 3072, 768, 776, 768, 3072, 0, STREAM));
  done(c, "fp8 misaligned", fcmf_gemm_fp8(c.c, A0 + 4, BIAS, B0, BIAS, C0, nullptr, nullptr, nullptr, 8192, 3072, 768, 768, 768, 3072, 0, STREAM));
  done(c, "fp8 M < 256", fcmf_gemm_fp8(c.c, A0, BIAS, B0, BIAS, C0, nullptr, nullptr, nullptr, 128, 3072, 768, 768, 768, 3072, 0, STREAM));
  done(c, "fp8 C extent", fcmf_gemm_fp8(c.c, A0, BIAS, B0, BIAS, C0, nullptr, nullptr, nullptr, 49152, 64008, 768, 768, 768, 64008, 0, STREAM));
  done(c, "fp8 empty", fcmf_gemm_fp8(c.c, A0, BIAS, B0, BIAS, C0, nullptr, nullptr, nullptr, 0, 3072, 768, 768, 768, 3072, 0, STREAM));
}

int main(int argc, char** argv) {
  static char buf[1 << 22];
  setvbuf(stdout, buf, _IOFBF, sizeof buf);
  add_ctx("null", false, 0);
  add_ctx("no-ws", true, 0);
  add_ctx("ws256M", true, 256ll << 20);
  add_ctx("ws1M", true, 1ll << 20);
  for (int tile : {0, 128, 192, 256}) for (int kb : {32, 64}) for (int cus : {64, 256}) {
    char tag[48];
    snprintf(tag, sizeof tag, "tune%d/kb%d/cu%d", tile, kb, cus);
    add_ctx(tag, true, 256ll << 20, tile, kb, cus);
  }
  // `gemm_dispatch_probe FIRST COUNT` runs the contexts FIRST .. FIRST + COUNT - 1 only (to spread the sweep over processes)
  const int first = argc > 2 ? atoi(argv[1]) : 0, count = argc > 2 ? atoi(argv[2]) : g_nctx;
  for (int i = first; i < first + count && i < g_nctx; ++i) {
    sweep_gemm(g_ctx[i], 0);
    // (misaligned / odd-ld operands go to the generic kernel, whose plan reads no context setting: two contexts cover them)
    if (i == 0 || i == 2) { sweep_gemm(g_ctx[i], 1); sweep_gemm(g_ctx[i], 2); }
    sweep_rest(g_ctx[i]);
  }
  print_summary();
  return 0;
}
