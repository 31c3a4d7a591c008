// CPU-only probe of the VALU attention's host dispatch (csrc/attn_small.hip): calls fcmf_attn_small_fwd / _bwd / _bwd_grouped with
// descriptors of fake device addresses and prints, for every call, the return code and every launch the call made -- host stub,
// grid, block, dynamic LDS, the dynamic-LDS limit in force (hip_launch_stubs.h) and every field of the AttnK parameter block.
// Two builds of attn_small.hip dispatch alike exactly when their dumps are byte-identical.
//
// Build and run (no GPU needed), from csrc/ after `make attn_small.o`:
//   clang++ -std=c++17 -O1 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -I../../include -I../../tools -c ../../tools/attn_small_dispatch_probe.cpp -o aprobe.o
//   hipcc --offload-arch=gfx950 -rdynamic aprobe.o attn_small.o -ldl -o attn_small_dispatch_probe
//   ./attn_small_dispatch_probe | sha256sum     # the dump (about 9 GB); the summary (counts per stub and return code) goes to stderr
//   ./attn_small_dispatch_probe cases           # only the rows given on stdin (one "G R heads d T1 T2 group_div mask bias causal" per
//                                               # line, as tests/test_ops_gpu.py's ATTN_CASES), both dtypes, variants 0 and 2
// AttnK below mirrors attn_small.hip: keep it in step with it.
#include "fcmf_hip.h"
#include "hip_launch_stubs.h"

struct AttnK {
  fcmf_attn_desc a;
  void* out; float* lse;
  const void* dout; const void* o_in;
  void *dq, *dk1, *dv1, *dk2, *dv2; float* dbias;
  float *pd2, *ds2;
  int RB, TLP, KVF;
};

static void print_launch_params(const std::string&, void** args) {
  const AttnK& p = *(AttnK*)args[0];
  const fcmf_attn_desc& a = p.a;
  printf("   dtype=%d G=%d heads=%d d=%d R=%d T1=%d T2=%d gd=%d q_sg=%lld q_sr=%lld k1_sg=%lld k1_st=%lld k2_sg=%lld k2_sr=%lld k2_st=%lld o_sg=%lld o_sr=%lld"
         " q=%p k1=%p v1=%p k2=%p v2=%p mask=%p bias=%p scale=%a p=%a seed=%llu causal=%d quirk=%d",
         a.dtype, a.G, a.heads, a.d, a.R, a.T1, a.T2, a.group_div, (long long)a.q_sg, (long long)a.q_sr, (long long)a.k1_sg, (long long)a.k1_st,
         (long long)a.k2_sg, (long long)a.k2_sr, (long long)a.k2_st, (long long)a.o_sg, (long long)a.o_sr, a.q, a.k1, a.v1, a.k2, a.v2,
         (void*)a.mask, (void*)a.bias, a.scale, a.dropout_p, (unsigned long long)a.seed, a.causal, a.head_quirk);
  printf(" out=%p lse=%p dout=%p o_in=%p dq=%p dk1=%p dv1=%p dk2=%p dv2=%p dbias=%p pd2=%p ds2=%p RB=%d TLP=%d KVF=%d", p.out, (void*)p.lse,
         p.dout, p.o_in, p.dq, p.dk1, p.dv1, p.dk2, p.dv2, (void*)p.dbias, (void*)p.pd2, (void*)p.ds2, p.RB, p.TLP, p.KVF);
}

static char* const Q0 = (char*)0x10000000, * const K1 = (char*)0x20000000, * const V1 = (char*)0x28000000, * const K2 = (char*)0x30000000,
           * const V2 = (char*)0x38000000, * const OUT = (char*)0x40000000, * const DOUT = (char*)0x48000000, * const DQ = (char*)0x50000000,
           * const DK1 = (char*)0x58000000, * const DV1 = (char*)0x60000000, * const DK2 = (char*)0x68000000, * const DV2 = (char*)0x70000000;
static float* const MASK = (float*)0x78000000, * const BIAS = (float*)0x80000000, * const LSE = (float*)0x88000000,
            * const DBIAS = (float*)0x90000000, * const SCRATCH = (float*)0x98000000;
static void* const STREAM = (void*)0x1000;

// variant 0: dense strides, aligned addresses; 1: row strides that are no multiple of 8; 2: out / dq off by 2 bytes; 3: q off by 2 bytes
static fcmf_attn_desc make_desc(int dtype, int G, int R, int heads, int d, int T1, int T2, int gd, bool mask, bool bias, bool causal, bool quirk,
                                bool kv_same, int variant) {
  fcmf_attn_desc a{};
  const int64_t HD = (int64_t)heads * d + (variant == 1 ? 3 : 0);
  a.dtype = dtype; a.G = G; a.heads = heads; a.d = d; a.R = R; a.T1 = T1; a.T2 = T2; a.group_div = gd;
  a.q_sr = HD; a.q_sg = R * HD;
  a.k1_st = HD; a.k1_sg = T1 * HD;
  a.k2_st = HD; a.k2_sr = T2 * HD; a.k2_sg = (int64_t)R * T2 * HD;
  a.o_sr = (int64_t)heads * d; a.o_sg = R * a.o_sr;
  a.q = Q0 + (variant == 3 ? 2 : 0);
  if (T1) { a.k1 = K1; a.v1 = kv_same ? K1 : V1; }
  if (T2) { a.k2 = K2; a.v2 = V2; }
  a.mask = mask ? MASK : nullptr; a.bias = bias ? BIAS : nullptr;
  a.scale = 0.125f; a.dropout_p = 0.1f; a.seed = 1234; a.causal = causal; a.head_quirk = quirk;
  return a;
}
static void done(const char* what, int rc) {
  printf("%s rc=%d\n", what, rc);
  ++g_count["rc " + std::to_string(rc)];
}
// the forward, and the backward with / without dbias, dv1 (NULL: v1 == k1) and the grouped entry point
static void calls(const char* tag, int dtype, int G, int R, int heads, int d, int T1, int T2, int gd, int flags, int variant) {
  const bool mask = flags & 1, bias = flags & 2, causal = flags & 4, quirk = flags & 8;
  char what[200];
  const int off = variant == 2 ? 2 : 0;
  fcmf_attn_desc a = make_desc(dtype, G, R, heads, d, T1, T2, gd, mask, bias, causal, quirk, false, variant);
  snprintf(what, sizeof what, "%s fwd t%d G%d R%d h%d d%d T%d+%d gd%d f%d v%d", tag, dtype, G, R, heads, d, T1, T2, gd, flags, variant);
  done(what, fcmf_attn_small_fwd(&a, OUT + off, LSE, STREAM));
  for (int opt = 0; opt < 8; ++opt) {
    const bool dbias = opt & 1, dv1 = !(opt & 2), grouped = opt & 4;
    a = make_desc(dtype, G, R, heads, d, T1, T2, gd, mask, bias, causal, quirk, !dv1, variant);
    snprintf(what, sizeof what, "%s bwd t%d G%d R%d h%d d%d T%d+%d gd%d f%d v%d o%d", tag, dtype, G, R, heads, d, T1, T2, gd, flags, variant, opt);
    void* dk1 = T1 ? DK1 : nullptr; void* pdv1 = T1 && dv1 ? DV1 : nullptr;
    void* dk2 = T2 ? DK2 : nullptr; void* dv2 = T2 ? DV2 : nullptr;
    if (grouped)
      done(what, fcmf_attn_small_bwd_grouped(&a, OUT, DOUT, LSE, DQ + off, dk1, pdv1, dk2, dv2, dbias ? DBIAS : nullptr, SCRATCH, 1ll << 30, STREAM));
    else
      done(what, fcmf_attn_small_bwd(&a, OUT, DOUT, LSE, DQ + off, dk1, pdv1, dk2, dv2, dbias ? DBIAS : nullptr, STREAM));
  }
}

int main(int argc, char** argv) {
  static char buf[1 << 22];
  setvbuf(stdout, buf, _IOFBF, sizeof buf);
  if (argc > 1 && !strcmp(argv[1], "cases")) {
    int G, R, heads, d, T1, T2, gd, mask, bias, causal;
    while (scanf("%d %d %d %d %d %d %d %d %d %d", &G, &R, &heads, &d, &T1, &T2, &gd, &mask, &bias, &causal) == 10)
      for (int dtype : {FCMF_F32, FCMF_BF16}) for (int variant : {0, 2}) calls("case", dtype, G, R, heads, d, T1, T2, gd, mask | bias << 1 | causal << 2, variant);
    print_summary();
    return 0;
  }
  static const int Rs[] = {1, 7, 16, 17, 36, 64, 65, 100, 128, 129, 150};
  static const int T1s[] = {0, 6, 36, 64, 65, 100, 128, 130, 170, 256, 412};
  static const int T2s[] = {0, 2, 20, 36, 49, 70, 128};
  static const int ds[] = {12, 16, 20, 32, 64, 96, 128};
  static const int gds[] = {1, 2, 6, 16};
  for (int dtype : {FCMF_F32, FCMF_BF16}) for (int R : Rs) for (int T1 : T1s) for (int T2 : T2s) for (int d : ds) for (int gd : gds)
    for (int flags = 0; flags < 16; ++flags) for (int variant = 0; variant < 4; ++variant)
      calls("sweep", dtype, 48, R, 3, d, T1, T2, gd, flags, variant);      // 48 groups: a multiple of every group_div
  // beyond the grid: bad descriptors, a scratch that is too small, more keys than the LDS holds, a group's scratch rows past 150 KiB
  fcmf_attn_desc a = make_desc(FCMF_F32, 4, 8, 2, 128, 512, 0, 1, false, false, false, false, false, 0);
  done("f32 512 keys d128 fwd", fcmf_attn_small_fwd(&a, OUT, LSE, STREAM));
  done("null out", fcmf_attn_small_fwd(&a, nullptr, LSE, STREAM));
  done("null desc", fcmf_attn_small_fwd(nullptr, OUT, LSE, STREAM));
  a = make_desc(FCMF_F64, 4, 8, 2, 64, 16, 0, 1, false, false, false, false, false, 0);
  done("f64", fcmf_attn_small_fwd(&a, OUT, LSE, STREAM));
  a = make_desc(FCMF_BF16, 4, 8, 2, 64, 400, 128, 1, false, false, false, false, false, 0);
  done("528 keys", fcmf_attn_small_fwd(&a, OUT, LSE, STREAM));
  a = make_desc(FCMF_BF16, 16, 7, 40, 64, 128, 128, 8, true, false, false, false, false, 0);
  done("grouped 40 heads", fcmf_attn_small_bwd_grouped(&a, OUT, DOUT, LSE, DQ, DK1, DV1, DK2, DV2, nullptr, SCRATCH, 1ll << 30, STREAM));
  a = make_desc(FCMF_BF16, 12, 7, 3, 64, 128, 36, 6, true, false, false, false, false, 0);
  done("grouped small scratch", fcmf_attn_small_bwd_grouped(&a, OUT, DOUT, LSE, DQ, DK1, DV1, DK2, DV2, nullptr, SCRATCH, 1024, STREAM));
  done("grouped null scratch", fcmf_attn_small_bwd_grouped(&a, OUT, DOUT, LSE, DQ, DK1, DV1, DK2, DV2, nullptr, nullptr, 0, STREAM));
  done("bwd null dk2", fcmf_attn_small_bwd(&a, OUT, DOUT, LSE, DQ, DK1, DV1, nullptr, DV2, nullptr, STREAM));
  done("bwd null dv1, v1 != k1", fcmf_attn_small_bwd(&a, OUT, DOUT, LSE, DQ, DK1, nullptr, DK2, DV2, nullptr, STREAM));
  print_summary();
  return 0;
}
