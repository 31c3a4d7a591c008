// The HIP runtime calls a dispatch probe intercepts (tools/gemm_dispatch_probe.cpp, tools/attn_small_dispatch_probe.cpp): they are
// defined HERE, in the executable, and so take precedence over the runtime's -- nothing reaches a device and no address is
// dereferenced.  Every launch is printed as host stub, grid, block, dynamic LDS, the dynamic-LDS limit in force for that kernel
// (-1: never raised) and the stream; the probe that includes this header prints the kernel's parameters by name in
// print_launch_params.  Include it in exactly one translation unit of a probe.
#pragma once
#include <hip/hip_runtime_api.h>
#include <dlfcn.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

static void print_launch_params(const std::string& stub, void** args);   // the probe's own: no newline at the end

static std::map<const void*, int> g_attr;            // kernel -> dynamic-LDS limit last set
static std::map<std::string, long> g_count;          // summary (written to stderr by print_summary)
static dim3 g_grid, g_block; static size_t g_smem; static hipStream_t g_stream;

static std::string stub_name(const void* f) {
  Dl_info di;
  if (dladdr(f, &di) && di.dli_sname) return di.dli_sname;
  static std::map<const void*, int> seen;
  return "kernel#" + std::to_string(seen.emplace(f, (int)seen.size()).first->second);
}
static void print_summary() {
  fflush(stdout);
  for (const auto& kv : g_count) fprintf(stderr, "%10ld  %s\n", kv.second, kv.first.c_str());
}

extern "C" hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t smem, hipStream_t st) {
  g_grid = grid; g_block = block; g_smem = smem; g_stream = st;
  return hipSuccess;
}
extern "C" hipError_t __hipPopCallConfiguration(dim3* grid, dim3* block, size_t* smem, hipStream_t* st) {
  *grid = g_grid; *block = g_block; *smem = g_smem; *st = g_stream;
  return hipSuccess;
}
extern "C" hipError_t hipFuncSetAttribute(const void* f, hipFuncAttribute attr, int value) {
  if (attr == hipFuncAttributeMaxDynamicSharedMemorySize) g_attr[f] = value;
  return hipSuccess;
}
extern "C" hipError_t hipGetLastError(void) { return hipSuccess; }
// the table upload of a weight-gradient list: staging memory from the heap, events that are always complete, and the copy printed
// as its size and an FNV-1a hash of what it carries (the matrices, the items and the reduce table)
extern "C" hipError_t hipHostMalloc(void** p, size_t n, unsigned) { *p = malloc(n); return *p ? hipSuccess : hipErrorOutOfMemory; }
extern "C" hipError_t hipHostFree(void* p) { free(p); return hipSuccess; }
extern "C" hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { *e = (hipEvent_t)malloc(1); return hipSuccess; }
extern "C" hipError_t hipEventDestroy(hipEvent_t e) { free((void*)e); return hipSuccess; }
extern "C" hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }
extern "C" hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
extern "C" hipError_t hipMemcpyAsync(void* dst, const void* src, size_t n, hipMemcpyKind, hipStream_t) {
  unsigned long long h = 1469598103934665603ull;
  for (size_t i = 0; i < n; ++i) h = (h ^ ((const unsigned char*)src)[i]) * 1099511628211ull;
  printf("  upload %p %zu bytes fnv=%016llx\n", dst, n, h);
  return hipSuccess;
}
extern "C" hipError_t hipMemsetAsync(void* p, int v, size_t n, hipStream_t) { printf("  memset %p %d %zu\n", p, v, n); return hipSuccess; }
extern "C" hipError_t hipLaunchKernel(const void* f, dim3 g, dim3 b, void** a, size_t smem, hipStream_t st) {
  const std::string name = stub_name(f);
  ++g_count["launch " + name];
  printf("  %s grid=(%u,%u,%u) block=%u smem=%zu attr=%d stream=%p\n", name.c_str(), g.x, g.y, g.z, b.x, smem, g_attr.count(f) ? g_attr[f] : -1, (void*)st);
  print_launch_params(name, a);
  printf("\n");
  return hipSuccess;
}
