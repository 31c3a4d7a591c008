// Tile images, MFMA operand fragments and the parameter block shared by the MFMA attention kernels (attn_mfma.hip: up to
// 256 keys resident in LDS; attn_long.hip: any number of keys streamed through it).  bf16, head dim 64, 256-thread workgroups.
#pragma once
#include "common.h"

constexpr int AD = 64;             // head dim
constexpr int AT = 128;            // tile rows (queries / keys)
constexpr int TILE_B = AT * AD * 2;  // 16 KiB

// [rows][64 bf16] tile, 128-B rows: 32-B pair index XOR ((r>>1)&1 | ((r>>3)&1)<<1)
__device__ __forceinline__ int vkey(int r) { return ((r >> 1) & 1) | (((r >> 3) & 1) << 1); }
__device__ __forceinline__ int off64(int r, int c8) { return r * 128 + ((((c8 >> 1) ^ vkey(r))) << 5) + ((c8 & 1) << 4); }
// [32 keys][128 q bf16] chunk images of the backward (Pdrop^T, dS^T), 256-B rows: 16-B chunk XOR key16(row & 15), a GF(2)-linear key
// (bit columns 2, 4, 8, 9) under which BOTH read patterns are conflict free -- the ds_read_b128 operand reads of phase 2 (row = lane & 15,
// chunk = 4 s + (lane >> 4)) and the ds_read_b64_tr_b16 reads of dS^T (tools/lds_conflicts.py searches the 4 x 4 bit matrices; the
// ds_write_b64 of phase 1 puts 16 rows of one column into a 128-B bank window and is 2-way under any key).  The round-3 key
// ((r & 3) << 2 | (r >> 2) & 3) left every operand read 2-way: 30 % of the kernel's LDS cycles were bank conflicts (r03_attn_pmc.txt).
__device__ __forceinline__ int key16(int r) { return ((r & 7) << 1) ^ (((r >> 3) & 1) * 9); }
__device__ __forceinline__ int off128(int r, int ch) { return r * 256 + ((ch ^ key16(r)) << 4); }
// per-wave P tile of the forward [32][128 bf16]: chunk XOR (row & 15)
__device__ __forceinline__ int offp(int r, int ch) { return r * 256 + ((ch ^ (r & 15)) << 4); }

// forward-only V image: 32-B pair index XOR ((r>>1)&3), conflict free for the KEY-PERMUTED transposed reads
// (k-slot j of k-step s = key 32s + 4*(lane>>4) + (j&3) + 16*(j>>2): the order in which the S^T accumulator
// registers of two adjacent key fragments line up as an MFMA operand, so P never leaves the registers)
__device__ __forceinline__ int off64p(int r, int c8) { return r * 128 + ((((c8 >> 1) ^ ((r >> 1) & 3))) << 5) + ((c8 & 1) << 4); }

typedef bf16x4 __attribute__((address_space(3))) * lds_v4_t;

// stage a [rows<=128][64] bf16 tile (row stride ld elements) into the off64 image, zero-filling
__device__ __forceinline__ void stage_tile(char* lds, const bf16_t* __restrict__ src, int64_t ld, int rows, int tid) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = tid + 256 * i, r = c >> 3, c8 = c & 7;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (r < rows) v = *reinterpret_cast<const uint4*>(src + (int64_t)r * ld + c8 * 8);
    *reinterpret_cast<uint4*>(lds + off64(r, c8)) = v;
  }
}
__device__ __forceinline__ void stage_tile_p(char* lds, const bf16_t* __restrict__ src, int64_t ld, int rows, int tid) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = tid + 256 * i, r = c >> 3, c8 = c & 7;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (r < rows) v = *reinterpret_cast<const uint4*>(src + (int64_t)r * ld + c8 * 8);
    *reinterpret_cast<uint4*>(lds + off64p(r, c8)) = v;
  }
}
// A[row = tile column c0 + (lane&15)][k = keys in the permuted order above] from the off64p image
__device__ __forceinline__ bf16x8 frag_tr64p(const char* lds, int c0, int s, int lane) {
  const int g4 = lane >> 4, i16 = lane & 15, q4 = i16 >> 2, p = i16 & 3;
  const int r = 32 * s + 4 * g4 + q4, c8 = (c0 >> 3) + (p >> 1);
  bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_v4_t)(lds + off64p(r, c8) + (p & 1) * 8));
  bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_v4_t)(lds + off64p(r + 16, c8) + (p & 1) * 8));
  bf16x8 o;
  o[0] = lo[0]; o[1] = lo[1]; o[2] = lo[2]; o[3] = lo[3]; o[4] = hi[0]; o[5] = hi[1]; o[6] = hi[2]; o[7] = hi[3];
  return o;
}
// the same staging in two halves, so that a kernel can put ALL its tile loads in flight before the first LDS write
// (the fused form exposes one global round trip per tile)
struct TileRegs { uint4 v[4]; };
__device__ __forceinline__ TileRegs load_tile(const bf16_t* __restrict__ src, int64_t ld, int rows, int tid) {
  TileRegs t;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = tid + 256 * i, r = c >> 3, c8 = c & 7;
    t.v[i] = make_uint4(0, 0, 0, 0);
    if (r < rows) t.v[i] = *reinterpret_cast<const uint4*>(src + (int64_t)r * ld + c8 * 8);
  }
  return t;
}
// load_tile without a branch per piece: a row past the end reads the last valid row of the matrix instead (src[(rows - 1) * ld]
// must exist; rows may be <= 0 for a tile that starts past the end, as long as the matrix has a row before it) and zero_tail()
// clears it before store_tile.  hipcc turns every conditional piece of load_tile into a branch and gives up counting across them:
// it drains the loads in flight (vmcnt(0)) in the middle of a batch.  Unconditional loads stay one batch with one wait.
__device__ __forceinline__ TileRegs load_tile_clamped(const bf16_t* __restrict__ src, int64_t ld, int rows, int tid) {
  TileRegs t;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = tid + 256 * i, r = c >> 3, c8 = c & 7;
    t.v[i] = *reinterpret_cast<const uint4*>(src + (int64_t)min(r, rows - 1) * ld + c8 * 8);
  }
  return t;
}
__device__ __forceinline__ void zero_tail(TileRegs& t, int rows, int tid) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (((tid + 256 * i) >> 3) >= rows) t.v[i] = make_uint4(0, 0, 0, 0);
}
template <bool PERMUTED>
__device__ __forceinline__ void store_tile(char* lds, const TileRegs& t, int tid) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = tid + 256 * i, r = c >> 3, c8 = c & 7;
    *reinterpret_cast<uint4*>(lds + (PERMUTED ? off64p(r, c8) : off64(r, c8))) = t.v[i];
  }
}
// MFMA operand (rows x0..x0+15, k-step s over the 64 columns) by row read
__device__ __forceinline__ bf16x8 frag_row64(const char* lds, int x0, int s, int lane) {
  return *reinterpret_cast<const bf16x8*>(lds + off64(x0 + (lane & 15), 4 * s + (lane >> 4)));
}
// MFMA operand whose "row" index is the tile COLUMN (c0..c0+15) and whose k index is the tile ROW
// (32*s .. 32*s+31): transposed read of the row-major image
__device__ __forceinline__ bf16x8 frag_tr64(const char* lds, int c0, int s, int lane) {
  const int g4 = lane >> 4, i16 = lane & 15, q4 = i16 >> 2, p = i16 & 3;
  const int r = 32 * s + 8 * g4 + q4, c8 = (c0 >> 3) + (p >> 1);
  bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_v4_t)(lds + off64(r, c8) + (p & 1) * 8));
  bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_v4_t)(lds + off64(r + 4, c8) + (p & 1) * 8));
  bf16x8 o;
  o[0] = lo[0]; o[1] = lo[1]; o[2] = lo[2]; o[3] = lo[3]; o[4] = hi[0]; o[5] = hi[1]; o[6] = hi[2]; o[7] = hi[3];
  return o;
}
__device__ __forceinline__ bf16x8 frag_row128(const char* lds, int x0, int s, int lane) {
  return *reinterpret_cast<const bf16x8*>(lds + off128(x0 + (lane & 15), 4 * s + (lane >> 4)));
}
__device__ __forceinline__ bf16x8 frag_tr128(const char* lds, int c0, int s, int lane) {
  const int g4 = lane >> 4, i16 = lane & 15, q4 = i16 >> 2, p = i16 & 3;
  const int r = 32 * s + 8 * g4 + q4, ch = (c0 >> 3) + (p >> 1);
  bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_v4_t)(lds + off128(r, ch) + (p & 1) * 8));
  bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_v4_t)(lds + off128(r + 4, ch) + (p & 1) * 8));
  bf16x8 o;
  o[0] = lo[0]; o[1] = lo[1]; o[2] = lo[2]; o[3] = lo[3]; o[4] = hi[0]; o[5] = hi[1]; o[6] = hi[2]; o[7] = hi[3];
  return o;
}
__device__ __forceinline__ void store4(bf16_t* p, f32x4 v) {
  bf16x4 o;
  o[0] = (bf16_t)v[0]; o[1] = (bf16_t)v[1]; o[2] = (bf16_t)v[2]; o[3] = (bf16_t)v[3];
  *reinterpret_cast<bf16x4*>(p) = o;
}

// sum over the 16 lanes of a DPP row (lanes 16i .. 16i+15), result in every lane: four row rotations as DPP operands of
// the adds -- no LDS crossbar traffic (ds_bpermute), which a __shfl_xor butterfly would cost
__device__ __forceinline__ float row16_sum(float x) {
#define FCMF_ROR_ADD(n) x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x120 + (n), 0xf, 0xf, true))
  FCMF_ROR_ADD(8); FCMF_ROR_ADD(4); FCMF_ROR_ADD(2); FCMF_ROR_ADD(1);
#undef FCMF_ROR_ADD
  return x;
}

struct AttnMfmaParams {
  const bf16_t *q, *k, *v, *o, *dout;
  const float* mask;
  bf16_t *out, *dq, *dk, *dv;
  float* lse;
  float* colsum;       // backward, optional: [G][3 * heads * 64] f32, row g = column sums of dq | dk | dv of sequence g
  int G, heads, Tq, Tk;
  int64_t ldq, ldk, ldo;
  float scale, p;
  uint64_t seed;
};

// Q fragments of the wave's 32 query rows straight from global memory in operand layout (16 B per lane)
__device__ __forceinline__ void load_q_frags(const AttnMfmaParams& P, int g, int h, int q0, int lane, bf16x8 (&qf)[2][2]) {
#pragma unroll
  for (int f = 0; f < 2; ++f)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int row = q0 + 16 * f + (lane & 15);
      uint4 v = make_uint4(0, 0, 0, 0);
      if (row < P.Tq) v = *reinterpret_cast<const uint4*>(P.q + ((int64_t)g * P.Tq + row) * P.ldq + h * AD + 32 * s + 8 * (lane >> 4));
      qf[f][s] = *reinterpret_cast<bf16x8*>(&v);
    }
}
// the same without a branch per fragment (see load_tile_clamped): rows past Tq read row Tq - 1; zero_q_tail() clears them
__device__ __forceinline__ void load_q_frags_clamped(const AttnMfmaParams& P, int g, int h, int q0, int lane, bf16x8 (&qf)[2][2]) {
#pragma unroll
  for (int f = 0; f < 2; ++f)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int row = min(q0 + 16 * f + (lane & 15), P.Tq - 1);
      const uint4 v = *reinterpret_cast<const uint4*>(P.q + ((int64_t)g * P.Tq + row) * P.ldq + h * AD + 32 * s + 8 * (lane >> 4));
      qf[f][s] = *reinterpret_cast<const bf16x8*>(&v);
    }
}
__device__ __forceinline__ void zero_q_tail(const AttnMfmaParams& P, int q0, int lane, bf16x8 (&qf)[2][2]) {
#pragma unroll
  for (int f = 0; f < 2; ++f)
    if (q0 + 16 * f + (lane & 15) >= P.Tq) {
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j) qf[f][s][j] = (bf16_t)0.f;
    }
}
