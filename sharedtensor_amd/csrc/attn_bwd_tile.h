// Tile helpers of the attention backward kernels for head dim 64, shared by
// attn_bwd_kernels.hip (MHA) and gqa_attn_bwd_kernels.hip (GQA): the LDS tile
// swizzle, the two LDS read patterns that feed mfma_f32_32x32x16_bf16, the
// workgroup-to-XCD grid map and the staged whole-row epilogue, with and
// without the column sums of what it stores (MHA only).  The header
// comment of attn_bwd_kernels.hip derives the swizzle and the lane layouts.
// Everything sits in an anonymous namespace: each kernel file gets its own
// copy, inlined.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace shamd {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kD = 64;          // head dim
constexpr int kRW = 32;         // rows (queries or keys) per wave
constexpr int kWaves = 4;
constexpr int kRB = kRW * kWaves;  // rows per workgroup
constexpr int kTile = 64;       // rows per LDS tile
constexpr int kTileBytes = kTile * kD * 2;
constexpr int kXcd = 8;
constexpr float kLog2e = 1.4426950408889634f;

struct BwdStrides {
  int64_t b, t, h;  // elements
};

// the chunk swizzle of a row: f((row >> 1) & 7)
__device__ __forceinline__ int swz(int row) {
  int x = (row >> 1) & 7;
  return x ^ ((x & 1) << 2);
}
// byte offset of 16-byte chunk `ch` (0..7) of row `row` in a tile
__device__ __forceinline__ int t_off(int row, int ch) {
  return row * 128 + ((ch ^ swz(row)) << 4);
}

__device__ __forceinline__ u32x4 load16_or_zero(const uint16_t* p, bool ok) {
  u32x4 z = {0, 0, 0, 0};
  return ok ? *reinterpret_cast<const u32x4*>(p) : z;
}

// the other lane half's value (lane ^ 32)
__device__ __forceinline__ float other_half(float x, int lane) {
  return __builtin_bit_cast(
      float, __builtin_amdgcn_ds_bpermute((lane ^ 32) << 2,
                                          __builtin_bit_cast(int, x)));
}

// Per-lane parts of the two LDS read patterns.
struct LaneOffs {
  // row-wise A operand: row 32 blk + r, chunk 2 ks + hi -> row_ks[ks] +
  // 32 * 128 * blk (the swizzle depends on r alone)
  int row_ks[4];
  // transposed A operand: tr[p] is the lane's address for rows 0..3 + 4 hi
  // of a 16-row group and a column block nb with nb ^ jj == p (jj: second
  // 8 rows of the group, which flips bit 2 of the swizzle)
  int tr[2];
};

__device__ __forceinline__ LaneOffs lane_offs(int lane) {
  LaneOffs o;
  const int r = lane & 31, hi = lane >> 5;
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) o.row_ks[ks] = t_off(r, 2 * ks + hi);
  // 16-lane group g reads rows 4 (g >> 1) + 0..3, columns 16 (g & 1) + 0..15
  // of the 32-column block; lane 4 qq + p of the group supplies row qq,
  // columns 4 p .. 4 p + 3
  const int grp = lane >> 4, gi = lane & 15;
  const int tq = gi >> 2, tp = gi & 3;
  const int row = 4 * (grp >> 1) + tq;
#pragma unroll
  for (int p = 0; p < 2; ++p)
    o.tr[p] = t_off(row, 4 * p + 2 * (grp & 1) + (tp >> 1)) + 8 * (tp & 1);
  return o;
}

// A operand read row-wise: lane holds tile[32 blk + r][16 ks + 8 hi + j]
__device__ __forceinline__ bf16x8 row_frag(const unsigned char* tile,
                                           const LaneOffs& lo, int blk,
                                           int ks) {
  u32x4 t = *reinterpret_cast<const u32x4*>(tile + blk * (kRW * 128) +
                                            lo.row_ks[ks]);
  return __builtin_bit_cast(bf16x8, t);
}

// A operand read transposed: lane holds, as element j,
// tile[16 ss + 8 (j >> 2) + 4 hi + (j & 3)][32 nb + r], the row order the
// registers 8 (ss & 1) .. + 7 of a 32 x 32 mfma result have
__device__ __forceinline__ bf16x8 tr_frag(const unsigned char* tile,
                                          const LaneOffs& lo, int ss, int nb) {
  bf16x8 f;
#pragma unroll
  for (int jj = 0; jj < 2; ++jj) {
    // rows 16 ss + 8 jj + ..: (row >> 1) & 7 gains 4 jj, the swizzle flips
    // bit 2 of the chunk with jj, as nb does
    auto* a = reinterpret_cast<__attribute__((address_space(3))) s16x4*>(
        (uintptr_t)(tile + (16 * ss + 8 * jj) * 128 + lo.tr[nb ^ jj]));
    s16x4 tr = __builtin_amdgcn_ds_read_tr16_b64_v4i16(a);
    bf16x4 tb = __builtin_bit_cast(bf16x4, tr);
#pragma unroll
    for (int e = 0; e < 4; ++e) f[4 * jj + e] = tb[e];
  }
  return f;
}

// blockIdx -> (batch*head, block slot): block ids round-robin over the XCDs,
// the blocks of one (b, h) consecutive on one XCD
__device__ __forceinline__ bool grid_map(int nbh, int nblk, int& bh,
                                         int& slot_in_bh) {
  const int xcd = blockIdx.x % kXcd;
  const int slot = blockIdx.x / kXcd;
  bh = (slot / nblk) * kXcd + xcd;
  slot_in_bh = slot % nblk;
  return bh < nbh;
}

// fp32 rows of a wave -> bf16 through the wave's 4 KB of LDS -> whole-row
// global stores.  acc: lane holds row r, columns 32 nb + (reg & 3) +
// 8 (reg >> 2) + 4 hi.
__device__ __forceinline__ void stage_rows(unsigned char* Ow,
                                           const f32x16 (&acc)[2], float mul,
                                           int r, int hi) {
#pragma unroll
  for (int nb = 0; nb < 2; ++nb)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      bf16x4 f;
#pragma unroll
      for (int e = 0; e < 4; ++e) f[e] = (__bf16)(acc[nb][4 * g + e] * mul);
      // d = 32 nb + 8 g + 4 hi + e: chunk 4 nb + g, its half hi
      *reinterpret_cast<bf16x4*>(Ow + t_off(r, 4 * nb + g) + 8 * hi) = f;
    }
}

__device__ __forceinline__ void store_rows(const unsigned char* Ow,
                                           uint16_t* dst, int64_t row_stride,
                                           int row0, int T, int lane) {
#pragma unroll
  for (int pass = 0; pass < 4; ++pass) {
    int row = pass * 8 + (lane >> 3), ch = lane & 7;
    u32x4 val = *reinterpret_cast<const u32x4*>(Ow + t_off(row, ch));
    int gr = row0 + row;
    if (gr < T)
      *reinterpret_cast<u32x4*>(dst + (int64_t)gr * row_stride + 8 * ch) = val;
  }
}

// store_rows that also sums, per column, the bf16 values it stores.  A lane
// meets the same 16-byte chunk (8 columns) in all four passes, so the sums of
// its rows pass, pass + 8, ... live in cs[0..7], added in pass order.  Rows at
// or past T are neither stored nor summed.
__device__ __forceinline__ void store_rows_colsum(const unsigned char* Ow,
                                                  uint16_t* dst,
                                                  int64_t row_stride, int row0,
                                                  int T, int lane,
                                                  float (&cs)[8]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) cs[e] = 0.f;
#pragma unroll
  for (int pass = 0; pass < 4; ++pass) {
    int row = pass * 8 + (lane >> 3), ch = lane & 7;
    u32x4 val = *reinterpret_cast<const u32x4*>(Ow + t_off(row, ch));
    int gr = row0 + row;
    if (gr < T) {
      *reinterpret_cast<u32x4*>(dst + (int64_t)gr * row_stride + 8 * ch) = val;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        cs[2 * i] += __builtin_bit_cast(float, val[i] << 16);
        cs[2 * i + 1] += __builtin_bit_cast(float, val[i] & 0xffff0000u);
      }
    }
  }
}

// Column sums of a workgroup's NOUT staged outputs -> one fp32 partial row of
// 64 columns per output.  cs[o]: the lane's sums from store_rows_colsum.
// The 8 lanes of a wave that share a chunk (lane, lane ^ 8, ^ 16, ^ 32) are
// added as a butterfly: both sides of an exchange add the same two numbers,
// so every lane ends with the same bits.  Then each wave puts its NOUT x 64
// sums at the start of its own staging area (`wave_bytes` apart, its rows
// are read by then) and thread 64 o + c adds the four waves of column c of
// output o in wave order.  Every thread of the workgroup calls it.
template <int NOUT>
__device__ __forceinline__ void colsum_partial_rows(unsigned char* lds,
                                                    int wave_bytes, int wave,
                                                    int tid,
                                                    float (&cs)[NOUT][8],
                                                    float* const (&dst)[NOUT]) {
  const int lane = tid & 63;
#pragma unroll
  for (int m = 8; m < 64; m <<= 1)
#pragma unroll
    for (int o = 0; o < NOUT; ++o)
#pragma unroll
      for (int e = 0; e < 8; ++e)
        cs[o][e] += __builtin_bit_cast(
            float, __builtin_amdgcn_ds_bpermute(
                       (lane ^ m) << 2, __builtin_bit_cast(int, cs[o][e])));
  // orders the reads of the staged rows before the overwrite
  __syncthreads();
  if (lane < 8) {
    float* mine = reinterpret_cast<float*>(lds + wave * wave_bytes) + 8 * lane;
#pragma unroll
    for (int o = 0; o < NOUT; ++o) {
      f32x4 a = {cs[o][0], cs[o][1], cs[o][2], cs[o][3]};
      f32x4 b = {cs[o][4], cs[o][5], cs[o][6], cs[o][7]};
      *reinterpret_cast<f32x4*>(mine + kD * o) = a;
      *reinterpret_cast<f32x4*>(mine + kD * o + 4) = b;
    }
  }
  __syncthreads();
  if (tid < NOUT * kD) {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < kWaves; ++w)
      t += reinterpret_cast<const float*>(lds + w * wave_bytes)[tid];
    float* d = dst[0];
#pragma unroll
    for (int o = 1; o < NOUT; ++o)
      if (tid >= o * kD) d = dst[o];
    d[tid % kD] = t;
  }
}

}  // namespace
}  // namespace shamd
