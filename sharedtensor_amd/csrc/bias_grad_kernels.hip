// Bias gradients taken in the pass that already streams the data.
//
//   k_gelu_bwd_colsum  dx = bf16(dy * gelu'(x)) and the column sums of the
//                      rounded dx (fc.bias.grad) in one pass
//   k_pack3_colsum     dst[r, s*C + c] = src_s[r, c] for three (R, C) sources
//                      and the 3C column sums of what was copied
//                      (the backward of qkv.split plus qkv.bias.grad)
//   k_bg_reduce        per-block partial rows -> bf16 column sums
//
// Layout.  The N columns are N/8 column groups of 8 bf16 (one 16-byte
// access).  A 1024-thread block is CT column threads x RT = 1024/CT row
// threads; blockIdx.x picks a tile of CT column groups, blockIdx.y a set of
// rows, and the grid strides over rows.  A thread therefore meets the same 8
// columns in every row it visits and keeps their sums in 8 fp32 registers.
// At the end the RT row threads of a block that share columns are added in
// row-thread order through LDS, and the block writes one fp32 partial row of
// its CT*8 columns: partial is (gridDim.y, N).  The grid is capped at
// BG_TARGET_BLOCKS, so the partials stay below 2 MB for any N up to the cap
// and the second stage is a few microseconds.  Everything is summed in a
// fixed order and there are no atomics: the sums repeat bit for bit.
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#include "device_util.h"
#include "gelu_math.h"
#include "hip_api.h"

namespace shamd {

constexpr int BG_THREADS = 1024;
// Grid cap: two resident blocks on each of MI355X's 256 CUs.  A constant,
// not a device query, so that the partials buffer has a fixed bound and the
// summation order is the same on every device; the row loop strides, so a
// device with fewer CUs runs the same grid in more rounds.
constexpr int BG_TARGET_BLOCKS = 512;
constexpr int BG_MAX_CT = 128;         // 2 KB of a row per block and row
// rows a thread has in flight per loop iteration.  A second row costs the
// GELU kernel 16 registers, which takes it past 64 and to one block per CU;
// the copy has them to spare.
constexpr int BG_GELU_ROWS = 1;
constexpr int BG_PACK_ROWS = 2;

struct BgGeom {
  int ct_shift;   // log2(column threads)
  int gx, gy;     // column tiles, row sets
};

// Depends on R and N alone, so the summation order is the same from call to
// call and from device to device.
static BgGeom bg_geom(int64_t R, int64_t n8, int rows) {
  // the largest power of two that divides the column groups fills every
  // lane; widths where that is below 16 get 16 lanes with some idle
  int shift = 0;
  while ((2 << shift) <= BG_MAX_CT && n8 % (2 << shift) == 0) ++shift;
  if (shift < 4) {
    shift = 0;
    while (shift < 4 && (1 << shift) < n8) ++shift;
  }
  BgGeom g;
  g.ct_shift = shift;
  const int ct = 1 << shift, rt = BG_THREADS >> shift;
  const int64_t gx = (n8 + ct - 1) / ct;
  if (gx > 65535) throw std::runtime_error("bias_grad: too many columns");
  g.gx = static_cast<int>(gx);
  int gymax = BG_TARGET_BLOCKS / g.gx;
  if (gymax < 1) gymax = 1;
  // a block takes `rows` rows per row thread and loop iteration
  const int64_t need = (R + rows * rt - 1) / (rows * rt);
  g.gy = static_cast<int>(need < gymax ? (need > 0 ? need : 1) : gymax);
  return g;
}

static __device__ __forceinline__ void bg_acc(float* a, const uint4& o) {
  const uint32_t* op = &o.x;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    a[2 * k] += bf16x2_lo(op[k]);
    a[2 * k + 1] += bf16x2_hi(op[k]);
  }
}

// Adds the row threads of the block column by column, row thread 0 first,
// and writes the block's partial row.  Every thread of the block calls it.
static __device__ __forceinline__ void bg_block_partial(
    const float* a, float* red, float* __restrict__ partial, int ct_shift,
    int64_t N) {
  float4* r4 = reinterpret_cast<float4*>(red);
  r4[2 * threadIdx.x] = make_float4(a[0], a[1], a[2], a[3]);
  r4[2 * threadIdx.x + 1] = make_float4(a[4], a[5], a[6], a[7]);
  __syncthreads();
  const int w = 8 << ct_shift;              // columns of the tile
  const int rt = BG_THREADS >> ct_shift;
  const int j = threadIdx.x;
  const int64_t col = static_cast<int64_t>(blockIdx.x) * w + j;
  if (j < w && col < N) {
    float t = 0.f;
    for (int y = 0; y < rt; ++y) t += red[y * w + j];
    partial[static_cast<int64_t>(blockIdx.y) * N + col] = t;
  }
}

static __device__ __forceinline__ uint4 bg_gelu_bwd8(const uint4& d,
                                                     const uint4& u) {
  uint4 o;
  const uint32_t* up = &u.x;
  const uint32_t* dp = &d.x;
  uint32_t* op = &o.x;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    op[k] = bf16x2_pack(bf16x2_lo(dp[k]) * gelu_grad_f(bf16x2_lo(up[k])),
                        bf16x2_hi(dp[k]) * gelu_grad_f(bf16x2_hi(up[k])));
  return o;
}

__global__ __launch_bounds__(BG_THREADS) void k_gelu_bwd_colsum(
    const uint4* __restrict__ dy, const uint4* __restrict__ x,
    uint4* __restrict__ dx, float* __restrict__ partial, int64_t R,
    int64_t n8, int ct_shift) {
  __shared__ float red[BG_THREADS * 8];
  const int cx = threadIdx.x & ((1 << ct_shift) - 1);
  const int ty = threadIdx.x >> ct_shift;
  const int rt = BG_THREADS >> ct_shift;
  const int64_t cj = (static_cast<int64_t>(blockIdx.x) << ct_shift) + cx;
  float a[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) a[k] = 0.f;
  if (cj < n8) {
    const int64_t stride = static_cast<int64_t>(gridDim.y) * rt;
#pragma unroll 1
    for (int64_t r = static_cast<int64_t>(blockIdx.y) * rt + ty; r < R;
         r += stride) {
      const int64_t i = r * n8 + cj;
      const uint4 o = bg_gelu_bwd8(dy[i], x[i]);
      dx[i] = o;
      bg_acc(a, o);
    }
  }
  bg_block_partial(a, red, partial, ct_shift, n8 * 8);
}

// n8 counts the column groups of the destination (3 * C / 8), c8 those of
// one source.
__global__ __launch_bounds__(BG_THREADS) void k_pack3_colsum(
    const uint4* __restrict__ s0, const uint4* __restrict__ s1,
    const uint4* __restrict__ s2, uint4* __restrict__ dst,
    float* __restrict__ partial, int64_t R, int64_t c8, int ct_shift) {
  __shared__ float red[BG_THREADS * 8];
  const int cx = threadIdx.x & ((1 << ct_shift) - 1);
  const int ty = threadIdx.x >> ct_shift;
  const int rt = BG_THREADS >> ct_shift;
  const int64_t n8 = 3 * c8;
  const int64_t cj = (static_cast<int64_t>(blockIdx.x) << ct_shift) + cx;
  float a[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) a[k] = 0.f;
  if (cj < n8) {
    const int which = cj < c8 ? 0 : (cj < 2 * c8 ? 1 : 2);
    const uint4* __restrict__ src = which == 0 ? s0 : (which == 1 ? s1 : s2);
    const int64_t cs = cj - which * c8;
    const int64_t stride = static_cast<int64_t>(gridDim.y) * rt;
#pragma unroll 1
    for (int64_t r = static_cast<int64_t>(blockIdx.y) * rt + ty; r < R;
         r += 2 * stride) {
      const int64_t r1 = r + stride;
      const bool two = r1 < R;
      const int64_t ra = two ? r1 : r;
      const uint4 v0 = src[r * c8 + cs];
      const uint4 v1 = src[ra * c8 + cs];
      dst[r * n8 + cj] = v0;
      bg_acc(a, v0);
      if (two) {
        dst[r1 * n8 + cj] = v1;
        bg_acc(a, v1);
      }
    }
  }
  bg_block_partial(a, red, partial, ct_shift, n8 * 8);
}

// Sums the G partial rows column by column and writes bf16.  A block owns 32
// columns; its 8 row groups each sum every 8th partial row, then row group 0
// adds the 8 group sums in order.
__global__ __launch_bounds__(256) void k_bg_reduce(
    const float* __restrict__ partial, int G, int64_t N,
    uint16_t* __restrict__ out) {
  __shared__ float red[8][33];
  const int cg = threadIdx.x & 31, rg = threadIdx.x >> 5;
  const int64_t j = static_cast<int64_t>(blockIdx.x) * 32 + cg;
  float a = 0.f;
  if (j < N)
    for (int g = rg; g < G; g += 8) a += partial[static_cast<int64_t>(g) * N + j];
  red[rg][cg] = a;
  __syncthreads();
  if (rg == 0 && j < N) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) t += red[i][cg];
    out[j] = f32_to_bf16(t);
  }
}

static void bg_check_shape(int64_t R, int64_t N) {
  if (R <= 0) throw std::runtime_error("bias_grad: empty input");
  if (N <= 0 || N % 8)
    throw std::runtime_error("bias_grad: columns must be a multiple of 8");
}

int64_t hip_bias_grad_partial_floats(int64_t N) {
  // gy * N <= (BG_TARGET_BLOCKS / gx) * N <= BG_TARGET_BLOCKS * CT * 8, or a
  // single row of N when the column tiles alone exceed the target
  const int64_t cap = static_cast<int64_t>(BG_TARGET_BLOCKS) * BG_MAX_CT * 8;
  return N > cap ? N : cap;
}

int64_t hip_bias_grad_sweep_rows(int64_t R, int64_t N, bool pack) {
  bg_check_shape(R, N);
  const int rows = pack ? BG_PACK_ROWS : BG_GELU_ROWS;
  const BgGeom g = bg_geom(R, N / 8, rows);
  return rows * static_cast<int64_t>(g.gy) * (BG_THREADS >> g.ct_shift);
}

static void bg_reduce(const float* partial, int G, int64_t N, void* out,
                      hipStream_t s) {
  hipLaunchKernelGGL(k_bg_reduce, dim3(static_cast<uint32_t>((N + 31) / 32)),
                     dim3(256), 0, s, partial, G, N,
                     static_cast<uint16_t*>(out));
  HIP_CHECK(hipGetLastError());
}

void hip_gelu_bwd_colsum(const void* dy, const void* x, void* dx, void* db,
                         float* partial, int64_t R, int64_t C,
                         hipStream_t s) {
  bg_check_shape(R, C);
  check_align(dy, 16, "bias_grad", "dy");
  check_align(x, 16, "bias_grad", "x");
  check_align(dx, 16, "bias_grad", "dx");
  check_align(partial, 16, "bias_grad", "partial");
  if (!db) throw std::runtime_error("bias_grad: null db");
  const BgGeom g = bg_geom(R, C / 8, BG_GELU_ROWS);
  hipLaunchKernelGGL(k_gelu_bwd_colsum, dim3(g.gx, g.gy), dim3(BG_THREADS), 0,
                     s, static_cast<const uint4*>(dy),
                     static_cast<const uint4*>(x), static_cast<uint4*>(dx),
                     partial, R, C / 8, g.ct_shift);
  HIP_CHECK(hipGetLastError());
  bg_reduce(partial, g.gy, C, db, s);
}

void hip_pack3_colsum(const void* s0, const void* s1, const void* s2,
                      void* dst, void* db, float* partial, int64_t R,
                      int64_t C, hipStream_t s) {
  bg_check_shape(R, C);
  check_align(s0, 16, "bias_grad", "src0");
  check_align(s1, 16, "bias_grad", "src1");
  check_align(s2, 16, "bias_grad", "src2");
  check_align(dst, 16, "bias_grad", "dst");
  check_align(partial, 16, "bias_grad", "partial");
  if (!db) throw std::runtime_error("bias_grad: null db");
  const BgGeom g = bg_geom(R, 3 * C / 8, BG_PACK_ROWS);
  hipLaunchKernelGGL(k_pack3_colsum, dim3(g.gx, g.gy), dim3(BG_THREADS), 0, s,
                     static_cast<const uint4*>(s0),
                     static_cast<const uint4*>(s1),
                     static_cast<const uint4*>(s2), static_cast<uint4*>(dst),
                     partial, R, C / 8, g.ct_shift);
  HIP_CHECK(hipGetLastError());
  bg_reduce(partial, g.gy, 3 * C, db, s);
}

}  // namespace shamd
