// Fused residual-add + bf16 RMSNorm, forward and backward, for the Llama
// residual chain  x = x + f(rms(x)).
//
// The unfused chain moves 13 activations per RMSNorm (add: 3, rms fwd: 2,
// rms bwd dx: 3, rms bwd dw: 2, autograd's residual-gradient add: 3).
// These kernels move 8:
//   fwd:  reads x, delta            writes x_new = x + delta, y = RMS(x_new)
//   bwd:  reads dy, x_new, d_x_new  writes dx_total = RMS_dx(dy) + d_x_new
//         and accumulates dgamma in the same pass
//
// Layout: the one add_ln_kernels.hip uses, widened to 16-byte accesses.  One
// 64-lane wave owns a row; C = NV * 512, so a row is exactly NV x (64 lanes
// x 16 B), every lane issues NV uint4 loads per tensor and the row reduction
// is shuffle-only — no LDS, no barrier in the row loop.  In backward a lane
// owns the same 8*NV columns for every row of its grid-stride loop, so the
// dgamma column sums live in registers.  They leave the kernel as one fp32
// partial row per block; k_add_rms_reduce sums the partials in a fixed order
// and writes bf16 — no float atomics, no zero-fill, no cast kernel, so
// backward repeats bit for bit.
//
// Other widths keep using the block-per-row kernels in ln_kernels.hip.
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#include "device_util.h"
#include "hip_api.h"  // declaration parity check

namespace shamd {

// Hides a packed register group from the optimiser.  Without it the
// "recompute after the reduction" below is folded back into values kept
// across the reduction (and the weight's unpacking is hoisted out of the row
// loop), which doubles the register count and halves the occupancy.
static __device__ __forceinline__ void arms_opaque(uint4& p) {
  asm volatile("" : "+v"(p.x), "+v"(p.y), "+v"(p.z), "+v"(p.w));
}

constexpr int ARMS_THREADS = 256;      // 4 rows in flight per block
constexpr int ARMS_WAVES = ARMS_THREADS / 64;
constexpr int ARMS_MAX_BLOCKS = 1024;  // bounds the partials buffer
constexpr int ARMS_MAX_NV = 8;         // C = 512, 1024, ..., 4096

template <int NV>
__global__ __launch_bounds__(ARMS_THREADS) void k_add_rms_fwd(
    const uint16_t* __restrict__ x, const uint16_t* __restrict__ delta,
    const uint16_t* __restrict__ w, uint16_t* __restrict__ x_new,
    uint16_t* __restrict__ y, float* __restrict__ rstd, int64_t R, float eps) {
  constexpr int C = NV * 512;
  const int lane = threadIdx.x & 63;
  const int64_t r = static_cast<int64_t>(blockIdx.x) * ARMS_WAVES +
                    __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (r >= R) return;  // wave-uniform: whole wave leaves; no barrier below
  const uint4* xr = reinterpret_cast<const uint4*>(x + r * C);
  // the row stays packed (4 dwords per chunk); it is unpacked once for the
  // sum of squares and once more for y, which costs shifts, not registers
  uint4 px[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) px[k] = xr[k * 64 + lane];
  if (delta) {
    const uint4* dr = reinterpret_cast<const uint4*>(delta + r * C);
    uint4* xo = reinterpret_cast<uint4*>(x_new + r * C);
    uint4 pd[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) pd[k] = dr[k * 64 + lane];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      float a[8], d[8];
      unpack8(px[k], a);
      unpack8(pd[k], d);
#pragma unroll
      for (int j = 0; j < 8; ++j) a[j] += d[j];
      // statistics and y come from the rounded sum, as if x_new had been
      // written by a separate add and read back
      px[k] = pack8(a);
      xo[k * 64 + lane] = px[k];
    }
  }
  float q = 0.f;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    float v[8];
    unpack8(px[k], v);
#pragma unroll
    for (int j = 0; j < 8; ++j) q += v[j] * v[j];
  }
  const float rs = rsqrtf(wave_sum(q) * (1.f / C) + eps);
  if (lane == 0) rstd[r] = rs;
  uint4* yr = reinterpret_cast<uint4*>(y + r * C);
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    float v[8], ww[8], o[8];
    unpack8(px[k], v);
    unpack8(reinterpret_cast<const uint4*>(w)[k * 64 + lane], ww);
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = v[j] * rs * ww[j];
    yr[k * 64 + lane] = pack8(o);
  }
}

// Waves per SIMD the backward kernel is compiled for.  A lane needs 24
// registers per chunk (see the row loop); left alone, the scheduler spends
// twice that on instruction-level parallelism the memory system cannot use.
constexpr int arms_bwd_waves(int nv) { return nv <= 4 ? 4 : 2; }

// partial is (gridDim.x, C) fp32; every element is written, so it needs no
// zeroing.  DRES says whether dres (the residual-stream gradient) is there:
// a template parameter, so the row loop has no branch.
template <int NV, bool DRES>
__global__ __launch_bounds__(ARMS_THREADS)
__attribute__((amdgpu_waves_per_eu(arms_bwd_waves(NV)))) void k_add_rms_bwd(
    const uint16_t* __restrict__ dy, const uint16_t* __restrict__ xn,
    const uint16_t* __restrict__ w, const float* __restrict__ rstd,
    const uint16_t* __restrict__ dres, uint16_t* __restrict__ dx,
    float* __restrict__ partial, int64_t R) {
  constexpr int C = NV * 512;
  __shared__ float4 red[C / 4];
  const int lane = threadIdx.x & 63;
  // wave-uniform by construction; saying so keeps the row index and every
  // row base address in scalar registers
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float ag[NV][8];
#pragma unroll
  for (int k = 0; k < NV; ++k)
#pragma unroll
    for (int j = 0; j < 8; ++j) ag[k][j] = 0.f;
  uint4 pw[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k)
    pw[k] = reinterpret_cast<const uint4*>(w)[k * 64 + lane];
  const int64_t stride = static_cast<int64_t>(gridDim.x) * ARMS_WAVES;
#pragma unroll 1
  for (int64_t r = static_cast<int64_t>(blockIdx.x) * ARMS_WAVES + wave;
       r < R; r += stride) {
    const uint4* dyr = reinterpret_cast<const uint4*>(dy + r * C);
    const uint4* xr = reinterpret_cast<const uint4*>(xn + r * C);
    uint4 pg[NV], px[NV], pr[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) pg[k] = dyr[k * 64 + lane];
#pragma unroll
    for (int k = 0; k < NV; ++k) px[k] = xr[k * 64 + lane];
    if constexpr (DRES) {
      const uint4* rr = reinterpret_cast<const uint4*>(dres + r * C);
#pragma unroll
      for (int k = 0; k < NV; ++k) pr[k] = rr[k * 64 + lane];
    }
    const float rs = rstd[r];
    float s = 0.f;
    // a lane holds per chunk 8 fp32 sums and 4 x 4 packed dwords (dy, x,
    // d_x_new, w); everything else is unpacked where it is used
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      float d[8], xv[8], ww[8];
      arms_opaque(pw[k]);
      unpack8(pg[k], d);
      unpack8(px[k], xv);
      unpack8(pw[k], ww);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float h = xv[j] * rs;
        ag[k][j] += d[j] * h;
        s += d[j] * ww[j] * h;
      }
    }
    const float t = wave_sum(s) * (1.f / C);
    uint4* dxr = reinterpret_cast<uint4*>(dx + r * C);
    // dy * w and x * rs are recomputed from the packed registers here, not
    // kept across the reduction, which would cost 16 registers per chunk
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      float d[8], xv[8], ww[8], o[8];
      arms_opaque(pg[k]);
      arms_opaque(px[k]);
      arms_opaque(pw[k]);
      unpack8(pg[k], d);
      unpack8(px[k], xv);
      unpack8(pw[k], ww);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        o[j] = (d[j] * ww[j] - xv[j] * rs * t) * rs;
      if constexpr (DRES) {
        float rv[8];
        unpack8(pr[k], rv);
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] += rv[j];
      }
      dxr[k * 64 + lane] = pack8(o);
    }
  }
  // combine the block's waves in wave order (fixed, so repeatable), then
  // one partial row per block.  Every wave reaches every barrier: the row
  // loop above has none, and a wave with no rows arrives with zeros.
#pragma unroll 1
  for (int wv = 0; wv < ARMS_WAVES; ++wv) {
    if (wave == wv) {
#pragma unroll
      for (int k = 0; k < NV; ++k) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int i = (k * 64 + lane) * 2 + h;
          float4 a = make_float4(ag[k][4 * h], ag[k][4 * h + 1],
                                 ag[k][4 * h + 2], ag[k][4 * h + 3]);
          if (wv != 0) {
            const float4 p = red[i];
            a.x += p.x; a.y += p.y; a.z += p.z; a.w += p.w;
          }
          red[i] = a;
        }
      }
    }
    __syncthreads();
  }
  float4* pout = reinterpret_cast<float4*>(partial) +
                 static_cast<int64_t>(blockIdx.x) * (C / 4);
  for (int i = threadIdx.x; i < C / 4; i += ARMS_THREADS) pout[i] = red[i];
}

// Sums the G partial rows column by column and writes bf16.  A block owns 16
// columns; its 16 row-groups each sum every 16th partial row, then row-group
// 0 adds the 16 group sums in order.  The single-sum form of
// k_add_ln_reduce.
__global__ __launch_bounds__(256) void k_add_rms_reduce(
    const float* __restrict__ partial, int G, int C,
    uint16_t* __restrict__ out) {
  __shared__ float red[16][17];
  const int cg = threadIdx.x & 15, rg = threadIdx.x >> 4;
  const int j = blockIdx.x * 16 + cg;
  float a = 0.f;
  if (j < C)
    for (int g = rg; g < G; g += 16)
      a += partial[static_cast<int64_t>(g) * C + j];
  red[rg][cg] = a;
  __syncthreads();
  if (rg == 0 && j < C) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) t += red[i][cg];
    out[j] = f32_to_bf16(t);
  }
}

bool hip_add_rms_supported(int C) {
  return C > 0 && C % 512 == 0 && C / 512 <= ARMS_MAX_NV;
}

int hip_add_rms_max_blocks() { return ARMS_MAX_BLOCKS; }

void hip_add_rms_fwd(const void* x, const void* delta, const void* w,
                     void* x_new, void* y, float* rstd, int64_t R, int C,
                     float eps, hipStream_t s) {
  if (!hip_add_rms_supported(C)) throw std::runtime_error("add_rms: bad C");
  if (delta && !x_new) throw std::runtime_error("add_rms: delta needs x_new");
  if (!x || !w || !y || !rstd)
    throw std::runtime_error("add_rms: null x, weight, y or rstd");
  check_align(x, 16, "add_rms", "x");
  check_align(delta, 16, "add_rms", "delta");
  check_align(w, 16, "add_rms", "weight");
  check_align(x_new, 16, "add_rms", "x_new");
  check_align(y, 16, "add_rms", "y");
  if (R <= 0) return;
  const int64_t blocks = (R + ARMS_WAVES - 1) / ARMS_WAVES;
  if (blocks > 0x7FFFFFFF) throw std::runtime_error("add_rms: R too large");
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(static_cast<uint32_t>(blocks)),
                       dim3(ARMS_THREADS), 0, s,
                       static_cast<const uint16_t*>(x),
                       static_cast<const uint16_t*>(delta),
                       static_cast<const uint16_t*>(w),
                       static_cast<uint16_t*>(x_new),
                       static_cast<uint16_t*>(y), rstd, R, eps);
  };
  dispatch_cpt<1, 2, 3, 4, 5, 6, 7, 8>(
      C / 512, [&](auto NV) { launch(k_add_rms_fwd<NV()>); });
  HIP_CHECK(hipGetLastError());
}

// Blocks that fit on the device at once for one instantiation (the grid
// loops over rows, so more blocks would only add partial rows), clamped to
// the partials buffer.  Depends on the device and the kernel alone, so the
// summation order is the same from call to call.
template <typename K>
static int arms_resident_blocks(K kern, int* cache) {
  int dev = 0;
  HIP_CHECK(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64) dev = 0;
  if (cache[dev] == 0) {
    int per_cu = 0, cus = 0;
    HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(
        &per_cu, kern, ARMS_THREADS, 0));
    HIP_CHECK(hipDeviceGetAttribute(
        &cus, hipDeviceAttributeMultiprocessorCount, dev));
    int g = per_cu * cus;
    if (g < 1) g = 1;
    if (g > ARMS_MAX_BLOCKS) g = ARMS_MAX_BLOCKS;
    cache[dev] = g;
  }
  return cache[dev];
}

void hip_add_rms_bwd(const void* dy, const void* x_new, const void* w,
                     const float* rstd, const void* d_x_new, void* dx_total,
                     void* dgamma, float* partial, int64_t R, int C,
                     hipStream_t s) {
  if (!hip_add_rms_supported(C)) throw std::runtime_error("add_rms: bad C");
  if (!dy || !x_new || !w || !rstd || !dx_total || !dgamma || !partial)
    throw std::runtime_error("add_rms: null backward argument");
  check_align(dy, 16, "add_rms", "dy");
  check_align(x_new, 16, "add_rms", "x_new");
  check_align(w, 16, "add_rms", "weight");
  check_align(d_x_new, 16, "add_rms", "d_x_new");
  check_align(dx_total, 16, "add_rms", "dx_total");
  check_align(partial, 16, "add_rms", "partials");
  if (R <= 0) throw std::runtime_error("add_rms: empty input");
  static int cache[ARMS_MAX_NV][2][64];
  int grid = 0;
  auto launch = [&](auto kern, int* c) {
    grid = arms_resident_blocks(kern, c);
    const int64_t need = (R + ARMS_WAVES - 1) / ARMS_WAVES;
    if (need < grid) grid = static_cast<int>(need);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(ARMS_THREADS), 0, s,
                       static_cast<const uint16_t*>(dy),
                       static_cast<const uint16_t*>(x_new),
                       static_cast<const uint16_t*>(w), rstd,
                       static_cast<const uint16_t*>(d_x_new),
                       static_cast<uint16_t*>(dx_total), partial, R);
  };
  dispatch_cpt<1, 2, 3, 4, 5, 6, 7, 8>(C / 512, [&](auto NV) {
    if (d_x_new) launch(k_add_rms_bwd<NV(), true>, cache[NV() - 1][1]);
    else launch(k_add_rms_bwd<NV(), false>, cache[NV() - 1][0]);
  });
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_add_rms_reduce, dim3(C / 16), dim3(256), 0, s, partial,
                     grid, C, static_cast<uint16_t*>(dgamma));
  HIP_CHECK(hipGetLastError());
}

}  // namespace shamd
