// Fused residual-add + bf16 LayerNorm, forward and backward, for the
// transformer residual chain  x = x + f(ln(x)).
//
// The unfused chain moves 13 activations per LayerNorm (add: 3, ln fwd: 2,
// ln bwd dx: 3, ln bwd dw/db: 2, autograd's residual-gradient add: 3).
// These kernels move 8:
//   fwd:  reads x, delta            writes x_new = x + delta, y = LN(x_new)
//   bwd:  reads dy, x_new, d_x_new  writes dx_total = LN_dx(dy) + d_x_new
//         and accumulates dgamma / dbeta (/ d delta_bias) in the same pass
//
// Layout: one 64-lane wave owns a row.  C = NV * 256, so a row is exactly
// NV x (64 lanes x 8 B): every lane issues NV uint2 loads per tensor and the
// row reductions are shuffle-only — no LDS, no barrier in the row loop.
// In backward a lane owns the same 4*NV columns for every row of its
// grid-stride loop, so the column sums live in registers (NV is a template
// parameter for that reason, see LN_MAXC in ln_kernels.hip).  They leave the
// kernel as one fp32 partial row per block; k_add_ln_reduce sums the
// partials in a fixed order and writes bf16 — no float atomics, so backward
// repeats bit for bit.
//
// Other widths keep using the block-per-row kernels in ln_kernels.hip.
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#include "device_util.h"
#include "hip_api.h"  // declaration parity check

namespace shamd {

constexpr int ALN_FWD_THREADS = 256;   // 4 rows per block
constexpr int ALN_BWD_THREADS = 256;   // 4 rows in flight per block
constexpr int ALN_BWD_WAVES = ALN_BWD_THREADS / 64;
constexpr int ALN_MAX_BLOCKS = 1024;   // bounds the partials buffer
constexpr int ALN_MAX_NV = 4;          // C = 256, 512, 768, 1024

template <int NV>
__global__ __launch_bounds__(ALN_FWD_THREADS) void k_add_ln_fwd(
    const uint16_t* __restrict__ x, const uint16_t* __restrict__ delta,
    const uint16_t* __restrict__ dbias, const uint16_t* __restrict__ w,
    const uint16_t* __restrict__ b, uint16_t* __restrict__ x_new,
    uint16_t* __restrict__ y, float* __restrict__ mean,
    float* __restrict__ rstd, int64_t R, float eps) {
  constexpr int C = NV * 256;
  const int lane = threadIdx.x & 63;
  const int64_t r =
      static_cast<int64_t>(blockIdx.x) * (ALN_FWD_THREADS / 64) +
      __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform
  if (r >= R) return;  // whole wave leaves; no barrier below
  const uint2* xr = reinterpret_cast<const uint2*>(x + r * C);
  float v[NV][4];
  uint2 px[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) px[k] = xr[k * 64 + lane];
  if (delta) {
    const uint2* dr = reinterpret_cast<const uint2*>(delta + r * C);
    uint2* xo = reinterpret_cast<uint2*>(x_new + r * C);
    uint2 pd[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) pd[k] = dr[k * 64 + lane];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      float a[4], d[4];
      unpack4(px[k], a);
      unpack4(pd[k], d);
#pragma unroll
      for (int j = 0; j < 4; ++j) a[j] += d[j];
      if (dbias) {
        float bb[4];
        unpack4(reinterpret_cast<const uint2*>(dbias)[k * 64 + lane], bb);
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] += bb[j];
      }
      // statistics and y come from the rounded sum, as if x_new had been
      // written by a separate add and read back
      uint2 o = pack4(a);
      xo[k * 64 + lane] = o;
      unpack4(o, v[k]);
    }
  } else {
#pragma unroll
    for (int k = 0; k < NV; ++k) unpack4(px[k], v[k]);
  }
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < NV; ++k) s += (v[k][0] + v[k][1]) + (v[k][2] + v[k][3]);
  const float m = wave_sum(s) * (1.f / C);
  float q = 0.f;
#pragma unroll
  for (int k = 0; k < NV; ++k)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float d = v[k][j] - m;
      q += d * d;
    }
  const float rs = rsqrtf(wave_sum(q) * (1.f / C) + eps);
  if (lane == 0) {
    mean[r] = m;
    rstd[r] = rs;
  }
  uint2* yr = reinterpret_cast<uint2*>(y + r * C);
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    float ww[4], o[4];
    unpack4(reinterpret_cast<const uint2*>(w)[k * 64 + lane], ww);
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (v[k][j] - m) * rs * ww[j];
    if (b) {
      float bb[4];
      unpack4(reinterpret_cast<const uint2*>(b)[k * 64 + lane], bb);
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] += bb[j];
    }
    yr[k * 64 + lane] = pack4(o);
  }
}

// partial is (gridDim.x, NS, C) fp32 with NS = 2 (dgamma, dbeta) or 3
// (+ d delta_bias); every element is written, so it needs no zeroing.
template <int NV, bool DDB>
__global__ __launch_bounds__(ALN_BWD_THREADS) void k_add_ln_bwd(
    const uint16_t* __restrict__ dy, const uint16_t* __restrict__ xn,
    const uint16_t* __restrict__ w, const float* __restrict__ mean,
    const float* __restrict__ rstd, const uint16_t* __restrict__ dres,
    uint16_t* __restrict__ dx, float* __restrict__ partial, int64_t R) {
  constexpr int C = NV * 256;
  constexpr int NS = DDB ? 3 : 2;
  __shared__ float4 red[NS * C / 4];
  const int lane = threadIdx.x & 63;
  // wave-uniform by construction; saying so keeps the row index and every
  // row base address in scalar registers
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float ag[NV][4], ab[NV][4], ad[DDB ? NV : 1][4];
  uint2 pw[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    pw[k] = reinterpret_cast<const uint2*>(w)[k * 64 + lane];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      ag[k][j] = 0.f;
      ab[k][j] = 0.f;
      if constexpr (DDB) ad[k][j] = 0.f;
    }
  }
  const int64_t stride = static_cast<int64_t>(gridDim.x) * ALN_BWD_WAVES;
#pragma unroll 1
  for (int64_t r = static_cast<int64_t>(blockIdx.x) * ALN_BWD_WAVES + wave;
       r < R; r += stride) {
    const uint2* dyr = reinterpret_cast<const uint2*>(dy + r * C);
    const uint2* xr = reinterpret_cast<const uint2*>(xn + r * C);
    uint2 pg[NV], px[NV], pr[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) pg[k] = dyr[k * 64 + lane];
#pragma unroll
    for (int k = 0; k < NV; ++k) px[k] = xr[k * 64 + lane];
    if (dres) {
      const uint2* rr = reinterpret_cast<const uint2*>(dres + r * C);
#pragma unroll
      for (int k = 0; k < NV; ++k) pr[k] = rr[k * 64 + lane];
    }
    const float m = mean[r], rs = rstd[r];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      float d[4], xv[4], ww[4];
      unpack4(pg[k], d);
      unpack4(px[k], xv);
      unpack4(pw[k], ww);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float h = (xv[j] - m) * rs;
        const float g = d[j] * ww[j];
        ag[k][j] += d[j] * h;
        ab[k][j] += d[j];
        s1 += g;
        s2 += g * h;
      }
    }
    // the two row sums ride one butterfly, so their shuffles overlap
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float u1 = __shfl_xor(s1, o, 64), u2 = __shfl_xor(s2, o, 64);
      s1 += u1;
      s2 += u2;
    }
    const float t1 = s1 * (1.f / C), t2 = s2 * (1.f / C);
    uint2* dxr = reinterpret_cast<uint2*>(dx + r * C);
    // g and x-hat are recomputed from the packed registers here, not kept
    // across the reduction, which would cost 8 registers per chunk
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      float d[4], xv[4], ww[4], o[4];
      unpack4(pg[k], d);
      unpack4(px[k], xv);
      unpack4(pw[k], ww);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        o[j] = (d[j] * ww[j] - t1 - (xv[j] - m) * rs * t2) * rs;
      if (dres) {
        float rv[4];
        unpack4(pr[k], rv);
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] += rv[j];
      }
      if constexpr (DDB) {
#pragma unroll
        for (int j = 0; j < 4; ++j) ad[k][j] += o[j];
      }
      dxr[k * 64 + lane] = pack4(o);
    }
  }
  // combine the block's waves in wave order (fixed, so repeatable), then
  // one partial row per block
#pragma unroll 1
  for (int wv = 0; wv < ALN_BWD_WAVES; ++wv) {
    if (wave == wv) {
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        const int i = k * 64 + lane;
        float4 a = make_float4(ag[k][0], ag[k][1], ag[k][2], ag[k][3]);
        float4 bsum = make_float4(ab[k][0], ab[k][1], ab[k][2], ab[k][3]);
        if (wv != 0) {
          float4 p = red[i], q = red[C / 4 + i];
          a.x += p.x; a.y += p.y; a.z += p.z; a.w += p.w;
          bsum.x += q.x; bsum.y += q.y; bsum.z += q.z; bsum.w += q.w;
        }
        red[i] = a;
        red[C / 4 + i] = bsum;
        if constexpr (DDB) {
          float4 c = make_float4(ad[k][0], ad[k][1], ad[k][2], ad[k][3]);
          if (wv != 0) {
            float4 p = red[2 * (C / 4) + i];
            c.x += p.x; c.y += p.y; c.z += p.z; c.w += p.w;
          }
          red[2 * (C / 4) + i] = c;
        }
      }
    }
    __syncthreads();
  }
  float4* pout = reinterpret_cast<float4*>(partial) +
                 static_cast<int64_t>(blockIdx.x) * (NS * C / 4);
  for (int i = threadIdx.x; i < NS * C / 4; i += ALN_BWD_THREADS)
    pout[i] = red[i];
}

// Sums the G partial rows column by column and writes bf16.  A block owns 16
// columns; its 16 row-groups each sum every 16th partial row, then thread
// row-group 0 adds the 16 group sums in order.  nsc = NS * C.
__global__ __launch_bounds__(256) void k_add_ln_reduce(
    const float* __restrict__ partial, int G, int nsc, int C,
    uint16_t* __restrict__ o0, uint16_t* __restrict__ o1,
    uint16_t* __restrict__ o2) {
  __shared__ float red[16][17];
  const int cg = threadIdx.x & 15, rg = threadIdx.x >> 4;
  const int j = blockIdx.x * 16 + cg;
  float a = 0.f;
  if (j < nsc)
    for (int g = rg; g < G; g += 16)
      a += partial[static_cast<int64_t>(g) * nsc + j];
  red[rg][cg] = a;
  __syncthreads();
  if (rg == 0 && j < nsc) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) t += red[i][cg];
    const int s = j / C, c = j - s * C;
    uint16_t* out = s == 0 ? o0 : (s == 1 ? o1 : o2);
    if (out) out[c] = f32_to_bf16(t);
  }
}

bool hip_add_ln_supported(int C) {
  return C > 0 && C % 256 == 0 && C / 256 <= ALN_MAX_NV;
}

int hip_add_ln_max_blocks() { return ALN_MAX_BLOCKS; }

void hip_add_ln_fwd(const void* x, const void* delta, const void* dbias,
                    const void* w, const void* b, void* x_new, void* y,
                    float* mean, float* rstd, int64_t R, int C, float eps,
                    hipStream_t s) {
  if (!hip_add_ln_supported(C)) throw std::runtime_error("add_ln: bad C");
  if (delta && !x_new) throw std::runtime_error("add_ln: delta needs x_new");
  if (dbias && !delta) throw std::runtime_error("add_ln: dbias needs delta");
  check_align(x, 8, "add_ln", "x");
  check_align(delta, 8, "add_ln", "delta");
  check_align(dbias, 8, "add_ln", "delta_bias");
  check_align(w, 8, "add_ln", "weight");
  check_align(b, 8, "add_ln", "bias");
  check_align(x_new, 8, "add_ln", "x_new");
  check_align(y, 8, "add_ln", "y");
  if (R <= 0) return;
  constexpr int rows = ALN_FWD_THREADS / 64;
  const int64_t blocks = (R + rows - 1) / rows;
  if (blocks > 0x7FFFFFFF) throw std::runtime_error("add_ln: R too large");
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(static_cast<uint32_t>(blocks)),
                       dim3(ALN_FWD_THREADS), 0, s,
                       static_cast<const uint16_t*>(x),
                       static_cast<const uint16_t*>(delta),
                       static_cast<const uint16_t*>(dbias),
                       static_cast<const uint16_t*>(w),
                       static_cast<const uint16_t*>(b),
                       static_cast<uint16_t*>(x_new),
                       static_cast<uint16_t*>(y), mean, rstd, R, eps);
  };
  dispatch_cpt<1, 2, 3, 4>(C / 256,
                           [&](auto NV) { launch(k_add_ln_fwd<NV()>); });
  HIP_CHECK(hipGetLastError());
}

// Blocks that fit on the device at once for one instantiation (the grid
// loops over rows, so more blocks would only add partial rows), clamped to
// the partials buffer.  Depends on the device and the kernel alone, so the
// summation order is the same from call to call.
template <typename K>
static int aln_resident_blocks(K kern, int* cache) {
  int dev = 0;
  HIP_CHECK(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64) dev = 0;
  if (cache[dev] == 0) {
    int per_cu = 0, cus = 0;
    HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(
        &per_cu, kern, ALN_BWD_THREADS, 0));
    HIP_CHECK(hipDeviceGetAttribute(
        &cus, hipDeviceAttributeMultiprocessorCount, dev));
    int g = per_cu * cus;
    if (g < 1) g = 1;
    if (g > ALN_MAX_BLOCKS) g = ALN_MAX_BLOCKS;
    cache[dev] = g;
  }
  return cache[dev];
}

void hip_add_ln_bwd(const void* dy, const void* x_new, const void* w,
                    const float* mean, const float* rstd, const void* d_x_new,
                    void* dx_total, void* dgamma, void* dbeta, void* ddbias,
                    float* partial, int64_t R, int C, hipStream_t s) {
  if (!hip_add_ln_supported(C)) throw std::runtime_error("add_ln: bad C");
  check_align(dy, 8, "add_ln", "dy");
  check_align(x_new, 8, "add_ln", "x_new");
  check_align(w, 8, "add_ln", "weight");
  check_align(d_x_new, 8, "add_ln", "d_x_new");
  check_align(dx_total, 8, "add_ln", "dx_total");
  if (reinterpret_cast<uintptr_t>(partial) & 15u)
    throw std::runtime_error("add_ln: partials are not 16-byte aligned");
  if (R <= 0) throw std::runtime_error("add_ln: empty input");
  static int cache[ALN_MAX_NV][2][64];
  int grid = 0;
  auto launch = [&](auto kern, int* c) {
    grid = aln_resident_blocks(kern, c);
    const int64_t need = (R + ALN_BWD_WAVES - 1) / ALN_BWD_WAVES;
    if (need < grid) grid = static_cast<int>(need);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(ALN_BWD_THREADS), 0, s,
                       static_cast<const uint16_t*>(dy),
                       static_cast<const uint16_t*>(x_new),
                       static_cast<const uint16_t*>(w), mean, rstd,
                       static_cast<const uint16_t*>(d_x_new),
                       static_cast<uint16_t*>(dx_total), partial, R);
  };
  const int nv = C / 256;
  if (ddbias)
    dispatch_cpt<1, 2, 3, 4>(nv, [&](auto NV) {
      launch(k_add_ln_bwd<NV(), true>, cache[NV() - 1][1]);
    });
  else
    dispatch_cpt<1, 2, 3, 4>(nv, [&](auto NV) {
      launch(k_add_ln_bwd<NV(), false>, cache[NV() - 1][0]);
    });
  HIP_CHECK(hipGetLastError());
  const int nsc = (ddbias ? 3 : 2) * C;
  hipLaunchKernelGGL(k_add_ln_reduce, dim3(nsc / 16), dim3(256), 0, s, partial,
                     grid, nsc, C, static_cast<uint16_t*>(dgamma),
                     static_cast<uint16_t*>(dbeta),
                     static_cast<uint16_t*>(ddbias));
  HIP_CHECK(hipGetLastError());
}

}  // namespace shamd
