// Fused bf16 LayerNorm forward/backward for the training path.
//
// torch's native LayerNorm backward on MI355X measured ~4.4x off the HBM
// roofline for GPT-2-small shapes (110 us per (32768, 768) call vs ~25 us
// of traffic; profiles/gpt2_train_step_kernels.txt).  These kernels do:
//   fwd:      one pass — block per row, fp32 statistics, bf16 in/out,
//             saves mean/rstd for backward
//   bwd dx:   one pass — block per row, two fused row-reductions
//   bwd dw/db: one pass — grid-stride over rows, per-thread column
//             accumulators in registers, one fp32 atomic per column per block
//
// Shapes: x is (R, C) row-major bf16, C <= 4096 (the wrapper falls back to
// torch otherwise), weights/bias bf16[C].
//
// For C a multiple of 256 up to 1024 (GPT-2-small's 768) the training path
// now runs the wave-per-row kernels in add_ln_kernels.hip, which also fold
// the residual add and the dgamma/dbeta sums into one pass each way; the
// LayerNorm kernels here serve every other width.
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#include "device_util.h"
#include "hip_api.h"  // declaration parity check

namespace shamd {

constexpr int LN_BLOCK = 256;  // 4 waves

// Per-thread register cache for a row's owned elements.  CPT (elements per
// thread) is a template parameter so the caches index statically and stay
// in registers — a runtime loop bound would push them to scratch memory.
constexpr int LN_MAXC = 4096;

template <int CPT>  // pairs per thread
__global__ void k_ln_fwd(const uint16_t* __restrict__ x,
                         const uint16_t* __restrict__ w,
                         const uint16_t* __restrict__ b,
                         uint16_t* __restrict__ y, float* __restrict__ mean,
                         float* __restrict__ rstd, int C, float eps) {
  __shared__ float lds4[4];
  const int64_t r = blockIdx.x;
  const int C2 = C >> 1;  // wrapper guarantees C is even
  const uint32_t* xr = reinterpret_cast<const uint32_t*>(x + r * C);
  const uint32_t* wp = reinterpret_cast<const uint32_t*>(w);
  const uint32_t* bp = reinterpret_cast<const uint32_t*>(b);
  uint32_t* yr = reinterpret_cast<uint32_t*>(y + r * C);
  float x0[CPT], x1[CPT];
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < CPT; ++k) {
    int c = threadIdx.x + k * LN_BLOCK;
    float a = 0.f, bb = 0.f;
    if (c < C2) {
      uint32_t pk = xr[c];
      a = bf16x2_lo(pk);
      bb = bf16x2_hi(pk);
    }
    x0[k] = a;
    x1[k] = bb;
    s += a + bb;
  }
  float m = block_sum<LN_BLOCK>(s, lds4) / C;
  // two-pass variance from the cached row: sum((x - m)^2) does not cancel
  // the way sum(x^2)/C - m^2 does when |mean| >> std.  Columns past the row
  // hold 0 in the cache and must add 0 here, not m^2.
  float ss = 0.f;
#pragma unroll
  for (int k = 0; k < CPT; ++k) {
    int c = threadIdx.x + k * LN_BLOCK;
    if (c < C2) {
      float d0 = x0[k] - m, d1 = x1[k] - m;
      ss += d0 * d0 + d1 * d1;
    }
  }
  float rs = rsqrtf(block_sum<LN_BLOCK>(ss, lds4) / C + eps);
  if (threadIdx.x == 0) {
    mean[r] = m;
    rstd[r] = rs;
  }
#pragma unroll
  for (int k = 0; k < CPT; ++k) {
    int c = threadIdx.x + k * LN_BLOCK;
    if (c < C2) {
      uint32_t wk = wp[c];
      float o0 = (x0[k] - m) * rs * bf16x2_lo(wk);
      float o1 = (x1[k] - m) * rs * bf16x2_hi(wk);
      if (bp) {
        uint32_t bk = bp[c];
        o0 += bf16x2_lo(bk);
        o1 += bf16x2_hi(bk);
      }
      yr[c] = bf16x2_pack(o0, o1);
    }
  }
}

template <int CPT>
__global__ void k_ln_bwd_dx(const uint16_t* __restrict__ dy,
                            const uint16_t* __restrict__ x,
                            const uint16_t* __restrict__ w,
                            const float* __restrict__ mean,
                            const float* __restrict__ rstd,
                            uint16_t* __restrict__ dx, int C) {
  __shared__ float lds4[4];
  const int64_t r = blockIdx.x;
  const int C2 = C >> 1;
  const uint32_t* xr = reinterpret_cast<const uint32_t*>(x + r * C);
  const uint32_t* dyr = reinterpret_cast<const uint32_t*>(dy + r * C);
  const uint32_t* wp = reinterpret_cast<const uint32_t*>(w);
  uint32_t* dxr = reinterpret_cast<uint32_t*>(dx + r * C);
  float m = mean[r], rs = rstd[r];
  float a0[CPT], a1[CPT], h0[CPT], h1[CPT];
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int k = 0; k < CPT; ++k) {
    int c = threadIdx.x + k * LN_BLOCK;
    float u0 = 0.f, u1 = 0.f, v0 = 0.f, v1 = 0.f;
    if (c < C2) {
      uint32_t dk = dyr[c], wk = wp[c], xk = xr[c];
      u0 = bf16x2_lo(dk) * bf16x2_lo(wk);
      u1 = bf16x2_hi(dk) * bf16x2_hi(wk);
      v0 = (bf16x2_lo(xk) - m) * rs;
      v1 = (bf16x2_hi(xk) - m) * rs;
    }
    a0[k] = u0;
    a1[k] = u1;
    h0[k] = v0;
    h1[k] = v1;
    s1 += u0 + u1;
    s2 += u0 * v0 + u1 * v1;
  }
  float t1 = block_sum<LN_BLOCK>(s1, lds4) / C;
  float t2 = block_sum<LN_BLOCK>(s2, lds4) / C;
#pragma unroll
  for (int k = 0; k < CPT; ++k) {
    int c = threadIdx.x + k * LN_BLOCK;
    if (c < C2)
      dxr[c] = bf16x2_pack((a0[k] - t1 - h0[k] * t2) * rs,
                           (a1[k] - t1 - h1[k] * t2) * rs);
  }
}

// dgamma/dbeta: each thread owns the columns {tid, tid+256, ...} and
// accumulates them in registers across its grid-stride rows; one fp32
// atomic per owned column per block at the end.  (Scalar ownership: the
// pair-vectorized variant measured 2x slower here — partial-wave idling in
// the odd half-iteration outweighs the wider loads.)
template <int CPT>
__global__ void k_ln_bwd_dwdb(const uint16_t* __restrict__ dy,
                              const uint16_t* __restrict__ x,
                              const float* __restrict__ mean,
                              const float* __restrict__ rstd,
                              float* __restrict__ dgamma,
                              float* __restrict__ dbeta, int64_t R, int C) {
  float accg[CPT], accb[CPT];
#pragma unroll
  for (int k = 0; k < CPT; ++k) accg[k] = accb[k] = 0.f;
  for (int64_t r = blockIdx.x; r < R; r += gridDim.x) {
    const uint16_t* xr = x + r * C;
    const uint16_t* dyr = dy + r * C;
    float m = mean[r], rs = rstd[r];
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
      int c = threadIdx.x + k * LN_BLOCK;
      if (c < C) {
        float g = bf16_to_f32(dyr[c]);
        float xh = (bf16_to_f32(xr[c]) - m) * rs;
        accg[k] += g * xh;
        accb[k] += g;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < CPT; ++k) {
    int c = threadIdx.x + k * LN_BLOCK;
    if (c < C) {
      atomicAdd(&dgamma[c], accg[k]);
      atomicAdd(&dbeta[c], accb[k]);
    }
  }
}

// ------------------------------------------------------------- RMSNorm
// Fused bf16 RMSNorm for the Llama training path (round-1 weak #5: the
// module-level fp32 upcast re-read the whole (B,T,C) activation per call —
// the same cast-traffic tax FusedLayerNorm removed for GPT-2).
//   fwd:    y = x * rsqrt(mean(x^2) + eps) * w, one pass, saves fp32 rstd
//   bwd dx: dx = rs * (dy*w - x * rs^2 * mean(dy*w*x))  — ONE row reduction
//   bwd dw: grid-stride rows, register column accumulators (as LN dw/db)

template <int CPT>  // pairs per thread
__global__ void k_rms_fwd(const uint16_t* __restrict__ x,
                          const uint16_t* __restrict__ w,
                          uint16_t* __restrict__ y, float* __restrict__ rstd,
                          int C, float eps) {
  __shared__ float lds4[4];
  const int64_t r = blockIdx.x;
  const int C2 = C >> 1;
  const uint32_t* xr = reinterpret_cast<const uint32_t*>(x + r * C);
  const uint32_t* wp = reinterpret_cast<const uint32_t*>(w);
  uint32_t* yr = reinterpret_cast<uint32_t*>(y + r * C);
  float x0[CPT], x1[CPT];
  float ss = 0.f;
#pragma unroll
  for (int k = 0; k < CPT; ++k) {
    int c = threadIdx.x + k * LN_BLOCK;
    float a = 0.f, b = 0.f;
    if (c < C2) {
      uint32_t pk = xr[c];
      a = bf16x2_lo(pk);
      b = bf16x2_hi(pk);
    }
    x0[k] = a;
    x1[k] = b;
    ss += a * a + b * b;
  }
  float tot2 = block_sum<LN_BLOCK>(ss, lds4);
  float rs = rsqrtf(tot2 / C + eps);
  if (threadIdx.x == 0) rstd[r] = rs;
#pragma unroll
  for (int k = 0; k < CPT; ++k) {
    int c = threadIdx.x + k * LN_BLOCK;
    if (c < C2) {
      uint32_t wk = wp[c];
      yr[c] = bf16x2_pack(x0[k] * rs * bf16x2_lo(wk),
                          x1[k] * rs * bf16x2_hi(wk));
    }
  }
}

template <int CPT>
__global__ void k_rms_bwd_dx(const uint16_t* __restrict__ dy,
                             const uint16_t* __restrict__ x,
                             const uint16_t* __restrict__ w,
                             const float* __restrict__ rstd,
                             uint16_t* __restrict__ dx, int C) {
  __shared__ float lds4[4];
  const int64_t r = blockIdx.x;
  const int C2 = C >> 1;
  const uint32_t* xr = reinterpret_cast<const uint32_t*>(x + r * C);
  const uint32_t* dyr = reinterpret_cast<const uint32_t*>(dy + r * C);
  const uint32_t* wp = reinterpret_cast<const uint32_t*>(w);
  uint32_t* dxr = reinterpret_cast<uint32_t*>(dx + r * C);
  float rs = rstd[r];
  float g0[CPT], g1[CPT], v0[CPT], v1[CPT];
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < CPT; ++k) {
    int c = threadIdx.x + k * LN_BLOCK;
    float u0 = 0.f, u1 = 0.f, a = 0.f, b = 0.f;
    if (c < C2) {
      uint32_t dk = dyr[c], wk = wp[c], xk = xr[c];
      u0 = bf16x2_lo(dk) * bf16x2_lo(wk);
      u1 = bf16x2_hi(dk) * bf16x2_hi(wk);
      a = bf16x2_lo(xk);
      b = bf16x2_hi(xk);
    }
    g0[k] = u0;
    g1[k] = u1;
    v0[k] = a;
    v1[k] = b;
    s += u0 * a + u1 * b;
  }
  float t = block_sum<LN_BLOCK>(s, lds4) / C * rs * rs;
#pragma unroll
  for (int k = 0; k < CPT; ++k) {
    int c = threadIdx.x + k * LN_BLOCK;
    if (c < C2)
      dxr[c] = bf16x2_pack((g0[k] - v0[k] * t) * rs,
                           (g1[k] - v1[k] * t) * rs);
  }
}

template <int CPT>
__global__ void k_rms_bwd_dw(const uint16_t* __restrict__ dy,
                             const uint16_t* __restrict__ x,
                             const float* __restrict__ rstd,
                             float* __restrict__ dgamma, int64_t R, int C) {
  float accg[CPT];
#pragma unroll
  for (int k = 0; k < CPT; ++k) accg[k] = 0.f;
  for (int64_t r = blockIdx.x; r < R; r += gridDim.x) {
    const uint16_t* xr = x + r * C;
    const uint16_t* dyr = dy + r * C;
    float rs = rstd[r];
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
      int c = threadIdx.x + k * LN_BLOCK;
      if (c < C)
        accg[k] += bf16_to_f32(dyr[c]) * bf16_to_f32(xr[c]) * rs;
    }
  }
#pragma unroll
  for (int k = 0; k < CPT; ++k) {
    int c = threadIdx.x + k * LN_BLOCK;
    if (c < C) atomicAdd(&dgamma[c], accg[k]);
  }
}

void hip_rms_fwd(const void* x, const void* w, void* y, float* rstd,
                 int64_t R, int C, float eps, hipStream_t s) {
  if (C > LN_MAXC || (C & 1)) throw std::runtime_error("rms: bad C");
  // the fwd and dx kernels load and store bf16 pairs as uint32 (the dw/db and
  // colsum kernels load scalars and take any bf16 pointer)
  check_align(x, 4, "ln/rms", "x");
  check_align(w, 4, "ln/rms", "weight");
  check_align(y, 4, "ln/rms", "y");
  if (R <= 0) return;  // a grid of 0 blocks is an invalid configuration
  int cpt = (C / 2 + LN_BLOCK - 1) / LN_BLOCK;
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(static_cast<uint32_t>(R)), dim3(LN_BLOCK), 0,
                       s, static_cast<const uint16_t*>(x),
                       static_cast<const uint16_t*>(w),
                       static_cast<uint16_t*>(y), rstd, C, eps);
  };
  dispatch_cpt<1, 2, 3, 4, 8>(cpt, [&](auto K) { launch(k_rms_fwd<K()>); });
  HIP_CHECK(hipGetLastError());
}

void hip_rms_bwd(const void* dy, const void* x, const void* w,
                 const float* rstd, void* dx, float* dgamma, int64_t R, int C,
                 hipStream_t s) {
  if (C > LN_MAXC || (C & 1)) throw std::runtime_error("rms: bad C");
  check_align(dy, 4, "ln/rms", "dy");
  check_align(x, 4, "ln/rms", "x");
  check_align(w, 4, "ln/rms", "weight");
  check_align(dx, 4, "ln/rms", "dx");
  if (R <= 0) return;  // dgamma stays as the caller zeroed it
  int cpt = (C / 2 + LN_BLOCK - 1) / LN_BLOCK;
  auto launch_dx = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(static_cast<uint32_t>(R)), dim3(LN_BLOCK), 0,
                       s, static_cast<const uint16_t*>(dy),
                       static_cast<const uint16_t*>(x),
                       static_cast<const uint16_t*>(w), rstd,
                       static_cast<uint16_t*>(dx), C);
  };
  dispatch_cpt<1, 2, 3, 4, 8>(
      cpt, [&](auto K) { launch_dx(k_rms_bwd_dx<K()>); });
  HIP_CHECK(hipGetLastError());
  int g = R < 2048 ? static_cast<int>(R) : 2048;  // 8 blocks/CU (see LN note)
  int ecpt = (C + LN_BLOCK - 1) / LN_BLOCK;
  auto launch_dw = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(g), dim3(LN_BLOCK), 0, s,
                       static_cast<const uint16_t*>(dy),
                       static_cast<const uint16_t*>(x), rstd, dgamma, R, C);
  };
  dispatch_cpt<1, 2, 3, 4, 8, 16>(
      ecpt, [&](auto K) { launch_dw(k_rms_bwd_dw<K()>); });
  HIP_CHECK(hipGetLastError());
}

// Column sum of a (R, C) bf16 matrix into fp32 out[C] — the bias-gradient
// reduction of Linear backward (torch's reduce_kernel measured ~1.7 TB/s
// at GPT-2 shapes).  Same register-accumulator geometry as k_ln_bwd_dwdb:
// each thread owns columns {tid, tid+256, ...} across grid-stride rows,
// one fp32 atomic per owned column per block.
template <int CPT>
__global__ void k_colsum_bf16(const uint16_t* __restrict__ x,
                              float* __restrict__ out, int64_t R, int C) {
  float acc[CPT];
#pragma unroll
  for (int k = 0; k < CPT; ++k) acc[k] = 0.f;
  for (int64_t r = blockIdx.x; r < R; r += gridDim.x) {
    const uint16_t* xr = x + r * C;
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
      int c = threadIdx.x + k * LN_BLOCK;
      if (c < C) acc[k] += bf16_to_f32(xr[c]);
    }
  }
#pragma unroll
  for (int k = 0; k < CPT; ++k) {
    int c = threadIdx.x + k * LN_BLOCK;
    if (c < C) atomicAdd(&out[c], acc[k]);
  }
}

void hip_colsum_bf16(const void* x, float* out, int64_t R, int C,
                     hipStream_t s) {
  if (C > LN_MAXC) throw std::runtime_error("colsum: C too large");
  if (R <= 0) return;  // out stays as the caller zeroed it
  int g = R < 2048 ? static_cast<int>(R) : 2048;
  int ecpt = (C + LN_BLOCK - 1) / LN_BLOCK;
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(g), dim3(LN_BLOCK), 0, s,
                       static_cast<const uint16_t*>(x), out, R, C);
  };
  dispatch_cpt<1, 2, 3, 4, 8, 16>(
      ecpt, [&](auto K) { launch(k_colsum_bf16<K()>); });
  HIP_CHECK(hipGetLastError());
}

void hip_ln_fwd(const void* x, const void* w, const void* b, void* y,
                float* mean, float* rstd, int64_t R, int C, float eps,
                hipStream_t s) {
  if (C > LN_MAXC || (C & 1)) throw std::runtime_error("ln: bad C");
  check_align(x, 4, "ln/rms", "x");
  check_align(w, 4, "ln/rms", "weight");
  check_align(b, 4, "ln/rms", "bias");
  check_align(y, 4, "ln/rms", "y");
  if (R <= 0) return;
  int cpt = (C / 2 + LN_BLOCK - 1) / LN_BLOCK;
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(static_cast<uint32_t>(R)), dim3(LN_BLOCK), 0,
                       s, static_cast<const uint16_t*>(x),
                       static_cast<const uint16_t*>(w),
                       static_cast<const uint16_t*>(b),
                       static_cast<uint16_t*>(y), mean, rstd, C, eps);
  };
  dispatch_cpt<1, 2, 3, 4, 8>(cpt, [&](auto K) { launch(k_ln_fwd<K()>); });
  HIP_CHECK(hipGetLastError());
}

void hip_ln_bwd(const void* dy, const void* x, const void* w,
                const float* mean, const float* rstd, void* dx, float* dgamma,
                float* dbeta, int64_t R, int C, hipStream_t s) {
  if (C > LN_MAXC || (C & 1)) throw std::runtime_error("ln: bad C");
  check_align(dy, 4, "ln/rms", "dy");
  check_align(x, 4, "ln/rms", "x");
  check_align(w, 4, "ln/rms", "weight");
  check_align(dx, 4, "ln/rms", "dx");
  if (R <= 0) return;  // dgamma/dbeta stay as the caller zeroed them
  int cpt = (C / 2 + LN_BLOCK - 1) / LN_BLOCK;
  auto launch_dx = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(static_cast<uint32_t>(R)), dim3(LN_BLOCK), 0,
                       s, static_cast<const uint16_t*>(dy),
                       static_cast<const uint16_t*>(x),
                       static_cast<const uint16_t*>(w), mean, rstd,
                       static_cast<uint16_t*>(dx), C);
  };
  dispatch_cpt<1, 2, 3, 4, 8>(
      cpt, [&](auto K) { launch_dx(k_ln_bwd_dx<K()>); });
  HIP_CHECK(hipGetLastError());
  // 2048 blocks = 8 per CU: enough waves to hide the strided bf16 loads
  // (256 blocks measured 0.67 TB/s — latency-bound at 1 block/CU); the
  // per-column atomic count stays trivial (2048 per column).
  int g = R < 2048 ? static_cast<int>(R) : 2048;
  int ecpt = (C + LN_BLOCK - 1) / LN_BLOCK;  // element (not pair) ownership
  auto launch_dw = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(g), dim3(LN_BLOCK), 0, s,
                       static_cast<const uint16_t*>(dy),
                       static_cast<const uint16_t*>(x), mean, rstd, dgamma,
                       dbeta, R, C);
  };
  dispatch_cpt<1, 2, 3, 4, 8, 16>(
      ecpt, [&](auto K) { launch_dw(k_ln_bwd_dwdb<K()>); });
  HIP_CHECK(hipGetLastError());
}

}  // namespace shamd
