// Device-side pieces shared by the fused optimizer kernels: the ungrouped
// ones in hip_kernels.hip and the parameter-group ones in
// optim_group_kernels.hip.  The per-element bodies live here so that both
// families run one operation chain: a grouped step equals, segment by
// segment, the ungrouped step run with that segment's rate and decay.
#pragma once

#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>

#include "common.h"
#include "device_util.h"

namespace shamd {

// a + b rounded on its own.  The optimizers' u = -lr * (...) would otherwise
// be contracted into the shadow's old + u, which then is no longer the
// rounding of what atomicAdd(values, u) stored (visible where old ~ -u).
__device__ __forceinline__ float add_uncontracted(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}

// g * coef rounded to fp32 on its own (gradient clipping): the optimizers
// use the rounded product wherever they used g, so a clipped step equals an
// unclipped step on gradients scaled beforehand, bit for bit.  The
// parameter-group kernels round lr * lr_scale the same way.
__device__ __forceinline__ float mul_uncontracted(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

// Residual-delta storage policies --------------------------------------

struct DeltaF32 {
  using T = float;
  static __device__ __forceinline__ float load(const T* p, int64_t i) {
    return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  static __device__ __forceinline__ void atomic_add(T* p, int64_t i, float v) {
    atomicAdd(p + i, v);
  }
};

struct DeltaBF16 {
  using T = uint16_t;
  static __device__ __forceinline__ float load(const T* p, int64_t i) {
    return bf16_to_f32(p[i]);
  }
  static __device__ __forceinline__ void atomic_add(T* p, int64_t i, float v) {
    // hardware packed bf16 atomic on the containing (even, odd) pair; the
    // neighbour lane receives -0.0, the exact identity (x + -0.0 == x for
    // every x; +0.0 would turn a -0.0 neighbour into +0.0)
    auto* base = reinterpret_cast<__hip_bfloat162*>(p + (i & ~int64_t(1)));
    __hip_bfloat16 bv = __float2bfloat16(v);
    __hip_bfloat16 bz = __float2bfloat16(-0.0f);
    __hip_bfloat162 val = (i & 1) ? __hip_bfloat162(bz, bv)
                                  : __hip_bfloat162(bv, bz);
    unsafeAtomicAdd(base, val);
  }
};

__device__ __forceinline__ float gval(const float* g, int64_t i) { return g[i]; }
__device__ __forceinline__ float gval(const uint16_t* g, int64_t i) {
  return bf16_to_f32(g[i]);
}

// Per-element bodies ----------------------------------------------------
//
// The moment updates spell out which product is fused into the sum and
// which is rounded on its own.  Left to the compiler, the choice differed
// between instantiations (a packed multiply instead of the FMA once g was
// itself a product), and a clipped step was no longer the unclipped step on
// scaled gradients.  The forms below are the ones the compiler had picked
// for the kernels without clipping, so those compute what they always did.

template <typename DP, bool CLIP>
__device__ __forceinline__ void sgd_element(
    int64_t i, float* __restrict__ mom, const float* __restrict__ grad,
    float lr, float momentum, float coef, float* values, typename DP::T* d1,
    typename DP::T* d2, typename DP::T* d3) {
  float g = CLIP ? mul_uncontracted(grad[i], coef) : grad[i];
  float m = fmaf(momentum, mom[i], g);
  mom[i] = m;
  float u = -lr * m;
  if (values) atomicAdd(values + i, u);
  if (d1) DP::atomic_add(d1, i, u);
  if (d2) DP::atomic_add(d2, i, u);
  if (d3) DP::atomic_add(d3, i, u);
}

template <typename DP, bool CLIP>
__device__ __forceinline__ void sgd_bf16_element(
    int64_t i, float* __restrict__ mom, const uint16_t* __restrict__ grad,
    uint16_t* __restrict__ shadow, float lr, float momentum, float coef,
    float* __restrict__ values, typename DP::T* d1, typename DP::T* d2,
    typename DP::T* d3) {
  float g = bf16_to_f32(grad[i]);
  if (CLIP) g = mul_uncontracted(g, coef);
  float m = fmaf(momentum, mom[i], g);
  mom[i] = m;
  float u = -lr * m;
  float old = atomicAdd(values + i, u);
  shadow[i] = f32_to_bf16(add_uncontracted(old, u));
  if (d1) DP::atomic_add(d1, i, u);
  if (d2) DP::atomic_add(d2, i, u);
  if (d3) DP::atomic_add(d3, i, u);
}

template <typename DP, typename GT, bool CLIP>
__device__ __forceinline__ void adamw_element(
    int64_t i, float* __restrict__ mom, float* __restrict__ vel,
    const GT* __restrict__ grad, uint16_t* __restrict__ shadow, float lr,
    float beta1, float beta2, float eps, float wd, float inv_bc1,
    float inv_bc2, float coef, float* __restrict__ values, typename DP::T* d1,
    typename DP::T* d2, typename DP::T* d3) {
  float g = gval(grad, i);
  if (CLIP) g = mul_uncontracted(g, coef);
  float m = fmaf(1.f - beta1, g, mul_uncontracted(beta1, mom[i]));
  mom[i] = m;
  float v = fmaf(g, mul_uncontracted(1.f - beta2, g),
                 mul_uncontracted(beta2, vel[i]));
  vel[i] = v;
  float w = __hip_atomic_load(values + i, __ATOMIC_RELAXED,
                              __HIP_MEMORY_SCOPE_AGENT);
  float u = -lr * (m * inv_bc1 / (sqrtf(v * inv_bc2) + eps) + wd * w);
  float old = atomicAdd(values + i, u);
  if (shadow) shadow[i] = f32_to_bf16(add_uncontracted(old, u));
  if (d1) DP::atomic_add(d1, i, u);
  if (d2) DP::atomic_add(d2, i, u);
  if (d3) DP::atomic_add(d3, i, u);
}

}  // namespace shamd
