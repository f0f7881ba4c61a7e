// Device-side tanh-GELU math shared by gelu_kernels.hip and
// bias_grad_kernels.hip, so both evaluate the very same expressions.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_util.h"

namespace shamd {

// gelu(x) = 0.5 x (1 + tanh(k (x + 0.044715 x^3))), k = sqrt(2/pi)
constexpr float GK = 0.7978845608028654f;
constexpr float GC = 0.044715f;

static __device__ __forceinline__ float gelu_f(float x) {
  float inner = GK * (x + GC * x * x * x);
  return 0.5f * x * (1.f + tanhf(inner));
}

// gelu'(x) is 1 or 0 to well below fp32 resolution for |x| >= 10, so the
// formula is evaluated at x clamped to [-10, 10]: unclamped, x * x reaches
// inf for |x| > 1.8e19 and sech2 == 0 then meets it as 0 * inf = NaN.  NaN
// passes through the clamp (fminf/fmaxf return the other operand, so the
// NaN is put back by hand).
static __device__ __forceinline__ float gelu_grad_f(float xin) {
  float x = fminf(fmaxf(xin, -10.f), 10.f);
  if (xin != xin) x = xin;
  float x2 = x * x;
  float inner = GK * x * (1.f + GC * x2);
  float t = tanhf(inner);
  float sech2 = 1.f - t * t;
  return 0.5f * (1.f + t) + 0.5f * x * sech2 * GK * (1.f + 3.f * GC * x2);
}

}  // namespace shamd
