// Fused bf16 GELU (tanh approximation) forward/backward.
//
// Elementwise and HBM-bound; uint4 (8 x bf16) loads/stores and fast-math
// transcendentals (outputs are bf16-rounded anyway).
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#include "device_util.h"
#include "gelu_math.h"
#include "hip_api.h"

namespace shamd {

// uint4 (8 bf16) per iteration — the pair-only variant measured SLOWER
// than torch's 8-wide elementwise kernels in round 1; round 2's SwiGLU
// showed uint4 vectorization is what closes (and flips) the gap.
__global__ void k_gelu_fwd(const uint4* __restrict__ x,
                           uint4* __restrict__ y, int64_t n8) {
  int64_t g = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n8; i += g) {
    uint4 u = x[i];
    uint4 o;
    const uint32_t* up = &u.x;
    uint32_t* op = &o.x;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      op[k] = bf16x2_pack(gelu_f(bf16x2_lo(up[k])), gelu_f(bf16x2_hi(up[k])));
    y[i] = o;
  }
}

__global__ void k_gelu_bwd(const uint4* __restrict__ dy,
                           const uint4* __restrict__ x,
                           uint4* __restrict__ dx, int64_t n8) {
  int64_t g = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n8; i += g) {
    uint4 u = x[i], d = dy[i];
    uint4 o;
    const uint32_t* up = &u.x;
    const uint32_t* dp = &d.x;
    uint32_t* op = &o.x;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      op[k] = bf16x2_pack(bf16x2_lo(dp[k]) * gelu_grad_f(bf16x2_lo(up[k])),
                          bf16x2_hi(dp[k]) * gelu_grad_f(bf16x2_hi(up[k])));
    dx[i] = o;
  }
}

static inline int gelu_grid(int64_t npairs) {
  int64_t g = (npairs + 255) / 256;
  return static_cast<int>(g < 16384 ? (g > 0 ? g : 1) : 16384);
}

void hip_gelu_fwd(const void* x, void* y, int64_t n, hipStream_t s) {
  // the wrapper arranges n % 8 == 0 and 16-byte alignment; both are
  // checked here because nothing else guarantees them
  if (n % 8) throw std::runtime_error("gelu: n must be a multiple of 8");
  check_align(x, 16, "gelu", "x");
  check_align(y, 16, "gelu", "y");
  if (n <= 0) return;
  hipLaunchKernelGGL(k_gelu_fwd, dim3(gelu_grid(n / 8)), dim3(256), 0, s,
                     static_cast<const uint4*>(x),
                     static_cast<uint4*>(y), n / 8);
  HIP_CHECK(hipGetLastError());
}

void hip_gelu_bwd(const void* dy, const void* x, void* dx, int64_t n,
                  hipStream_t s) {
  if (n % 8) throw std::runtime_error("gelu: n must be a multiple of 8");
  check_align(dy, 16, "gelu", "dy");
  check_align(x, 16, "gelu", "x");
  check_align(dx, 16, "gelu", "dx");
  if (n <= 0) return;
  hipLaunchKernelGGL(k_gelu_bwd, dim3(gelu_grid(n / 8)), dim3(256), 0, s,
                     static_cast<const uint4*>(dy),
                     static_cast<const uint4*>(x),
                     static_cast<uint4*>(dx), n / 8);
  HIP_CHECK(hipGetLastError());
}

}  // namespace shamd
