// Global-norm gradient clipping for the fused optimizer steps.
//
// One read-only pass over the flat gradient gives its sum of squares in
// fp64; a one-block kernel turns that into the clip state (common.h,
// ClipState) that k_fused_sgd* / k_fused_adamw read as a single scalar.  No
// host round trip and no write to the gradient.
//
// Determinism: squares of fp32 or bf16 values are exact in fp64; every lane
// sums its elements in a fixed order, lanes combine by shuffle, waves through
// LDS in wave order, and each block stores one partial.  There are no
// atomics, so the same input gives the same bits on every run.
#include <hip/hip_runtime.h>

#include <cmath>
#include <stdexcept>
#include <string>

#include "device_util.h"
#include "hip_api.h"

namespace shamd {

constexpr int GC_BLOCK = 256;
constexpr int GC_WAVES = GC_BLOCK / 64;

__device__ __forceinline__ double gc_sq(float f) {
  double d = static_cast<double>(f);
  return d * d;
}
__device__ __forceinline__ double gc_elem_sq(const float* g, int64_t i) {
  return gc_sq(g[i]);
}
__device__ __forceinline__ double gc_elem_sq(const uint16_t* g, int64_t i) {
  return gc_sq(bf16_to_f32(g[i]));
}

// acc[0..3] += squares of the 16 bytes in q
__device__ __forceinline__ void gc_vec_sq(const float*, uint4 q, double* acc) {
  acc[0] += gc_sq(__uint_as_float(q.x));
  acc[1] += gc_sq(__uint_as_float(q.y));
  acc[2] += gc_sq(__uint_as_float(q.z));
  acc[3] += gc_sq(__uint_as_float(q.w));
}
__device__ __forceinline__ void gc_vec_sq(const uint16_t*, uint4 q, double* acc) {
  const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    acc[k] += gc_sq(bf16x2_lo(w[k]));
    acc[k] += gc_sq(bf16x2_hi(w[k]));
  }
}

// Sum over the block in a fixed order; the result is valid in thread 0.
__device__ __forceinline__ double gc_block_sum(double acc) {
  __shared__ double wave_part[GC_WAVES];
  for (int w = 32; w > 0; w >>= 1) acc += __shfl_down(acc, w, 64);
  if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = acc;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 0; w < GC_WAVES; ++w) s += wave_part[w];
  }
  return s;
}

// partials[blockIdx.x] = sum of g[i]^2 over the block's share of [0, n).
// The body runs on 16-byte vectors from the first 16-byte boundary at or
// after g; the up to VEC-1 elements in front of it and behind the last whole
// vector are peeled onto the first threads of block 0, so g needs only the
// alignment of its element type.
template <typename GT>
__global__ void __launch_bounds__(GC_BLOCK)
k_grad_sumsq(const GT* __restrict__ g, int64_t n, double* __restrict__ partials) {
  constexpr int VEC = 16 / sizeof(GT);
  int64_t head = static_cast<int64_t>(
      ((16u - (reinterpret_cast<uintptr_t>(g) & 15u)) & 15u) / sizeof(GT));
  if (head > n) head = n;
  const int64_t nvec = (n - head) / VEC;
  const int64_t tail0 = head + nvec * VEC;
  const int64_t tid = blockIdx.x * static_cast<int64_t>(GC_BLOCK) + threadIdx.x;
  const int64_t gstride = static_cast<int64_t>(gridDim.x) * GC_BLOCK;

  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  const uint4* gv = reinterpret_cast<const uint4*>(g + head);
#pragma unroll 2
  for (int64_t i = tid; i < nvec; i += gstride) gc_vec_sq(g, gv[i], acc);
  // head and tail: fewer than 2 * VEC elements, one per thread
  if (tid < head) {
    acc[0] += gc_elem_sq(g, tid);
  } else if (tid - head < n - tail0) {
    acc[0] += gc_elem_sq(g, tail0 + (tid - head));
  }
  double s = gc_block_sum((acc[0] + acc[1]) + (acc[2] + acc[3]));
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// One block.  Thread t sums its run of consecutive partials in index order,
// thread 0 then sums the runs in index order: a fixed order that does not
// depend on how the first kernel was scheduled.
__global__ void __launch_bounds__(GC_BLOCK)
k_grad_clip_finalize(const double* __restrict__ partials, int nparts,
                     double max_norm, ClipState* __restrict__ st) {
  __shared__ double run[GC_BLOCK];
  const int per = (nparts + GC_BLOCK - 1) / GC_BLOCK;
  const int lo = threadIdx.x * per;
  const int hi = lo + per < nparts ? lo + per : nparts;
  double s = 0.0;
  for (int i = lo; i < hi; ++i) s += partials[i];
  run[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x != 0) return;
  double sumsq = 0.0;
  for (int t = 0; t < GC_BLOCK; ++t) sumsq += run[t];
  const double nrm = sqrt(sumsq);
  // inf - inf or a NaN gradient gives NaN, an inf gradient gives inf
  const bool bad = isnan(sumsq) || isinf(sumsq);
  double c = max_norm / (nrm + 1e-6);
  if (c > 1.0) c = 1.0;
  st->sumsq = sumsq;
  st->norm = static_cast<float>(nrm);
  st->coef = bad ? 0.0f : static_cast<float>(c);
  st->skip = bad ? 1u : 0u;
  if (bad) st->skipped_total = st->skipped_total + 1u;
}

void hip_grad_clip_coef(const void* grad, bool grad_bf16, int64_t n,
                        double max_norm, double* scratch, ClipState* state,
                        hipStream_t s) {
  if (!(max_norm > 0.0) || std::isinf(max_norm))
    throw std::invalid_argument("grad_clip_coef: max_norm must be finite and > 0");
  if (n < 1) throw std::invalid_argument("grad_clip_coef: n must be >= 1");
  if (!grad || !scratch || !state)
    throw std::invalid_argument("grad_clip_coef: null pointer");
  const uintptr_t a = reinterpret_cast<uintptr_t>(grad);
  if (a % (grad_bf16 ? 2 : 4))
    throw std::invalid_argument("grad_clip_coef: grad is not element-aligned");
  if (reinterpret_cast<uintptr_t>(scratch) % 8 ||
      reinterpret_cast<uintptr_t>(state) % 8)
    throw std::invalid_argument("grad_clip_coef: scratch/state need 8-byte alignment");
  const int vec = grad_bf16 ? 8 : 4;
  int64_t blocks = (n / vec + GC_BLOCK - 1) / GC_BLOCK;
  if (blocks < 1) blocks = 1;
  if (blocks > GRAD_CLIP_MAX_BLOCKS) blocks = GRAD_CLIP_MAX_BLOCKS;
  const int g = static_cast<int>(blocks);
  if (grad_bf16)
    hipLaunchKernelGGL(k_grad_sumsq<uint16_t>, dim3(g), dim3(GC_BLOCK), 0, s,
                       static_cast<const uint16_t*>(grad), n, scratch);
  else
    hipLaunchKernelGGL(k_grad_sumsq<float>, dim3(g), dim3(GC_BLOCK), 0, s,
                       static_cast<const float*>(grad), n, scratch);
  hipLaunchKernelGGL(k_grad_clip_finalize, dim3(1), dim3(GC_BLOCK), 0, s,
                     scratch, g, max_norm, state);
  HIP_CHECK(hipGetLastError());
}

}  // namespace shamd
