// Helpers every HIP kernel file shares: the error macro, bf16 conversion and
// packing, wave and block reductions on the device side; the pointer-alignment
// check and the template-instantiation dispatch on the host side.  One
// definition each, so a fix reaches every kernel.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <stdexcept>
#include <string>
#include <type_traits>

namespace shamd {

#define HIP_CHECK(expr)                                                    \
  do {                                                                     \
    hipError_t _e = (expr);                                                \
    if (_e != hipSuccess)                                                  \
      throw std::runtime_error(std::string("HIP error: ") +                \
                               hipGetErrorString(_e) + " at " __FILE__ ":" + \
                               std::to_string(__LINE__));                  \
  } while (0)

// ------------------------------------------------------------------ bf16

static __device__ __forceinline__ float bf16_to_f32(uint16_t u) {
  return __uint_as_float(static_cast<uint32_t>(u) << 16);
}

// round to nearest even; every NaN becomes the quiet NaN 0x7FC0
static __device__ __forceinline__ uint16_t f32_to_bf16(float f) {
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return 0x7FC0;
  u += 0x7FFFu + ((u >> 16) & 1u);
  return static_cast<uint16_t>(u >> 16);
}

// A bf16 pair in one dword: the element at the lower address in the low half.
static __device__ __forceinline__ float bf16x2_lo(uint32_t p) {
  return __uint_as_float(p << 16);
}
static __device__ __forceinline__ float bf16x2_hi(uint32_t p) {
  return __uint_as_float(p & 0xFFFF0000u);
}
static __device__ __forceinline__ uint32_t bf16x2_pack(float lo, float hi) {
  return static_cast<uint32_t>(f32_to_bf16(lo)) |
         (static_cast<uint32_t>(f32_to_bf16(hi)) << 16);
}

// 4 bf16 (8-byte access) and 8 bf16 (16-byte access) to and from fp32
static __device__ __forceinline__ void unpack4(uint2 p, float* v) {
  v[0] = bf16x2_lo(p.x);
  v[1] = bf16x2_hi(p.x);
  v[2] = bf16x2_lo(p.y);
  v[3] = bf16x2_hi(p.y);
}
static __device__ __forceinline__ uint2 pack4(const float* v) {
  uint2 p;
  p.x = bf16x2_pack(v[0], v[1]);
  p.y = bf16x2_pack(v[2], v[3]);
  return p;
}
static __device__ __forceinline__ void unpack8(uint4 p, float* v) {
  v[0] = bf16x2_lo(p.x);
  v[1] = bf16x2_hi(p.x);
  v[2] = bf16x2_lo(p.y);
  v[3] = bf16x2_hi(p.y);
  v[4] = bf16x2_lo(p.z);
  v[5] = bf16x2_hi(p.z);
  v[6] = bf16x2_lo(p.w);
  v[7] = bf16x2_hi(p.w);
}
static __device__ __forceinline__ uint4 pack8(const float* v) {
  uint4 p;
  p.x = bf16x2_pack(v[0], v[1]);
  p.y = bf16x2_pack(v[2], v[3]);
  p.z = bf16x2_pack(v[4], v[5]);
  p.w = bf16x2_pack(v[6], v[7]);
  return p;
}

// ------------------------------------------------------------ reductions

// Butterfly sum over the 64 lanes of a wave; every lane gets the total.
static __device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Block-wide sum / max of one value per thread (BLK/64-wave block): wave shfl
// tree, then the wave results are combined through lds[BLK / 64] in wave
// order.  Every thread of the block calls it and gets the result.
//
// The sum starts from lds[0], not from 0.f: one add fewer, and the only value
// that can differ is the sign of an exactly-zero total.  No caller depends on
// it (cross-entropy's exp-sum is >= 1 and its sum of logits is only ever
// added to a finite logsumexp).
template <int BLK>
static __device__ __forceinline__ float block_sum(float v, float* lds) {
  for (int w = 32; w > 0; w >>= 1) v += __shfl_down(v, w, 64);
  int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) lds[wave] = v;
  __syncthreads();
  float t = lds[0];
#pragma unroll
  for (int i = 1; i < BLK / 64; ++i) t += lds[i];
  __syncthreads();
  return t;
}

template <int BLK>
static __device__ __forceinline__ float block_max(float v, float* lds) {
  for (int w = 32; w > 0; w >>= 1) v = fmaxf(v, __shfl_down(v, w, 64));
  int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) lds[wave] = v;
  __syncthreads();
  float t = -INFINITY;
#pragma unroll
  for (int i = 0; i < BLK / 64; ++i) t = fmaxf(t, lds[i]);
  __syncthreads();
  return t;
}

// ------------------------------------------------------------------ host

// The kernels load and store vectors of `bytes` bytes.  contiguous() keeps an
// offset view of a larger buffer as it is, so the launchers check every
// pointer before any launch.  A null pointer (an optional tensor) passes.
inline void check_align(const void* p, unsigned bytes, const char* op,
                        const char* what) {
  if (reinterpret_cast<uintptr_t>(p) & (bytes - 1))
    throw std::runtime_error(std::string(op) + ": " + what + " is not " +
                             std::to_string(bytes) + "-byte aligned");
}

// Calls f(std::integral_constant<int, V>) with the first listed V >= n, so
// that f can name a template instantiation by it: the listed values are the
// instantiations that exist.  An n above the last one throws — a kernel built
// for less would leave part of the row undone.
template <int V, int... Rest, typename F>
inline void dispatch_cpt(int n, F&& f) {
  if (n <= V)
    f(std::integral_constant<int, V>{});
  else if constexpr (sizeof...(Rest) > 0)
    dispatch_cpt<Rest...>(n, f);
  else
    throw std::runtime_error("dispatch_cpt: no instantiation for " +
                             std::to_string(n));
}

// Calls f(std::bool_constant<b>), for a bool template argument.
template <typename F>
inline void dispatch_bool(bool b, F&& f) {
  if (b)
    f(std::true_type{});
  else
    f(std::false_type{});
}

}  // namespace shamd
