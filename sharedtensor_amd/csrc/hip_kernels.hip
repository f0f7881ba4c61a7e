// CDNA4 (gfx950) kernels for the shared-tensor delta codec.
//
// These replace the reference's single-threaded CPU loops
// (/root/reference/src/sharedtensor.c:106-111, 156-174, 334-344) with
// HBM-bandwidth-bound GPU passes:
//   * k_reduce_*   — per-tensor RMS / absmax: per-lane register accumulation
//                    across grid-stride iterations, one 64-lane __shfl tree +
//                    one atomic per wave per tensor-run (naive per-iteration
//                    atomics measured 21 GB/s — serialized f64 atomics)
//   * k_quant_*    — fused quantize + error-feedback debit + pack; 1-bit uses
//                    __ballot (one uint64 per wave, LSB-first layout
//                    byte-identical to the reference wire format); optional
//                    fused next-round scale statistics (lagged-scale mode)
//   * k_apply      — fused decode + multi-destination atomic scatter
//                    (replica + gossip-forward buffers in one pass)
//   * k_add_scatter / k_fused_sgd* — addFromInternal and the optimizer update
//                    fused with the 4-way delta staging
//
// Residual delta buffers are fp32 by default or bf16 (DeltaBF16 policy) to
// halve their HBM footprint for 100 GB-scale tensors: the per-round debit
// quanta (+-scale, q*e4m3*pow2, int4*pow2) are exactly representable in
// bf16, so only the accumulated remainder rounds.  bf16 accumulation uses
// the hardware packed atomic (global_atomic_pk_add_bf16) on element pairs —
// all padded regions are even-sized and 4-byte aligned.
//
// All element loops are grid-stride with 256-thread blocks (4 waves);
// wavefront size is 64 (CDNA4).
#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>

#include <type_traits>
#include <stdexcept>
#include <string>

#include "device_util.h"
#include "hip_api.h"
#include "optim_step.h"

namespace shamd {

constexpr int BLOCK = 256;

static inline int grid_for(int64_t n) {
  int64_t g = (n + BLOCK - 1) / BLOCK;
  // >> 256 workgroups fills all 8 XCDs; cap and grid-stride beyond.
  return static_cast<int>(g < 32768 ? (g > 0 ? g : 1) : 32768);
}

// ---------------------------------------------------------------- helpers

// bf16 conversions live in device_util.h; add/mul_uncontracted and the
// residual-delta storage policies (DeltaF32, DeltaBF16) in optim_step.h.

// Binary search: largest t with poffs[t] <= j.  T is small (1..few hundred)
// and the array is L2-hot; for T==1 the caller's fast path skips this.
__device__ __forceinline__ int find_tensor(const int64_t* poffs, int T, int64_t j) {
  int lo = 0, hi = T - 1;
  while (lo < hi) {
    int mid = (lo + hi + 1) >> 1;
    if (poffs[mid] <= j) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ float d_e4m3_to_f32(uint8_t v) {
  uint32_t exp = (v >> 3) & 0xF;
  uint32_t man = v & 7;
  float out;
  if (exp == 0xF && man == 7) {
    out = __builtin_nanf("");
  } else if (exp == 0) {
    out = static_cast<float>(man) * 0x1p-9f;
  } else {
    uint32_t bits = ((exp - 7 + 127) << 23) | (man << 20);
    out = __uint_as_float(bits);
  }
  return (v & 0x80) ? -out : out;
}

__device__ __forceinline__ uint8_t d_f32_to_e4m3(float xf) {
  if (xf != xf) return 0x7F;
  float cl = xf > 448.f ? 448.f : (xf < -448.f ? -448.f : xf);
  uint32_t u = __float_as_uint(cl);
  uint8_t sign = (u >> 24) & 0x80;
  uint32_t abs = u & 0x7FFFFFFFu;
  if (abs == 0) return sign;
  int e = static_cast<int>(abs >> 23) - 127;
  uint32_t mant = (abs & 0x7FFFFFu) | 0x800000u;
  int shift = (e >= -6) ? 20 : (14 - e);
  if (shift > 24) return sign;
  uint32_t q = mant >> shift;
  uint32_t rem = mant & ((1u << shift) - 1);
  uint32_t half = 1u << (shift - 1);
  if (rem > half || (rem == half && (q & 1))) q++;
  if (e >= -6) {
    if (q == 16) { q = 8; e++; }
    return sign | static_cast<uint8_t>(((e + 7) << 3) | (q - 8));
  }
  if (q >= 8) return sign | 0x08;
  return sign | static_cast<uint8_t>(q);
}

__device__ __forceinline__ float d_pow2_floor(double x) {
  if (!(x > 0.0) || isinf(x) || isnan(x)) return 0.0f;
  int e;
  frexp(x, &e);
  return static_cast<float>(ldexp(1.0, e - 1));
}

__device__ __forceinline__ float d_pow2_ceil(double x) {
  if (!(x > 0.0) || isinf(x) || isnan(x)) return 0.0f;
  int e;
  double m = frexp(x, &e);
  return static_cast<float>(ldexp(1.0, m == 0.5 ? e - 1 : e));
}

// ------------------------------------------------------------- reductions

__device__ __forceinline__ void wave_flush_sumsq(double acc, int t, double* sumsq) {
  for (int w = 32; w > 0; w >>= 1) acc += __shfl_down(acc, w, 64);
  if ((threadIdx.x & 63) == 0 && acc != 0.0) atomicAdd(&sumsq[t], acc);
}

// Maximum of two magnitudes (sign bit clear) through their bit patterns:
// the order of non-negative floats, with +inf above every finite value and
// NaN above +inf.  A float compare would drop a NaN; this way a poisoned
// residual reaches k_finalize_scales, which answers it with scale 0.
__device__ __forceinline__ float mag_max(float a, float b) {
  uint32_t ua = __float_as_uint(a), ub = __float_as_uint(b);
  return __uint_as_float(ua > ub ? ua : ub);
}

__device__ __forceinline__ void wave_flush_max(float acc, int t, uint32_t* amax) {
  for (int w = 32; w > 0; w >>= 1) acc = mag_max(acc, __shfl_down(acc, w, 64));
  if ((threadIdx.x & 63) == 0 && __float_as_uint(acc) != 0)
    atomicMax(&amax[t], __float_as_uint(acc));
}

// Per-half-wave maximum for k_quant_int4, whose threads hold two elements
// each: a tensor boundary (64 elements) can fall on lane 32, so each 32-lane
// half reduces on its own and flushes into its own tensor's slot.  Call it
// from wave-uniform control flow only.
__device__ __forceinline__ void halfwave_flush_max(float acc, int t, uint32_t* amax) {
  for (int w = 16; w > 0; w >>= 1) acc = mag_max(acc, __shfl_down(acc, w, 32));
  if ((threadIdx.x & 31) == 0 && __float_as_uint(acc) != 0)
    atomicMax(&amax[t], __float_as_uint(acc));
}

// Sum of squares per tensor (1-bit codec).  A wave never straddles tensors
// within an iteration (poffs are 64-aligned), so the flush condition is
// wave-uniform.
template <typename DP>
__global__ void k_reduce_sumsq(const typename DP::T* __restrict__ delta,
                               const int64_t* offs, const int64_t* poffs,
                               int T, int64_t pe, int stride, double* sumsq) {
  int64_t gstride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  double acc = 0.0;
  int cur_t = -1;
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < pe; j += gstride) {
    int t = (T == 1) ? 0 : find_tensor(poffs, T, j);
    if (t != cur_t) {
      if (cur_t >= 0) wave_flush_sumsq(acc, cur_t, sumsq);
      acc = 0.0;
      cur_t = t;
    }
    int64_t L = j - poffs[t];
    int64_t sz = offs[t + 1] - offs[t];
    if (L < sz && (stride == 1 || (L % stride) == 0)) {
      double f = static_cast<double>(DP::load(delta, offs[t] + L));
      acc += f * f;
    }
  }
  if (cur_t >= 0) wave_flush_sumsq(acc, cur_t, sumsq);
}

template <typename DP>
__global__ void k_reduce_absmax(const typename DP::T* __restrict__ delta,
                                const int64_t* offs, const int64_t* poffs,
                                int T, int64_t pe, uint32_t* amax) {
  int64_t gstride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  float acc = 0.0f;
  int cur_t = -1;
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < pe; j += gstride) {
    int t = (T == 1) ? 0 : find_tensor(poffs, T, j);
    if (t != cur_t) {
      if (cur_t >= 0) wave_flush_max(acc, cur_t, amax);
      acc = 0.0f;
      cur_t = t;
    }
    int64_t L = j - poffs[t];
    int64_t sz = offs[t + 1] - offs[t];
    if (L < sz) {
      acc = mag_max(acc, fabsf(DP::load(delta, offs[t] + L)));
    }
  }
  if (cur_t >= 0) wave_flush_max(acc, cur_t, amax);
}

__global__ void k_finalize_scales(Codec c, const void* reduce_buf,
                                  const int64_t* offs, int T, int stride,
                                  float* scales) {
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= T) return;
  if (c == Codec::OneBit) {
    int64_t sz = offs[t + 1] - offs[t];
    int64_t cnt = (sz + stride - 1) / stride;
    double ss = reinterpret_cast<const double*>(reduce_buf)[t];
    scales[t] = d_pow2_floor(sqrt(ss / static_cast<double>(cnt > 0 ? cnt : 1)));
  } else {
    float mx = __uint_as_float(reinterpret_cast<const uint32_t*>(reduce_buf)[t]);
    double den = (c == Codec::Fp8) ? 448.0 : 7.0;
    scales[t] = (mx > 0.0f && !isinf(mx) && !isnan(mx))
                    ? d_pow2_ceil(static_cast<double>(mx) / den)
                    : 0.0f;
  }
}

// --------------------------------------------------------------- quantize
// The debit is an atomic add of -sent so concurrent adds (training thread,
// gossip forwards) landing between the read and the update are preserved —
// the GPU version of the reference's benign-race contract made lossless.

template <typename DP>
__global__ void k_quant_1bit(typename DP::T* __restrict__ delta,
                             const int64_t* offs, const int64_t* poffs, int T,
                             int64_t pe, const float* __restrict__ scales,
                             uint64_t* __restrict__ words, double* stats_out) {
  int64_t gstride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  double acc = 0.0;
  int cur_t = -1;
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < pe; j += gstride) {
    int t = (T == 1) ? 0 : find_tensor(poffs, T, j);
    if (stats_out && t != cur_t) {
      if (cur_t >= 0) wave_flush_sumsq(acc, cur_t, stats_out);
      acc = 0.0;
      cur_t = t;
    }
    int64_t L = j - poffs[t];
    int64_t sz = offs[t + 1] - offs[t];
    float s = scales[t];
    bool neg = false;  // bit value: 1 means -scale was sent
    if (L < sz) {
      int64_t g = offs[t] + L;
      float v = DP::load(delta, g);
      if (s != 0.0f) {
        neg = !(v > 0.0f);
        DP::atomic_add(delta, g, neg ? s : -s);
      }
      if (stats_out) {
        // fp32 subtraction first: the statistic must see the same rounded
        // residual that lands in memory
        float rf = (s == 0.0f) ? v : (v - (neg ? -s : s));
        acc += static_cast<double>(rf) * static_cast<double>(rf);
      }
    }
    uint64_t mask = __ballot(neg);
    if ((threadIdx.x & 63) == 0) words[j >> 6] = mask;
  }
  if (stats_out && cur_t >= 0) wave_flush_sumsq(acc, cur_t, stats_out);
}

template <typename DP>
__global__ void k_quant_fp8(typename DP::T* __restrict__ delta,
                            const int64_t* offs, const int64_t* poffs, int T,
                            int64_t pe, const float* __restrict__ scales,
                            uint8_t* __restrict__ payload, uint32_t* stats_out) {
  int64_t gstride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  float amax = 0.0f;
  int cur_t = -1;
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < pe; j += gstride) {
    int t = (T == 1) ? 0 : find_tensor(poffs, T, j);
    if (stats_out && t != cur_t) {
      if (cur_t >= 0) wave_flush_max(amax, cur_t, stats_out);
      amax = 0.0f;
      cur_t = t;
    }
    int64_t L = j - poffs[t];
    int64_t sz = offs[t + 1] - offs[t];
    float s = scales[t];
    uint8_t q = 0;
    if (L < sz) {
      int64_t g = offs[t] + L;
      float v = DP::load(delta, g);
      float sent = 0.0f;
      if (s != 0.0f) {
        q = d_f32_to_e4m3(v / s);
        sent = d_e4m3_to_f32(q) * s;
        DP::atomic_add(delta, g, -sent);
      }
      if (stats_out) {
        amax = mag_max(amax, fabsf(v - sent));
      }
    }
    payload[j] = q;
  }
  if (stats_out && cur_t >= 0) wave_flush_max(amax, cur_t, stats_out);
}

template <typename DP>
__global__ void k_quant_int4(typename DP::T* __restrict__ delta,
                             const int64_t* offs, const int64_t* poffs, int T,
                             int64_t pe, const float* __restrict__ scales,
                             uint8_t* __restrict__ payload, uint32_t* stats_out) {
  // one thread per payload byte = 2 elements (both in the same tensor:
  // padded regions are 64-aligned, hence even).  nb is only a multiple of
  // 32, so the loop runs to a 64-multiple with clamped indices to keep the
  // wave fully convergent for the stats __shfl flush (clamped lanes fill a
  // whole 32-lane half and share the last tensor).
  int64_t nb = pe / 2;
  int64_t nbp = (nb + 63) & ~int64_t(63);
  int64_t gstride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  float amax = 0.0f;
  int cur_t = -1;
  for (int64_t b = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; b < nbp; b += gstride) {
    bool act = b < nb;
    int64_t j0 = (act ? b : nb - 1) * 2;
    int t = (T == 1) ? 0 : find_tensor(poffs, T, j0);
    // a wave covers 128 elements, so t is uniform over each 32-lane half
    // only; the vote keeps the shuffles in wave-uniform control flow (the
    // loop bound and cur_t >= 0 are wave-uniform too)
    if (stats_out && __any(t != cur_t)) {
      if (cur_t >= 0) halfwave_flush_max(amax, cur_t, stats_out);
      amax = 0.0f;
      cur_t = t;
    }
    int64_t base = j0 - poffs[t];
    int64_t sz = offs[t + 1] - offs[t];
    float s = scales[t];
    uint8_t byte = 0;
    for (int k = 0; k < 2; ++k) {
      int64_t L = base + k;
      if (act && L < sz) {
        int64_t g = offs[t] + L;
        float v = DP::load(delta, g);
        float sent = 0.0f;
        if (s != 0.0f) {
          float r = nearbyintf(v / s);
          r = r > 7.f ? 7.f : (r < -7.f ? -7.f : r);
          int8_t q = static_cast<int8_t>(r);
          byte |= static_cast<uint8_t>(q & 0xF) << (k * 4);
          sent = static_cast<float>(q) * s;
          DP::atomic_add(delta, g, -sent);
        }
        if (stats_out) {
          amax = mag_max(amax, fabsf(v - sent));
        }
      }
    }
    if (act) payload[b] = byte;
  }
  if (stats_out && cur_t >= 0) halfwave_flush_max(amax, cur_t, stats_out);
}

// ------------------------------------------------------------------ apply
// destinations: the fp32 replica (values) and up to two gossip-forward
// residual buffers (delta-typed), all in one pass over the payload.

template <int CODEC, typename DP>
__global__ void k_apply(const uint8_t* __restrict__ payload,
                        const int64_t* offs, const int64_t* poffs, int T,
                        int64_t pe, const float* __restrict__ scales,
                        float* values, typename DP::T* d1, typename DP::T* d2) {
  int64_t gstride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < pe; j += gstride) {
    int t = (T == 1) ? 0 : find_tensor(poffs, T, j);
    int64_t L = j - poffs[t];
    int64_t sz = offs[t + 1] - offs[t];
    if (L >= sz) continue;
    float s = scales[t];
    if (s == 0.0f) continue;
    float v;
    if (CODEC == 0) {
      uint64_t w = reinterpret_cast<const uint64_t*>(payload)[j >> 6];
      v = ((w >> (j & 63)) & 1) ? -s : s;
    } else if (CODEC == 1) {
      v = d_e4m3_to_f32(payload[j]) * s;
    } else {
      int8_t q = static_cast<int8_t>((payload[j >> 1] >> ((j & 1) * 4)) & 0xF);
      if (q > 7) q -= 16;
      v = static_cast<float>(q) * s;
      if (v == 0.0f) continue;
    }
    int64_t g = offs[t] + L;
    if (values) atomicAdd(values + g, v);
    if (d1) DP::atomic_add(d1, g, v);
    if (d2) DP::atomic_add(d2, g, v);
  }
}

template <typename DP>
__global__ void k_add_scatter(const float* __restrict__ src, int64_t n,
                              float alpha, float* values, typename DP::T* d1,
                              typename DP::T* d2, typename DP::T* d3) {
  int64_t gstride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += gstride) {
    float v = alpha * src[i];
    if (v == 0.0f) continue;
    if (values) atomicAdd(values + i, v);
    if (d1) DP::atomic_add(d1, i, v);
    if (d2) DP::atomic_add(d2, i, v);
    if (d3) DP::atomic_add(d3, i, v);
  }
}

// src is a (possibly bf16) residual buffer: used by the rejoin
// reconciliation to re-add the preserved unsent up-residual into the fresh
// replica and child slots.
template <typename DP>
__global__ void k_add_delta_scatter(const typename DP::T* __restrict__ src,
                                    int64_t n, float* values,
                                    typename DP::T* d1, typename DP::T* d2) {
  int64_t gstride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += gstride) {
    float v = DP::load(src, i);
    if (v == 0.0f) continue;
    if (values) atomicAdd(values + i, v);
    if (d1) DP::atomic_add(d1, i, v);
    if (d2) DP::atomic_add(d2, i, v);
  }
}

// Fused snapshot capture + debit (join fast path, engine.cpp
// send_snapshot): out[i] := values[i] and delta[i] -= out[i] in ONE pass.
// The captured buffer IS the authoritative exactly-what-was-sent bytes, so
// the old capture -> D2H -> TCP -> H2D -> debit round trip collapses to
// capture+debit -> D2H -> TCP, and chunks pipeline against the socket.
template <typename DP>
__global__ void k_snapshot_capture(const float* __restrict__ values,
                                   typename DP::T* delta,
                                   float* __restrict__ out, int64_t n) {
  int64_t gstride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += gstride) {
    float v = __hip_atomic_load(values + i, __ATOMIC_RELAXED,
                                __HIP_MEMORY_SCOPE_AGENT);
    out[i] = v;
    if (v != 0.0f) DP::atomic_add(delta, i, -v);
  }
}

// CLIP (all three fused optimizers): `clip` is the state grad_clip_coef
// wrote.  skip set: every thread returns before it touches any buffer.
// Otherwise the gradient is fl32(g * coef).  Without CLIP the pointer is
// unused and the kernel is what it was before clipping existed.
//
// The per-element bodies (optim_step.h) are shared with the parameter-group
// kernels of optim_group_kernels.hip.
template <typename DP, bool CLIP>
__global__ void k_fused_sgd(float* __restrict__ mom,
                            const float* __restrict__ grad, float lr,
                            float momentum, int64_t n, float* values,
                            typename DP::T* d1, typename DP::T* d2,
                            typename DP::T* d3, const ClipState* clip) {
  float coef = 1.0f;
  if (CLIP) {
    if (clip->skip) return;
    coef = clip->coef;
  }
  int64_t gstride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += gstride) {
    sgd_element<DP, CLIP>(i, mom, grad, lr, momentum, coef, values, d1, d2,
                          d3);
  }
}

// Mixed-precision fused optimizer: bf16 gradients in, fp32 master update,
// bf16 shadow parameters out — one HBM pass covering what autocast training
// otherwise spends three cast/copy kernel families on.  The atomicAdd's
// return value folds any concurrently-applied gossip into the shadow.
template <typename DP, bool CLIP>
__global__ void k_fused_sgd_bf16(float* __restrict__ mom,
                                 const uint16_t* __restrict__ grad,
                                 uint16_t* __restrict__ shadow, float lr,
                                 float momentum, int64_t n,
                                 float* __restrict__ values,
                                 typename DP::T* d1, typename DP::T* d2,
                                 typename DP::T* d3, const ClipState* clip) {
  float coef = 1.0f;
  if (CLIP) {
    if (clip->skip) return;
    coef = clip->coef;
  }
  int64_t gstride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += gstride) {
    sgd_bf16_element<DP, CLIP>(i, mom, grad, shadow, lr, momentum, coef,
                               values, d1, d2, d3);
  }
}

// -------------------------------------------------------------- launchers

void hip_reduce_scales(Codec c, const void* delta, bool delta_bf16,
                       const DevTable& tb, void* reduce_buf, float* scales_out,
                       int stride, hipStream_t s) {
  HIP_CHECK(hipMemsetAsync(reduce_buf, 0, tb.T * 8, s));
  // 2048 blocks = 8 per CU (full wave occupancy) while keeping the flush
  // atomic count at ~8K per launch.
  int g = grid_for(tb.pe);
  if (g > 2048) g = 2048;
  if (c == Codec::OneBit) {
    if (delta_bf16)
      hipLaunchKernelGGL((k_reduce_sumsq<DeltaBF16>), dim3(g), dim3(BLOCK), 0, s,
                         static_cast<const uint16_t*>(delta), tb.offs, tb.poffs,
                         tb.T, tb.pe, stride, static_cast<double*>(reduce_buf));
    else
      hipLaunchKernelGGL((k_reduce_sumsq<DeltaF32>), dim3(g), dim3(BLOCK), 0, s,
                         static_cast<const float*>(delta), tb.offs, tb.poffs,
                         tb.T, tb.pe, stride, static_cast<double*>(reduce_buf));
  } else {
    if (delta_bf16)
      hipLaunchKernelGGL((k_reduce_absmax<DeltaBF16>), dim3(g), dim3(BLOCK), 0, s,
                         static_cast<const uint16_t*>(delta), tb.offs, tb.poffs,
                         tb.T, tb.pe, static_cast<uint32_t*>(reduce_buf));
    else
      hipLaunchKernelGGL((k_reduce_absmax<DeltaF32>), dim3(g), dim3(BLOCK), 0, s,
                         static_cast<const float*>(delta), tb.offs, tb.poffs,
                         tb.T, tb.pe, static_cast<uint32_t*>(reduce_buf));
  }
  int gt = (tb.T + BLOCK - 1) / BLOCK;
  hipLaunchKernelGGL(k_finalize_scales, dim3(gt), dim3(BLOCK), 0, s, c,
                     reduce_buf, tb.offs, tb.T, stride, scales_out);
  HIP_CHECK(hipGetLastError());
}

void hip_finalize_scales(Codec c, const DevTable& tb, const void* reduce_buf,
                         float* scales_out, int stride, hipStream_t s) {
  int gt = (tb.T + BLOCK - 1) / BLOCK;
  hipLaunchKernelGGL(k_finalize_scales, dim3(gt), dim3(BLOCK), 0, s, c,
                     reduce_buf, tb.offs, tb.T, stride, scales_out);
  HIP_CHECK(hipGetLastError());
}

template <typename DP>
static void quantize_dispatch(Codec c, void* delta, const DevTable& tb,
                              const float* scales_dev, uint8_t* payload,
                              hipStream_t s, void* stats_out) {
  int g = grid_for(c == Codec::Int4 ? tb.pe / 2 : tb.pe);
  if (stats_out && g > 2048) g = 2048;  // bound the flush-atomic count
  auto* d = static_cast<typename DP::T*>(delta);
  switch (c) {
    case Codec::OneBit:
      hipLaunchKernelGGL((k_quant_1bit<DP>), dim3(g), dim3(BLOCK), 0, s, d,
                         tb.offs, tb.poffs, tb.T, tb.pe, scales_dev,
                         reinterpret_cast<uint64_t*>(payload),
                         static_cast<double*>(stats_out));
      break;
    case Codec::Fp8:
      hipLaunchKernelGGL((k_quant_fp8<DP>), dim3(g), dim3(BLOCK), 0, s, d,
                         tb.offs, tb.poffs, tb.T, tb.pe, scales_dev, payload,
                         static_cast<uint32_t*>(stats_out));
      break;
    case Codec::Int4:
      hipLaunchKernelGGL((k_quant_int4<DP>), dim3(g), dim3(BLOCK), 0, s, d,
                         tb.offs, tb.poffs, tb.T, tb.pe, scales_dev, payload,
                         static_cast<uint32_t*>(stats_out));
      break;
  }
}

void hip_quantize(Codec c, void* delta, bool delta_bf16, const DevTable& tb,
                  const float* scales_dev, uint8_t* payload, hipStream_t s,
                  void* stats_out) {
  if (delta_bf16)
    quantize_dispatch<DeltaBF16>(c, delta, tb, scales_dev, payload, s, stats_out);
  else
    quantize_dispatch<DeltaF32>(c, delta, tb, scales_dev, payload, s, stats_out);
  HIP_CHECK(hipGetLastError());
}

template <typename DP>
static void apply_dispatch(Codec c, const uint8_t* payload, const DevTable& tb,
                           const float* scales_dev, float* values, void* d1,
                           void* d2, hipStream_t s) {
  int g = grid_for(tb.pe);
  auto* t1 = static_cast<typename DP::T*>(d1);
  auto* t2 = static_cast<typename DP::T*>(d2);
  switch (c) {
    case Codec::OneBit:
      hipLaunchKernelGGL((k_apply<0, DP>), dim3(g), dim3(BLOCK), 0, s, payload,
                         tb.offs, tb.poffs, tb.T, tb.pe, scales_dev, values, t1, t2);
      break;
    case Codec::Fp8:
      hipLaunchKernelGGL((k_apply<1, DP>), dim3(g), dim3(BLOCK), 0, s, payload,
                         tb.offs, tb.poffs, tb.T, tb.pe, scales_dev, values, t1, t2);
      break;
    case Codec::Int4:
      hipLaunchKernelGGL((k_apply<2, DP>), dim3(g), dim3(BLOCK), 0, s, payload,
                         tb.offs, tb.poffs, tb.T, tb.pe, scales_dev, values, t1, t2);
      break;
  }
}

void hip_apply(Codec c, const uint8_t* payload, const DevTable& tb,
               const float* scales_dev, float* values, void* d1, void* d2,
               bool delta_bf16, hipStream_t s) {
  if (delta_bf16)
    apply_dispatch<DeltaBF16>(c, payload, tb, scales_dev, values, d1, d2, s);
  else
    apply_dispatch<DeltaF32>(c, payload, tb, scales_dev, values, d1, d2, s);
  HIP_CHECK(hipGetLastError());
}

void hip_add_scatter(const float* src, int64_t n, float alpha, float* values,
                     void* d1, void* d2, void* d3, bool delta_bf16,
                     hipStream_t s) {
  if (delta_bf16)
    hipLaunchKernelGGL((k_add_scatter<DeltaBF16>), dim3(grid_for(n)),
                       dim3(BLOCK), 0, s, src, n, alpha, values,
                       static_cast<uint16_t*>(d1), static_cast<uint16_t*>(d2),
                       static_cast<uint16_t*>(d3));
  else
    hipLaunchKernelGGL((k_add_scatter<DeltaF32>), dim3(grid_for(n)),
                       dim3(BLOCK), 0, s, src, n, alpha, values,
                       static_cast<float*>(d1), static_cast<float*>(d2),
                       static_cast<float*>(d3));
  HIP_CHECK(hipGetLastError());
}

void hip_snapshot_capture(const float* values, void* delta, bool delta_bf16,
                          float* out, int64_t n, hipStream_t s) {
  if (delta_bf16)
    hipLaunchKernelGGL((k_snapshot_capture<DeltaBF16>), dim3(grid_for(n)),
                       dim3(BLOCK), 0, s, values,
                       static_cast<uint16_t*>(delta), out, n);
  else
    hipLaunchKernelGGL((k_snapshot_capture<DeltaF32>), dim3(grid_for(n)),
                       dim3(BLOCK), 0, s, values, static_cast<float*>(delta),
                       out, n);
  HIP_CHECK(hipGetLastError());
}

void hip_add_delta_scatter(const void* src_delta, bool delta_bf16, int64_t n,
                           float* values, void* d1, void* d2, hipStream_t s) {
  if (delta_bf16)
    hipLaunchKernelGGL((k_add_delta_scatter<DeltaBF16>), dim3(grid_for(n)),
                       dim3(BLOCK), 0, s,
                       static_cast<const uint16_t*>(src_delta), n, values,
                       static_cast<uint16_t*>(d1), static_cast<uint16_t*>(d2));
  else
    hipLaunchKernelGGL((k_add_delta_scatter<DeltaF32>), dim3(grid_for(n)),
                       dim3(BLOCK), 0, s, static_cast<const float*>(src_delta),
                       n, values, static_cast<float*>(d1),
                       static_cast<float*>(d2));
  HIP_CHECK(hipGetLastError());
}

// Fused AdamW feeding the shared tensor — one HBM pass over {m, v, grad,
// values, link deltas}: decoupled weight decay against the pre-update
// master weight (torch.optim.AdamW semantics), fp32 m/v state, update
// applied to the replica with atomicAdd (concurrent gossip folds in) and
// staged into every link residual.  inv_bc1/2 = 1/(1-beta^t) host-side.
template <typename DP, typename GT, bool CLIP>
__global__ void k_fused_adamw(float* __restrict__ mom, float* __restrict__ vel,
                              const GT* __restrict__ grad,
                              uint16_t* __restrict__ shadow, float lr,
                              float beta1, float beta2, float eps, float wd,
                              float inv_bc1, float inv_bc2, int64_t n,
                              float* __restrict__ values, typename DP::T* d1,
                              typename DP::T* d2, typename DP::T* d3,
                              const ClipState* clip) {
  float coef = 1.0f;
  if (CLIP) {
    if (clip->skip) return;
    coef = clip->coef;
  }
  int64_t gstride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += gstride) {
    adamw_element<DP, GT, CLIP>(i, mom, vel, grad, shadow, lr, beta1, beta2,
                                eps, wd, inv_bc1, inv_bc2, coef, values, d1,
                                d2, d3);
  }
}

void hip_fused_adamw(float* mom, float* vel, const void* grad, bool grad_bf16,
                     uint16_t* shadow, float lr, float beta1, float beta2,
                     float eps, float wd, float inv_bc1, float inv_bc2,
                     int64_t n, float* values, void* d1, void* d2, void* d3,
                     bool delta_bf16, hipStream_t s, const ClipState* clip) {
  auto launch = [&](auto dp_tag, auto g_ptr, auto clip_tag) {
    using DP = decltype(dp_tag);
    using GT = std::remove_pointer_t<decltype(g_ptr)>;
    hipLaunchKernelGGL((k_fused_adamw<DP, GT, decltype(clip_tag)::value>),
                       dim3(grid_for(n)), dim3(BLOCK), 0, s, mom, vel, g_ptr,
                       shadow, lr, beta1, beta2, eps, wd, inv_bc1, inv_bc2, n,
                       values, static_cast<typename DP::T*>(d1),
                       static_cast<typename DP::T*>(d2),
                       static_cast<typename DP::T*>(d3), clip);
  };
  auto by_grad = [&](auto dp_tag, auto clip_tag) {
    if (grad_bf16) launch(dp_tag, static_cast<const uint16_t*>(grad), clip_tag);
    else launch(dp_tag, static_cast<const float*>(grad), clip_tag);
  };
  auto by_delta = [&](auto clip_tag) {
    if (delta_bf16) by_grad(DeltaBF16{}, clip_tag);
    else by_grad(DeltaF32{}, clip_tag);
  };
  if (clip) by_delta(std::true_type{});
  else by_delta(std::false_type{});
  HIP_CHECK(hipGetLastError());
}

void hip_fused_sgd(float* mom, const float* grad, float lr, float momentum,
                   int64_t n, float* values, void* d1, void* d2, void* d3,
                   bool delta_bf16, hipStream_t s, const ClipState* clip) {
  auto launch = [&](auto dp_tag, auto clip_tag) {
    using DP = decltype(dp_tag);
    hipLaunchKernelGGL((k_fused_sgd<DP, decltype(clip_tag)::value>),
                       dim3(grid_for(n)), dim3(BLOCK), 0, s, mom, grad, lr,
                       momentum, n, values, static_cast<typename DP::T*>(d1),
                       static_cast<typename DP::T*>(d2),
                       static_cast<typename DP::T*>(d3), clip);
  };
  auto by_delta = [&](auto clip_tag) {
    if (delta_bf16) launch(DeltaBF16{}, clip_tag);
    else launch(DeltaF32{}, clip_tag);
  };
  if (clip) by_delta(std::true_type{});
  else by_delta(std::false_type{});
  HIP_CHECK(hipGetLastError());
}

void hip_fused_sgd_bf16(float* mom, const uint16_t* grad, uint16_t* shadow,
                        float lr, float momentum, int64_t n, float* values,
                        void* d1, void* d2, void* d3, bool delta_bf16,
                        hipStream_t s, const ClipState* clip) {
  auto launch = [&](auto dp_tag, auto clip_tag) {
    using DP = decltype(dp_tag);
    hipLaunchKernelGGL((k_fused_sgd_bf16<DP, decltype(clip_tag)::value>),
                       dim3(grid_for(n)), dim3(BLOCK), 0, s, mom, grad, shadow,
                       lr, momentum, n, values,
                       static_cast<typename DP::T*>(d1),
                       static_cast<typename DP::T*>(d2),
                       static_cast<typename DP::T*>(d3), clip);
  };
  auto by_delta = [&](auto clip_tag) {
    if (delta_bf16) launch(DeltaBF16{}, clip_tag);
    else launch(DeltaF32{}, clip_tag);
  };
  if (clip) by_delta(std::true_type{});
  else by_delta(std::false_type{});
  HIP_CHECK(hipGetLastError());
}

}  // namespace shamd
