// Fused bf16 rotary position embedding for the Llama q/k pair: ONE kernel
// per direction rotates q (B, Hq, T, D) and k (B, Hkv, T, D) together.
//
// Eager apply_rope runs, per tensor, two strided slices, four fp32
// multiplies, a subtract, an add, a stack and a cast (~10 kernels, fp32
// intermediates saved for backward), twice per layer; autograd replays a
// longer chain.  In passes over the bf16 activation A = q + k (an fp32
// half-width intermediate is one A, a full-width one two):
//   fwd: read A, write A          (2 passes vs 19 for eager: 4 muls at 1.5,
//        sub + add at 3 each, stack 4, cast 3)
//   bwd: read dA, write dA        (2 passes; eager replays a longer chain
//        and sums the two gradient terms in bf16)
// The rotation's gradient is the rotation by the negated angle, so the same
// kernel serves backward (INVERSE) and no activation is saved.
//
// Both sides are addressed by element strides for B, H and T (D contiguous):
// forward reads the (B,T,H,D) storage the q/k projections wrote and writes
// (B,H,T,D) for SDPA; backward does the reverse, so neither direction needs
// a layout copy.  16-byte accesses (8 bf16 = 4 pairs per lane) when D % 8
// == 0 and everything is 16-byte aligned, a pair-per-lane path otherwise.
//
// Arithmetic reproduces the eager fp32 op sequence exactly — separate
// multiplies, one add/subtract, one round to bf16 — so contraction into FMA
// is switched off where the rotation is computed.
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#include "device_util.h"
#include "hip_api.h"

namespace shamd {

// (o1, o2) = rotation of (x1, x2) by the angle whose cos/sin are c/s, as
// bf16 pair bits.  o1 = rn(x1*c) - rn(x2*s), o2 = rn(x1*s) + rn(x2*c): no
// FMA, so the result is bit-identical to the eager mul/mul/sub kernels.
static __device__ __forceinline__ uint32_t rp_rot(float x1, float x2, float c,
                                                  float s) {
#pragma clang fp contract(off)
  float a = x1 * c;
  float b = x2 * s;
  float d = x1 * s;
  float e = x2 * c;
  float o1 = a - b;
  float o2 = d + e;
  return bf16x2_pack(o1, o2);
}

constexpr int RP_BLOCK = 256;

// One tensor's two sides: element strides, D contiguous.
struct RopeSide {
  const uint16_t* in;
  uint16_t* out;
  int64_t isb, ish, ist;
  int64_t osb, osh, ost;
};

// Work item = VEC consecutive elements of one (b, h, t) row; within a batch
// entry the items are ordered (t, h, chunk) over the Hq + Hkv heads, so
// neighbouring lanes share a cos/sin row.  blockIdx.y strides over b.
//   nchunk = D / VEC, W = (Hq + Hkv) * nchunk, TW = T * W (< 2^31, checked
//   by the host); chunk_shift = log2(nchunk) or -1.
template <int VEC, bool INVERSE>
__global__ void __launch_bounds__(RP_BLOCK)
k_rope_qk(RopeSide q, RopeSide k, const float* __restrict__ cos,
          const float* __restrict__ sin, int64_t B, uint32_t Hq,
          uint32_t nchunk, int chunk_shift, uint32_t W, uint32_t TW,
          int64_t half) {
  const uint32_t step = gridDim.x * RP_BLOCK;
  for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
    for (uint32_t idx = blockIdx.x * RP_BLOCK + threadIdx.x; idx < TW;
         idx += step) {
      uint32_t t = idx / W;
      uint32_t j = idx - t * W;
      uint32_t h = chunk_shift >= 0 ? (j >> chunk_shift) : (j / nchunk);
      uint32_t ch = j - h * nchunk;
      bool is_q = h < Hq;
      int64_t hh = is_q ? h : h - Hq;
      int64_t d0 = static_cast<int64_t>(ch) * VEC;
      const uint16_t* ip =
          (is_q ? q.in : k.in) + b * (is_q ? q.isb : k.isb) +
          hh * (is_q ? q.ish : k.ish) +
          static_cast<int64_t>(t) * (is_q ? q.ist : k.ist) + d0;
      uint16_t* op =
          (is_q ? q.out : k.out) + b * (is_q ? q.osb : k.osb) +
          hh * (is_q ? q.osh : k.osh) +
          static_cast<int64_t>(t) * (is_q ? q.ost : k.ost) + d0;
      int64_t tab = static_cast<int64_t>(t) * half + (d0 >> 1);
      if constexpr (VEC == 8) {
        uint4 x = *reinterpret_cast<const uint4*>(ip);
        float4 c = *reinterpret_cast<const float4*>(cos + tab);
        float4 s = *reinterpret_cast<const float4*>(sin + tab);
        if (INVERSE) {
          s.x = -s.x; s.y = -s.y; s.z = -s.z; s.w = -s.w;
        }
        uint4 o;
        o.x = rp_rot(bf16x2_lo(x.x), bf16x2_hi(x.x), c.x, s.x);
        o.y = rp_rot(bf16x2_lo(x.y), bf16x2_hi(x.y), c.y, s.y);
        o.z = rp_rot(bf16x2_lo(x.z), bf16x2_hi(x.z), c.z, s.z);
        o.w = rp_rot(bf16x2_lo(x.w), bf16x2_hi(x.w), c.w, s.w);
        *reinterpret_cast<uint4*>(op) = o;
      } else {
        float x1 = bf16_to_f32(ip[0]);
        float x2 = bf16_to_f32(ip[1]);
        float c = cos[tab];
        float s = INVERSE ? -sin[tab] : sin[tab];
        uint32_t o = rp_rot(x1, x2, c, s);
        op[0] = static_cast<uint16_t>(o & 0xFFFFu);
        op[1] = static_cast<uint16_t>(o >> 16);
      }
    }
  }
}

static inline bool rp_aligned16(const void* p) {
  return (reinterpret_cast<uintptr_t>(p) & 15u) == 0;
}
static inline bool rp_strides8(const RopeStrides& s) {
  return s.b % 8 == 0 && s.h % 8 == 0 && s.t % 8 == 0;
}

template <int VEC>
static void rp_launch(const RopeSide& q, const RopeSide& k, const float* cos,
                      const float* sin, int64_t B, int64_t Hq, int64_t Hkv,
                      int64_t T, int64_t D, bool inverse, hipStream_t s) {
  int64_t nchunk = D / VEC;
  int64_t W = (Hq + Hkv) * nchunk;
  int64_t TW = T * W;
  if (TW >= (int64_t(1) << 31))
    throw std::runtime_error("rope: T*(Hq+Hkv)*D too large for one batch "
                             "entry's work index");
  int shift = -1;
  if ((nchunk & (nchunk - 1)) == 0)
    for (shift = 0; (int64_t(1) << shift) < nchunk; ++shift) {}
  int64_t gx = (TW + RP_BLOCK - 1) / RP_BLOCK;
  if (gx > 4096) gx = 4096;
  int64_t gy = B < 1024 ? B : 1024;
  dim3 grid(static_cast<unsigned>(gx), static_cast<unsigned>(gy));
  auto kern = inverse ? k_rope_qk<VEC, true> : k_rope_qk<VEC, false>;
  hipLaunchKernelGGL(kern, grid, dim3(RP_BLOCK), 0, s, q, k, cos, sin, B,
                     static_cast<uint32_t>(Hq), static_cast<uint32_t>(nchunk),
                     shift, static_cast<uint32_t>(W),
                     static_cast<uint32_t>(TW), D / 2);
  HIP_CHECK(hipGetLastError());
}

void hip_rope_qk(const void* q, const void* k, void* q_out, void* k_out,
                 const float* cos, const float* sin, int64_t B, int64_t Hq,
                 int64_t Hkv, int64_t T, int64_t D, const RopeStrides& q_in,
                 const RopeStrides& k_in, const RopeStrides& q_os,
                 const RopeStrides& k_os, bool inverse, hipStream_t s) {
  if (!q || !q_out || !cos || !sin)
    throw std::runtime_error("rope: null q, q_out, cos or sin pointer");
  if (D <= 0 || D % 2)
    throw std::runtime_error("rope: head dim must be even and positive");
  if (B < 0 || T < 0 || Hq <= 0 || Hkv < 0)
    throw std::runtime_error("rope: bad shape");
  if (!k) Hkv = 0;  // single-tensor use
  if (Hkv > 0 && !k_out)
    throw std::runtime_error("rope: k given without k_out");
  if (B == 0 || T == 0) return;

  RopeSide qs{static_cast<const uint16_t*>(q), static_cast<uint16_t*>(q_out),
              q_in.b, q_in.h, q_in.t, q_os.b, q_os.h, q_os.t};
  RopeSide ks = qs;  // never dereferenced when Hkv == 0
  if (Hkv > 0)
    ks = RopeSide{static_cast<const uint16_t*>(k),
                  static_cast<uint16_t*>(k_out),
                  k_in.b, k_in.h, k_in.t, k_os.b, k_os.h, k_os.t};

  bool vec = D % 8 == 0 && rp_aligned16(q) && rp_aligned16(q_out) &&
             rp_aligned16(cos) && rp_aligned16(sin) && rp_strides8(q_in) &&
             rp_strides8(q_os);
  if (vec && Hkv > 0)
    vec = rp_aligned16(k) && rp_aligned16(k_out) && rp_strides8(k_in) &&
          rp_strides8(k_os);
  if (vec)
    rp_launch<8>(qs, ks, cos, sin, B, Hq, Hkv, T, D, inverse, s);
  else
    rp_launch<2>(qs, ks, cos, sin, B, Hq, Hkv, T, D, inverse, s);
}

}  // namespace shamd
