// Device helpers shared by the fused cross-entropy kernel files
// (ce_kernels.hip: plain mean; ce_opts_kernels.hip: ignore_index, label
// smoothing, z-loss), so that both run one operation chain: the
// head/body/tail row split and the per-chunk max / exp-sum / gradient / store
// steps.  bf16 packing and the block reductions come from device_util.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <stdexcept>
#include <string>

#include "device_util.h"

namespace shamd {

constexpr int CE_BLOCK = 256;  // 4 waves (fwd: measured vs 512, see launcher)

// register capacity of the one-pass fwd+grad instantiations: 1024 threads x
// NCHUNK chunks x 8 elements (the <= 7-element head and tail ride on top)
constexpr int CE_ROW_BLOCK = 1024;
constexpr int64_t CE_ROW_CAP7 = int64_t(CE_ROW_BLOCK) * 7 * 8;    // GPT-2
constexpr int64_t CE_ROW_CAP16 = int64_t(CE_ROW_BLOCK) * 16 * 8;  // Llama

// Rows are only 2-byte aligned when V is odd (GPT-2: V = 50257), so each
// row is processed as [head: up to 7 elems | body: 16-byte-aligned chunks of
// 8 elems | tail: up to 7 elems].  The body moves with 16-byte loads and
// stores; the at most 14 edge elements go one by one, edge e to "edge
// thread" e, so nothing outside the row is ever read or written.
struct CeRow {
  int head, tail;
  int64_t nbody;  // 16-byte chunks
};

static __device__ __forceinline__ CeRow ce_row_split(const uint16_t* xr,
                                                     int64_t V) {
  CeRow g;
  int h = static_cast<int>((16 - (reinterpret_cast<uintptr_t>(xr) & 15)) & 15) >> 1;
  g.head = h < V ? h : static_cast<int>(V);
  g.nbody = (V - g.head) >> 3;
  g.tail = static_cast<int>(V - g.head - (g.nbody << 3));
  return g;
}

// row index of edge element e (e < head + tail)
static __device__ __forceinline__ int64_t ce_edge_index(const CeRow& g, int e,
                                                        int64_t V) {
  return e < g.head ? e : V - g.tail + (e - g.head);
}

static __device__ __forceinline__ float ce_max8(const uint4& u) {
  float a = fmaxf(fmaxf(bf16x2_lo(u.x), bf16x2_hi(u.x)),
                  fmaxf(bf16x2_lo(u.y), bf16x2_hi(u.y)));
  float b = fmaxf(fmaxf(bf16x2_lo(u.z), bf16x2_hi(u.z)),
                  fmaxf(bf16x2_lo(u.w), bf16x2_hi(u.w)));
  return fmaxf(a, b);
}

static __device__ __forceinline__ float ce_expsum8(const uint4& u, float m) {
  float a = __expf(bf16x2_lo(u.x) - m) + __expf(bf16x2_hi(u.x) - m);
  float b = __expf(bf16x2_lo(u.y) - m) + __expf(bf16x2_hi(u.y) - m);
  float c = __expf(bf16x2_lo(u.z) - m) + __expf(bf16x2_hi(u.z) - m);
  float d = __expf(bf16x2_lo(u.w) - m) + __expf(bf16x2_hi(u.w) - m);
  return (a + b) + (c + d);
}

static __device__ __forceinline__ float ce_grad1(float x, float lse,
                                                 float gscale, bool hot) {
  return gscale * (__expf(x - lse) - (hot ? 1.f : 0.f));
}

// gradient of one pair; d = (target index) - (index of the pair's low elem)
static __device__ __forceinline__ uint32_t ce_grad_pair(uint32_t p, float lse,
                                                        float gscale, int d) {
  return bf16x2_pack(ce_grad1(bf16x2_lo(p), lse, gscale, d == 0),
                     ce_grad1(bf16x2_hi(p), lse, gscale, d == 1));
}

// gradient of one body chunk; d = (target index) - (index of its first elem)
static __device__ __forceinline__ uint4 ce_grad8(const uint4& u, float lse,
                                                 float gscale, int d) {
  uint4 o;
  o.x = ce_grad_pair(u.x, lse, gscale, d);
  o.y = ce_grad_pair(u.y, lse, gscale, d - 2);
  o.z = ce_grad_pair(u.z, lse, gscale, d - 4);
  o.w = ce_grad_pair(u.w, lse, gscale, d - 6);
  return o;
}

// target offset of a chunk as an int; anything outside [0, 8) is "not here"
static __device__ __forceinline__ int ce_clamp_d(int64_t d) {
  return d < -8 ? -8 : (d > 8 ? 8 : static_cast<int>(d));
}

// dlogits rows have the logits' 16-byte phase whenever both buffers start on
// a 16-byte boundary (every torch allocation); a view at another offset
// stores its body element-wise instead
static __device__ __forceinline__ void ce_store8(uint16_t* dst, const uint4& o,
                                                 bool aligned) {
  if (aligned) {
    *reinterpret_cast<uint4*>(dst) = o;
  } else {
    dst[0] = static_cast<uint16_t>(o.x);
    dst[1] = static_cast<uint16_t>(o.x >> 16);
    dst[2] = static_cast<uint16_t>(o.y);
    dst[3] = static_cast<uint16_t>(o.y >> 16);
    dst[4] = static_cast<uint16_t>(o.z);
    dst[5] = static_cast<uint16_t>(o.z >> 16);
    dst[6] = static_cast<uint16_t>(o.w);
    dst[7] = static_cast<uint16_t>(o.w >> 16);
  }
}

}  // namespace shamd
