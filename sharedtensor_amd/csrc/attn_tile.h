// What the attention forward (attn_fwd_tile.h) and backward (attn_bwd_tile.h)
// tile headers share: vector types, the workgroup shape, the strides struct,
// the workgroup-to-XCD grid map, and the launchers' checks of the problem,
// the strides and the grid.  Everything sits in an anonymous namespace: each
// kernel file gets its own copy, inlined.
//
// The guarded 16-byte load and the lane-half exchange are not here: each
// header keeps the form its kernels were tuned with.  The head-dim-64
// forward sits at exactly 128 VGPRs, and with the backward's vector-typed
// load and ds_bpermute exchange it spills 12 bytes per lane to scratch
// (profiles/r15/).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <initializer_list>

#include "device_util.h"

namespace shamd {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kRW = 32;         // rows (queries or keys) per wave
constexpr int kWaves = 4;
constexpr int kRB = kRW * kWaves;  // rows per workgroup
constexpr int kTile = 64;       // rows per LDS tile
constexpr int kXcd = 8;
constexpr float kLog2e = 1.4426950408889634f;

struct AttnStrides {
  int64_t b, t, h;  // elements
};

// blockIdx -> (batch*head, block slot): block ids round-robin over the XCDs,
// the blocks of one (b, h) consecutive on one XCD
__device__ __forceinline__ bool grid_map(int nbh, int nblk, int& bh,
                                         int& slot_in_bh) {
  const int xcd = blockIdx.x % kXcd;
  const int slot = blockIdx.x / kXcd;
  bh = (slot / nblk) * kXcd + xcd;
  slot_in_bh = slot % nblk;
  return bh < nbh;
}

// ------------------------------------------------------------------ host

inline AttnStrides strides3(const int64_t* p) {
  return AttnStrides{p[0], p[1], p[2]};
}

// Shape, scale and lse stride of a launch; returns G = Hq / Hkv.  A grouped
// op takes G in {2, 4, 8}; the MHA ops pass Hq == Hkv and grouped = false.
inline int64_t check_attn_problem(const char* op, int64_t B, int64_t Hq,
                                  int64_t Hkv, int64_t T, int64_t lse_stride,
                                  float scale, bool grouped) {
  if (B <= 0 || Hq <= 0 || Hkv <= 0 || T <= 0)
    throw std::runtime_error(std::string(op) + ": empty problem");
  if (Hq % Hkv)
    throw std::runtime_error(std::string(op) +
                             ": Hq must be a multiple of Hkv");
  const int64_t G = Hq / Hkv;
  if (grouped && G != 2 && G != 4 && G != 8)
    throw std::runtime_error(std::string(op) + ": group size must be 2, 4 or 8");
  if (!(scale > 0.f) || scale > 3.0e38f)
    throw std::runtime_error(std::string(op) + ": scale must be positive");
  if (lse_stride < T)
    throw std::runtime_error(std::string(op) + ": lse row shorter than T");
  return G;
}

inline void check_attn_strides(const char* op,
                               std::initializer_list<const int64_t*> strides) {
  for (const int64_t* st : strides)
    for (int i = 0; i < 3; ++i)
      if (st[i] < 0 || st[i] % 8)
        throw std::runtime_error(std::string(op) +
                                 ": strides must be multiples of 8 elements");
}

// nbk = B * Hkv rounded up to whole XCD rounds, times the blocks of one
// (b, kv head): the grid of every attention kernel
inline int64_t attn_grid(const char* op, int64_t B, int64_t Hq, int64_t Hkv,
                         int64_t T, int64_t blocks) {
  const int64_t grid = (B * Hkv + kXcd - 1) / kXcd * kXcd * blocks;
  if (grid > 0x7fffffff || T > (1 << 30) || B * Hq > 0x7fffffff)
    throw std::runtime_error(std::string(op) + ": problem too large");
  return grid;
}

}  // namespace
}  // namespace shamd
