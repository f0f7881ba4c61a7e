// Parameter-group variants of the fused optimizer steps (gfx950).
//
// Same single HBM pass and same per-element operation chain as k_fused_sgd,
// k_fused_sgd_bf16 and k_fused_adamw (the bodies are shared, optim_step.h),
// but the learning rate and the weight decay come from the group table of
// common.h: element i uses fl32(lr * lr_scale[g]) and weight_decay[g] of
// the group g of the segment that holds i.
//
// Geometry: that of the ungrouped kernels.  256-thread blocks, block b
// handles the tiles b, b + gridDim.x, ... of GROUP_TILE = 256 contiguous
// elements, thread t the element t of the tile, so every buffer is touched
// in the same pattern and exactly as often.
//
// Table access.  Per tile, not per element:
//   * the block binary-searches the segment of the tile's first element.
//     Index and address are the same in all lanes, so these are scalar
//     loads of an L2-resident table (<= 12 steps at the segment cap);
//   * a tile that lies inside that segment (all but S - 1 of them) takes
//     its rate and decay from those uniform values: no LDS, no barrier;
//   * a tile with a boundary in it stages the next GROUP_TILE segments, one
//     per thread, into LDS (tile-relative end, rate, decay: 3 KB).  Every
//     segment holds at least one element, so these cover the tile.  Each
//     thread then finds its own segment with 8 LDS probes.
// Offsets are int64 throughout; only tile-relative ends (<= 256) are int.
//
// bf16 residuals: an element's packed atomic carries its own u in its half
// and -0.0 in the other (DeltaBF16::atomic_add), so a pair whose halves
// belong to different groups needs no special case.
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>
#include <type_traits>

#include "device_util.h"
#include "hip_api.h"
#include "optim_step.h"

namespace shamd {

static_assert(GROUP_TILE == 256, "one element per thread of a 256-block");

static inline int group_grid_for(int64_t n) {
  int64_t g = (n + GROUP_TILE - 1) / GROUP_TILE;
  return static_cast<int>(
      g < GROUP_GRID_BLOCKS ? (g > 0 ? g : 1) : GROUP_GRID_BLOCKS);
}

// Calls body(i, lr_eff, wd) once for every i in [0, n).  All threads of the
// block must enter (barriers inside).
template <typename Body>
__device__ __forceinline__ void for_each_grouped(
    const int32_t* __restrict__ table, float lr, int64_t n, Body&& body) {
  __shared__ int s_end[GROUP_TILE];
  __shared__ float s_lr[GROUP_TILE];
  __shared__ float s_wd[GROUP_TILE];

  const int S = table[2];
  const int G = table[3];
  const int64_t* __restrict__ seg_end =
      reinterpret_cast<const int64_t*>(table + GROUP_HEADER_WORDS);
  const int32_t* __restrict__ seg_group =
      table + GROUP_HEADER_WORDS + 2 * static_cast<int64_t>(S);
  const float* __restrict__ lr_scale =
      reinterpret_cast<const float*>(seg_group + S);
  const float* __restrict__ wdecay = lr_scale + G;

  const int tid = threadIdx.x;
  const int64_t ntiles = (n + GROUP_TILE - 1) / GROUP_TILE;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t t0 = tile * GROUP_TILE;
    // first segment that ends after t0: the one that holds t0
    int lo = 0, hi = S - 1;
    while (lo < hi) {
      int mid = (lo + hi) >> 1;
      if (seg_end[mid] > t0) hi = mid; else lo = mid + 1;
    }
    float lr_e, wd_e;
    if (seg_end[lo] - t0 >= GROUP_TILE) {
      const int g = seg_group[lo];
      lr_e = mul_uncontracted(lr, lr_scale[g]);
      wd_e = wdecay[g];
    } else {
      __syncthreads();  // readers of the previous boundary tile are done
      const int s = lo + tid;
      int rel = GROUP_TILE;  // past the table: never the answer below n
      float l = 0.f, w = 0.f;
      if (s < S) {
        const int64_t e = seg_end[s] - t0;
        if (e < GROUP_TILE) rel = static_cast<int>(e);
        const int g = seg_group[s];
        l = mul_uncontracted(lr, lr_scale[g]);
        w = wdecay[g];
      }
      s_end[tid] = rel;
      s_lr[tid] = l;
      s_wd[tid] = w;
      __syncthreads();
      // first staged segment that ends after this thread's element
      int a = 0, b = GROUP_TILE - 1;
      while (a < b) {
        int mid = (a + b) >> 1;
        if (s_end[mid] > tid) b = mid; else a = mid + 1;
      }
      lr_e = s_lr[a];
      wd_e = s_wd[a];
    }
    const int64_t i = t0 + tid;
    if (i < n) body(i, lr_e, wd_e);
  }
}

// CLIP: as in the ungrouped kernels.  skip set: every thread returns before
// it touches any buffer (and before any barrier: the state is the same for
// all of them).
template <typename DP, bool CLIP>
__global__ void
k_fused_sgd_grp(float* __restrict__ mom, const float* __restrict__ grad,
                float lr, float momentum, int64_t n, float* values,
                typename DP::T* d1, typename DP::T* d2, typename DP::T* d3,
                const ClipState* clip, const int32_t* __restrict__ table) {
  float coef = 1.0f;
  if (CLIP) {
    if (clip->skip) return;
    coef = clip->coef;
  }
  for_each_grouped(table, lr, n, [&](int64_t i, float lr_e, float) {
    sgd_element<DP, CLIP>(i, mom, grad, lr_e, momentum, coef, values, d1, d2,
                          d3);
  });
}

template <typename DP, bool CLIP>
__global__ void
k_fused_sgd_bf16_grp(float* __restrict__ mom,
                     const uint16_t* __restrict__ grad,
                     uint16_t* __restrict__ shadow, float lr, float momentum,
                     int64_t n, float* __restrict__ values,
                     typename DP::T* d1, typename DP::T* d2,
                     typename DP::T* d3, const ClipState* clip,
                     const int32_t* __restrict__ table) {
  float coef = 1.0f;
  if (CLIP) {
    if (clip->skip) return;
    coef = clip->coef;
  }
  for_each_grouped(table, lr, n, [&](int64_t i, float lr_e, float) {
    sgd_bf16_element<DP, CLIP>(i, mom, grad, shadow, lr_e, momentum, coef,
                               values, d1, d2, d3);
  });
}

template <typename DP, typename GT, bool CLIP>
__global__ void
k_fused_adamw_grp(float* __restrict__ mom, float* __restrict__ vel,
                  const GT* __restrict__ grad, uint16_t* __restrict__ shadow,
                  float lr, float beta1, float beta2, float eps,
                  float inv_bc1, float inv_bc2, int64_t n,
                  float* __restrict__ values, typename DP::T* d1,
                  typename DP::T* d2, typename DP::T* d3,
                  const ClipState* clip, const int32_t* __restrict__ table) {
  float coef = 1.0f;
  if (CLIP) {
    if (clip->skip) return;
    coef = clip->coef;
  }
  for_each_grouped(table, lr, n, [&](int64_t i, float lr_e, float wd_e) {
    adamw_element<DP, GT, CLIP>(i, mom, vel, grad, shadow, lr_e, beta1, beta2,
                                eps, wd_e, inv_bc1, inv_bc2, coef, values, d1,
                                d2, d3);
  });
}

// -------------------------------------------------------------- launchers

void hip_fused_adamw_grouped(float* mom, float* vel, const void* grad,
                             bool grad_bf16, uint16_t* shadow, float lr,
                             float beta1, float beta2, float eps,
                             float inv_bc1, float inv_bc2, int64_t n,
                             float* values, void* d1, void* d2, void* d3,
                             bool delta_bf16, hipStream_t s,
                             const ClipState* clip, const void* table) {
  if (!table) throw std::invalid_argument("grouped step without a group table");
  auto tab = static_cast<const int32_t*>(table);
  auto launch = [&](auto dp_tag, auto g_ptr, auto clip_tag) {
    using DP = decltype(dp_tag);
    using GT = std::remove_pointer_t<decltype(g_ptr)>;
    hipLaunchKernelGGL((k_fused_adamw_grp<DP, GT, decltype(clip_tag)::value>),
                       dim3(group_grid_for(n)), dim3(GROUP_TILE), 0, s, mom,
                       vel, g_ptr, shadow, lr, beta1, beta2, eps, inv_bc1,
                       inv_bc2, n, values, static_cast<typename DP::T*>(d1),
                       static_cast<typename DP::T*>(d2),
                       static_cast<typename DP::T*>(d3), clip, tab);
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

void hip_fused_sgd_grouped(float* mom, const float* grad, float lr,
                           float momentum, int64_t n, float* values, void* d1,
                           void* d2, void* d3, bool delta_bf16, hipStream_t s,
                           const ClipState* clip, const void* table) {
  if (!table) throw std::invalid_argument("grouped step without a group table");
  auto tab = static_cast<const int32_t*>(table);
  auto launch = [&](auto dp_tag, auto clip_tag) {
    using DP = decltype(dp_tag);
    hipLaunchKernelGGL((k_fused_sgd_grp<DP, decltype(clip_tag)::value>),
                       dim3(group_grid_for(n)), dim3(GROUP_TILE), 0, s, mom,
                       grad, lr, momentum, n, values,
                       static_cast<typename DP::T*>(d1),
                       static_cast<typename DP::T*>(d2),
                       static_cast<typename DP::T*>(d3), clip, tab);
  };
  auto by_delta = [&](auto clip_tag) {
    if (delta_bf16) launch(DeltaBF16{}, clip_tag);
    else launch(DeltaF32{}, clip_tag);
  };
  if (clip) by_delta(std::true_type{});
  else by_delta(std::false_type{});
  HIP_CHECK(hipGetLastError());
}

void hip_fused_sgd_bf16_grouped(float* mom, const uint16_t* grad,
                                uint16_t* shadow, float lr, float momentum,
                                int64_t n, float* values, void* d1, void* d2,
                                void* d3, bool delta_bf16, hipStream_t s,
                                const ClipState* clip, const void* table) {
  if (!table) throw std::invalid_argument("grouped step without a group table");
  auto tab = static_cast<const int32_t*>(table);
  auto launch = [&](auto dp_tag, auto clip_tag) {
    using DP = decltype(dp_tag);
    hipLaunchKernelGGL((k_fused_sgd_bf16_grp<DP, decltype(clip_tag)::value>),
                       dim3(group_grid_for(n)), dim3(GROUP_TILE), 0, s, mom,
                       grad, shadow, lr, momentum, n, values,
                       static_cast<typename DP::T*>(d1),
                       static_cast<typename DP::T*>(d2),
                       static_cast<typename DP::T*>(d3), clip, tab);
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
