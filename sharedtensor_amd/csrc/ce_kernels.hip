// Fused bf16 cross-entropy for the training path.
//
// torch's route (autocast CE on (R=B*T, V=50257) bf16 logits) runs separate
// softmax forward + backward kernels with fp32 intermediates — ~6% of a
// GPT-2-small step.  Here:
//   fwd+grad: k_ce_fwd_grad, block per row with the whole row held in
//        registers: ONE read of the logits gives max, exp-sum, loss and the
//        bf16 dlogits for an upstream gradient of 1 (one read + one write of
//        the R x V matrix per step instead of three reads + one write)
//   fwd: stats only (no_grad / V beyond the register capacity): block per
//        row, independent max pass + exp-sum pass (fp32 math, fast-math exp
//        — outputs are bf16-rounded anyway); emits per-row loss and saves
//        (max, logsumexp) for backward
//   bwd: one pass writing bf16 dlogits = g * (softmax - onehot); in
//        skip_if_unit mode it returns at once when g == 1 (the one-pass
//        forward already wrote exactly that)
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <stdexcept>
#include <string>

#include "ce_common.h"  // device helpers shared with ce_opts_kernels.hip
#include "hip_api.h"

namespace shamd {

template <int BLK>
__global__ void k_ce_fwd(const uint16_t* __restrict__ logits,
                         const int32_t* __restrict__ targets,
                         float* __restrict__ loss, float* __restrict__ row_m,
                         float* __restrict__ row_lse, int64_t V) {
  // two independent passes (max, then sum of exp) — an online single pass
  // has a loop-carried (m, s) dependency per thread and measured 5x slower.
  // The second pass is a second trip to HBM / Infinity Cache (rows are
  // ~100 KB and ~25 MB are live per XCD against a 4 MiB L2); the training
  // path avoids it with k_ce_fwd_grad below.
  __shared__ float lds4[BLK / 64];
  const int64_t r = blockIdx.x;
  const uint16_t* xr = logits + r * V;
  const CeRow g = ce_row_split(xr, V);
  const uint4* xb = reinterpret_cast<const uint4*>(xr + g.head);
  const int e = threadIdx.x;
  const bool edge = e < g.head + g.tail;
  const float xe =
      edge ? bf16_to_f32(xr[ce_edge_index(g, e, V)]) : -INFINITY;

  float m = xe;
  for (int64_t c = threadIdx.x; c < g.nbody; c += BLK) m = fmaxf(m, ce_max8(xb[c]));
  m = block_max<BLK>(m, lds4);

  float s = edge ? __expf(xe - m) : 0.f;
  for (int64_t c = threadIdx.x; c < g.nbody; c += BLK) s += ce_expsum8(xb[c], m);
  float tot = block_sum<BLK>(s, lds4);
  if (threadIdx.x == 0) {
    float lse = __logf(tot) + m;
    float xt = bf16_to_f32(xr[targets[r]]);
    loss[r] = lse - xt;
    row_m[r] = m;
    row_lse[r] = lse;
  }
}

// One block per row, the row in registers: NCHUNK 16-byte chunks per thread,
// every load issued before the first use.  Unlike the LDS-staged attempt
// (see hip_ce_fwd) this keeps 16 waves per block and, at <= 64 VGPRs, two
// rows per CU, so one row's loads overlap the other's reduce and stores.
// Writes dlogits for an upstream gradient of exactly 1 with k_ce_bwd's
// formula and rounding; only the summation order inside lse differs.
// Measured (profiles/r04, R=65536, V=50257): <1024, 7> at 64 VGPRs, no
// scratch, 2.42 ms = 5.5 TB/s on one read + one write, against 5.65 ms for
// k_ce_fwd + k_ce_bwd before.  <1024, 16> (V up to 131072) sits at 128 VGPRs,
// one row per CU.
template <int BLK, int NCHUNK>
__global__ void __launch_bounds__(BLK, NCHUNK <= 7 ? 8 : 4)
k_ce_fwd_grad(const uint16_t* __restrict__ logits,
              const int32_t* __restrict__ targets, float* __restrict__ loss,
              float* __restrict__ row_lse, uint16_t* __restrict__ dlogits,
              float inv_r, int64_t V) {
  __shared__ float ldsw[BLK / 64];
  const int64_t r = blockIdx.x;
  const uint16_t* xr = logits + r * V;
  uint16_t* dr = dlogits + r * V;
  const CeRow g = ce_row_split(xr, V);
  const int nbody = static_cast<int>(g.nbody);  // <= BLK * NCHUNK (launcher)
  const uint4* xb = reinterpret_cast<const uint4*>(xr + g.head);

  // edge elements live in the last threads, which hold the fewest chunks
  const int e = BLK - 1 - static_cast<int>(threadIdx.x);
  const bool edge = e < g.head + g.tail;
  const int64_t ei = ce_edge_index(g, e, V);

  // masked lanes re-read the last chunk (never outside the row) and are
  // ignored below: a select per load would serialise the loads
  uint4 v[NCHUNK];
  if (nbody > 0) {
    const int last = nbody - 1;
#pragma unroll
    for (int k = 0; k < NCHUNK; ++k) {
      int c = k * BLK + static_cast<int>(threadIdx.x);
      v[k] = xb[c < last ? c : last];
    }
  } else {
#pragma unroll
    for (int k = 0; k < NCHUNK; ++k) v[k] = make_uint4(0, 0, 0, 0);
  }
  const float xe = edge ? bf16_to_f32(xr[ei]) : -INFINITY;
  const int tgt = targets[r];

  float m = xe;
#pragma unroll
  for (int k = 0; k < NCHUNK; ++k)
    if (k * BLK + static_cast<int>(threadIdx.x) < nbody) m = fmaxf(m, ce_max8(v[k]));
  m = block_max<BLK>(m, ldsw);

  float s = edge ? __expf(xe - m) : 0.f;
#pragma unroll
  for (int k = 0; k < NCHUNK; ++k)
    if (k * BLK + static_cast<int>(threadIdx.x) < nbody) s += ce_expsum8(v[k], m);
  const float tot = block_sum<BLK>(s, ldsw);
  const float lse = __logf(tot) + m;
  if (threadIdx.x == 0) {
    loss[r] = lse - bf16_to_f32(xr[tgt]);
    row_lse[r] = lse;
  }

  uint16_t* db = dr + g.head;
  const bool aligned = (reinterpret_cast<uintptr_t>(db) & 15) == 0;
#pragma unroll
  for (int k = 0; k < NCHUNK; ++k) {
    int c = k * BLK + static_cast<int>(threadIdx.x);
    if (c < nbody)
      ce_store8(db + 8 * c, ce_grad8(v[k], lse, inv_r, tgt - g.head - 8 * c),
                aligned);
  }
  if (edge) dr[ei] = f32_to_bf16(ce_grad1(xe, lse, inv_r, ei == tgt));
}

// Grid-stride over rows.  SKIP_IF_UNIT: the buffer already holds the g == 1
// result from k_ce_fwd_grad, so every block returns when *gscale_dev is
// exactly 1 (decided on the device: no host sync) and otherwise recomputes
// the rows from logits and row_lse as usual — no double rounding.
template <int BLK, bool SKIP_IF_UNIT>
__global__ void k_ce_bwd(const uint16_t* __restrict__ logits,
                         const int32_t* __restrict__ targets,
                         const float* __restrict__ row_lse,
                         uint16_t* __restrict__ dlogits,
                         const float* __restrict__ gscale_dev, float inv_r,
                         int64_t R, int64_t V) {
  const float gup = *gscale_dev;  // upstream grad read on device: no host
                                  // sync in the backward pass
  if (SKIP_IF_UNIT && gup == 1.0f) return;
  const float gscale = gup * inv_r;
  for (int64_t r = blockIdx.x; r < R; r += gridDim.x) {
    const uint16_t* xr = logits + r * V;
    uint16_t* dr = dlogits + r * V;
    const float lse = row_lse[r];
    const int64_t tgt = targets[r];
    const CeRow g = ce_row_split(xr, V);
    const uint4* xb = reinterpret_cast<const uint4*>(xr + g.head);
    uint16_t* db = dr + g.head;
    const bool aligned = (reinterpret_cast<uintptr_t>(db) & 15) == 0;
    // four 16-byte loads in flight per thread: one at a time leaves the
    // loop bound by load latency
    constexpr int U = 4;
    const int64_t t0 = tgt - g.head;
    int64_t c = threadIdx.x;
    for (; c + (U - 1) * BLK < g.nbody; c += U * BLK) {
      uint4 u[U];
#pragma unroll
      for (int i = 0; i < U; ++i) u[i] = xb[c + i * BLK];
#pragma unroll
      for (int i = 0; i < U; ++i) {
        int64_t ci = c + i * BLK;
        ce_store8(db + 8 * ci, ce_grad8(u[i], lse, gscale, ce_clamp_d(t0 - 8 * ci)),
                  aligned);
      }
    }
    for (; c < g.nbody; c += BLK)
      ce_store8(db + 8 * c, ce_grad8(xb[c], lse, gscale, ce_clamp_d(t0 - 8 * c)),
                aligned);
    const int e = threadIdx.x;
    if (e < g.head + g.tail) {
      int64_t ei = ce_edge_index(g, e, V);
      dr[ei] = f32_to_bf16(
          ce_grad1(bf16_to_f32(xr[ei]), lse, gscale, ei == tgt));
    }
  }
}

void hip_ce_fwd(const void* logits, const int32_t* targets, float* loss,
                float* row_m, float* row_lse, int64_t R, int64_t V,
                hipStream_t s) {
  // NOTE (measured, profiles/r02): an LDS-staged single-read variant
  // (whole 100 KB row resident in the 160 KiB LDS) ran 4x SLOWER than this
  // two-pass kernel -- at 100 KB/block only one block fits per CU and four
  // waves cannot hide the global-load latency; the second pass's re-read
  // is cheaper than the lost occupancy.
  // block-size knob (SHTENS_CE_BLOCK=512); measured r02: 512 is within
  // noise of 256 (2.63 vs 2.66 ms fwd) — the kernel is bound by the
  // re-read + exp throughput, not wave count — so 256 stays default
  const char* e = std::getenv("SHTENS_CE_BLOCK");
  if (e && std::atoi(e) == 512)
    hipLaunchKernelGGL(k_ce_fwd<512>, dim3(static_cast<uint32_t>(R)),
                       dim3(512), 0, s,
                       static_cast<const uint16_t*>(logits), targets, loss,
                       row_m, row_lse, V);
  else
    hipLaunchKernelGGL(k_ce_fwd<CE_BLOCK>, dim3(static_cast<uint32_t>(R)),
                       dim3(CE_BLOCK), 0, s,
                       static_cast<const uint16_t*>(logits), targets, loss,
                       row_m, row_lse, V);
  HIP_CHECK(hipGetLastError());
}

// register capacity of the k_ce_fwd_grad instantiations: ce_common.h
int64_t hip_ce_fwd_grad_max_v() { return CE_ROW_CAP16; }

void hip_ce_fwd_grad(const void* logits, const int32_t* targets, float* loss,
                     float* row_lse, void* dlogits, float inv_r, int64_t R,
                     int64_t V, hipStream_t s) {
  if (V < 1 || V > CE_ROW_CAP16)
    throw std::runtime_error("hip_ce_fwd_grad: V beyond the register capacity");
  if (V <= CE_ROW_CAP7)
    hipLaunchKernelGGL((k_ce_fwd_grad<CE_ROW_BLOCK, 7>),
                       dim3(static_cast<uint32_t>(R)), dim3(CE_ROW_BLOCK), 0,
                       s, static_cast<const uint16_t*>(logits), targets, loss,
                       row_lse, static_cast<uint16_t*>(dlogits), inv_r, V);
  else
    hipLaunchKernelGGL((k_ce_fwd_grad<CE_ROW_BLOCK, 16>),
                       dim3(static_cast<uint32_t>(R)), dim3(CE_ROW_BLOCK), 0,
                       s, static_cast<const uint16_t*>(logits), targets, loss,
                       row_lse, static_cast<uint16_t*>(dlogits), inv_r, V);
  HIP_CHECK(hipGetLastError());
}

template <int BLK>
static void launch_ce_bwd(const void* logits, const int32_t* targets,
                          const float* row_lse, void* dlogits,
                          const float* gscale_dev, float inv_r, int64_t R,
                          int64_t V, bool skip_if_unit, hipStream_t s) {
  // skip_if_unit: a bounded grid (2048 threads fill each of the 256 CUs),
  // so the usual no-op costs one wave of blocks (6 us measured) instead of
  // R empty ones.  The full pass keeps one block per row: on the bounded
  // grid it measured 3.36 ms against 2.62 ms (R=65536, V=50257).
  const int64_t cap = skip_if_unit ? 256 * (2048 / BLK) : (int64_t(1) << 31) - 1;
  const dim3 grid(static_cast<uint32_t>(R < cap ? R : cap));
  if (skip_if_unit)
    hipLaunchKernelGGL((k_ce_bwd<BLK, true>), grid, dim3(BLK), 0, s,
                       static_cast<const uint16_t*>(logits), targets, row_lse,
                       static_cast<uint16_t*>(dlogits), gscale_dev, inv_r, R,
                       V);
  else
    hipLaunchKernelGGL((k_ce_bwd<BLK, false>), grid, dim3(BLK), 0, s,
                       static_cast<const uint16_t*>(logits), targets, row_lse,
                       static_cast<uint16_t*>(dlogits), gscale_dev, inv_r, R,
                       V);
}

void hip_ce_bwd(const void* logits, const int32_t* targets,
                const float* row_lse, void* dlogits, const float* gscale_dev,
                float inv_r, int64_t R, int64_t V, bool skip_if_unit,
                hipStream_t s) {
  if (R <= 0) return;
  const char* e = std::getenv("SHTENS_CE_BLOCK");
  if (e && std::atoi(e) == 512)
    launch_ce_bwd<512>(logits, targets, row_lse, dlogits, gscale_dev, inv_r,
                       R, V, skip_if_unit, s);
  else
    launch_ce_bwd<CE_BLOCK>(logits, targets, row_lse, dlogits, gscale_dev,
                            inv_r, R, V, skip_if_unit, s);
  HIP_CHECK(hipGetLastError());
}

}  // namespace shamd
