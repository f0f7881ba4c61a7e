// Fused bf16 cross-entropy with ignore_index, label smoothing and z-loss.
//
// Same one-pass design as ce_kernels.hip (one read of a logits row, one
// write of its dlogits row), through the same device helpers (ce_common.h).
// Row r is valid when targets[r] != ignore_index and 0 <= targets[r] < V;
// per valid row, in fp32:
//   loss_r = (1-eps)*(lse - x_t) + eps*(lse - (1/V)*sum_j x_j) + z*lse^2
//   dx_j   = g * inv_count * [(1 + 2*z*lse)*exp(x_j - lse)
//                             - (1-eps)*[j == t] - eps/V]
// with inv_count = 1 / (number of valid rows), counted on the device:
//   scan:     k_ce_opts_scan, one block over the R targets, writes the
//             16-byte CeOptState (hip_api.h) that the other kernels read
//             from device memory — no host sync anywhere
//   fwd+grad: k_ce_opts_fwd_grad, k_ce_fwd_grad's block-per-row kernel
//   fwd:      k_ce_opts_fwd, stats only (no_grad / V beyond the registers)
//   bwd:      k_ce_opts_bwd, k_ce_bwd with the same options
// A row that is not valid is never read: the decision is taken from the
// target alone, uniformly across the block, before any logits load.  Its
// dlogits row is +0 (stored with the valid rows' head/body/tail split, so
// nothing outside the row is written), its row_lse 0 and its loss_r 0 — or
// NaN when the target is out of range and not ignore_index, which makes the
// mean NaN.
// EXTRA is the compile-time switch "smoothing or z-loss on".  With EXTRA
// false a valid row runs k_ce_fwd_grad's / k_ce_bwd's operation chain
// exactly (same loads, reductions, ce_grad1, gscale = inv_count) and pays
// for no extra reduction.
#include <hip/hip_runtime.h>

#include <cmath>
#include <stdexcept>
#include <string>
#include <type_traits>

#include "ce_common.h"
#include "hip_api.h"

namespace shamd {

enum : int { CE_ROW_VALID = 0, CE_ROW_IGNORED = 1, CE_ROW_BAD = 2 };

static __device__ __forceinline__ int ce_row_kind(int64_t t, int64_t V,
                                                  int ignore, int has_ignore) {
  if (has_ignore && t == ignore) return CE_ROW_IGNORED;
  return (t >= 0 && t < V) ? CE_ROW_VALID : CE_ROW_BAD;
}

// acc + the 8 elements of a chunk, on the packed pairs (v_dot2c_f32_bf16
// against (1, 1): fp32 accumulate, every product exact).  Unpacking to
// floats here made the compiler keep the unpacked row live next to the
// packed one: 37 spilled VGPRs in the 7-chunk one-pass kernel.
typedef __bf16 ce_bf16x2 __attribute__((ext_vector_type(2)));
static __device__ __forceinline__ float ce_pair_sum(uint32_t p, float acc) {
  return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(ce_bf16x2, p),
                                         __builtin_bit_cast(ce_bf16x2, 0x3F803F80u),
                                         acc, false);
}
static __device__ __forceinline__ float ce_sum8(const uint4& u, float acc) {
  return ce_pair_sum(u.w, ce_pair_sum(u.z, ce_pair_sum(u.y, ce_pair_sum(u.x, acc))));
}

// loss_r of a valid row; sx = sum_j x_j (unused unless EXTRA)
template <bool EXTRA>
static __device__ __forceinline__ float ce_row_loss(float lse, float xt,
                                                    float sx, int64_t V,
                                                    float eps, float z) {
  if constexpr (EXTRA)
    return (1.f - eps) * (lse - xt) + eps * (lse - sx / static_cast<float>(V)) +
           z * lse * lse;
  else
    return lse - xt;
}

// block-uniform value into a scalar register (the value is unchanged)
static __device__ __forceinline__ float ce_uniform(float v) {
  return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}

// Per-row gradient coefficients.  EXTRA false: ce_grad1 / ce_grad8 as they
// are, on gscale.  EXTRA true: dx = a*softmax - b - c*[hot] with the three
// row constants a = gscale*(1 + 2*z*lse), b = gscale*eps/V and
// c = gscale*(1-eps) held in scalar registers (lse is block-uniform), so
// the register-resident row keeps its vector registers; the multiply-add is
// spelled out so that the one-pass kernel and the backward kernel round
// alike.
template <bool EXTRA>
struct CeGrad {
  float gscale;   // g * inv_count
  float a, nb, c;

  __device__ __forceinline__ float one(float x, float lse, bool hot) const {
    if constexpr (EXTRA) {
      float t = __fmaf_rn(a, __expf(x - lse), nb);
      return hot ? t - c : t;
    } else {
      return ce_grad1(x, lse, gscale, hot);
    }
  }
  __device__ __forceinline__ uint32_t pair(uint32_t p, float lse, int d) const {
    return bf16x2_pack(one(bf16x2_lo(p), lse, d == 0),
                       one(bf16x2_hi(p), lse, d == 1));
  }
  // d = (target index) - (index of the chunk's first elem)
  __device__ __forceinline__ uint4 chunk(const uint4& u, float lse, int d) const {
    if constexpr (EXTRA) {
      uint4 o;
      o.x = pair(u.x, lse, d);
      o.y = pair(u.y, lse, d - 2);
      o.z = pair(u.z, lse, d - 4);
      o.w = pair(u.w, lse, d - 6);
      return o;
    } else {
      return ce_grad8(u, lse, gscale, d);
    }
  }
};

template <bool EXTRA>
static __device__ __forceinline__ CeGrad<EXTRA> ce_make_grad(float gscale,
                                                             float lse,
                                                             int64_t V,
                                                             float eps,
                                                             float z) {
  CeGrad<EXTRA> c;
  c.gscale = gscale;
  if constexpr (EXTRA) {
    c.a = ce_uniform(gscale * (1.f + 2.f * z * lse));
    c.nb = ce_uniform(-(gscale * (eps / static_cast<float>(V))));
    c.c = ce_uniform(gscale * (1.f - eps));
  } else {
    c.a = c.nb = c.c = 0.f;
  }
  return c;
}

// +0 into every element of a dlogits row, split like a valid row's stores
template <int BLK>
static __device__ __forceinline__ void ce_zero_row(uint16_t* dr, const CeRow& g,
                                                   int64_t V) {
  uint16_t* db = dr + g.head;
  const bool aligned = (reinterpret_cast<uintptr_t>(db) & 15) == 0;
  const uint4 zero = make_uint4(0, 0, 0, 0);
  for (int64_t c = threadIdx.x; c < g.nbody; c += BLK)
    ce_store8(db + 8 * c, zero, aligned);
  const int e = threadIdx.x;
  if (e < g.head + g.tail) dr[ce_edge_index(g, e, V)] = 0;
}

// One block strides over the targets; per-thread counts are combined with a
// wave shuffle tree and an in-order LDS sum: no atomics, one fixed order.
template <int BLK>
__global__ void __launch_bounds__(BLK)
k_ce_opts_scan(const int32_t* __restrict__ targets, int64_t R, int64_t V,
               int ignore, int has_ignore, CeOptState* __restrict__ state) {
  __shared__ uint32_t lv[BLK / 64], lb[BLK / 64];
  uint32_t nv = 0, nb = 0;
  for (int64_t r = threadIdx.x; r < R; r += BLK) {
    const int k = ce_row_kind(targets[r], V, ignore, has_ignore);
    nv += k == CE_ROW_VALID;
    nb += k == CE_ROW_BAD;
  }
  for (int w = 32; w > 0; w >>= 1) {
    nv += __shfl_down(nv, w, 64);
    nb += __shfl_down(nb, w, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    lv[threadIdx.x >> 6] = nv;
    lb[threadIdx.x >> 6] = nb;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t tv = 0, tb = 0;
    for (int i = 0; i < BLK / 64; ++i) {
      tv += lv[i];
      tb += lb[i];
    }
    state->inv_count = __fdiv_rn(1.0f, static_cast<float>(tv));
    state->n_valid = tv;
    state->n_bad = tb;
    state->pad = 0;
  }
}

// k_ce_fwd_grad (ce_kernels.hip) with the options; see there for the design.
template <int BLK, int NCHUNK, bool EXTRA>
__global__ void __launch_bounds__(BLK, NCHUNK <= 7 ? 8 : 4)
k_ce_opts_fwd_grad(const uint16_t* __restrict__ logits,
                   const int32_t* __restrict__ targets,
                   float* __restrict__ loss, float* __restrict__ row_lse,
                   uint16_t* __restrict__ dlogits,
                   const CeOptState* __restrict__ state, int64_t V, int ignore,
                   int has_ignore, float eps, float z) {
  __shared__ float ldsw[BLK / 64];
  const int64_t r = blockIdx.x;
  const uint16_t* xr = logits + r * V;
  uint16_t* dr = dlogits + r * V;
  const CeRow g = ce_row_split(xr, V);
  const int tgt = targets[r];

  // block-uniform (blockIdx and kernel arguments only), before any load
  const int kind = ce_row_kind(tgt, V, ignore, has_ignore);
  if (kind != CE_ROW_VALID) {
    ce_zero_row<BLK>(dr, g, V);
    if (threadIdx.x == 0) {
      loss[r] = kind == CE_ROW_BAD ? NAN : 0.f;
      row_lse[r] = 0.f;
    }
    return;
  }

  const int nbody = static_cast<int>(g.nbody);  // <= BLK * NCHUNK (launcher)
  const uint4* xb = reinterpret_cast<const uint4*>(xr + g.head);

  // edge elements live in the last threads, which hold the fewest chunks
  const int e = BLK - 1 - static_cast<int>(threadIdx.x);
  const bool edge = e < g.head + g.tail;
  // EXTRA: V fits an int, and the narrower index is the register that
  // keeps the 7-chunk instantiation at 64 VGPRs without a spill (the plain
  // one fits with k_ce_fwd_grad's 64-bit index and spills with this one)
  using edge_index_t = std::conditional_t<EXTRA, int, int64_t>;
  const edge_index_t ei = static_cast<edge_index_t>(ce_edge_index(g, e, V));

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
  const float inv_count = state->inv_count;

  float m = xe;
#pragma unroll
  for (int k = 0; k < NCHUNK; ++k)
    if (k * BLK + static_cast<int>(threadIdx.x) < nbody) m = fmaxf(m, ce_max8(v[k]));
  m = block_max<BLK>(m, ldsw);

  // EXTRA: one more block reduction, sum_j x_j; block-uniform results move
  // to scalar registers so the row keeps the vector ones
  float sx = 0.f;
  if constexpr (EXTRA) {
    m = ce_uniform(m);
    float a = edge ? xe : 0.f;
#pragma unroll
    for (int k = 0; k < NCHUNK; ++k)
      if (k * BLK + static_cast<int>(threadIdx.x) < nbody) a = ce_sum8(v[k], a);
    sx = ce_uniform(block_sum<BLK>(a, ldsw));
  }

  float s = edge ? __expf(xe - m) : 0.f;
#pragma unroll
  for (int k = 0; k < NCHUNK; ++k)
    if (k * BLK + static_cast<int>(threadIdx.x) < nbody) s += ce_expsum8(v[k], m);
  const float tot = block_sum<BLK>(s, ldsw);
  float lse = __logf(tot) + m;
  if constexpr (EXTRA) lse = ce_uniform(lse);

  // EXTRA: lse and sx sit in scalar registers, so the longer loss formula
  // waits until the row's registers are free (after the stores)
  if constexpr (!EXTRA) {
    if (threadIdx.x == 0) {
      loss[r] = ce_row_loss<EXTRA>(lse, bf16_to_f32(xr[tgt]), sx, V, eps, z);
      row_lse[r] = lse;
    }
  }

  const CeGrad<EXTRA> cg = ce_make_grad<EXTRA>(inv_count, lse, V, eps, z);
  uint16_t* db = dr + g.head;
  const bool aligned = (reinterpret_cast<uintptr_t>(db) & 15) == 0;
#pragma unroll
  for (int k = 0; k < NCHUNK; ++k) {
    int c = k * BLK + static_cast<int>(threadIdx.x);
    if (c < nbody)
      ce_store8(db + 8 * c, cg.chunk(v[k], lse, tgt - g.head - 8 * c), aligned);
  }
  if (edge) dr[ei] = f32_to_bf16(cg.one(xe, lse, ei == tgt));
  if constexpr (EXTRA) {
    if (threadIdx.x == 0) {
      loss[r] = ce_row_loss<EXTRA>(lse, bf16_to_f32(xr[tgt]), sx, V, eps, z);
      row_lse[r] = lse;
    }
  }
}

// k_ce_fwd (ce_kernels.hip) with the options: stats only, two passes.
template <int BLK, bool EXTRA>
__global__ void k_ce_opts_fwd(const uint16_t* __restrict__ logits,
                              const int32_t* __restrict__ targets,
                              float* __restrict__ loss,
                              float* __restrict__ row_lse, int64_t V,
                              int ignore, int has_ignore, float eps, float z) {
  __shared__ float lds4[BLK / 64];
  const int64_t r = blockIdx.x;
  const int tgt = targets[r];
  const int kind = ce_row_kind(tgt, V, ignore, has_ignore);
  if (kind != CE_ROW_VALID) {
    if (threadIdx.x == 0) {
      loss[r] = kind == CE_ROW_BAD ? NAN : 0.f;
      row_lse[r] = 0.f;
    }
    return;
  }
  const uint16_t* xr = logits + r * V;
  const CeRow g = ce_row_split(xr, V);
  const uint4* xb = reinterpret_cast<const uint4*>(xr + g.head);
  const int e = threadIdx.x;
  const bool edge = e < g.head + g.tail;
  const float xe =
      edge ? bf16_to_f32(xr[ce_edge_index(g, e, V)]) : -INFINITY;

  float m = xe;
  float a = edge ? xe : 0.f;
  for (int64_t c = threadIdx.x; c < g.nbody; c += BLK) {
    const uint4 u = xb[c];
    m = fmaxf(m, ce_max8(u));
    if constexpr (EXTRA) a = ce_sum8(u, a);
  }
  m = block_max<BLK>(m, lds4);
  float sx = 0.f;
  if constexpr (EXTRA) sx = block_sum<BLK>(a, lds4);

  float s = edge ? __expf(xe - m) : 0.f;
  for (int64_t c = threadIdx.x; c < g.nbody; c += BLK) s += ce_expsum8(xb[c], m);
  float tot = block_sum<BLK>(s, lds4);
  if (threadIdx.x == 0) {
    float lse = __logf(tot) + m;
    loss[r] = ce_row_loss<EXTRA>(lse, bf16_to_f32(xr[tgt]), sx, V, eps, z);
    row_lse[r] = lse;
  }
}

// k_ce_bwd (ce_kernels.hip) with the options.  Grid-stride over rows;
// SKIP_IF_UNIT: the buffer already holds the g == 1 result from
// k_ce_opts_fwd_grad, so every block returns when *gscale_dev is exactly 1.
template <int BLK, bool SKIP_IF_UNIT, bool EXTRA>
__global__ void k_ce_opts_bwd(const uint16_t* __restrict__ logits,
                              const int32_t* __restrict__ targets,
                              const float* __restrict__ row_lse,
                              uint16_t* __restrict__ dlogits,
                              const float* __restrict__ gscale_dev,
                              const CeOptState* __restrict__ state, int64_t R,
                              int64_t V, int ignore, int has_ignore, float eps,
                              float z) {
  const float gup = *gscale_dev;  // upstream grad read on device: no host
                                  // sync in the backward pass
  if (SKIP_IF_UNIT && gup == 1.0f) return;
  const float gscale = gup * state->inv_count;
  for (int64_t r = blockIdx.x; r < R; r += gridDim.x) {
    const uint16_t* xr = logits + r * V;
    uint16_t* dr = dlogits + r * V;
    const int64_t tgt = targets[r];
    const CeRow g = ce_row_split(xr, V);
    if (ce_row_kind(tgt, V, ignore, has_ignore) != CE_ROW_VALID) {
      ce_zero_row<BLK>(dr, g, V);
      continue;
    }
    const float lse = row_lse[r];
    const CeGrad<EXTRA> cg = ce_make_grad<EXTRA>(gscale, lse, V, eps, z);
    const uint4* xb = reinterpret_cast<const uint4*>(xr + g.head);
    uint16_t* db = dr + g.head;
    const bool aligned = (reinterpret_cast<uintptr_t>(db) & 15) == 0;
    // four 16-byte loads in flight per thread, as k_ce_bwd
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
        ce_store8(db + 8 * ci, cg.chunk(u[i], lse, ce_clamp_d(t0 - 8 * ci)),
                  aligned);
      }
    }
    for (; c < g.nbody; c += BLK)
      ce_store8(db + 8 * c, cg.chunk(xb[c], lse, ce_clamp_d(t0 - 8 * c)),
                aligned);
    const int e = threadIdx.x;
    if (e < g.head + g.tail) {
      int64_t ei = ce_edge_index(g, e, V);
      dr[ei] = f32_to_bf16(cg.one(bf16_to_f32(xr[ei]), lse, ei == tgt));
    }
  }
}

static void ce_opts_check(const char* who, const CeOpts& o, int64_t R,
                          int64_t V) {
  if (R < 1 || R > (int64_t(1) << 31) - 1 || V < 1)
    throw std::invalid_argument(std::string(who) + ": bad shape");
  if (!(o.eps >= 0.f && o.eps < 1.f) || !(o.z >= 0.f) || !std::isfinite(o.z))
    throw std::invalid_argument(std::string(who) +
                                ": label_smoothing must be in [0, 1) and "
                                "z_loss finite and >= 0");
}

static bool ce_opts_extra(const CeOpts& o) { return o.eps != 0.f || o.z != 0.f; }

void hip_ce_opts_scan(const int32_t* targets, int64_t R, int64_t V,
                      const CeOpts& o, CeOptState* state, hipStream_t s) {
  ce_opts_check("hip_ce_opts_scan", o, R, V);
  // R*4 bytes (256 KB at R = 65536): one block striding over R is enough
  hipLaunchKernelGGL(k_ce_opts_scan<CE_ROW_BLOCK>, dim3(1), dim3(CE_ROW_BLOCK),
                     0, s, targets, R, V, o.ignore_index,
                     o.has_ignore ? 1 : 0, state);
  HIP_CHECK(hipGetLastError());
}

template <int NCHUNK, bool EXTRA>
static void launch_ce_opts_fwd_grad(const void* logits, const int32_t* targets,
                                    float* loss, float* row_lse, void* dlogits,
                                    const CeOptState* state, const CeOpts& o,
                                    int64_t R, int64_t V, hipStream_t s) {
  hipLaunchKernelGGL((k_ce_opts_fwd_grad<CE_ROW_BLOCK, NCHUNK, EXTRA>),
                     dim3(static_cast<uint32_t>(R)), dim3(CE_ROW_BLOCK), 0, s,
                     static_cast<const uint16_t*>(logits), targets, loss,
                     row_lse, static_cast<uint16_t*>(dlogits), state, V,
                     o.ignore_index, o.has_ignore ? 1 : 0, o.eps, o.z);
}

void hip_ce_opts_fwd_grad(const void* logits, const int32_t* targets,
                          float* loss, float* row_lse, void* dlogits,
                          const CeOptState* state, const CeOpts& o, int64_t R,
                          int64_t V, hipStream_t s) {
  ce_opts_check("hip_ce_opts_fwd_grad", o, R, V);
  if (V > CE_ROW_CAP16)
    throw std::runtime_error(
        "hip_ce_opts_fwd_grad: V beyond the register capacity");
  const bool x = ce_opts_extra(o);
  if (V <= CE_ROW_CAP7) {
    if (x)
      launch_ce_opts_fwd_grad<7, true>(logits, targets, loss, row_lse, dlogits,
                                       state, o, R, V, s);
    else
      launch_ce_opts_fwd_grad<7, false>(logits, targets, loss, row_lse,
                                        dlogits, state, o, R, V, s);
  } else {
    if (x)
      launch_ce_opts_fwd_grad<16, true>(logits, targets, loss, row_lse,
                                        dlogits, state, o, R, V, s);
    else
      launch_ce_opts_fwd_grad<16, false>(logits, targets, loss, row_lse,
                                         dlogits, state, o, R, V, s);
  }
  HIP_CHECK(hipGetLastError());
}

void hip_ce_opts_fwd(const void* logits, const int32_t* targets, float* loss,
                     float* row_lse, const CeOpts& o, int64_t R, int64_t V,
                     hipStream_t s) {
  ce_opts_check("hip_ce_opts_fwd", o, R, V);
  const dim3 grid(static_cast<uint32_t>(R));
  if (ce_opts_extra(o))
    hipLaunchKernelGGL((k_ce_opts_fwd<CE_BLOCK, true>), grid, dim3(CE_BLOCK),
                       0, s, static_cast<const uint16_t*>(logits), targets,
                       loss, row_lse, V, o.ignore_index, o.has_ignore ? 1 : 0,
                       o.eps, o.z);
  else
    hipLaunchKernelGGL((k_ce_opts_fwd<CE_BLOCK, false>), grid, dim3(CE_BLOCK),
                       0, s, static_cast<const uint16_t*>(logits), targets,
                       loss, row_lse, V, o.ignore_index, o.has_ignore ? 1 : 0,
                       o.eps, o.z);
  HIP_CHECK(hipGetLastError());
}

template <bool SKIP, bool EXTRA>
static void launch_ce_opts_bwd(const void* logits, const int32_t* targets,
                               const float* row_lse, void* dlogits,
                               const float* gscale_dev,
                               const CeOptState* state, const CeOpts& o,
                               int64_t R, int64_t V, hipStream_t s) {
  // grids as launch_ce_bwd: bounded for the usual no-op, block per row for
  // the full pass
  const int64_t cap = SKIP ? 256 * (2048 / CE_BLOCK) : (int64_t(1) << 31) - 1;
  const dim3 grid(static_cast<uint32_t>(R < cap ? R : cap));
  hipLaunchKernelGGL((k_ce_opts_bwd<CE_BLOCK, SKIP, EXTRA>), grid,
                     dim3(CE_BLOCK), 0, s,
                     static_cast<const uint16_t*>(logits), targets, row_lse,
                     static_cast<uint16_t*>(dlogits), gscale_dev, state, R, V,
                     o.ignore_index, o.has_ignore ? 1 : 0, o.eps, o.z);
}

void hip_ce_opts_bwd(const void* logits, const int32_t* targets,
                     const float* row_lse, void* dlogits,
                     const float* gscale_dev, const CeOptState* state,
                     const CeOpts& o, int64_t R, int64_t V, bool skip_if_unit,
                     hipStream_t s) {
  ce_opts_check("hip_ce_opts_bwd", o, R, V);
  const bool x = ce_opts_extra(o);
  if (skip_if_unit) {
    if (x)
      launch_ce_opts_bwd<true, true>(logits, targets, row_lse, dlogits,
                                     gscale_dev, state, o, R, V, s);
    else
      launch_ce_opts_bwd<true, false>(logits, targets, row_lse, dlogits,
                                      gscale_dev, state, o, R, V, s);
  } else {
    if (x)
      launch_ce_opts_bwd<false, true>(logits, targets, row_lse, dlogits,
                                      gscale_dev, state, o, R, V, s);
    else
      launch_ce_opts_bwd<false, false>(logits, targets, row_lse, dlogits,
                                       gscale_dev, state, o, R, V, s);
  }
  HIP_CHECK(hipGetLastError());
}

}  // namespace shamd
