// Fused bf16 cross-entropy for the training path: the plain mean loss and
// the one with ignore_index, label smoothing and z-loss, one kernel family.
//
// torch's route (autocast CE on (R=B*T, V=50257) bf16 logits) runs separate
// softmax forward + backward kernels with fp32 intermediates — ~6% of a
// GPT-2-small step.  Here:
//   fwd+grad: k_ce_fwd_grad, block per row with the whole row held in
//        registers: ONE read of the logits gives max, exp-sum, loss and the
//        bf16 dlogits for an upstream gradient of 1 (one read + one write of
//        the R x V matrix per step instead of three reads + one write)
//   fwd: k_ce_fwd, stats only (no_grad / V beyond the register capacity):
//        block per row, independent max pass + exp-sum pass (fp32 math,
//        fast-math exp — outputs are bf16-rounded anyway); emits per-row
//        loss and saves (max, logsumexp) for backward
//   bwd: k_ce_bwd, one pass writing bf16 dlogits = g * (softmax - onehot);
//        in skip_if_unit mode it returns at once when g == 1 (the one-pass
//        forward already wrote exactly that)
//   scan: k_ce_opts_scan, one block over the R targets, writes the 16-byte
//        CeOptState (hip_api.h) that the option kernels read from device
//        memory — no host sync anywhere
//
// Each kernel is written once and templated on a row policy, passed by value
// as its last argument (CePlain, CeMasked, CeMaskedExtra below).  With the
// options, row r is valid when targets[r] != ignore_index and
// 0 <= targets[r] < V; per valid row, in fp32:
//   loss_r = (1-eps)*(lse - x_t) + eps*(lse - (1/V)*sum_j x_j) + z*lse^2
//   dx_j   = g * inv_count * [(1 + 2*z*lse)*exp(x_j - lse)
//                             - (1-eps)*[j == t] - eps/V]
// with inv_count = 1 / (number of valid rows), counted on the device.
// A row that is not valid is never read: the decision is taken from the
// target alone, uniformly across the block, before any logits load.  Its
// dlogits row is +0 (stored with the valid rows' head/body/tail split, so
// nothing outside the row is written), its row_lse 0 and its loss_r 0 — or
// NaN when the target is out of range and not ignore_index, which makes the
// mean NaN.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <type_traits>

#include "device_util.h"
#include "hip_api.h"

namespace shamd {

constexpr int CE_BLOCK = 256;  // 4 waves (fwd: measured vs 512, see launcher)

// register capacity of the one-pass fwd+grad instantiations: 1024 threads x
// NCHUNK chunks x 8 elements (the <= 7-element head and tail ride on top)
constexpr int CE_ROW_BLOCK = 1024;
constexpr int64_t CE_ROW_CAP7 = int64_t(CE_ROW_BLOCK) * 7 * 8;    // GPT-2
constexpr int64_t CE_ROW_CAP16 = int64_t(CE_ROW_BLOCK) * 16 * 8;  // Llama

// ------------------------------------------------------------ row policies

enum : int { CE_ROW_VALID = 0, CE_ROW_IGNORED = 1, CE_ROW_BAD = 2 };

static __device__ __forceinline__ int ce_row_kind(int64_t t, int64_t V,
                                                  int ignore, int has_ignore) {
  if (has_ignore && t == ignore) return CE_ROW_IGNORED;
  return (t >= 0 && t < V) ? CE_ROW_VALID : CE_ROW_BAD;
}

// What differs between the plain mean and the options.  MASKED: rows are
// classified by ce_row_kind and 1/count comes from CeOptState.  EXTRA is the
// compile-time switch "smoothing or z-loss on"; without it a valid row runs
// the plain operation chain exactly (same loads, reductions, ce_grad1) and
// pays for no extra reduction.  The kernels branch on these with
// `if constexpr` only.

// Mean over all R rows.  No target check: xr[targets[r]] is read as it is.
struct CePlain {
  static constexpr bool MASKED = false, EXTRA = false;
  float inv_r;  // 1 / R
  __device__ __forceinline__ float inv_count() const { return inv_r; }
};

// ignore_index and out-of-range targets; mean over the valid rows.
struct CeMasked {
  static constexpr bool MASKED = true, EXTRA = false;
  const CeOptState* state;  // written by k_ce_opts_scan (unused by k_ce_fwd)
  int ignore, has_ignore;
  // Read through the constant address space (nothing writes the state while
  // a kernel that reads it runs): a uniform load from there is a scalar load.
  // A pointer inside a by-value argument cannot be __restrict__, and without
  // that the one-pass kernel holds the value in a vector register from the
  // row loads to the stores.
  __device__ __forceinline__ float inv_count() const {
    using ConstState = const CeOptState __attribute__((address_space(4)));
    return ((ConstState*)state)->inv_count;
  }
  __device__ __forceinline__ int kind(int64_t t, int64_t V) const {
    return ce_row_kind(t, V, ignore, has_ignore);
  }
};

// CeMasked plus label smoothing eps and z-loss weight z.  The two are kept
// 8 bytes apart: side by side they are fetched as one <2 x float>, and with
// that the 7-chunk one-pass kernel spills 4 VGPRs.
struct CeMaskedExtra : CeMasked {
  static constexpr bool EXTRA = true;
  float eps;
  alignas(8) float z;
};

// ------------------------------------------------------------- row helpers

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
template <class P>
static __device__ __forceinline__ float ce_row_loss(const P& p, float lse,
                                                    float xt, float sx,
                                                    int64_t V) {
  if constexpr (P::EXTRA)
    return (1.f - p.eps) * (lse - xt) +
           p.eps * (lse - sx / static_cast<float>(V)) + p.z * lse * lse;
  else
    return lse - xt;
}

// block-uniform value into a scalar register (the value is unchanged)
static __device__ __forceinline__ float ce_uniform(float v) {
  return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
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

template <class P>
static __device__ __forceinline__ CeGrad<P::EXTRA> ce_make_grad(const P& p,
                                                                float gscale,
                                                                float lse,
                                                                int64_t V) {
  CeGrad<P::EXTRA> c;
  c.gscale = gscale;
  if constexpr (P::EXTRA) {
    c.a = ce_uniform(gscale * (1.f + 2.f * p.z * lse));
    c.nb = ce_uniform(-(gscale * (p.eps / static_cast<float>(V))));
    c.c = ce_uniform(gscale * (1.f - p.eps));
  } else {
    c.a = c.nb = c.c = 0.f;
  }
  return c;
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

// loss and row_lse of a row that is not valid
static __device__ __forceinline__ void ce_invalid_row_stats(int kind, int64_t r,
                                                            float* loss,
                                                            float* row_lse) {
  if (threadIdx.x == 0) {
    loss[r] = kind == CE_ROW_BAD ? NAN : 0.f;
    row_lse[r] = 0.f;
  }
}

// ----------------------------------------------------------------- kernels

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

// Stats only.  row_m may be null (the option path does not save it).
template <int BLK, class P>
__global__ void k_ce_fwd(const uint16_t* __restrict__ logits,
                         const int32_t* __restrict__ targets,
                         float* __restrict__ loss, float* __restrict__ row_m,
                         float* __restrict__ row_lse, int64_t V, P p) {
  // two independent passes (max, then sum of exp) — an online single pass
  // has a loop-carried (m, s) dependency per thread and measured 5x slower.
  // The second pass is a second trip to HBM / Infinity Cache (rows are
  // ~100 KB and ~25 MB are live per XCD against a 4 MiB L2); the training
  // path avoids it with k_ce_fwd_grad below.
  __shared__ float lds4[BLK / 64];
  const int64_t r = blockIdx.x;
  int tgt = 0;
  if constexpr (P::MASKED) {
    tgt = targets[r];
    const int kind = p.kind(tgt, V);
    if (kind != CE_ROW_VALID) {
      ce_invalid_row_stats(kind, r, loss, row_lse);
      return;
    }
  }
  const uint16_t* xr = logits + r * V;
  const CeRow g = ce_row_split(xr, V);
  const uint4* xb = reinterpret_cast<const uint4*>(xr + g.head);
  const int e = threadIdx.x;
  const bool edge = e < g.head + g.tail;
  const float xe =
      edge ? bf16_to_f32(xr[ce_edge_index(g, e, V)]) : -INFINITY;

  // EXTRA: sum_j x_j rides on the max pass
  float m = xe;
  float a = edge ? xe : 0.f;
  for (int64_t c = threadIdx.x; c < g.nbody; c += BLK) {
    const uint4 u = xb[c];
    m = fmaxf(m, ce_max8(u));
    if constexpr (P::EXTRA) a = ce_sum8(u, a);
  }
  m = block_max<BLK>(m, lds4);
  float sx = 0.f;
  if constexpr (P::EXTRA) sx = block_sum<BLK>(a, lds4);

  float s = edge ? __expf(xe - m) : 0.f;
  for (int64_t c = threadIdx.x; c < g.nbody; c += BLK) s += ce_expsum8(xb[c], m);
  float tot = block_sum<BLK>(s, lds4);
  if (threadIdx.x == 0) {
    float lse = __logf(tot) + m;
    if constexpr (!P::MASKED) tgt = targets[r];
    loss[r] = ce_row_loss(p, lse, bf16_to_f32(xr[tgt]), sx, V);
    if (row_m) row_m[r] = m;
    row_lse[r] = lse;
  }
}

// One block per row, the row in registers: NCHUNK 16-byte chunks per thread,
// every load issued before the first use.  Unlike the LDS-staged attempt
// (see hip_ce_fwd) this keeps 16 waves per block and, at <= 64 VGPRs, two
// rows per CU, so one row's loads overlap the other's reduce and stores.
// Writes dlogits for an upstream gradient of exactly 1 with k_ce_bwd's
// formula and rounding; only the summation order inside lse differs.
// Measured (profiles/r04, R=65536, V=50257): <1024, 7, CePlain> at 64 VGPRs,
// no scratch, 2.42 ms = 5.5 TB/s on one read + one write, against 5.65 ms
// for k_ce_fwd + k_ce_bwd before.  <1024, 16> (V up to 131072) sits at 128
// VGPRs, one row per CU.
template <int BLK, int NCHUNK, class P>
__global__ void __launch_bounds__(BLK, NCHUNK <= 7 ? 8 : 4)
k_ce_fwd_grad(const uint16_t* __restrict__ logits,
              const int32_t* __restrict__ targets, float* __restrict__ loss,
              float* __restrict__ row_lse, uint16_t* __restrict__ dlogits,
              int64_t V, P p) {
  __shared__ float ldsw[BLK / 64];
  const int64_t r = blockIdx.x;
  const uint16_t* xr = logits + r * V;
  uint16_t* dr = dlogits + r * V;
  const CeRow g = ce_row_split(xr, V);

  // The target is loaded where it costs no register: before the row loads
  // when the row has to be classified, after them otherwise.
  int tgt = 0;
  if constexpr (P::MASKED) {
    tgt = targets[r];
    // block-uniform (blockIdx and kernel arguments only), before any load
    const int kind = p.kind(tgt, V);
    if (kind != CE_ROW_VALID) {
      ce_zero_row<BLK>(dr, g, V);
      ce_invalid_row_stats(kind, r, loss, row_lse);
      return;
    }
  }

  const int nbody = static_cast<int>(g.nbody);  // <= BLK * NCHUNK (launcher)
  const uint4* xb = reinterpret_cast<const uint4*>(xr + g.head);

  // edge elements live in the last threads, which hold the fewest chunks
  const int e = BLK - 1 - static_cast<int>(threadIdx.x);
  const bool edge = e < g.head + g.tail;
  // EXTRA: V fits an int, and the narrower index is the register that
  // keeps the 7-chunk instantiation at 64 VGPRs without a spill (the others
  // fit with the 64-bit index and spill with this one)
  using edge_index_t = std::conditional_t<P::EXTRA, int, int64_t>;
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
  if constexpr (!P::MASKED) tgt = targets[r];
  const float inv_count = p.inv_count();

  float m = xe;
#pragma unroll
  for (int k = 0; k < NCHUNK; ++k)
    if (k * BLK + static_cast<int>(threadIdx.x) < nbody) m = fmaxf(m, ce_max8(v[k]));
  m = block_max<BLK>(m, ldsw);

  // EXTRA: one more block reduction, sum_j x_j; block-uniform results move
  // to scalar registers so the row keeps the vector ones
  float sx = 0.f;
  if constexpr (P::EXTRA) {
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
  if constexpr (P::EXTRA) lse = ce_uniform(lse);

  // EXTRA: lse and sx sit in scalar registers, so the longer loss formula
  // waits until the row's registers are free (after the stores)
  if constexpr (!P::EXTRA) {
    if (threadIdx.x == 0) {
      loss[r] = ce_row_loss(p, lse, bf16_to_f32(xr[tgt]), sx, V);
      row_lse[r] = lse;
    }
  }

  const CeGrad<P::EXTRA> cg = ce_make_grad(p, inv_count, lse, V);
  uint16_t* db = dr + g.head;
  const bool aligned = (reinterpret_cast<uintptr_t>(db) & 15) == 0;
#pragma unroll
  for (int k = 0; k < NCHUNK; ++k) {
    int c = k * BLK + static_cast<int>(threadIdx.x);
    if (c < nbody)
      ce_store8(db + 8 * c, cg.chunk(v[k], lse, tgt - g.head - 8 * c), aligned);
  }
  if (edge) dr[ei] = f32_to_bf16(cg.one(xe, lse, ei == tgt));
  if constexpr (P::EXTRA) {
    if (threadIdx.x == 0) {
      loss[r] = ce_row_loss(p, lse, bf16_to_f32(xr[tgt]), sx, V);
      row_lse[r] = lse;
    }
  }
}

// Grid-stride over rows.  SKIP_IF_UNIT: the buffer already holds the g == 1
// result from k_ce_fwd_grad, so every block returns when *gscale_dev is
// exactly 1 (decided on the device: no host sync) and otherwise recomputes
// the rows from logits and row_lse as usual — no double rounding.
template <int BLK, bool SKIP_IF_UNIT, class P>
__global__ void k_ce_bwd(const uint16_t* __restrict__ logits,
                         const int32_t* __restrict__ targets,
                         const float* __restrict__ row_lse,
                         uint16_t* __restrict__ dlogits,
                         const float* __restrict__ gscale_dev, int64_t R,
                         int64_t V, P p) {
  const float gup = *gscale_dev;  // upstream grad read on device: no host
                                  // sync in the backward pass
  if (SKIP_IF_UNIT && gup == 1.0f) return;
  const float gscale = gup * p.inv_count();
  for (int64_t r = blockIdx.x; r < R; r += gridDim.x) {
    const uint16_t* xr = logits + r * V;
    uint16_t* dr = dlogits + r * V;
    const float lse = row_lse[r];
    const int64_t tgt = targets[r];
    const CeRow g = ce_row_split(xr, V);
    if constexpr (P::MASKED) {
      if (p.kind(tgt, V) != CE_ROW_VALID) {
        ce_zero_row<BLK>(dr, g, V);
        continue;
      }
    }
    const CeGrad<P::EXTRA> cg = ce_make_grad(p, gscale, lse, V);
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

// --------------------------------------------------------------- launchers

// One launch helper per kernel; the public launchers below build the policy.

template <int BLK, class P>
static void launch_ce_fwd(const void* logits, const int32_t* targets,
                          float* loss, float* row_m, float* row_lse, int64_t R,
                          int64_t V, const P& p, hipStream_t s) {
  hipLaunchKernelGGL((k_ce_fwd<BLK, P>), dim3(static_cast<uint32_t>(R)),
                     dim3(BLK), 0, s, static_cast<const uint16_t*>(logits),
                     targets, loss, row_m, row_lse, V, p);
  HIP_CHECK(hipGetLastError());
}

// V <= CE_ROW_CAP16 (checked by the callers, each with its own message)
template <class P>
static void launch_ce_fwd_grad(const void* logits, const int32_t* targets,
                               float* loss, float* row_lse, void* dlogits,
                               int64_t R, int64_t V, const P& p,
                               hipStream_t s) {
  const int chunks = static_cast<int>((V + CE_ROW_BLOCK * 8 - 1) / (CE_ROW_BLOCK * 8));
  dispatch_cpt<7, 16>(chunks, [&](auto nchunk) {
    hipLaunchKernelGGL((k_ce_fwd_grad<CE_ROW_BLOCK, nchunk(), P>),
                       dim3(static_cast<uint32_t>(R)), dim3(CE_ROW_BLOCK), 0,
                       s, static_cast<const uint16_t*>(logits), targets, loss,
                       row_lse, static_cast<uint16_t*>(dlogits), V, p);
  });
  HIP_CHECK(hipGetLastError());
}

template <int BLK, class P>
static void launch_ce_bwd(const void* logits, const int32_t* targets,
                          const float* row_lse, void* dlogits,
                          const float* gscale_dev, int64_t R, int64_t V,
                          bool skip_if_unit, const P& p, hipStream_t s) {
  // skip_if_unit: a bounded grid (2048 threads fill each of the 256 CUs),
  // so the usual no-op costs one wave of blocks (6 us measured) instead of
  // R empty ones.  The full pass keeps one block per row: on the bounded
  // grid it measured 3.36 ms against 2.62 ms (R=65536, V=50257).
  const int64_t cap = skip_if_unit ? 256 * (2048 / BLK) : (int64_t(1) << 31) - 1;
  const dim3 grid(static_cast<uint32_t>(R < cap ? R : cap));
  dispatch_bool(skip_if_unit, [&](auto skip) {
    hipLaunchKernelGGL((k_ce_bwd<BLK, skip(), P>), grid, dim3(BLK), 0, s,
                       static_cast<const uint16_t*>(logits), targets, row_lse,
                       static_cast<uint16_t*>(dlogits), gscale_dev, R, V, p);
  });
  HIP_CHECK(hipGetLastError());
}

// block-size knob of the plain launchers (SHTENS_CE_BLOCK=512); measured
// r02: 512 is within noise of 256 (2.63 vs 2.66 ms fwd) — the kernel is
// bound by the re-read + exp throughput, not wave count — so 256 stays
// default
static bool ce_block_512() {
  const char* e = std::getenv("SHTENS_CE_BLOCK");
  return e && std::atoi(e) == 512;
}

void hip_ce_fwd(const void* logits, const int32_t* targets, float* loss,
                float* row_m, float* row_lse, int64_t R, int64_t V,
                hipStream_t s) {
  // NOTE (measured, profiles/r02): an LDS-staged single-read variant
  // (whole 100 KB row resident in the 160 KiB LDS) ran 4x SLOWER than this
  // two-pass kernel -- at 100 KB/block only one block fits per CU and four
  // waves cannot hide the global-load latency; the second pass's re-read
  // is cheaper than the lost occupancy.
  const CePlain p{0.f};  // the stats-only forward takes no mean
  if (ce_block_512())
    launch_ce_fwd<512>(logits, targets, loss, row_m, row_lse, R, V, p, s);
  else
    launch_ce_fwd<CE_BLOCK>(logits, targets, loss, row_m, row_lse, R, V, p, s);
}

// register capacity of the k_ce_fwd_grad instantiations
int64_t hip_ce_fwd_grad_max_v() { return CE_ROW_CAP16; }

void hip_ce_fwd_grad(const void* logits, const int32_t* targets, float* loss,
                     float* row_lse, void* dlogits, float inv_r, int64_t R,
                     int64_t V, hipStream_t s) {
  if (V < 1 || V > CE_ROW_CAP16)
    throw std::runtime_error("hip_ce_fwd_grad: V beyond the register capacity");
  launch_ce_fwd_grad(logits, targets, loss, row_lse, dlogits, R, V,
                     CePlain{inv_r}, s);
}

void hip_ce_bwd(const void* logits, const int32_t* targets,
                const float* row_lse, void* dlogits, const float* gscale_dev,
                float inv_r, int64_t R, int64_t V, bool skip_if_unit,
                hipStream_t s) {
  if (R <= 0) return;
  const CePlain p{inv_r};
  if (ce_block_512())
    launch_ce_bwd<512>(logits, targets, row_lse, dlogits, gscale_dev, R, V,
                       skip_if_unit, p, s);
  else
    launch_ce_bwd<CE_BLOCK>(logits, targets, row_lse, dlogits, gscale_dev, R,
                            V, skip_if_unit, p, s);
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

// f(policy) with the policy that the options ask for
template <typename F>
static void ce_with_policy(const CeOptState* state, const CeOpts& o, F&& f) {
  const CeMasked m{state, o.ignore_index, o.has_ignore ? 1 : 0};
  if (o.eps != 0.f || o.z != 0.f)
    f(CeMaskedExtra{m, o.eps, o.z});
  else
    f(m);
}

void hip_ce_opts_scan(const int32_t* targets, int64_t R, int64_t V,
                      const CeOpts& o, CeOptState* state, hipStream_t s) {
  ce_opts_check("hip_ce_opts_scan", o, R, V);
  // R*4 bytes (256 KB at R = 65536): one block striding over R is enough
  hipLaunchKernelGGL(k_ce_opts_scan<CE_ROW_BLOCK>, dim3(1), dim3(CE_ROW_BLOCK),
                     0, s, targets, R, V, o.ignore_index,
                     o.has_ignore ? 1 : 0, state);
  HIP_CHECK(hipGetLastError());
}

void hip_ce_opts_fwd_grad(const void* logits, const int32_t* targets,
                          float* loss, float* row_lse, void* dlogits,
                          const CeOptState* state, const CeOpts& o, int64_t R,
                          int64_t V, hipStream_t s) {
  ce_opts_check("hip_ce_opts_fwd_grad", o, R, V);
  if (V > CE_ROW_CAP16)
    throw std::runtime_error(
        "hip_ce_opts_fwd_grad: V beyond the register capacity");
  ce_with_policy(state, o, [&](const auto& p) {
    launch_ce_fwd_grad(logits, targets, loss, row_lse, dlogits, R, V, p, s);
  });
}

void hip_ce_opts_fwd(const void* logits, const int32_t* targets, float* loss,
                     float* row_lse, const CeOpts& o, int64_t R, int64_t V,
                     hipStream_t s) {
  ce_opts_check("hip_ce_opts_fwd", o, R, V);
  // no state: the stats-only forward takes no mean; no row_m: not saved
  ce_with_policy(nullptr, o, [&](const auto& p) {
    launch_ce_fwd<CE_BLOCK>(logits, targets, loss, nullptr, row_lse, R, V, p, s);
  });
}

void hip_ce_opts_bwd(const void* logits, const int32_t* targets,
                     const float* row_lse, void* dlogits,
                     const float* gscale_dev, const CeOptState* state,
                     const CeOpts& o, int64_t R, int64_t V, bool skip_if_unit,
                     hipStream_t s) {
  ce_opts_check("hip_ce_opts_bwd", o, R, V);
  ce_with_policy(state, o, [&](const auto& p) {
    launch_ce_bwd<CE_BLOCK>(logits, targets, row_lse, dlogits, gscale_dev, R,
                            V, skip_if_unit, p, s);
  });
}

}  // namespace shamd
