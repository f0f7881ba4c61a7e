// Causal bf16 grouped-query attention backward for head dim 64 (Llama), the
// counterpart of gqa_attn_kernels.hip: Hq = G Hkv query heads, query head h
// reads kv head h / G, G in {2, 4, 8}.  fp32 accumulation, bf16 in and out,
// no dropout, no bias, top-left aligned causal mask (Tq == Tk).  Two kernels,
// no atomics, one fp32 workspace delta (B, Hq, T); every output element is
// written once by one lane from one fixed-order sum, so repeats are
// bit-identical.  dK and dV of a kv head are sums over its G query heads;
// they are summed in the fp32 accumulators of one workgroup and rounded to
// bf16 once (the library path expands K/V, rounds G gradients to bf16 and
// adds those).
//
// The math, the tile swizzle and the lane layouts are those of
// attn_bwd_kernels.hip (see its header); the helpers are shared through
// attn_bwd_tile.h.  This file is built with the same EXTRA_FLAGS entry in
// build.py, so the per-score dS arithmetic compiles as it does there.
//
// Plan (tests/test_gqa_attn_resource_usage.py holds the kernels to it):
//
//   k_gqa_bwd_dq_hd64<HW>: a wave is a query head, the mapping of the
//   forward: workgroup = 4 waves = HW heads of one kv group x 128 / HW
//   consecutive query positions, HW = min(G, 4); G = 8 takes two workgroups
//   (head halves) per kv head and position block.  One staged K/V tile feeds
//   HW heads.  The kernel is attn_bwd_dq_body<HW> (attn_bwd_tile.h), which
//   k_attn_bwd_dq runs with HW = 1, G = 1, followed by the plain store.
//   * Grid: the forward's (all workgroups of one (b, kv head) consecutive on
//     one XCD, heaviest (last) position block first, head halves adjacent).
//   * Resources: amdgpu_waves_per_eu(3, 3): at most 168 VGPRs, no AGPRs, no
//     scratch, no spills, 32 KB of LDS -> 3 waves/SIMD, k_attn_bwd_dq's line
//     (which misses 4 waves/SIMD for the reason given there).
//
//   k_gqa_bwd_dkdv_hd64: workgroup = 4 waves = 128 keys of one (b, kv head),
//   a lane owns one key.  K and V fragments and the 64 fp32 accumulators of
//   dK^T and dV^T stay in registers across the whole group.
//   * One flattened loop over (g, query tile), g = 0 .. G-1, 64-query tiles
//     from the diagonal tile to the end.  Q, dO, -lse log2(e) and delta
//     tiles of head G kvh + g are double-buffered in LDS, 2 x (8 KB + 8 KB +
//     512 B) = 33 KB.  The `issue` of the next iteration crosses the head
//     boundary, so the pipeline never drains between heads; the buffer
//     parity follows the flattened index, not the tile index (an odd tile
//     count flips it at every head boundary).  The per-head pointers are
//     wave-uniform scalar arithmetic.
//   * The half-tile arithmetic is k_attn_bwd_dkdv's (dkdv_half_tile).
//   * dK is scaled and dK, dV rounded once in the epilogue, and staged
//     through LDS to whole-row stores.
//   * Grid: one workgroup per (b, kv head, key block), the key blocks of one
//     (b, kv head) consecutive on one XCD, first (heaviest) key block first.
//     A workgroup runs G times longer than k_attn_bwd_dkdv's and there are G
//     times fewer of them.  At B=8, Hkv=8, T=2048 (1024 workgroups, the
//     heaviest as long as 94% of the ideal makespan) the backward is 0.07 ms
//     behind the MHA kernels on expanded K/V before the expansion is
//     charged, and ahead at B=64 (profiles/r12/).  Ordering all
//     (b, kv head) by key block globally heaviest-first was not tried.
//   * Resources: amdgpu_waves_per_eu(2, 2): at most 256 VGPRs, no AGPRs, no
//     scratch, no spills, 33 KB of LDS -> 2 waves/SIMD, k_attn_bwd_dkdv's
//     line.
//
// As built: k_gqa_bwd_dq_hd64<2> and <4> 154 VGPRs each (k_attn_bwd_dq:
// 156), k_gqa_bwd_dkdv_hd64 194 VGPRs and 76 SGPRs (k_attn_bwd_dkdv: 198 and
// 68: the per-head pointers went to scalar registers); no AGPRs, scratch or
// spills.  No deviation from the plan.
//
// Every T is bounds-checked: rows at or past T are read as zeros (never from
// memory) and never stored.
#include <hip/hip_runtime.h>

#include "attn_bwd_tile.h"
#include "device_util.h"
#include "hip_api.h"

namespace shamd {
namespace {

// ------------------------------------------------------------------ dQ

// nbk = B * Hkv, nqb = position blocks of 128 / HW rows, nhalf = G / HW
template <int HW>
__global__ __launch_bounds__(256)
    __attribute__((amdgpu_waves_per_eu(3, 3))) void k_gqa_bwd_dq_hd64(
    const uint16_t* __restrict__ q, const uint16_t* __restrict__ k,
    const uint16_t* __restrict__ v, const uint16_t* __restrict__ out,
    const uint16_t* __restrict__ dout, const float* __restrict__ lse,
    uint16_t* __restrict__ dq, float* __restrict__ delta, int nbk, int Hkv,
    int G, int T, int nqb, AttnStrides sq, AttnStrides sk, AttnStrides sv,
    AttnStrides so, AttnStrides sdo, AttnStrides sdq, int64_t lse_stride,
    float scale) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[4 * kTileBytes];
  int bk, slot;
  if (!grid_map(nbk, nqb * (G / HW), bk, slot)) return;  // whole workgroup
  const DqRows w = attn_bwd_dq_body<HW>(lds, bk, slot, q, k, v, out, dout, lse,
                                        delta, Hkv, G, T, nqb, sq, sk, sv, so,
                                        sdo, lse_stride, scale);
  store_rows(w.Ow, dq + w.b * sdq.b + w.h * sdq.h, sdq.t, w.qw0, T,
             threadIdx.x & 63);
}

// ------------------------------------------------------------- dK, dV

// nbk = B * Hkv, nkb = key blocks of 128 keys
__global__ __launch_bounds__(256)
    __attribute__((amdgpu_waves_per_eu(2, 2))) void k_gqa_bwd_dkdv_hd64(
    const uint16_t* __restrict__ q, const uint16_t* __restrict__ k,
    const uint16_t* __restrict__ v, const uint16_t* __restrict__ dout,
    const float* __restrict__ lse, const float* __restrict__ delta,
    uint16_t* __restrict__ dk, uint16_t* __restrict__ dv, int nbk, int Hkv,
    int G, int T, int nkb, AttnStrides sq, AttnStrides sk, AttnStrides sv,
    AttnStrides sdo, AttnStrides sdk, AttnStrides sdv, int64_t lse_stride,
    float scale) {
  __shared__ __attribute__((aligned(16))) unsigned char
      lds[4 * kTileBytes + 2 * 2 * kTile * 4];
  // Q buffers at 0 and kTileBytes, dO buffers behind them, then per buffer
  // 64 floats of -lse log2(e) and 64 of delta
  unsigned char* const ldsQ = lds;
  unsigned char* const ldsD = lds + 2 * kTileBytes;
  float* const ldsLD = reinterpret_cast<float*>(lds + 4 * kTileBytes);

  int bk, kblk;
  if (!grid_map(nbk, nkb, bk, kblk)) return;  // whole workgroup
  const int b = bk / Hkv, kvh = bk % Hkv;     // first key block first

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int r = lane & 31, hi = lane >> 5;
  const LaneOffs lo = lane_offs(lane);

  const int k0 = kblk * kRB;
  const int kw0 = k0 + wave * kRW;  // the wave's first key
  const int krow = kw0 + r;         // this lane's key
  const bool kok = krow < T;

  const uint16_t* kp = k + b * sk.b + kvh * sk.h + (int64_t)krow * sk.t;
  const uint16_t* vp = v + b * sv.b + kvh * sv.h + (int64_t)krow * sv.t;
  // head G kvh of the group; head g of it is g strides further
  const int h0 = G * kvh;
  const int64_t bh0 = (int64_t)b * Hkv * G + h0;
  const uint16_t* const qp0 = q + b * sq.b + h0 * sq.h;
  const uint16_t* const dop0 = dout + b * sdo.b + h0 * sdo.h;
  const float* const lsep0 = lse + bh0 * lse_stride;
  const float* const deltap0 = delta + bh0 * T;

  // K and V fragments: B operands; lane holds X[krow][16 ks + 8 hi + j]
  bf16x8 kf[4], vf[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    const int d0 = 16 * ks + 8 * hi;
    kf[ks] = __builtin_bit_cast(bf16x8, load16_or_zero(kp + d0, kok));
    vf[ks] = __builtin_bit_cast(bf16x8, load16_or_zero(vp + d0, kok));
  }
  const float scale_log2e = scale * kLog2e;

  // staging: thread covers 16-byte chunk (tid & 7) of queries (tid >> 3) and
  // (tid >> 3) + 32 of the tile, for Q and for dO; threads 0..63 one lse,
  // threads 64..127 one delta.  g (the head inside the group) is
  // wave-uniform.
  const int srow = tid >> 3, sch = tid & 7;
  u32x4 stQ[2], stD[2];
  float stL = 0.f;
  auto issue = [&](int g, int qt0) {
    const uint16_t* qp = qp0 + g * sq.h;
    const uint16_t* dop = dop0 + g * sdo.h;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      int row = qt0 + srow + 32 * i;
      bool ok = row < T;
      stQ[i] = load16_or_zero(qp + (int64_t)row * sq.t + 8 * sch, ok);
      stD[i] = load16_or_zero(dop + (int64_t)row * sdo.t + 8 * sch, ok);
    }
    if (tid < 2 * kTile) {
      int row = qt0 + (tid & (kTile - 1));
      stL = 0.f;
      if (row < T)
        stL = tid < kTile ? -lsep0[g * lse_stride + row] * kLog2e
                          : deltap0[(int64_t)g * T + row];
    }
  };
  auto commit = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      int off = buf * kTileBytes + t_off(srow + 32 * i, sch);
      *reinterpret_cast<u32x4*>(ldsQ + off) = stQ[i];
      *reinterpret_cast<u32x4*>(ldsD + off) = stD[i];
    }
    if (tid < 2 * kTile) ldsLD[buf * 2 * kTile + tid] = stL;
  };

  const int t_begin = k0 / kTile;               // the tile of the block's keys
  const int t_end = (T + kTile - 1) / kTile;    // > t_begin: k0 < T
  const int n_it = G * (t_end - t_begin);       // flattened (g, tile) count

  // dK^T, dV^T: lane holds dX[krow][32 nb + (reg&3) + 8 (reg>>2) + 4 hi],
  // summed over the whole group
  f32x16 dka[2], dva[2];
#pragma unroll
  for (int nb = 0; nb < 2; ++nb)
#pragma unroll
    for (int i = 0; i < 16; ++i) dka[nb][i] = dva[nb][i] = 0.f;

  issue(0, t_begin * kTile);
  commit(0);
  __syncthreads();

  // (g, t) of the iteration whose tile is being issued: one ahead of `it`
  int gn = 0, tn = t_begin;
  for (int it = 0; it < n_it; ++it) {
    const int cur = it & 1;        // parity of the flattened index
    const int qt0 = tn * kTile;    // the current tile's first query
    const bool more = it + 1 < n_it;
    if (++tn == t_end) {           // next iteration: next tile or next head
      tn = t_begin;
      ++gn;
    }
    if (more) issue(gn, tn * kTile);

    const unsigned char* Qt = ldsQ + cur * kTileBytes;
    const unsigned char* Dt = ldsD + cur * kTileBytes;
    const float* LD = ldsLD + cur * 2 * kTile;
    // queries of the tile are qt0 + 4 hi + c, c a register constant; query c
    // sees the lane's key when c >= need.  Tiles past the diagonal: all do.
    const int need = qt0 < kw0 + kRW - 1 ? krow - qt0 - 4 * hi : 0;

#pragma unroll
    for (int qh = 0; qh < 2; ++qh) {
      // wave-uniform: the half tile has queries that see the wave's keys
      if (qt0 + 32 * qh + 31 < kw0) continue;
      dkdv_half_tile(Qt, Dt, LD, lo, qh, hi, need, scale_log2e, kf, vf, dka,
                     dva);
    }

    if (more) commit(cur ^ 1);
    __syncthreads();
  }

  // the loop's last barrier is behind every wave: the tiles are dead; a wave
  // owns 8 KB, dK rows in the first 4 KB and dV rows in the second
  unsigned char* const Ow = lds + wave * (2 * kRW * 128);
  stage_rows(Ow, dka, scale, r, hi);
  stage_rows(Ow + kRW * 128, dva, 1.f, r, hi);
  __syncthreads();
  store_rows(Ow, dk + b * sdk.b + kvh * sdk.h, sdk.t, kw0, T, lane);
  store_rows(Ow + kRW * 128, dv + b * sdv.b + kvh * sdv.h, sdv.t, kw0, T, lane);
}

}  // namespace

void hip_gqa_attn_bwd_causal_hd64(
    const void* q, const void* k, const void* v, const void* out,
    const void* dout, const float* lse, void* dq, void* dk, void* dv,
    float* delta, int64_t B, int64_t Hq, int64_t Hkv, int64_t T,
    const int64_t* qs, const int64_t* ks, const int64_t* vs,
    const int64_t* os, const int64_t* dos, const int64_t* dqs,
    const int64_t* dks, const int64_t* dvs, int64_t lse_stride, float scale,
    hipStream_t s) {
  const char* op = "gqa_attn_bwd_causal_hd64";
  const int64_t G = check_attn_bwd(op, q, k, v, out, dout, lse, dq, dk, dv,
                                   delta, B, Hq, Hkv, T, qs, ks, vs, os, dos,
                                   dqs, dks, dvs, lse_stride, scale,
                                   /*grouped=*/true);
  const int HW = G < 4 ? 2 : 4;
  const int64_t pb = kRB / HW;
  const int64_t nqb = (T + pb - 1) / pb;
  const int64_t nkb = (T + kRB - 1) / kRB;
  const int64_t nbk = B * Hkv;
  const int64_t grid_dq = attn_grid(op, B, Hq, Hkv, T, nqb * (G / HW));
  const int64_t grid_kv = attn_grid(op, B, Hq, Hkv, T, nkb);
  auto st3 = strides3;
  auto u16 = [](const void* p) { return static_cast<const uint16_t*>(p); };
  auto launch_dq = [&](auto kern) {
    kern<<<dim3((unsigned)grid_dq), dim3(256), 0, s>>>(
        u16(q), u16(k), u16(v), u16(out), u16(dout), lse,
        static_cast<uint16_t*>(dq), delta, (int)nbk, (int)Hkv, (int)G, (int)T,
        (int)nqb, st3(qs), st3(ks), st3(vs), st3(os), st3(dos), st3(dqs),
        lse_stride, scale);
  };
  if (HW == 2)
    launch_dq(k_gqa_bwd_dq_hd64<2>);
  else
    launch_dq(k_gqa_bwd_dq_hd64<4>);
  HIP_CHECK(hipGetLastError());
  k_gqa_bwd_dkdv_hd64<<<dim3((unsigned)grid_kv), dim3(256), 0, s>>>(
      u16(q), u16(k), u16(v), u16(dout), lse, delta,
      static_cast<uint16_t*>(dk), static_cast<uint16_t*>(dv), (int)nbk,
      (int)Hkv, (int)G, (int)T, (int)nkb, st3(qs), st3(ks), st3(vs), st3(dos),
      st3(dks), st3(dvs), lse_stride, scale);
  HIP_CHECK(hipGetLastError());
}

}  // namespace shamd
