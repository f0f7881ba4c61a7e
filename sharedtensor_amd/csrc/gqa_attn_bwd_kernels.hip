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
//   HW heads.  The per-wave code is k_attn_bwd_dq's: Q and dO in registers,
//   K and V tiles double-buffered in LDS (2 x (8 + 8) KB, one barrier per
//   tile), half tiles of 32 keys, dS^T never leaves registers, delta written
//   to the workspace on the way.  Only the wave's q/out/dout/dq base, its
//   head index for lse and delta and kv_end = min(T, q0 + 128 / HW) differ.
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
//   * The tile body is k_attn_bwd_dkdv's.
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
// 154), k_gqa_bwd_dkdv_hd64 194 VGPRs and 76 SGPRs (k_attn_bwd_dkdv: 198 and
// 62: the per-head pointers went to scalar registers); no AGPRs, scratch or
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
    int G, int T, int nqb, BwdStrides sq, BwdStrides sk, BwdStrides sv,
    BwdStrides so, BwdStrides sdo, BwdStrides sdq, int64_t lse_stride,
    float scale) {
  constexpr int kWPH = kWaves / HW;  // waves per head
  constexpr int kPB = kRW * kWPH;    // positions per workgroup
  __shared__ __attribute__((aligned(16))) unsigned char lds[4 * kTileBytes];
  // K buffers at 0 and kTileBytes, V buffers behind them
  unsigned char* const ldsK = lds;
  unsigned char* const ldsV = lds + 2 * kTileBytes;

  const int nhalf = G / HW;
  int bk, slot;
  if (!grid_map(nbk, nqb * nhalf, bk, slot)) return;  // whole workgroup
  const int qb = nqb - 1 - slot / nhalf;              // heaviest block first
  const int half = slot % nhalf;
  const int b = bk / Hkv, kvh = bk % Hkv;

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int r = lane & 31, hi = lane >> 5;
  const LaneOffs lo = lane_offs(lane);

  const int Hq = Hkv * G;
  const int h = G * kvh + HW * half + wave / kWPH;  // the wave's query head
  const int64_t bh = (int64_t)b * Hq + h;
  const int q0 = qb * kPB;
  const int qw0 = q0 + (wave % kWPH) * kRW;  // the wave's first query row
  const int qrow = qw0 + r;                  // this lane's query row
  const bool qok = qrow < T;

  const uint16_t* qp = q + b * sq.b + h * sq.h + (int64_t)qrow * sq.t;
  const uint16_t* op = out + b * so.b + h * so.h + (int64_t)qrow * so.t;
  const uint16_t* dop = dout + b * sdo.b + h * sdo.h + (int64_t)qrow * sdo.t;
  const uint16_t* kp = k + b * sk.b + kvh * sk.h;
  const uint16_t* vp = v + b * sv.b + kvh * sv.h;

  // Q and dO fragments: B operands; lane holds X[qrow][16 ks + 8 hi + j].
  // delta from the same elements of dO and O.
  bf16x8 qf[4], dof[4];
  float dl = 0.f;
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    const int d0 = 16 * ks + 8 * hi;
    qf[ks] = __builtin_bit_cast(bf16x8, load16_or_zero(qp + d0, qok));
    dof[ks] = __builtin_bit_cast(bf16x8, load16_or_zero(dop + d0, qok));
    bf16x8 of = __builtin_bit_cast(bf16x8, load16_or_zero(op + d0, qok));
#pragma unroll
    for (int e = 0; e < 8; ++e)
      dl = __builtin_fmaf((float)dof[ks][e], (float)of[e], dl);
  }
  dl += other_half(dl, lane);
  if (hi == 0 && qok) delta[bh * T + qrow] = dl;
  // -lse * log2(e); rows past T: any finite value, their dS is 0 * finite
  const float nl = qok ? -lse[bh * lse_stride + qrow] * kLog2e : 0.f;
  const float scale_log2e = scale * kLog2e;

  // staging: thread covers 16-byte chunk (tid & 7) of keys (tid >> 3) and
  // (tid >> 3) + 32 of the tile, for K and for V
  const int skey = tid >> 3, sch = tid & 7;
  u32x4 stK[2], stV[2];
  auto issue = [&](int kv0) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      int key = kv0 + skey + 32 * i;
      bool ok = key < T;
      stK[i] = load16_or_zero(kp + (int64_t)key * sk.t + 8 * sch, ok);
      stV[i] = load16_or_zero(vp + (int64_t)key * sv.t + 8 * sch, ok);
    }
  };
  auto commit = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      int off = buf * kTileBytes + t_off(skey + 32 * i, sch);
      *reinterpret_cast<u32x4*>(ldsK + off) = stK[i];
      *reinterpret_cast<u32x4*>(ldsV + off) = stV[i];
    }
  };

  const int kv_end = min(T, q0 + kPB);              // keys this block can see
  const int ntiles = (kv_end + kTile - 1) / kTile;  // >= 1

  f32x16 acc[2];  // dQ^T: lane holds dQ[qrow][32 nb + (reg&3) + 8 (reg>>2) + 4 hi]
#pragma unroll
  for (int nb = 0; nb < 2; ++nb)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[nb][i] = 0.f;

  issue(0);
  commit(0);
  __syncthreads();

  for (int t = 0; t < ntiles; ++t) {
    const int cur = t & 1;
    const int kv0 = t * kTile;
    const bool more = t + 1 < ntiles;
    if (more) issue(kv0 + kTile);

    const unsigned char* Kt = ldsK + cur * kTileBytes;
    const unsigned char* Vt = ldsV + cur * kTileBytes;
    // keys of the tile are kv0 + 4 hi + c, c a register constant; key c is
    // visible when c <= vis.  Tiles below the diagonal: everything.
    const int vis = kv0 + kTile - 1 > qw0 ? qrow - kv0 - 4 * hi : kTile;

#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      // wave-uniform: the half tile has keys the wave's rows can see
      if (kv0 + 32 * kb > qw0 + kRW - 1) continue;

      // S^T = K Q^T and dP^T = V dO^T for keys kv0 + 32 kb + keymap(reg, hi)
      f32x16 s, dp;
#pragma unroll
      for (int i = 0; i < 16; ++i) s[i] = dp[i] = 0.f;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag(Kt, lo, kb, ks),
                                                    qf[ks], s, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag(Vt, lo, kb, ks),
                                                     dof[ks], dp, 0, 0, 0);
      }

      bf16x8 dsf[2];  // dS^T fragments: k-steps 2 kb and 2 kb + 1
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        float p = __builtin_amdgcn_exp2f(
            __builtin_fmaf(s[i], scale_log2e, nl));
        if (32 * kb + (i & 3) + 8 * (i >> 2) > vis) p = 0.f;
        dsf[i >> 3][i & 7] = (__bf16)(p * (dp[i] - dl));
      }

      // dQ^T += K^T dS^T
#pragma unroll
      for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2)
          acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              tr_frag(Kt, lo, 2 * kb + h2, nb), dsf[h2], acc[nb], 0, 0, 0);
    }

    if (more) commit(cur ^ 1);
    __syncthreads();
  }

  // the loop's last barrier is behind every wave: the tiles are dead
  unsigned char* const Ow = lds + wave * (kRW * 128);
  stage_rows(Ow, acc, scale, r, hi);
  __syncthreads();
  store_rows(Ow, dq + b * sdq.b + h * sdq.h, sdq.t, qw0, T, lane);
}

// ------------------------------------------------------------- dK, dV

// nbk = B * Hkv, nkb = key blocks of 128 keys
__global__ __launch_bounds__(256)
    __attribute__((amdgpu_waves_per_eu(2, 2))) void k_gqa_bwd_dkdv_hd64(
    const uint16_t* __restrict__ q, const uint16_t* __restrict__ k,
    const uint16_t* __restrict__ v, const uint16_t* __restrict__ dout,
    const float* __restrict__ lse, const float* __restrict__ delta,
    uint16_t* __restrict__ dk, uint16_t* __restrict__ dv, int nbk, int Hkv,
    int G, int T, int nkb, BwdStrides sq, BwdStrides sk, BwdStrides sv,
    BwdStrides sdo, BwdStrides sdk, BwdStrides sdv, int64_t lse_stride,
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

      // S = Q K^T and dP = dO V^T for queries qt0 + 32 qh + rowmap(reg, hi)
      f32x16 s, dp;
#pragma unroll
      for (int i = 0; i < 16; ++i) s[i] = dp[i] = 0.f;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag(Qt, lo, qh, ks),
                                                    kf[ks], s, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag(Dt, lo, qh, ks),
                                                     vf[ks], dp, 0, 0, 0);
      }

      bf16x8 pf[2], dsf[2];  // P and dS fragments: k-steps 2 qh and 2 qh + 1
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        // registers 4 g4 .. 4 g4 + 3 are queries 32 qh + 8 g4 + 4 hi + 0..3
        const int c0 = 32 * qh + 8 * g4;
        f32x4 nl4 = *reinterpret_cast<const f32x4*>(LD + c0 + 4 * hi);
        f32x4 dl4 = *reinterpret_cast<const f32x4*>(LD + kTile + c0 + 4 * hi);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int i = 4 * g4 + e;
          float p = __builtin_amdgcn_exp2f(
              __builtin_fmaf(s[i], scale_log2e, nl4[e]));
          if (c0 + e < need) p = 0.f;
          pf[i >> 3][i & 7] = (__bf16)p;
          dsf[i >> 3][i & 7] = (__bf16)(p * (dp[i] - dl4[e]));
        }
      }

      // dV^T += dO^T P, dK^T += Q^T dS
#pragma unroll
      for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2) {
          dva[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              tr_frag(Dt, lo, 2 * qh + h2, nb), pf[h2], dva[nb], 0, 0, 0);
          dka[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              tr_frag(Qt, lo, 2 * qh + h2, nb), dsf[h2], dka[nb], 0, 0, 0);
        }
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

// no two rows of a (B, T, H, 64) output may overlap: with the dimensions of
// more than one element ordered by stride, the smallest stride covers a
// 64-element row and every further one the whole extent of the dimension
// before it
bool rows_disjoint(const int64_t* st, int64_t B, int64_t T, int64_t H) {
  const int64_t dims[3] = {B, T, H};
  int64_t sd[3][2];
  int n = 0;
  for (int i = 0; i < 3; ++i)
    if (dims[i] > 1) {
      int j = n++;
      for (; j > 0 && sd[j - 1][0] > st[i]; --j) {
        sd[j][0] = sd[j - 1][0];
        sd[j][1] = sd[j - 1][1];
      }
      sd[j][0] = st[i];
      sd[j][1] = dims[i];
    }
  int64_t need = kD;
  for (int i = 0; i < n; ++i) {
    if (sd[i][0] < need) return false;
    need = sd[i][0] * sd[i][1];
  }
  return true;
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
  if (B <= 0 || Hq <= 0 || Hkv <= 0 || T <= 0)
    throw std::runtime_error(std::string(op) + ": empty problem");
  if (Hq % Hkv)
    throw std::runtime_error(std::string(op) +
                             ": Hq must be a multiple of Hkv");
  const int64_t G = Hq / Hkv;
  if (G != 2 && G != 4 && G != 8)
    throw std::runtime_error(std::string(op) + ": group size must be 2, 4 or 8");
  if (!(scale > 0.f) || scale > 3.0e38f)
    throw std::runtime_error(std::string(op) + ": scale must be positive");
  if (lse_stride < T)
    throw std::runtime_error(std::string(op) + ": lse row shorter than T");
  const void* ptrs[] = {q, k, v, out, dout, dq, dk, dv};
  const char* names[] = {"q", "k", "v", "out", "dout", "dq", "dk", "dv"};
  for (int i = 0; i < 8; ++i) {
    if (!ptrs[i])
      throw std::runtime_error(std::string(op) + ": " + names[i] + " is null");
    check_align(ptrs[i], 16, op, names[i]);
  }
  if (!lse || !delta)
    throw std::runtime_error(std::string(op) + ": lse or delta is null");
  check_align(lse, 4, op, "lse");
  check_align(delta, 4, op, "delta");
  for (const int64_t* st : {qs, ks, vs, os, dos, dqs, dks, dvs})
    for (int i = 0; i < 3; ++i)
      if (st[i] < 0 || st[i] % 8)
        throw std::runtime_error(std::string(op) +
                                 ": strides must be multiples of 8 elements");
  if (!rows_disjoint(dqs, B, T, Hq) || !rows_disjoint(dks, B, T, Hkv) ||
      !rows_disjoint(dvs, B, T, Hkv))
    throw std::runtime_error(std::string(op) + ": output rows would overlap");
  const int HW = G < 4 ? 2 : 4;
  const int64_t pb = kRB / HW;
  const int64_t nqb = (T + pb - 1) / pb;
  const int64_t nkb = (T + kRB - 1) / kRB;
  const int64_t nbk = B * Hkv;
  const int64_t nbk8 = (nbk + kXcd - 1) / kXcd * kXcd;
  const int64_t grid_dq = nbk8 * nqb * (G / HW);
  const int64_t grid_kv = nbk8 * nkb;
  if (grid_dq > 0x7fffffff || T > (1 << 30) || B * Hq > 0x7fffffff)
    throw std::runtime_error(std::string(op) + ": problem too large");
  auto st3 = [](const int64_t* p) { return BwdStrides{p[0], p[1], p[2]}; };
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
