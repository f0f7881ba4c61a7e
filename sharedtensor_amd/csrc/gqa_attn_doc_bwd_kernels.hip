// Document-masked causal bf16 grouped-query attention backward for head dim
// 64 (packed Llama batches), the counterpart of gqa_attn_doc_kernels.hip and
// the gqa_attn_bwd_kernels.hip kernels with one more mask.  Query i sees key j
// when doc_start[b, i] <= j <= i; seen from the key, when
// j <= i < doc_end[b, j].  doc_start and doc_end are (B, T) int32, both
// non-decreasing in t.  Two kernels, no atomics, one fp32 workspace delta
// (B, Hq, T); every output element is written once by one lane from one
// fixed-order sum, so repeats are bit-identical.  dK and dV of a kv head are
// summed over its G query heads in the fp32 accumulators of one workgroup and
// rounded to bf16 once.
//
// The math, the tile swizzle, the lane layouts and the helpers are those of
// attn_bwd_tile.h; the loops are written anew here, so that the plain kernels
// compile as they did.  Built with the NO_PACKED_FP32 entry of
// build.EXTRA_FLAGS like the other backward files: the per-score dS
// arithmetic is theirs.
//
// Plan (tests/test_gqa_attn_doc_resource_usage.py holds the kernels to it):
//
//   k_gqa_bwd_dq_doc_hd64<HW>: the mapping of the forward, a wave is a query
//   head with 32 rows, workgroup = HW heads x 128 / HW positions.
//   * The workgroup stages KV tiles from doc_start[its first row] / 64; a
//     wave skips the 32-key half tiles that end before doc_start[its first
//     row], as it skips those above its rows.  Both are uniform loads.
//   * A tile takes the lower mask only if kv0 < doc_start[last row of the
//     wave], the diagonal mask only if it crosses the diagonal: as bounds
//     `lo <= c <= vis` on the register's key constant c, set per tile from
//     wave-uniform tests, so interior tiles compare against bounds that never
//     bite.  The lane's doc_start is loaded once, before the loop.
//   * P = exp2(s - lse) takes the row's lse over its own document.  Scores
//     are finite here (masking selects p = 0, it does not add -inf), so a
//     row that sees nothing of a tile has p = 0 and dS = 0 without a NaN.
//   * Resources: amdgpu_waves_per_eu(3, 3): at most 168 VGPRs, no AGPRs, no
//     scratch, no spills, 32 KB of LDS -> 3 waves/SIMD, k_gqa_bwd_dq_hd64's
//     line.
//
//   k_gqa_bwd_dkdv_doc_hd64: workgroup = 4 waves = 128 keys of one
//   (b, kv head), a lane owns one key; one flattened loop over (g, query
//   tile) as in k_gqa_bwd_dkdv_hd64.
//   * The last query tile is the one that holds doc_end[last key of the
//     block] - 1, not the end of the sequence: a uniform load.
//   * A wave skips the 32-query half tiles that begin at or past
//     doc_end[its last key], as it skips those before its keys.
//   * Query c of a tile sees the lane's key when need <= c < lim; lim bites
//     only in tiles that reach doc_end[the wave's first key], the smallest of
//     the wave, a wave-uniform test.  The lane's doc_end is loaded once.
//   * Grid: the positional order of k_gqa_bwd_dkdv_hd64, first key block
//     first.  Under document masks the work of a block is
//     doc_end[its last key] - its first key, not T - its first key, so the
//     order is heaviest-first only inside a document; ordering by that
//     length in the launcher needs the lengths on the host and was not
//     tried.
//   * Resources: amdgpu_waves_per_eu(2, 2): at most 256 VGPRs, no AGPRs, no
//     scratch, no spills, 33 KB of LDS -> 2 waves/SIMD.
//
// doc_start and doc_end steer loop bounds, so the uniform values that do are
// clamped to [0, row] and [key + 1, T]: wrong arrays give wrong numbers, never
// an address outside the operands.  Every T is bounds-checked: rows at or
// past T are read as zeros (never from memory) and never stored.
#include <hip/hip_runtime.h>

#include "attn_bwd_tile.h"
#include "device_util.h"
#include "hip_api.h"

namespace shamd {
namespace {

constexpr int kNever = 1 << 30;  // a bound no register constant reaches

// ------------------------------------------------------------------ dQ

// nbk = B * Hkv, nqb = position blocks of 128 / HW rows
template <int HW>
__global__ __launch_bounds__(256)
    __attribute__((amdgpu_waves_per_eu(3, 3))) void k_gqa_bwd_dq_doc_hd64(
    const uint16_t* __restrict__ q, const uint16_t* __restrict__ k,
    const uint16_t* __restrict__ v, const uint16_t* __restrict__ out,
    const uint16_t* __restrict__ dout, const float* __restrict__ lse,
    const int* __restrict__ doc_start, uint16_t* __restrict__ dq,
    float* __restrict__ delta, int nbk, int Hkv, int G, int T, int nqb,
    AttnStrides sq, AttnStrides sk, AttnStrides sv, AttnStrides so,
    AttnStrides sdo, AttnStrides sdq, int64_t lse_stride, float scale) {
  constexpr int kWPH = kWaves / HW;  // waves per head
  constexpr int kPB = kRW * kWPH;    // positions per workgroup
  __shared__ __attribute__((aligned(16))) unsigned char lds[4 * kTileBytes];
  // K buffers at 0 and kTileBytes, V buffers behind them
  unsigned char* const ldsK = lds;
  unsigned char* const ldsV = lds + 2 * kTileBytes;

  const int nhalf = G / HW;
  int bk, slot;
  if (!grid_map(nbk, nqb * nhalf, bk, slot)) return;  // whole workgroup
  const int qb = nqb - 1 - slot / nhalf;  // last block first
  const int half = slot % nhalf;
  const int b = bk / Hkv, kvh = bk % Hkv;

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int r = lane & 31, hi = lane >> 5;
  const LaneOffs lo = lane_offs(lane);

  const int Hq = Hkv * G;
  const int h = G * kvh + HW * half + wave / kWPH;  // the wave's query head
  const int64_t bh = (int64_t)b * Hq + h;
  const int q0 = qb * kPB;                   // < T
  const int qw0 = q0 + (wave % kWPH) * kRW;  // the wave's first query row
  const int qrow = qw0 + r;                  // this lane's query row
  const bool qok = qrow < T;

  const uint16_t* qp = q + b * sq.b + h * sq.h + (int64_t)qrow * sq.t;
  const uint16_t* op = out + b * so.b + h * so.h + (int64_t)qrow * so.t;
  const uint16_t* dop = dout + b * sdo.b + h * sdo.h + (int64_t)qrow * sdo.t;
  const uint16_t* kp = k + b * sk.b + kvh * sk.h;
  const uint16_t* vp = v + b * sv.b + kvh * sv.h;

  // document starts: of the workgroup's first row, of the wave's first and
  // last rows (uniform) and of the lane's row.  Rows at or past T take the
  // values of row T - 1 (uniform) or 0 (lane: their dS is 0 anyway).
  const int* dsp = doc_start + (int64_t)b * T;
  const int ds_wg = min(max(dsp[q0], 0), q0);
  const int rw0 = min(qw0, T - 1), rw1 = min(qw0 + kRW - 1, T - 1);
  const int ds_first = dsp[rw0];
  const int ds_last = dsp[rw1];
  const int ds_row = qok ? dsp[qrow] : 0;

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
  const int t_begin = ds_wg / kTile;                // <= q0 / kTile < ntiles

  f32x16 acc[2];  // dQ^T: lane holds dQ[qrow][32 nb + (reg&3) + 8 (reg>>2) + 4 hi]
#pragma unroll
  for (int nb = 0; nb < 2; ++nb)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[nb][i] = 0.f;

  issue(t_begin * kTile);
  commit(t_begin & 1);
  __syncthreads();

  for (int t = t_begin; t < ntiles; ++t) {
    const int cur = t & 1;
    const int kv0 = t * kTile;
    const bool more = t + 1 < ntiles;
    if (more) issue(kv0 + kTile);

    const unsigned char* Kt = ldsK + cur * kTileBytes;
    const unsigned char* Vt = ldsV + cur * kTileBytes;
    // keys of the tile are kv0 + 4 hi + c, c a register constant; key c is
    // visible when low <= c <= vis.  Tiles below the diagonal and tiles
    // inside the document of the wave's last row: a bound that never bites.
    const int vis = kv0 + kTile - 1 > qw0 ? qrow - kv0 - 4 * hi : kTile;
    const int low = kv0 < ds_last ? ds_row - kv0 - 4 * hi : -kNever;

#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      // wave-uniform: the half tile has keys the wave's rows can see
      if (kv0 + 32 * kb > qw0 + kRW - 1 || kv0 + 32 * kb + 31 < ds_first)
        continue;

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
        const int c = 32 * kb + (i & 3) + 8 * (i >> 2);
        float p = __builtin_amdgcn_exp2f(
            __builtin_fmaf(s[i], scale_log2e, nl));
        if (c > vis || c < low) p = 0.f;
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

// dkdv_half_tile (attn_bwd_tile.h) with an upper bound: query c of the tile
// sees the lane's key when need <= c < lim.
__device__ __forceinline__ void dkdv_doc_half_tile(
    const unsigned char* Qt, const unsigned char* Dt, const float* LD,
    const LaneOffs& lo, int qh, int hi, int need, int lim, float scale_log2e,
    const bf16x8 (&kf)[4], const bf16x8 (&vf)[4], f32x16 (&dka)[2],
    f32x16 (&dva)[2]) {
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
  for (int g = 0; g < 4; ++g) {
    // registers 4 g .. 4 g + 3 are queries 32 qh + 8 g + 4 hi + 0..3
    const int c0 = 32 * qh + 8 * g;
    f32x4 nl4 = *reinterpret_cast<const f32x4*>(LD + c0 + 4 * hi);
    f32x4 dl4 = *reinterpret_cast<const f32x4*>(LD + kTile + c0 + 4 * hi);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int i = 4 * g + e;
      float p = __builtin_amdgcn_exp2f(
          __builtin_fmaf(s[i], scale_log2e, nl4[e]));
      if (c0 + e < need || c0 + e >= lim) p = 0.f;
      pf[i >> 3][i & 7] = (__bf16)p;
      dsf[i >> 3][i & 7] = (__bf16)(p * (dp[i] - dl4[e]));
    }
  }

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

// nbk = B * Hkv, nkb = key blocks of 128 keys
__global__ __launch_bounds__(256)
    __attribute__((amdgpu_waves_per_eu(2, 2))) void k_gqa_bwd_dkdv_doc_hd64(
    const uint16_t* __restrict__ q, const uint16_t* __restrict__ k,
    const uint16_t* __restrict__ v, const uint16_t* __restrict__ dout,
    const float* __restrict__ lse, const float* __restrict__ delta,
    const int* __restrict__ doc_end, uint16_t* __restrict__ dk,
    uint16_t* __restrict__ dv, int nbk, int Hkv, int G, int T, int nkb,
    AttnStrides sq, AttnStrides sk, AttnStrides sv, AttnStrides sdo,
    AttnStrides sdk, AttnStrides sdv, int64_t lse_stride, float scale) {
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

  const int k0 = kblk * kRB;        // < T
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

  // document ends: of the workgroup's last key, of the wave's first and last
  // keys (uniform) and of the lane's key.  Keys at or past T take the values
  // of key T - 1 (uniform) or 0 (lane: no query sees them).
  const int* dep = doc_end + (int64_t)b * T;
  const int kl = min(k0 + kRB - 1, T - 1);
  const int de_wg = min(max(dep[kl], kl + 1), T);
  const int de_first = dep[min(kw0, T - 1)];
  const int de_last = dep[min(kw0 + kRW - 1, T - 1)];
  const int de_row = kok ? dep[krow] : 0;

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

  const int t_begin = k0 / kTile;                  // the tile of the block's keys
  const int t_end = (de_wg + kTile - 1) / kTile;   // > t_begin: de_wg > k0
  const int n_it = G * (t_end - t_begin);          // flattened (g, tile) count

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
    // sees the lane's key when need <= c < lim.  Tiles past the diagonal and
    // tiles that end inside the document of the wave's first key: a bound
    // that never bites.
    const int need = qt0 < kw0 + kRW - 1 ? krow - qt0 - 4 * hi : 0;
    const int lim = qt0 + kTile > de_first ? de_row - qt0 - 4 * hi : kNever;

#pragma unroll
    for (int qh = 0; qh < 2; ++qh) {
      // wave-uniform: the half tile has queries that see the wave's keys
      if (qt0 + 32 * qh + 31 < kw0 || qt0 + 32 * qh >= de_last) continue;
      dkdv_doc_half_tile(Qt, Dt, LD, lo, qh, hi, need, lim, scale_log2e, kf,
                         vf, dka, dva);
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

void hip_gqa_attn_bwd_doc_hd64(
    const void* q, const void* k, const void* v, const void* out,
    const void* dout, const float* lse, const int32_t* doc_start,
    const int32_t* doc_end, void* dq, void* dk, void* dv, float* delta,
    int64_t B, int64_t Hq, int64_t Hkv, int64_t T, const int64_t* qs,
    const int64_t* ks, const int64_t* vs, const int64_t* os,
    const int64_t* dos, const int64_t* dqs, const int64_t* dks,
    const int64_t* dvs, int64_t lse_stride, float scale, hipStream_t s) {
  const char* op = "gqa_attn_bwd_doc_hd64";
  const int64_t G = check_attn_bwd(op, q, k, v, out, dout, lse, dq, dk, dv,
                                   delta, B, Hq, Hkv, T, qs, ks, vs, os, dos,
                                   dqs, dks, dvs, lse_stride, scale,
                                   /*grouped=*/true);
  if (!doc_start || !doc_end)
    throw std::runtime_error(std::string(op) +
                             ": doc_start or doc_end is null");
  check_align(doc_start, 4, op, "doc_start");
  check_align(doc_end, 4, op, "doc_end");
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
        u16(q), u16(k), u16(v), u16(out), u16(dout), lse, doc_start,
        static_cast<uint16_t*>(dq), delta, (int)nbk, (int)Hkv, (int)G, (int)T,
        (int)nqb, st3(qs), st3(ks), st3(vs), st3(os), st3(dos), st3(dqs),
        lse_stride, scale);
  };
  if (HW == 2)
    launch_dq(k_gqa_bwd_dq_doc_hd64<2>);
  else
    launch_dq(k_gqa_bwd_dq_doc_hd64<4>);
  HIP_CHECK(hipGetLastError());
  k_gqa_bwd_dkdv_doc_hd64<<<dim3((unsigned)grid_kv), dim3(256), 0, s>>>(
      u16(q), u16(k), u16(v), u16(dout), lse, delta, doc_end,
      static_cast<uint16_t*>(dk), static_cast<uint16_t*>(dv), (int)nbk,
      (int)Hkv, (int)G, (int)T, (int)nkb, st3(qs), st3(ks), st3(vs), st3(dos),
      st3(dks), st3(dvs), lse_stride, scale);
  HIP_CHECK(hipGetLastError());
}

}  // namespace shamd
