// What the attention backward kernels for head dim 64 share,
// attn_bwd_kernels.hip (MHA) and gqa_attn_bwd_kernels.hip (GQA): the LDS tile
// swizzle, the two LDS read patterns that feed mfma_f32_32x32x16_bf16, the
// staged whole-row epilogue, with and without the column sums of what it
// stores (MHA only), the dQ kernel up to its store (attn_bwd_dq_body; MHA is
// its HW = 1, G = 1 case), the half tile of the dK/dV kernels
// (dkdv_half_tile) and the launchers' argument checks.  The header comment
// of attn_bwd_kernels.hip derives the swizzle and the lane layouts.
// gqa_attn_hd128_bwd_kernels.hip (head dim 128) takes the swizzle, the two
// read patterns and the checks from here, a 256-byte row being two 64-column
// halves of this tile format.  Everything sits in an anonymous namespace: each kernel file gets its own
// copy, inlined.
#pragma once

#include "attn_tile.h"

namespace shamd {
namespace {

constexpr int kD = 64;          // head dim
constexpr int kTileBytes = kTile * kD * 2;

// the chunk swizzle of a row: f((row >> 1) & 7)
__device__ __forceinline__ int swz(int row) {
  int x = (row >> 1) & 7;
  return x ^ ((x & 1) << 2);
}
// byte offset of 16-byte chunk `ch` (0..7) of row `row` in a tile
__device__ __forceinline__ int t_off(int row, int ch) {
  return row * 128 + ((ch ^ swz(row)) << 4);
}

__device__ __forceinline__ u32x4 load16_or_zero(const uint16_t* p, bool ok) {
  u32x4 z = {0, 0, 0, 0};
  return ok ? *reinterpret_cast<const u32x4*>(p) : z;
}

// the other lane half's value (lane ^ 32)
__device__ __forceinline__ float other_half(float x, int lane) {
  return __builtin_bit_cast(
      float, __builtin_amdgcn_ds_bpermute((lane ^ 32) << 2,
                                          __builtin_bit_cast(int, x)));
}

// Per-lane parts of the two LDS read patterns.
struct LaneOffs {
  // row-wise A operand: row 32 blk + r, chunk 2 ks + hi -> row_ks[ks] +
  // 32 * 128 * blk (the swizzle depends on r alone)
  int row_ks[4];
  // transposed A operand: tr[p] is the lane's address for rows 0..3 + 4 hi
  // of a 16-row group and a column block nb with nb ^ jj == p (jj: second
  // 8 rows of the group, which flips bit 2 of the swizzle)
  int tr[2];
};

__device__ __forceinline__ LaneOffs lane_offs(int lane) {
  LaneOffs o;
  const int r = lane & 31, hi = lane >> 5;
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) o.row_ks[ks] = t_off(r, 2 * ks + hi);
  // 16-lane group g reads rows 4 (g >> 1) + 0..3, columns 16 (g & 1) + 0..15
  // of the 32-column block; lane 4 qq + p of the group supplies row qq,
  // columns 4 p .. 4 p + 3
  const int grp = lane >> 4, gi = lane & 15;
  const int tq = gi >> 2, tp = gi & 3;
  const int row = 4 * (grp >> 1) + tq;
#pragma unroll
  for (int p = 0; p < 2; ++p)
    o.tr[p] = t_off(row, 4 * p + 2 * (grp & 1) + (tp >> 1)) + 8 * (tp & 1);
  return o;
}

// A operand read row-wise: lane holds tile[32 blk + r][16 ks + 8 hi + j]
__device__ __forceinline__ bf16x8 row_frag(const unsigned char* tile,
                                           const LaneOffs& lo, int blk,
                                           int ks) {
  u32x4 t = *reinterpret_cast<const u32x4*>(tile + blk * (kRW * 128) +
                                            lo.row_ks[ks]);
  return __builtin_bit_cast(bf16x8, t);
}

// A operand read transposed: lane holds, as element j,
// tile[16 ss + 8 (j >> 2) + 4 hi + (j & 3)][32 nb + r], the row order the
// registers 8 (ss & 1) .. + 7 of a 32 x 32 mfma result have
__device__ __forceinline__ bf16x8 tr_frag(const unsigned char* tile,
                                          const LaneOffs& lo, int ss, int nb) {
  bf16x8 f;
#pragma unroll
  for (int jj = 0; jj < 2; ++jj) {
    // rows 16 ss + 8 jj + ..: (row >> 1) & 7 gains 4 jj, the swizzle flips
    // bit 2 of the chunk with jj, as nb does
    auto* a = reinterpret_cast<__attribute__((address_space(3))) s16x4*>(
        (uintptr_t)(tile + (16 * ss + 8 * jj) * 128 + lo.tr[nb ^ jj]));
    s16x4 tr = __builtin_amdgcn_ds_read_tr16_b64_v4i16(a);
    bf16x4 tb = __builtin_bit_cast(bf16x4, tr);
#pragma unroll
    for (int e = 0; e < 4; ++e) f[4 * jj + e] = tb[e];
  }
  return f;
}

// fp32 rows of a wave -> bf16 through the wave's 4 KB of LDS -> whole-row
// global stores.  acc: lane holds row r, columns 32 nb + (reg & 3) +
// 8 (reg >> 2) + 4 hi.
__device__ __forceinline__ void stage_rows(unsigned char* Ow,
                                           const f32x16 (&acc)[2], float mul,
                                           int r, int hi) {
#pragma unroll
  for (int nb = 0; nb < 2; ++nb)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      bf16x4 f;
#pragma unroll
      for (int e = 0; e < 4; ++e) f[e] = (__bf16)(acc[nb][4 * g + e] * mul);
      // d = 32 nb + 8 g + 4 hi + e: chunk 4 nb + g, its half hi
      *reinterpret_cast<bf16x4*>(Ow + t_off(r, 4 * nb + g) + 8 * hi) = f;
    }
}

__device__ __forceinline__ void store_rows(const unsigned char* Ow,
                                           uint16_t* dst, int64_t row_stride,
                                           int row0, int T, int lane) {
#pragma unroll
  for (int pass = 0; pass < 4; ++pass) {
    int row = pass * 8 + (lane >> 3), ch = lane & 7;
    u32x4 val = *reinterpret_cast<const u32x4*>(Ow + t_off(row, ch));
    int gr = row0 + row;
    if (gr < T)
      *reinterpret_cast<u32x4*>(dst + (int64_t)gr * row_stride + 8 * ch) = val;
  }
}

// store_rows that also sums, per column, the bf16 values it stores.  A lane
// meets the same 16-byte chunk (8 columns) in all four passes, so the sums of
// its rows pass, pass + 8, ... live in cs[0..7], added in pass order.  Rows at
// or past T are neither stored nor summed.
__device__ __forceinline__ void store_rows_colsum(const unsigned char* Ow,
                                                  uint16_t* dst,
                                                  int64_t row_stride, int row0,
                                                  int T, int lane,
                                                  float (&cs)[8]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) cs[e] = 0.f;
#pragma unroll
  for (int pass = 0; pass < 4; ++pass) {
    int row = pass * 8 + (lane >> 3), ch = lane & 7;
    u32x4 val = *reinterpret_cast<const u32x4*>(Ow + t_off(row, ch));
    int gr = row0 + row;
    if (gr < T) {
      *reinterpret_cast<u32x4*>(dst + (int64_t)gr * row_stride + 8 * ch) = val;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        cs[2 * i] += __builtin_bit_cast(float, val[i] << 16);
        cs[2 * i + 1] += __builtin_bit_cast(float, val[i] & 0xffff0000u);
      }
    }
  }
}

// Column sums of a workgroup's NOUT staged outputs -> one fp32 partial row of
// 64 columns per output.  cs[o]: the lane's sums from store_rows_colsum.
// The 8 lanes of a wave that share a chunk (lane, lane ^ 8, ^ 16, ^ 32) are
// added as a butterfly: both sides of an exchange add the same two numbers,
// so every lane ends with the same bits.  Then each wave puts its NOUT x 64
// sums at the start of its own staging area (`wave_bytes` apart, its rows
// are read by then) and thread 64 o + c adds the four waves of column c of
// output o in wave order.  Every thread of the workgroup calls it.
template <int NOUT>
__device__ __forceinline__ void colsum_partial_rows(unsigned char* lds,
                                                    int wave_bytes, int wave,
                                                    int tid,
                                                    float (&cs)[NOUT][8],
                                                    float* const (&dst)[NOUT]) {
  const int lane = tid & 63;
#pragma unroll
  for (int m = 8; m < 64; m <<= 1)
#pragma unroll
    for (int o = 0; o < NOUT; ++o)
#pragma unroll
      for (int e = 0; e < 8; ++e)
        cs[o][e] += __builtin_bit_cast(
            float, __builtin_amdgcn_ds_bpermute(
                       (lane ^ m) << 2, __builtin_bit_cast(int, cs[o][e])));
  // orders the reads of the staged rows before the overwrite
  __syncthreads();
  if (lane < 8) {
    float* mine = reinterpret_cast<float*>(lds + wave * wave_bytes) + 8 * lane;
#pragma unroll
    for (int o = 0; o < NOUT; ++o) {
      f32x4 a = {cs[o][0], cs[o][1], cs[o][2], cs[o][3]};
      f32x4 b = {cs[o][4], cs[o][5], cs[o][6], cs[o][7]};
      *reinterpret_cast<f32x4*>(mine + kD * o) = a;
      *reinterpret_cast<f32x4*>(mine + kD * o + 4) = b;
    }
  }
  __syncthreads();
  if (tid < NOUT * kD) {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < kWaves; ++w)
      t += reinterpret_cast<const float*>(lds + w * wave_bytes)[tid];
    float* d = dst[0];
#pragma unroll
    for (int o = 1; o < NOUT; ++o)
      if (tid >= o * kD) d = dst[o];
    d[tid % kD] = t;
  }
}

// ------------------------------------------------------------------ dQ

// What the store epilogue of a dQ kernel needs: the wave's batch, query head,
// position block, first query row and its 4 KB of staged bf16 dQ rows.
struct DqRows {
  int b, h, qb, qw0;
  unsigned char* Ow;
};

// A dQ kernel from its prologue through stage_rows and the barrier behind
// it, for the workgroup of kv head `bk`, block slot `slot` (grid_map over
// nqb * G / HW slots).  A wave is a query head: workgroup = 4 waves = HW heads
// of one kv group x 128 / HW consecutive query positions.  lds: 4 tiles.
// nqb = position blocks of 128 / HW rows.
template <int HW>
__device__ __forceinline__ DqRows attn_bwd_dq_body(
    unsigned char* lds, int bk, int slot, const uint16_t* q,
    const uint16_t* k, const uint16_t* v, const uint16_t* out,
    const uint16_t* dout, const float* lse, float* delta, int Hkv, int G,
    int T, int nqb, AttnStrides sq, AttnStrides sk, AttnStrides sv,
    AttnStrides so, AttnStrides sdo, int64_t lse_stride, float scale) {
  constexpr int kWPH = kWaves / HW;  // waves per head
  constexpr int kPB = kRW * kWPH;    // positions per workgroup
  // K buffers at 0 and kTileBytes, V buffers behind them
  unsigned char* const ldsK = lds;
  unsigned char* const ldsV = lds + 2 * kTileBytes;

  const int nhalf = G / HW;
  const int qb = nqb - 1 - slot / nhalf;  // heaviest block first
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
  return DqRows{b, h, qb, qw0, Ow};
}

// ------------------------------------------------------------- dK, dV

// One 32-query half tile qh of a dK/dV kernel: S = Q K^T and dP = dO V^T for
// queries 32 qh + rowmap(reg, hi) of the tile, P and dS per register, then
// dV^T += dO^T P and dK^T += Q^T dS.  LD: the tile's 64 -lse log2(e) and 64
// delta values, read as 16-byte broadcast reads.  Query c of the tile sees
// the lane's key when c >= need.
__device__ __forceinline__ void dkdv_half_tile(
    const unsigned char* Qt, const unsigned char* Dt, const float* LD,
    const LaneOffs& lo, int qh, int hi, int need, float scale_log2e,
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
      if (c0 + e < need) p = 0.f;
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

// ------------------------------------------------------------------ host

// no two rows of a (B, T, H, row) output may overlap: with the dimensions of
// more than one element ordered by stride, the smallest stride covers a
// `row`-element row and every further one the whole extent of the dimension
// before it
inline bool rows_disjoint(const int64_t* st, int64_t B, int64_t T, int64_t H,
                          int64_t row = kD) {
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
  int64_t need = row;
  for (int i = 0; i < n; ++i) {
    if (sd[i][0] < need) return false;
    need = sd[i][0] * sd[i][1];
  }
  return true;
}

// The checks both backward launchers make before they size their grids;
// returns G = Hq / Hkv.  The MHA op passes Hq == Hkv and grouped = false, the
// head-dim-128 op row = 128.
inline int64_t check_attn_bwd(
    const char* op, const void* q, const void* k, const void* v,
    const void* out, const void* dout, const float* lse, const void* dq,
    const void* dk, const void* dv, const float* delta, int64_t B, int64_t Hq,
    int64_t Hkv, int64_t T, const int64_t* qs, const int64_t* ks,
    const int64_t* vs, const int64_t* os, const int64_t* dos,
    const int64_t* dqs, const int64_t* dks, const int64_t* dvs,
    int64_t lse_stride, float scale, bool grouped, int64_t row = kD) {
  const int64_t G =
      check_attn_problem(op, B, Hq, Hkv, T, lse_stride, scale, grouped);
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
  check_attn_strides(op, {qs, ks, vs, os, dos, dqs, dks, dvs});
  if (!rows_disjoint(dqs, B, T, Hq, row) ||
      !rows_disjoint(dks, B, T, Hkv, row) ||
      !rows_disjoint(dvs, B, T, Hkv, row))
    throw std::runtime_error(std::string(op) + ": output rows would overlap");
  return G;
}

}  // namespace
}  // namespace shamd
