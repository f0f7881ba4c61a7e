// Causal bf16 grouped-query attention backward for head dim 128 (Llama-3-8B:
// 32 query heads, 8 kv heads, G = 4), the counterpart of
// gqa_attn_hd128_kernels.hip under the contract of gqa_attn_bwd_kernels.hip:
// Hq = G Hkv query heads, query head h reads kv head h / G, G in {2, 4, 8};
// fp32 accumulation, bf16 in and out, no dropout, no bias, top-left aligned
// causal mask (Tq == Tk).  Two kernels, no atomics, one fp32 workspace delta
// (B, Hq, T); every output element is written once by one lane from one
// fixed-order sum, so repeats are bit-identical.  K and V are read in place
// through their strides, never expanded; dK and dV of a kv head are summed
// over its G query heads in the fp32 accumulators of one workgroup and
// rounded to bf16 once.
//
// The math, the lane layouts and the t_off swizzle are those of
// attn_bwd_kernels.hip (see its header), taken from attn_bwd_tile.h:
// mfma_f32_32x32x16_bf16, S^T and dP^T with the lane owning a row, row_frag
// and tr_frag.  A 256-byte row is stored as in the hd128 forward: two
// 64-column halves, each a [rows][128 B] t_off tile, the second half behind
// the first.  A row-wise read (chunk 2 ks + hi, ks = 0..7) lies in half
// ks >> 2 and a transposed read (column block nb = 0..3) in half nb >> 1, so
// both are the hd64 reads at a shifted base and keep the hd64 bank pattern
// (profiles/r11/lds_bank_conflicts.txt).  Staging writes put 8 lanes on the
// 128 bytes of one row of one half, which is the hd64 write.
//
// Plan where head dim 128 breaks the hd64 one
// (tests/test_gqa_attn_hd128_bwd_resource_usage.py holds the kernels to it):
//
//   k_gqa_bwd_dq_hd128<HW>, HW = min(G, 4): a wave is a query head, the grid
//   map is k_gqa_bwd_dq_hd64's (heaviest position block first, head halves
//   adjacent).
//   * Registers per lane: Q and dO fragments 8 x bf16x8 each = 64, dQ^T
//     4 x f32x16 = 64, s and dp of one 32-key half tile 32, dS fragments 8,
//     the next 64-key K and V tile staged through registers 32: 200 before
//     addresses.  amdgpu_waves_per_eu(2, 2): 256 registers, no scratch, no
//     spills.
//   * LDS: K and V 64-key tiles of 16 KB, double buffered: 64 KB static, two
//     workgroups per CU, the 2 waves/SIMD the registers give.
//   * Per half tile 8 k-steps each of K Q^T and V dO^T, then 4 column blocks
//     x 2 k-steps of K^T dS^T; one barrier per 64-key tile.
//   * delta is computed here from the lane's own 64 dO and O elements: one
//     sequential fma chain per lane half, the two halves added once.
//   * The epilogue stages 32 x 256 B of dQ per wave through the dead tiles to
//     whole-row stores.
//
//   k_gqa_bwd_dkdv_hd128: workgroup = 4 waves = 128 keys of one (b, kv head),
//   a lane owns a key; one flattened (g, query tile) loop whose pipeline
//   crosses head boundaries without draining, buffer parity following the
//   flattened index; the grid is k_gqa_bwd_dkdv_hd64's, first (heaviest) key
//   block first.
//   * The hd64 plan does not fit: K and V fragments 64, dK^T and dV^T 128,
//     s, dp, P and dS of a half tile 48: 240 before staging or addresses.
//   * 32-query tiles (Q 8 KB + dO 8 KB per buffer): 8 + 8 MFMAs of S and dP
//     and 2 x 4 x 2 of dV^T and dK^T, 32 per wave per barrier, the cadence of
//     hd64's 64-query tile.
//   * Lever A: the V fragments live in LDS.  The block's 128 x 256 B of V
//     (32 KB) is stored once in the prologue and read row-wise as the B
//     operand of dP in every tile.  Persistent registers: K fragments 32 +
//     accumulators 128 = 160; with s, dp, P, dS (48) and 16 registers of
//     Q/dO staging 224 before addresses.  amdgpu_waves_per_eu(2, 2).
//   * LDS read per wave and tile: row-wise Q, dO and V 8 KB each, 16
//     transposed fragments of 1 KB: 40 KB for 32 MFMAs, 1280 B per MFMA.
//     With V in registers (or lever B, direct-to-LDS loads) it would be
//     1024 B per MFMA, hd64's figure; lever A pays 25% more LDS reads for not
//     depending on loads that cannot zero-fill rows past T.
//   * LDS: 32 KB of V + 2 x (8 KB + 8 KB) + 2 x 64 floats of -lse log2(e) and
//     delta = 66048 B, over the 64 KB a static allocation may be: it is
//     dynamic (the launcher raises the kernel's limit once per device), the
//     compile report shows 0 B.  Two workgroups fit the CU's 160 KB.
//   * dK is scaled and dK, dV rounded once in the epilogue, and staged
//     (16 KB per wave) through the dead tiles to whole-row stores.
//   * Ordering all (b, kv head) globally heaviest-first was not tried.
//
// As built (gfx950, -O3, without packed fp32 ops, build.py EXTRA_FLAGS):
// k_gqa_bwd_dq_hd128<2> and <4> 234 VGPRs, 54 and 52 SGPRs, 65536 B of LDS;
// k_gqa_bwd_dkdv_hd128 249 VGPRs, 77 SGPRs, 0 B static + 66048 B dynamic LDS;
// all three no AGPRs, no scratch, no spills, 2 waves/SIMD.  No deviation
// from the plan; lever B and waves_per_eu(1, 1) were not needed.
//
// Every T is bounds-checked: rows at or past T are read as zeros (never from
// memory), contribute exactly nothing, and are never stored.
#include <hip/hip_runtime.h>

#include "attn_bwd_tile.h"
#include "device_util.h"
#include "hip_api.h"

namespace shamd {
namespace {

constexpr int kD128 = 128;
constexpr int kKvHalf = kTile * 128;  // 64-key K or V tile: two 8 KB halves
constexpr int kKvTile = 2 * kKvHalf;
constexpr int kQRows = 32;            // query tile of the dK/dV kernel
constexpr int kQHalf = kQRows * 128;  // two 4 KB halves
constexpr int kQTile = 2 * kQHalf;
constexpr int kVHalf = kRB * 128;     // the key block's V: two 16 KB halves
constexpr int kVBlock = 2 * kVHalf;
constexpr int kDkdvLds = kVBlock + 4 * kQTile + 2 * 2 * kQRows * 4;

// fp32 rows of a wave -> bf16 through the wave's 8 KB of LDS (two 4 KB
// halves) -> whole-row global stores.  acc: lane holds row r, columns
// 32 nb + (reg & 3) + 8 (reg >> 2) + 4 hi.
__device__ __forceinline__ void stage_rows128(unsigned char* Ow,
                                              const f32x16 (&acc)[4],
                                              float mul, int r, int hi) {
#pragma unroll
  for (int nb = 0; nb < 4; ++nb)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      bf16x4 f;
#pragma unroll
      for (int e = 0; e < 4; ++e) f[e] = (__bf16)(acc[nb][4 * g + e] * mul);
      // d = 32 nb + 8 g + 4 hi + e: half nb >> 1, chunk 4 (nb & 1) + g
      *reinterpret_cast<bf16x4*>(Ow + (nb >> 1) * kQHalf +
                                 t_off(r, 4 * (nb & 1) + g) + 8 * hi) = f;
    }
}

// 16 lanes store the 256 bytes of one row
__device__ __forceinline__ void store_rows128(const unsigned char* Ow,
                                              uint16_t* dst,
                                              int64_t row_stride, int row0,
                                              int T, int lane) {
#pragma unroll
  for (int pass = 0; pass < 8; ++pass) {
    int row = pass * 4 + (lane >> 4), c = lane & 15;
    u32x4 val = *reinterpret_cast<const u32x4*>(Ow + (c >> 3) * kQHalf +
                                                t_off(row, c & 7));
    int gr = row0 + row;
    if (gr < T)
      *reinterpret_cast<u32x4*>(dst + (int64_t)gr * row_stride + 8 * c) = val;
  }
}

// ------------------------------------------------------------------ dQ

// nbk = B * Hkv, nqb = position blocks of 128 / HW rows, G / HW head halves
template <int HW>
__global__ __launch_bounds__(256)
    __attribute__((amdgpu_waves_per_eu(2, 2))) void k_gqa_bwd_dq_hd128(
    const uint16_t* __restrict__ q, const uint16_t* __restrict__ k,
    const uint16_t* __restrict__ v, const uint16_t* __restrict__ out,
    const uint16_t* __restrict__ dout, const float* __restrict__ lse,
    uint16_t* __restrict__ dq, float* __restrict__ delta, int nbk, int Hkv,
    int G, int T, int nqb, AttnStrides sq, AttnStrides sk, AttnStrides sv,
    AttnStrides so, AttnStrides sdo, AttnStrides sdq, int64_t lse_stride,
    float scale) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[4 * kKvTile];
  constexpr int kWPH = kWaves / HW;  // waves per head
  constexpr int kPB = kRW * kWPH;    // positions per workgroup
  // K buffers at 0 and kKvTile, V buffers behind them
  unsigned char* const ldsK = lds;
  unsigned char* const ldsV = lds + 2 * kKvTile;

  int bk, slot;
  const int nhalf = G / HW;
  if (!grid_map(nbk, nqb * nhalf, bk, slot)) return;  // whole workgroup
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
  // delta from the same elements of dO and O: one fma chain per lane half.
  bf16x8 qf[8], dof[8];
  float dl = 0.f;
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) {
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

  // staging: thread covers 16-byte chunk (tid & 7) of both halves of keys
  // (tid >> 3) and (tid >> 3) + 32 of the tile, for K and for V; i = 2 jk + hf
  const int skey = tid >> 3, sch = tid & 7;
  u32x4 stK[4], stV[4];
  auto issue = [&](int kv0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int key = kv0 + skey + 32 * (i >> 1);
      bool ok = key < T;
      int col = 64 * (i & 1) + 8 * sch;
      stK[i] = load16_or_zero(kp + (int64_t)key * sk.t + col, ok);
      stV[i] = load16_or_zero(vp + (int64_t)key * sv.t + col, ok);
    }
  };
  auto commit = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int off = buf * kKvTile + (i & 1) * kKvHalf +
                t_off(skey + 32 * (i >> 1), sch);
      *reinterpret_cast<u32x4*>(ldsK + off) = stK[i];
      *reinterpret_cast<u32x4*>(ldsV + off) = stV[i];
    }
  };

  const int kv_end = min(T, q0 + kPB);              // keys this block can see
  const int ntiles = (kv_end + kTile - 1) / kTile;  // >= 1

  // dQ^T: lane holds dQ[qrow][32 nb + (reg&3) + 8 (reg>>2) + 4 hi]
  f32x16 acc[4];
#pragma unroll
  for (int nb = 0; nb < 4; ++nb)
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

    const unsigned char* Kt = ldsK + cur * kKvTile;
    const unsigned char* Vt = ldsV + cur * kKvTile;
    // keys of the tile are kv0 + 4 hi + c, c a register constant; key c is
    // visible when c <= vis.  Tiles below the diagonal: everything.
    const int vis = kv0 + kTile - 1 > qw0 ? qrow - kv0 - 4 * hi : kTile;

#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      // wave-uniform: the half tile has keys the wave's rows can see
      if (kv0 + 32 * kb > qw0 + kRW - 1) continue;

      // S^T = K Q^T and dP^T = V dO^T for keys kv0 + 32 kb + keymap(reg, hi):
      // one MFMA chain of 8 k-steps each
      f32x16 s, dp;
#pragma unroll
      for (int i = 0; i < 16; ++i) s[i] = dp[i] = 0.f;
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) {
        const int ho = (ks >> 2) * kKvHalf;
        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            row_frag(Kt + ho, lo, kb, ks & 3), qf[ks], s, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            row_frag(Vt + ho, lo, kb, ks & 3), dof[ks], dp, 0, 0, 0);
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
      for (int nb = 0; nb < 4; ++nb)
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2)
          acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              tr_frag(Kt + (nb >> 1) * kKvHalf, lo, 2 * kb + h2, nb & 1),
              dsf[h2], acc[nb], 0, 0, 0);
    }

    if (more) commit(cur ^ 1);
    __syncthreads();
  }

  // the loop's last barrier is behind every wave: the tiles are dead
  unsigned char* const Ow = lds + wave * kQTile;
  stage_rows128(Ow, acc, scale, r, hi);
  __syncthreads();
  store_rows128(Ow, dq + b * sdq.b + h * sdq.h, sdq.t, qw0, T, lane);
}

// ------------------------------------------------------------- dK, dV

// nbk = B * Hkv, nkb = key blocks of 128 keys; kDkdvLds bytes of dynamic LDS
__global__ __launch_bounds__(256)
    __attribute__((amdgpu_waves_per_eu(2, 2))) void k_gqa_bwd_dkdv_hd128(
    const uint16_t* __restrict__ q, const uint16_t* __restrict__ k,
    const uint16_t* __restrict__ v, const uint16_t* __restrict__ dout,
    const float* __restrict__ lse, const float* __restrict__ delta,
    uint16_t* __restrict__ dk, uint16_t* __restrict__ dv, int nbk, int Hkv,
    int G, int T, int nkb, AttnStrides sq, AttnStrides sk, AttnStrides sv,
    AttnStrides sdo, AttnStrides sdk, AttnStrides sdv, int64_t lse_stride,
    float scale) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  // the block's V, then Q buffers, dO buffers, and per buffer 32 floats of
  // -lse log2(e) and 32 of delta
  unsigned char* const ldsVb = lds;
  unsigned char* const ldsQ = lds + kVBlock;
  unsigned char* const ldsD = ldsQ + 2 * kQTile;
  float* const ldsLD = reinterpret_cast<float*>(ldsD + 2 * kQTile);

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
  const uint16_t* vp0 = v + b * sv.b + kvh * sv.h;
  // head G kvh of the group; head g of it is g strides further
  const int h0 = G * kvh;
  const int64_t bh0 = (int64_t)b * Hkv * G + h0;
  const uint16_t* const qp0 = q + b * sq.b + h0 * sq.h;
  const uint16_t* const dop0 = dout + b * sdo.b + h0 * sdo.h;
  const float* const lsep0 = lse + bh0 * lse_stride;
  const float* const deltap0 = delta + bh0 * T;

  // staging: thread covers 16-byte chunk (tid & 7) of both halves of row
  // (tid >> 3), for Q and for dO; threads 0..31 one lse, 32..63 one delta.
  // g (the head inside the group) is wave-uniform.
  const int srow = tid >> 3, sch = tid & 7;

  // the block's V rows, once: rows srow + 32 j of both halves
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int row = srow + 32 * j;
    const bool ok = k0 + row < T;
    const uint16_t* vp = vp0 + (int64_t)(k0 + row) * sv.t + 8 * sch;
#pragma unroll
    for (int hf = 0; hf < 2; ++hf)
      *reinterpret_cast<u32x4*>(ldsVb + hf * kVHalf + t_off(row, sch)) =
          load16_or_zero(vp + 64 * hf, ok);
  }

  // K fragments: B operands; lane holds K[krow][16 ks + 8 hi + j]
  bf16x8 kf[8];
#pragma unroll
  for (int ks = 0; ks < 8; ++ks)
    kf[ks] = __builtin_bit_cast(
        bf16x8, load16_or_zero(kp + 16 * ks + 8 * hi, kok));
  const float scale_log2e = scale * kLog2e;

  u32x4 stQ[2], stD[2];
  float stL = 0.f;
  auto issue = [&](int g, int qt0) {
    const int row = qt0 + srow;
    const bool ok = row < T;
    const uint16_t* qp = qp0 + g * sq.h + (int64_t)row * sq.t + 8 * sch;
    const uint16_t* dop = dop0 + g * sdo.h + (int64_t)row * sdo.t + 8 * sch;
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      stQ[hf] = load16_or_zero(qp + 64 * hf, ok);
      stD[hf] = load16_or_zero(dop + 64 * hf, ok);
    }
    if (tid < 2 * kQRows) {
      int lrow = qt0 + (tid & (kQRows - 1));
      stL = 0.f;
      if (lrow < T)
        stL = tid < kQRows ? -lsep0[g * lse_stride + lrow] * kLog2e
                           : deltap0[(int64_t)g * T + lrow];
    }
  };
  auto commit = [&](int buf) {
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      int off = buf * kQTile + hf * kQHalf + t_off(srow, sch);
      *reinterpret_cast<u32x4*>(ldsQ + off) = stQ[hf];
      *reinterpret_cast<u32x4*>(ldsD + off) = stD[hf];
    }
    if (tid < 2 * kQRows) ldsLD[buf * 2 * kQRows + tid] = stL;
  };

  const int t_begin = k0 / kQRows;               // the tile of the first key
  const int t_end = (T + kQRows - 1) / kQRows;   // > t_begin: k0 < T
  const int n_it = G * (t_end - t_begin);        // flattened (g, tile) count

  // dK^T, dV^T: lane holds dX[krow][32 nb + (reg&3) + 8 (reg>>2) + 4 hi],
  // summed over the whole group
  f32x16 dka[4], dva[4];
#pragma unroll
  for (int nb = 0; nb < 4; ++nb)
#pragma unroll
    for (int i = 0; i < 16; ++i) dka[nb][i] = dva[nb][i] = 0.f;

  issue(0, t_begin * kQRows);
  commit(0);
  __syncthreads();  // publishes V too

  // (g, t) of the iteration whose tile is being issued: one ahead of `it`
  int gn = 0, tn = t_begin;
  for (int it = 0; it < n_it; ++it) {
    const int cur = it & 1;        // parity of the flattened index
    const int qt0 = tn * kQRows;   // the current tile's first query
    const bool more = it + 1 < n_it;
    if (++tn == t_end) {           // next iteration: next tile or next head
      tn = t_begin;
      ++gn;
    }
    if (more) issue(gn, tn * kQRows);

    // wave-uniform: the tile has queries that see the wave's keys
    if (qt0 + kQRows - 1 >= kw0) {
      const unsigned char* Qt = ldsQ + cur * kQTile;
      const unsigned char* Dt = ldsD + cur * kQTile;
      const float* LD = ldsLD + cur * 2 * kQRows;
      // queries of the tile are qt0 + 4 hi + c, c a register constant; query
      // c sees the lane's key when c >= need.  Past the diagonal: all do.
      const int need = qt0 < kw0 + kRW - 1 ? krow - qt0 - 4 * hi : 0;

      // S = Q K^T and dP = dO V^T for queries qt0 + rowmap(reg, hi): one MFMA
      // chain of 8 k-steps each, V's B operand read row-wise from LDS
      f32x16 s, dp;
#pragma unroll
      for (int i = 0; i < 16; ++i) s[i] = dp[i] = 0.f;
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) {
        const int hf = ks >> 2;
        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            row_frag(Qt + hf * kQHalf, lo, 0, ks & 3), kf[ks], s, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            row_frag(Dt + hf * kQHalf, lo, 0, ks & 3),
            row_frag(ldsVb + hf * kVHalf, lo, wave, ks & 3), dp, 0, 0, 0);
      }

      bf16x8 pf[2], dsf[2];  // P and dS fragments: k-steps 0 and 1
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        // registers 4 g .. 4 g + 3 are queries 8 g + 4 hi + 0..3
        const int c0 = 8 * g;
        f32x4 nl4 = *reinterpret_cast<const f32x4*>(LD + c0 + 4 * hi);
        f32x4 dl4 = *reinterpret_cast<const f32x4*>(LD + kQRows + c0 + 4 * hi);
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

      // dV^T += dO^T P and dK^T += Q^T dS
#pragma unroll
      for (int nb = 0; nb < 4; ++nb)
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2) {
          const int ho = (nb >> 1) * kQHalf;
          dva[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              tr_frag(Dt + ho, lo, h2, nb & 1), pf[h2], dva[nb], 0, 0, 0);
          dka[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              tr_frag(Qt + ho, lo, h2, nb & 1), dsf[h2], dka[nb], 0, 0, 0);
        }
    }

    if (more) commit(cur ^ 1);
    __syncthreads();
  }

  // the loop's last barrier is behind every wave: V and the tiles are dead; a
  // wave owns 16 KB, dK rows in the first 8 KB and dV rows in the second
  unsigned char* const Ow = lds + wave * (2 * kQTile);
  stage_rows128(Ow, dka, scale, r, hi);
  stage_rows128(Ow + kQTile, dva, 1.f, r, hi);
  __syncthreads();
  store_rows128(Ow, dk + b * sdk.b + kvh * sdk.h, sdk.t, kw0, T, lane);
  store_rows128(Ow + kQTile, dv + b * sdv.b + kvh * sdv.h, sdv.t, kw0, T,
                lane);
}

// The dK/dV kernel's LDS is over the static 64 KB: raise its dynamic limit,
// once per device.
void allow_dkdv_lds() {
  static bool done[64] = {};
  int dev = 0;
  HIP_CHECK(hipGetDevice(&dev));
  if (dev >= 0 && dev < 64 && done[dev]) return;
  HIP_CHECK(hipFuncSetAttribute(
      reinterpret_cast<const void*>(k_gqa_bwd_dkdv_hd128),
      hipFuncAttributeMaxDynamicSharedMemorySize, kDkdvLds));
  if (dev >= 0 && dev < 64) done[dev] = true;
}

}  // namespace

void hip_gqa_attn_bwd_causal_hd128(
    const void* q, const void* k, const void* v, const void* out,
    const void* dout, const float* lse, void* dq, void* dk, void* dv,
    float* delta, int64_t B, int64_t Hq, int64_t Hkv, int64_t T,
    const int64_t* qs, const int64_t* ks, const int64_t* vs,
    const int64_t* os, const int64_t* dos, const int64_t* dqs,
    const int64_t* dks, const int64_t* dvs, int64_t lse_stride, float scale,
    hipStream_t s) {
  const char* op = "gqa_attn_bwd_causal_hd128";
  const int64_t G = check_attn_bwd(op, q, k, v, out, dout, lse, dq, dk, dv,
                                   delta, B, Hq, Hkv, T, qs, ks, vs, os, dos,
                                   dqs, dks, dvs, lse_stride, scale,
                                   /*grouped=*/true, /*row=*/kD128);
  const int HW = G < 4 ? 2 : 4;
  const int64_t pb = kRB / HW;
  const int64_t nqb = (T + pb - 1) / pb;
  const int64_t nkb = (T + kRB - 1) / kRB;
  const int64_t nbk = B * Hkv;
  const int64_t grid_dq = attn_grid(op, B, Hq, Hkv, T, nqb * (G / HW));
  const int64_t grid_kv = attn_grid(op, B, Hq, Hkv, T, nkb);
  allow_dkdv_lds();
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
    launch_dq(k_gqa_bwd_dq_hd128<2>);
  else
    launch_dq(k_gqa_bwd_dq_hd128<4>);
  HIP_CHECK(hipGetLastError());
  k_gqa_bwd_dkdv_hd128<<<dim3((unsigned)grid_kv), dim3(256), kDkdvLds, s>>>(
      u16(q), u16(k), u16(v), u16(dout), lse, delta,
      static_cast<uint16_t*>(dk), static_cast<uint16_t*>(dv), (int)nbk,
      (int)Hkv, (int)G, (int)T, (int)nkb, st3(qs), st3(ks), st3(vs), st3(dos),
      st3(dks), st3(dvs), lse_stride, scale);
  HIP_CHECK(hipGetLastError());
}

}  // namespace shamd
