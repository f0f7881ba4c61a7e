// Causal bf16 attention backward for head dim 64 (GPT-2), the counterpart of
// attn_kernels.hip: fp32 accumulation, bf16 in and out, no dropout, no bias,
// top-left aligned causal mask (Tq == Tk).  Two kernels, no atomics, one fp32
// workspace delta (B, H, T); every output element is written once by one
// lane from one fixed-order sum, so repeats are bit-identical.
//
// The softmax is not recomputed: with the forward's natural-log lse,
//   P = exp2(s * scale * log2(e) - lse * log2(e)),
//   dS = P * (dP - delta),  delta[q] = sum_d dO[q][d] O[q][d],
//   dQ = scale dS K,  dK = scale dS^T Q,  dV = P^T dO.
//
// Plan (tests/test_attn_bwd_resource_usage.py holds both kernels to it):
//   * Tiles in LDS are 64 rows x 128 B.  16-byte chunk c of row r sits at
//     chunk c ^ f((r >> 1) & 7), f(x) = x ^ ((x & 1) << 2).  One swizzle
//     serves both reads of a tile, so no tile is staged twice:
//       - row-wise (ds_read_b128, 16 consecutive rows, one chunk): f is a
//         bijection of 0..7, so the 16 lanes touch 16 different 16-byte
//         slots of the 256-byte bank line, as the forward's K swizzle does;
//       - transposed (ds_read_b64_tr_b16, a 32-lane half fetches 4 rows
//         r0..r0+3 x 64 B, r0 a multiple of 4): rows r0, r0+1 get f = x and
//         rows r0+2, r0+3 get f = x ^ 5, which moves their 64 bytes to the
//         other half of the 128-byte row, so the 4 x 64 B cover the bank
//         line once, as the forward's V swizzle does.
//     This was chosen from the bank arithmetic; the counters then showed 4.1%
//     (dq) and 4.6% (dkdv) of the LDS-active cycles as bank-conflict cycles,
//     against 3.4% in the forward (profiles/r11/).  Staging K twice (48 KB,
//     one workgroup per CU fewer in k_attn_bwd_dq) was not measured.
//   * The lane layouts are the forward's.  mfma_32x32x16(A, B) with A read
//     row-wise from LDS and B held in registers gives a lane one column
//     (lane & 31) and the 16 rows (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).
//     Registers 8s .. 8s+7 of such a result, converted to bf16, are the B
//     operand of k-step s of a second mfma whose A operand is the transposed
//     read of a tile: that read delivers the rows in the same permuted
//     order, so P and dS never move between lanes or through LDS.
//
//   k_attn_bwd_dq: workgroup = 4 waves = 128 query rows of one (b, h), a
//   lane owns one query; loops over 64-key tiles up to the diagonal.
//   * Q and dO stay in registers (B operands).  delta comes from the lane's
//     half rows of dO and O plus one exchange between the lane halves and is
//     written to the workspace (no preprocess pass).
//   * K and V tiles double-buffered in LDS, 2 x (8 KB + 8 KB) = 32 KB, next
//     tile's global loads issued before the MFMAs, one barrier per tile.
//   * per 32-key half tile: S^T = mfma(K, Q), dP^T = mfma(V, dO) (V read
//     row-wise like K), dS^T = P^T (dP^T - delta) per lane,
//     dQ^T += mfma(K^T, dS^T).  Working on half tiles keeps S^T and dP^T at
//     16 registers each; half tiles wholly above a wave's rows are skipped,
//     only the tile that crosses the diagonal is masked.
//   * scale is applied once to dQ in the epilogue; dQ goes through LDS so
//     that every global store is a whole 128-byte row.
//   * Grid: the forward's (query blocks of one (b, h) consecutive on one
//     XCD, heaviest (last) block first).
//   * Resources: amdgpu_waves_per_eu(3, 3): at most 160 VGPRs (156 as
//     built; 168 is the limit of the occupancy step), no AGPRs, no scratch,
//     no spills, 32 KB of LDS -> 3 waves/SIMD, 3 workgroups per CU.
//     Q, dO, dQ^T, S^T, dP^T, dS^T and the 16 staging registers are 136
//     before any address; held to 128 registers (4 waves/SIMD) the compiler
//     spills 38 of them into the tile loop.
//
//   k_attn_bwd_dkdv: workgroup = 4 waves = 128 keys of one (b, h), a lane
//   owns one key; loops over 64-query tiles from the diagonal tile to the end.
//   * K and V stay in registers (B operands); dK^T and dV^T are 64 fp32
//     accumulator registers per lane.
//   * Q and dO tiles plus 64 (-lse log2 e) and 64 delta values are
//     double-buffered in LDS: 2 x (8 KB + 8 KB + 512 B) = 33 KB.
//   * per 32-query half tile: S = mfma(Q, K), dP = mfma(dO, V); P and dS per
//     register, lse and delta of the register's query read from LDS as
//     16-byte broadcast reads; dV^T += mfma(dO^T, P), dK^T += mfma(Q^T, dS).
//   * Half tiles wholly before a wave's keys are skipped, only the tile that
//     crosses the diagonal is masked, queries at or past T contribute zero
//     (their Q, dO, lse and delta are staged as zeros).
//   * dK is scaled in the epilogue; dK and dV go through LDS to whole-row
//     stores.
//   * Grid: key blocks of one (b, h) consecutive on one XCD, first
//     (heaviest) key block first.
//   * Resources: K, V, the accumulators, S, dP and the staging registers do
//     not fit 128 registers.  amdgpu_waves_per_eu(2, 2): at most 200 VGPRs
//     (198 as built; 256 is the limit of the occupancy step), no AGPRs, no
//     scratch, no spills -> 2 waves/SIMD, 2 workgroups per CU (LDS would
//     allow 4).
//
// Column sums (qkv.bias.grad).  With the partials pointers set (csq; csk and
// csv), the store epilogue also sums, per column, the bf16 values it stores
// (store_rows_colsum, colsum_partial_rows in attn_bwd_tile.h): 4 rows per
// lane, the 8 lanes of a chunk, then the 4 waves through the staging LDS the
// wave has just read, so LDS stays at 32 KB and 33 KB.  The workgroup writes
// 64 fp32 sums per output to row b * nblocks + block, columns 64 h.. of its
// output's third of the 3C-wide partial row; k_colsum_reduce
// (bias_grad_kernels.hip) sums the rows.  Fixed order, no atomics.  The
// pointers are kernel arguments checked at run time, not a second
// instantiation: the null path costs one scalar branch, the epilogue's eight
// sums live in registers the accumulators have left (156 and 198 VGPRs as
// built, the occupancy steps are unchanged), and one code object keeps the
// plain path of the A/B arm identical to the kernel that is shipped.
//
// Every T is bounds-checked: rows at or past T are read as zeros (never from
// memory) and never stored.
#include <hip/hip_runtime.h>

#include "attn_bwd_tile.h"
#include "device_util.h"
#include "hip_api.h"

namespace shamd {
namespace {

// The tile swizzle, the two LDS read patterns, the staged epilogue, the dQ
// body and the dK/dV half tile live in attn_bwd_tile.h, shared with
// gqa_attn_bwd_kernels.hip.

// ------------------------------------------------------------------ dQ

__global__ __launch_bounds__(256)
    __attribute__((amdgpu_waves_per_eu(3, 3))) void k_attn_bwd_dq(
    const uint16_t* __restrict__ q, const uint16_t* __restrict__ k,
    const uint16_t* __restrict__ v, const uint16_t* __restrict__ out,
    const uint16_t* __restrict__ dout, const float* __restrict__ lse,
    uint16_t* __restrict__ dq, float* __restrict__ delta, int nbh, int H,
    int T, int nqb, AttnStrides sq, AttnStrides sk, AttnStrides sv,
    AttnStrides so, AttnStrides sdo, AttnStrides sdq, int64_t lse_stride,
    float scale, float* __restrict__ csq, int64_t cs_ld) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[4 * kTileBytes];
  int bh, slot;
  if (!grid_map(nbh, nqb, bh, slot)) return;  // whole workgroup
  const DqRows w = attn_bwd_dq_body<1>(lds, bh, slot, q, k, v, out, dout, lse,
                                       delta, H, 1, T, nqb, sq, sk, sv, so,
                                       sdo, lse_stride, scale);
  const int tid = threadIdx.x, lane = tid & 63;
  uint16_t* const dqp = dq + w.b * sdq.b + w.h * sdq.h;
  if (!csq) {  // kernel argument: the whole workgroup takes one side
    store_rows(w.Ow, dqp, sdq.t, w.qw0, T, lane);
    return;
  }
  float cs[1][8];
  store_rows_colsum(w.Ow, dqp, sdq.t, w.qw0, T, lane, cs[0]);
  float* const part[1] = {csq + ((int64_t)w.b * nqb + w.qb) * cs_ld +
                          w.h * kD};
  colsum_partial_rows<1>(lds, kRW * 128,
                         __builtin_amdgcn_readfirstlane(tid >> 6), tid, cs,
                         part);
}

// ------------------------------------------------------------- dK, dV

__global__ __launch_bounds__(256)
    __attribute__((amdgpu_waves_per_eu(2, 2))) void k_attn_bwd_dkdv(
    const uint16_t* __restrict__ q, const uint16_t* __restrict__ k,
    const uint16_t* __restrict__ v, const uint16_t* __restrict__ dout,
    const float* __restrict__ lse, const float* __restrict__ delta,
    uint16_t* __restrict__ dk, uint16_t* __restrict__ dv, int nbh, int H,
    int T, int nkb, AttnStrides sq, AttnStrides sk, AttnStrides sv,
    AttnStrides sdo, AttnStrides sdk, AttnStrides sdv, int64_t lse_stride,
    float scale, float* __restrict__ csk, float* __restrict__ csv,
    int64_t cs_ld) {
  __shared__ __attribute__((aligned(16))) unsigned char
      lds[4 * kTileBytes + 2 * 2 * kTile * 4];
  // Q buffers at 0 and kTileBytes, dO buffers behind them, then per buffer
  // 64 floats of -lse log2(e) and 64 of delta
  unsigned char* const ldsQ = lds;
  unsigned char* const ldsD = lds + 2 * kTileBytes;
  float* const ldsLD = reinterpret_cast<float*>(lds + 4 * kTileBytes);

  int bh, kblk;
  if (!grid_map(nbh, nkb, bh, kblk)) return;  // whole workgroup
  const int b = bh / H, h = bh % H;           // first key block first

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int r = lane & 31, hi = lane >> 5;
  const LaneOffs lo = lane_offs(lane);

  const int k0 = kblk * kRB;
  const int kw0 = k0 + wave * kRW;  // the wave's first key
  const int krow = kw0 + r;         // this lane's key
  const bool kok = krow < T;

  const uint16_t* kp = k + b * sk.b + h * sk.h + (int64_t)krow * sk.t;
  const uint16_t* vp = v + b * sv.b + h * sv.h + (int64_t)krow * sv.t;
  const uint16_t* qp = q + b * sq.b + h * sq.h;
  const uint16_t* dop = dout + b * sdo.b + h * sdo.h;
  const float* lsep = lse + (int64_t)bh * lse_stride;
  const float* deltap = delta + (int64_t)bh * T;

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
  // threads 64..127 one delta
  const int srow = tid >> 3, sch = tid & 7;
  u32x4 stQ[2], stD[2];
  float stL = 0.f;
  auto issue = [&](int qt0) {
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
      if (row < T) stL = tid < kTile ? -lsep[row] * kLog2e : deltap[row];
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

  // dK^T, dV^T: lane holds dX[krow][32 nb + (reg&3) + 8 (reg>>2) + 4 hi]
  f32x16 dka[2], dva[2];
#pragma unroll
  for (int nb = 0; nb < 2; ++nb)
#pragma unroll
    for (int i = 0; i < 16; ++i) dka[nb][i] = dva[nb][i] = 0.f;

  issue(t_begin * kTile);
  commit(0);
  __syncthreads();

  for (int t = t_begin; t < t_end; ++t) {
    const int cur = (t - t_begin) & 1;
    const int qt0 = t * kTile;
    const bool more = t + 1 < t_end;
    if (more) issue(qt0 + kTile);

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
  uint16_t* const dkp = dk + b * sdk.b + h * sdk.h;
  uint16_t* const dvp = dv + b * sdv.b + h * sdv.h;
  if (!csk) {  // kernel argument: the whole workgroup takes one side
    store_rows(Ow, dkp, sdk.t, kw0, T, lane);
    store_rows(Ow + kRW * 128, dvp, sdv.t, kw0, T, lane);
    return;
  }
  float cs[2][8];
  store_rows_colsum(Ow, dkp, sdk.t, kw0, T, lane, cs[0]);
  store_rows_colsum(Ow + kRW * 128, dvp, sdv.t, kw0, T, lane, cs[1]);
  const int64_t poff = ((int64_t)b * nkb + kblk) * cs_ld + h * kD;
  float* const part[2] = {csk + poff, csv + poff};
  colsum_partial_rows<2>(lds, 2 * kRW * 128, wave, tid, cs, part);
}

}  // namespace

void hip_attn_bwd_causal_hd64(const void* q, const void* k, const void* v,
                              const void* out, const void* dout,
                              const float* lse, void* dq, void* dk, void* dv,
                              float* delta, int64_t B, int64_t H, int64_t T,
                              const int64_t* qs, const int64_t* ks,
                              const int64_t* vs, const int64_t* os,
                              const int64_t* dos, const int64_t* dqs,
                              const int64_t* dks, const int64_t* dvs,
                              int64_t lse_stride, float scale,
                              float* colsum_partial, void* db, hipStream_t s) {
  const char* op = "attn_bwd_causal_hd64";
  if ((colsum_partial == nullptr) != (db == nullptr))
    throw std::runtime_error(std::string(op) +
                             ": colsum_partial and db go together");
  check_align(colsum_partial, 16, op, "colsum_partial");
  check_attn_bwd(op, q, k, v, out, dout, lse, dq, dk, dv, delta, B, H, H, T,
                 qs, ks, vs, os, dos, dqs, dks, dvs, lse_stride, scale,
                 /*grouped=*/false);
  const int64_t nblk = (T + kRB - 1) / kRB;
  const int64_t nbh = B * H;
  const int64_t C = H * kD;  // a partial row is [dq | dk | dv], C columns each
  const int64_t grid = attn_grid(op, B, H, H, T, nblk);
  auto st3 = strides3;
  auto u16 = [](const void* p) { return static_cast<const uint16_t*>(p); };
  k_attn_bwd_dq<<<dim3((unsigned)grid), dim3(256), 0, s>>>(
      u16(q), u16(k), u16(v), u16(out), u16(dout), lse,
      static_cast<uint16_t*>(dq), delta, (int)nbh, (int)H, (int)T, (int)nblk,
      st3(qs), st3(ks), st3(vs), st3(os), st3(dos), st3(dqs), lse_stride,
      scale, colsum_partial, 3 * C);
  HIP_CHECK(hipGetLastError());
  k_attn_bwd_dkdv<<<dim3((unsigned)grid), dim3(256), 0, s>>>(
      u16(q), u16(k), u16(v), u16(dout), lse, delta,
      static_cast<uint16_t*>(dk), static_cast<uint16_t*>(dv), (int)nbh, (int)H,
      (int)T, (int)nblk, st3(qs), st3(ks), st3(vs), st3(dos), st3(dks),
      st3(dvs), lse_stride, scale, colsum_partial ? colsum_partial + C : nullptr,
      colsum_partial ? colsum_partial + 2 * C : nullptr, 3 * C);
  HIP_CHECK(hipGetLastError());
  if (colsum_partial)
    hip_colsum_reduce(colsum_partial, B * nblk, 3 * C, 3 * C, db, nullptr,
                      nullptr, s);
}

int64_t hip_attn_bwd_colsum_floats(int64_t B, int64_t H, int64_t T) {
  if (B <= 0 || H <= 0 || T <= 0)
    throw std::runtime_error("attn_bwd_causal_hd64: empty problem");
  return B * ((T + kRB - 1) / kRB) * 3 * H * kD;
}

}  // namespace shamd
