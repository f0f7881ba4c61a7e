// The causal bf16 attention forward, once: the body of k_attn_fwd_causal_hd64
// (attn_kernels.hip), k_gqa_fwd_hd64 (gqa_attn_kernels.hip) and
// k_gqa_fwd_hd128 (gqa_attn_hd128_kernels.hip), and the checks of their
// launchers.  Flash style: the T x T score matrix lives only in registers,
// one KV tile at a time, with an online softmax.  fp32 accumulation, bf16 in
// and out, no dropout, no bias, top-left aligned causal mask (Tq == Tk).  Each
// kernel file's header keeps its own plan: mapping, resources, measurements.
//
// Mechanics, for head dim D (64 or 128) and HW query heads per workgroup:
//   * A wave owns 32 query rows of one query head.  workgroup = 4 waves = HW
//     heads of one kv group x 128 / HW consecutive positions; G / HW
//     workgroups (head halves) per kv head and position block.  MHA is
//     HW = 1, G = 1: one head, 128 rows.  KV tile = 64 keys, staged once for
//     the HW heads.
//   * Q stays in registers (D / 16 x bf16x8 per lane) for the whole block.
//   * K and V tiles are double-buffered in LDS, 2 x 2 x 64 x 2 D bytes.  The
//     next tile's global loads are issued before the current tile's MFMAs
//     and written to LDS after them; one barrier per tile.  A tile is D / 64
//     halves of [64 rows][128 B], one per 64 columns, 8 KB apart:
//       - K: 16-byte chunk c of key row r sits at chunk c ^ ((r >> 1) & 7),
//         so the ds_read_b128 of a 16-lane group (16 consecutive keys, one
//         chunk) touches 16 different 16-byte slots of the 256-byte bank
//         line.
//       - V: the two 64-byte halves of rows with bit 1 set are swapped, so
//         the 4 rows x 64 B that one 32-lane half fetches with
//         ds_read_b64_tr_b16 cover the bank line once.
//     Every K read of an MFMA step and every transposed V read lies inside
//     one half, so head dim 128 sees the bank pattern of head dim 64.
//   * S^T = mfma_32x32x16(K, Q): a lane owns one query (lane & 31) and, per
//     32-key block, the 16 keys (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).
//     Row max and row sum are per-lane loops plus one exchange between the
//     two lane halves; alpha and l need no cross-lane traffic.
//   * Registers 8s .. 8s+7 of S^T, converted pairwise to bf16, are the B
//     operand of k-step s of O^T += mfma_32x32x16(V^T, P^T): the transposed V
//     read delivers V in exactly that permuted key order, so P never moves
//     between lanes or through LDS.
//   * exp2 with scale * log2(e) folded into one fma per score.
//   * KV tiles wholly above a wave's rows are skipped by that wave; only the
//     tile that crosses the diagonal is masked.  Both conditions are
//     wave-uniform, on the wave's own first row qw0.
//   * O is staged through the (then idle) LDS so that every global store is
//     16 bytes of a whole row of the contiguous (B, T, Hq, D) output.  lse is
//     (B, Hq, lse_stride >= T).
//   * Grid: all workgroups of one (b, kv head) are consecutive on one XCD
//     (blockIdx % 8), heaviest (last) position block first, the head halves
//     adjacent, so K/V are re-read from that XCD's L2.
//
// Every T is bounds-checked: query rows and key rows at or past T are read
// as zeros (never from memory) and never stored.
#pragma once

#include "attn_tile.h"

namespace shamd {
namespace {

// byte offset of 16-byte chunk `ch` (0..7) of key row `row` inside one
// 64-column half of a K tile
__device__ __forceinline__ int k_off(int row, int ch) {
  return row * 128 + ((ch ^ ((row >> 1) & 7)) << 4);
}
// the same for a V tile
__device__ __forceinline__ int v_off(int row, int ch) {
  return row * 128 + ((ch ^ (((row >> 1) & 1) << 2)) << 4);
}

__device__ __forceinline__ uint4 load16_or_zero(const uint16_t* p, bool ok) {
  uint4 z = make_uint4(0, 0, 0, 0);
  return ok ? *reinterpret_cast<const uint4*>(p) : z;
}

// the other lane half's value (lane ^ 32)
__device__ __forceinline__ float other_half(float x) {
  return __shfl_xor(x, 32, 64);
}

constexpr int kHalfBytes = kTile * 128;  // one 64-column half of a tile

// Thread (staging) or lane (epilogue) i covers 16-byte chunk i & 7 of column
// half `half` of row `row`, and the rows a fixed step below it.  Head dim
// 128: 16 consecutive lanes cover two rows of one half (256 contiguous bytes
// before the swizzle), not the two halves of one row, which sit on the same
// banks.
template <int D>
__device__ __forceinline__ void chunk_row(int i, int& row, int& half) {
  if constexpr (D == 128) {
    row = 2 * (i >> 5) + ((i >> 3) & 1);
    half = (i >> 4) & 1;
  } else {
    row = i >> 3;
    half = 0;
  }
}

// nbk = B * Hkv, nqb = position blocks of 128 / HW rows.  The body declares
// the LDS itself and its pointer parameters carry no __restrict__ (the
// kernels' do): handed the LDS as a pointer, or with __restrict__ repeated
// here, the head-dim-64 kernels compile to 9 spilled VGPRs.
template <int D, int HW>
__device__ __forceinline__ void attn_fwd_body(
    const uint16_t* q, const uint16_t* k, const uint16_t* v, uint16_t* out,
    float* lse, int nbk, int Hkv, int G, int T, int nqb, AttnStrides sq,
    AttnStrides sk, AttnStrides sv, int64_t lse_stride, float scale_log2e) {
  static_assert(D == 64 || D == 128);
  constexpr int kWPH = kWaves / HW;   // waves per head
  constexpr int kPB = kRW * kWPH;     // positions per workgroup
  constexpr int kTileBytes = (D / 64) * kHalfBytes;
  // K buffers at 0 and kTileBytes, V buffers behind them
  __shared__ __attribute__((aligned(16))) unsigned char lds[4 * kTileBytes];
  unsigned char* const ldsK = lds;
  unsigned char* const ldsV = lds + 2 * kTileBytes;

  // blockIdx -> (kv head, position block, head half)
  const int nhalf = G / HW;
  int bk, sl;
  if (!grid_map(nbk, nqb * nhalf, bk, sl)) return;  // whole workgroup
  const int qb = nqb - 1 - sl / nhalf;
  const int half = sl % nhalf;
  const int b = bk / Hkv, kvh = bk % Hkv;

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int r = lane & 31, hi = lane >> 5;

  const int Hq = Hkv * G;
  const int h = G * kvh + HW * half + wave / kWPH;  // the wave's query head
  const int q0 = qb * kPB;
  const int qw0 = q0 + (wave % kWPH) * kRW;  // the wave's first query row
  const int qrow = qw0 + r;                  // this lane's query row

  const uint16_t* qp = q + b * sq.b + h * sq.h;
  const uint16_t* kp = k + b * sk.b + kvh * sk.h;
  const uint16_t* vp = v + b * sv.b + kvh * sv.h;

  // Q fragment: B operand of mfma(K, Q); lane holds Q[qrow][16 ks + 8 hi + j]
  bf16x8 qf[D / 16];
#pragma unroll
  for (int ks = 0; ks < D / 16; ++ks)
    qf[ks] = __builtin_bit_cast(
        bf16x8, load16_or_zero(qp + (int64_t)qrow * sq.t + 16 * ks + 8 * hi,
                               qrow < T));

  // staging: thread covers chunk sch of half shalf of keys skey + kStep i,
  // for K and for V
  constexpr int kStN = D / 32, kStep = kTile / kStN;
  int skey, shalf;
  chunk_row<D>(tid, skey, shalf);
  const int sch = tid & 7, scol = 64 * shalf + 8 * sch;
  uint4 stK[kStN], stV[kStN];
  auto issue = [&](int kv0) {
#pragma unroll
    for (int i = 0; i < kStN; ++i) {
      int key = kv0 + skey + kStep * i;
      bool ok = key < T;
      stK[i] = load16_or_zero(kp + (int64_t)key * sk.t + scol, ok);
      stV[i] = load16_or_zero(vp + (int64_t)key * sv.t + scol, ok);
    }
  };
  auto commit = [&](int buf) {
#pragma unroll
    for (int i = 0; i < kStN; ++i) {
      int row = skey + kStep * i;
      int base = buf * kTileBytes + shalf * kHalfBytes;
      *reinterpret_cast<uint4*>(ldsK + base + k_off(row, sch)) = stK[i];
      *reinterpret_cast<uint4*>(ldsV + base + v_off(row, sch)) = stV[i];
    }
  };

  const int kv_end = min(T, q0 + kPB);              // keys this block can see
  const int ntiles = (kv_end + kTile - 1) / kTile;  // >= 1

  // O^T: lane holds O[qrow][32 nb + (reg&3) + 8 (reg>>2) + 4 hi]
  f32x16 o[D / 32];
#pragma unroll
  for (int nb = 0; nb < D / 32; ++nb)
#pragma unroll
    for (int i = 0; i < 16; ++i) o[nb][i] = 0.f;
  float m = -INFINITY;  // running max of score * scale * log2(e)
  float l = 0.f;        // this lane half's share of the running sum

  // transposed-read address of V inside a half, without the (s, jj, nb) part:
  // 16-lane group g reads rows k0 .. k0+3, columns 32 nb + 16 (g & 1) + 0..15;
  // lane 4 qq + p of the group supplies row qq, columns 4 p .. 4 p + 3
  const int grp = lane >> 4, gi = lane & 15;
  const int tr_q = gi >> 2, tr_p = gi & 3;

  issue(0);
  commit(0);
  __syncthreads();

  for (int t = 0; t < ntiles; ++t) {
    const int cur = t & 1;
    const int kv0 = t * kTile;
    const bool more = t + 1 < ntiles;
    if (more) issue(kv0 + kTile);

    if (kv0 <= qw0 + kRW - 1) {  // wave-uniform: the tile has visible keys
      const unsigned char* Kt = ldsK + cur * kTileBytes;
      const unsigned char* Vt = ldsV + cur * kTileBytes;

      // S^T = K Q^T: s[kb][reg] = score(qrow, kv0 + 32 kb + keymap(reg, hi));
      // k-step ks reads chunk 2 (ks & 3) + hi of half ks >> 2
      f32x16 s[2];
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
        for (int i = 0; i < 16; ++i) s[kb][i] = 0.f;
#pragma unroll
        for (int ks = 0; ks < D / 16; ++ks) {
          uint4 kk = *reinterpret_cast<const uint4*>(
              Kt + (ks >> 2) * kHalfBytes +
              k_off(32 * kb + r, 2 * (ks & 3) + hi));
          s[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              __builtin_bit_cast(bf16x8, kk), qf[ks], s[kb], 0, 0, 0);
        }
      }

      if (kv0 + kTile - 1 > qw0) {  // wave-uniform: the tile crosses the diagonal
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            int key = kv0 + 32 * kb + (i & 3) + 8 * (i >> 2) + 4 * hi;
            if (key > qrow) s[kb][i] = -INFINITY;
          }
      }

      // every row has a visible key in every tile its wave processes, so the
      // new max is finite and exp2(-inf - m) is a clean 0
      float mx = s[0][0];
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int i = 0; i < 16; ++i) mx = fmaxf(mx, s[kb][i]);
      mx = fmaxf(mx, other_half(mx));
      const float mn = fmaxf(m, mx * scale_log2e);
      const float alpha = __builtin_amdgcn_exp2f(m - mn);
      m = mn;

      float rs = 0.f;
      bf16x8 pf[4];  // P^T fragments: k-step ss = 2 kb + half of the regs
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          float p = __builtin_amdgcn_exp2f(
              __builtin_fmaf(s[kb][i], scale_log2e, -mn));
          rs += p;
          pf[2 * kb + (i >> 3)][i & 7] = (__bf16)p;
        }
      l = l * alpha + rs;
#pragma unroll
      for (int nb = 0; nb < D / 32; ++nb)
#pragma unroll
        for (int i = 0; i < 16; ++i) o[nb][i] *= alpha;

      // O^T += V^T P^T; element j of the fragment of k-step ss is key
      // 16 ss + 8 (j >> 2) + 4 hi + (j & 3), the order P's registers have;
      // column block nb is chunks 4 (nb & 1) .. + 3 of half nb >> 1
#pragma unroll
      for (int nb = 0; nb < D / 32; ++nb) {
#pragma unroll
        for (int ss = 0; ss < 4; ++ss) {
          bf16x8 vf;
#pragma unroll
          for (int jj = 0; jj < 2; ++jj) {
            int row = 16 * ss + 8 * jj + 4 * (grp >> 1) + tr_q;
            int ch = 4 * (nb & 1) + 2 * (grp & 1) + (tr_p >> 1);
            auto* a = reinterpret_cast<
                __attribute__((address_space(3))) s16x4*>(
                (uintptr_t)(Vt + (nb >> 1) * kHalfBytes + v_off(row, ch) +
                            8 * (tr_p & 1)));
            s16x4 tr = __builtin_amdgcn_ds_read_tr16_b64_v4i16(a);
            bf16x4 tb = __builtin_bit_cast(bf16x4, tr);
#pragma unroll
            for (int e = 0; e < 4; ++e) vf[4 * jj + e] = tb[e];
          }
          o[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf[ss], o[nb], 0,
                                                          0, 0);
        }
      }
    }

    if (more) commit(cur ^ 1);
    __syncthreads();
  }

  // ---- epilogue: normalise, lse, O through LDS to whole-row stores
  l += other_half(l);
  const float inv = 1.f / l;
  if (hi == 0 && qrow < T)
    lse[((int64_t)b * Hq + h) * lse_stride + qrow] =
        (m + __builtin_amdgcn_logf(l)) * 0.6931471805599453f;

  // the loop's last barrier is behind every wave: K/V tiles are dead.  Each
  // wave owns D / 64 halves of [32 rows][8 chunks of 16 B], chunks swizzled
  // like K.
  constexpr int kOHalf = kRW * 128;
  unsigned char* const Ow = lds + wave * ((D / 64) * kOHalf);
#pragma unroll
  for (int nb = 0; nb < D / 32; ++nb)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float f[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) f[e] = o[nb][4 * g + e] * inv;
      // d = 32 nb + 8 g + 4 hi + e: half nb >> 1, chunk 4 (nb & 1) + g, its
      // half hi
      *reinterpret_cast<uint2*>(Ow + (nb >> 1) * kOHalf +
                                k_off(r, 4 * (nb & 1) + g) + 8 * hi) = pack4(f);
    }
  __syncthreads();
  uint16_t* op = out + ((int64_t)b * T * Hq + h) * D;
  // a pass stores 512 / D whole rows
  constexpr int kPassRows = 512 / D;
  int erow, ehalf;
  chunk_row<D>(lane, erow, ehalf);
  const int ech = lane & 7;
#pragma unroll
  for (int pass = 0; pass < kRW / kPassRows; ++pass) {
    int row = pass * kPassRows + erow;
    uint4 val = *reinterpret_cast<const uint4*>(Ow + ehalf * kOHalf +
                                                k_off(row, ech));
    int qr = qw0 + row;
    if (qr < T)
      *reinterpret_cast<uint4*>(op + (int64_t)qr * Hq * D + 64 * ehalf +
                                8 * ech) = val;
  }
}

// ------------------------------------------------------------------ host

struct FwdLaunch {
  int64_t G, nbk, nqb, grid;
  int HW;  // min(G, 4)
};

// Every check of a forward launcher, and the grid it launches.  The MHA op
// passes Hq == Hkv and grouped = false.
inline FwdLaunch check_attn_fwd(const char* op, const void* q, const void* k,
                                const void* v, const void* out,
                                const float* lse, int64_t B, int64_t Hq,
                                int64_t Hkv, int64_t T, const int64_t* qs,
                                const int64_t* ks, const int64_t* vs,
                                int64_t lse_stride, float scale, bool grouped) {
  FwdLaunch p;
  p.G = check_attn_problem(op, B, Hq, Hkv, T, lse_stride, scale, grouped);
  if (!q || !k || !v || !out || !lse)
    throw std::runtime_error(std::string(op) + ": null pointer");
  check_align(q, 16, op, "q");
  check_align(k, 16, op, "k");
  check_align(v, 16, op, "v");
  check_align(out, 16, op, "out");
  check_align(lse, 4, op, "lse");
  check_attn_strides(op, {qs, ks, vs});
  p.HW = p.G < 4 ? (int)p.G : 4;
  const int64_t pb = kRB / p.HW;
  p.nqb = (T + pb - 1) / pb;
  p.nbk = B * Hkv;
  p.grid = attn_grid(op, B, Hq, Hkv, T, p.nqb * (p.G / p.HW));
  return p;
}

}  // namespace
}  // namespace shamd
