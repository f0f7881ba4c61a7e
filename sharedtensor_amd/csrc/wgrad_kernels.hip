// Split-K bf16 weight gradient of a Linear: dW[N, K] = dY[M, N]^T X[M, K],
// fp32 MFMA accumulation, bf16 out.  M is tokens (the reduction), N and K are
// features.  Written for the regime the GPT-2 layers are in: a small output
// (768 x 768 .. 768 x 3072) under a 65536-long reduction.
//
// Plan (tests/test_wgrad_resource_usage.py holds the kernels to it):
//   * workgroup = one output tile of (128 NP) x (128 KP) and a contiguous
//     range of 64-token steps; a wave owns 64 x 64 of the tile as 2 x 2
//     accumulators of mfma_f32_32x32x16_bf16.
//   * both operands are token-major, so per step the workgroup stages
//     [64 tokens][128 features] panels (256-byte rows) of dY and of X in LDS
//     with 16-byte loads and stores, and every MFMA fragment (8 tokens of one
//     feature) comes from two ds_read_b64_tr_b16.  16-byte chunk ch of token
//     row r sits at chunk ch ^ (((r & 3) << 2) | ((r >> 2) & 3)): the 4 rows
//     x 64 B that a 32-lane half fetches cover the 256-byte bank line once,
//     and the 8 lanes of a ds_write_b128 group hit 8 different slots.
//   * element j of lane half h of a fragment is token 8 (j >> 2) + 4 h +
//     (j & 3) of the 16-token MFMA step, for A and for B alike: the sum over
//     tokens does not care about their order as long as both agree.
//   * the next step's global loads are issued before the current step's
//     MFMAs and written to LDS after them.  NBUF = 2: two LDS stages, one
//     barrier per step.  NBUF = 1: one stage, two barriers per step, half the
//     LDS, so more workgroups per CU.
//   * workgroup ids are remapped (bijectively, any grid size) so that the ids
//     sharing an XCD are consecutive (split, tile) pairs: tiles of one split
//     read the same token range from that XCD's L2.
//   * split == 1: the tile is stored as bf16.  Otherwise it goes as fp32 to
//     ws[split][N][K] and k_wgrad_reduce sums the splits in index order and
//     rounds once: no atomics, bit-identical from call to call.  A split with
//     no steps stores zeros.
//
// N and K are multiples of the tile and M of 64 (the launcher checks), so the
// kernels need no bounds tests: every access is inside the tile's rows.
#include <hip/hip_runtime.h>

#include "device_util.h"
#include "hip_api.h"

namespace shamd {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

constexpr int kStep = 64;              // tokens per step
constexpr int kPanelCols = 128;        // features per LDS panel
constexpr int kPanelBytes = kStep * kPanelCols * 2;
constexpr int kXcd = 8;

// byte offset of 16-byte chunk `ch` (0..15) of token row `row` in a panel
__device__ __forceinline__ int p_off(int row, int ch) {
  return row * 256 + ((ch ^ (((row & 3) << 2) | ((row >> 2) & 3))) << 4);
}

template <int NP, int KP, int NBUF>
__global__ __launch_bounds__(256 * NP * KP)
    __attribute__((amdgpu_waves_per_eu(NBUF == 1 ? 3 : 2,
                                       NBUF == 1 ? 3 : 2))) void k_wgrad(
    const uint16_t* __restrict__ dy, const uint16_t* __restrict__ x,
    uint16_t* __restrict__ dw, float* __restrict__ ws, int steps, int N, int K,
    int64_t ldy, int64_t ldx, int64_t ldw, int split, int tiles_k, int tiles) {
  constexpr int NT = 256 * NP * KP;
  constexpr int kStage = (NP + KP) * kPanelBytes;
  constexpr int kChunks = (NP + KP) * 1024 / NT;  // 16-byte chunks per thread
  static_assert((NP + KP) * 1024 % NT == 0 && 1024 % NT == 0, "staging map");
  __shared__ __attribute__((aligned(16))) unsigned char lds[NBUF * kStage];

  // block id -> (split, tile): ids that share an XCD become consecutive
  const int nwg = gridDim.x, orig = blockIdx.x;
  const int xcd = orig % kXcd, q8 = nwg / kXcd, r8 = nwg % kXcd;
  const int wg =
      (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) +
      orig / kXcd;
  const int sp = wg / tiles, tile = wg % tiles;
  const int n0 = (tile / tiles_k) * (kPanelCols * NP);
  const int k0 = (tile % tiles_k) * (kPanelCols * KP);

  // this split's steps: the first `steps % split` splits get one more
  const int sq = steps / split, sr = steps % split;
  const int s_begin = sp * sq + min(sp, sr);
  const int s_count = sq + (sp < sr ? 1 : 0);

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int wn = wave / (2 * KP), wk = wave % (2 * KP);  // 64 x 64 sub-tile

  // staging: chunk c = tid + i NT of the stage; 1024 chunks per panel, 16 per
  // token row.  The panel of chunk i is the same for every thread.
  const int srow = (tid & 1023) >> 4, sch = tid & 15;
  // named registers, not an array: indexed through the two lambdas, an
  // array of uint4 went to scratch
  constexpr int kCA = NP * 1024 / NT, kCB = KP * 1024 / NT;
  static_assert(kCA + kCB == kChunks && kCA <= 4 && kCB <= 4, "staging map");
  uint4 sa0, sa1, sa2, sa3, sb0, sb1, sb2, sb3;
  const int64_t tok0 = (int64_t)s_begin * kStep + srow;
  const uint16_t* const pa = dy + tok0 * ldy + n0 + 8 * sch;
  const uint16_t* const pb = x + tok0 * ldx + k0 + 8 * sch;
  // chunk i of an operand: panel (i NT) >> 10, token row srow + 16-row group
  // ((i NT) & 1023) >> 4
#define SHAMD_WG_LOAD(reg, i, p, ld, cnt)                                    \
  if constexpr ((i) < (cnt))                                                 \
    reg = *reinterpret_cast<const uint4*>(                                   \
        (p) + (t + ((((i) * NT) & 1023) >> 4)) * (ld) +                      \
        (((i) * NT) >> 10) * kPanelCols)
#define SHAMD_WG_STORE(reg, i, p0, cnt)                                      \
  if constexpr ((i) < (cnt))                                                 \
    *reinterpret_cast<uint4*>(                                               \
        base + ((p0) + (((i) * NT) >> 10)) * kPanelBytes +                   \
        p_off(srow + ((((i) * NT) & 1023) >> 4), sch)) = reg
  auto issue = [&](int step) {
    const int64_t t = (int64_t)step * kStep;
    SHAMD_WG_LOAD(sa0, 0, pa, ldy, kCA);
    SHAMD_WG_LOAD(sa1, 1, pa, ldy, kCA);
    SHAMD_WG_LOAD(sa2, 2, pa, ldy, kCA);
    SHAMD_WG_LOAD(sa3, 3, pa, ldy, kCA);
    SHAMD_WG_LOAD(sb0, 0, pb, ldx, kCB);
    SHAMD_WG_LOAD(sb1, 1, pb, ldx, kCB);
    SHAMD_WG_LOAD(sb2, 2, pb, ldx, kCB);
    SHAMD_WG_LOAD(sb3, 3, pb, ldx, kCB);
  };
  auto commit = [&](int buf) {
    unsigned char* const base = lds + buf * kStage;
    SHAMD_WG_STORE(sa0, 0, 0, kCA);
    SHAMD_WG_STORE(sa1, 1, 0, kCA);
    SHAMD_WG_STORE(sa2, 2, 0, kCA);
    SHAMD_WG_STORE(sa3, 3, 0, kCA);
    SHAMD_WG_STORE(sb0, 0, NP, kCB);
    SHAMD_WG_STORE(sb1, 1, NP, kCB);
    SHAMD_WG_STORE(sb2, 2, NP, kCB);
    SHAMD_WG_STORE(sb3, 3, NP, kCB);
  };
#undef SHAMD_WG_LOAD
#undef SHAMD_WG_STORE

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  // transposed read: the 16-lane group g = lane >> 4 fetches token rows
  // t0 .. t0+3 (t0 = 16 ss + 8 jj + 4 (g >> 1)) x 16 features; lane 4 qq + p
  // of the group supplies row qq, features 4 p .. 4 p + 3, and receives
  // feature (lane & 15) of the four rows.
  const int grp = lane >> 4, gi = lane & 15;
  const int tr_q = gi >> 2, tr_p = gi & 3, hi = grp >> 1;
  // feature chunk inside the panel, without the 32-column block part
  const int a_ch = (wn & 1) * 8 + 2 * (grp & 1) + (tr_p >> 1);
  const int b_ch = (wk & 1) * 8 + 2 * (grp & 1) + (tr_p >> 1);
  const int a_panel = (wn >> 1) * kPanelBytes;
  const int b_panel = (NP + (wk >> 1)) * kPanelBytes;

  auto frag = [&](const unsigned char* panel, int ch, int ss) -> bf16x8 {
    bf16x8 f;
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
      const int row = 16 * ss + 8 * jj + 4 * hi + tr_q;
      auto* a = reinterpret_cast<__attribute__((address_space(3))) s16x4*>(
          (uintptr_t)(panel + p_off(row, ch) + 8 * (tr_p & 1)));
      s16x4 tr = __builtin_amdgcn_ds_read_tr16_b64_v4i16(a);
      bf16x4 tb = __builtin_bit_cast(bf16x4, tr);
#pragma unroll
      for (int e = 0; e < 4; ++e) f[4 * jj + e] = tb[e];
    }
    return f;
  };
  auto compute = [&](int buf) {
    const unsigned char* A = lds + buf * kStage + a_panel;
    const unsigned char* B = lds + buf * kStage + b_panel;
#pragma unroll
    for (int ss = 0; ss < 4; ++ss) {
      bf16x8 a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        a[i] = frag(A, a_ch + 4 * i, ss);
        b[i] = frag(B, b_ch + 4 * i, ss);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              a[i], b[j], acc[i][j], 0, 0, 0);
    }
  };

  // s_count is the same for the whole workgroup: every barrier below is
  // reached by all of its waves or by none
  if (s_count > 0) {
    issue(0);
    commit(0);
    __syncthreads();
    for (int t = 0; t < s_count; ++t) {
      const bool more = t + 1 < s_count;
      if (more) issue(t + 1);
      if constexpr (NBUF == 2) {
        compute(t & 1);
        if (more) commit((t & 1) ^ 1);
        __syncthreads();
      } else {
        compute(0);
        __syncthreads();
        if (more) commit(0);
        __syncthreads();
      }
    }
  }

  // ---- epilogue: acc[i][j][reg] is row (reg & 3) + 8 (reg >> 2) + 4 (lane
  // >> 5), column lane & 31 of its 32 x 32 block
  const int row0 = n0 + wn * 64 + 4 * (lane >> 5);
  const int col0 = k0 + wk * 64 + (lane & 31);
  if (split == 1) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int row = row0 + 32 * i + (e & 3) + 8 * (e >> 2);
          dw[(int64_t)row * ldw + col0 + 32 * j] = f32_to_bf16(acc[i][j][e]);
        }
  } else {
    float* out = ws + (int64_t)sp * N * K;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int row = row0 + 32 * i + (e & 3) + 8 * (e >> 2);
          out[(int64_t)row * K + col0 + 32 * j] = acc[i][j][e];
        }
  }
}

// The 256 x 256 tile: the same split-K scheme, panels, swizzle, transposed
// fragment reads and XCD remap as k_wgrad, with a larger register tile per
// wave so that every fragment read from LDS feeds more MFMAs
// (tests/test_wgrad256_resource_usage.py holds it to this plan).
//   * a stage is 2 dY panels + 2 X panels, 64 KB; two stages, one barrier per
//     step, one workgroup per CU.
//   * 4 waves, one per SIMD; a wave owns 128 x 128 as 4 x 4 accumulators
//     (256 registers, which the compiler keeps in AGPRs): 8 fragments per 16
//     MFMAs against 4 per 4 in k_wgrad.
//   * the fragments of the next 16-token step are read while the MFMAs of the
//     current one issue.
//   * CS: the workgroups of K-tile 0 also sum, in fp32, the dY values they
//     stage (a thread always stages the same 8 feature columns of either dY
//     panel), combine the NT / 16 threads of a column through LDS in a fixed
//     order, and store the 256 column sums: as bf16 to db when split == 1,
//     else as fp32 to wsb[split][N], which k_wgrad_reduce adds in split order.
//     A split with no steps stores zeros.
template <bool CS>
__global__ __launch_bounds__(256)
    __attribute__((amdgpu_waves_per_eu(1, 1))) void k_wgrad256(
    const uint16_t* __restrict__ dy, const uint16_t* __restrict__ x,
    uint16_t* __restrict__ dw, float* __restrict__ ws,
    uint16_t* __restrict__ db, float* __restrict__ wsb, int steps, int N,
    int K, int64_t ldy, int64_t ldx, int64_t ldw, int split, int tiles_k,
    int tiles) {
  constexpr int NW = 4, NT = 64 * NW;
  constexpr int kStage = 4 * kPanelBytes;
  constexpr int kC = 2 * 1024 / NT;  // 16-byte chunks per thread and operand
  constexpr int BJ = 16 / NW;        // 32-column blocks of a wave's X range
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * kStage];

  // block id -> (split, tile): ids that share an XCD become consecutive
  const int nwg = gridDim.x, orig = blockIdx.x;
  const int xcd = orig % kXcd, q8 = nwg / kXcd, r8 = nwg % kXcd;
  const int wg =
      (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) +
      orig / kXcd;
  const int sp = wg / tiles, tile = wg % tiles;
  const int n0 = (tile / tiles_k) * 256;
  const int k0 = (tile % tiles_k) * 256;
  const bool colsum = CS && k0 == 0;  // the same for the whole workgroup

  const int sq = steps / split, sr = steps % split;
  const int s_begin = sp * sq + min(sp, sr);
  const int s_count = sq + (sp < sr ? 1 : 0);

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int wn = wave / (NW / 2), wk = wave % (NW / 2);

  // staging as in k_wgrad: chunk c = tid + i NT of an operand's two panels
  const int srow = tid >> 4, sch = tid & 15;
  uint4 sa0, sa1, sa2, sa3, sa4, sa5, sa6, sa7;
  uint4 sb0, sb1, sb2, sb3, sb4, sb5, sb6, sb7;
  float c0[8], c1[8];  // column sums of dY panel 0 and 1
#pragma unroll
  for (int e = 0; e < 8; ++e) c0[e] = c1[e] = 0.f;
  // a global address is a workgroup-uniform 64-bit part (scalar registers)
  // plus a 32-bit byte offset per thread: 16 pointers per thread would not
  // fit beside the accumulators (the launcher bounds the strides)
  const char* const ga =
      reinterpret_cast<const char*>(dy + (int64_t)s_begin * kStep * ldy + n0);
  const char* const gb =
      reinterpret_cast<const char*>(x + (int64_t)s_begin * kStep * ldx + k0);
  const uint32_t va = 2u * (uint32_t)(srow * (int)ldy + 8 * sch);
  const uint32_t vb = 2u * (uint32_t)(srow * (int)ldx + 8 * sch);
#define SHAMD_WG_LOAD(reg, i, g, v, ld)                                      \
  if constexpr ((i) < kC)                                                    \
    reg = *reinterpret_cast<const uint4*>(                                   \
        (g) + 2 * ((t + ((((i) * NT) & 1023) >> 4)) * (ld) +                 \
                   (((i) * NT) >> 10) * kPanelCols) + (uint64_t)(v))
#define SHAMD_WG_STORE(reg, i, p0)                                           \
  if constexpr ((i) < kC)                                                    \
    *reinterpret_cast<uint4*>(                                               \
        base + ((p0) + (((i) * NT) >> 10)) * kPanelBytes +                   \
        p_off(srow + ((((i) * NT) & 1023) >> 4), sch)) = reg
#define SHAMD_WG_CSUM(reg, i)                                                \
  if constexpr ((i) < kC) {                                                  \
    float v[8];                                                              \
    unpack8(reg, v);                                                         \
    _Pragma("unroll") for (int e = 0; e < 8; ++e) {                          \
      if constexpr ((((i) * NT) >> 10) != 0) c1[e] += v[e];                         \
      else c0[e] += v[e];                                                    \
    }                                                                        \
  }
  auto issue = [&](int step) {
    const int64_t t = (int64_t)step * kStep;
    SHAMD_WG_LOAD(sa0, 0, ga, va, ldy);
    SHAMD_WG_LOAD(sa1, 1, ga, va, ldy);
    SHAMD_WG_LOAD(sa2, 2, ga, va, ldy);
    SHAMD_WG_LOAD(sa3, 3, ga, va, ldy);
    SHAMD_WG_LOAD(sa4, 4, ga, va, ldy);
    SHAMD_WG_LOAD(sa5, 5, ga, va, ldy);
    SHAMD_WG_LOAD(sa6, 6, ga, va, ldy);
    SHAMD_WG_LOAD(sa7, 7, ga, va, ldy);
    SHAMD_WG_LOAD(sb0, 0, gb, vb, ldx);
    SHAMD_WG_LOAD(sb1, 1, gb, vb, ldx);
    SHAMD_WG_LOAD(sb2, 2, gb, vb, ldx);
    SHAMD_WG_LOAD(sb3, 3, gb, vb, ldx);
    SHAMD_WG_LOAD(sb4, 4, gb, vb, ldx);
    SHAMD_WG_LOAD(sb5, 5, gb, vb, ldx);
    SHAMD_WG_LOAD(sb6, 6, gb, vb, ldx);
    SHAMD_WG_LOAD(sb7, 7, gb, vb, ldx);
  };
  auto commit = [&](int buf) {
    unsigned char* const base = lds + buf * kStage;
    SHAMD_WG_STORE(sa0, 0, 0);
    SHAMD_WG_STORE(sa1, 1, 0);
    SHAMD_WG_STORE(sa2, 2, 0);
    SHAMD_WG_STORE(sa3, 3, 0);
    SHAMD_WG_STORE(sa4, 4, 0);
    SHAMD_WG_STORE(sa5, 5, 0);
    SHAMD_WG_STORE(sa6, 6, 0);
    SHAMD_WG_STORE(sa7, 7, 0);
    SHAMD_WG_STORE(sb0, 0, 2);
    SHAMD_WG_STORE(sb1, 1, 2);
    SHAMD_WG_STORE(sb2, 2, 2);
    SHAMD_WG_STORE(sb3, 3, 2);
    SHAMD_WG_STORE(sb4, 4, 2);
    SHAMD_WG_STORE(sb5, 5, 2);
    SHAMD_WG_STORE(sb6, 6, 2);
    SHAMD_WG_STORE(sb7, 7, 2);
    if constexpr (CS) {
      if (colsum) {
        SHAMD_WG_CSUM(sa0, 0);
        SHAMD_WG_CSUM(sa1, 1);
        SHAMD_WG_CSUM(sa2, 2);
        SHAMD_WG_CSUM(sa3, 3);
        SHAMD_WG_CSUM(sa4, 4);
        SHAMD_WG_CSUM(sa5, 5);
        SHAMD_WG_CSUM(sa6, 6);
        SHAMD_WG_CSUM(sa7, 7);
      }
    }
  };
#undef SHAMD_WG_LOAD
#undef SHAMD_WG_STORE
#undef SHAMD_WG_CSUM

  f32x16 acc[4][BJ];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < BJ; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  // fragment addressing as in k_wgrad; a wave's dY range is one whole panel
  // and so is its X range
  const int grp = lane >> 4, gi = lane & 15;
  const int tr_q = gi >> 2, tr_p = gi & 3, hi = grp >> 1;
  const int a_ch = 2 * (grp & 1) + (tr_p >> 1);
  const int b_ch = a_ch;
  const int a_panel = wn * kPanelBytes;
  const int b_panel = (2 + wk) * kPanelBytes;

  auto frag = [&](const unsigned char* panel, int ch, int ss) -> bf16x8 {
    bf16x8 f;
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
      const int row = 16 * ss + 8 * jj + 4 * hi + tr_q;
      auto* a = reinterpret_cast<__attribute__((address_space(3))) s16x4*>(
          (uintptr_t)(panel + p_off(row, ch) + 8 * (tr_p & 1)));
      s16x4 tr = __builtin_amdgcn_ds_read_tr16_b64_v4i16(a);
      bf16x4 tb = __builtin_bit_cast(bf16x4, tr);
#pragma unroll
      for (int e = 0; e < 4; ++e) f[4 * jj + e] = tb[e];
    }
    return f;
  };
  auto compute = [&](int buf) {
    const unsigned char* A = lds + buf * kStage + a_panel;
    const unsigned char* B = lds + buf * kStage + b_panel;
    // a[i] feeds the BJ MFMAs of row i and is read again for the next
    // 16-token step right after them; b[j] is live through the whole step,
    // so it has two copies
    bf16x8 a[4], b[2][BJ];
#pragma unroll
    for (int j = 0; j < BJ; ++j) b[0][j] = frag(B, b_ch + 4 * j, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = frag(A, a_ch + 4 * i, 0);
#pragma unroll
    for (int ss = 0; ss < 4; ++ss) {
      if (ss < 3) {
#pragma unroll
        for (int j = 0; j < BJ; ++j)
          b[(ss + 1) & 1][j] = frag(B, b_ch + 4 * j, ss + 1);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < BJ; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              a[i], b[ss & 1][j], acc[i][j], 0, 0, 0);
        if (ss < 3) a[i] = frag(A, a_ch + 4 * i, ss + 1);
      }
    }
  };

  // s_count is the same for the whole workgroup: every barrier below is
  // reached by all of its waves or by none
  if (s_count > 0) {
    issue(0);
    commit(0);
    __syncthreads();
    for (int t = 0; t < s_count; ++t) {
      const bool more = t + 1 < s_count;
      if (more) issue(t + 1);
      compute(t & 1);
      if (more) commit((t & 1) ^ 1);
      __syncthreads();
    }
  }

  // ---- epilogue, as in k_wgrad.  The scheduling barriers keep the row
  // addresses of one 32 x 32 block at a time in registers: computed all at
  // once, beside 256 accumulators, they spilled.
  // A block stays in its accumulator registers until its turn.
#define SHAMD_WG_PIN(v) asm volatile("" : "+a"(v))
  const int row0 = n0 + wn * 128 + 4 * (lane >> 5);
  const int col0 = k0 + wk * (32 * BJ) + (lane & 31);
  if (split == 1) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < BJ; ++j) {
        uint16_t* o = dw + (int64_t)(row0 + 32 * i) * ldw + col0 + 32 * j;
        SHAMD_WG_PIN(acc[i][j]);
#pragma unroll
        for (int e = 0; e < 16; ++e)
          o[((e & 3) + 8 * (e >> 2)) * ldw] = f32_to_bf16(acc[i][j][e]);
        __builtin_amdgcn_sched_barrier(0);
      }
  } else {
    float* out = ws + (int64_t)sp * N * K;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < BJ; ++j) {
        float* o = out + (int64_t)(row0 + 32 * i) * K + col0 + 32 * j;
        SHAMD_WG_PIN(acc[i][j]);
#pragma unroll
        for (int e = 0; e < 16; ++e)
          o[(int64_t)((e & 3) + 8 * (e >> 2)) * K] = acc[i][j][e];
        __builtin_amdgcn_sched_barrier(0);
      }
  }
#undef SHAMD_WG_PIN

  if constexpr (CS) {
    if (colsum) {
      // the last barrier of the loop (or no loop at all) left the LDS free
      float* red = reinterpret_cast<float*>(lds);  // [NT / 16][256]
      float* mine = red + srow * 256 + 8 * sch;
      *reinterpret_cast<float4*>(mine) = make_float4(c0[0], c0[1], c0[2], c0[3]);
      *reinterpret_cast<float4*>(mine + 4) =
          make_float4(c0[4], c0[5], c0[6], c0[7]);
      *reinterpret_cast<float4*>(mine + 128) =
          make_float4(c1[0], c1[1], c1[2], c1[3]);
      *reinterpret_cast<float4*>(mine + 132) =
          make_float4(c1[4], c1[5], c1[6], c1[7]);
      __syncthreads();
      if (tid < 256) {
        float s = red[tid];
        for (int r = 1; r < NT / 16; ++r) s += red[r * 256 + tid];
        if (split == 1)
          db[n0 + tid] = f32_to_bf16(s);
        else
          wsb[(int64_t)sp * N + n0 + tid] = s;
      }
    }
  }
}

// k_wgrad256 with a software-pipelined step loop: the same tile, split
// scheme, swizzle, fragment layout, XCD remap and epilogue, and the same
// MFMAs in the same order on every accumulator, so dW has the same bits
// (tests/test_wgrad256p_resource_usage.py holds it to this plan).
//   * global -> LDS without registers: 16-byte direct-to-LDS loads.  Such a
//     load writes LDS at (wave-uniform base) + 16 lane, so the swizzle moves
//     to the global side: the lane that lands on 16-byte slot s of token row
//     r fetches chunk s ^ sw(r) of that row, where p_off(r, ch) = 256 r +
//     16 (ch ^ sw(r)).  16 lanes still cover one contiguous 256-byte row
//     segment, permuted.  One load of one wave fills 4 rows of one panel.
//   * the LDS is a ring of R = 4 slots of 32 tokens (2 dY + 2 X half panels
//     of [32][128], 32 KB; 128 KB in all).  Rows keep p_off: a slot is the
//     upper or lower half of a k_wgrad256 stage, byte for byte.  Each slot is
//     an array of its own, so that the compiler can tell a fragment read of
//     one slot from a load landing in another and does not wait for it.
//   * half step h (32 tokens, slot h % R) runs as: the 16 MFMAs of tokens
//     0..15, under which the fragments of tokens 16..31 are read; then wait
//     until this wave's loads of h + 1 have landed (a partial vmcnt: those of
//     h + 2 stay in flight), barrier, issue the loads of h + R - 1 into the
//     slot of h - 1, which every wave has left; then the 16 MFMAs of tokens
//     16..31, under which the first fragments of h + 1 are read.  Loads are
//     in flight for two half steps = one 64-token step, across two barriers.
//     (As built today the compiler adds one full vmcnt wait per turn of the
//     ring, so this holds for three half steps of four.)
//   * NO LOAD PAST THE OPERANDS: a load of half step h is issued only under
//     `h < hc` (hc = 2 s_count, workgroup-uniform), in the prologue and in
//     the loop alike.  The last split ends at the last row of dY and X; a
//     prefetch beyond hc would read past the end of the allocations.
//   * CS: the workgroups of K-tile 0 read the dY half panels of the slot they
//     are about to compute on back from LDS (a thread owns 8 columns of one
//     panel and 4 of the 32 rows), sum in fp32 in a fixed order, and combine
//     the 8 row groups through the first slot after the loop, as k_wgrad256.
template <bool CS>
__global__ __launch_bounds__(256)
    __attribute__((amdgpu_waves_per_eu(1, 1))) void k_wgrad256p(
    const uint16_t* __restrict__ dy, const uint16_t* __restrict__ x,
    uint16_t* __restrict__ dw, float* __restrict__ ws,
    uint16_t* __restrict__ db, float* __restrict__ wsb, int steps, int N,
    int K, int64_t ldy, int64_t ldx, int64_t ldw, int split, int tiles_k,
    int tiles) {
  typedef __attribute__((address_space(3))) unsigned char lds_u8;
  typedef const __attribute__((address_space(1))) void* gptr;
  constexpr int NW = 4, NT = 64 * NW;
  constexpr int BJ = 16 / NW;
  constexpr int R = 4;                         // ring slots
  constexpr int kHalf = 32;                    // tokens per slot
  constexpr int kHPanel = kHalf * 256;         // a [32][128] half panel
  constexpr int kSlot = 4 * kHPanel;
  constexpr int kLoads = kSlot / (NT * 16);    // loads per thread and slot
  static_assert(kLoads == 8 && kStep == 2 * kHalf, "ring plan");
  __shared__ __attribute__((aligned(16))) unsigned char ring0[kSlot];
  __shared__ __attribute__((aligned(16))) unsigned char ring1[kSlot];
  __shared__ __attribute__((aligned(16))) unsigned char ring2[kSlot];
  __shared__ __attribute__((aligned(16))) unsigned char ring3[kSlot];
  auto slot = [&](auto s) -> lds_u8* {
    constexpr int S = decltype(s)::value;
    if constexpr (S == 0) return (lds_u8*)ring0;
    else if constexpr (S == 1) return (lds_u8*)ring1;
    else if constexpr (S == 2) return (lds_u8*)ring2;
    else return (lds_u8*)ring3;
  };

  // block id -> (split, tile): ids that share an XCD become consecutive
  const int nwg = gridDim.x, orig = blockIdx.x;
  const int xcd = orig % kXcd, q8 = nwg / kXcd, r8 = nwg % kXcd;
  const int wg =
      (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) +
      orig / kXcd;
  const int sp = wg / tiles, tile = wg % tiles;
  const int n0 = (tile / tiles_k) * 256;
  const int k0 = (tile % tiles_k) * 256;
  const bool colsum = CS && k0 == 0;  // the same for the whole workgroup

  const int sq = steps / split, sr = steps % split;
  const int s_begin = sp * sq + min(sp, sr);
  const int s_count = sq + (sp < sr ? 1 : 0);
  const int hc = 2 * s_count;  // half steps; no load is issued for h >= hc

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int wn = wave / (NW / 2), wk = wave % (NW / 2);

  // load i of a slot: half panel i >> 1 (dY 0, 1, X 0, 1), rows 16 (i & 1) +
  // 4 wave .. + 3.  Lane l lands on row 4 wave + (l >> 4) of those 16, slot
  // l & 15, and fetches the chunk that p_off puts there.
  const int lrow = 4 * wave + (lane >> 4);
  const int lch = (lane & 15) ^ (((lrow & 3) << 2) | ((lrow >> 2) & 3));
  // uniform 64-bit base plus a 32-bit byte offset per thread, as k_wgrad256
  const char* const ga =
      reinterpret_cast<const char*>(dy + (int64_t)s_begin * kStep * ldy + n0);
  const char* const gb =
      reinterpret_cast<const char*>(x + (int64_t)s_begin * kStep * ldx + k0);
  const uint32_t va = 2u * (uint32_t)(lrow * (int)ldy + 8 * lch);
  const uint32_t vb = 2u * (uint32_t)(lrow * (int)ldx + 8 * lch);
  // the callers test h < hc: see the header
  auto dma = [&](lds_u8* base, int h) {
    const int64_t t = (int64_t)h * kHalf;
#pragma unroll
    for (int i = 0; i < kLoads; ++i) {
      const int p = i >> 1, r16 = 16 * (i & 1);
      const char* g =
          p < 2 ? ga + 2 * ((t + r16) * ldy + (p & 1) * kPanelCols) +
                      (uint64_t)va
                : gb + 2 * ((t + r16) * ldx + (p & 1) * kPanelCols) +
                      (uint64_t)vb;
      __builtin_amdgcn_global_load_lds(
          (gptr)g, base + p * kHPanel + r16 * 256 + wave * 1024, 16, 0, 0);
    }
  };
  // s_waitcnt with only vmcnt set (gfx9 encoding: vmcnt in bits 3:0 and
  // 15:14, expcnt 6:4 and lgkmcnt 11:8 left at "no wait")
#define SHAMD_WG_VMCNT(n) \
  __builtin_amdgcn_s_waitcnt(((n) & 15) | (((n) >> 4) << 14) | 0x0f70)
  // A bare barrier: the release fence of __syncthreads() would wait for every
  // load in flight (they write LDS).  What must be ordered is ordered by
  // hand: the vmcnt wait in front, and the reads of the slot that is loaded
  // next were consumed by MFMAs issued before the barrier.  The scheduling
  // barriers keep the compiler from moving LDS reads across it.  This rests
  // on how the compiler treats these builtins (s_barrier has side effects,
  // sched_barrier(0) lets nothing cross), not on a fence the LLVM memory
  // model promises: reread the ISA of the loop after a compiler update
  // (profiles/r19/README.md says what to look for).
#define SHAMD_WG_BARRIER()                 \
  do {                                     \
    __builtin_amdgcn_sched_barrier(0);     \
    __builtin_amdgcn_s_barrier();          \
    __builtin_amdgcn_sched_barrier(0);     \
  } while (0)
  // one LDS read after every MFMA, 16 times
#define SHAMD_WG_INTERLEAVE()                                   \
  _Pragma("unroll") for (int q = 0; q < 16; ++q) {              \
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);          \
    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);          \
  }

  // column sums: thread owns chunk cs_ch of dY half panel cs_p, rows cs_r +
  // 8 k of a slot
  const int cs_ch = tid & 15, cs_p = (tid >> 4) & 1, cs_r = tid >> 5;
  float c[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) c[e] = 0.f;
  // rows cs_r + 8 k: k and k + 2 share the swizzle, 16 rows apart
  const int cs_off[2] = {cs_p * kHPanel + p_off(cs_r, cs_ch),
                         cs_p * kHPanel + p_off(cs_r + 8, cs_ch)};
  auto csum = [&](lds_u8* base) {
#pragma unroll
    for (int k = 0; k < kHalf / 8; ++k) {
      typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
      const u32x4 q = *reinterpret_cast<
          const __attribute__((address_space(3))) u32x4*>(
          base + cs_off[k & 1] + (k >> 1) * (16 * 256));
      float v[8];
      unpack8(make_uint4(q[0], q[1], q[2], q[3]), v);
#pragma unroll
      for (int e = 0; e < 8; ++e) c[e] += v[e];
    }
  };

  f32x16 acc[4][BJ];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < BJ; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  // fragment addressing as in k_wgrad256; ss is 0 or 1 inside a slot
  const int grp = lane >> 4, gi = lane & 15;
  const int tr_q = gi >> 2, tr_p = gi & 3, hi = grp >> 1;
  const int a_ch = 2 * (grp & 1) + (tr_p >> 1);
  const int a_panel = wn * kHPanel;
  const int b_panel = (2 + wk) * kHPanel;

  // Byte offsets of the two reads of fragment i at tokens 0..15 of a slot,
  // with the wave's half panel folded in; tokens 16..31 are 16 rows further.
  // Kept as values so that slot, ss and nothing else become the immediate
  // offset of a read: derived anew per read, the XOR forms took 88 address
  // registers.
  int a_off[4][2], b_off[BJ][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
      const int o =
          p_off(8 * jj + 4 * hi + tr_q, a_ch + 4 * i) + 8 * (tr_p & 1);
      a_off[i][jj] = a_panel + o;
      b_off[i][jj] = b_panel + o;
    }
  auto frag = [&](lds_u8* base, const int (&off)[2], int ss) -> bf16x8 {
    bf16x8 f;
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
      auto* a = reinterpret_cast<__attribute__((address_space(3))) s16x4*>(
          base + off[jj] + ss * (16 * 256));
      s16x4 tr = __builtin_amdgcn_ds_read_tr16_b64_v4i16(a);
      bf16x4 tb = __builtin_bit_cast(bf16x4, tr);
#pragma unroll
      for (int e = 0; e < 4; ++e) f[4 * jj + e] = tb[e];
    }
    return f;
  };

  // a[i] and b[0][j] hold the fragments of tokens 0..15 of the half step
  // about to run; b[1][j] those of tokens 16..31
  bf16x8 a[4], b[2][BJ];
  auto half_step = [&](auto s, int h) {
    constexpr int S = decltype(s)::value;
    lds_u8* const cur = slot(std::integral_constant<int, S>{});
    lds_u8* const nxt = slot(std::integral_constant<int, (S + 1) % R>{});
    lds_u8* const fre = slot(std::integral_constant<int, (S + R - 1) % R>{});
    if constexpr (CS) {
      if (colsum) csum(cur);
    }
#pragma unroll
    for (int j = 0; j < BJ; ++j) b[1][j] = frag(cur, b_off[j], 1);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int j = 0; j < BJ; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            a[i], b[0][j], acc[i][j], 0, 0, 0);
      a[i] = frag(cur, a_off[i], 1);
    }
    SHAMD_WG_INTERLEAVE();
    // this wave's loads of h + 1 have landed; those of h + 2, if any, stay
    // in flight.  Behind the barrier every wave's have, and every wave has
    // left the slot of h - 1.  After the last half step nothing is in flight
    // and the fragments read below are stale bytes of the ring, unused.
    if (h + 2 < hc)
      SHAMD_WG_VMCNT(kLoads);
    else
      SHAMD_WG_VMCNT(0);
    SHAMD_WG_BARRIER();
    if (h + R - 1 < hc) dma(fre, h + R - 1);
#pragma unroll
    for (int j = 0; j < BJ; ++j) b[0][j] = frag(nxt, b_off[j], 0);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int j = 0; j < BJ; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            a[i], b[1][j], acc[i][j], 0, 0, 0);
      a[i] = frag(nxt, a_off[i], 0);
    }
    SHAMD_WG_INTERLEAVE();
  };

  // hc is the same for the whole workgroup: every barrier is reached by all
  // of its waves or by none
  if (hc > 0) {
    using std::integral_constant;
    // half steps 0 .. R - 2 into the slots from S0 on, each only if it
    // exists, and the first fragments
    auto prologue = [&](auto s0) {
      constexpr int S0 = decltype(s0)::value;
      lds_u8* const first = slot(integral_constant<int, S0>{});
      dma(first, 0);
      if (1 < hc) dma(slot(integral_constant<int, (S0 + 1) % R>{}), 1);
      if (2 < hc) dma(slot(integral_constant<int, (S0 + 2) % R>{}), 2);
      if (2 < hc)
        SHAMD_WG_VMCNT(2 * kLoads);
      else if (1 < hc)
        SHAMD_WG_VMCNT(kLoads);
      else
        SHAMD_WG_VMCNT(0);
      SHAMD_WG_BARRIER();
#pragma unroll
      for (int j = 0; j < BJ; ++j)
        b[0][j] = frag(first, b_off[j], 0);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        a[i] = frag(first, a_off[i], 0);
    };
    // the loop body is one whole turn of the ring, two steps, without a
    // branch around MFMAs (with one, the accumulators spilled); an odd step
    // count runs its first step in slots 2 and 3
    int h = 0;
    if (s_count & 1) {
      prologue(integral_constant<int, 2>{});
      half_step(integral_constant<int, 2>{}, 0);
      half_step(integral_constant<int, 3>{}, 1);
      h = 2;
    } else {
      prologue(integral_constant<int, 0>{});
    }
    for (; h < hc; h += R) {
      half_step(integral_constant<int, 0>{}, h);
      half_step(integral_constant<int, 1>{}, h + 1);
      half_step(integral_constant<int, 2>{}, h + 2);
      half_step(integral_constant<int, 3>{}, h + 3);
    }
  }
#undef SHAMD_WG_VMCNT
#undef SHAMD_WG_BARRIER
#undef SHAMD_WG_INTERLEAVE

  // ---- epilogue, as in k_wgrad256
#define SHAMD_WG_PIN(v) asm volatile("" : "+a"(v))
  const int row0 = n0 + wn * 128 + 4 * (lane >> 5);
  const int col0 = k0 + wk * (32 * BJ) + (lane & 31);
  if (split == 1) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < BJ; ++j) {
        uint16_t* o = dw + (int64_t)(row0 + 32 * i) * ldw + col0 + 32 * j;
        SHAMD_WG_PIN(acc[i][j]);
#pragma unroll
        for (int e = 0; e < 16; ++e)
          o[((e & 3) + 8 * (e >> 2)) * ldw] = f32_to_bf16(acc[i][j][e]);
        __builtin_amdgcn_sched_barrier(0);
      }
  } else {
    float* out = ws + (int64_t)sp * N * K;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < BJ; ++j) {
        float* o = out + (int64_t)(row0 + 32 * i) * K + col0 + 32 * j;
        SHAMD_WG_PIN(acc[i][j]);
#pragma unroll
        for (int e = 0; e < 16; ++e)
          o[(int64_t)((e & 3) + 8 * (e >> 2)) * K] = acc[i][j][e];
        __builtin_amdgcn_sched_barrier(0);
      }
  }
#undef SHAMD_WG_PIN

  if constexpr (CS) {
    if (colsum) {
      // every wave has left the ring behind this barrier
      __syncthreads();
      float* red = reinterpret_cast<float*>(ring0);  // [kHalf / 4][256]
      float* mine = red + cs_r * 256 + cs_p * 128 + 8 * cs_ch;
      *reinterpret_cast<float4*>(mine) = make_float4(c[0], c[1], c[2], c[3]);
      *reinterpret_cast<float4*>(mine + 4) =
          make_float4(c[4], c[5], c[6], c[7]);
      __syncthreads();
      float s = red[tid];
      for (int r = 1; r < NT / 32; ++r) s += red[r * 256 + tid];
      if (split == 1)
        db[n0 + tid] = f32_to_bf16(s);
      else
        wsb[(int64_t)sp * N + n0 + tid] = s;
    }
  }
}

// dW = bf16(sum over splits, in index order, of ws[split][N][K]); a thread
// owns 8 consecutive columns of one row (K is a multiple of 8).  With db, the
// blocks after those of dW do the same for db = bf16(sum of wsb[split][N]).
__global__ __launch_bounds__(256) void k_wgrad_reduce(
    const float* __restrict__ ws, uint16_t* __restrict__ dw, int64_t groups,
    int K8, int64_t NK, int64_t ldw, int split,
    const float* __restrict__ wsb, uint16_t* __restrict__ db, int N8) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t bias0 = (groups + 255) / 256 * 256;  // first thread of db
  const float* p;
  uint16_t* o;
  int64_t stride;
  if (g < groups) {
    const int64_t row = g / K8;
    const int col = (int)(g % K8) * 8;
    p = ws + row * (int64_t)(K8 * 8) + col;
    o = dw + row * ldw + col;
    stride = NK;
  } else if (g >= bias0 && g - bias0 < N8) {
    p = wsb + (g - bias0) * 8;
    o = db + (g - bias0) * 8;
    stride = (int64_t)N8 * 8;
  } else {
    return;
  }
  float v[8];
  {
    const float4 a = *reinterpret_cast<const float4*>(p);
    const float4 b = *reinterpret_cast<const float4*>(p + 4);
    v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w;
    v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
  }
  for (int s = 1; s < split; ++s) {
    const float4 a = *reinterpret_cast<const float4*>(p + s * stride);
    const float4 b = *reinterpret_cast<const float4*>(p + s * stride + 4);
    v[0] += a.x, v[1] += a.y, v[2] += a.z, v[3] += a.w;
    v[4] += b.x, v[5] += b.y, v[6] += b.z, v[7] += b.w;
  }
  *reinterpret_cast<uint4*>(o) = pack8(v);
}

struct Variant {
  int tile_n, tile_k;
  bool colsum;  // can write db
};
constexpr Variant kVariants[] = {{128, 128, false},
                                 {128, 128, false},
                                 {256, 128, false},
                                 {256, 256, true},
                                 {256, 256, true}};
constexpr int kNumVariants = sizeof(kVariants) / sizeof(kVariants[0]);

}  // namespace

int hip_wgrad_num_variants() { return kNumVariants; }

void hip_wgrad_tile(int variant, int* tile_n, int* tile_k) {
  if (variant < 0 || variant >= kNumVariants)
    throw std::runtime_error("wgrad_bf16: unknown variant");
  *tile_n = kVariants[variant].tile_n;
  *tile_k = kVariants[variant].tile_k;
}

void hip_wgrad_bf16(const void* dy, const void* x, void* dw, float* ws,
                    int64_t ws_floats, int64_t M, int64_t N, int64_t K,
                    int64_t ldy, int64_t ldx, int64_t ldw, int64_t split,
                    int variant, hipStream_t s, void* db, float* wsb,
                    int64_t wsb_floats) {
  const char* op = "wgrad_bf16";
  auto fail = [&](const char* what) {
    throw std::runtime_error(std::string(op) + ": " + what);
  };
  if (variant < 0 || variant >= kNumVariants) fail("unknown variant");
  const int tn = kVariants[variant].tile_n, tk = kVariants[variant].tile_k;
  if (M <= 0 || N <= 0 || K <= 0) fail("empty problem");
  if (M % kStep) fail("M must be a multiple of 64");
  if (N % tn || K % tk) fail("N and K must be multiples of the tile");
  if (ldy < N || ldx < K || ldw < K) fail("row stride shorter than the row");
  if (ldy % 8 || ldx % 8 || ldw % 8)
    fail("row strides must be multiples of 8 elements");
  // k_wgrad256 and k_wgrad256p keep a thread's byte offset inside 64 rows in
  // 32 bits
  if (ldy > (1 << 24) || ldx > (1 << 24)) fail("row stride too large");
  check_align(dy, 16, op, "dy");
  check_align(x, 16, op, "x");
  check_align(dw, 16, op, "dw");
  const int64_t steps = M / kStep;
  const int64_t tiles = (N / tn) * (K / tk);
  if (split < 1 || split > 4096) fail("split out of range");
  if (steps > 0x7fffffff / kStep || N > (1 << 24) || K > (1 << 24) ||
      tiles * split > 0x7fffffff)
    fail("problem too large");
  if (split > 1) {
    if (ws == nullptr || ws_floats < split * N * K)
      fail("workspace smaller than split * N * K floats");
    check_align(ws, 16, op, "ws");
  }
  if (db != nullptr) {
    if (!kVariants[variant].colsum) fail("this variant takes no db");
    check_align(db, 16, op, "db");
    if (split > 1) {
      if (wsb == nullptr || wsb_floats < split * N)
        fail("db workspace smaller than split * N floats");
      check_align(wsb, 16, op, "wsb");
    }
  }
  auto* dyp = static_cast<const uint16_t*>(dy);
  auto* xp = static_cast<const uint16_t*>(x);
  auto* dwp = static_cast<uint16_t*>(dw);
  auto* dbp = static_cast<uint16_t*>(db);
  const dim3 grid((unsigned)(tiles * split));
  const int tiles_k = (int)(K / tk);
#define SHAMD_WGRAD_LAUNCH(NP, KP, NBUF)                                     \
  k_wgrad<NP, KP, NBUF><<<grid, dim3(256 * NP * KP), 0, s>>>(                \
      dyp, xp, dwp, ws, (int)steps, (int)N, (int)K, ldy, ldx, ldw,           \
      (int)split, tiles_k, (int)tiles)
  switch (variant) {
    case 0: SHAMD_WGRAD_LAUNCH(1, 1, 2); break;
    case 1: SHAMD_WGRAD_LAUNCH(1, 1, 1); break;
    case 2: SHAMD_WGRAD_LAUNCH(2, 1, 2); break;
    case 3:
      dispatch_bool(db != nullptr, [&](auto cs) {
        k_wgrad256<decltype(cs)::value><<<grid, dim3(256), 0, s>>>(
            dyp, xp, dwp, ws, dbp, wsb, (int)steps, (int)N, (int)K, ldy, ldx,
            ldw, (int)split, tiles_k, (int)tiles);
      });
      break;
    default:
      dispatch_bool(db != nullptr, [&](auto cs) {
        k_wgrad256p<decltype(cs)::value><<<grid, dim3(256), 0, s>>>(
            dyp, xp, dwp, ws, dbp, wsb, (int)steps, (int)N, (int)K, ldy, ldx,
            ldw, (int)split, tiles_k, (int)tiles);
      });
      break;
  }
#undef SHAMD_WGRAD_LAUNCH
  HIP_CHECK(hipGetLastError());
  if (split > 1) {
    const int64_t groups = N * K / 8;
    const int64_t blocks =
        (groups + 255) / 256 + (db != nullptr ? (N / 8 + 255) / 256 : 0);
    k_wgrad_reduce<<<dim3((unsigned)blocks), dim3(256), 0, s>>>(
        ws, dwp, groups, (int)(K / 8), N * K, ldw, (int)split, wsb, dbp,
        db != nullptr ? (int)(N / 8) : 0);
    HIP_CHECK(hipGetLastError());
  }
}

}  // namespace shamd
