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

// dW = bf16(sum over splits, in index order, of ws[split][N][K]); a thread
// owns 8 consecutive columns of one row (K is a multiple of 8)
__global__ __launch_bounds__(256) void k_wgrad_reduce(
    const float* __restrict__ ws, uint16_t* __restrict__ dw, int64_t groups,
    int K8, int64_t NK, int64_t ldw, int split) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= groups) return;
  const int64_t row = g / K8;
  const int col = (int)(g % K8) * 8;
  const float* p = ws + row * (int64_t)(K8 * 8) + col;
  float v[8];
  {
    const float4 a = *reinterpret_cast<const float4*>(p);
    const float4 b = *reinterpret_cast<const float4*>(p + 4);
    v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w;
    v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
  }
  for (int s = 1; s < split; ++s) {
    const float4 a = *reinterpret_cast<const float4*>(p + s * NK);
    const float4 b = *reinterpret_cast<const float4*>(p + s * NK + 4);
    v[0] += a.x, v[1] += a.y, v[2] += a.z, v[3] += a.w;
    v[4] += b.x, v[5] += b.y, v[6] += b.z, v[7] += b.w;
  }
  *reinterpret_cast<uint4*>(dw + row * ldw + col) = pack8(v);
}

struct Variant {
  int tile_n, tile_k;
};
constexpr Variant kVariants[] = {{128, 128}, {128, 128}, {256, 128}};
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
                    int variant, hipStream_t s) {
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
  auto* dyp = static_cast<const uint16_t*>(dy);
  auto* xp = static_cast<const uint16_t*>(x);
  auto* dwp = static_cast<uint16_t*>(dw);
  const dim3 grid((unsigned)(tiles * split));
  const int tiles_k = (int)(K / tk);
#define SHAMD_WGRAD_LAUNCH(NP, KP, NBUF)                                     \
  k_wgrad<NP, KP, NBUF><<<grid, dim3(256 * NP * KP), 0, s>>>(                \
      dyp, xp, dwp, ws, (int)steps, (int)N, (int)K, ldy, ldx, ldw,           \
      (int)split, tiles_k, (int)tiles)
  switch (variant) {
    case 0: SHAMD_WGRAD_LAUNCH(1, 1, 2); break;
    case 1: SHAMD_WGRAD_LAUNCH(1, 1, 1); break;
    default: SHAMD_WGRAD_LAUNCH(2, 1, 2); break;
  }
#undef SHAMD_WGRAD_LAUNCH
  HIP_CHECK(hipGetLastError());
  if (split > 1) {
    const int64_t groups = N * K / 8;
    k_wgrad_reduce<<<dim3((unsigned)((groups + 255) / 256)), dim3(256), 0,
                     s>>>(ws, dwp, groups, (int)(K / 8), N * K, ldw,
                          (int)split);
    HIP_CHECK(hipGetLastError());
  }
}

}  // namespace shamd
