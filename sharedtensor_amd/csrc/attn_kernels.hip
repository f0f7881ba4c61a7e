// Causal bf16 attention forward for head dim 64 (GPT-2), flash style: the
// T x T score matrix lives only in registers, one KV tile at a time, with an
// online softmax.  fp32 accumulation, bf16 in and out, no dropout, no bias,
// top-left aligned causal mask (Tq == Tk).
//
// Plan (tests/test_attn_resource_usage.py holds the kernel to it):
//   * workgroup = 4 waves = 128 query rows of one (batch, head); a wave owns
//     32 rows.  KV tile = 64 keys.
//   * Q stays in registers (4 x bf16x8 per lane) for the whole block.
//   * K and V tiles are double-buffered in LDS, 2 x (8 KB + 8 KB) = 32 KB.
//     The next tile's global loads are issued before the current tile's
//     MFMAs and written to LDS after them; one barrier per tile.  Issuing
//     them after Q K^T instead measured the same (330.2 against 330.3 us,
//     bit-equal results), so the simpler order stays.
//       - K rows are 128 B; 16-byte chunk c of key row r sits at chunk
//         c ^ ((r >> 1) & 7), so the ds_read_b128 of a 16-lane group (16
//         consecutive keys, one chunk) touches 16 different 16-byte slots of
//         the 256-byte bank line.
//       - V rows are 128 B; the two 64-byte halves of rows with bit 1 set are
//         swapped, so the 4 rows x 64 B that one 32-lane half fetches with
//         ds_read_b64_tr_b16 cover the bank line once.
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
//     tile that crosses the diagonal is masked.
//   * O is staged through the (then idle) LDS so that every global store is a
//     whole 128-byte row of (B, T, H, 64).
//   * Grid: the query blocks of one (b, h) are consecutive on one XCD
//     (blockIdx % 8), heaviest (last) query block first, so K/V are re-read
//     from that XCD's L2.
//   * Resources: at most 128 VGPRs, no AGPRs, no scratch, no spills, 32 KB
//     of LDS -> 4 waves/SIMD, i.e. 4 workgroups per CU (LDS would allow 5).
//
// Every T is bounds-checked: query rows and key rows at or past T are read
// as zeros (never from memory) and never stored.
#include <hip/hip_runtime.h>

#include "device_util.h"
#include "hip_api.h"

namespace shamd {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

constexpr int kD = 64;         // head dim
constexpr int kQW = 32;        // query rows per wave
constexpr int kWaves = 4;
constexpr int kQB = kQW * kWaves;  // query rows per workgroup
constexpr int kKV = 64;        // keys per tile
constexpr int kTileBytes = kKV * kD * 2;
constexpr int kXcd = 8;

struct AttnStrides {
  int64_t b, t, h;  // elements
};

// byte offset of 16-byte chunk `ch` (0..7) of key row `row` in a K tile
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

// waves_per_eu(4, 4): the body fits 128 VGPRs without scratch; left alone the
// compiler takes 142 + AGPRs and halves the occupancy (measured 351 us at 2
// waves/SIMD, 335 us at 3, 330 us at 4 on the B=64 H=12 T=1024 shape).
__global__ __launch_bounds__(256)
    __attribute__((amdgpu_waves_per_eu(4, 4))) void k_attn_fwd_causal_hd64(
    const uint16_t* __restrict__ q, const uint16_t* __restrict__ k,
    const uint16_t* __restrict__ v, uint16_t* __restrict__ out,
    float* __restrict__ lse, int nbh, int H, int T, int nqb, AttnStrides sq,
    AttnStrides sk, AttnStrides sv, int64_t lse_stride, float scale_log2e) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[4 * kTileBytes];
  // K buffers at 0 and kTileBytes, V buffers behind them
  unsigned char* const ldsK = lds;
  unsigned char* const ldsV = lds + 2 * kTileBytes;

  // blockIdx -> (head, query block): block ids round-robin over the XCDs
  const int xcd = blockIdx.x % kXcd;
  const int slot = blockIdx.x / kXcd;
  const int bh = (slot / nqb) * kXcd + xcd;
  if (bh >= nbh) return;  // whole workgroup, before any barrier
  const int qb = nqb - 1 - slot % nqb;
  const int b = bh / H, h = bh % H;

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int r = lane & 31, hi = lane >> 5;

  const int q0 = qb * kQB;
  const int qw0 = q0 + wave * kQW;  // the wave's first query row
  const int qrow = qw0 + r;         // this lane's query row

  const uint16_t* qp = q + b * sq.b + h * sq.h;
  const uint16_t* kp = k + b * sk.b + h * sk.h;
  const uint16_t* vp = v + b * sv.b + h * sv.h;

  // Q fragment: B operand of mfma(K, Q); lane holds Q[qrow][16 ks + 8 hi + j]
  bf16x8 qf[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    uint4 t = load16_or_zero(qp + (int64_t)qrow * sq.t + 16 * ks + 8 * hi,
                             qrow < T);
    qf[ks] = __builtin_bit_cast(bf16x8, t);
  }

  // staging: thread covers 16-byte chunk (tid & 7) of keys (tid >> 3) and
  // (tid >> 3) + 32 of the tile, for K and for V
  const int skey = tid >> 3, sch = tid & 7;
  uint4 stK[2], stV[2];
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
      int row = skey + 32 * i;
      *reinterpret_cast<uint4*>(ldsK + buf * kTileBytes + k_off(row, sch)) =
          stK[i];
      *reinterpret_cast<uint4*>(ldsV + buf * kTileBytes + v_off(row, sch)) =
          stV[i];
    }
  };

  const int kv_end = min(T, q0 + kQB);          // keys this block can see
  const int ntiles = (kv_end + kKV - 1) / kKV;  // >= 1

  f32x16 o[2];  // O^T: lane holds O[qrow][32 nb + (reg&3) + 8 (reg>>2) + 4 hi]
#pragma unroll
  for (int nb = 0; nb < 2; ++nb)
#pragma unroll
    for (int i = 0; i < 16; ++i) o[nb][i] = 0.f;
  float m = -INFINITY;  // running max of score * scale * log2(e)
  float l = 0.f;        // this lane half's share of the running sum

  // transposed-read address of V inside a tile, without the (s, jj, nb) part:
  // 16-lane group g reads rows k0 .. k0+3, columns 32 nb + 16 (g & 1) + 0..15;
  // lane 4 qq + p of the group supplies row qq, columns 4 p .. 4 p + 3
  const int grp = lane >> 4, gi = lane & 15;
  const int tr_q = gi >> 2, tr_p = gi & 3;

  issue(0);
  commit(0);
  __syncthreads();

  for (int t = 0; t < ntiles; ++t) {
    const int cur = t & 1;
    const int kv0 = t * kKV;
    const bool more = t + 1 < ntiles;
    if (more) issue(kv0 + kKV);

    if (kv0 <= qw0 + kQW - 1) {  // wave-uniform: the tile has visible keys
      const unsigned char* Kt = ldsK + cur * kTileBytes;
      const unsigned char* Vt = ldsV + cur * kTileBytes;

      // S^T = K Q^T: s[kb][reg] = score(qrow, kv0 + 32 kb + keymap(reg, hi))
      f32x16 s[2];
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
        for (int i = 0; i < 16; ++i) s[kb][i] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          uint4 kk = *reinterpret_cast<const uint4*>(
              Kt + k_off(32 * kb + r, 2 * ks + hi));
          s[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              __builtin_bit_cast(bf16x8, kk), qf[ks], s[kb], 0, 0, 0);
        }
      }

      if (kv0 + kKV - 1 > qw0) {  // wave-uniform: the tile crosses the diagonal
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
      for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int i = 0; i < 16; ++i) o[nb][i] *= alpha;

      // O^T += V^T P^T; element j of the fragment of k-step ss is key
      // 16 ss + 8 (j >> 2) + 4 hi + (j & 3), the order P's registers have
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) {
#pragma unroll
        for (int ss = 0; ss < 4; ++ss) {
          bf16x8 vf;
#pragma unroll
          for (int jj = 0; jj < 2; ++jj) {
            int row = 16 * ss + 8 * jj + 4 * (grp >> 1) + tr_q;
            int ch = 4 * nb + 2 * (grp & 1) + (tr_p >> 1);
            auto* a = reinterpret_cast<
                __attribute__((address_space(3))) s16x4*>(
                (uintptr_t)(Vt + v_off(row, ch) + 8 * (tr_p & 1)));
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
    lse[(int64_t)bh * lse_stride + qrow] =
        (m + __builtin_amdgcn_logf(l)) * 0.6931471805599453f;

  // the loop's last barrier is behind every wave: K/V tiles are dead.  Each
  // wave owns 4 KB: [32 rows][8 chunks of 16 B], chunks swizzled like K.
  unsigned char* const Ow = lds + wave * (kQW * 128);
#pragma unroll
  for (int nb = 0; nb < 2; ++nb)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float f[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) f[e] = o[nb][4 * g + e] * inv;
      // d = 32 nb + 8 g + 4 hi + e: chunk 4 nb + g, its half hi
      *reinterpret_cast<uint2*>(Ow + k_off(r, 4 * nb + g) + 8 * hi) = pack4(f);
    }
  __syncthreads();
  uint16_t* op = out + ((int64_t)b * T * H + h) * kD;
#pragma unroll
  for (int pass = 0; pass < 4; ++pass) {
    int row = pass * 8 + (lane >> 3), ch = lane & 7;
    uint4 val = *reinterpret_cast<const uint4*>(Ow + k_off(row, ch));
    int qr = qw0 + row;
    if (qr < T)
      *reinterpret_cast<uint4*>(op + (int64_t)qr * H * kD + 8 * ch) = val;
  }
}

}  // namespace

void hip_attn_fwd_causal_hd64(const void* q, const void* k, const void* v,
                              void* out, float* lse, int64_t B, int64_t H,
                              int64_t T, const int64_t* qs, const int64_t* ks,
                              const int64_t* vs, int64_t lse_stride,
                              float scale, hipStream_t s) {
  const char* op = "attn_fwd_causal_hd64";
  if (B <= 0 || H <= 0 || T <= 0)
    throw std::runtime_error(std::string(op) + ": empty problem");
  if (!(scale > 0.f) || scale > 3.0e38f)
    throw std::runtime_error(std::string(op) + ": scale must be positive");
  if (lse_stride < T)
    throw std::runtime_error(std::string(op) + ": lse row shorter than T");
  check_align(q, 16, op, "q");
  check_align(k, 16, op, "k");
  check_align(v, 16, op, "v");
  check_align(out, 16, op, "out");
  check_align(lse, 4, op, "lse");
  for (const int64_t* st : {qs, ks, vs})
    for (int i = 0; i < 3; ++i)
      if (st[i] < 0 || st[i] % 8)
        throw std::runtime_error(std::string(op) +
                                 ": strides must be multiples of 8 elements");
  const int64_t nqb = (T + kQB - 1) / kQB;
  const int64_t nbh = B * H;
  const int64_t grid = (nbh + kXcd - 1) / kXcd * kXcd * nqb;
  if (grid > 0x7fffffff || T > (1 << 30) || nbh > 0x7fffffff)
    throw std::runtime_error(std::string(op) + ": problem too large");
  AttnStrides a{qs[0], qs[1], qs[2]}, bb{ks[0], ks[1], ks[2]},
      c{vs[0], vs[1], vs[2]};
  k_attn_fwd_causal_hd64<<<dim3((unsigned)grid), dim3(256), 0, s>>>(
      static_cast<const uint16_t*>(q), static_cast<const uint16_t*>(k),
      static_cast<const uint16_t*>(v), static_cast<uint16_t*>(out), lse,
      (int)nbh, (int)H, (int)T, (int)nqb, a, bb, c, lse_stride,
      scale * 1.4426950408889634f);
  HIP_CHECK(hipGetLastError());
}

}  // namespace shamd
