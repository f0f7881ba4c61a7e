// Document-masked causal bf16 grouped-query attention forward for head dim 64
// (packed Llama batches): the gqa_attn_kernels.hip kernel with one more mask.
// A batch row holds several documents, contiguous runs of positions; query i
// sees key j when doc_start[b, i] <= j <= i, doc_start[b, i] being the first
// position of the document that holds i.  doc_start is (B, T) int32 and
// non-decreasing in t.  There is no T x T object anywhere.
//
// Plan (tests/test_gqa_attn_doc_resource_usage.py holds the kernel to it):
//   * Mapping, tiles, swizzles, lane layouts, grid and bounds rules are those
//     of attn_fwd_body<64, HW> (attn_fwd_tile.h): a wave is a query head with
//     32 rows, workgroup = HW heads x 128 / HW positions, 64-key tiles double
//     buffered in LDS.  The loop is written anew here, so that the plain
//     kernels compile as they did.
//   * The masks pay: doc_start is monotone, so the first KV tile a wave needs
//     is doc_start[its first row] / 64, and the workgroup stages from
//     doc_start[its first row] / 64, the minimum over its waves.  Both are
//     uniform loads (the address depends on blockIdx and the wave index
//     alone).  Tiles before a wave's first are skipped by that wave, like the
//     tiles above its rows.
//   * A tile takes the lower mask only if kv0 < doc_start[last row of the
//     wave] and the diagonal mask only if it crosses the diagonal; both tests
//     are wave-uniform and interior tiles stay mask-free.  The lane's own
//     doc_start is loaded once, before the loop.
//   * A wave whose rows span two documents meets tiles in which its later
//     rows see nothing.  Their running maximum stays -inf, and the reference
//     maximum of the tile is clamped to -FLT_MAX: exp2(-inf - (-FLT_MAX)) is
//     a clean 0 for alpha and for every p, with no branch per element, and
//     the first tile with a visible key rescales by exp2(-FLT_MAX - m) = 0
//     times a zero sum.  Every row sees itself, so l > 0 at the end.
//   * Resources: amdgpu_waves_per_eu(4, 4), at most 128 VGPRs, no AGPRs, no
//     scratch, no spills, 32 KB of LDS -> 4 waves/SIMD, the plain kernel's
//     line.
//
// doc_start values steer loop bounds, so the two uniform ones are clamped to
// [0, row]: a wrong array gives wrong numbers, never an address outside K/V.
#include <hip/hip_runtime.h>

#include <cfloat>

#include "attn_fwd_tile.h"
#include "device_util.h"
#include "hip_api.h"

namespace shamd {
namespace {

// nbk = B * Hkv, nqb = position blocks of 128 / HW rows
template <int HW>
__global__ __launch_bounds__(256)
    __attribute__((amdgpu_waves_per_eu(4, 4))) void k_gqa_fwd_doc_hd64(
    const uint16_t* __restrict__ q, const uint16_t* __restrict__ k,
    const uint16_t* __restrict__ v, const int* __restrict__ doc_start,
    uint16_t* __restrict__ out, float* __restrict__ lse, int nbk, int Hkv,
    int G, int T, int nqb, AttnStrides sq, AttnStrides sk, AttnStrides sv,
    int64_t lse_stride, float scale_log2e) {
  constexpr int kWPH = kWaves / HW;   // waves per head
  constexpr int kPB = kRW * kWPH;     // positions per workgroup
  constexpr int kTileBytes = kHalfBytes;
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
  const int q0 = qb * kPB;                          // < T
  const int qw0 = q0 + (wave % kWPH) * kRW;  // the wave's first query row
  const int qrow = qw0 + r;                  // this lane's query row

  const uint16_t* qp = q + b * sq.b + h * sq.h;
  const uint16_t* kp = k + b * sk.b + kvh * sk.h;
  const uint16_t* vp = v + b * sv.b + kvh * sv.h;

  // document starts: of the workgroup's first row, of the wave's first and
  // last rows (uniform, clamped) and of the lane's row.  Rows at or past T
  // take the values of row T - 1 (uniform) or 0 (lane: nothing to mask).
  const int* dsp = doc_start + (int64_t)b * T;
  const int ds_wg = min(max(dsp[q0], 0), q0);
  const int rw0 = min(qw0, T - 1), rw1 = min(qw0 + kRW - 1, T - 1);
  const int ds_first = min(max(dsp[rw0], 0), rw0);
  const int ds_last = dsp[rw1];
  const int ds_row = qrow < T ? dsp[qrow] : 0;

  // Q fragment: B operand of mfma(K, Q); lane holds Q[qrow][16 ks + 8 hi + j]
  bf16x8 qf[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks)
    qf[ks] = __builtin_bit_cast(
        bf16x8, load16_or_zero(qp + (int64_t)qrow * sq.t + 16 * ks + 8 * hi,
                               qrow < T));

  // staging: thread covers chunk sch of keys skey and skey + 32, for K and V
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

  const int kv_end = min(T, q0 + kPB);              // keys this block can see
  const int ntiles = (kv_end + kTile - 1) / kTile;  // >= 1
  const int t_begin = ds_wg / kTile;                // <= q0 / kTile < ntiles
  const int kv_first = ds_first / kTile * kTile;    // the wave's first tile

  // O^T: lane holds O[qrow][32 nb + (reg&3) + 8 (reg>>2) + 4 hi]
  f32x16 o[2];
#pragma unroll
  for (int nb = 0; nb < 2; ++nb)
#pragma unroll
    for (int i = 0; i < 16; ++i) o[nb][i] = 0.f;
  float m = -INFINITY;  // running max of score * scale * log2(e)
  float l = 0.f;        // this lane half's share of the running sum

  // transposed-read address of V, without the (s, jj, nb) part: 16-lane group
  // g reads rows k0 .. k0+3, columns 32 nb + 16 (g & 1) + 0..15; lane
  // 4 qq + p of the group supplies row qq, columns 4 p .. 4 p + 3
  const int grp = lane >> 4, gi = lane & 15;
  const int tr_q = gi >> 2, tr_p = gi & 3;

  issue(t_begin * kTile);
  commit(t_begin & 1);
  __syncthreads();

  for (int t = t_begin; t < ntiles; ++t) {
    const int cur = t & 1;
    const int kv0 = t * kTile;
    const bool more = t + 1 < ntiles;
    if (more) issue(kv0 + kTile);

    // wave-uniform: the tile has keys that rows of the wave can see
    if (kv0 <= qw0 + kRW - 1 && kv0 >= kv_first) {
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

      // wave-uniform: the tile crosses the diagonal, or holds keys before the
      // document of the wave's last row
      if (kv0 + kTile - 1 > qw0 || kv0 < ds_last) {
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            int key = kv0 + 32 * kb + (i & 3) + 8 * (i >> 2) + 4 * hi;
            if (key > qrow || key < ds_row) s[kb][i] = -INFINITY;
          }
      }

      // a row may see no key of this tile: the clamp keeps mn finite, so
      // alpha and every p of such a row are exp2(-inf) = 0
      float mx = s[0][0];
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int i = 0; i < 16; ++i) mx = fmaxf(mx, s[kb][i]);
      mx = fmaxf(mx, other_half(mx));
      const float mn = fmaxf(fmaxf(m, mx * scale_log2e), -FLT_MAX);
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
    lse[((int64_t)b * Hq + h) * lse_stride + qrow] =
        (m + __builtin_amdgcn_logf(l)) * 0.6931471805599453f;

  // the loop's last barrier is behind every wave: K/V tiles are dead.  Each
  // wave owns [32 rows][8 chunks of 16 B], chunks swizzled like K.
  unsigned char* const Ow = lds + wave * (kRW * 128);
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
  uint16_t* op = out + ((int64_t)b * T * Hq + h) * 64;
#pragma unroll
  for (int pass = 0; pass < 4; ++pass) {  // a pass stores 8 whole rows
    int row = pass * 8 + (lane >> 3), ch = lane & 7;
    uint4 val = *reinterpret_cast<const uint4*>(Ow + k_off(row, ch));
    int qr = qw0 + row;
    if (qr < T)
      *reinterpret_cast<uint4*>(op + (int64_t)qr * Hq * 64 + 8 * ch) = val;
  }
}

}  // namespace

void hip_gqa_attn_fwd_doc_hd64(
    const void* q, const void* k, const void* v, const int32_t* doc_start,
    void* out, float* lse, int64_t B, int64_t Hq, int64_t Hkv, int64_t T,
    const int64_t* qs, const int64_t* ks, const int64_t* vs,
    int64_t lse_stride, float scale, hipStream_t s) {
  const char* op = "gqa_attn_fwd_doc_hd64";
  const FwdLaunch p = check_attn_fwd(op, q, k, v, out, lse, B, Hq, Hkv, T, qs,
                                     ks, vs, lse_stride, scale,
                                     /*grouped=*/true);
  if (!doc_start) throw std::runtime_error(std::string(op) + ": null pointer");
  check_align(doc_start, 4, op, "doc_start");
  auto launch = [&](auto kern) {
    kern<<<dim3((unsigned)p.grid), dim3(256), 0, s>>>(
        static_cast<const uint16_t*>(q), static_cast<const uint16_t*>(k),
        static_cast<const uint16_t*>(v), doc_start,
        static_cast<uint16_t*>(out), lse, (int)p.nbk, (int)Hkv, (int)p.G,
        (int)T, (int)p.nqb, strides3(qs), strides3(ks), strides3(vs),
        lse_stride, scale * kLog2e);
  };
  if (p.HW == 2)
    launch(k_gqa_fwd_doc_hd64<2>);
  else
    launch(k_gqa_fwd_doc_hd64<4>);
  HIP_CHECK(hipGetLastError());
}

}  // namespace shamd
