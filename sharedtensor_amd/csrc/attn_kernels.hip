// Causal bf16 attention forward for head dim 64 (GPT-2): the G = 1, one head
// per workgroup case of the forward body in attn_fwd_tile.h, whose header
// describes the mechanics (tiles, swizzles, lane layouts, online softmax,
// staged epilogue).
//
// Plan (tests/test_attn_resource_usage.py holds the kernel to it):
//   * workgroup = 4 waves = 128 query rows of one (batch, head); a wave owns
//     32 rows.  KV tile = 64 keys, double-buffered: 2 x (8 KB + 8 KB) = 32 KB.
//   * The next tile's global loads are issued before the current tile's
//     MFMAs.  Issuing them after Q K^T instead measured the same (330.2
//     against 330.3 us, bit-equal results), so the simpler order stays.
//   * Grid: the query blocks of one (b, h) are consecutive on one XCD
//     (blockIdx % 8), heaviest (last) query block first, so K/V are re-read
//     from that XCD's L2.
//   * Resources: at most 128 VGPRs, no AGPRs, no scratch, no spills, 32 KB
//     of LDS -> 4 waves/SIMD, i.e. 4 workgroups per CU (LDS would allow 5).
#include <hip/hip_runtime.h>

#include "attn_fwd_tile.h"
#include "device_util.h"
#include "hip_api.h"

namespace shamd {
namespace {

// waves_per_eu(4, 4): the body fits 128 VGPRs without scratch; left alone the
// compiler takes 142 + AGPRs and halves the occupancy (measured 351 us at 2
// waves/SIMD, 335 us at 3, 330 us at 4 on the B=64 H=12 T=1024 shape).
__global__ __launch_bounds__(256)
    __attribute__((amdgpu_waves_per_eu(4, 4))) void k_attn_fwd_causal_hd64(
    const uint16_t* __restrict__ q, const uint16_t* __restrict__ k,
    const uint16_t* __restrict__ v, uint16_t* __restrict__ out,
    float* __restrict__ lse, int nbh, int H, int T, int nqb, AttnStrides sq,
    AttnStrides sk, AttnStrides sv, int64_t lse_stride, float scale_log2e) {
  attn_fwd_body<64, 1>(q, k, v, out, lse, nbh, H, 1, T, nqb, sq, sk, sv,
                       lse_stride, scale_log2e);
}

}  // namespace

void hip_attn_fwd_causal_hd64(const void* q, const void* k, const void* v,
                              void* out, float* lse, int64_t B, int64_t H,
                              int64_t T, const int64_t* qs, const int64_t* ks,
                              const int64_t* vs, int64_t lse_stride,
                              float scale, hipStream_t s) {
  const FwdLaunch p =
      check_attn_fwd("attn_fwd_causal_hd64", q, k, v, out, lse, B, H, H, T, qs,
                     ks, vs, lse_stride, scale, /*grouped=*/false);
  k_attn_fwd_causal_hd64<<<dim3((unsigned)p.grid), dim3(256), 0, s>>>(
      static_cast<const uint16_t*>(q), static_cast<const uint16_t*>(k),
      static_cast<const uint16_t*>(v), static_cast<uint16_t*>(out), lse,
      (int)p.nbk, (int)H, (int)T, (int)p.nqb, strides3(qs), strides3(ks),
      strides3(vs), lse_stride, scale * kLog2e);
  HIP_CHECK(hipGetLastError());
}

}  // namespace shamd
