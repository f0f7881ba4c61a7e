// Causal bf16 grouped-query attention forward for head dim 64 (Llama): Hq =
// G Hkv query heads, query head h reads kv head h / G, G in {2, 4, 8}.  The
// GQA counterpart of attn_kernels.hip: flash style, fp32 accumulation, bf16
// in and out, no dropout, no bias, top-left aligned causal mask (Tq == Tk).
//
// Plan (tests/test_gqa_attn_resource_usage.py holds the kernel to it):
//   * A wave is a query head.  workgroup = 4 waves = HW heads of one kv group
//     x 128 / HW consecutive query positions, HW = min(G, 4), a template
//     parameter:
//       - HW = 4 (G = 4, 8): wave w is head G kvh + 4 half + w, all four
//         waves own the same 32 positions; G = 8 takes two workgroups per kv
//         head and position block (half = 0, 1);
//       - HW = 2 (G = 2): waves 0-1 are head 2 kvh, waves 2-3 head 2 kvh + 1,
//         64 positions each, 32 per wave.
//     One K/V tile staged in LDS feeds HW heads, so per staged byte the
//     workgroup does the MFMA work of the MHA kernel, and staging traffic
//     and workgroup count equal those of MHA with Hq heads.  With HW = 4
//     every wave has the same causal extent: no wave idles through the
//     barriers of tiles above its rows.
//   * The per-wave code, the tiles, the grid map and the bounds checks are
//     the forward body's, described once in attn_fwd_tile.h; this file is
//     its <64, HW> case.
//   * Resources: amdgpu_waves_per_eu(4, 4): at most 128 VGPRs (128 as built
//     for HW = 2 and HW = 4), no AGPRs, no scratch, no spills, 32 KB of LDS
//     -> 4 waves/SIMD, the MHA forward's line.  No deviation from the plan.
//
// Whether this mapping is faster than the MHA kernel on expanded K/V rests
// on the argument above until benchmarks/bench_model_kernels.py has measured
// it (profiles/r12/).
#include <hip/hip_runtime.h>

#include "attn_fwd_tile.h"
#include "device_util.h"
#include "hip_api.h"

namespace shamd {
namespace {

// nbk = B * Hkv, nqb = position blocks of 128 / HW rows
template <int HW>
__global__ __launch_bounds__(256)
    __attribute__((amdgpu_waves_per_eu(4, 4))) void k_gqa_fwd_hd64(
    const uint16_t* __restrict__ q, const uint16_t* __restrict__ k,
    const uint16_t* __restrict__ v, uint16_t* __restrict__ out,
    float* __restrict__ lse, int nbk, int Hkv, int G, int T, int nqb,
    AttnStrides sq, AttnStrides sk, AttnStrides sv, int64_t lse_stride,
    float scale_log2e) {
  attn_fwd_body<64, HW>(q, k, v, out, lse, nbk, Hkv, G, T, nqb, sq, sk,
                        sv, lse_stride, scale_log2e);
}

}  // namespace

void hip_gqa_attn_fwd_causal_hd64(
    const void* q, const void* k, const void* v, void* out, float* lse,
    int64_t B, int64_t Hq, int64_t Hkv, int64_t T, const int64_t* qs,
    const int64_t* ks, const int64_t* vs, int64_t lse_stride, float scale,
    hipStream_t s) {
  const FwdLaunch p =
      check_attn_fwd("gqa_attn_fwd_causal_hd64", q, k, v, out, lse, B, Hq, Hkv, T, qs, ks, vs,
                     lse_stride, scale, /*grouped=*/true);
  auto launch = [&](auto kern) {
    kern<<<dim3((unsigned)p.grid), dim3(256), 0, s>>>(
        static_cast<const uint16_t*>(q), static_cast<const uint16_t*>(k),
        static_cast<const uint16_t*>(v), static_cast<uint16_t*>(out), lse,
        (int)p.nbk, (int)Hkv, (int)p.G, (int)T, (int)p.nqb, strides3(qs),
        strides3(ks), strides3(vs), lse_stride, scale * kLog2e);
  };
  if (p.HW == 2)
    launch(k_gqa_fwd_hd64<2>);
  else
    launch(k_gqa_fwd_hd64<4>);
  HIP_CHECK(hipGetLastError());
}

}  // namespace shamd
