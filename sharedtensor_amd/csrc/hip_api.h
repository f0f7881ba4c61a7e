// Host-callable launchers for the CDNA4 codec kernels (hip_kernels.hip).
//
// Element-space contract (shared with codec_cpu.cpp / ops/oracle.py):
//   * values/delta buffers are the UNPADDED concatenation of the table's
//     tensors (offs[t] element starts, offs[T] = n).
//   * the packed payload lives in PADDED element space: tensor t occupies
//     padded elements [poffs[t], poffs[t+1]), poffs multiples of 64, so a
//     64-lane wavefront never straddles a tensor and __ballot packs one
//     uint64 word per wave (LSB-first layout identical to the reference's
//     byte stream, sharedtensor.c:166-177).
//   * scales: fp32[T] at the head of the message buffer; payload starts at
//     align8(4*T).
#pragma once

#include <hip/hip_runtime.h>

#include "common.h"

namespace shamd {

inline int64_t align8(int64_t x) { return (x + 7) & ~int64_t(7); }

struct DevTable {
  int64_t* offs = nullptr;    // device, T+1 unpadded element offsets
  int64_t* poffs = nullptr;   // device, T+1 padded element offsets
  int T = 0;
  int64_t n = 0;              // offs[T]
  int64_t pe = 0;             // poffs[T]
};

// Residual delta buffers are fp32 (delta_bf16=false) or bf16
// (delta_bf16=true, halves delta HBM for 100 GB-scale tensors; debit quanta
// are exactly representable in bf16).  `delta`/`d1..d3` pointers are typed
// accordingly (void* at this interface).

// reduce_buf: device scratch, >= 8*T bytes (double sumsq for 1bit,
// fp32 absmax for fp8/int4). scales_out: device fp32[T].
void hip_reduce_scales(Codec c, const void* delta, bool delta_bf16,
                       const DevTable& tb, void* reduce_buf, float* scales_out,
                       int sample_stride, hipStream_t s);

// delta is debited in place (atomic, lossless vs concurrent adds);
// payload receives the packed bytes for the whole padded space.
// stats_out (nullable, 8*T bytes): accumulate post-quantize residual
// statistics for lagged-scale mode (zero it before the call).
void hip_quantize(Codec c, void* delta, bool delta_bf16, const DevTable& tb,
                  const float* scales_dev, uint8_t* payload, hipStream_t s,
                  void* stats_out = nullptr);

// Finalize scales from an already-populated reduce/stats buffer (lagged
// mode: the buffer was filled by the previous round's quantize).
void hip_finalize_scales(Codec c, const DevTable& tb, const void* reduce_buf,
                         float* scales_out, int sample_stride, hipStream_t s);

// Decode payload and accumulate into the fp32 replica (values, nullable)
// plus up to two gossip-forward residual buffers (sharedtensor.c:106-127).
void hip_apply(Codec c, const uint8_t* payload, const DevTable& tb,
               const float* scales_dev, float* values, void* d1, void* d2,
               bool delta_bf16, hipStream_t s);

// {values, d1..d3} += alpha * src over the flat unpadded space
// (addFromInternal, sharedtensor.c:334-344; alpha=-1 implements the
// snapshot debit).
void hip_add_scatter(const float* src, int64_t n, float alpha, float* values,
                     void* d1, void* d2, void* d3, bool delta_bf16,
                     hipStream_t s);

// Fused join-snapshot capture: out := values (atomic 32-bit loads) and
// delta -= out in one pass; `out` is the authoritative sent-bytes buffer.
void hip_snapshot_capture(const float* values, void* delta, bool delta_bf16,
                          float* out, int64_t n, hipStream_t s);

// {values, d1, d2} += src_delta (delta-typed source; rejoin reconciliation).
void hip_add_delta_scatter(const void* src_delta, bool delta_bf16, int64_t n,
                           float* values, void* d1, void* d2, hipStream_t s);

// Fused SGD-momentum update feeding the shared tensor: m = mu*m + g;
// u = -lr*m; {values, link deltas} += u.  One pass over HBM instead of four.
void hip_fused_sgd(float* mom, const float* grad, float lr, float momentum,
                   int64_t n, float* values, void* d1, void* d2, void* d3,
                   bool delta_bf16, hipStream_t s,
                   const ClipState* clip = nullptr);

// Mixed-precision variant: bf16 grads in, fp32 master (values) updated,
// bf16 shadow params refreshed (folding concurrent gossip via the
// atomicAdd return), link deltas staged — all in one pass.
void hip_fused_sgd_bf16(float* mom, const uint16_t* grad, uint16_t* shadow,
                        float lr, float momentum, int64_t n, float* values,
                        void* d1, void* d2, void* d3, bool delta_bf16,
                        hipStream_t s, const ClipState* clip = nullptr);

// Fused AdamW feeding the shared tensor (torch.optim.AdamW semantics:
// decoupled weight decay on the pre-update weight): m/v fp32 state, grads
// fp32 or bf16, optional bf16 shadow refresh, update applied to values and
// staged into the link deltas — one HBM pass.  inv_bc* = 1/(1-beta*^t).
void hip_fused_adamw(float* mom, float* vel, const void* grad, bool grad_bf16,
                     uint16_t* shadow, float lr, float beta1, float beta2,
                     float eps, float wd, float inv_bc1, float inv_bc2,
                     int64_t n, float* values, void* d1, void* d2, void* d3,
                     bool delta_bf16, hipStream_t s,
                     const ClipState* clip = nullptr);

// Parameter-group variants (optim_group_kernels.hip).  `table` is the group
// table of common.h in device memory (build_group_table; never null here).
// Element i uses lr_eff = fl32(lr * lr_scale[g]), rounded once, wherever the
// ungrouped step uses lr, and weight_decay[g] for wd, g being the group of
// the segment that holds i; everything else, clip included, is the ungrouped
// step, and the results equal it bit for bit segment by segment.  SGD has
// no weight decay and reads lr_scale only.
void hip_fused_sgd_grouped(float* mom, const float* grad, float lr,
                           float momentum, int64_t n, float* values, void* d1,
                           void* d2, void* d3, bool delta_bf16, hipStream_t s,
                           const ClipState* clip, const void* table);
void hip_fused_sgd_bf16_grouped(float* mom, const uint16_t* grad,
                                uint16_t* shadow, float lr, float momentum,
                                int64_t n, float* values, void* d1, void* d2,
                                void* d3, bool delta_bf16, hipStream_t s,
                                const ClipState* clip, const void* table);
void hip_fused_adamw_grouped(float* mom, float* vel, const void* grad,
                             bool grad_bf16, uint16_t* shadow, float lr,
                             float beta1, float beta2, float eps,
                             float inv_bc1, float inv_bc2, int64_t n,
                             float* values, void* d1, void* d2, void* d3,
                             bool delta_bf16, hipStream_t s,
                             const ClipState* clip, const void* table);

// Global-norm gradient clipping (grad_clip_kernels.hip).  One read-only pass
// over grad (fp32, or bf16 with grad_bf16; aligned to its element size, any
// n >= 1) sums g*g in fp64 into one partial per block, a one-block kernel
// sums the partials in index order and writes *state (common.h ClipState):
// no atomics, so the state repeats bit for bit.  `scratch` holds
// GRAD_CLIP_MAX_BLOCKS doubles and needs no zeroing; `state` must be zeroed
// once before its first use (skipped_total is only ever incremented).  Both
// launches go to `s` with nothing in between.  Throws std::invalid_argument
// before any launch unless max_norm is finite and > 0.
//
// The fused optimizers above take that state as `clip` (device memory, may
// be null).  Null: the kernels and their results are what they are without
// clipping.  skip set: every thread returns before any load or store of
// mom, vel, values, shadow or the residuals.  Otherwise fl32(g * coef),
// rounded once and never contracted into the following FMA, stands wherever
// g stood; bf16 gradients are widened first and never rounded back.
void hip_grad_clip_coef(const void* grad, bool grad_bf16, int64_t n,
                        double max_norm, double* scratch, ClipState* state,
                        hipStream_t s);

// Fused bf16 LayerNorm for the training path (ln_kernels.hip): fwd saves
// fp32 mean/rstd; bwd = dx pass + register-accumulated dgamma/dbeta pass.
void hip_ln_fwd(const void* x, const void* w, const void* b, void* y,
                float* mean, float* rstd, int64_t R, int C, float eps,
                hipStream_t s);
void hip_ln_bwd(const void* dy, const void* x, const void* w,
                const float* mean, const float* rstd, void* dx, float* dgamma,
                float* dbeta, int64_t R, int C, hipStream_t s);

// Fused residual add + bf16 LayerNorm (add_ln_kernels.hip), wave per row,
// for C a multiple of 256 up to 1024 (hip_add_ln_supported).  All tensor
// pointers are bf16 and 8-byte aligned; mean/rstd/partial are fp32.
//   fwd: x_new = bf16(x + delta [+ dbias]); y = LN(x_new).  delta == null
//        means plain LN of x (x_new is not written, dbias must be null).
//   bwd: dx_total = LN_dx(dy) + d_x_new (null: no residual gradient), one
//        rounding; dgamma/dbeta/ddbias (null: not wanted) are written as
//        bf16 by a second kernel from per-block partials — no atomics.
//        `partial` holds hip_add_ln_max_blocks() * 3 * C floats, 16-byte
//        aligned, and needs no zeroing.
bool hip_add_ln_supported(int C);
int hip_add_ln_max_blocks();
void hip_add_ln_fwd(const void* x, const void* delta, const void* dbias,
                    const void* w, const void* b, void* x_new, void* y,
                    float* mean, float* rstd, int64_t R, int C, float eps,
                    hipStream_t s);
void hip_add_ln_bwd(const void* dy, const void* x_new, const void* w,
                    const float* mean, const float* rstd, const void* d_x_new,
                    void* dx_total, void* dgamma, void* dbeta, void* ddbias,
                    float* partial, int64_t R, int C, hipStream_t s);

// Column sum of (R, C) bf16 into fp32 out[C] (Linear backward bias grad);
// caller zeroes `out` first.
void hip_colsum_bf16(const void* x, float* out, int64_t R, int C,
                     hipStream_t s);

// Fused bf16 RMSNorm for the Llama training path (ln_kernels.hip): fwd
// saves fp32 rstd; bwd = single-reduction dx pass + register-accumulated
// dgamma pass.
void hip_rms_fwd(const void* x, const void* w, void* y, float* rstd,
                 int64_t R, int C, float eps, hipStream_t s);
void hip_rms_bwd(const void* dy, const void* x, const void* w,
                 const float* rstd, void* dx, float* dgamma, int64_t R, int C,
                 hipStream_t s);

// Fused residual add + bf16 RMSNorm (add_rms_kernels.hip), wave per row,
// for C a multiple of 512 up to 4096 (hip_add_rms_supported).  All tensor
// pointers are bf16 and 16-byte aligned; rstd/partial are fp32.  Both
// throw on an unsupported C or a misaligned pointer.
//   fwd: x_new = bf16(x + delta); y = x_new * rstd * w from the rounded
//        x_new.  delta == null means plain RMSNorm of x (x_new is not
//        written); delta without x_new throws.  R == 0 launches nothing.
//   bwd: dx_total = RMS_dx(dy) + d_x_new (null: no residual gradient), one
//        rounding; dgamma is written as bf16 by a second kernel from
//        per-block partials — no atomics, so it repeats bit for bit.
//        `partial` holds hip_add_rms_max_blocks() * C floats and needs no
//        zeroing.  R == 0 throws.
bool hip_add_rms_supported(int C);
int hip_add_rms_max_blocks();
void hip_add_rms_fwd(const void* x, const void* delta, const void* w,
                     void* x_new, void* y, float* rstd, int64_t R, int C,
                     float eps, hipStream_t s);
void hip_add_rms_bwd(const void* dy, const void* x_new, const void* w,
                     const float* rstd, const void* d_x_new, void* dx_total,
                     void* dgamma, float* partial, int64_t R, int C,
                     hipStream_t s);

// Fused bf16 cross-entropy (ce_kernels.hip), plain mean over the R rows; the
// targets are not checked.  Two-pass stats-only fwd saving per-row
// (max, lse); bwd writes bf16 dlogits = g*(softmax - onehot), or in
// skip_if_unit mode leaves the buffer alone when *gscale_dev == 1.
void hip_ce_fwd(const void* logits, const int32_t* targets, float* loss,
                float* row_m, float* row_lse, int64_t R, int64_t V,
                hipStream_t s);
void hip_ce_bwd(const void* logits, const int32_t* targets,
                const float* row_lse, void* dlogits, const float* gscale_dev,
                float inv_r, int64_t R, int64_t V, bool skip_if_unit,
                hipStream_t s);
// One-pass fwd + grad: one read of the logits gives loss, row_lse and the
// bf16 dlogits for an upstream gradient of 1 (inv_r = 1/R).  Throws when
// V > hip_ce_fwd_grad_max_v() (the row must fit one block's registers).
int64_t hip_ce_fwd_grad_max_v();
void hip_ce_fwd_grad(const void* logits, const int32_t* targets, float* loss,
                     float* row_lse, void* dlogits, float inv_r, int64_t R,
                     int64_t V, hipStream_t s);

// Fused cross-entropy with options: the same kernels (ce_kernels.hip) with a
// row policy that masks rows and takes 1/count from the device.  Row r is
// valid when targets[r] != ignore_index (if has_ignore) and
// 0 <= targets[r] < V.
// Per valid row:
//   loss_r = (1-eps)*(lse - x_t) + eps*(lse - mean_j x_j) + z*lse^2
//   dx_j   = g*inv_count*[(1 + 2*z*lse)*softmax_j - (1-eps)*[j==t] - eps/V]
// An ignored row is never read: loss_r = 0, row_lse = 0, dlogits row = +0.
// A row with an out-of-range target is treated the same except that its
// loss_r is NaN.
//
// Device state written by hip_ce_opts_scan and read by the other kernels
// from device memory (no host sync), 16 bytes:
struct CeOptState {
  float inv_count;   // 1.0f / n_valid, IEEE division (+inf when n_valid == 0)
  uint32_t n_valid;  // rows that count
  uint32_t n_bad;    // rows whose target is out of range and not ignored
  uint32_t pad;
};
struct CeOpts {
  int32_t ignore_index;
  bool has_ignore;
  float eps;  // label smoothing, [0, 1)
  float z;    // z-loss weight, >= 0
};
// one block, no atomics, fixed reduction order: bitwise reproducible
void hip_ce_opts_scan(const int32_t* targets, int64_t R, int64_t V,
                      const CeOpts& o, CeOptState* state, hipStream_t s);
// one-pass fwd + grad (upstream gradient 1); V <= hip_ce_fwd_grad_max_v()
void hip_ce_opts_fwd_grad(const void* logits, const int32_t* targets,
                          float* loss, float* row_lse, void* dlogits,
                          const CeOptState* state, const CeOpts& o, int64_t R,
                          int64_t V, hipStream_t s);
// stats-only forward (no_grad, or V beyond the register capacity)
void hip_ce_opts_fwd(const void* logits, const int32_t* targets, float* loss,
                     float* row_lse, const CeOpts& o, int64_t R, int64_t V,
                     hipStream_t s);
// full backward from logits and row_lse; skip_if_unit as hip_ce_bwd
void hip_ce_opts_bwd(const void* logits, const int32_t* targets,
                     const float* row_lse, void* dlogits,
                     const float* gscale_dev, const CeOptState* state,
                     const CeOpts& o, int64_t R, int64_t V, bool skip_if_unit,
                     hipStream_t s);

// Fused bf16 SwiGLU (swiglu_kernels.hip): y = silu(x1)*x3 one kernel each
// way; n must be a multiple of 8, buffers 16-byte aligned (uint4 loads).
void hip_swiglu_fwd(const void* x1, const void* x3, void* y, int64_t n,
                    hipStream_t s);
void hip_swiglu_bwd(const void* dy, const void* x1, const void* x3, void* dx1,
                    void* dx3, int64_t n, hipStream_t s);

// Fused bf16 RoPE for q and k in one launch (rope_kernels.hip).  q is
// logically (B, Hq, T, D) and k (B, Hkv, T, D), each side addressed by
// element strides for B, H, T with D contiguous; cos/sin are fp32 (>=T, D/2)
// row-major.  Pairs (2i, 2i+1) rotate by the angle at (t, i); `inverse`
// rotates by the negated angle (the gradient).  k == null rotates q alone.
// Throws on odd D or a null q/q_out/cos/sin.  16-byte accesses when D % 8
// == 0 and all bases/strides keep 16-byte alignment, pairs otherwise.
struct RopeStrides {
  int64_t b = 0, h = 0, t = 0;
};
void hip_rope_qk(const void* q, const void* k, void* q_out, void* k_out,
                 const float* cos, const float* sin, int64_t B, int64_t Hq,
                 int64_t Hkv, int64_t T, int64_t D, const RopeStrides& q_in,
                 const RopeStrides& k_in, const RopeStrides& q_os,
                 const RopeStrides& k_os, bool inverse, hipStream_t s);

// Fused bf16 GELU-tanh (gelu_kernels.hip); n must be a multiple of 8,
// buffers 16-byte aligned (uint4 loads).
void hip_gelu_fwd(const void* x, void* y, int64_t n, hipStream_t s);
void hip_gelu_bwd(const void* dy, const void* x, void* dx, int64_t n,
                  hipStream_t s);

// Bias gradients fused into the pass before them (bias_grad_kernels.hip).
// All tensors bf16 and 16-byte aligned, C a multiple of 8, R > 0; both throw
// otherwise.  `db` receives the bf16 column sums (fp32 accumulation of the
// bf16 values written, fixed order, no atomics); `partial` is fp32 scratch of
// hip_bias_grad_partial_floats(columns of the output) and needs no zeroing.
//   gelu_bwd_colsum: dx = bf16(dy * gelu'(x)) as hip_gelu_bwd, db[C] = column
//                    sums of dx.
//   pack3_colsum:    dst (R, 3C) = [s0 | s1 | s2], each (R, C) with row
//                    stride C; db[3C] = column sums of dst.
// hip_bias_grad_sweep_rows: rows one iteration of the grid's row loop covers
// for an (R, N) output of the GELU kernel or, with `pack`, of the pack kernel
// (tests size their grid-stride cases with it).
int64_t hip_bias_grad_partial_floats(int64_t N);
int64_t hip_bias_grad_sweep_rows(int64_t R, int64_t N, bool pack);
void hip_gelu_bwd_colsum(const void* dy, const void* x, void* dx, void* db,
                         float* partial, int64_t R, int64_t C, hipStream_t s);
void hip_pack3_colsum(const void* s0, const void* s1, const void* s2,
                      void* dst, void* db, float* partial, int64_t R,
                      int64_t C, hipStream_t s);

// Causal bf16 attention forward, head dim 64 (attn_kernels.hip).  q, k, v are
// read in place through element strides {batch, token, head} (each a
// multiple of 8, pointers 16-byte aligned, the 64 elements of a head
// contiguous); Tq == Tk == T, mask top-left aligned.  `out` is written as
// contiguous (B, T, H, 64) bf16; `lse` (B, H, lse_stride >= T) fp32 receives
// ln(sum exp(scale * score)) in its first T entries per row, the rest is left
// alone.  scale > 0.  Throws on anything else.
void hip_attn_fwd_causal_hd64(const void* q, const void* k, const void* v,
                              void* out, float* lse, int64_t B, int64_t H,
                              int64_t T, const int64_t* q_strides,
                              const int64_t* k_strides,
                              const int64_t* v_strides, int64_t lse_stride,
                              float scale, hipStream_t s);

// Split-K bf16 weight gradient dW[N, K] = dY[M, N]^T X[M, K]
// (wgrad_kernels.hip), fp32 accumulation.  ldy, ldx, ldw are row strides in
// elements (multiples of 8, pointers 16-byte aligned).  `variant` picks the
// tile (hip_wgrad_tile); N and K must be multiples of it and M of 64.  Each
// workgroup takes one tile and one of `split` contiguous ranges of 64-token
// steps; with split > 1 the partial tiles go as fp32 through `ws`
// (split * N * K floats, 16-byte aligned, written before it is read) and a
// second kernel sums them in split order: no atomics, the same bits on every
// call.  Runs on stream `s`.  Throws on anything else.
int hip_wgrad_num_variants();
void hip_wgrad_tile(int variant, int* tile_n, int* tile_k);
void hip_wgrad_bf16(const void* dy, const void* x, void* dw, float* ws,
                    int64_t ws_floats, int64_t M, int64_t N, int64_t K,
                    int64_t ldy, int64_t ldx, int64_t ldw, int64_t split,
                    int variant, hipStream_t s);

}  // namespace shamd
