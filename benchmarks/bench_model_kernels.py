#!/usr/bin/env python3
"""Microbenchmark the model-side fused kernels (LN, add+LN, GELU, RMSNorm,
add+RMSNorm, colsum, SwiGLU, RoPE, CE) vs their torch equivalents at the
GPT-2-small B=64 and llama-1B bench shapes.  `--only-rope` runs the RoPE
section alone, `--only-add-rms` the add+RMSNorm section, `--only-bias-grad`
the fused bias-gradient section, `--only-attn` the attention forward,
`--only-attn-bwd` the attention backward, `--only-gqa-attn` grouped-query
attention forward and backward, `--only-gqa-attn-hd128` grouped-query
attention at head dim 128, `--only-wgrad` the split-K weight-gradient
kernel, `--only-qkv-attn-bwd` the attention backward into the packed dqkv
with the bias-gradient epilogue, and the second-stage column reduce."""
import json
import sys
import time

import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from sharedtensor_amd import _core  # noqa: E402


def t(fn, iters=10, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3  # ms


def bench_rope(out):
    # ---- RoPE (llama-1B shape: B*T=16384, T=4096, 32 q + 8 kv heads, D=64)
    # fused q+k launch vs eager apply_rope on q and on k; effective TB/s
    # from the mandatory bytes: one read + one write of q and k per direction
    from sharedtensor_amd.models.llama import apply_rope, rope_freqs
    from sharedtensor_amd.ops import fused_rope
    Bq, Tq, Hq, Hkv, Dq = 4, 4096, 32, 8, 64
    rq = torch.randn(Bq, Tq, Hq, Dq, device="cuda").to(
        torch.bfloat16).transpose(1, 2).requires_grad_(True)
    rk = torch.randn(Bq, Tq, Hkv, Dq, device="cuda").to(
        torch.bfloat16).transpose(1, 2).requires_grad_(True)
    rgq = torch.randn(Bq, Hq, Tq, Dq, device="cuda").to(torch.bfloat16)
    rgk = torch.randn(Bq, Hkv, Tq, Dq, device="cuda").to(torch.bfloat16)
    rcos, rsin = rope_freqs(Dq, Tq, 500000.0, "cuda")
    assert fused_rope.can_use(rq, rk, rcos, rsin)
    rope_bytes = 2 * (rq.numel() + rk.numel()) * 2
    with torch.no_grad():
        ms = t(lambda: fused_rope.fused_rope_qk(rq, rk, rcos, rsin), iters=50)
    out["rope_fwd_ms"] = round(ms, 4)
    out["rope_fwd_tbps"] = round(rope_bytes / ms / 1e9, 2)
    ry = fused_rope.fused_rope_qk(rq, rk, rcos, rsin)
    ms = t(lambda: torch.autograd.grad(ry, (rq, rk), (rgq, rgk),
                                       retain_graph=True), iters=50)
    out["rope_bwd_ms"] = round(ms, 4)
    out["rope_bwd_tbps"] = round(rope_bytes / ms / 1e9, 2)
    with torch.no_grad():
        out["torch_rope_fwd_ms"] = round(t(lambda: (
            apply_rope(rq, rcos, rsin), apply_rope(rk, rcos, rsin)),
            iters=50), 4)
    ryt = (apply_rope(rq, rcos, rsin), apply_rope(rk, rcos, rsin))
    out["torch_rope_bwd_ms"] = round(t(lambda: torch.autograd.grad(
        ryt, (rq, rk), (rgq, rgk), retain_graph=True), iters=50), 4)


def bench_add_rms(out):
    # ---- fused add + RMSNorm vs the unfused sequence it replaces (llama-1B
    # C=2048 and llama-8B C=4096, R=16384).  effective TB/s = mandatory
    # bytes / time, with A = one (R, C) bf16 activation: forward must move
    # 4A (x, delta in; x_new, y out), backward 4A (dy, x_new, d_x_new in;
    # dx out).  Of the 8 the fused pair moves, 3 + 5 are reads and writes
    # the unfused sequence also pays for; it moves 13.
    s = torch.cuda.current_stream().cuda_stream
    R = 16384
    for C in (2048, 4096):
        A = R * C * 2
        x = torch.randn(R, C, device="cuda").to(torch.bfloat16)
        delta = torch.randn(R, C, device="cuda").to(torch.bfloat16)
        w = torch.randn(C, device="cuda").to(torch.bfloat16)
        dy = torch.randn(R, C, device="cuda").to(torch.bfloat16)
        dres = torch.randn(R, C, device="cuda").to(torch.bfloat16)
        x_new, y, dx = (torch.empty_like(x) for _ in range(3))
        dx2 = torch.empty_like(x)
        rstd = torch.empty(R, dtype=torch.float32, device="cuda")
        dg = torch.empty(C, dtype=torch.bfloat16, device="cuda")
        dg32 = torch.zeros(C, dtype=torch.float32, device="cuda")
        part = torch.empty(_core.add_rms_max_blocks() * C,
                           dtype=torch.float32, device="cuda")
        ms = t(lambda: _core.add_rms_fwd(
            x.data_ptr(), delta.data_ptr(), w.data_ptr(), x_new.data_ptr(),
            y.data_ptr(), rstd.data_ptr(), R, C, 1e-5, s), iters=30)
        out[f"add_rms{C}_fwd_ms"] = round(ms, 4)
        out[f"add_rms{C}_fwd_tbps"] = round(4 * A / ms / 1e9, 2)
        ms = t(lambda: _core.add_rms_bwd(
            dy.data_ptr(), x_new.data_ptr(), w.data_ptr(), rstd.data_ptr(),
            dres.data_ptr(), dx.data_ptr(), dg.data_ptr(), part.data_ptr(),
            R, C, s), iters=30)
        out[f"add_rms{C}_bwd_ms"] = round(ms, 4)
        out[f"add_rms{C}_bwd_tbps"] = round(4 * A / ms / 1e9, 2)

        def unfused_fwd():
            torch.add(x, delta, out=x_new)
            _core.rms_fwd(x_new.data_ptr(), w.data_ptr(), y.data_ptr(),
                          rstd.data_ptr(), R, C, 1e-5, s)

        def unfused_bwd():
            dg32.zero_()
            _core.rms_bwd(dy.data_ptr(), x_new.data_ptr(), w.data_ptr(),
                          rstd.data_ptr(), dx.data_ptr(), dg32.data_ptr(),
                          R, C, s)
            torch.add(dx, dres, out=dx2)
            dg32.to(torch.bfloat16)
        ms = t(unfused_fwd, iters=30)
        out[f"unfused_add_rms{C}_fwd_ms"] = round(ms, 4)
        out[f"unfused_add_rms{C}_fwd_tbps"] = round(4 * A / ms / 1e9, 2)
        ms = t(unfused_bwd, iters=30)
        out[f"unfused_add_rms{C}_bwd_ms"] = round(ms, 4)
        out[f"unfused_add_rms{C}_bwd_tbps"] = round(4 * A / ms / 1e9, 2)


def bench_bias_grad(out):
    # ---- bias gradients fused into GELU backward and the qkv gradient pack
    # (GPT-2-small B=64: R=65536, fc C=3072, qkv 3 x 768) against the torch
    # kernels they replace.  Both sides include the bias reduce.  Effective
    # TB/s from the mandatory bytes: GELU backward reads dy and x and writes
    # dx (3A); the pack reads and writes 3 x (R, 768) (2A').
    s = torch.cuda.current_stream().cuda_stream
    R, C = 65536, 3072
    x = (torch.randn(R, C, device="cuda") * 2).to(torch.bfloat16)
    dy = torch.randn(R, C, device="cuda").to(torch.bfloat16)
    dx = torch.empty_like(x)
    db = torch.empty(C, dtype=torch.bfloat16, device="cuda")
    part = torch.empty(_core.bias_grad_partial_floats(C),
                       dtype=torch.float32, device="cuda")
    ms = t(lambda: _core.gelu_bwd_colsum(
        dy.data_ptr(), x.data_ptr(), dx.data_ptr(), db.data_ptr(),
        part.data_ptr(), R, C, s), iters=30)
    out["gelu_bwd_colsum_ms"] = round(ms, 4)
    out["gelu_bwd_colsum_tbps"] = round(3 * x.numel() * 2 / ms / 1e9, 2)
    xt = x.clone().requires_grad_(True)
    yt = torch.nn.functional.gelu(xt, approximate="tanh")

    def torch_gelu_bwd():
        (g,) = torch.autograd.grad(yt, xt, dy, retain_graph=True)
        return g.sum(0)
    ms = t(torch_gelu_bwd, iters=30)
    out["torch_gelu_bwd_plus_reduce_ms"] = round(ms, 4)
    out["torch_gelu_bwd_plus_reduce_tbps"] = round(
        3 * x.numel() * 2 / ms / 1e9, 2)

    Cq = 768
    srcs = [torch.randn(R, Cq, device="cuda").to(torch.bfloat16)
            for _ in range(3)]
    dst = torch.empty(R, 3 * Cq, dtype=torch.bfloat16, device="cuda")
    dbq = torch.empty(3 * Cq, dtype=torch.bfloat16, device="cuda")
    ms = t(lambda: _core.pack3_colsum(
        srcs[0].data_ptr(), srcs[1].data_ptr(), srcs[2].data_ptr(),
        dst.data_ptr(), dbq.data_ptr(), part.data_ptr(), R, Cq, s), iters=30)
    out["pack3_colsum_ms"] = round(ms, 4)
    out["pack3_colsum_tbps"] = round(2 * dst.numel() * 2 / ms / 1e9, 2)
    ms = t(lambda: torch.cat(srcs, dim=1).sum(0), iters=30)
    out["torch_cat_plus_reduce_ms"] = round(ms, 4)
    out["torch_cat_plus_reduce_tbps"] = round(
        2 * dst.numel() * 2 / ms / 1e9, 2)
    # the parts on their own, for the README
    out["torch_cat_ms"] = round(t(lambda: torch.cat(srcs, dim=1), iters=30), 4)
    out["torch_reduce2304_ms"] = round(t(lambda: dst.sum(0), iters=30), 4)
    out["torch_reduce3072_ms"] = round(t(lambda: dx.sum(0), iters=30), 4)


def bench_attn(out, rounds=7, iters=20):
    # ---- causal attention forward at the GPT-2-small B=64 shape (H=12,
    # T=1024, D=64) on the strided q, k, v views of a packed (B, T, 3C)
    # buffer: our kernel against the aten efficient-attention forward.  Arms
    # interleaved round by round, device-event timed; median and range over
    # the rounds.  103 GFLOP (causal half of 4 B H T^2 D) and 0.4 GB
    # (q, k, v, out once) per call.
    from torch.nn.attention import SDPBackend, sdpa_kernel
    from sharedtensor_amd.ops import fused_attn
    B, H, T, D = 64, 12, 1024, 64
    C = H * D
    qkv = torch.randn(B, T, 3 * C, device="cuda").to(torch.bfloat16)
    q, k, v = (x.view(B, T, H, D).transpose(1, 2)
               for x in qkv.split(C, dim=2))
    assert fused_attn.can_use(q, k, v)
    o = torch.empty(B, T, H, D, dtype=torch.bfloat16, device="cuda")
    lse = torch.empty(B, H, T, dtype=torch.float32, device="cuda")
    pri = [SDPBackend.EFFICIENT_ATTENTION, SDPBackend.FLASH_ATTENTION,
           SDPBackend.MATH]

    def aten():
        with sdpa_kernel(pri, set_priority=True):
            return torch.ops.aten._scaled_dot_product_efficient_attention(
                q, k, v, None, True, 0.0, True)

    arms = {"aten_efficient_attn_fwd": aten,
            "fused_attn_fwd": lambda: fused_attn.attn_forward(
                q, k, v, out=o, lse=lse)}

    def timed(fn):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    for fn in arms.values():
        timed(fn)
    ms = {n: [] for n in arms}
    for _ in range(rounds):
        for n, fn in arms.items():
            ms[n].append(timed(fn))
    flop = 4 * B * H * T * T * D / 2
    byts = 4 * B * H * T * D * 2
    out["attn_shape"] = dict(B=B, H=H, T=T, D=D, rounds=rounds, iters=iters)
    for n, xs in ms.items():
        xs = sorted(xs)
        med = xs[len(xs) // 2]
        out[n + "_ms_median"] = round(med, 4)
        out[n + "_ms_range"] = [round(xs[0], 4), round(xs[-1], 4)]
        out[n + "_tflops"] = round(flop / med / 1e9, 1)
        out[n + "_tbps"] = round(byts / med / 1e9, 2)


def bench_attn_bwd(out, rounds=7, iters=20):
    # ---- causal attention backward at the same shape and layout: our two
    # kernels (attn_backward) against the aten efficient-attention backward,
    # both fed the out and lse of our forward.  Arms interleaved round by
    # round, device-event timed; median and range over the rounds.  258 GFLOP
    # (causal half of five B H T^2 D products) and 0.8 GB (q, k, v, out, dout
    # read and dq, dk, dv written once) per call.
    from torch.nn.attention import SDPBackend, sdpa_kernel
    from sharedtensor_amd.ops import fused_attn
    B, H, T, D = 64, 12, 1024, 64
    C = H * D
    qkv = torch.randn(B, T, 3 * C, device="cuda").to(torch.bfloat16)
    q, k, v = (x.view(B, T, H, D).transpose(1, 2)
               for x in qkv.split(C, dim=2))
    dout = torch.randn(B, T, H, D, device="cuda").to(
        torch.bfloat16).transpose(1, 2)
    o, lse = fused_attn.attn_forward(q, k, v)
    o = o.transpose(1, 2)
    assert fused_attn.can_use_backward(q, k, v, o, lse, dout)
    grads = [torch.empty(B, T, H, D, dtype=torch.bfloat16,
                         device="cuda").transpose(1, 2) for _ in range(3)]
    delta = torch.empty(B, H, T, dtype=torch.float32, device="cuda")
    seed, offset = fused_attn._philox_state()
    pri = [SDPBackend.EFFICIENT_ATTENTION, SDPBackend.FLASH_ATTENTION,
           SDPBackend.MATH]
    bwd = torch.ops.aten._scaled_dot_product_efficient_attention_backward

    def aten():
        with sdpa_kernel(pri, set_priority=True):
            return bwd(dout, q, k, v, None, o, lse, seed, offset, 0.0,
                       [True, True, True, False], True)

    arms = {"aten_efficient_attn_bwd": aten,
            "fused_attn_bwd": lambda: fused_attn.attn_backward(
                q, k, v, o, lse, dout, None, *grads, delta=delta)}

    def timed(fn):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    for fn in arms.values():
        timed(fn)
    ms = {n: [] for n in arms}
    for _ in range(rounds):
        for n, fn in arms.items():
            ms[n].append(timed(fn))
    flop = 10 * B * H * T * T * D / 2
    byts = 8 * B * H * T * D * 2
    out["attn_bwd_shape"] = dict(B=B, H=H, T=T, D=D, rounds=rounds,
                                 iters=iters)
    for n, xs in ms.items():
        xs = sorted(xs)
        med = xs[len(xs) // 2]
        out[n + "_ms_median"] = round(med, 4)
        out[n + "_ms_range"] = [round(xs[0], 4), round(xs[-1], 4)]
        out[n + "_tflops"] = round(flop / med / 1e9, 1)
        out[n + "_tbps"] = round(byts / med / 1e9, 2)
    out["fused_median_below_aten_min"] = bool(
        out["fused_attn_bwd_ms_median"]
        < out["aten_efficient_attn_bwd_ms_range"][0])
    # repeats of the fused arm are bit-identical
    first = [g.clone() for g in grads]
    arms["fused_attn_bwd"]()
    torch.cuda.synchronize()
    out["fused_repeat_bit_equal"] = all(
        torch.equal(a, b) for a, b in zip(first, grads))


def bench_gqa_attn(out, rounds=7, iters=20):
    # ---- causal grouped-query attention, forward and backward, at the
    # profile's Llama-1B shape (B=8, T=2048) and at the shape
    # `bench.py --model llama1b` runs by default (B=64, T=1024); Hq=32,
    # Hkv=8, D=64, q/k/v in the model's layout.  Three arms, interleaved round
    # by round, device-event timed, median and range over the rounds:
    #   sdpa  the SDPA enable_gqa call the model makes (the parent); its
    #         backward is timed as forward + backward minus forward
    #   gqa   the new kernels (ops/fused_gqa_attn.py)
    #   mha   the MHA kernels (ops/fused_attn.py) on repeat_interleave'd K/V;
    #         the expansion (and, backward, the group sum of dk and dv) is
    #         timed on its own as `expand`
    # FLOP: the causal half of 2 (forward) or 5 (backward) B Hq T^2 D products.
    import torch.nn.functional as F
    from torch.nn.attention import SDPBackend, sdpa_kernel
    from sharedtensor_amd.ops import fused_attn, fused_gqa_attn
    pri = [SDPBackend.EFFICIENT_ATTENTION, SDPBackend.FLASH_ATTENTION,
           SDPBackend.MATH]
    Hq, Hkv, D = 32, 8, 64
    G = Hq // Hkv

    def timed(fn):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    for B, T in ((8, 2048), (64, 1024)):
        mk = lambda h: torch.randn(B, T, h, D, device="cuda").to(
            torch.bfloat16).transpose(1, 2)
        q, k, v, dout = mk(Hq), mk(Hkv), mk(Hkv), mk(Hq)
        assert fused_gqa_attn.can_use(q, k, v)
        o, lse = fused_gqa_attn.gqa_forward(q, k, v)
        ot = o.transpose(1, 2)
        ke, ve = (x.repeat_interleave(G, dim=1) for x in (k, v))
        gq, gke, gve = (torch.empty_like(q) for _ in range(3))
        gk, gv = torch.empty_like(k), torch.empty_like(v)
        delta = torch.empty(B, Hq, T, dtype=torch.float32, device="cuda")
        qr, kr, vr = (x.detach().clone().requires_grad_() for x in (q, k, v))

        def sdpa(x=q, y=k, z=v):
            with sdpa_kernel(pri, set_priority=True):
                return F.scaled_dot_product_attention(x, y, z, is_causal=True,
                                                      enable_gqa=True)

        def sdpa_fwd_bwd():
            sdpa(qr, kr, vr).backward(dout)
            qr.grad = kr.grad = vr.grad = None

        def expand_bwd():
            for x in (k, v):
                x.repeat_interleave(G, dim=1)
            for x in (gke, gve):
                x.view(B, Hkv, G, T, D).sum(2)

        arms = {
            "fwd_sdpa": sdpa,
            "fwd_gqa": lambda: fused_gqa_attn.gqa_forward(q, k, v, out=o,
                                                          lse=lse),
            "fwd_mha": lambda: fused_attn.attn_forward(q, ke, ve, out=o,
                                                       lse=lse),
            "fwd_expand": lambda: [x.repeat_interleave(G, dim=1)
                                   for x in (k, v)],
            "fwdbwd_sdpa": sdpa_fwd_bwd,
            "bwd_gqa": lambda: fused_gqa_attn.gqa_backward(
                q, k, v, ot, lse, dout, None, gq, gk, gv, delta=delta),
            "bwd_mha": lambda: fused_attn.attn_backward(
                q, ke, ve, ot, lse, dout, None, gq, gke, gve, delta=delta),
            "bwd_expand": expand_bwd,
        }
        for fn in arms.values():
            timed(fn)
        ms = {n: [] for n in arms}
        for _ in range(rounds):
            for n, fn in arms.items():
                ms[n].append(timed(fn))
        ms["bwd_sdpa"] = [a - b for a, b in zip(ms["fwdbwd_sdpa"],
                                                ms["fwd_sdpa"])]
        flop = B * Hq * T * T * D
        rec = dict(B=B, Hq=Hq, Hkv=Hkv, T=T, D=D, rounds=rounds, iters=iters)
        for n, xs in ms.items():
            xs = sorted(xs)
            med = xs[len(xs) // 2]
            rec[n] = dict(ms_median=round(med, 4),
                          ms_range=[round(xs[0], 4), round(xs[-1], 4)])
            if "expand" not in n:
                mult = {"fwd": 2, "bwd": 5, "fwdbwd": 7}[n.split("_")[0]]
                rec[n]["tflops"] = round(mult * flop / med / 1e9, 1)
        out[f"gqa_attn_B{B}_T{T}"] = rec


def bench_gqa_attn_hd128(out, rounds=7, iters=20):
    # ---- causal grouped-query attention at head dim 128 (Llama-3-8B: Hq=32,
    # Hkv=8), q/k/v in the model's layout, at (B, T) = (8, 2048) and
    # (2, 8192).  Arms interleaved round by round, device-event timed, median
    # and range over the rounds:
    #   fwd_sdpa       the SDPA enable_gqa call the model makes (the parent)
    #   fwd_gqa128     csrc/gqa_attn_hd128_kernels.hip
    #   fwdbwd_sdpa    forward + backward of the SDPA call through autograd
    #   fwdbwd_gqa128  forward + backward of fused_causal_gqa_attention: our
    #                  forward, K/V expansion, the aten backward, the group sum
    #   bwd_aten128    the backward alone of that path, fed our forward's out
    #                  and lse: K/V expansion, the aten backward, the group sums
    #   bwd_gqa128     csrc/gqa_attn_hd128_bwd_kernels.hip on the same inputs
    # FLOP: the causal half of 2 (forward), 5 (backward) or 7 (both)
    # B Hq T^2 D products.
    import torch.nn.functional as F
    from torch.nn.attention import SDPBackend, sdpa_kernel
    from sharedtensor_amd.ops import fused_gqa_attn
    from sharedtensor_amd.ops.fused_attn import _philox_state
    pri = [SDPBackend.EFFICIENT_ATTENTION, SDPBackend.FLASH_ATTENTION,
           SDPBackend.MATH]
    Hq, Hkv, D = 32, 8, 128
    G = Hq // Hkv

    def timed(fn):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    for B, T in ((8, 2048), (2, 8192)):
        mk = lambda h: torch.randn(B, T, h, D, device="cuda").to(
            torch.bfloat16).transpose(1, 2)
        q, k, v, dout = mk(Hq), mk(Hkv), mk(Hkv), mk(Hq)
        assert fused_gqa_attn.can_use(q, k, v)
        o, lse = fused_gqa_attn.gqa_forward(q, k, v)
        qr, kr, vr = (x.detach().clone().requires_grad_() for x in (q, k, v))

        def sdpa(x=q, y=k, z=v):
            with sdpa_kernel(pri, set_priority=True):
                return F.scaled_dot_product_attention(x, y, z, is_causal=True,
                                                      enable_gqa=True)

        def fwd_bwd(fn):
            def run():
                fn(qr, kr, vr).backward(dout)
                qr.grad = kr.grad = vr.grad = None
            return run

        ot = o.transpose(1, 2)
        gq, gk, gv = (torch.empty_like(x) for x in (q, k, v))
        delta = torch.empty(B, Hq, T, dtype=torch.float32, device="cuda")
        seed, offset = _philox_state()

        def bwd_aten():  # _FusedCausalGqaAttnHd128.backward
            ke, ve = (x.repeat_interleave(G, dim=1) for x in (k, v))
            with sdpa_kernel(pri, set_priority=True):
                _, dk, dv, _ = torch.ops.aten.\
                    _scaled_dot_product_efficient_attention_backward(
                        dout, q, ke, ve, None, ot, lse, seed, offset, 0.0,
                        [True, True, True, False], True, scale=D ** -0.5)
            for x in (dk, dv):
                x.unflatten(1, (Hkv, G)).sum(2)

        arms = {
            "fwd_sdpa": sdpa,
            "fwd_gqa128": lambda: fused_gqa_attn.gqa_forward(q, k, v, out=o,
                                                             lse=lse),
            "fwdbwd_sdpa": fwd_bwd(sdpa),
            "fwdbwd_gqa128": fwd_bwd(fused_gqa_attn.fused_causal_gqa_attention),
            "bwd_aten128": bwd_aten,
            "bwd_gqa128": lambda: fused_gqa_attn.gqa_backward_hd128(
                q, k, v, ot, lse, dout, None, gq, gk, gv, delta=delta),
        }
        for fn in arms.values():
            timed(fn)
        ms = {n: [] for n in arms}
        for _ in range(rounds):
            for n, fn in arms.items():
                ms[n].append(timed(fn))
        flop = B * Hq * T * T * D
        rec = dict(B=B, Hq=Hq, Hkv=Hkv, T=T, D=D, rounds=rounds, iters=iters)
        for n, xs in ms.items():
            xs = sorted(xs)
            med = xs[len(xs) // 2]
            mult = {"fwd": 2, "bwd": 5, "fwdbwd": 7}[n.split("_")[0]]
            rec[n] = dict(ms_median=round(med, 4),
                          ms_range=[round(xs[0], 4), round(xs[-1], 4)],
                          tflops=round(mult * flop / med / 1e9, 1))
        rec["fwdbwd_gqa128_wholly_below_sdpa"] = (
            rec["fwdbwd_gqa128"]["ms_range"][1]
            < rec["fwdbwd_sdpa"]["ms_range"][0])
        rec["bwd_gqa128_wholly_below_aten128"] = (
            rec["bwd_gqa128"]["ms_range"][1]
            < rec["bwd_aten128"]["ms_range"][0])
        out[f"gqa_attn_hd128_B{B}_T{T}"] = rec


def bench_gqa_attn_doc(out, rounds=7, iters=20):
    # ---- document-masked grouped-query attention (packed batches) at B=64,
    # Hq=32, Hkv=8, T=1024, D=64, q/k/v in the model's layout.  All arms in
    # one interleaved, device-event timed run:
    #   plain      the plain causal kernels (no document mask)
    #   idle       the document kernels with one document per row: what the
    #              mask machinery costs when it has nothing to mask
    #   doc        the document kernels, documents of mean length 256
    #   sdpa_mask  SDPA with the dense (B, 1, T, T) boolean mask of the same
    #              documents, the route a packed batch had before; its
    #              backward is forward + backward minus forward
    # `doc_below_sdpa_mask`: the doc arm's forward + backward range lies
    # wholly below the SDPA arm's, the condition of llama.FUSE_GQA_ATTN_DOC.
    import torch.nn.functional as F
    from torch.nn.attention import SDPBackend, sdpa_kernel
    from sharedtensor_amd.ops import fused_gqa_attn as fg
    pri = [SDPBackend.EFFICIENT_ATTENTION, SDPBackend.FLASH_ATTENTION,
           SDPBackend.MATH]
    B, Hq, Hkv, T, D = 64, 32, 8, 1024, 64
    mk = lambda h: torch.randn(B, T, h, D, device="cuda").to(
        torch.bfloat16).transpose(1, 2)
    q, k, v, dout = mk(Hq), mk(Hkv), mk(Hkv), mk(Hq)
    gen = torch.Generator().manual_seed(0)
    ids = torch.zeros(B, T, dtype=torch.long)
    for b in range(B):  # lengths uniform in 1..511: mean 256
        cuts = torch.randint(1, 512, (T,), generator=gen).cumsum(0)
        ids[b] = torch.bucketize(torch.arange(T), cuts, right=True)
    ids = ids.cuda()
    one = fg.doc_start_end(torch.zeros_like(ids))
    many = fg.doc_start_end(ids)
    mask = ((ids[:, :, None] == ids[:, None, :])
            & torch.ones(T, T, device="cuda", dtype=torch.bool).tril())[:, None]
    o, lse = fg.gqa_forward(q, k, v)
    ot = o.transpose(1, 2)
    gq, gk, gv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    delta = torch.empty(B, Hq, T, dtype=torch.float32, device="cuda")
    qr, kr, vr = (x.detach().clone().requires_grad_() for x in (q, k, v))

    def sdpa(x=q, y=k, z=v):
        with sdpa_kernel(pri, set_priority=True):
            return F.scaled_dot_product_attention(x, y, z, attn_mask=mask,
                                                  enable_gqa=True)

    def sdpa_fwd_bwd():
        sdpa(qr, kr, vr).backward(dout)
        qr.grad = kr.grad = vr.grad = None

    def fwd(doc):
        return lambda: fg.gqa_forward(q, k, v, out=o, lse=lse,
                                      doc_start=doc and doc[0])

    def bwd(doc):
        kw = dict(doc_start=doc[0], doc_end=doc[1]) if doc else {}
        return lambda: fg.gqa_backward(q, k, v, ot, lse, dout, None, gq, gk,
                                       gv, delta=delta, **kw)

    # the timed backwards read the plain forward's out and lse: the work per
    # tile does not depend on the values
    ms = _interleaved({
        "fwd_plain": fwd(None), "fwd_idle": fwd(one), "fwd_doc": fwd(many),
        "fwd_sdpa_mask": sdpa,
        "bwd_plain": bwd(None), "bwd_idle": bwd(one), "bwd_doc": bwd(many),
        "fwdbwd_sdpa_mask": sdpa_fwd_bwd}, rounds, iters)
    ms["fwdbwd_doc"] = sorted(a + b for a, b in zip(ms["fwd_doc"],
                                                    ms["bwd_doc"]))
    rec = dict(B=B, Hq=Hq, Hkv=Hkv, T=T, D=D, rounds=rounds, iters=iters,
               docs_per_row=round((ids.max(1).values + 1).float().mean().item(),
                                  2))
    for n, xs in ms.items():
        rec[n] = dict(ms_median=round(xs[len(xs) // 2], 4),
                      ms_range=[round(xs[0], 4), round(xs[-1], 4)])
    rec["doc_below_sdpa_mask"] = bool(
        ms["fwdbwd_doc"][-1] < ms["fwdbwd_sdpa_mask"][0])
    out[f"gqa_attn_doc_B{B}_T{T}"] = rec


def _interleaved(arms, rounds, iters):
    """Device-event time per call of each arm: one warm pass, then `rounds`
    rounds of `iters` calls, arms interleaved.  {arm: sorted ms}."""
    def timed(fn):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    for fn in arms.values():
        timed(fn)
    ms = {n: [] for n in arms}
    for _ in range(rounds):
        for n, fn in arms.items():
            ms[n].append(timed(fn))
    return {n: sorted(xs) for n, xs in ms.items()}


def bench_qkv_attn_bwd(out, rounds=7, iters=20):
    # ---- attention backward up to the packed dqkv and qkv.bias.grad at
    # B=64 H=12 T=1024.  Parent arm: attn_backward into three separate
    # (B, T, H, 64) buffers, then pack3_colsum.  Branch arm: attn_backward
    # into the three views of dqkv with the column-sum epilogue, then
    # k_colsum_reduce (inside the same call).  "plain" is attn_backward alone
    # into separate buffers: branch minus plain is what the epilogue, the
    # packed stores and the reduce cost together.
    from sharedtensor_amd.ops import fused_attn
    B, H, T, D = 64, 12, 1024, 64
    C = H * D
    s = torch.cuda.current_stream().cuda_stream
    qkv = torch.randn(B, T, 3 * C, device="cuda").to(torch.bfloat16)
    q, k, v = fused_attn._heads(qkv, H)
    dout = torch.randn(B, T, H, D, device="cuda").to(
        torch.bfloat16).transpose(1, 2)
    o, lse = fused_attn.attn_forward(q, k, v)
    o = o.transpose(1, 2)
    sep = [torch.empty(B, T, H, D, dtype=torch.bfloat16, device="cuda")
           for _ in range(3)]
    sep_v = [g.transpose(1, 2) for g in sep]
    delta = torch.empty(B, H, T, dtype=torch.float32, device="cuda")
    dqkv_p = torch.empty(B, T, 3 * C, dtype=torch.bfloat16, device="cuda")
    dqkv_b = torch.empty_like(dqkv_p)
    db_p = torch.empty(3 * C, dtype=torch.bfloat16, device="cuda")
    db_b = torch.empty_like(db_p)
    part_p = torch.empty(_core.bias_grad_partial_floats(3 * C),
                         dtype=torch.float32, device="cuda")
    part_b = torch.empty(_core.attn_bwd_colsum_floats(B, H, T),
                         dtype=torch.float32, device="cuda")
    views = fused_attn._heads(dqkv_b, H)

    def plain():
        fused_attn.attn_backward(q, k, v, o, lse, dout, None, *sep_v,
                                 delta=delta)

    def parent():
        plain()
        _core.pack3_colsum(sep[0].data_ptr(), sep[1].data_ptr(),
                           sep[2].data_ptr(), dqkv_p.data_ptr(),
                           db_p.data_ptr(), part_p.data_ptr(), B * T, C, s)

    def branch():
        fused_attn.attn_backward(q, k, v, o, lse, dout, None, *views,
                                 delta=delta, partial=part_b, db=db_b)

    ms = _interleaved({"parent_attn_bwd_pack3": parent,
                       "branch_attn_bwd_packed": branch,
                       "plain_attn_bwd": plain}, rounds, iters)
    out["qkv_attn_bwd_shape"] = dict(B=B, H=H, T=T, D=D, rounds=rounds,
                                     iters=iters)
    for n, xs in ms.items():
        out[n + "_ms_median"] = round(xs[len(xs) // 2], 4)
        out[n + "_ms_range"] = [round(xs[0], 4), round(xs[-1], 4)]
    out["branch_max_below_parent_min"] = bool(
        ms["branch_attn_bwd_packed"][-1] < ms["parent_attn_bwd_pack3"][0])
    torch.cuda.synchronize()
    out["dqkv_bit_equal"] = bool(torch.equal(dqkv_p, dqkv_b))
    out["db_max_abs_diff"] = float((db_p.float() - db_b.float()).abs().max())

    # ---- the second-stage column reduce against k_add_ln_reduce on the
    # add+LayerNorm partials: G = 1024 rows of 3 C (with proj-bias grad) and
    # 2 C (without) floats, C = 768
    G = 1024
    for nsc in (2304, 1536):
        part = torch.randn(G * nsc, device="cuda")
        o_old = torch.empty(3, C, dtype=torch.bfloat16, device="cuda")
        o_new = torch.empty_like(o_old)
        third = nsc == 3 * C

        def old():
            _core.add_ln_reduce(part.data_ptr(), G, nsc, C,
                                o_old[0].data_ptr(), o_old[1].data_ptr(),
                                o_old[2].data_ptr() if third else 0, s)

        def new():
            _core.colsum_reduce(part.data_ptr(), G, nsc, C,
                                o_new[0].data_ptr(), o_new[1].data_ptr(),
                                o_new[2].data_ptr() if third else 0, s)

        ms = _interleaved({"k_add_ln_reduce": old, "k_colsum_reduce": new},
                          rounds, 10 * iters)
        for n, xs in ms.items():
            key = f"{n}_G{G}_N{nsc}"
            out[key + "_us_median"] = round(1e3 * xs[len(xs) // 2], 2)
            out[key + "_us_range"] = [round(1e3 * xs[0], 2),
                                      round(1e3 * xs[-1], 2)]
        out[f"colsum_reduce_max_below_add_ln_min_N{nsc}"] = bool(
            ms["k_colsum_reduce"][-1] < ms["k_add_ln_reduce"][0])
        rows = 3 if third else 2
        out[f"reduce_max_abs_diff_N{nsc}"] = float(
            (o_old[:rows].float() - o_new[:rows].float()).abs().max())


def load_tunableop():
    """The checked-in TunableOp GEMM table, loaded as bench.py loads it."""
    import os
    import torch.cuda.tunable as tunable
    fn = os.path.join(__file__.rsplit("/", 2)[0], "sharedtensor_amd",
                      "tunableop_gfx950.csv")
    tunable.enable(True)
    tunable.tuning_enable(False)
    tunable.read_file(fn)


def bench_wgrad(out, rounds=7, iters=20, sweep=False):
    # ---- dW = dY^T X of the four GPT-2-small layer Linears at M = 65536
    # tokens: our split-K kernel plus its reduce pass against torch.mm with
    # the tuned GEMM table.  Arms interleaved round by round, device-event
    # timed; median and range over the rounds.  `--sweep` adds every kernel
    # variant at 1 to 3 workgroups per CU.
    from sharedtensor_amd.ops import fused_wgrad as fw
    load_tunableop()
    M = 65536
    shapes = {"attn_qkv": (2304, 768), "attn_proj": (768, 768),
              "mlp_fc": (3072, 768), "mlp_proj": (768, 3072)}

    def timed(fn):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    out["wgrad_setup"] = dict(M=M, rounds=rounds, iters=iters)
    for name, (N, K) in shapes.items():
        dy = torch.randn(M, N, device="cuda").to(torch.bfloat16)
        x = torch.randn(M, K, device="cuda").to(torch.bfloat16)
        dw = torch.empty(N, K, dtype=torch.bfloat16, device="cuda")
        dyt = dy.t()
        arms = {"torch_mm": lambda: torch.mm(dyt, x, out=dw)}
        variant = fw.TUNED.get((N, K), fw.DEFAULT_VARIANT)
        arms["fused"] = lambda v=variant: fw.wgrad(dy, x, out=dw, variant=v)
        if sweep:
            for v, (tn, tk, _) in fw.VARIANTS.items():
                tiles = (N // tn) * (K // tk)
                for per_cu in (1, 2, 3):
                    sp = fw.choose_split(tiles, M // fw.STEP, per_cu)
                    arms[f"fused_v{v}_split{sp}"] = \
                        lambda v=v, sp=sp: fw.wgrad(dy, x, out=dw, variant=v,
                                                    split=sp)
        # the 256 x 256 variant against what it would replace: the library
        # call for the MLP shapes, variant 1 for the attention ones; for
        # mlp.fc also kernel + column sums against mm + dy.sum(0)
        # fused256p: the pipelined loop (variant 4)
        v256, v256p = 3, 4
        arms["fused_v1"] = lambda: fw.wgrad(dy, x, out=dw, variant=1)
        arms["fused256"] = lambda: fw.wgrad(dy, x, out=dw, variant=v256)
        arms["fused256p"] = lambda: fw.wgrad(dy, x, out=dw, variant=v256p)
        if name == "mlp_fc":
            db = torch.empty(N, dtype=torch.bfloat16, device="cuda")
            arms["torch_mm_sum0"] = lambda: (torch.mm(dyt, x, out=dw),
                                             torch.sum(dy, 0, out=db))
            arms["fused256_db"] = lambda: fw.wgrad(dy, x, out=dw,
                                                   variant=v256, db_out=db)
            arms["fused256p_db"] = lambda: fw.wgrad(dy, x, out=dw,
                                                    variant=v256p, db_out=db)
        for fn in arms.values():
            timed(fn)
        ms = {n: [] for n in arms}
        for _ in range(rounds):
            for n, fn in arms.items():
                ms[n].append(timed(fn))
        flop = 2.0 * M * N * K
        rec = dict(N=N, K=K, wired=(N, K) in fw.TUNED, variant=variant)
        for n, xs in ms.items():
            xs = sorted(xs)
            med = xs[len(xs) // 2]
            rec[n] = dict(ms_median=round(med, 4),
                          ms_range=[round(xs[0], 4), round(xs[-1], 4)],
                          tflops=round(flop / med / 1e9, 1))
        # the wiring rule: the median below the fastest round of the other
        base = "torch_mm" if name.startswith("mlp") else "fused_v1"
        rec["fused256_beats_" + base] = bool(
            rec["fused256"]["ms_median"] < rec[base]["ms_range"][0])
        if name == "mlp_fc":
            rec["fused256_db_beats_torch_mm_sum0"] = bool(
                rec["fused256_db"]["ms_median"]
                < rec["torch_mm_sum0"]["ms_range"][0])
        # variant 4 against what the shape had before it (profiles/r16/)
        before = {"mlp_fc": "fused256_db", "attn_proj": "fused_v1"}.get(
            name, "fused256")
        mine = "fused256p_db" if name == "mlp_fc" else "fused256p"
        rec["fused256p_beats_" + before] = bool(
            rec[mine]["ms_median"] < rec[before]["ms_range"][0])
        out["wgrad_" + name] = rec


def main():
    torch.cuda.set_device(0)
    s = torch.cuda.current_stream().cuda_stream
    out = {}
    if "--only-rope" in sys.argv[1:]:
        bench_rope(out)
        print(json.dumps(out, indent=1))
        return
    if "--only-bias-grad" in sys.argv[1:]:
        bench_bias_grad(out)
        print(json.dumps(out, indent=1))
        return
    if "--only-attn" in sys.argv[1:]:
        bench_attn(out)
        print(json.dumps(out, indent=1))
        return
    if "--only-attn-bwd" in sys.argv[1:]:
        bench_attn_bwd(out)
        print(json.dumps(out, indent=1))
        return
    if "--only-gqa-attn" in sys.argv[1:]:
        bench_gqa_attn(out)
        print(json.dumps(out, indent=1))
        return
    if "--only-gqa-attn-hd128" in sys.argv[1:]:
        bench_gqa_attn_hd128(out)
        print(json.dumps(out, indent=1))
        return
    if "--only-gqa-attn-doc" in sys.argv[1:]:
        bench_gqa_attn_doc(out)
        print(json.dumps(out, indent=1))
        return
    if "--only-wgrad" in sys.argv[1:]:
        bench_wgrad(out, sweep="--sweep" in sys.argv[1:])
        print(json.dumps(out, indent=1))
        return
    if "--only-qkv-attn-bwd" in sys.argv[1:]:
        bench_qkv_attn_bwd(out)
        print(json.dumps(out, indent=1))
        return
    if "--only-add-rms" in sys.argv[1:]:
        bench_add_rms(out)
        print(json.dumps(out, indent=1))
        return

    # ---- LN (R=65536, C=768) ----
    R, C = 65536, 768
    x = torch.randn(R, C, device="cuda").to(torch.bfloat16)
    w = torch.randn(C, device="cuda").to(torch.bfloat16)
    b = torch.randn(C, device="cuda").to(torch.bfloat16)
    dy = torch.randn(R, C, device="cuda").to(torch.bfloat16)
    y = torch.empty_like(x)
    dx = torch.empty_like(x)
    mean = torch.empty(R, dtype=torch.float32, device="cuda")
    rstd = torch.empty(R, dtype=torch.float32, device="cuda")
    dwdb = torch.zeros(2 * C, dtype=torch.float32, device="cuda")
    out["ln_fwd_ms"] = round(t(lambda: _core.ln_fwd(
        x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(),
        mean.data_ptr(), rstd.data_ptr(), R, C, 1e-5, s)), 3)
    out["ln_bwd_ms"] = round(t(lambda: _core.ln_bwd(
        dy.data_ptr(), x.data_ptr(), w.data_ptr(), mean.data_ptr(),
        rstd.data_ptr(), dx.data_ptr(), dwdb.data_ptr(),
        dwdb[C:].data_ptr(), R, C, s)), 3)
    xt = x.clone().requires_grad_(True)
    wt = w.clone().requires_grad_(True)
    bt = b.clone().requires_grad_(True)
    out["torch_ln_fwd_ms"] = round(t(lambda: torch.nn.functional.layer_norm(
        xt, (C,), wt, bt, 1e-5)), 3)
    yt = torch.nn.functional.layer_norm(xt, (C,), wt, bt, 1e-5)
    out["torch_ln_bwd_ms"] = round(t(lambda: torch.autograd.grad(
        yt, (xt, wt, bt), dy, retain_graph=True)), 3)

    # ---- fused add + LN vs the unfused sequence it replaces ----
    # effective TB/s = mandatory bytes / time, with A = one (R, C) bf16
    # activation: both forward and backward must move 4A
    A = R * C * 2
    delta = torch.randn(R, C, device="cuda").to(torch.bfloat16)
    dres = torch.randn(R, C, device="cuda").to(torch.bfloat16)
    x_new = torch.empty_like(x)
    sums = torch.empty(3, C, dtype=torch.bfloat16, device="cuda")
    part = torch.empty(_core.add_ln_max_blocks() * 3 * C,
                       dtype=torch.float32, device="cuda")
    ms = t(lambda: _core.add_ln_fwd(
        x.data_ptr(), delta.data_ptr(), 0, w.data_ptr(), b.data_ptr(),
        x_new.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
        R, C, 1e-5, s))
    out["add_ln_fwd_ms"] = round(ms, 3)
    out["add_ln_fwd_tbps"] = round(4 * A / ms / 1e9, 2)
    ms = t(lambda: _core.add_ln_bwd(
        dy.data_ptr(), x_new.data_ptr(), w.data_ptr(), mean.data_ptr(),
        rstd.data_ptr(), dres.data_ptr(), dx.data_ptr(), sums[0].data_ptr(),
        sums[1].data_ptr(), 0, part.data_ptr(), R, C, s))
    out["add_ln_bwd_ms"] = round(ms, 3)
    out["add_ln_bwd_tbps"] = round(4 * A / ms / 1e9, 2)
    ms = t(lambda: _core.add_ln_bwd(
        dy.data_ptr(), x_new.data_ptr(), w.data_ptr(), mean.data_ptr(),
        rstd.data_ptr(), dres.data_ptr(), dx.data_ptr(), sums[0].data_ptr(),
        sums[1].data_ptr(), sums[2].data_ptr(), part.data_ptr(), R, C, s))
    out["add_ln_bwd_ddbias_ms"] = round(ms, 3)

    def unfused_fwd():
        torch.add(x, delta, out=x_new)
        _core.ln_fwd(x_new.data_ptr(), w.data_ptr(), b.data_ptr(),
                     y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), R, C,
                     1e-5, s)

    def unfused_bwd():
        dwdb.zero_()
        _core.ln_bwd(dy.data_ptr(), x_new.data_ptr(), w.data_ptr(),
                     mean.data_ptr(), rstd.data_ptr(), dx.data_ptr(),
                     dwdb.data_ptr(), dwdb[C:].data_ptr(), R, C, s)
        torch.add(dx, dres, out=y)
        dwdb.to(torch.bfloat16)
    ms = t(unfused_fwd)
    out["unfused_add_ln_fwd_ms"] = round(ms, 3)
    out["unfused_add_ln_fwd_tbps"] = round(4 * A / ms / 1e9, 2)
    ms = t(unfused_bwd)
    out["unfused_add_ln_bwd_ms"] = round(ms, 3)
    out["unfused_add_ln_bwd_tbps"] = round(4 * A / ms / 1e9, 2)

    # ---- GELU (65536 x 3072) ----
    xg = torch.randn(65536, 3072, device="cuda").to(torch.bfloat16)
    yg = torch.empty_like(xg)
    dyg = torch.randn_like(xg)
    dxg = torch.empty_like(xg)
    ng = xg.numel()
    out["gelu_fwd_ms"] = round(t(lambda: _core.gelu_fwd(
        xg.data_ptr(), yg.data_ptr(), ng, s)), 3)
    out["gelu_bwd_ms"] = round(t(lambda: _core.gelu_bwd(
        dyg.data_ptr(), xg.data_ptr(), dxg.data_ptr(), ng, s)), 3)
    xt2 = xg.clone().requires_grad_(True)
    out["torch_gelu_fwd_ms"] = round(t(lambda: torch.nn.functional.gelu(
        xt2, approximate="tanh")), 3)
    yt2 = torch.nn.functional.gelu(xt2, approximate="tanh")
    out["torch_gelu_bwd_ms"] = round(t(lambda: torch.autograd.grad(
        yt2, xt2, dyg, retain_graph=True)), 3)

    # ---- RMSNorm (llama-1B shape R=B*T=16384, C=2048; 8B C=4096) ----
    for C2 in (2048, 4096):
        R2 = 16384
        xr = torch.randn(R2, C2, device="cuda").to(torch.bfloat16)
        wr = torch.randn(C2, device="cuda").to(torch.bfloat16)
        dyr = torch.randn(R2, C2, device="cuda").to(torch.bfloat16)
        yr = torch.empty_like(xr)
        dxr = torch.empty_like(xr)
        rstd2 = torch.empty(R2, dtype=torch.float32, device="cuda")
        dg = torch.zeros(C2, dtype=torch.float32, device="cuda")
        out[f"rms{C2}_fwd_ms"] = round(t(lambda: _core.rms_fwd(
            xr.data_ptr(), wr.data_ptr(), yr.data_ptr(), rstd2.data_ptr(),
            R2, C2, 1e-5, s)), 3)
        out[f"rms{C2}_bwd_ms"] = round(t(lambda: _core.rms_bwd(
            dyr.data_ptr(), xr.data_ptr(), wr.data_ptr(), rstd2.data_ptr(),
            dxr.data_ptr(), dg.data_ptr(), R2, C2, s)), 3)

        def torch_rms(xi, wi):  # the pre-fusion module path (fp32 upcast)
            xf = xi.float()
            h = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-5)
            return (h * wi.float()).to(xi.dtype)
        xt3 = xr.clone().requires_grad_(True)
        wt3 = wr.clone().requires_grad_(True)
        out[f"torch_rms{C2}_fwd_ms"] = round(t(lambda: torch_rms(xt3, wt3)), 3)
        yt3 = torch_rms(xt3, wt3)
        out[f"torch_rms{C2}_bwd_ms"] = round(t(lambda: torch.autograd.grad(
            yt3, (xt3, wt3), dyr, retain_graph=True)), 3)

    # ---- bias-grad column sum (R=65536, C=768 and 3072) ----
    for Cc in (768, 3072):
        Rc = 65536
        xc = torch.randn(Rc, Cc, device="cuda").to(torch.bfloat16)
        oc = torch.zeros(Cc, dtype=torch.float32, device="cuda")
        out[f"colsum{Cc}_ms"] = round(t(lambda: _core.colsum_bf16(
            xc.data_ptr(), oc.data_ptr(), Rc, Cc, s)), 3)
        out[f"torch_colsum{Cc}_ms"] = round(t(lambda: xc.sum(0)), 3)

    # ---- SwiGLU (llama-1B MLP shape R=8192, F=8192) ----
    Rs, Fs = 8192, 8192
    sx1 = torch.randn(Rs, Fs, device="cuda").to(torch.bfloat16)
    sx3 = torch.randn(Rs, Fs, device="cuda").to(torch.bfloat16)
    sdy = torch.randn(Rs, Fs, device="cuda").to(torch.bfloat16)
    sy = torch.empty_like(sx1)
    sdx1 = torch.empty_like(sx1)
    sdx3 = torch.empty_like(sx3)
    ns = sx1.numel()
    out["swiglu_fwd_ms"] = round(t(lambda: _core.swiglu_fwd(
        sx1.data_ptr(), sx3.data_ptr(), sy.data_ptr(), ns, s)), 3)
    out["swiglu_bwd_ms"] = round(t(lambda: _core.swiglu_bwd(
        sdy.data_ptr(), sx1.data_ptr(), sx3.data_ptr(), sdx1.data_ptr(),
        sdx3.data_ptr(), ns, s)), 3)
    sa = sx1.clone().requires_grad_(True)
    sb = sx3.clone().requires_grad_(True)
    out["torch_swiglu_fwd_ms"] = round(t(
        lambda: torch.nn.functional.silu(sa) * sb), 3)
    syt = torch.nn.functional.silu(sa) * sb
    out["torch_swiglu_bwd_ms"] = round(t(lambda: torch.autograd.grad(
        syt, (sa, sb), sdy, retain_graph=True)), 3)

    bench_rope(out)
    bench_add_rms(out)
    bench_bias_grad(out)

    # ---- CE (R=65536, V=50257) ----
    R, V = 65536, 50257
    logits = (torch.randn(R, V, device="cuda") * 2).to(torch.bfloat16)
    targets32 = torch.randint(0, V, (R,), device="cuda", dtype=torch.int32)
    targets = targets32.long()
    loss = torch.empty(R, dtype=torch.float32, device="cuda")
    row_m = torch.empty(R, dtype=torch.float32, device="cuda")
    row_lse = torch.empty(R, dtype=torch.float32, device="cuda")
    dlog = torch.empty_like(logits)
    g = torch.ones((), dtype=torch.float32, device="cuda")
    out["ce_fwd_ms"] = round(t(lambda: _core.ce_fwd(
        logits.data_ptr(), targets32.data_ptr(), loss.data_ptr(),
        row_m.data_ptr(), row_lse.data_ptr(), R, V, s), iters=5), 3)
    out["ce_bwd_ms"] = round(t(lambda: _core.ce_bwd(
        logits.data_ptr(), targets32.data_ptr(), row_lse.data_ptr(),
        dlog.data_ptr(), g.data_ptr(), 1.0 / R, R, V, s), iters=5), 3)
    # one-pass loss + dlogits: mandatory bytes = one read + one write of the
    # logits; compare with ce_fwd_ms + ce_bwd_ms (three reads + one write)
    ms = t(lambda: _core.ce_fwd_grad(
        logits.data_ptr(), targets32.data_ptr(), loss.data_ptr(),
        row_lse.data_ptr(), dlog.data_ptr(), 1.0 / R, R, V, s), iters=5)
    out["ce_fwd_grad_ms"] = round(ms, 3)
    out["ce_fwd_grad_tbps"] = round(2 * logits.numel() * 2 / ms / 1e9, 2)
    out["ce_bwd_skip_unit_ms"] = round(t(lambda: _core.ce_bwd(
        logits.data_ptr(), targets32.data_ptr(), row_lse.data_ptr(),
        dlog.data_ptr(), g.data_ptr(), 1.0 / R, R, V, s,
        skip_if_unit=True), iters=5), 4)
    lt = logits.clone().requires_grad_(True)
    out["torch_ce_fwd_ms"] = round(t(lambda: torch.nn.functional.cross_entropy(
        lt, targets), iters=5), 3)
    lt2 = logits.clone().requires_grad_(True)
    losst = torch.nn.functional.cross_entropy(lt2, targets)
    out["torch_ce_bwd_ms"] = round(t(lambda: torch.autograd.grad(
        losst, lt2, retain_graph=True), iters=5), 3)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
