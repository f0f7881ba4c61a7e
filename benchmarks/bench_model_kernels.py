#!/usr/bin/env python3
"""Microbenchmark the model-side fused kernels (LN, add+LN, GELU, RMSNorm,
add+RMSNorm, colsum, SwiGLU, RoPE, CE) vs their torch equivalents at the
GPT-2-small B=64 and llama-1B bench shapes.  `--only-rope` runs the RoPE
section alone, `--only-add-rms` the add+RMSNorm section, `--only-bias-grad`
the fused bias-gradient section, `--only-attn` the attention forward,
`--only-wgrad` the split-K weight-gradient kernel."""
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
    if "--only-wgrad" in sys.argv[1:]:
        bench_wgrad(out, sweep="--sweep" in sys.argv[1:])
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
