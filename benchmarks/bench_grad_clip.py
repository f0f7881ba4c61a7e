#!/usr/bin/env python3
"""Global-norm gradient clipping at GPT-2-small's flat parameter count, for
bf16 and fp32 gradients.  Three things are timed, interleaved round by round
so that they see the same machine:

  (a) reduce    grad_clip_coef alone: k_grad_sumsq + k_grad_clip_finalize
  (b) fused     (a) followed by the clipped fused AdamW step
  (c) torch     torch.nn.utils.clip_grad_norm_ over per-parameter views of the
                flat gradient (GPT-2-small's shapes) followed by the unclipped
                fused AdamW step: what a user can do without max_grad_norm
  (d) plain     the unclipped fused AdamW step alone, for scale

Every window is `--iters` calls between two device synchronisations, after a
warm-up of the same calls; a figure is the median over `--rounds` windows
and comes with the fastest and slowest window.  (a) is also given as GB/s of
the gradient bytes it must read, against the 6.29 TB/s that a float4 copy
reaches on an MI355X and the 8 TB/s of the HBM3E specification.

Needs a GPU; writes one JSON file (default profiles/grad_clip_bench.json).
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from sharedtensor_amd.engine import SharedFlat  # noqa: E402
from sharedtensor_amd.models.gpt2 import GPT2, GPT2Config  # noqa: E402
from sharedtensor_amd.utils import free_port  # noqa: E402

HBM_COPY_TBPS = 6.29   # measured float4 copy
HBM_SPEC_TBPS = 8.0
LR, BETAS, EPS, WD = 3e-4, (0.9, 0.999), 1e-8, 0.01
MAX_NORM = 1.0


def gpt2_small_shapes():
    """Shapes of GPT-2-small's parameters, tied weights counted once, as
    FlatParamShared lays them out."""
    with torch.device("meta"):
        model = GPT2(GPT2Config.small())
    seen, shapes = set(), []
    for p in model.parameters():
        if p.requires_grad and id(p) not in seen:
            seen.add(id(p))
            shapes.append(tuple(p.shape))
    return shapes


def window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3   # ms per call


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4),
            "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "windows": [round(x, 4) for x in ms]}


def bench_dtype(gdtype, shapes, iters, rounds, warmup):
    n = sum(int(torch.Size(s).numel()) for s in shapes)
    dev = torch.device("cuda:0")
    sh = SharedFlat("127.0.0.1", free_port(), [n], device=dev,
                    provision_up=False, expected_children=0)
    sh._start()
    try:
        gen = torch.Generator(device=dev).manual_seed(0)
        sh._add_flat(0.02 * torch.randn(n, device=dev, generator=gen))
        grad0 = (0.01 * torch.randn(n, device=dev, generator=gen)).to(gdtype)
        grad = grad0.clone()
        mom = torch.zeros(n, device=dev)
        vel = torch.zeros(n, device=dev)
        bf16 = gdtype == torch.bfloat16
        shadow = sh.values.to(torch.bfloat16) if bf16 else None
        # per-parameter views with .grad, as the trainer sets them up
        src = shadow if bf16 else sh.values
        params, off = [], 0
        for s in shapes:
            sz = int(torch.Size(s).numel())
            p = torch.nn.Parameter(src[off:off + sz].view(s),
                                   requires_grad=True)
            p.grad = grad[off:off + sz].view(s)
            params.append(p)
            off += sz
        step = [0]

        def adamw(clip_state=None):
            step[0] += 1
            if bf16:
                sh.fused_adamw_bf16_step(mom, vel, grad, shadow, step[0], LR,
                                         BETAS, EPS, WD,
                                         clip_state=clip_state)
            else:
                sh.fused_adamw_step(mom, vel, grad, step[0], LR, BETAS, EPS,
                                    WD, clip_state=clip_state)

        def reduce_only():
            sh.grad_clip_coef(grad, MAX_NORM)

        def fused():
            adamw(sh.grad_clip_coef(grad, MAX_NORM))

        def torch_clip():
            # scales grad in place: put the gradient back outside the window
            torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
            adamw()

        arms = {"a_reduce": reduce_only, "b_fused_clip_adamw": fused,
                "c_torch_clip_then_adamw": torch_clip, "d_adamw": adamw}
        times = {k: [] for k in arms}
        for k, fn in arms.items():
            for _ in range(warmup):
                fn()
        for _ in range(rounds):
            for k, fn in arms.items():
                grad.copy_(grad0)
                times[k].append(window(fn, iters))
        st = sh.decode_clip_state(sh.grad_clip_coef(grad0, MAX_NORM))
        ref = float(torch.linalg.vector_norm(grad0.double()))
        out = {k: summary(v) for k, v in times.items()}
        a = out["a_reduce"]
        gbytes = n * grad.element_size() / 1e9
        a["grad_gbytes"] = round(gbytes, 4)
        for key in ("median_ms", "min_ms", "max_ms"):
            a["gbps_at_" + key] = round(gbytes / a[key] * 1e3, 1)
        a["share_of_hbm_copy_roofline"] = round(
            gbytes / a["median_ms"] / HBM_COPY_TBPS, 3)
        a["share_of_hbm_spec"] = round(
            gbytes / a["median_ms"] / HBM_SPEC_TBPS, 3)
        b, c = out["b_fused_clip_adamw"], out["c_torch_clip_then_adamw"]
        out["b_over_c_median"] = round(b["median_ms"] / c["median_ms"], 4)
        out["b_slowest_vs_c_fastest_ms"] = [b["max_ms"], c["min_ms"]]
        out["grad_norm"] = {"kernel": st["grad_norm"], "torch_fp64": ref}
        return n, out
    finally:
        sh.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(
        __file__.rsplit("/", 2)[0], "profiles", "grad_clip_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_grad_clip.py needs a GPU")
    torch.cuda.set_device(0)
    shapes = gpt2_small_shapes()
    res = {"device": torch.cuda.get_device_name(0),
           "model": "GPT2Config.small()", "tensors": len(shapes),
           "iters_per_window": args.iters, "rounds": args.rounds,
           "max_norm": MAX_NORM,
           "hbm_copy_roofline_tbps": HBM_COPY_TBPS,
           "hbm_spec_tbps": HBM_SPEC_TBPS}
    for name, dt in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
        n, res[name] = bench_dtype(dt, shapes, args.iters, args.rounds,
                                   args.warmup)
        res["n"] = n
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
