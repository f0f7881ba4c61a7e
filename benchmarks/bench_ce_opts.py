#!/usr/bin/env python3
"""Fused cross-entropy with options at the GPT-2 bench shape (R = 65536 rows,
V = 50257, bf16 logits): forward + backward, interleaved round by round so
that every configuration sees the same machine.

  (a) default   today's one-pass kernel (no options)
  (b) ignore    ignore_index=-100, nothing masked
  (c) masked    ignore_index=-100, 25 % of the rows masked
  (d) smooth_z  label_smoothing=0.1, z_loss=1e-4 (nothing masked)

and, for (b)-(d), the route a user has without the feature:
F.cross_entropy(x.float(), ...) forward + backward (for (d) plus the z-loss
term from torch.logsumexp).

Every window is `--iters` forward+backward calls between two device
synchronisations, after a warm-up of the same calls; a figure is the median
over `--rounds` windows and comes with the fastest and slowest window.  The
fused figures are also given as TB/s of the bytes the design must move (one
read of the valid rows' logits and one write of every dlogits row).

Needs a GPU; writes one JSON file (default profiles/ce_opts_bench.json).
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from sharedtensor_amd.ops import fused_ce  # noqa: E402

IGNORE = -100
EPS, Z = 0.1, 1e-4


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--vocab", type=int, default=50257)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--torch-iters", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
        "profiles", "ce_opts_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_ce_opts.py needs a GPU")
    R, V = args.rows, args.vocab
    torch.manual_seed(0)
    logits = (torch.randn(R, V, device="cuda") * 3).to(torch.bfloat16)
    logits.requires_grad_(True)
    full = torch.randint(0, V, (R,), device="cuda")
    masked = full.clone()
    masked[torch.arange(R, device="cuda") % 4 == 0] = IGNORE
    n_masked = int((masked == IGNORE).sum())

    def step(loss_fn):
        def run():
            logits.grad = None
            loss_fn().backward()
        return run

    def torch_ce(t, eps=0.0, z=0.0):
        def loss_fn():
            x = logits.float()
            loss = F.cross_entropy(x, t, ignore_index=IGNORE,
                                   label_smoothing=eps)
            if z:
                loss = loss + z * (torch.logsumexp(x, dim=-1) ** 2).mean()
            return loss
        return loss_fn

    fce = fused_ce.fused_cross_entropy
    configs = {
        "a_default": (step(lambda: fce(logits, full)), args.iters),
        "b_ignore": (step(lambda: fce(logits, full, ignore_index=IGNORE)),
                     args.iters),
        "c_masked25": (step(lambda: fce(logits, masked, ignore_index=IGNORE)),
                       args.iters),
        "d_smooth_z": (step(lambda: fce(logits, full, label_smoothing=EPS,
                                        z_loss=Z)), args.iters),
        "b_ignore_torch": (step(torch_ce(full)), args.torch_iters),
        "c_masked25_torch": (step(torch_ce(masked)), args.torch_iters),
        "d_smooth_z_torch": (step(torch_ce(full, EPS, Z)), args.torch_iters),
    }

    # the configurations must agree before their times are compared
    check = {}
    for name, (fn, _) in configs.items():
        fn()
        torch.cuda.synchronize()
        check[name] = float(logits.grad.float().abs().sum())
    for name, (fn, _) in configs.items():
        for _ in range(args.warmup):
            fn()
    times = {name: [] for name in configs}
    for _ in range(args.rounds):
        for name, (fn, iters) in configs.items():
            times[name].append(window(fn, iters))

    res = {name: summary(ms) for name, ms in times.items()}
    row_bytes = V * 2
    moved = {"a_default": 2 * R * row_bytes, "b_ignore": 2 * R * row_bytes,
             "c_masked25": (2 * R - n_masked) * row_bytes,
             "d_smooth_z": 2 * R * row_bytes}
    for name, b in moved.items():
        res[name]["tb_per_s"] = round(b / (res[name]["median_ms"] * 1e-3) / 1e12, 3)
    med = {k: v["median_ms"] for k, v in res.items()}
    out = {
        "device": torch.cuda.get_device_name(0),
        "shape": {"R": R, "V": V, "masked_rows_c": n_masked},
        "options": {"ignore_index": IGNORE, "label_smoothing_d": EPS,
                    "z_loss_d": Z},
        "method": {"iters": args.iters, "torch_iters": args.torch_iters,
                   "rounds": args.rounds, "warmup": args.warmup,
                   "timed": "forward + backward, host clock around a window "
                            "that ends in a device synchronise"},
        "grad_abs_sum": check,
        "ms": res,
        "ratios": {
            "b_over_a": round(med["b_ignore"] / med["a_default"], 4),
            "c_over_b": round(med["c_masked25"] / med["b_ignore"], 4),
            "d_over_a": round(med["d_smooth_z"] / med["a_default"], 4),
            "torch_over_fused_b": round(med["b_ignore_torch"] / med["b_ignore"], 3),
            "torch_over_fused_c": round(med["c_masked25_torch"] / med["c_masked25"], 3),
            "torch_over_fused_d": round(med["d_smooth_z_torch"] / med["d_smooth_z"], 3),
        },
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"ms": med, "ratios": out["ratios"]}))


if __name__ == "__main__":
    main()
