#!/usr/bin/env python3
"""Parameter groups in the fused optimizer step: the grouped kernels against
the ungrouped ones, bf16 gradients and bf16 shadow, at the flat parameter
counts of GPT-2-small and Llama-1B with the segment tables that
no_decay_groups gives those models (built on the meta device).

Four arms per model, interleaved round by round so that they see the same
machine: AdamW ungrouped / grouped, SGD ungrouped / grouped.  The kernels
move identical bytes, so the target is parity: the grouped median should
lie within the ungrouped arm's own fastest-to-slowest window of this run.

Every window is `--iters` calls between two device synchronisations, after
a warm-up of the same calls; a figure is the median over `--rounds` windows
and comes with the fastest and slowest window.

Needs a GPU; writes one JSON file (default profiles/param_groups_bench.json).
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
from sharedtensor_amd.models.llama import Llama, LlamaConfig  # noqa: E402
from sharedtensor_amd.parallel import no_decay_groups  # noqa: E402
from sharedtensor_amd.utils import free_port  # noqa: E402

LR, BETAS, EPS, WD, MU = 3e-4, (0.9, 0.999), 1e-8, 0.1, 0.9


def segments(model):
    """(sizes, group per tensor) in FlatParamShared order, tied weights
    once; group 0 decays, group 1 (ndim < 2) does not, as no_decay_groups
    assigns them."""
    groups = no_decay_groups(model, WD)
    group_of = {name: gi for gi, g in enumerate(groups) for name in g["params"]}
    by_id = {}
    for name, p in model.named_parameters(remove_duplicate=False):
        by_id.setdefault(id(p), []).append(name)
    seen, sizes, owner = set(), [], []
    for p in model.parameters():
        if p.requires_grad and id(p) not in seen:
            seen.add(id(p))
            sizes.append(p.numel())
            (gi,) = {group_of[nm] for nm in by_id[id(p)] if nm in group_of}
            owner.append(gi)
    return sizes, owner, [g["weight_decay"] for g in groups]


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


def bench_model(model, iters, rounds, warmup):
    sizes, owner, decays = segments(model)
    n = sum(sizes)
    dev = torch.device("cuda:0")
    sh = SharedFlat("127.0.0.1", free_port(), [n], device=dev,
                    provision_up=False, expected_children=0)
    sh._start()
    try:
        gen = torch.Generator(device=dev).manual_seed(0)
        sh._add_flat(0.02 * torch.randn(n, device=dev, generator=gen))
        grad = (0.01 * torch.randn(n, device=dev, generator=gen)
                ).to(torch.bfloat16)
        mom = torch.zeros(n, device=dev)
        vel = torch.zeros(n, device=dev)
        shadow = sh.values.to(torch.bfloat16)
        adamw_table = sh.make_group_table(sizes, owner, [1.0] * len(decays),
                                          decays)
        sgd_table = sh.make_group_table(sizes, owner, [1.0] * len(decays),
                                        [0.0] * len(decays))
        step = [0]

        def adamw(groups=None):
            step[0] += 1
            sh.fused_adamw_bf16_step(mom, vel, grad, shadow, step[0], LR,
                                     BETAS, EPS, WD, groups=groups)

        def sgd(groups=None):
            sh.fused_sgd_bf16_step(mom, grad, shadow, LR, MU, groups=groups)

        arms = {"adamw_ungrouped": adamw,
                "adamw_grouped": lambda: adamw(adamw_table),
                "sgd_ungrouped": sgd,
                "sgd_grouped": lambda: sgd(sgd_table)}
        times = {k: [] for k in arms}
        for fn in arms.values():
            for _ in range(warmup):
                fn()
        for _ in range(rounds):
            for k, fn in arms.items():
                times[k].append(window(fn, iters))
        out = {k: summary(v) for k, v in times.items()}
        for opt in ("adamw", "sgd"):
            u, g = out[opt + "_ungrouped"], out[opt + "_grouped"]
            out[opt + "_grouped_over_ungrouped_median"] = round(
                g["median_ms"] / u["median_ms"], 4)
            out[opt + "_grouped_median_within_ungrouped_spread"] = bool(
                u["min_ms"] <= g["median_ms"] <= u["max_ms"])
        words = adamw_table.cpu()
        out["n"] = n
        out["tensors"] = len(sizes)
        out["segments_after_merging"] = int(words[2])
        out["groups"] = int(words[3])
        return out
    finally:
        sh.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(
        __file__.rsplit("/", 2)[0], "profiles", "param_groups_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_param_groups.py needs a GPU")
    torch.cuda.set_device(0)
    res = {"device": torch.cuda.get_device_name(0),
           "iters_per_window": args.iters, "rounds": args.rounds,
           "gradients": "bf16", "shadow": "bf16", "weight_decay": WD}
    with torch.device("meta"):
        models = {"gpt2_small": GPT2(GPT2Config.small()),
                  "llama_1b": Llama(LlamaConfig.llama_1b())}
    for name, model in models.items():
        res[name] = bench_model(model, args.iters, args.rounds, args.warmup)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
