"""Compiler resource report of csrc/gqa_attn_hd128_bwd_kernels.hip (no GPU
needed), every instantiation compiled with its EXTRA_FLAGS and held to the
plan in its header comment: no scratch, no spills, 2 waves/SIMD, VGPRs plus
AGPRs within that step's 256 registers, 64 KB of static LDS for the dQ
kernels and none for the dK/dV kernel, whose 66048 B are dynamic."""
import pytest

import build
from resource_report import kernel_resources

VGPR_FILE = 512  # unified VGPR + AGPR budget of one SIMD lane
SRC = "gqa_attn_hd128_bwd_kernels.hip"
PLAN = {"k_gqa_bwd_dq_hd128ILi2E": dict(waves=2, lds=64 * 1024),
        "k_gqa_bwd_dq_hd128ILi4E": dict(waves=2, lds=64 * 1024),
        "k_gqa_bwd_dkdv_hd128": dict(waves=2, lds=0)}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    with pytest.MonkeyPatch.context() as mp:  # hipcc appends these itself
        mp.setenv("HIPCC_COMPILE_FLAGS_APPEND", " ".join(build.EXTRA_FLAGS[SRC]))
        found = kernel_resources(SRC, tmp_path_factory.mktemp("gqa_hd128_bwd"))
    assert len(found) == len(PLAN), sorted(found)  # every instantiation
    return found


@pytest.mark.parametrize("name", sorted(PLAN))
def test_gqa_hd128_bwd_kernel_follows_plan(kernels, name):
    plan = PLAN[name]
    (res,) = [v for k, v in kernels.items() if name in k]
    assert res["ScratchSize"] == 0, res
    assert res["VGPRs Spill"] == 0 and res["SGPRs Spill"] == 0, res
    regs = -(-res["VGPRs"] // 8) * 8 + -(-res["AGPRs"] // 8) * 8
    assert regs <= VGPR_FILE // plan["waves"], res
    assert res["LDS"] == plan["lds"], res
    assert res["Occupancy"] == plan["waves"], res
