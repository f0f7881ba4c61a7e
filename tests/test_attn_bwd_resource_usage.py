"""Compiler resource report of the attention backward kernels (no GPU needed:
hipcc cross-compiles for gfx950), compiled with the flags build.py gives the
file and held to the plan in the header comment of csrc/attn_bwd_kernels.hip:
no scratch, no spills and no AGPRs in either kernel; k_attn_bwd_dq at most
160 VGPRs, 32 KB of LDS, 3 waves/SIMD; k_attn_bwd_dkdv at most 200 VGPRs,
33 KB of LDS, 2 waves/SIMD."""
import pytest

import build
from resource_report import kernel_resources

VGPR_FILE = 512  # unified VGPR + AGPR budget of one SIMD lane

PLAN = {
    "k_attn_bwd_dq": dict(vgprs=160, lds=32 * 1024, waves=3),
    "k_attn_bwd_dkdv": dict(vgprs=200, lds=33 * 1024, waves=2),
}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    with pytest.MonkeyPatch.context() as mp:  # hipcc appends these itself
        mp.setenv("HIPCC_COMPILE_FLAGS_APPEND",
                  " ".join(build.EXTRA_FLAGS["attn_bwd_kernels.hip"]))
        return kernel_resources("attn_bwd_kernels.hip",
                                tmp_path_factory.mktemp("attn_bwd"))


@pytest.mark.parametrize("name", sorted(PLAN))
def test_attn_bwd_kernel_follows_plan(kernels, name):
    plan = PLAN[name]
    (res,) = [v for k, v in kernels.items() if name in k]
    assert res["ScratchSize"] == 0, res
    assert res["VGPRs Spill"] == 0 and res["SGPRs Spill"] == 0, res
    assert res["AGPRs"] == 0, res
    assert res["VGPRs"] <= plan["vgprs"], res
    assert res["LDS"] == plan["lds"], res
    regs = -(-res["VGPRs"] // 8) * 8
    assert min(8, VGPR_FILE // regs) == plan["waves"], res
    assert res["Occupancy"] == plan["waves"], res
