"""Compiler resource report of the document-masked grouped-query attention
kernels (no GPU needed: hipcc cross-compiles for gfx950), every template
instantiation held to the plan in the header comments of
csrc/gqa_attn_doc_kernels.hip and csrc/gqa_attn_doc_bwd_kernels.hip: no
scratch, no spills, no AGPRs, and the occupancy and LDS of the plain
counterpart in tests/test_gqa_attn_resource_usage.py."""
import pytest

import build
from resource_report import kernel_resources

VGPR_FILE = 512  # unified VGPR + AGPR budget of one SIMD lane

PLAN = {
    "k_gqa_fwd_doc_hd64ILi2E": dict(waves=4, lds=32 * 1024),
    "k_gqa_fwd_doc_hd64ILi4E": dict(waves=4, lds=32 * 1024),
    "k_gqa_bwd_dq_doc_hd64ILi2E": dict(waves=3, lds=32 * 1024),
    "k_gqa_bwd_dq_doc_hd64ILi4E": dict(waves=3, lds=32 * 1024),
    "k_gqa_bwd_dkdv_doc_hd64": dict(waves=2, lds=33 * 1024),
}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("gqa_attn_doc")
    found = kernel_resources("gqa_attn_doc_kernels.hip", tmp)
    with pytest.MonkeyPatch.context() as mp:  # hipcc appends these itself
        mp.setenv("HIPCC_COMPILE_FLAGS_APPEND",
                  " ".join(build.EXTRA_FLAGS["gqa_attn_doc_bwd_kernels.hip"]))
        found.update(kernel_resources("gqa_attn_doc_bwd_kernels.hip", tmp))
    assert len(found) == len(PLAN), sorted(found)  # every instantiation
    return found


@pytest.mark.parametrize("name", sorted(PLAN))
def test_gqa_doc_kernel_follows_plan(kernels, name):
    plan = PLAN[name]
    (res,) = [v for k, v in kernels.items() if name in k]
    assert res["ScratchSize"] == 0, res
    assert res["VGPRs Spill"] == 0 and res["SGPRs Spill"] == 0, res
    assert res["AGPRs"] == 0, res
    assert res["VGPRs"] <= VGPR_FILE // plan["waves"] // 8 * 8, res
    assert res["LDS"] == plan["lds"], res
    regs = -(-res["VGPRs"] // 8) * 8
    assert min(8, VGPR_FILE // regs) == plan["waves"], res
    assert res["Occupancy"] == plan["waves"], res
