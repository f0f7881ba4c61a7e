"""Compiler resource report of the attention forward kernel (no GPU needed:
hipcc cross-compiles for gfx950).

The header comment of csrc/attn_kernels.hip states the plan: at most 128
VGPRs, no AGPRs, no scratch, no spills, 32 KB of LDS, hence 4 waves/SIMD and
4 workgroups of 4 waves per CU.  A spill would put scratch traffic into the
tile loop; more registers or more LDS would take a workgroup off every CU.
"""
from resource_report import kernel_resources

LDS_PER_CU = 160 * 1024
SIMDS_PER_CU = 4
WAVES_PER_BLOCK = 4     # 256 threads
VGPR_FILE = 512         # unified VGPR + AGPR budget of one SIMD lane


def test_attn_fwd_no_scratch_four_blocks_per_cu(tmp_path):
    kernels = kernel_resources("attn_kernels.hip", tmp_path)
    (res,) = [v for k, v in kernels.items() if "k_attn_fwd_causal_hd64" in k]
    assert res["ScratchSize"] == 0, res
    assert res["VGPRs Spill"] == 0 and res["SGPRs Spill"] == 0, res
    assert res["VGPRs"] <= 128 and res["AGPRs"] == 0, res
    assert res["LDS"] == 32 * 1024, res
    # what the header claims, from the figures themselves
    regs = -(-(res["VGPRs"] + res["AGPRs"]) // 8) * 8
    waves_by_regs = min(8, VGPR_FILE // regs)
    assert waves_by_regs == 4 and res["Occupancy"] == 4, res
    blocks_by_waves = waves_by_regs * SIMDS_PER_CU // WAVES_PER_BLOCK
    blocks_by_lds = LDS_PER_CU // res["LDS"]
    assert blocks_by_lds == 5
    assert min(blocks_by_waves, blocks_by_lds) == 4
