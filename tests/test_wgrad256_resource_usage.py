"""Compiler resource report of the 256 x 256 weight-gradient kernel (no GPU
needed: hipcc cross-compiles for gfx950).

The plan in csrc/wgrad_kernels.hip: no scratch and no spills (a spilled
accumulator or staging register would put memory traffic into the step
loop); all LDS in the one staging array, two stages of 2 + 2 panels = 128 KB,
which the column-sum combine reuses; one wave per SIMD, whose 512 registers
hold the 256 accumulators (as AGPRs) beside everything else; one workgroup
per CU.  With and without the column sums.
"""
import re

from resource_report import kernel_resources

LDS_PER_CU = 160 * 1024
VGPR_FILE = 512
PANEL = 64 * 128 * 2    # one [64 tokens][128 features] bf16 panel


def test_wgrad256_no_scratch_lds_and_occupancy_as_planned(tmp_path):
    kernels = kernel_resources("wgrad_kernels.hip", tmp_path)
    found = {}
    for name, res in kernels.items():
        m = re.search(r"10k_wgrad256ILb([01])EE", name)
        if m:
            found[bool(int(m.group(1)))] = res
    assert set(found) == {False, True}, sorted(kernels)
    for colsum, res in sorted(found.items()):
        print(f"WGRAD256 resources <colsum={colsum}>: VGPRs {res['VGPRs']} "
              f"AGPRs {res['AGPRs']} LDS {res['LDS']} occupancy "
              f"{res['Occupancy']} waves/SIMD")
        assert res["ScratchSize"] == 0, res
        assert res["VGPRs Spill"] == 0 and res["SGPRs Spill"] == 0, res
        assert res["LDS"] == 2 * 4 * PANEL, res
        assert LDS_PER_CU // res["LDS"] == 1
        # the 4 x 4 accumulators of 16 registers each
        assert res["AGPRs"] == 256, res
        assert res["VGPRs"] + res["AGPRs"] <= VGPR_FILE, res
        assert res["Occupancy"] == 1, res
