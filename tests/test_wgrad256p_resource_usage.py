"""Compiler resource report of the pipelined 256 x 256 weight-gradient kernel
k_wgrad256p (no GPU needed: hipcc cross-compiles for gfx950).

The plan in csrc/wgrad_kernels.hip: no scratch and no spills; a ring of four
32-token slots of 2 + 2 half panels, 128 KB, which the column-sum combine
reuses; 256 accumulators in AGPRs; one wave per SIMD; and, with the staging
registers gone, no more VGPRs than k_wgrad256 in the same report.
"""
import re

from resource_report import kernel_resources

LDS_PER_CU = 160 * 1024
VGPR_FILE = 512
HALF_PANEL = 32 * 128 * 2   # one [32 tokens][128 features] bf16 half panel


def test_wgrad256p_resources_as_planned(tmp_path):
    kernels = kernel_resources("wgrad_kernels.hip", tmp_path)
    new, old = {}, {}
    for name, res in kernels.items():
        m = re.search(r"11k_wgrad256pILb([01])EE", name)
        if m:
            new[bool(int(m.group(1)))] = res
        m = re.search(r"10k_wgrad256ILb([01])EE", name)
        if m:
            old[bool(int(m.group(1)))] = res
    assert set(new) == {False, True} == set(old), sorted(kernels)
    for colsum, res in sorted(new.items()):
        print(f"WGRAD256P resources <colsum={colsum}>: VGPRs {res['VGPRs']} "
              f"(k_wgrad256: {old[colsum]['VGPRs']}) AGPRs {res['AGPRs']} "
              f"LDS {res['LDS']} occupancy {res['Occupancy']} waves/SIMD")
    for colsum, res in sorted(new.items()):
        assert res["ScratchSize"] == 0, res
        assert res["VGPRs Spill"] == 0 and res["SGPRs Spill"] == 0, res
        assert res["LDS"] == 4 * 4 * HALF_PANEL, res
        assert res["LDS"] <= LDS_PER_CU
        assert res["AGPRs"] == 256, res
        assert res["VGPRs"] + res["AGPRs"] <= VGPR_FILE, res
        assert res["Occupancy"] == 1, res
        assert res["VGPRs"] <= old[colsum]["VGPRs"], (res, old[colsum])
