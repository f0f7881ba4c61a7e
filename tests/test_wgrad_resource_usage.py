"""Compiler resource report of the split-K weight-gradient kernels (no GPU
needed: hipcc cross-compiles for gfx950).

The header comment of csrc/wgrad_kernels.hip states the plan: no scratch, no
spills, all LDS in one array of 32 KB per stage and 128 x 128 tile.  A spill
or a private array in scratch would put memory traffic into the step loop;
LDS beyond 160 KB would not launch.  The VGPR and occupancy figures found
are printed as a record (profiles/r09/).
"""
import re

from resource_report import kernel_resources

LDS_PER_CU = 160 * 1024
VGPR_FILE = 512
PANEL = 64 * 128 * 2    # one [64 tokens][128 features] bf16 panel

# template arguments <NP, KP, NBUF> -> waves per SIMD the kernel is built for
BUILT = {(1, 1, 2): 2, (1, 1, 1): 3, (2, 1, 2): 2}


def test_wgrad_kernels_no_scratch_lds_as_planned(tmp_path):
    kernels = kernel_resources("wgrad_kernels.hip", tmp_path)
    found = {}
    for name, res in kernels.items():
        m = re.search(r"7k_wgradILi(\d)ELi(\d)ELi(\d)EE", name)
        if m:
            found[tuple(int(g) for g in m.groups())] = res
    assert set(found) == set(BUILT), sorted(found)
    for (np_, kp, nbuf), res in sorted(found.items()):
        waves_per_block = 4 * np_ * kp
        regs = -(-(res["VGPRs"] + res["AGPRs"]) // 8) * 8
        waves_by_regs = min(8, VGPR_FILE // regs)
        blocks = min(waves_by_regs * 4 // waves_per_block,
                     LDS_PER_CU // res["LDS"])
        print(f"WGRAD resources <{np_},{kp},{nbuf}>: VGPRs {res['VGPRs']} "
              f"AGPRs {res['AGPRs']} LDS {res['LDS']} occupancy "
              f"{res['Occupancy']} waves/SIMD, {blocks} workgroups/CU")
        assert res["ScratchSize"] == 0, res
        assert res["VGPRs Spill"] == 0 and res["SGPRs Spill"] == 0, res
        # one array: the stages and nothing else (a private array promoted
        # to LDS would show here)
        assert res["LDS"] == nbuf * (np_ + kp) * PANEL, res
        assert res["LDS"] <= LDS_PER_CU
        assert waves_by_regs >= BUILT[(np_, kp, nbuf)], res
        assert res["Occupancy"] >= BUILT[(np_, kp, nbuf)], res
        assert blocks >= 1


def test_reduce_kernel_is_small(tmp_path):
    kernels = kernel_resources("wgrad_kernels.hip", tmp_path)
    (res,) = [v for k, v in kernels.items() if "k_wgrad_reduce" in k]
    assert res["ScratchSize"] == 0 and res["LDS"] == 0, res
    assert res["VGPRs Spill"] == 0 and res["SGPRs Spill"] == 0, res
    assert res["Occupancy"] == 8, res
