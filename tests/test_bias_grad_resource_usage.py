"""Compiler resource report of the bias-gradient kernels (no GPU needed:
hipcc cross-compiles for gfx950).

k_gelu_bwd_colsum and k_pack3_colsum run 1024-thread blocks (4 waves/SIMD
each) and size their grid for two blocks per CU; above 64 VGPRs only one
block fits and half of the grid waits for the other.  A spill to scratch
would add HBM traffic to kernels whose point is to remove a pass.
"""
from resource_report import kernel_resources


def test_bias_grad_kernels_no_scratch_two_blocks_per_cu(tmp_path):
    kernels = kernel_resources("bias_grad_kernels.hip", tmp_path)
    (gelu,) = [v for k, v in kernels.items() if "k_gelu_bwd_colsum" in k]
    (pack,) = [v for k, v in kernels.items() if "k_pack3_colsum" in k]
    (red,) = [v for k, v in kernels.items() if "k_bg_reduce" in k]
    for name, res in kernels.items():
        assert res["ScratchSize"] == 0, (name, res)
    # 1024 threads = 4 waves/SIMD per block; two blocks need 8 and, at
    # 32 KB of LDS each, fit the CU's LDS with room to spare
    for res in (gelu, pack):
        assert res["VGPRs"] <= 64 and res["Occupancy"] == 8, res
        assert res["LDS"] <= 32768, res
    assert red["Occupancy"] == 8, red
