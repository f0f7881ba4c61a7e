"""Compiler resource report of the bias-gradient kernels (no GPU needed:
hipcc cross-compiles for gfx950).

k_gelu_bwd_colsum and k_pack3_colsum run 1024-thread blocks (4 waves/SIMD
each) and size their grid for two blocks per CU; above 64 VGPRs only one
block fits and half of the grid waits for the other.  A spill to scratch
would add HBM traffic to kernels whose point is to remove a pass.
"""
import os
import re
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "sharedtensor_amd", "csrc")


def _report(tmp_path):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = [os.path.join(rocm, "bin", "hipcc"), "--offload-device-only", "-c",
           os.path.join(CSRC, "bias_grad_kernels.hip"), "-o",
           str(tmp_path / "bias_grad_dev.out"), "--offload-arch=gfx950",
           "-std=c++20", "-O3", "-DSHAMD_WITH_HIP", "-DNDEBUG", f"-I{CSRC}",
           f"-I{rocm}/include", "-Rpass-analysis=kernel-resource-usage"]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    kernels, name = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels[name] = {}
            continue
        m = re.search(r"\s(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|"
                      r"Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): "
                      r"(\d+)", line)
        if m and name:
            kernels[name][m.group(1).split(" ")[0]] = int(m.group(2))
    return kernels


def test_bias_grad_kernels_no_scratch_two_blocks_per_cu(tmp_path):
    kernels = _report(tmp_path)
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
