"""Compiler resource report of the one-pass cross-entropy kernel (no GPU
needed: hipcc cross-compiles for gfx950).

k_ce_fwd_grad keeps a whole vocabulary row in registers; a spill to scratch
would turn its single HBM read into several, and more than 64 VGPRs in the
GPT-2 instantiation would leave one row per CU instead of two.
"""
import os
import re
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "sharedtensor_amd", "csrc")


def _report(tmp_path):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = [os.path.join(rocm, "bin", "hipcc"), "--offload-device-only", "-c",
           os.path.join(CSRC, "ce_kernels.hip"), "-o",
           str(tmp_path / "ce_dev.out"), "--offload-arch=gfx950",
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
                      r"Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and name:
            kernels[name][m.group(1).split(" ")[0]] = int(m.group(2))
    return kernels


def test_ce_fwd_grad_has_no_scratch_and_two_rows_per_cu(tmp_path):
    kernels = _report(tmp_path)
    grad = {k: v for k, v in kernels.items() if "k_ce_fwd_grad" in k}
    assert len(grad) == 2, sorted(kernels)
    for name, res in grad.items():
        assert res["ScratchSize"] == 0, (name, res)
    (gpt2,) = [v for k, v in grad.items() if "ILi1024ELi7EE" in k]
    (llama,) = [v for k, v in grad.items() if "ILi1024ELi16EE" in k]
    # 1024 threads = 4 waves/SIMD per block
    assert gpt2["VGPRs"] <= 64 and gpt2["Occupancy"] == 8, gpt2
    assert llama["VGPRs"] <= 128 and llama["Occupancy"] >= 4, llama
    # no CE kernel may spill
    for name, res in kernels.items():
        assert res["ScratchSize"] == 0, (name, res)
