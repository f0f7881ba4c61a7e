"""Compiler resource report of the cross-entropy option kernels (no GPU
needed: hipcc cross-compiles for gfx950).

k_ce_opts_fwd_grad keeps a whole vocabulary row in registers, like
k_ce_fwd_grad: a spill to scratch would turn its single HBM read into
several, and more than 64 VGPRs in a 7-chunk instantiation would leave one
row per CU instead of two.  Both 7-chunk instantiations (masking only, and
smoothing / z-loss) hold the 64-VGPR bound.
"""
import os
import re
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "sharedtensor_amd", "csrc")


def _report(tmp_path):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = [os.path.join(rocm, "bin", "hipcc"), "--offload-device-only", "-c",
           os.path.join(CSRC, "ce_opts_kernels.hip"), "-o",
           str(tmp_path / "ce_opts_dev.out"), "--offload-arch=gfx950",
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


def test_ce_opts_kernels_have_no_scratch_and_keep_the_row_budget(tmp_path):
    kernels = _report(tmp_path)
    # scan, 2 x 2 one-pass, 2 stats-only forward, 2 x 2 backward
    assert len(kernels) == 11, sorted(kernels)
    for name, res in kernels.items():
        assert res["ScratchSize"] == 0, (name, res)
    grad = {k: v for k, v in kernels.items() if "k_ce_opts_fwd_grad" in k}
    assert len(grad) == 4, sorted(kernels)
    # <1024, NCHUNK, EXTRA>; 1024 threads = 4 waves/SIMD per block
    for extra in ("Lb0E", "Lb1E"):
        (c7,) = [v for k, v in grad.items() if "ILi1024ELi7E" + extra in k]
        (c16,) = [v for k, v in grad.items() if "ILi1024ELi16E" + extra in k]
        assert c7["VGPRs"] <= 64 and c7["Occupancy"] == 8, (extra, c7)
        assert c16["VGPRs"] <= 128 and c16["Occupancy"] >= 4, (extra, c16)
