"""Compiler resource report of the fused add+RMSNorm kernels (no GPU needed:
hipcc cross-compiles for gfx950).

At C=4096 a backward lane holds 64 fp32 column sums plus 128 dwords of
packed inputs; a spill to scratch would put extra memory traffic into a
kernel whose whole point is to move 8 activations instead of 13.
"""
import os
import re
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "sharedtensor_amd", "csrc")


def _report(tmp_path):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = [os.path.join(rocm, "bin", "hipcc"), "--offload-device-only", "-c",
           os.path.join(CSRC, "add_rms_kernels.hip"), "-o",
           str(tmp_path / "add_rms_dev.out"), "--offload-arch=gfx950",
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


def test_add_rms_kernels_have_no_scratch(tmp_path):
    kernels = _report(tmp_path)
    for name, res in sorted(kernels.items()):
        print(name, res)
    # one forward per width C = 512 * NV, one backward per width and per
    # presence of the residual-stream gradient, and the partials reducer
    want = ["k_add_rms_reduce"]
    want += [f"k_add_rms_fwdILi{nv}EE" for nv in range(1, 9)]
    want += [f"k_add_rms_bwdILi{nv}ELb{b}EE" for nv in range(1, 9)
             for b in (0, 1)]
    for tag in want:
        assert sum(tag in k for k in kernels) == 1, (tag, sorted(kernels))
    assert len(kernels) == len(want), sorted(kernels)
    for name, res in kernels.items():
        assert res["ScratchSize"] == 0, (name, res)
