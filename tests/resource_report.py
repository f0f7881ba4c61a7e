"""The compiler's resource report of one HIP kernel file, for the
tests/test_*_resource_usage.py files (no GPU needed: hipcc cross-compiles
for gfx950)."""
import os
import re
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "sharedtensor_amd", "csrc")

_FIELDS = {
    "VGPRs": "VGPRs",
    "AGPRs": "AGPRs",
    "TotalSGPRs": "SGPRs",
    "ScratchSize [bytes/lane]": "ScratchSize",
    "Occupancy [waves/SIMD]": "Occupancy",
    "LDS Size [bytes/block]": "LDS",
    "VGPRs Spill": "VGPRs Spill",
    "SGPRs Spill": "SGPRs Spill",
}
_FIELD = re.compile(r"remark:\s+(%s): (\d+)"
                    % "|".join(re.escape(f) for f in _FIELDS))


def kernel_resources(src, tmp_path):
    """Compiles csrc/<src> for gfx950 with
    -Rpass-analysis=kernel-resource-usage and returns
    {mangled kernel name: {"VGPRs", "AGPRs", "SGPRs", "ScratchSize",
    "Occupancy", "LDS", "VGPRs Spill", "SGPRs Spill"}}."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = [os.path.join(rocm, "bin", "hipcc"), "--offload-device-only", "-c",
           os.path.join(CSRC, src), "-o", str(tmp_path / (src + ".out")),
           "--offload-arch=gfx950", "-std=c++20", "-O3", "-DSHAMD_WITH_HIP",
           "-DNDEBUG", f"-I{CSRC}", f"-I{rocm}/include",
           "-Rpass-analysis=kernel-resource-usage"]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    kernels, name = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels[name] = {}
            continue
        m = _FIELD.search(line)
        if m and name:
            kernels[name][_FIELDS[m.group(1)]] = int(m.group(2))
    return kernels
