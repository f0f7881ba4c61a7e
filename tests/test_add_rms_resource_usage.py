"""Compiler resource report of the fused add+RMSNorm kernels (no GPU needed:
hipcc cross-compiles for gfx950).

At C=4096 a backward lane holds 64 fp32 column sums plus 128 dwords of
packed inputs; a spill to scratch would put extra memory traffic into a
kernel whose whole point is to move 8 activations instead of 13.
"""
from resource_report import kernel_resources


def test_add_rms_kernels_have_no_scratch(tmp_path):
    kernels = kernel_resources("add_rms_kernels.hip", tmp_path)
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
