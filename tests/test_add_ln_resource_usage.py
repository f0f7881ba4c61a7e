"""Compiler resource report of the fused add+LayerNorm kernels (no GPU
needed: hipcc cross-compiles for gfx950).

At C=1024 with the delta-bias sum a backward lane holds 48 fp32 column sums
next to the packed inputs of its row; a spill to scratch would put extra
memory traffic into a kernel whose whole point is to move 8 activations
instead of 13.  The backward's only LDS is the `red` array of the wave
combine, NS rows of C floats (NS = 2: dgamma, dbeta; 3 with d delta_bias).
"""
import re

from resource_report import kernel_resources


def test_add_ln_kernels_have_no_scratch_and_the_declared_lds(tmp_path):
    kernels = kernel_resources("add_ln_kernels.hip", tmp_path)
    for name, res in sorted(kernels.items()):
        print(name, res)
    # one forward per width C = 256 * NV, one backward per width and per
    # presence of the delta-bias sum, and the benchmark arm's reducer
    want = ["k_add_ln_reduce"]
    want += [f"k_add_ln_fwdILi{nv}EE" for nv in range(1, 5)]
    want += [f"k_add_ln_bwdILi{nv}ELb{b}EE" for nv in range(1, 5)
             for b in (0, 1)]
    for tag in want:
        assert sum(tag in k for k in kernels) == 1, (tag, sorted(kernels))
    assert len(kernels) == len(want), sorted(kernels)
    for name, res in kernels.items():
        assert res["ScratchSize"] == 0, (name, res)
        m = re.search(r"k_add_ln_bwdILi(\d)ELb([01])EE", name)
        if m:
            nv, ddb = int(m.group(1)), int(m.group(2))
            assert res["LDS"] == (3 if ddb else 2) * 256 * nv * 4, (name, res)
        elif "k_add_ln_fwd" in name:
            assert res["LDS"] == 0, (name, res)
