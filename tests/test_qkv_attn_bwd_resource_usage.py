"""Compiler resource report (no GPU needed) of the kernels of the packed
attention backward: the two backward kernels, whose column-sum epilogue is a
runtime branch of the same kernels, and k_colsum_reduce.  No scratch, no
spills, and the occupancy the headers of csrc/attn_bwd_kernels.hip and
csrc/bias_grad_kernels.hip state."""
import pytest

import build
from resource_report import kernel_resources

# kernel -> (file, occupancy in waves/SIMD, LDS bytes)
PLAN = {
    "k_attn_bwd_dq": ("attn_bwd_kernels.hip", 3, 32 * 1024),
    "k_attn_bwd_dkdv": ("attn_bwd_kernels.hip", 2, 33 * 1024),
    "k_colsum_reduce": ("bias_grad_kernels.hip", 8, 20 * 1024),
}


@pytest.fixture(scope="module")
def reports(tmp_path_factory):
    out = {}
    for src in sorted({p[0] for p in PLAN.values()}):
        with pytest.MonkeyPatch.context() as mp:  # hipcc appends these itself
            mp.setenv("HIPCC_COMPILE_FLAGS_APPEND",
                      " ".join(build.EXTRA_FLAGS.get(src, [])))
            out[src] = kernel_resources(
                src, tmp_path_factory.mktemp(src.split(".")[0]))
    return out


@pytest.mark.parametrize("name", sorted(PLAN))
def test_kernel_follows_plan(reports, name):
    src, waves, lds = PLAN[name]
    (res,) = [v for k, v in reports[src].items() if name in k]
    assert res["ScratchSize"] == 0, res
    assert res["VGPRs Spill"] == 0 and res["SGPRs Spill"] == 0, res
    assert res["AGPRs"] == 0, res
    assert res["Occupancy"] == waves, res
    assert res["LDS"] == lds, res


def test_column_sum_epilogue_is_compiled_in(reports):
    """Each backward kernel is compiled once: the column-sum epilogue is a
    runtime branch of the kernels the plan above holds, so the figures there
    are the figures of the column-sum build, not of a plain twin."""
    names = list(reports["attn_bwd_kernels.hip"])
    assert sum("k_attn_bwd_dq" in n for n in names) == 1
    assert sum("k_attn_bwd_dkdv" in n for n in names) == 1
