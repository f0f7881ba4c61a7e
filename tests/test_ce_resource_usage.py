"""Compiler resource report of the cross-entropy kernels (no GPU needed:
hipcc cross-compiles for gfx950).

k_ce_fwd_grad keeps a whole vocabulary row in registers; a spill to scratch
would turn its single HBM read into several, and more than 64 VGPRs in a
7-chunk (GPT-2) instantiation would leave one row per CU instead of two.
All three row policies (plain, masking only, smoothing / z-loss) hold the
bound.
"""
import pytest

from resource_report import kernel_resources


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return kernel_resources("ce_kernels.hip",
                            tmp_path_factory.mktemp("ce_resource_usage"))


def _row_budget(kernels, policy):
    """<1024, NCHUNK, policy>; 1024 threads = 4 waves/SIMD per block"""
    grad = {k: v for k, v in kernels.items() if "k_ce_fwd_grad" in k}
    assert len(grad) == 6, sorted(kernels)
    (c7,) = [v for k, v in grad.items() if "ILi1024ELi7E" + policy in k]
    (c16,) = [v for k, v in grad.items() if "ILi1024ELi16E" + policy in k]
    assert c7["VGPRs"] <= 64 and c7["Occupancy"] == 8, (policy, c7)
    assert c16["VGPRs"] <= 128 and c16["Occupancy"] >= 4, (policy, c16)


def test_ce_fwd_grad_has_no_scratch_and_two_rows_per_cu(kernels):
    _row_budget(kernels, "NS_7CePlainE")
    # no CE kernel may spill
    for name, res in kernels.items():
        assert res["ScratchSize"] == 0, (name, res)


def test_ce_opts_kernels_have_no_scratch_and_keep_the_row_budget(kernels):
    # 19: the scan;
    # k_ce_fwd_grad <1024, 7 | 16> x 3 policies = 6;
    # k_ce_fwd <256> x 3 policies + <512, plain> = 4;
    # k_ce_bwd <256, skip off | on> x 3 policies + <512, off | on, plain> = 8
    assert len(kernels) == 19, sorted(kernels)
    assert sum("k_ce_opts_scan" in k for k in kernels) == 1, sorted(kernels)
    assert sum("8k_ce_fwdI" in k for k in kernels) == 4, sorted(kernels)
    assert sum("8k_ce_bwdI" in k for k in kernels) == 8, sorted(kernels)
    for name, res in kernels.items():
        assert res["ScratchSize"] == 0, (name, res)
    for policy in ("NS_8CeMaskedE", "NS_13CeMaskedExtraE"):
        _row_budget(kernels, policy)
