"""colsum_bf16 numerics vs the fp64 sum (bias-grad reduction kernel; measured
SLOWER than torch's reduce at GPT-2 shapes — kept as a tested building
block with the negative result recorded in profiles/README.md)."""
import pytest
import torch

import kernel_bounds as kb
from sharedtensor_amd import _core

pytestmark = pytest.mark.gpu


def colsum(x):
    R, C = x.shape
    o = torch.zeros(C, dtype=torch.float32, device="cuda")
    _core.colsum_bf16(x.data_ptr(), o.data_ptr(), R, C,
                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("R,C", [(65536, 768), (1000, 3072), (7, 64)])
def test_matches_fp32_sum(R, C):
    """fp32 accumulation in any order: (R + 1) * 2^-24 * sum|x| per column.
    That worst-case bound grows with R and at R = 65536 is wider than the
    fixed tolerance this test has always had, so both are asserted."""
    torch.cuda.set_device(0)
    torch.manual_seed(R + C)
    x = torch.randn(R, C, device="cuda").to(torch.bfloat16)
    xd = x.double()
    o = colsum(x)
    kb.assert_f32(o, xd.sum(0), (R + 1) * kb.U * xd.abs().sum(0),
                  "colsum", "out", f"randn/R={R}")
    torch.testing.assert_close(o, x.float().sum(0), rtol=1e-3, atol=1e-1)


@pytest.mark.parametrize("R,C", [(4099, 66), (2049, 4094), (7, 2),
                                 (1, 4096), (65536, 768)])
def test_exact_on_integer_inputs(R, C):
    """Integer-valued bf16 in [-4, 4]: every partial sum is an integer below
    2^24, so fp32 adds are exact in any order and the result equals the fp64
    sum bit for bit — a dropped or doubled row cannot hide in a tolerance."""
    g = torch.Generator(device="cuda").manual_seed(R * 3 + C)
    x = torch.randint(-4, 5, (R, C), device="cuda",
                      generator=g).to(torch.bfloat16)
    assert torch.equal(colsum(x).double(), x.double().sum(0))
