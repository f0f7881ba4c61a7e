"""ops/fused_attn.can_use_backward off the device, and the floors of
tests/attn_bwd_floors.py against an fp32 evaluation of the kernel's formulas
at T = 1, the one case where the floors decide (dq = dk = 0, dv = dout)."""
import pytest
import torch

from attn_bwd_floors import floors, reference
from sharedtensor_amd.ops import fused_attn

LOG2E = 1.4426950408889634


def test_can_use_backward_false_off_device():
    bf = torch.zeros(2, 3, 16, 64, dtype=torch.bfloat16)
    lse = torch.zeros(2, 3, 16)
    assert not fused_attn.can_use_backward(bf, bf, bf, bf, lse, bf)  # CPU
    with pytest.raises(ValueError):
        fused_attn.attn_backward(bf, bf, bf, bf, lse, bf, 0.125)


@pytest.mark.parametrize("qscale", [1.0, 10.0])
def test_fp32_formulas_stay_inside_floors_at_t1(qscale):
    g = torch.Generator().manual_seed(5)
    q, k, v, do = (torch.randn(2, 3, 1, 64, generator=g).bfloat16()
                   for _ in range(4))
    q = (q.float() * qscale).bfloat16()
    scale = 0.125
    ref = reference(q, k, v, do, scale)
    fl = floors(ref, q, k, v, do, scale)
    # the kernels' formulas in fp32, the two 64-term sums in different orders
    qf, kf, vf, dof = (t.float() for t in (q, k, v, do))
    s = (qf * kf).sum(-1, keepdim=True)
    lse = s * scale                              # the forward at T = 1
    p = torch.exp2(s * (scale * LOG2E) - lse * LOG2E)
    o = vf                                       # out at T = 1, exact in bf16
    dp = (dof @ vf.transpose(-1, -2))
    delta = (dof.flip(-1) * o.flip(-1)).cumsum(-1)[..., -1:]
    ds = p * (dp - delta)
    got = dict(dq=scale * ds * kf, dk=scale * ds * qf, dv=p * dof)
    for name in ("dq", "dk", "dv"):
        err = (got[name].double() - ref[name]).abs()
        assert (err <= fl[name]).all(), (name, err.max(), fl[name].max())
