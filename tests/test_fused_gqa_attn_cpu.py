"""ops/fused_gqa_attn.can_use off the device, and the floors of
tests/test_gpu_fused_gqa_attn.py against an fp32 evaluation of the kernels'
formulas at T = 1, the one length where the floors decide (dq = dk = 0,
dv = the group's sum of dout)."""
import pytest
import torch

from sharedtensor_amd.ops import fused_gqa_attn
from test_gpu_fused_gqa_attn import (expand, gqa_floors, gqa_reference,
                                     group_sum)

LOG2E = 1.4426950408889634


def test_can_use_false_off_device():
    q = torch.zeros(2, 8, 16, 64, dtype=torch.bfloat16)
    kv = torch.zeros(2, 2, 16, 64, dtype=torch.bfloat16)
    lse = torch.zeros(2, 8, 16)
    assert not fused_gqa_attn.can_use(q, kv, kv)  # CPU
    assert not fused_gqa_attn.can_use_backward(q, kv, kv, q, lse, q)
    with pytest.raises(ValueError):
        fused_gqa_attn.gqa_forward(q, kv, kv)
    with pytest.raises(ValueError):
        fused_gqa_attn.gqa_backward(q, kv, kv, q, lse, q, 0.125)


@pytest.mark.parametrize("G", [2, 4, 8])
@pytest.mark.parametrize("qscale", [1.0, 10.0])
def test_fp32_formulas_stay_inside_floors_at_t1(qscale, G):
    g = torch.Generator().manual_seed(5 + G)
    q, do = (torch.randn(2, 2 * G, 1, 64, generator=g).bfloat16()
             for _ in range(2))
    k, v = (torch.randn(2, 2, 1, 64, generator=g).bfloat16() for _ in range(2))
    q = (q.float() * qscale).bfloat16()
    scale = 0.125
    ref = gqa_reference(q, k, v, do, G, scale)
    fl = gqa_floors(ref, q, k, v, do, G, scale)
    # the kernels' formulas in fp32, the two 64-term sums in different
    # orders, dk and dv summed over the group head by head
    qf, dof = q.float(), do.float()
    kf, vf = expand(k, G).float(), expand(v, G).float()
    s = (qf * kf).sum(-1, keepdim=True)
    lse = s * scale                              # the forward at T = 1
    p = torch.exp2(s * (scale * LOG2E) - lse * LOG2E)
    o = vf                                       # out at T = 1, exact in bf16
    dp = (dof * vf).sum(-1, keepdim=True)
    delta = (dof.flip(-1) * o.flip(-1)).cumsum(-1)[..., -1:]
    ds = p * (dp - delta)
    got = dict(dq=scale * ds * kf, dk=scale * group_sum(ds * qf, G),
               dv=group_sum(p * dof, G))
    for name, x in got.items():
        err = (x.double() - ref[name]).abs()
        assert (err <= fl[name]).all(), (name, err.max(), fl[name].max())
