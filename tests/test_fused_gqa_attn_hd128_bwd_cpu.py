"""ops/fused_gqa_attn's head-dim-128 backward off the device:
can_use_backward_hd128 is False, and gqa_backward_hd128 and the Function asked
for it raise."""
import pytest
import torch

from sharedtensor_amd.ops import fused_gqa_attn


def test_hd128_backward_refuses_off_device():
    q = torch.zeros(2, 8, 16, 128, dtype=torch.bfloat16)
    kv = torch.zeros(2, 2, 16, 128, dtype=torch.bfloat16)
    lse = torch.zeros(2, 8, 16)
    assert not fused_gqa_attn.can_use_backward_hd128(q, kv, kv, q, lse, q)
    with pytest.raises(ValueError):
        fused_gqa_attn.gqa_backward_hd128(q, kv, kv, q, lse, q)
    with pytest.raises(ValueError):
        fused_gqa_attn.fused_causal_gqa_attention(q, kv, kv,
                                                  own_backward_hd128=True)
