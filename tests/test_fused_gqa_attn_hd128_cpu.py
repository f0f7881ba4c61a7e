"""ops/fused_gqa_attn at head dim 128 off the device: can_use is False and
the forward, the backward and the Function raise."""
import pytest
import torch

from sharedtensor_amd.ops import fused_gqa_attn


def test_hd128_can_use_false_off_device():
    q = torch.zeros(2, 8, 16, 128, dtype=torch.bfloat16)
    kv = torch.zeros(2, 2, 16, 128, dtype=torch.bfloat16)
    lse = torch.zeros(2, 8, 16)
    assert not fused_gqa_attn.can_use(q, kv, kv)  # CPU
    assert not fused_gqa_attn.can_use_backward(q, kv, kv, q, lse, q)
    with pytest.raises(ValueError):
        fused_gqa_attn.gqa_forward(q, kv, kv)
    with pytest.raises(ValueError):
        fused_gqa_attn.gqa_backward(q, kv, kv, q, lse, q)
    with pytest.raises(ValueError):
        fused_gqa_attn.fused_causal_gqa_attention(q, kv, kv)
