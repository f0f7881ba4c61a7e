"""ops/fused_attn.can_use turns down what the kernel does not take, and the
model then keeps the SDPA path: on the CPU, with the tiny config (fp32, head
dim 32), whatever the FUSE_ATTN_FWD flag says."""
import pytest
import torch

from sharedtensor_amd.models import gpt2
from sharedtensor_amd.ops import fused_attn


def test_can_use_false_off_device():
    bf = torch.zeros(2, 3, 16, 64, dtype=torch.bfloat16)
    f32 = torch.zeros(2, 3, 16, 64)
    d32 = torch.zeros(2, 3, 16, 32, dtype=torch.bfloat16)
    kv1 = torch.zeros(2, 1, 16, 64, dtype=torch.bfloat16)
    assert not fused_attn.can_use(bf, bf, bf)      # CPU
    assert not fused_attn.can_use(f32, f32, f32)   # fp32
    assert not fused_attn.can_use(d32, d32, d32)   # D = 32
    assert not fused_attn.can_use(bf, kv1, kv1)    # mismatched head counts
    with pytest.raises(ValueError):
        fused_attn.attn_forward(bf, bf, bf)


@pytest.mark.parametrize("env", [None, "1"])
def test_tiny_model_keeps_sdpa_path(monkeypatch, env):
    if env is None:
        monkeypatch.delenv("SHTENS_FUSED_ATTN", raising=False)
    else:
        monkeypatch.setenv("SHTENS_FUSED_ATTN", env)

    def boom(*a, **k):
        raise AssertionError("fused attention ran on inputs it cannot take")
    monkeypatch.setattr(fused_attn, "fused_causal_attention", boom)

    torch.manual_seed(0)
    model = gpt2.GPT2(gpt2.GPT2Config.tiny())
    idx = torch.randint(0, 256, (2, 32))

    def run(flag):
        monkeypatch.setattr(gpt2, "FUSE_ATTN_FWD", flag)
        model.zero_grad(set_to_none=True)
        _, loss = model(idx, idx)
        loss.backward()
        return loss.detach().clone(), \
            model.blocks[0].attn.qkv.weight.grad.clone()

    loss_on, g_on = run(True)
    loss_off, g_off = run(False)
    assert torch.equal(loss_on, loss_off) and torch.equal(g_on, g_off)
