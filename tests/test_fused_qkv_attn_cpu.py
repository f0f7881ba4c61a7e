"""Off the device the packed qkv + attention node never applies: with
SHTENS_FUSED_QKV_ATTN 0 and 1 the tiny model gives the same loss and the
same gradients, and ``can_use_packed`` says no.  Plus the derived column-sum
bound of colsum_bounds.py against an fp32 evaluation of the kernels' tree."""
import numpy as np
import pytest
import torch

from colsum_bounds import ATTN_EPILOGUE_ADDS, colsum_check, reduce_adds
from sharedtensor_amd.models.gpt2 import GPT2, GPT2Config
from sharedtensor_amd.ops import fused_attn


def _step(monkeypatch, flag):
    monkeypatch.setenv("SHTENS_FUSED_QKV_ATTN", flag)
    torch.manual_seed(0)
    model = GPT2(GPT2Config.tiny())
    for p in model.parameters():  # biases are zero-initialised
        if p.dim() == 1:
            torch.nn.init.normal_(p, std=0.1)
    idx = torch.randint(0, 256, (2, 33), generator=torch.Generator().manual_seed(1))
    _, loss = model(idx[:, :-1], idx[:, 1:])
    loss.backward()
    return loss.detach(), {n: p.grad for n, p in model.named_parameters()}


def test_flag_is_a_no_op_on_the_cpu(monkeypatch):
    calls = []
    real = fused_attn.fused_qkv_causal_attention
    monkeypatch.setattr(fused_attn, "fused_qkv_causal_attention",
                        lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    l0, g0 = _step(monkeypatch, "0")
    l1, g1 = _step(monkeypatch, "1")
    assert not calls
    assert torch.equal(l0, l1)
    assert g0.keys() == g1.keys()
    for name in g0:
        assert torch.equal(g0[name], g1[name]), name


def test_can_use_packed_false_off_device():
    qkv = torch.zeros(2, 16, 3 * 128, dtype=torch.bfloat16)
    b = torch.zeros(3 * 128, dtype=torch.bfloat16)
    assert not fused_attn.can_use_packed(qkv, b, 2)
    with pytest.raises(ValueError):
        fused_attn.fused_qkv_causal_attention(qkv, b, 2)


def test_bound_holds_for_an_fp32_evaluation_of_the_tree():
    """bf16 values summed in fp32 in the kernels' order (4 rows, 8 lanes, 4
    waves per 128-row block, then the second stage's row groups) stay inside
    the bound: a bound an fp32 evaluation could not meet would be one no
    kernel can."""
    f = np.float32
    g = torch.Generator().manual_seed(9)
    R, N, G = 128 * 70, 24, 70
    x = (torch.randn(R, N, generator=g) * 3).bfloat16()
    a = x.float().numpy().reshape(G, 4, 4, 8, N)     # block, wave, pass, lane
    lane = np.zeros((G, 4, 8, N), f)
    for p in range(4):
        lane = lane + a[:, :, p]
    for m in (1, 2, 4):                              # butterfly over 8 lanes
        lane = lane + lane[:, :, np.arange(8) ^ m]
    part = np.zeros((G, N), f)
    for w in range(4):
        part = part + lane[:, w, 0]
    rg = np.zeros((64, N), f)
    for r in range(G):                               # row group r % 64
        rg[r % 64] = rg[r % 64] + part[r]
    q4 = np.zeros((16, N), f)
    for i in range(64):
        q4[i // 4] = q4[i // 4] + rg[i]
    tot = np.zeros(N, f)
    for i in range(16):
        tot = tot + q4[i]
    got = torch.from_numpy(tot).bfloat16()
    worst = colsum_check(got, x, ATTN_EPILOGUE_ADDS + reduce_adds(G), "emu")
    assert 0 <= worst <= 1
