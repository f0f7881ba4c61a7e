"""Fused bf16 GELU-tanh (hand-written CDNA4 kernels, csrc/gelu_kernels.hip).

uint4 (8 x bf16) accesses reach parity with torch's gelu forward on MI355X
(0.195 vs 0.194 ms at (65536, 3072), both at the elementwise bandwidth limit;
round 1's pair-load variant was 26% slower — profiles/README.md), so there is
nothing to gain: kept as a correct, tested alternative, NOT wired into the
models.  k_gelu_bwd_colsum (ops/fused_bias_grad.py, off by default) shares
gelu_grad_f with the backward kernel here."""
from __future__ import annotations

import torch

from .. import _core
from .alignment import aligned


class _FusedGeluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = aligned(x.contiguous(), 16)  # the kernels load uint4
        y = torch.empty_like(x)
        s = torch.cuda.current_stream(x.device).cuda_stream
        _core.gelu_fwd(x.data_ptr(), y.data_ptr(), x.numel(), s)
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        dy = aligned(dy.contiguous(), 16)
        dx = torch.empty_like(x)
        s = torch.cuda.current_stream(x.device).cuda_stream
        _core.gelu_bwd(dy.data_ptr(), x.data_ptr(), dx.data_ptr(), x.numel(), s)
        return dx


def fused_gelu(x: torch.Tensor) -> torch.Tensor:
    return _FusedGeluFn.apply(x)


def can_use(x: torch.Tensor) -> bool:
    return x.is_cuda and x.dtype == torch.bfloat16 and x.numel() % 8 == 0
