"""Fused bf16 cross-entropy (hand-written CDNA4 kernels, csrc/ce_kernels.hip).

Replaces torch's softmax-forward + softmax-backward pair (and its fp32
intermediates) for the (B*T, vocab) bf16 logits of the language-model head,
fp32 math, bf16 tensors, reduction='mean' semantics.

When the logits need a gradient, forward runs the one-pass kernel: a single
read of the logits gives the loss and the bf16 dlogits for an upstream
gradient of 1, and backward only has to check on the device that the
upstream gradient really is 1 (it recomputes the buffer otherwise).  Without
a gradient, or for a vocabulary too large for one block's registers, forward
is the stats-only two-pass kernel and backward the classic dlogits pass.
SHTENS_CE_ONEPASS=0 forces that two-kernel path (for A/B measurements).
"""
from __future__ import annotations

import os

import torch

from .. import _core


def _onepass_enabled() -> bool:
    return os.environ.get("SHTENS_CE_ONEPASS", "1") != "0"


class _FusedCEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, targets):
        logits = logits.contiguous()
        R, V = logits.shape
        t32 = targets.to(torch.int32).contiguous()
        loss = torch.empty(R, dtype=torch.float32, device=logits.device)
        row_lse = torch.empty(R, dtype=torch.float32, device=logits.device)
        s = torch.cuda.current_stream(logits.device).cuda_stream
        ctx.onepass = (ctx.needs_input_grad[0] and _onepass_enabled()
                       and V <= _core.ce_fwd_grad_max_v())
        if ctx.onepass:
            # same peak memory as allocating it in backward: both points
            # are the activation peak
            dlogits = torch.empty_like(logits)
            _core.ce_fwd_grad(logits.data_ptr(), t32.data_ptr(),
                              loss.data_ptr(), row_lse.data_ptr(),
                              dlogits.data_ptr(), 1.0 / R, R, V, s)
            ctx.save_for_backward(logits, t32, row_lse, dlogits)
        else:
            row_m = torch.empty(R, dtype=torch.float32, device=logits.device)
            _core.ce_fwd(logits.data_ptr(), t32.data_ptr(), loss.data_ptr(),
                         row_m.data_ptr(), row_lse.data_ptr(), R, V, s)
            ctx.save_for_backward(logits, t32, row_lse)
        return loss.mean()

    @staticmethod
    def backward(ctx, dloss):
        logits, t32, row_lse = ctx.saved_tensors[:3]
        R, V = logits.shape
        g = dloss.to(device=logits.device, dtype=torch.float32).contiguous()
        s = torch.cuda.current_stream(logits.device).cuda_stream
        # the precomputed buffer serves the first backward only: after that
        # it may be somebody's .grad (retain_graph=True)
        first = ctx.onepass
        ctx.onepass = False
        dlogits = ctx.saved_tensors[3] if first else torch.empty_like(logits)
        _core.ce_bwd(logits.data_ptr(), t32.data_ptr(), row_lse.data_ptr(),
                     dlogits.data_ptr(), g.data_ptr(), 1.0 / R, R, V, s,
                     skip_if_unit=first)
        return dlogits, None


def fused_cross_entropy(logits: torch.Tensor, targets: torch.Tensor) -> torch.Tensor:
    """Mean cross-entropy over rows; logits (R, V) bf16 cuda, targets (R,)."""
    return _FusedCEFn.apply(logits, targets)


def can_use(logits: torch.Tensor) -> bool:
    return (logits.is_cuda and logits.dtype == torch.bfloat16
            and logits.dim() == 2)
