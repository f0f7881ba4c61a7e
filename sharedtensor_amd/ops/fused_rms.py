"""Fused bf16 RMSNorm (hand-written CDNA4 kernels, csrc/ln_kernels.hip).

Round-1 weak #5: the Llama RMSNorm module upcast the whole (B, T, C)
activation to fp32 per call — the same cast-traffic tax FusedLayerNorm
removed for GPT-2 (profiles/README.md).  These kernels keep tensors bf16
end-to-end with fp32 statistics: fwd saves rstd, backward is one
single-reduction dx pass plus a register-accumulated dgamma pass.

`fused_add_rms_norm` folds the residual add in (csrc/add_rms_kernels.hip,
wave per row, C a multiple of 512 up to 4096): forward computes
``x_new = x + delta`` and ``y = RMSNorm(x_new)`` in one pass, backward
``dx_total = RMS_dx(dy) + d_x_new`` and dgamma in one pass, so a residual
block's norm moves 8 activations instead of 13.  dgamma goes through
per-block partials and a small reducer that writes bf16: no atomics, backward
repeats bit for bit.
"""
from __future__ import annotations

import os

import torch

from .. import _core
from .alignment import aligned

MAX_C = 4096  # per-thread register accumulators in the dgamma kernel


class _FusedRMSNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, eps):
        # the block-per-row kernels load bf16 pairs as uint32
        x = aligned(x.contiguous(), 4)
        weight = aligned(weight, 4)
        C = x.shape[-1]
        R = x.numel() // C
        y = torch.empty_like(x)
        rstd = torch.empty(R, dtype=torch.float32, device=x.device)
        s = torch.cuda.current_stream(x.device).cuda_stream
        _core.rms_fwd(x.data_ptr(), weight.data_ptr(), y.data_ptr(),
                      rstd.data_ptr(), R, C, float(eps), s)
        ctx.save_for_backward(x, weight, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, rstd = ctx.saved_tensors
        dy = aligned(dy.contiguous(), 4)
        C = x.shape[-1]
        R = x.numel() // C
        dx = torch.empty_like(x)
        dgamma = torch.zeros(C, dtype=torch.float32, device=x.device)
        s = torch.cuda.current_stream(x.device).cuda_stream
        _core.rms_bwd(dy.data_ptr(), x.data_ptr(), w.data_ptr(),
                      rstd.data_ptr(), dx.data_ptr(), dgamma.data_ptr(),
                      R, C, s)
        return dx, dgamma.to(w.dtype), None


def fused_rms_norm(x: torch.Tensor, weight: torch.Tensor,
                   eps: float) -> torch.Tensor:
    return _FusedRMSNormFn.apply(x, weight, eps)


# fp32 scratch for the dgamma partials of the add+RMS backward, one per
# (device, stream); the kernels overwrite what they read, so it is never
# zeroed
_partials: dict = {}


def _wave_path(C: int, *tensors) -> bool:
    """True when the wave-per-row add+RMS kernels cover this call: supported
    width and every tensor 16-byte aligned (they move 8 bf16 at a time)."""
    return (_core.add_rms_supported(C)
            and all(t is None or t.data_ptr() % 16 == 0 for t in tensors))


def _partials_for(device, C: int, stream: int) -> torch.Tensor:
    key = (device.index, stream)
    n = _core.add_rms_max_blocks() * C
    buf = _partials.get(key)
    if buf is None or buf.numel() < n:
        buf = torch.empty(n, dtype=torch.float32, device=device)
        _partials[key] = buf
    return buf


class _FusedAddRMSNormFn(torch.autograd.Function):
    """(x, delta) -> (x_new, y) on the wave-per-row kernels
    (csrc/add_rms_kernels.hip).  Saves x_new, weight and rstd — the
    activation memory plain RMSNorm saves."""

    @staticmethod
    def forward(ctx, x, delta, weight, eps):
        # an output the loss does not use arrives in backward as None, not
        # as a full-size zero tensor, and becomes a null pointer
        ctx.set_materialize_grads(False)
        C = x.shape[-1]
        R = x.numel() // C
        x_new = torch.empty_like(x)
        y = torch.empty_like(x)
        rstd = torch.empty(R, dtype=torch.float32, device=x.device)
        if R:
            s = torch.cuda.current_stream(x.device).cuda_stream
            _core.add_rms_fwd(x.data_ptr(), delta.data_ptr(),
                              weight.data_ptr(), x_new.data_ptr(),
                              y.data_ptr(), rstd.data_ptr(), R, C, float(eps),
                              s)
        ctx.save_for_backward(x_new, weight, rstd)
        return x_new, y

    @staticmethod
    def backward(ctx, d_x_new, dy):
        x_new, w, rstd = ctx.saved_tensors
        if d_x_new is not None:
            d_x_new = d_x_new.contiguous()
        if dy is None:
            # only the residual stream was used: the norm contributes nothing
            return d_x_new, d_x_new, None, None
        dy = dy.contiguous()
        if dy.data_ptr() % 16 or (d_x_new is not None
                                  and d_x_new.data_ptr() % 16):
            # contiguous() keeps a misaligned view as it is; a copy aligns it
            dy = dy.clone()
            d_x_new = d_x_new.clone() if d_x_new is not None else None
        C = x_new.shape[-1]
        R = x_new.numel() // C
        dx = torch.empty_like(x_new)
        dgamma = torch.empty(C, dtype=torch.bfloat16, device=x_new.device)
        if R == 0:
            dgamma.zero_()
        else:
            stream = torch.cuda.current_stream(x_new.device).cuda_stream
            part = _partials_for(x_new.device, C, stream)
            _core.add_rms_bwd(dy.data_ptr(), x_new.data_ptr(), w.data_ptr(),
                              rstd.data_ptr(),
                              d_x_new.data_ptr() if d_x_new is not None else 0,
                              dx.data_ptr(), dgamma.data_ptr(),
                              part.data_ptr(), R, C, stream)
        return dx, dx, dgamma, None


def fused_add_rms_norm(x: torch.Tensor, delta: torch.Tensor,
                       weight: torch.Tensor, eps: float):
    """``x_new = x + delta; y = RMSNorm(x_new)`` -> (x_new, y).

    ``x_new`` is the bf16 rounding of the fp32 sum, exactly what torch's add
    gives; rstd and ``y`` are computed from that rounded value.  In backward
    the gradient reaching ``x_new`` from later layers is added to the norm's
    dx inside the kernel and the one resulting tensor is the gradient of both
    ``x`` and ``delta``.  ``delta=None`` is plain ``fused_rms_norm`` (x_new
    is x).  Widths or alignments the wave-per-row kernels do not cover take
    a torch add followed by ``fused_rms_norm``.
    """
    if delta is None:
        return x, fused_rms_norm(x, weight, eps)
    if delta.shape != x.shape:
        raise ValueError("x and delta differ in shape")
    x = x.contiguous()
    delta = delta.contiguous()
    if _wave_path(x.shape[-1], x, delta, weight):
        return _FusedAddRMSNormFn.apply(x, delta, weight, eps)
    x_new = x + delta
    return x_new, fused_rms_norm(x_new, weight, eps)


def can_use_add(x: torch.Tensor, weight: torch.Tensor) -> bool:
    """Whether the model should route a residual add through
    `fused_add_rms_norm`; SHTENS_NO_FUSED_ADD_RMS=1 restores add-then-norm."""
    if os.environ.get("SHTENS_NO_FUSED_ADD_RMS") == "1":  # A/B knob
        return False
    return can_use(x, weight)


def can_use(x: torch.Tensor, weight: torch.Tensor) -> bool:
    if os.environ.get("SHTENS_NO_FUSED_RMS") == "1":  # A/B measurement knob
        return False
    return (x.is_cuda and x.dtype == torch.bfloat16
            and weight.dtype == torch.bfloat16
            and x.shape[-1] == weight.numel() and x.shape[-1] <= MAX_C
            and x.shape[-1] % 2 == 0)
