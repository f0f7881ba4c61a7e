"""Fused bf16 LayerNorm, with the residual add folded in.

Two generations of hand-written CDNA4 kernels back this module:

* csrc/add_ln_kernels.hip — wave-per-row kernels for C a multiple of 256 up
  to 1024 (GPT-2-small's 768 among them).  Forward computes
  ``x_new = x + delta`` and ``y = LN(x_new)`` in one pass; backward computes
  ``dx_total = LN_dx(dy) + d_x_new`` and the dgamma/dbeta (and delta-bias)
  column sums in one pass, so a residual block's LayerNorm moves 8
  activations instead of 13.  Column sums go through per-block partials and
  a small reducer that writes bf16: no atomics, backward repeats bit for bit.
* csrc/ln_kernels.hip — block-per-row kernels (one fwd pass, dx pass +
  register-accumulated dgamma/dbeta pass with fp32 atomics) for every other
  even C up to 4096; the residual add stays a torch op there.

fp32 statistics, bf16 tensors in/out.  torch's native LayerNorm backward
measured ~4.4x off the HBM roofline on MI355X for transformer shapes, which
is why neither path uses it.
"""
from __future__ import annotations

import torch

from .. import _core
from .alignment import aligned

MAX_C = 4096  # per-thread register accumulators in the dw/db kernel

# fp32 scratch for the column-sum partials, one per (device, stream); the
# kernels overwrite what they read, so it is never zeroed
_partials: dict = {}


def _wave_path(C: int, *tensors) -> bool:
    """True when the wave-per-row kernels cover this call: supported width
    and every tensor 8-byte aligned (they load and store 4 bf16 at a time)."""
    return (_core.add_ln_supported(C)
            and all(t is None or t.data_ptr() % 8 == 0 for t in tensors))


def _ptr(t) -> int:
    return t.data_ptr() if t is not None else 0


def _partials_for(device, C: int, stream: int) -> torch.Tensor:
    key = (device.index, stream)
    n = _core.add_ln_max_blocks() * 3 * C
    buf = _partials.get(key)
    if buf is None or buf.numel() < n:
        buf = torch.empty(n, dtype=torch.float32, device=device)
        _partials[key] = buf
    return buf


def _wave_fwd(x, delta, delta_bias, weight, bias, eps):
    C = x.shape[-1]
    R = x.numel() // C
    x_new = torch.empty_like(x) if delta is not None else None
    y = torch.empty_like(x)
    mean = torch.empty(R, dtype=torch.float32, device=x.device)
    rstd = torch.empty(R, dtype=torch.float32, device=x.device)
    if R:
        s = torch.cuda.current_stream(x.device).cuda_stream
        _core.add_ln_fwd(x.data_ptr(), _ptr(delta), _ptr(delta_bias),
                         weight.data_ptr(), _ptr(bias), _ptr(x_new),
                         y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), R, C,
                         float(eps), s)
    return x_new, y, mean, rstd


def _wave_bwd(dy, x_new, weight, mean, rstd, d_x_new, want_ddbias):
    """Returns (dx_total, dgamma, dbeta, ddbias) — the last three bf16[C]."""
    C = x_new.shape[-1]
    R = x_new.numel() // C
    dx = torch.empty_like(x_new)
    sums = torch.empty(3 if want_ddbias else 2, C, dtype=torch.bfloat16,
                       device=x_new.device)
    if R == 0:
        sums.zero_()
    else:
        stream = torch.cuda.current_stream(x_new.device).cuda_stream
        part = _partials_for(x_new.device, C, stream)
        _core.add_ln_bwd(dy.data_ptr(), x_new.data_ptr(), weight.data_ptr(),
                         mean.data_ptr(), rstd.data_ptr(), _ptr(d_x_new),
                         dx.data_ptr(), sums[0].data_ptr(),
                         sums[1].data_ptr(),
                         sums[2].data_ptr() if want_ddbias else 0,
                         part.data_ptr(), R, C, stream)
    return dx, sums[0], sums[1], sums[2] if want_ddbias else None


class _FusedLayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        x = x.contiguous()
        C = x.shape[-1]
        R = x.numel() // C
        ctx.has_bias = bias is not None
        ctx.wave = _wave_path(C, x, weight, bias)
        if ctx.wave:
            _, y, mean, rstd = _wave_fwd(x, None, None, weight, bias, eps)
            ctx.save_for_backward(x, weight, mean, rstd)
            return y
        # the block-per-row kernels load bf16 pairs as uint32
        x = aligned(x, 4)
        weight = aligned(weight, 4)
        bias = aligned(bias, 4)
        y = torch.empty_like(x)
        mean = torch.empty(R, dtype=torch.float32, device=x.device)
        rstd = torch.empty(R, dtype=torch.float32, device=x.device)
        s = torch.cuda.current_stream(x.device).cuda_stream
        _core.ln_fwd(x.data_ptr(), weight.data_ptr(),
                     bias.data_ptr() if bias is not None else 0,
                     y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), R, C,
                     float(eps), s)
        ctx.save_for_backward(x, weight, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, mean, rstd = ctx.saved_tensors
        dy = dy.contiguous()
        C = x.shape[-1]
        R = x.numel() // C
        if ctx.wave and dy.data_ptr() % 8 == 0:
            dx, dgamma, dbeta, _ = _wave_bwd(dy, x, w, mean, rstd, None,
                                             False)
            return dx, dgamma, dbeta if ctx.has_bias else None, None
        dy = aligned(dy, 4)
        dx = torch.empty_like(x)
        dwdb = torch.zeros(2 * C, dtype=torch.float32, device=x.device)
        dgamma, dbeta = dwdb[:C], dwdb[C:]
        s = torch.cuda.current_stream(x.device).cuda_stream
        _core.ln_bwd(dy.data_ptr(), x.data_ptr(), w.data_ptr(),
                     mean.data_ptr(), rstd.data_ptr(), dx.data_ptr(),
                     dgamma.data_ptr(), dbeta.data_ptr(), R, C, s)
        return (dx, dgamma.to(w.dtype),
                dbeta.to(w.dtype) if ctx.has_bias else None, None)


class _FusedAddLayerNormFn(torch.autograd.Function):
    """(x, delta) -> (x_new, y) on the wave-per-row kernels.  Saves x_new,
    weight, mean and rstd — the activation memory plain LN saves."""

    @staticmethod
    def forward(ctx, x, delta, weight, bias, eps, delta_bias):
        # an output the loss does not use arrives in backward as None, not
        # as a full-size zero tensor, and becomes a null pointer
        ctx.set_materialize_grads(False)
        x_new, y, mean, rstd = _wave_fwd(x, delta, delta_bias, weight, bias,
                                         eps)
        ctx.save_for_backward(x_new, weight, mean, rstd)
        ctx.has_bias = bias is not None
        ctx.has_delta_bias = delta_bias is not None
        return x_new, y

    @staticmethod
    def backward(ctx, d_x_new, dy):
        x_new, w, mean, rstd = ctx.saved_tensors
        if d_x_new is not None:
            d_x_new = d_x_new.contiguous()
        if dy is None:
            # only the residual stream was used: LN contributes nothing
            if d_x_new is None:
                return None, None, None, None, None, None
            ddb = None
            if ctx.has_delta_bias:
                ddb = d_x_new.reshape(-1, d_x_new.shape[-1]).sum(
                    0, dtype=torch.float32).to(d_x_new.dtype)
            return d_x_new, d_x_new, None, None, None, ddb
        dy = dy.contiguous()
        if dy.data_ptr() % 8 or (d_x_new is not None
                                 and d_x_new.data_ptr() % 8):
            # contiguous() keeps a misaligned view as it is; a copy aligns it
            dy = dy.clone()
            d_x_new = d_x_new.clone() if d_x_new is not None else None
        dx, dgamma, dbeta, ddb = _wave_bwd(dy, x_new, w, mean, rstd, d_x_new,
                                           ctx.has_delta_bias)
        return dx, dx, dgamma, dbeta if ctx.has_bias else None, None, ddb


def fused_layer_norm(x: torch.Tensor, weight: torch.Tensor,
                     bias: torch.Tensor, eps: float) -> torch.Tensor:
    return _FusedLayerNormFn.apply(x, weight, bias, eps)


def fused_add_layer_norm(x: torch.Tensor, delta: torch.Tensor,
                         weight: torch.Tensor, bias: torch.Tensor, eps: float,
                         delta_bias: torch.Tensor = None):
    """``x_new = x + delta [+ delta_bias]; y = LN(x_new)`` -> (x_new, y).

    ``x_new`` is the bf16 rounding of the fp32 sum, exactly what torch's add
    gives; statistics and ``y`` are computed from that rounded value.  In
    backward the gradient reaching ``x_new`` from later layers is added to
    LN's dx inside the kernel and the one resulting tensor is the gradient
    of both ``x`` and ``delta``; ``delta_bias`` receives its column sum.
    ``delta=None`` is plain LN (x_new is x).  Widths the wave-per-row
    kernels do not cover take a torch add followed by fused_layer_norm.
    """
    if delta is None:
        if delta_bias is not None:
            raise ValueError("delta_bias without delta")
        return x, fused_layer_norm(x, weight, bias, eps)
    if delta.shape != x.shape:
        raise ValueError("x and delta differ in shape")
    x = x.contiguous()
    delta = delta.contiguous()
    if delta_bias is not None:
        delta_bias = delta_bias.contiguous()
    if _wave_path(x.shape[-1], x, delta, weight, bias, delta_bias):
        return _FusedAddLayerNormFn.apply(x, delta, weight, bias, eps,
                                          delta_bias)
    if delta_bias is None:
        x_new = x + delta
    else:
        x_new = (x.float() + delta.float() + delta_bias.float()).to(x.dtype)
    return x_new, fused_layer_norm(x_new, weight, bias, eps)


def can_use(x: torch.Tensor, weight: torch.Tensor) -> bool:
    return (x.is_cuda and x.dtype == torch.bfloat16
            and weight.dtype == torch.bfloat16
            and x.shape[-1] == weight.numel() and x.shape[-1] <= MAX_C
            and x.shape[-1] % 2 == 0)
