"""Bias gradients of the GPT-2 `fc` and `qkv` Linears, taken in the pass
that already streams the data (csrc/bias_grad_kernels.hip).

The forward GEMMs keep their bias in the epilogue — the caller passes
``b.detach()`` to ``F.linear`` so autograd launches no bias reduce — and the
two Functions here give the bias its gradient instead:

* ``bias_gelu_bgrad(pre, b)``: forward is torch's own tanh GELU of ``pre``
  (the GEMM output, bias already added).  Backward computes
  ``dpre = dy * gelu'(pre)`` and the column sums of the bf16 ``dpre`` in one
  kernel; torch ran GeluBackward and then read ``dpre`` again to reduce it.
* ``qkv_split_bgrad(qkv, b)``: forward returns the q, k, v views.  Backward
  packs dq, dk, dv into ``dqkv`` and sums its columns in one kernel; torch
  ran a cat and then read ``dqkv`` again to reduce it.

Only the qkv half is wired into models/gpt2.py by default: the GELU half
measured slower than the two torch kernels it replaces (profiles/r07/).

Column sums go through per-block fp32 partials and a small second stage that
writes bf16: fixed order, no atomics, so backward repeats bit for bit.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from .. import _core
from .alignment import aligned

# fp32 scratch for the column-sum partials, one per (device, stream); the
# kernels overwrite what they read, so it is never zeroed
_partials: dict = {}


def _partials_for(device, ncols: int, stream: int) -> torch.Tensor:
    key = (device.index, stream)
    n = _core.bias_grad_partial_floats(ncols)
    buf = _partials.get(key)
    if buf is None or buf.numel() < n:
        buf = torch.empty(n, dtype=torch.float32, device=device)
        _partials[key] = buf
    return buf


def _bf16_cuda(*tensors) -> None:
    """The kernels read and write bf16 on the GPU and nothing else."""
    for t in tensors:
        if not t.is_cuda or t.dtype != torch.bfloat16:
            raise TypeError("fused_bias_grad: expected a CUDA bfloat16 "
                            f"tensor, got {t.dtype} on {t.device}")


def _vec(t: torch.Tensor) -> torch.Tensor:
    """Contiguous and 16-byte aligned: the kernels load uint4."""
    return aligned(t.contiguous(), 16)


class _BiasGeluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pre, b):
        _bf16_cuda(pre, b)
        if b.numel() != pre.shape[-1]:
            raise ValueError("bias and pre-activation widths differ")
        ctx.save_for_backward(pre)
        return F.gelu(pre, approximate="tanh")

    @staticmethod
    def backward(ctx, dy):
        (pre,) = ctx.saved_tensors
        _bf16_cuda(dy)
        C = pre.shape[-1]
        R = pre.numel() // C
        pre = _vec(pre)
        dy = _vec(dy)
        dpre = torch.empty_like(pre)
        db = torch.empty(C, dtype=torch.bfloat16, device=pre.device)
        if R == 0:
            return dpre, db.zero_()
        s = torch.cuda.current_stream(pre.device).cuda_stream
        part = _partials_for(pre.device, C, s)
        _core.gelu_bwd_colsum(dy.data_ptr(), pre.data_ptr(), dpre.data_ptr(),
                              db.data_ptr(), part.data_ptr(), R, C, s)
        return dpre, db


class _QkvSplitFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, b):
        _bf16_cuda(qkv, b)
        if b.numel() != qkv.shape[-1] or b.numel() % 3:
            raise ValueError("bias width must be the qkv width, 3 * C")
        ctx.shape = qkv.shape
        C = qkv.shape[-1] // 3
        q, k, v = qkv.split(C, dim=-1)
        return q, k, v

    @staticmethod
    def backward(ctx, dq, dk, dv):
        shape = ctx.shape
        C = shape[-1] // 3
        _bf16_cuda(dq, dk, dv)
        dq, dk, dv = _vec(dq), _vec(dk), _vec(dv)
        R = dq.numel() // C
        dqkv = torch.empty(shape, dtype=dq.dtype, device=dq.device)
        db = torch.empty(3 * C, dtype=torch.bfloat16, device=dq.device)
        if R == 0:
            return dqkv, db.zero_()
        s = torch.cuda.current_stream(dq.device).cuda_stream
        part = _partials_for(dq.device, 3 * C, s)
        _core.pack3_colsum(dq.data_ptr(), dk.data_ptr(), dv.data_ptr(),
                           dqkv.data_ptr(), db.data_ptr(), part.data_ptr(),
                           R, C, s)
        return dqkv, db


def bias_gelu_bgrad(pre: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """``gelu(pre)`` (tanh approximation) whose backward also hands ``b``
    the column sums of ``dpre``.  ``pre`` must already contain ``b``."""
    return _BiasGeluFn.apply(pre, b)


def qkv_split_bgrad(qkv: torch.Tensor, b: torch.Tensor):
    """``qkv.split(C, dim=-1)`` whose backward also hands ``b`` the column
    sums of the packed gradient.  ``qkv`` must already contain ``b``."""
    return _QkvSplitFn.apply(qkv, b)


def _common(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor) -> bool:
    # the Linear's output and the gradients are what the kernels touch; the
    # Functions align those themselves (_vec)
    return (x.is_cuda and x.dtype == torch.bfloat16
            and w.dtype == torch.bfloat16
            and b is not None and b.dtype == torch.bfloat16)


def can_use_gelu(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor) -> bool:
    """``x`` is the input of the fc Linear with weight ``w`` and bias ``b``."""
    return _common(x, w, b) and b.numel() % 8 == 0


def can_use_qkv(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor) -> bool:
    """``x`` is the input of the qkv Linear with weight ``w`` and bias ``b``."""
    return _common(x, w, b) and b.numel() % 24 == 0
