"""Causal bf16 attention for head dim 64 with a hand-written forward kernel
(csrc/attn_kernels.hip).

``fused_causal_attention(q, k, v)`` takes the (B, H, T, 64) views the model
builds from the packed qkv GEMM output and reads them in place through their
strides.  The forward writes ``out`` as contiguous (B, T, H, 64), returned as
its (B, H, T, 64) view, the layout the aten efficient-attention op returns,
so ``transpose(1, 2).contiguous()`` in the model stays a no-op, and ``lse``
(B, H, T) fp32, the natural log of the softmax denominator.  The backward is
the aten efficient-attention backward autograd runs on the SDPA path, fed
with our ``out`` and ``lse``: the backward kernels do not change.

``can_use`` says whether the kernel takes the inputs; callers keep the SDPA
path for everything else.  A call that passes ``can_use`` and then fails is
an error, never a silent fall-back.
"""
from __future__ import annotations

import math

import torch

from .. import _core

HEAD_DIM = 64


def _sdpa_priority():
    """The model's SDPA backend order (models/gpt2.py); the backward runs
    under it."""
    from torch.nn.attention import SDPBackend, sdpa_kernel
    return sdpa_kernel([SDPBackend.EFFICIENT_ATTENTION,
                        SDPBackend.FLASH_ATTENTION, SDPBackend.MATH],
                       set_priority=True)


def _strides_ok(t: torch.Tensor) -> bool:
    sb, sh, st, sd = t.stride()
    return (sd == 1 and sb % 8 == 0 and sh % 8 == 0 and st % 8 == 0
            and min(sb, sh, st) >= 0 and t.data_ptr() % 16 == 0)


def can_use(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor) -> bool:
    """q, k, v: (B, H, T, D).  True for CUDA bf16, D == 64, equal head counts
    and lengths, a non-empty problem, and strides the kernel reads in place:
    unit stride inside a head, every other stride a multiple of 8 elements,
    16-byte aligned base."""
    if not (q.is_cuda and k.is_cuda and v.is_cuda):
        return False
    if not (q.dtype == k.dtype == v.dtype == torch.bfloat16):
        return False
    if q.dim() != 4 or q.shape != k.shape or q.shape != v.shape:
        return False
    if q.shape[-1] != HEAD_DIM or q.numel() == 0:
        return False
    return _strides_ok(q) and _strides_ok(k) and _strides_ok(v)


def attn_forward(q, k, v, scale=None, out=None, lse=None):
    """Launch the kernel on the current stream.  Returns (out, lse): out
    (B, T, H, 64) bf16 contiguous, lse (B, H, T) fp32.  ``out``/``lse`` may be
    passed in (tests put guard regions around them)."""
    if not can_use(q, k, v):
        raise ValueError("fused_attn: inputs the kernel does not take "
                         "(see can_use)")
    B, H, T, D = q.shape
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    if out is None:
        out = torch.empty((B, T, H, D), dtype=q.dtype, device=q.device)
    if lse is None:
        lse = torch.empty((B, H, T), dtype=torch.float32, device=q.device)
    if (out.shape != (B, T, H, D) or not out.is_contiguous()
            or out.dtype != torch.bfloat16):
        raise ValueError("fused_attn: out must be contiguous (B, T, H, 64) bf16")
    if (lse.shape != (B, H, T) or not lse.is_contiguous()
            or lse.dtype != torch.float32):
        raise ValueError("fused_attn: lse must be contiguous (B, H, T) fp32")

    def bth(t):  # (batch, token, head) element strides of a (B, H, T, D) view
        sb, sh, st, _ = t.stride()
        return [sb, st, sh]

    s = torch.cuda.current_stream(q.device).cuda_stream
    _core.attn_fwd_causal_hd64(q.data_ptr(), k.data_ptr(), v.data_ptr(),
                               out.data_ptr(), lse.data_ptr(), B, H, T,
                               bth(q), bth(k), bth(v), T, float(scale), s)
    return out, lse


# dropout is 0, so the backward never reads the philox state; the aten
# forward returns two uninitialised int64 scalars on the CPU for it, and so
# do we
_philox = None


def _philox_state():
    global _philox
    if _philox is None:
        _philox = (torch.empty((), dtype=torch.int64),
                   torch.empty((), dtype=torch.int64))
    return _philox


class _FusedCausalAttn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, scale):
        out, lse = attn_forward(q, k, v, scale)
        out = out.transpose(1, 2)  # (B, H, T, D) view, as aten returns it
        ctx.save_for_backward(q, k, v, out, lse)
        ctx.scale = scale
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse = ctx.saved_tensors
        seed, offset = _philox_state()
        with _sdpa_priority():
            dq, dk, dv, _ = \
                torch.ops.aten._scaled_dot_product_efficient_attention_backward(
                    dout, q, k, v, None, out, lse, seed, offset, 0.0,
                    [True, True, True, False], True, scale=ctx.scale)
        return dq, dk, dv, None


def fused_causal_attention(q, k, v, scale=None):
    """softmax(scale * q k^T + causal mask) v for (B, H, T, 64) bf16 views;
    returns (B, H, T, 64) over a contiguous (B, T, H, 64) buffer."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    return _FusedCausalAttn.apply(q, k, v, float(scale))
