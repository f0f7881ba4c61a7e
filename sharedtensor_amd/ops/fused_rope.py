"""Fused bf16 RoPE for the Llama q/k pair (csrc/rope_kernels.hip): one
launch rotates q and k forward, one launch with the negated angle rotates
both gradients backward.  Eager `apply_rope` is ~10 kernels per tensor with
fp32 intermediates saved for backward; this saves only the cos/sin tables.

Forward reads q/k through their strides (the (B,T,H,D) storage the
projections wrote) and returns (B,H,T,D)-contiguous tensors, bit-identical
to `apply_rope`.  Backward writes (B,T,H,D)-contiguous storage and returns
its transpose(1,2) view, so the view/linear backward needs no copy."""
from __future__ import annotations

import os

import torch

from .. import _core


def _bht(x):
    return (x.stride(0), x.stride(1), x.stride(2))


def _launch(q, k, q_out, k_out, cos, sin, inverse):
    """q/k: (B,H,T,D) bf16 with D contiguous (k may be None); outputs are
    views of the same logical shape."""
    B, Hq, T, D = q.shape
    s = torch.cuda.current_stream(q.device).cuda_stream
    if k is None:
        _core.rope_qk(q.data_ptr(), 0, q_out.data_ptr(), 0, cos.data_ptr(),
                      sin.data_ptr(), B, Hq, 0, T, D, _bht(q), (0, 0, 0),
                      _bht(q_out), (0, 0, 0), inverse, s)
    else:
        _core.rope_qk(q.data_ptr(), k.data_ptr(), q_out.data_ptr(),
                      k_out.data_ptr(), cos.data_ptr(), sin.data_ptr(), B,
                      Hq, k.shape[1], T, D, _bht(q), _bht(k), _bht(q_out),
                      _bht(k_out), inverse, s)


def _d_contig(x):
    return x if x.stride(-1) == 1 else x.contiguous()


def _validate(q, k, cos, sin):
    """The kernel trusts its shapes; refuse anything it would misread."""
    for name, x in (("q", q), ("k", k)):
        if x is None and name == "k":
            continue
        if not (x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 4):
            raise ValueError(f"fused_rope_qk: {name} must be a 4-d bf16 "
                             "GPU tensor")
    B, _, T, D = q.shape
    if D == 0 or D % 2:
        raise ValueError("fused_rope_qk: head dim must be even and positive")
    if k is not None and (k.shape[0], k.shape[2], k.shape[3]) != (B, T, D):
        raise ValueError("fused_rope_qk: q and k must share B, T and D")
    for name, x in (("cos", cos), ("sin", sin)):
        if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2
                and x.is_contiguous() and x.shape[0] >= T
                and x.shape[1] == D // 2):
            raise ValueError(f"fused_rope_qk: {name} must be a contiguous "
                             "fp32 GPU table of shape (>=T, D/2)")


class _FusedRopeQKFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, cos, sin):
        _validate(q, k, cos, sin)
        T = q.shape[2]
        cos, sin = cos[:T], sin[:T]
        q = _d_contig(q)
        q_out = torch.empty(q.shape, dtype=q.dtype, device=q.device)
        k_out = None
        if k is not None:
            k = _d_contig(k)
            k_out = torch.empty(k.shape, dtype=k.dtype, device=k.device)
        _launch(q, k, q_out, k_out, cos, sin, False)
        # the rotation's gradient needs no activation: tables only
        ctx.save_for_backward(cos, sin)
        ctx.set_materialize_grads(False)
        return q_out, k_out

    @staticmethod
    def backward(ctx, dq, dk):
        cos, sin = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            dq = None
        if not ctx.needs_input_grad[1]:
            dk = None
        grads = [_d_contig(g) for g in (dq, dk) if g is not None]
        if not grads:
            return None, None, None, None
        # (B,T,H,D)-contiguous storage, handed back as the (B,H,T,D) view
        outs = [torch.empty((g.shape[0], g.shape[2], g.shape[1], g.shape[3]),
                            dtype=g.dtype, device=g.device).transpose(1, 2)
                for g in grads]
        if len(grads) == 2:
            _launch(grads[0], grads[1], outs[0], outs[1], cos, sin, True)
        else:
            _launch(grads[0], None, outs[0], None, cos, sin, True)
        it = iter(outs)
        return (next(it) if dq is not None else None,
                next(it) if dk is not None else None, None, None)


def fused_rope_qk(q, k, cos, sin):
    """Rotate q (B,Hq,T,D) and k (B,Hkv,T,D) with the fp32 (>=T, D/2)
    cos/sin tables; returns (q_rot, k_rot), each (B,H,T,D)-contiguous."""
    return _FusedRopeQKFn.apply(q, k, cos, sin)


def can_use(q, k, cos, sin) -> bool:
    if os.environ.get("SHTENS_NO_FUSED_ROPE") == "1":  # A/B knob
        return False
    if not (q.is_cuda and k.is_cuda and cos.is_cuda and sin.is_cuda):
        return False
    if q.dtype != torch.bfloat16 or k.dtype != torch.bfloat16:
        return False
    if cos.dtype != torch.float32 or sin.dtype != torch.float32:
        return False
    if q.dim() != 4 or k.dim() != 4 or cos.dim() != 2 or sin.dim() != 2:
        return False
    B, _, T, D = q.shape
    if (k.shape[0], k.shape[2], k.shape[3]) != (B, T, D):
        return False
    if D % 2 or D == 0 or q.stride(-1) != 1 or k.stride(-1) != 1:
        return False
    return (cos.is_contiguous() and sin.is_contiguous()
            and cos.shape == sin.shape and cos.shape[0] >= T
            and cos.shape[1] == D // 2)
