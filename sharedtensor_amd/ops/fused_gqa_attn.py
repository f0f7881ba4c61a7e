"""Causal bf16 grouped-query attention for head dim 64 with hand-written
forward (csrc/gqa_attn_kernels.hip) and backward
(csrc/gqa_attn_bwd_kernels.hip) kernels, and for head dim 128 with a
hand-written forward (csrc/gqa_attn_hd128_kernels.hip) and backward
(csrc/gqa_attn_hd128_bwd_kernels.hip): Hq = G * Hkv query heads, G in
{2, 4, 8}, query head h reads kv head h // G (the ``enable_gqa`` /
``repeat_interleave`` convention).

``fused_causal_gqa_attention(q, k, v)`` takes q as a (B, Hq, T, 64) view and
k, v as (B, Hkv, T, 64) views and reads them in place through their strides;
K and V are never expanded.  The forward writes ``out`` as contiguous
(B, T, Hq, 64), returned as its (B, Hq, T, 64) view, and ``lse`` (B, Hq, T)
fp32.  The backward is ``gqa_backward``: two HIP kernels, dk and dv summed
over the group in fp32 and rounded once, no atomics, bit-identical across
repeats.

At head dim 128 the same call runs our forward.  Its backward is by default
the aten efficient-attention backward on q and on K and V expanded over the
group, fed our ``out`` and ``lse`` (as ``fused_attn._FusedCausalAttn`` does
for MHA), dk and dv summed over the group; with ``own_backward_hd128=True``
it is ``gqa_backward_hd128``, which keeps the head dim 64 contract.
``can_use_backward`` and ``gqa_backward`` are head dim 64 only,
``can_use_backward_hd128`` and ``gqa_backward_hd128`` head dim 128 only.

With ``doc_ids`` (a (B, T) integer tensor whose equal values form contiguous
runs, one run per document of a packed batch row) query i sees key j only if
j <= i and both lie in the same document.  The mask is two int32 (B, T)
arrays from ``doc_start_end``, never a T x T object, and the kernels
(csrc/gqa_attn_doc_kernels.hip, csrc/gqa_attn_doc_bwd_kernels.hip) skip the
tiles outside a row's document.  Head dim 64 only; at head dim 128 the call
raises.  ``doc_ids=None`` is the plain causal path, untouched.

``can_use`` says whether the kernels take the inputs; G = 1 is not theirs
(ops/fused_attn.py has it).  A call outside ``can_use`` raises ``ValueError``;
there is never a silent fall-back.
"""
from __future__ import annotations

import math

import torch

from .. import _core
from .fused_attn import (HEAD_DIM, _bth, _philox_state, _sdpa_priority,
                         _strides_ok)

GROUPS = (2, 4, 8)
HEAD_DIMS = (HEAD_DIM, 128)  # forward and backward; one backward entry each


def doc_start_end(doc_ids: torch.Tensor):
    """(doc_start, doc_end) of a packed batch: int32 (B, T), the first
    position and one past the last position of the document that holds t,
    both non-decreasing in t.  ``doc_ids`` is a (B, T) integer tensor whose
    equal values form contiguous runs; anything else raises ``ValueError``
    (the check reads one flag back from the device)."""
    if not (torch.is_tensor(doc_ids) and doc_ids.dim() == 2
            and doc_ids.numel() > 0 and not doc_ids.dtype.is_floating_point
            and not doc_ids.dtype.is_complex
            and doc_ids.dtype != torch.bool):
        raise ValueError("fused_gqa_attn: doc_ids must be a non-empty (B, T) "
                         "integer tensor")
    B, T = doc_ids.shape
    pos = torch.arange(T, dtype=torch.int32, device=doc_ids.device)
    first = torch.ones((B, T), dtype=torch.bool, device=doc_ids.device)
    first[:, 1:] = doc_ids[:, 1:] != doc_ids[:, :-1]
    # as many runs as distinct values, or a value comes back after a gap
    ids = doc_ids.sort(dim=1).values
    distinct = 1 + (ids[:, 1:] != ids[:, :-1]).sum(1)
    if not bool((first.sum(1) == distinct).all()):
        raise ValueError("fused_gqa_attn: equal doc_ids must form contiguous "
                         "runs")
    start = torch.where(first, pos, 0).cummax(dim=1).values
    last = first.roll(-1, dims=1)  # column 0 is True: T - 1 ends a document
    end = torch.where(last, pos + 1, T).flip(1).cummin(dim=1).values.flip(1)
    return start.int().contiguous(), end.int().contiguous()


def _doc_ok(t, B, T, device) -> bool:
    return (torch.is_tensor(t) and t.dtype == torch.int32
            and t.shape == (B, T) and t.is_contiguous() and t.device == device)


def can_use(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
            doc_start=None, doc_end=None) -> bool:
    """q: (B, Hq, T, D); k, v: (B, Hkv, T, D), D 64 or 128.  True for CUDA
    bf16, Hq a multiple of Hkv by 2, 4 or 8, equal batch and length, a
    non-empty problem, and the stride rules of ``fused_attn.can_use``.  With
    ``doc_start`` (and, for the backward, ``doc_end``) also: D = 64 and
    contiguous int32 (B, T) arrays on q's device."""
    if doc_start is not None or doc_end is not None:
        if not can_use(q, k, v) or q.shape[-1] != HEAD_DIM:
            return False
        B, _, T, _ = q.shape
        return (_doc_ok(doc_start, B, T, q.device)
                and (doc_end is None or _doc_ok(doc_end, B, T, q.device)))
    if not (q.is_cuda and k.is_cuda and v.is_cuda):
        return False
    if not (q.dtype == k.dtype == v.dtype == torch.bfloat16):
        return False
    if q.dim() != 4 or k.dim() != 4 or k.shape != v.shape:
        return False
    B, Hq, T, D = q.shape
    if D not in HEAD_DIMS or q.numel() == 0 or k.numel() == 0:
        return False
    if k.shape[0] != B or k.shape[2] != T or k.shape[3] != D:
        return False
    Hkv = k.shape[1]
    if Hq % Hkv or Hq // Hkv not in GROUPS:
        return False
    return _strides_ok(q) and _strides_ok(k) and _strides_ok(v)


def gqa_forward(q, k, v, scale=None, out=None, lse=None, doc_start=None):
    """Launch the kernel on the current stream.  Returns (out, lse): out
    (B, T, Hq, D) bf16 contiguous, D 64 or 128, lse (B, Hq, T) fp32.
    ``out``/``lse`` may be passed in (tests put guard regions around them).
    With ``doc_start`` (of ``doc_start_end``) it is the document-masked
    kernel, head dim 64 only."""
    if not can_use(q, k, v, doc_start):
        raise ValueError("fused_gqa_attn: inputs the kernel does not take "
                         "(see can_use)")
    B, Hq, T, D = q.shape
    Hkv = k.shape[1]
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    if out is None:
        out = torch.empty((B, T, Hq, D), dtype=q.dtype, device=q.device)
    if lse is None:
        lse = torch.empty((B, Hq, T), dtype=torch.float32, device=q.device)
    if (out.shape != (B, T, Hq, D) or not out.is_contiguous()
            or out.dtype != torch.bfloat16 or out.device != q.device):
        raise ValueError("fused_gqa_attn: out must be contiguous "
                         "(B, T, Hq, 64 or 128) bf16")
    if (lse.shape != (B, Hq, T) or not lse.is_contiguous()
            or lse.dtype != torch.float32 or lse.device != q.device):
        raise ValueError("fused_gqa_attn: lse must be contiguous (B, Hq, T) "
                         "fp32")
    s = torch.cuda.current_stream(q.device).cuda_stream
    if doc_start is not None:
        _core.gqa_attn_fwd_doc_hd64(
            q.data_ptr(), k.data_ptr(), v.data_ptr(), doc_start.data_ptr(),
            out.data_ptr(), lse.data_ptr(), B, Hq, Hkv, T, _bth(q), _bth(k),
            _bth(v), T, float(scale), s)
        return out, lse
    launch = (_core.gqa_attn_fwd_causal_hd64 if D == HEAD_DIM
              else _core.gqa_attn_fwd_causal_hd128)
    launch(
        q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(),
        lse.data_ptr(), B, Hq, Hkv, T, _bth(q), _bth(k), _bth(v), T,
        float(scale), s)
    return out, lse


def _can_use_backward(q, k, v, out, lse, dout, D) -> bool:
    if not can_use(q, k, v) or q.shape[-1] != D:
        return False
    for t in (out, dout):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.bfloat16
                and t.shape == q.shape and _strides_ok(t)):
            return False
    return (torch.is_tensor(lse) and lse.is_cuda
            and lse.dtype == torch.float32
            and lse.shape == q.shape[:3] and lse.is_contiguous())


def can_use_backward(q, k, v, out, lse, dout) -> bool:
    """``can_use`` for the backward: q, k, v as there; out and dout bf16
    (B, Hq, T, 64) views under the same stride rules; lse contiguous
    (B, Hq, T) fp32.  Head dim 64 only."""
    return _can_use_backward(q, k, v, out, lse, dout, HEAD_DIM)


def can_use_backward_hd128(q, k, v, out, lse, dout) -> bool:
    """``can_use_backward`` for head dim 128, and for that alone."""
    return _can_use_backward(q, k, v, out, lse, dout, 128)


def _backward(D, launch, q, k, v, out, lse, dout, scale, dq, dk, dv, delta,
              doc=()):
    if (torch.is_tensor(dout) and torch.is_tensor(q) and dout.is_cuda
            and q.dim() == 4 and dout.dtype == torch.bfloat16
            and dout.shape == q.shape and not _strides_ok(dout)):
        dout = dout.contiguous()
    if not _can_use_backward(q, k, v, out, lse, dout, D) \
            or (doc and (doc[1] is None or not can_use(q, k, v, *doc))):
        raise ValueError("fused_gqa_attn: inputs the backward kernels do not "
                         "take (see can_use_backward"
                         + ("" if D == HEAD_DIM else "_hd128") + ")")
    B, Hq, T, _ = q.shape
    Hkv = k.shape[1]
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    grads = []
    for g, like in ((dq, q), (dk, k), (dv, v)):
        if g is None:
            g = torch.empty((B, T, like.shape[1], D), dtype=q.dtype,
                            device=q.device).transpose(1, 2)
        if (g.shape != like.shape or g.dtype != torch.bfloat16
                or g.device != q.device or not _strides_ok(g)
                or min(g.stride()[:3]) < D):
            raise ValueError("fused_gqa_attn: dq, dk, dv must be bf16 "
                             f"(B, H, T, {D}) views the kernel can write")
        grads.append(g)
    if delta is None:
        delta = torch.empty((B, Hq, T), dtype=torch.float32, device=q.device)
    if (delta.shape != (B, Hq, T) or not delta.is_contiguous()
            or delta.dtype != torch.float32 or delta.device != q.device):
        raise ValueError("fused_gqa_attn: delta must be contiguous "
                         "(B, Hq, T) fp32")
    dq, dk, dv = grads
    s = torch.cuda.current_stream(q.device).cuda_stream
    launch(
        q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(),
        dout.data_ptr(), lse.data_ptr(), *(t.data_ptr() for t in doc),
        dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), delta.data_ptr(),
        B, Hq, Hkv, T, _bth(q), _bth(k),
        _bth(v), _bth(out), _bth(dout), _bth(dq), _bth(dk), _bth(dv), T,
        float(scale), s)
    return dq, dk, dv


def gqa_backward(q, k, v, out, lse, dout, scale=None, dq=None, dk=None,
                 dv=None, delta=None, doc_start=None, doc_end=None):
    """dq (B, Hq, T, 64) and dk, dv (B, Hkv, T, 64) of ``gqa_forward`` on the
    current stream, as views of contiguous (B, T, H, 64) bf16 buffers.  A
    dout the kernel cannot read in place (a stride rule) is made contiguous
    once; anything else outside ``can_use_backward`` raises.  ``dq``/``dk``/
    ``dv`` (views to write into) and the fp32 (B, Hq, T) workspace ``delta``
    may be passed in (tests put guard regions around them).  With
    ``doc_start`` and ``doc_end`` (both or neither) it is the document-masked
    backward of ``gqa_forward(..., doc_start=doc_start)``."""
    if doc_start is not None or doc_end is not None:
        return _backward(HEAD_DIM, _core.gqa_attn_bwd_doc_hd64, q, k, v, out,
                         lse, dout, scale, dq, dk, dv, delta,
                         (doc_start, doc_end))
    return _backward(HEAD_DIM, _core.gqa_attn_bwd_causal_hd64, q, k, v, out,
                     lse, dout, scale, dq, dk, dv, delta)


def gqa_backward_hd128(q, k, v, out, lse, dout, scale=None, dq=None, dk=None,
                       dv=None, delta=None):
    """``gqa_backward`` for head dim 128 (csrc/gqa_attn_hd128_bwd_kernels.hip)
    under the same rules, with ``can_use_backward_hd128`` in the place of
    ``can_use_backward`` and (B, T, H, 128) buffers."""
    return _backward(128, _core.gqa_attn_bwd_causal_hd128, q, k, v, out, lse,
                     dout, scale, dq, dk, dv, delta)


class _FusedCausalGqaAttn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, scale):
        out, lse = gqa_forward(q, k, v, scale)
        out = out.transpose(1, 2)  # (B, Hq, T, D) view, as SDPA returns it
        ctx.save_for_backward(q, k, v, out, lse)
        ctx.scale = scale
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse = ctx.saved_tensors
        dq, dk, dv = gqa_backward(q, k, v, out, lse, dout, ctx.scale)
        return dq, dk, dv, None


class _FusedDocGqaAttn(torch.autograd.Function):
    """The document-masked kernels, head dim 64."""

    @staticmethod
    def forward(ctx, q, k, v, scale, doc_start, doc_end):
        if not can_use(q, k, v, doc_start, doc_end):
            raise ValueError("fused_gqa_attn: inputs the document-masked "
                             "kernels do not take (see can_use)")
        out, lse = gqa_forward(q, k, v, scale, doc_start=doc_start)
        out = out.transpose(1, 2)
        ctx.save_for_backward(q, k, v, out, lse, doc_start, doc_end)
        ctx.scale = scale
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse, doc_start, doc_end = ctx.saved_tensors
        dq, dk, dv = gqa_backward(q, k, v, out, lse, dout, ctx.scale,
                                  doc_start=doc_start, doc_end=doc_end)
        return dq, dk, dv, None, None, None


class _FusedCausalGqaAttnHd128(torch.autograd.Function):
    """Our forward; the aten efficient-attention backward on expanded K/V."""

    @staticmethod
    def forward(ctx, q, k, v, scale):
        out, lse = gqa_forward(q, k, v, scale)
        out = out.transpose(1, 2)  # (B, Hq, T, D) view, as aten returns it
        ctx.save_for_backward(q, k, v, out, lse)
        ctx.scale = scale
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse = ctx.saved_tensors
        Hkv = k.shape[1]
        G = q.shape[1] // Hkv
        ke, ve = (t.repeat_interleave(G, dim=1) for t in (k, v))
        seed, offset = _philox_state()
        with _sdpa_priority():
            dq, dk, dv, _ = \
                torch.ops.aten._scaled_dot_product_efficient_attention_backward(
                    dout, q, ke, ve, None, out, lse, seed, offset, 0.0,
                    [True, True, True, False], True, scale=ctx.scale)
        # bf16 per query head; the sum accumulates in fp32 and rounds once
        dk, dv = (t.unflatten(1, (Hkv, G)).sum(2) for t in (dk, dv))
        return dq, dk, dv, None


class _FusedCausalGqaAttnHd128Own(_FusedCausalGqaAttnHd128):
    """Our forward and our backward (``gqa_backward_hd128``)."""

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse = ctx.saved_tensors
        dq, dk, dv = gqa_backward_hd128(q, k, v, out, lse, dout, ctx.scale)
        return dq, dk, dv, None


def fused_causal_gqa_attention(q, k, v, scale=None, *,
                               own_backward_hd128=False, doc_ids=None,
                               doc_bounds=None):
    """softmax(scale * q k^T + causal mask) v with grouped kv heads, for bf16
    q (B, Hq, T, D) and k, v (B, Hkv, T, D) views, D 64 or 128; returns
    (B, Hq, T, D) over a contiguous (B, T, Hq, D) buffer.  The backward is
    ``gqa_backward`` at D = 64; at D = 128 it is the aten efficient-attention
    backward on expanded K/V, or ``gqa_backward_hd128`` with
    ``own_backward_hd128=True`` (which D = 64 ignores).  Inputs outside
    ``can_use`` raise.

    ``doc_ids`` (B, T), equal values in contiguous runs, adds the document
    mask of a packed batch: key j counts for query i only if both lie in one
    document.  D = 64 only.  A caller with many layers passes
    ``doc_bounds=doc_start_end(doc_ids)`` instead, built once."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    if doc_ids is not None or doc_bounds is not None:
        if doc_bounds is None:
            doc_bounds = doc_start_end(doc_ids)
        return _FusedDocGqaAttn.apply(q, k, v, float(scale), *doc_bounds)
    if torch.is_tensor(q) and q.dim() == 4 and q.shape[-1] == 128:
        fn = (_FusedCausalGqaAttnHd128Own if own_backward_hd128
              else _FusedCausalGqaAttnHd128)
        return fn.apply(q, k, v, float(scale))
    return _FusedCausalGqaAttn.apply(q, k, v, float(scale))
