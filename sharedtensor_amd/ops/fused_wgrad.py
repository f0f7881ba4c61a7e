"""Weight gradient of a bf16 Linear from a hand-written split-K kernel
(csrc/wgrad_kernels.hip): ``dW[N, K] = dY[M, N]^T X[M, K]`` with M the token
count, fp32 accumulation, bf16 out.

``linear_wgrad(x, weight, bias)`` is ``F.linear`` whose backward takes ``dW``
from that kernel.  The forward is the ``F.linear`` call itself, ``dX`` is the
aten matmul autograd runs today and the bias gradient is the same column sum,
so only the NT GEMM of the backward changes hands.

The kernel gives every workgroup one output tile and one of ``split``
contiguous ranges of 64-token steps; the partial tiles go through an fp32
workspace ``[split][N][K]`` and a second kernel adds them in split order.  No
atomics: two calls on the same inputs give the same bits.

``can_use`` says whether the kernel takes the operands; ``linear_wgrad``
computes the same thing in plain torch for everything else (CPU included).
A call that passes ``can_use`` and then fails is an error, never a silent
fall-back.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch
import torch.nn.functional as F

STEP = 64          # tokens per K-step of the kernel
NUM_CU = 256       # MI355X

# variant -> (tile_n, tile_k, workgroups per CU the split is sized for);
# csrc/wgrad_kernels.hip
#   0: 128 x 128, 4 waves, two LDS stages (64 KB), 2 workgroups fit a CU
#   1: 128 x 128, 4 waves, one LDS stage (32 KB), 3 fit; sizing the split
#      for 2 measured faster than for 3 (profiles/r09/)
#   2: 256 x 128, 8 waves, two LDS stages (96 KB), 1 fits
VARIANTS = {0: (128, 128, 2), 1: (128, 128, 2), 2: (256, 128, 1)}
DEFAULT_VARIANT = 1

# (N, K) of a weight -> variant, for the shapes whose microbenchmark beat the
# tuned library GEMM (profiles/r09/); models/gpt2.py routes only these
TUNED: dict = {(768, 768): 1, (2304, 768): 1}


def split_ranges(steps: int, split: int) -> List[Tuple[int, int]]:
    """(first step, step count) of each split, as the kernel computes them:
    contiguous, in order, the first ``steps % split`` one step longer."""
    if steps < 0 or split < 1:
        raise ValueError("steps >= 0 and split >= 1")
    q, r = divmod(steps, split)
    return [(s * q + min(s, r), q + (1 if s < r else 0)) for s in range(split)]


def choose_split(tiles: int, steps: int, per_cu: int,
                 num_cu: int = NUM_CU) -> int:
    """The largest split with ``tiles * split`` workgroups still resident at
    once (``per_cu`` per CU), at most one split per step, at least 1."""
    if tiles < 1 or steps < 1:
        raise ValueError("tiles >= 1 and steps >= 1")
    return max(1, min(steps, (num_cu * per_cu) // tiles))


def _mat_ok(t: torch.Tensor) -> bool:
    return (t.dim() == 2 and t.stride(1) == 1 and t.stride(0) % 8 == 0
            and t.stride(0) >= t.shape[1] and t.data_ptr() % 16 == 0)


def can_use(dy: torch.Tensor, x: torch.Tensor,
            variant: int = DEFAULT_VARIANT) -> bool:
    """dy (M, N) and x (M, K): CUDA bf16, unit stride inside a row, row
    strides multiples of 8 elements, 16-byte aligned bases, M a positive
    multiple of 64, N and K multiples of the variant's tile."""
    if variant not in VARIANTS:
        return False
    if not (dy.is_cuda and x.is_cuda and dy.device == x.device):
        return False
    if not (dy.dtype == x.dtype == torch.bfloat16):
        return False
    if not (_mat_ok(dy) and _mat_ok(x)) or dy.shape[0] != x.shape[0]:
        return False
    tn, tk, _ = VARIANTS[variant]
    M, N, K = dy.shape[0], dy.shape[1], x.shape[1]
    return M > 0 and M % STEP == 0 and N > 0 and K > 0 \
        and N % tn == 0 and K % tk == 0


# fp32 partials, one buffer per (device, stream); every split of every tile
# is written before the reduce kernel reads it, so it is never zeroed
_workspace: dict = {}


def _workspace_for(device, n: int, stream: int) -> torch.Tensor:
    key = (device.index, stream)
    buf = _workspace.get(key)
    if buf is None or buf.numel() < n:
        buf = torch.empty(n, dtype=torch.float32, device=device)
        _workspace[key] = buf
    return buf


def wgrad(dy: torch.Tensor, x: torch.Tensor, out: Optional[torch.Tensor] = None,
          split: Optional[int] = None, variant: Optional[int] = None,
          ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Launch the kernels on the current stream; returns dW (N, K) bf16.
    ``out`` (rows may be strided), ``split`` and ``ws`` may be passed in
    (tests put guard regions around ``out`` and ``ws``)."""
    from .. import _core
    if variant is None:
        variant = TUNED.get((dy.shape[1], x.shape[1]), DEFAULT_VARIANT)
    if not can_use(dy, x, variant):
        raise ValueError("fused_wgrad: operands the kernel does not take "
                         "(see can_use)")
    M, N, K = dy.shape[0], dy.shape[1], x.shape[1]
    tn, tk, per_cu = VARIANTS[variant]
    if out is None:
        out = torch.empty((N, K), dtype=torch.bfloat16, device=dy.device)
    if (out.shape != (N, K) or out.dtype != torch.bfloat16
            or out.device != dy.device or not _mat_ok(out)):
        raise ValueError("fused_wgrad: out must be (N, K) bf16 with unit "
                         "column stride and an aligned row stride")
    if split is None:
        split = choose_split((N // tn) * (K // tk), M // STEP, per_cu)
    s = torch.cuda.current_stream(dy.device).cuda_stream
    need = split * N * K if split > 1 else 0
    if need and ws is None:
        ws = _workspace_for(dy.device, need, s)
    if need and (ws.dtype != torch.float32 or not ws.is_contiguous()
                 or ws.numel() < need or ws.device != dy.device):
        raise ValueError("fused_wgrad: ws must be contiguous fp32 with at "
                         "least split * N * K elements")
    _core.wgrad_bf16(dy.data_ptr(), x.data_ptr(), out.data_ptr(),
                     ws.data_ptr() if need else 0, ws.numel() if need else 0,
                     M, N, K, dy.stride(0), x.stride(0), out.stride(0),
                     split, variant, s)
    return out


def _rows(t: torch.Tensor) -> torch.Tensor:
    """(..., C) -> (M, C) with unit column stride, a view where possible."""
    t = t.reshape(-1, t.shape[-1])
    return t if t.stride(1) == 1 else t.contiguous()


class _LinearWgrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return F.linear(x, weight, bias)

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dy2, x2 = _rows(dy), _rows(x)
        dx = dw = db = None
        # the gradients keep the dtypes of the forward operands, also when
        # backward() is called inside an autocast region
        with torch.autocast(device_type=dy.device.type, enabled=False):
            if ctx.needs_input_grad[0]:
                dx = dy2.to(weight.dtype).mm(weight).to(x.dtype).view(x.shape)
            if ctx.needs_input_grad[1]:
                variant = TUNED.get(tuple(weight.shape), DEFAULT_VARIANT)
                if weight.dtype == torch.bfloat16 and can_use(dy2, x2, variant):
                    dw = wgrad(dy2, x2, variant=variant)
                else:
                    dw = dy2.t().to(weight.dtype).mm(x2.to(weight.dtype))
            if ctx.has_bias and ctx.needs_input_grad[2]:
                db = dy2.sum(0)
        return dx, dw, db


def linear_wgrad(x: torch.Tensor, weight: torch.Tensor,
                 bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``F.linear(x, weight, bias)``; in the backward ``weight.grad`` comes
    from the split-K kernel where ``can_use`` holds and from torch's matmul
    everywhere else."""
    return _LinearWgrad.apply(x, weight, bias)


def wired(x: torch.Tensor, weight: torch.Tensor) -> bool:
    """Whether models/gpt2.py routes this Linear through ``linear_wgrad``:
    CUDA bf16 activations and weight, gradients on, a weight shape in
    ``TUNED`` and a token count the kernel takes."""
    if not (x.is_cuda and x.dtype == torch.bfloat16
            and weight.dtype == torch.bfloat16 and weight.dim() == 2
            and torch.is_grad_enabled() and weight.requires_grad):
        return False
    variant = TUNED.get(tuple(weight.shape))
    if variant is None or x.dim() < 2 or x.shape[-1] != weight.shape[1]:
        return False
    M = x.numel() // x.shape[-1]
    return M > 0 and M % STEP == 0 and x.shape[-1] % 8 == 0
