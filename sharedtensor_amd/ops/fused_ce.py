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

Options: ignore_index, label_smoothing and z_loss, the same kernels with
another row policy (csrc/ce_kernels.hip).  With all three at their defaults
the call is the path above, unchanged.  Otherwise a one-block scan of the
targets counts the valid rows on the device and the kernels read 1/n_valid
from device memory, so neither forward nor backward syncs with the host.  A row whose target equals ignore_index is
never read: it adds 0 to the loss and its dlogits row is exactly +0 (torch
gives NaN gradients when such a row holds NaN; here they are zero).  A row
whose target is out of range and is not ignore_index gets a zero dlogits row
too, but makes the loss NaN.  cross_entropy_reference states the semantics in
plain torch.
"""
from __future__ import annotations

import math
import os
from typing import Optional

import torch

from .. import _core


def _onepass_enabled() -> bool:
    return os.environ.get("SHTENS_CE_ONEPASS", "1") != "0"


class _FusedCEFn(torch.autograd.Function):
    """opts is None for the default call (plain kernels, 1/R, no scan and no
    state tensor), else the option kernels' keyword arguments."""

    @staticmethod
    def forward(ctx, logits, targets, opts):
        logits = logits.contiguous()
        R, V = logits.shape
        dev = logits.device
        t32 = targets.to(torch.int32).contiguous()
        loss = torch.empty(R, dtype=torch.float32, device=dev)
        row_lse = torch.empty(R, dtype=torch.float32, device=dev)
        s = torch.cuda.current_stream(dev).cuda_stream
        ptrs = (logits.data_ptr(), t32.data_ptr(), loss.data_ptr())
        ctx.opts = opts
        if opts is None:
            saved = ()
        else:
            # f32 inv_count | u32 n_valid | u32 n_bad | pad
            state = torch.empty(_core.CE_OPT_STATE_BYTES // 4,
                                dtype=torch.float32, device=dev)
            _core.ce_opts_scan(t32.data_ptr(), R, V, opts["ignore_index"],
                               opts["has_ignore"], state.data_ptr(), s)
            saved = (state,)
        ctx.onepass = (ctx.needs_input_grad[0] and _onepass_enabled()
                       and V <= _core.ce_fwd_grad_max_v())
        if ctx.onepass:
            # same peak memory as allocating it in backward: both points
            # are the activation peak
            dlogits = torch.empty_like(logits)
            saved += (dlogits,)
            if opts is None:
                _core.ce_fwd_grad(*ptrs, row_lse.data_ptr(),
                                  dlogits.data_ptr(), 1.0 / R, R, V, s)
            else:
                _core.ce_opts_fwd_grad(*ptrs, row_lse.data_ptr(),
                                       dlogits.data_ptr(), state.data_ptr(),
                                       R, V, stream=s, **opts)
        elif opts is None:
            row_m = torch.empty(R, dtype=torch.float32, device=dev)
            _core.ce_fwd(*ptrs, row_m.data_ptr(), row_lse.data_ptr(), R, V, s)
        else:
            _core.ce_opts_fwd(*ptrs, row_lse.data_ptr(), R, V, stream=s,
                              **opts)
        ctx.save_for_backward(logits, t32, row_lse, *saved)
        if opts is None:
            return loss.mean()
        # mean over the valid rows; inv_count stays on the device
        return loss.sum() * state[0]

    @staticmethod
    def backward(ctx, dloss):
        logits, t32, row_lse, *saved = ctx.saved_tensors
        R, V = logits.shape
        g = dloss.to(device=logits.device, dtype=torch.float32).contiguous()
        s = torch.cuda.current_stream(logits.device).cuda_stream
        # the precomputed buffer serves the first backward only: after that
        # it may be somebody's .grad (retain_graph=True)
        first = ctx.onepass
        ctx.onepass = False
        dlogits = saved[-1] if first else torch.empty_like(logits)
        ptrs = (logits.data_ptr(), t32.data_ptr(), row_lse.data_ptr(),
                dlogits.data_ptr(), g.data_ptr())
        if ctx.opts is None:
            _core.ce_bwd(*ptrs, 1.0 / R, R, V, s, skip_if_unit=first)
        else:
            _core.ce_opts_bwd(*ptrs, saved[0].data_ptr(), R, V, stream=s,
                              skip_if_unit=first, **ctx.opts)
        return dlogits, None, None


def _check_options(ignore_index, label_smoothing, z_loss):
    if ignore_index is not None:
        if isinstance(ignore_index, bool) or not isinstance(ignore_index, int):
            raise TypeError("ignore_index must be an int or None")
        if not -2 ** 31 <= ignore_index < 2 ** 31:
            raise ValueError("ignore_index must fit in 32 bits")
    label_smoothing = float(label_smoothing)
    z_loss = float(z_loss)
    if not (math.isfinite(label_smoothing) and 0.0 <= label_smoothing < 1.0):
        raise ValueError(
            f"label_smoothing must be in [0, 1), got {label_smoothing}")
    if not (math.isfinite(z_loss) and z_loss >= 0.0):
        raise ValueError(f"z_loss must be finite and >= 0, got {z_loss}")
    return label_smoothing, z_loss


def fused_cross_entropy(logits: torch.Tensor, targets: torch.Tensor, *,
                        ignore_index: Optional[int] = None,
                        label_smoothing: float = 0.0,
                        z_loss: float = 0.0) -> torch.Tensor:
    """Mean cross-entropy over the valid rows; logits (R, V) bf16 cuda,
    targets (R,).  Options and their edge cases: module docstring."""
    label_smoothing, z_loss = _check_options(ignore_index, label_smoothing,
                                             z_loss)
    opts = None
    if ignore_index is not None or label_smoothing != 0.0 or z_loss != 0.0:
        has_ignore = ignore_index is not None
        opts = dict(ignore_index=ignore_index if has_ignore else 0,
                    has_ignore=has_ignore, label_smoothing=label_smoothing,
                    z_loss=z_loss)
    return _FusedCEFn.apply(logits, targets, opts)


def cross_entropy_reference(logits_fp32: torch.Tensor, targets: torch.Tensor,
                            ignore_index: Optional[int] = None,
                            label_smoothing: float = 0.0,
                            z_loss: float = 0.0) -> torch.Tensor:
    """The semantics of fused_cross_entropy in plain torch, on any device.

    Row r is valid when targets[r] != ignore_index and 0 <= targets[r] < V.
    loss = sum over valid rows of
        (1-eps)*(lse - x_t) + eps*(lse - mean_j x_j) + z*lse**2
    divided by the number of valid rows (NaN when there is none).  Rows that
    are not valid do not reach the result, whatever they hold, and get a zero
    gradient; a row whose target is out of range and not ignore_index makes
    the loss NaN.  For z = 0 and targets in range this is
    F.cross_entropy(x, t, ignore_index=..., label_smoothing=eps).
    """
    label_smoothing, z_loss = _check_options(ignore_index, label_smoothing,
                                             z_loss)
    x = logits_fp32.float()
    V = x.shape[-1]
    x = x.reshape(-1, V)
    t = targets.reshape(-1).to(torch.int64)
    in_range = (t >= 0) & (t < V)
    ignored = (t == ignore_index) if ignore_index is not None \
        else torch.zeros_like(in_range)
    valid = in_range & ~ignored
    bad = ~in_range & ~ignored
    x = torch.where(valid[:, None], x, torch.zeros((), dtype=x.dtype,
                                                   device=x.device))
    lse = torch.logsumexp(x, dim=-1)
    xt = x.gather(1, t.clamp(0, V - 1)[:, None]).squeeze(1)
    per_row = (1.0 - label_smoothing) * (lse - xt) \
        + label_smoothing * (lse - x.mean(dim=-1)) + z_loss * lse * lse
    per_row = torch.where(valid, per_row, torch.zeros_like(per_row))
    per_row = torch.where(bad, torch.full_like(per_row, float("nan")), per_row)
    return per_row.sum() / valid.sum()


def can_use(logits: torch.Tensor) -> bool:
    return (logits.is_cuda and logits.dtype == torch.bfloat16
            and logits.dim() == 2)
