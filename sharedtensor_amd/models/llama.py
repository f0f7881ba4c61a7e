"""Llama-3-family models (RMSNorm, RoPE, GQA, SwiGLU).

BASELINE.json config 4 shares a Llama-3-8B's parameters as a
table-of-tensors (`SharedTable`, one scale per tensor) across 8 MI355X.
Llama-3-8B in fp32 is ~32 GB of parameters; replica + up to 3 link residual
deltas = <=128 GB, comfortably inside 288 GB of HBM3E per GPU.
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

# Run grouped-query attention in our own kernels (ops/fused_gqa_attn.py: bf16,
# head dim 64, causal, 2, 4 or 8 query heads per kv head), forward and
# backward, instead of SDPA with enable_gqa.  Measured at B=64, Hq=32, Hkv=8,
# T=1024: forward 0.686 ms against 1.140 ms, backward 1.655 ms against
# 4.788 ms for the SDPA call, and 507.6 / 508.3 / 508.5 ms per
# `bench.py --model llama1b` step against 577.3 / 578.0 / 578.8 for the
# parent, so it is on.  Numbers in profiles/r12/.
# SHTENS_FUSED_GQA_ATTN = 0 or 1 overrides the flag for an A/B run; inputs the
# kernels do not take keep the SDPA path.
FUSE_GQA_ATTN = True

# The same at head dim 128 (Llama-3-8B): our forward
# (csrc/gqa_attn_hd128_kernels.hip), the aten efficient-attention backward on
# K/V expanded over the group.  The flag is on only if forward + backward of
# that path lies wholly below the SDPA enable_gqa call's range at both
# benchmark shapes (benchmarks/bench_model_kernels.py --only-gqa-attn-hd128).
# Measured at Hq=32, Hkv=8, range over 7 rounds: B=8, T=2048 forward +
# backward 2.425-2.444 ms against 4.732-4.747 ms for the SDPA call (forward
# alone 0.621 against 0.742 ms); B=2, T=8192 7.572-7.647 ms against
# 13.188-13.229 ms (forward alone 1.999 against 2.428 ms), so it is on.  Most
# of the gain is the backward: on expanded K/V aten picks a 1.39 ms kernel
# where the enable_gqa call runs 4.14 ms of dk/dv and dq kernels.
# `bench.py --model llama8b --batch 4 --seq 2048`, three steps: 402.2 ms per
# step with the flag on against 453.5 ms off.  Numbers in profiles/r13/.
# SHTENS_FUSED_GQA_ATTN_HD128 = 0 or 1 overrides it; it is consulted only when
# head dim is 128.
FUSE_GQA_ATTN_HD128 = True

# Behind that forward, our own head-dim-128 backward
# (csrc/gqa_attn_hd128_bwd_kernels.hip, ops.fused_gqa_attn.gqa_backward_hd128)
# instead of the aten backward on expanded K/V.  It is consulted only when
# head dim is 128 and FUSE_GQA_ATTN_HD128 took the call.  The flag is on only
# if the own backward's range lies wholly below the aten arm's (expansion and
# group sums included) at both benchmark shapes, Hq=32, Hkv=8, 7 rounds, arms
# alternating in one call (benchmarks/bench_model_kernels.py
# --only-gqa-attn-hd128, arms bwd_gqa128 and bwd_aten128), and the
# `bench.py --model llama8b --batch 4 --seq 2048` step is faster than the
# parent's.
# Measured, range over 7 rounds: B=8, T=2048 backward 1.443-1.455 ms against
# 1.741-1.747 ms for the aten arm; B=2, T=8192 4.180-4.309 ms against
# 5.272-5.297 ms: wholly below at both shapes.  The llama8b step at
# 4 x 2048 tokens, five steps per run, runs alternating: 403.4 and 404.2 ms
# with the own backward against 402.2 and 404.1 ms for the parent's path.
# That is 0.65 ms behind on the means and inside the spread, not lower, so
# the flag is off.  Numbers in profiles/r18/.
# SHTENS_FUSED_GQA_ATTN_HD128_BWD = 0 or 1 overrides it.
FUSE_GQA_ATTN_HD128_BWD = False

# Packed batches (`Llama.forward(idx, targets, doc_ids)`): attention masked
# across document boundaries in our own kernels
# (csrc/gqa_attn_doc_kernels.hip, csrc/gqa_attn_doc_bwd_kernels.hip: bf16,
# head dim 64, G in {2, 4, 8}), which skip the tiles outside a row's
# document, instead of SDPA with a dense (B, 1, T, T) boolean mask.  It is
# consulted only when doc_ids is given, head dim is 64 and FUSE_GQA_ATTN took
# the call.  The flag stays on only if the document arm's range over 7 rounds
# lies wholly below the dense-mask SDPA arm's at B=64, Hq=32, Hkv=8, T=1024,
# documents of mean length 256 (benchmarks/bench_model_kernels.py
# --only-gqa-attn-doc).  Measured there (4.4 documents per row): forward +
# backward 1.213-1.217 ms (0.381 + 0.833 ms medians) against 40.77-40.83 ms
# for the SDPA call, and against 0.715 + 1.558 ms for the plain causal
# kernels on the same shape, so it is on.  With one document per row the
# document kernels take 0.675 + 1.612 ms.  Numbers in profiles/r20/.
# SHTENS_FUSED_GQA_ATTN_DOC = 0 or 1 overrides it.
FUSE_GQA_ATTN_DOC = True


def _flag(env: str, default: bool) -> bool:
    v = os.environ.get(env)
    return default if v is None else v == "1"


def _gqa_ok(q, k, v) -> bool:
    if q.shape[-1] == 128:
        on = _flag("SHTENS_FUSED_GQA_ATTN_HD128", FUSE_GQA_ATTN_HD128)
    else:
        on = _flag("SHTENS_FUSED_GQA_ATTN", FUSE_GQA_ATTN)
    if not (on and q.is_cuda):
        return False
    from ..ops import fused_gqa_attn
    return fused_gqa_attn.can_use(q, k, v)


@dataclass
class LlamaConfig:
    vocab_size: int = 128256
    n_layer: int = 32
    n_head: int = 32
    n_kv_head: int = 8
    dim: int = 4096
    ffn_dim: int = 14336
    block_size: int = 8192
    rope_theta: float = 500000.0
    norm_eps: float = 1e-5
    # loss options (ops/fused_ce.py); the defaults are the plain mean
    ignore_index: Optional[int] = None
    label_smoothing: float = 0.0
    z_loss: float = 0.0

    @classmethod
    def llama3_8b(cls):
        return cls()

    @classmethod
    def llama_1b(cls):  # Llama-3.2-1B-ish, for single-GPU runs
        return cls(n_layer=16, n_head=32, n_kv_head=8, dim=2048,
                   ffn_dim=8192, block_size=4096)

    @classmethod
    def tiny(cls):  # for CPU tests
        return cls(vocab_size=256, n_layer=2, n_head=4, n_kv_head=2, dim=64,
                   ffn_dim=128, block_size=64)


class RMSNorm(nn.Module):
    def __init__(self, dim, eps):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(dim))
        self.eps = eps

    def forward(self, x):
        if x.is_cuda and x.dtype == torch.bfloat16 \
                and self.weight.dtype == torch.bfloat16:
            # fused CDNA4 kernel: no fp32 upcast traffic on the (B,T,C)
            # activation (csrc/ln_kernels.hip, fp32 statistics inside)
            from ..ops import fused_rms
            if fused_rms.can_use(x, self.weight):
                return fused_rms.fused_rms_norm(x, self.weight, self.eps)
        dt = x.dtype
        x = x.float()
        x = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + self.eps)
        return (x * self.weight.float()).to(dt)


def add_rms(norm: RMSNorm, x, delta):
    """``x = x + delta; h = norm(x)`` -> (x, h).

    On the fused path the add rides inside the RMSNorm kernels, forward and
    backward (ops/fused_rms.py).  Everywhere else — CPU, fp32, a width the
    kernels do not cover, or SHTENS_NO_FUSED_ADD_RMS=1 — it is the plain
    torch add followed by ``norm(x)``, value for value what
    ``x = x + f(norm(x))`` computes.  ``delta=None`` is the first norm of the
    model: nothing to add.
    """
    if delta is None:
        return x, norm(x)
    if x.is_cuda and x.dtype == torch.bfloat16 \
            and norm.weight.dtype == torch.bfloat16:
        from ..ops import fused_rms
        if fused_rms.can_use_add(x, norm.weight):
            return fused_rms.fused_add_rms_norm(x, delta, norm.weight,
                                                norm.eps)
    x = x + delta
    return x, norm(x)


def rope_freqs(head_dim, max_seq, theta, device):
    inv = 1.0 / (theta ** (torch.arange(0, head_dim, 2, device=device).float() / head_dim))
    t = torch.arange(max_seq, device=device).float()
    f = torch.outer(t, inv)
    return torch.cos(f), torch.sin(f)


def apply_rope(x, cos, sin):
    # x: (B, H, T, D); pairwise rotate [x0, x1] halves interleaved as (even, odd).
    # Rotation runs in fp32 (cos/sin cache dtype); the result returns to
    # x's dtype so q/k match v for SDPA outside autocast.
    T = x.shape[2]
    c, s = cos[:T], sin[:T]  # (T, D/2)
    x1, x2 = x[..., 0::2], x[..., 1::2]
    o1 = x1 * c - x2 * s
    o2 = x1 * s + x2 * c
    out = torch.stack((o1, o2), dim=-1).flatten(-2)
    return out.to(x.dtype)


class LlamaAttention(nn.Module):
    def __init__(self, cfg: LlamaConfig):
        super().__init__()
        self.head_dim = cfg.dim // cfg.n_head
        self.n_head, self.n_kv = cfg.n_head, cfg.n_kv_head
        self.wq = nn.Linear(cfg.dim, cfg.n_head * self.head_dim, bias=False)
        self.wk = nn.Linear(cfg.dim, cfg.n_kv_head * self.head_dim, bias=False)
        self.wv = nn.Linear(cfg.dim, cfg.n_kv_head * self.head_dim, bias=False)
        self.wo = nn.Linear(cfg.n_head * self.head_dim, cfg.dim, bias=False)

    def _doc_attention(self, q, k, v, doc_ids, doc_bounds):
        """Causal attention inside each document of a packed row: the
        document-masked kernels where they take the call, SDPA with the
        dense boolean mask everywhere else (CPU, fp32, head dim 128, a flag
        off)."""
        from ..ops import fused_gqa_attn
        if doc_bounds is None:
            doc_bounds = fused_gqa_attn.doc_start_end(doc_ids)
        if q.shape[-1] == 64 and _gqa_ok(q, k, v) \
                and _flag("SHTENS_FUSED_GQA_ATTN_DOC", FUSE_GQA_ATTN_DOC):
            return fused_gqa_attn.fused_causal_gqa_attention(
                q, k, v, doc_bounds=doc_bounds)
        pos = torch.arange(q.shape[2], device=q.device)
        mask = ((pos >= doc_bounds[0][:, :, None])
                & (pos <= pos[:, None])).unsqueeze(1)  # (B, 1, T, T)
        gqa = self.n_kv != self.n_head
        if not q.is_cuda:
            return F.scaled_dot_product_attention(q, k, v, attn_mask=mask,
                                                  enable_gqa=gqa)
        from torch.nn.attention import SDPBackend, sdpa_kernel
        with sdpa_kernel([SDPBackend.EFFICIENT_ATTENTION,
                          SDPBackend.FLASH_ATTENTION, SDPBackend.MATH],
                         set_priority=True):
            return F.scaled_dot_product_attention(q, k, v, attn_mask=mask,
                                                  enable_gqa=gqa)

    def forward(self, x, cos, sin, doc_ids=None, doc_bounds=None):
        """``doc_ids`` (B, T), or ``doc_bounds`` =
        ``fused_gqa_attn.doc_start_end(doc_ids)`` built once for all layers,
        masks attention across the documents of a packed row."""
        B, T, _ = x.shape
        q = self.wq(x).view(B, T, self.n_head, self.head_dim).transpose(1, 2)
        k = self.wk(x).view(B, T, self.n_kv, self.head_dim).transpose(1, 2)
        v = self.wv(x).view(B, T, self.n_kv, self.head_dim).transpose(1, 2)
        fused = False
        if q.is_cuda and q.dtype == torch.bfloat16:
            # one fused CDNA4 launch rotates q and k (csrc/rope_kernels.hip),
            # bit-identical to the two apply_rope chains it replaces
            from ..ops import fused_rope
            fused = fused_rope.can_use(q, k, cos, sin)
            if fused:
                q, k = fused_rope.fused_rope_qk(q, k, cos, sin)
        if not fused:
            q = apply_rope(q, cos, sin)
            k = apply_rope(k, cos, sin)
        if doc_ids is not None or doc_bounds is not None:
            y = self._doc_attention(q, k, v, doc_ids, doc_bounds)
        elif _gqa_ok(q, k, v):
            # q, k (rotated) and v (the (B, T, H, D).transpose(1, 2) view)
            # are read in place through their strides; K/V are not expanded
            from ..ops import fused_gqa_attn
            own = q.shape[-1] == 128 and _flag(
                "SHTENS_FUSED_GQA_ATTN_HD128_BWD", FUSE_GQA_ATTN_HD128_BWD)
            y = fused_gqa_attn.fused_causal_gqa_attention(
                q, k, v, own_backward_hd128=own)
        elif x.is_cuda:
            # same backend priority as GPT-2 (+16% measured; MATH fallback
            # covers shapes a backend rejects, e.g. GQA corner cases)
            from torch.nn.attention import SDPBackend, sdpa_kernel
            with sdpa_kernel([SDPBackend.EFFICIENT_ATTENTION,
                              SDPBackend.FLASH_ATTENTION, SDPBackend.MATH],
                             set_priority=True):
                y = F.scaled_dot_product_attention(
                    q, k, v, is_causal=True,
                    enable_gqa=self.n_kv != self.n_head)
        else:
            y = F.scaled_dot_product_attention(
                q, k, v, is_causal=True, enable_gqa=self.n_kv != self.n_head)
        y = y.transpose(1, 2).contiguous().view(B, T, -1)
        return self.wo(y)


class LlamaMLP(nn.Module):
    def __init__(self, cfg: LlamaConfig):
        super().__init__()
        self.w1 = nn.Linear(cfg.dim, cfg.ffn_dim, bias=False)  # gate
        self.w3 = nn.Linear(cfg.dim, cfg.ffn_dim, bias=False)  # up
        self.w2 = nn.Linear(cfg.ffn_dim, cfg.dim, bias=False)  # down

    def forward(self, x):
        x1 = self.w1(x)
        x3 = self.w3(x)
        if x1.is_cuda and x1.dtype == torch.bfloat16:
            # one fused CDNA4 kernel instead of separate silu + mul
            # (csrc/swiglu_kernels.hip)
            from ..ops import fused_swiglu
            if fused_swiglu.can_use(x1, x3):
                return self.w2(fused_swiglu.fused_swiglu(x1, x3))
        return self.w2(F.silu(x1) * x3)


class LlamaBlock(nn.Module):
    def __init__(self, cfg: LlamaConfig):
        super().__init__()
        self.attn_norm = RMSNorm(cfg.dim, cfg.norm_eps)
        self.attn = LlamaAttention(cfg)
        self.mlp_norm = RMSNorm(cfg.dim, cfg.norm_eps)
        self.mlp = LlamaMLP(cfg)

    def forward(self, x, cos, sin, delta=None, doc_bounds=None):
        """Takes the residual stream and the previous block's MLP output not
        yet added to it; returns the same pair, so every residual add
        happens inside the RMSNorm that follows it.  With ``delta=None``
        this is ``x = x + attn(attn_norm(x))`` and the caller owes
        ``x + m`` for the MLP.  ``doc_bounds``: see LlamaAttention."""
        x, h = add_rms(self.attn_norm, x, delta)
        a = self.attn(h, cos, sin) if doc_bounds is None \
            else self.attn(h, cos, sin, doc_bounds=doc_bounds)
        x, h = add_rms(self.mlp_norm, x, a)
        return x, self.mlp(h)


class Llama(nn.Module):
    def __init__(self, cfg: LlamaConfig):
        super().__init__()
        self.cfg = cfg
        self.tok = nn.Embedding(cfg.vocab_size, cfg.dim)
        self.blocks = nn.ModuleList(LlamaBlock(cfg) for _ in range(cfg.n_layer))
        self.norm = RMSNorm(cfg.dim, cfg.norm_eps)
        self.lm_head = nn.Linear(cfg.dim, cfg.vocab_size, bias=False)
        std = 0.02
        for name, p in self.named_parameters():
            if p.dim() >= 2:
                nn.init.normal_(p, std=std / (math.sqrt(2 * cfg.n_layer)
                                              if name.endswith(("wo.weight", "w2.weight")) else 1.0))
        self._rope = None

    def _rope_cache(self, device, dtype):
        if self._rope is None or self._rope[0].device != device:
            cos, sin = rope_freqs(self.cfg.dim // self.cfg.n_head,
                                  self.cfg.block_size, self.cfg.rope_theta,
                                  device)
            self._rope = (cos, sin)
        return self._rope

    def forward(self, idx, targets=None, doc_ids=None):
        """``doc_ids`` (B, T), equal values in contiguous runs: a packed
        batch, attention masked across its document boundaries.  RoPE
        positions stay the absolute positions of the row."""
        x = self.tok(idx)
        cos, sin = self._rope_cache(idx.device, x.dtype)
        delta = None
        bounds = None
        if doc_ids is not None:
            if doc_ids.shape != idx.shape:
                raise ValueError("doc_ids must have the shape of idx")
            from ..ops import fused_gqa_attn
            bounds = fused_gqa_attn.doc_start_end(doc_ids)  # once, all layers
        for blk in self.blocks:
            x, delta = blk(x, cos, sin, delta) if bounds is None \
                else blk(x, cos, sin, delta, doc_bounds=bounds)
        _, x = add_rms(self.norm, x, delta)  # absorbs the last add
        logits = self.lm_head(x)
        if targets is None:
            return logits, None
        flat = logits.view(-1, logits.size(-1))
        tgt = targets.reshape(-1)
        cfg = self.cfg
        if cfg.ignore_index is not None or cfg.label_smoothing != 0.0 \
                or cfg.z_loss != 0.0:
            return logits, self._loss_with_options(flat, tgt)
        if flat.is_cuda and flat.dtype == torch.bfloat16 \
                and os.environ.get("SHTENS_NO_FUSED_CE_LLAMA") != "1":
            # one read of the bf16 logits gives loss and dlogits
            # (csrc/ce_kernels.hip) instead of an fp32 copy of the logits
            # plus torch's fp32 log-softmax; the knob is for A/B runs
            from ..ops import fused_ce
            if fused_ce.can_use(flat):
                return logits, fused_ce.fused_cross_entropy(flat, tgt)
        loss = F.cross_entropy(flat.float(), tgt)
        return logits, loss

    def _loss_with_options(self, flat, tgt):
        # cuda/bf16: the fused kernels with the options; every other path
        # (CPU, fp32, the A/B knob) the same semantics in plain torch
        from ..ops import fused_ce
        opts = dict(ignore_index=self.cfg.ignore_index,
                    label_smoothing=self.cfg.label_smoothing,
                    z_loss=self.cfg.z_loss)
        if fused_ce.can_use(flat) \
                and os.environ.get("SHTENS_NO_FUSED_CE_LLAMA") != "1":
            return fused_ce.fused_cross_entropy(flat, tgt, **opts)
        return fused_ce.cross_entropy_reference(flat.float(), tgt, **opts)

    def num_params(self):
        return sum(p.numel() for p in self.parameters())
