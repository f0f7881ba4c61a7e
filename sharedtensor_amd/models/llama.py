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

    def forward(self, x, cos, sin):
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
        if x.is_cuda:
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

    def forward(self, x, cos, sin, delta=None):
        """Takes the residual stream and the previous block's MLP output not
        yet added to it; returns the same pair, so every residual add
        happens inside the RMSNorm that follows it.  With ``delta=None``
        this is ``x = x + attn(attn_norm(x))`` and the caller owes
        ``x + m`` for the MLP."""
        x, h = add_rms(self.attn_norm, x, delta)
        x, h = add_rms(self.mlp_norm, x, self.attn(h, cos, sin))
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

    def forward(self, idx, targets=None):
        x = self.tok(idx)
        cos, sin = self._rope_cache(idx.device, x.dtype)
        delta = None
        for blk in self.blocks:
            x, delta = blk(x, cos, sin, delta)
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
