"""GPT-2 model family — the flagship async-DP workload.

The reference repo names char-rnn as its intended training example
(/root/reference/README.md:37); BASELINE.json config 3 upgrades that to
GPT-2-small (char-rnn-style next-token loss) trained async-data-parallel with
all parameters as one shared tensor.  The model is plain PyTorch-ROCm: on
MI355X the matmuls run on MFMA via rocBLAS/hipBLASLt and attention via
torch SDPA; the shared-parameter machinery (this framework's contribution)
runs in our HIP kernels underneath it.
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
class GPT2Config:
    vocab_size: int = 50257
    n_layer: int = 12
    n_head: int = 12
    n_embd: int = 768
    block_size: int = 1024
    dropout: float = 0.0
    # loss options (ops/fused_ce.py); the defaults are the plain mean
    ignore_index: Optional[int] = None
    label_smoothing: float = 0.0
    z_loss: float = 0.0

    @classmethod
    def small(cls):  # 124M — the benchmark config
        return cls()

    @classmethod
    def tiny(cls):  # for CPU tests
        return cls(vocab_size=256, n_layer=2, n_head=2, n_embd=64,
                   block_size=64)


# Route the bias of the two residual-feeding `proj` Linears through the
# fused add+LayerNorm: the GEMM runs without bias, the add kernel adds it,
# and its gradient is a column sum the LayerNorm backward already holds.
# Measured +0.4% tokens/s on top of the add fusion, clear of run-to-run
# noise (profiles/r03/bench_ln_fusion_ab.json); False restores the GEMM
# epilogue bias.
FUSE_PROJ_BIAS = True

# Take qkv.bias.grad inside the pack of dq/dk/dv and fc.bias.grad inside GELU
# backward (ops/fused_bias_grad.py): the forward GEMMs keep their bias, only
# the route of its gradient changes.  The qkv half measured 0.124 ms against
# 0.283 ms for torch's cat + reduce and is on.  The GELU half measured
# 0.378 ms against 0.356 ms for GeluBackward + reduce (profiles/r07/), so it
# stays off: a tested alternative, like ops/fused_gelu.py.
# SHTENS_FUSED_QKV_BGRAD / SHTENS_FUSED_GELU_BGRAD = 0 or 1 override either
# flag for an A/B run.
FUSE_QKV_BIAS_GRAD = True
FUSE_FC_BIAS_GRAD = False

# Run the attention forward in our own kernel (ops/fused_attn.py: bf16, head
# dim 64, causal) instead of the SDPA efficient-attention forward; the
# backward stays the aten one, fed with our out and lse.  Numbers in
# profiles/r08/.  SHTENS_FUSED_ATTN = 0 or 1 overrides the flag for an A/B
# run; inputs the kernel does not take keep the SDPA path.
FUSE_ATTN_FWD = True

# Take the weight gradient of the four layer Linears (attn.qkv, attn.proj,
# mlp.fc, mlp.proj) from our split-K kernel (ops/fused_wgrad.py) instead of
# the library's NT GEMM; forward, dX and the bias gradients stay where they
# are.  Only the weight shapes in fused_wgrad.TUNED, the ones that won their
# measurement, take it: attn.proj 0.099 ms against 0.173 ms for the tuned
# library GEMM and attn.qkv 0.303 against 0.336.  mlp.fc (0.410 against
# 0.394) and mlp.proj (0.414 against 0.404) lost and keep aten, as does
# lm_head (large output, tied weight).  Numbers in profiles/r09/.
# SHTENS_FUSED_WGRAD = 0 or 1 overrides the flag for an A/B run.
FUSE_WGRAD = True


def _flag(env: str, default: bool) -> bool:
    v = os.environ.get(env)
    return default if v is None else v == "1"


def _linear(x, weight, bias=None):
    """``F.linear``, with ``weight.grad`` from the split-K kernel for the
    shapes it is wired for."""
    if _flag("SHTENS_FUSED_WGRAD", FUSE_WGRAD) and x.is_cuda:
        from ..ops import fused_wgrad
        if fused_wgrad.wired(x, weight):
            return fused_wgrad.linear_wgrad(x, weight, bias)
    return F.linear(x, weight, bias)


def _attn_ok(q, k, v) -> bool:
    if not (_flag("SHTENS_FUSED_ATTN", FUSE_ATTN_FWD) and q.is_cuda):
        return False
    from ..ops import fused_attn
    return fused_attn.can_use(q, k, v)


def _bias_grad_ok(flag: bool, which: str, x, lin: nn.Linear) -> bool:
    if not (flag and x.is_cuda and x.dtype == torch.bfloat16
            and lin.bias is not None and torch.is_grad_enabled()):
        return False
    from ..ops import fused_bias_grad as fb
    check = fb.can_use_gelu if which == "gelu" else fb.can_use_qkv
    return check(x, lin.weight, lin.bias)


class FusedLayerNorm(nn.LayerNorm):
    """LayerNorm that stays in bf16 under autocast.

    torch's autocast policy runs LayerNorm in fp32, casting the whole
    (B, T, C) activation up and back down every call — measured at ~9% of a
    GPT-2-small step on MI355X (profiles/gpt2_train_step_kernels.txt).  The
    native layer_norm kernel already accumulates statistics in fp32, so when
    weights and input share a low-precision dtype we bypass the autocast
    upcast entirely.
    """

    def forward(self, x):
        if (x.is_cuda and x.dtype == torch.bfloat16
                and self.weight.dtype == torch.bfloat16):
            from ..ops import fused_ln
            if fused_ln.can_use(x, self.weight):
                return fused_ln.fused_layer_norm(x, self.weight, self.bias,
                                                 self.eps)
            with torch.autocast("cuda", enabled=False):
                return F.layer_norm(x, self.normalized_shape, self.weight,
                                    self.bias, self.eps)
        return super().forward(x)


def _fused_ln_ok(ln: nn.LayerNorm, x: torch.Tensor) -> bool:
    if (x.is_cuda and x.dtype == torch.bfloat16
            and ln.weight.dtype == torch.bfloat16):
        from ..ops import fused_ln
        return fused_ln.can_use(x, ln.weight)
    return False


def add_ln(ln: nn.LayerNorm, x, delta, delta_bias=None):
    """``x = x + delta [+ delta_bias]; h = ln(x)`` -> (x, h).

    On the fused path the add rides inside the LayerNorm kernels, forward
    and backward (ops/fused_ln.py).  Everywhere else — CPU, fp32, or
    ``fused_ln.can_use`` false — it is the plain torch add followed by
    ``ln(x)``, value for value what ``x = x + f(ln(x))`` computes.
    ``delta=None`` is the first LayerNorm of the model: nothing to add.
    """
    if delta is None:
        return x, ln(x)
    if _fused_ln_ok(ln, x):
        from ..ops import fused_ln
        return fused_ln.fused_add_layer_norm(x, delta, ln.weight, ln.bias,
                                             ln.eps, delta_bias)
    x = x + delta
    if delta_bias is not None:
        x = x + delta_bias
    return x, ln(x)


class CausalSelfAttention(nn.Module):
    def __init__(self, cfg: GPT2Config):
        super().__init__()
        assert cfg.n_embd % cfg.n_head == 0
        self.qkv = nn.Linear(cfg.n_embd, 3 * cfg.n_embd)
        self.proj = nn.Linear(cfg.n_embd, cfg.n_embd)
        self.n_head = cfg.n_head
        self.head_dim = cfg.n_embd // cfg.n_head

    def forward(self, x, proj_bias=True):
        B, T, C = x.shape
        if _bias_grad_ok(_flag("SHTENS_FUSED_QKV_BGRAD", FUSE_QKV_BIAS_GRAD),
                         "qkv", x, self.qkv):
            from ..ops import fused_bias_grad
            qkv = _linear(x, self.qkv.weight, self.qkv.bias.detach())
            q, k, v = fused_bias_grad.qkv_split_bgrad(qkv, self.qkv.bias)
        else:
            q, k, v = _linear(x, self.qkv.weight,
                              self.qkv.bias).split(C, dim=2)
        q = q.view(B, T, self.n_head, self.head_dim).transpose(1, 2)
        k = k.view(B, T, self.n_head, self.head_dim).transpose(1, 2)
        v = v.view(B, T, self.n_head, self.head_dim).transpose(1, 2)
        if _attn_ok(q, k, v):
            from ..ops import fused_attn
            y = fused_attn.fused_causal_attention(q, k, v)
        elif x.is_cuda:
            # CK efficient-attention measured +16% end-to-end over the
            # default aotriton flash backend on MI355X at these shapes
            # (profiles/README.md), identical loss; priority list falls
            # back when a shape is unsupported
            from torch.nn.attention import SDPBackend, sdpa_kernel
            with sdpa_kernel([SDPBackend.EFFICIENT_ATTENTION,
                              SDPBackend.FLASH_ATTENTION, SDPBackend.MATH],
                             set_priority=True):
                y = F.scaled_dot_product_attention(q, k, v, is_causal=True)
        else:
            y = F.scaled_dot_product_attention(q, k, v, is_causal=True)
        y = y.transpose(1, 2).contiguous().view(B, T, C)
        if not proj_bias:  # the caller adds proj.bias (see Block)
            return _linear(y, self.proj.weight)
        return _linear(y, self.proj.weight, self.proj.bias)


class MLP(nn.Module):
    def __init__(self, cfg: GPT2Config):
        super().__init__()
        self.fc = nn.Linear(cfg.n_embd, 4 * cfg.n_embd)
        self.proj = nn.Linear(4 * cfg.n_embd, cfg.n_embd)

    def forward(self, x, proj_bias=True):
        # torch's gelu forward ties our fused kernel here (0.194 vs 0.195 ms
        # on the B=64 shape, profiles/README.md; ops/fused_gelu.py kept as a
        # measured alternative) — keep the library kernel
        if _bias_grad_ok(_flag("SHTENS_FUSED_GELU_BGRAD", FUSE_FC_BIAS_GRAD),
                         "gelu", x, self.fc):
            from ..ops import fused_bias_grad
            pre = _linear(x, self.fc.weight, self.fc.bias.detach())
            h = fused_bias_grad.bias_gelu_bgrad(pre, self.fc.bias)
        else:
            h = F.gelu(_linear(x, self.fc.weight, self.fc.bias),
                       approximate="tanh")
        if not proj_bias:  # the caller adds proj.bias (see Block)
            return _linear(h, self.proj.weight)
        return _linear(h, self.proj.weight, self.proj.bias)


class Block(nn.Module):
    def __init__(self, cfg: GPT2Config):
        super().__init__()
        self.ln1 = FusedLayerNorm(cfg.n_embd)
        self.attn = CausalSelfAttention(cfg)
        self.ln2 = FusedLayerNorm(cfg.n_embd)
        self.mlp = MLP(cfg)

    def forward(self, x, delta=None, delta_bias=None, fuse_proj_bias=False):
        """Takes the residual stream and the previous sub-layer's output not
        yet added to it; returns the same pair (plus that output's bias when
        ``fuse_proj_bias`` leaves it to the next add), so every residual add
        happens inside the LayerNorm that follows it.  With ``delta=None``
        this is ``x = x + attn(ln1(x))`` and the caller owes
        ``x + delta`` for the MLP."""
        x, h = add_ln(self.ln1, x, delta, delta_bias)
        fuse = fuse_proj_bias and _fused_ln_ok(self.ln2, x)
        a = self.attn(h, proj_bias=not fuse)
        x, h = add_ln(self.ln2, x, a, self.attn.proj.bias if fuse else None)
        m = self.mlp(h, proj_bias=not fuse)
        return x, m, (self.mlp.proj.bias if fuse else None)


class GPT2(nn.Module):
    def __init__(self, cfg: GPT2Config):
        super().__init__()
        self.cfg = cfg
        self.wte = nn.Embedding(cfg.vocab_size, cfg.n_embd)
        self.wpe = nn.Embedding(cfg.block_size, cfg.n_embd)
        self.blocks = nn.ModuleList(Block(cfg) for _ in range(cfg.n_layer))
        self.ln_f = FusedLayerNorm(cfg.n_embd)
        self.lm_head = nn.Linear(cfg.n_embd, cfg.vocab_size, bias=False)
        self.lm_head.weight = self.wte.weight  # weight tying
        self.apply(self._init)
        for name, p in self.named_parameters():
            if name.endswith("proj.weight"):
                nn.init.normal_(p, std=0.02 / math.sqrt(2 * cfg.n_layer))

    @staticmethod
    def _init(m):
        if isinstance(m, nn.Linear):
            nn.init.normal_(m.weight, std=0.02)
            if m.bias is not None:
                nn.init.zeros_(m.bias)
        elif isinstance(m, nn.Embedding):
            nn.init.normal_(m.weight, std=0.02)

    def forward(self, idx, targets=None):
        B, T = idx.shape
        pos = torch.arange(T, device=idx.device)
        x = self.wte(idx) + self.wpe(pos)
        delta = delta_bias = None
        for blk in self.blocks:
            x, delta, delta_bias = blk(x, delta, delta_bias,
                                       FUSE_PROJ_BIAS)
        _, x = add_ln(self.ln_f, x, delta, delta_bias)
        logits = self.lm_head(x)
        if targets is None:
            return logits, None
        flat = logits.view(-1, logits.size(-1))
        tgt = targets.reshape(-1)
        cfg = self.cfg
        if cfg.ignore_index is not None or cfg.label_smoothing != 0.0 \
                or cfg.z_loss != 0.0:
            # cuda/bf16: the fused kernels with the options; every other
            # path the same semantics in plain torch
            from ..ops import fused_ce
            opts = dict(ignore_index=cfg.ignore_index,
                        label_smoothing=cfg.label_smoothing,
                        z_loss=cfg.z_loss)
            if fused_ce.can_use(flat):
                return logits, fused_ce.fused_cross_entropy(flat, tgt, **opts)
            return logits, fused_ce.cross_entropy_reference(flat.float(), tgt,
                                                            **opts)
        if flat.is_cuda and flat.dtype == torch.bfloat16:
            from ..ops import fused_ce
            if fused_ce.can_use(flat):
                return logits, fused_ce.fused_cross_entropy(flat, tgt)
        loss = F.cross_entropy(flat, tgt)
        return logits, loss

    def num_params(self) -> int:
        return sum(p.numel() for p in self.parameters())
