"""Async data parallelism over the shared-tensor engine.

The reference's one parallelism strategy: N workers
each run a local training loop against a replicated parameter tensor; the
engine gossips compressed deltas continuously in the background, fully
overlapped with compute.  There is no lockstep all-reduce — staleness is
bounded by the compression scale, not by synchronization.

This module wires a torch model into that scheme MI355X-style:
  * all parameters live as views of one flat fp32 replica in HBM3E
    (zero-copy: the forward pass reads the live gossip target)
  * all gradients accumulate into one flat buffer (views as .grad)
  * the optimizer update is ONE fused HIP kernel (k_fused_sgd) that computes
    momentum, applies -lr*m to the replica AND stages it into every link's
    residual delta in a single HBM pass.
  * optional global-norm gradient clipping (max_grad_norm): one extra
    read-only pass over the flat gradient leaves the clip coefficient in
    device memory, the fused step reads it from there — no host sync, no
    extra gradient write — and a step whose gradient holds an inf or NaN
    is skipped on the device, so it never reaches the replica or the link
    residuals.
  * optional parameter groups (param_groups): per-tensor weight decay and
    learning-rate scale from a small segment table that the same fused
    kernel reads — biases and norm gains without decay, still one pass.
"""
from __future__ import annotations

import math
import os
from typing import List, Optional

import torch

from ..engine import _SharedBase


def tree_parent(rank: int) -> int:
    """rank 0 is the root; children of r are 2r+1, 2r+2 (balanced binary
    tree over one node's GPUs — each edge is one xGMI hop)."""
    return (rank - 1) // 2


def tree_children(rank: int, world: int):
    return [c for c in (2 * rank + 1, 2 * rank + 2) if c < world]


class FlatParamShared(_SharedBase):
    """Shares a model's parameters as one flat fp32 tensor (BASELINE
    config 3: 'params as one shared tensor')."""

    def __init__(self, model: torch.nn.Module, host: str, port_base: int,
                 rank: int, world: int, param_dtype: torch.dtype = torch.float32,
                 **kw):
        params = [p for p in model.parameters() if p.requires_grad]
        # dedupe tied parameters (GPT-2 ties lm_head.weight to wte.weight)
        seen, uniq = set(), []
        for p in params:
            if id(p) not in seen:
                seen.add(id(p))
                uniq.append(p)
        self.params = uniq
        # every name of each unique parameter (a tied one has several)
        names = {}
        for name, p in model.named_parameters(remove_duplicate=False):
            names.setdefault(id(p), []).append(name)
        self.param_names = [names.get(id(p), []) for p in self.params]
        sizes = [p.numel() for p in self.params]
        device = self.params[0].device
        n = sum(sizes)

        nchild = len(tree_children(rank, world))
        explicit_parent = ""
        listen_port = 0
        if world > 1:
            listen_port = port_base + rank
            if rank > 0:
                explicit_parent = f"{host}:{port_base + tree_parent(rank)}"
        kw.setdefault("expected_children", nchild if world > 1 else 0)
        super().__init__(host, port_base, [n], device=device,
                         provision_up=rank > 0,
                         explicit_parent=explicit_parent,
                         listen_port=listen_port, **kw)

        # snapshot initial params, re-point them into the replica slab (fp32)
        # or into a bf16 shadow of it (mixed precision: bf16 matmuls without
        # autocast's per-op weight casts; fp32 master stays in the engine)
        init_flat = torch.cat([p.detach().reshape(-1) for p in self.params]).float()
        self.param_dtype = param_dtype
        self.mom_flat = torch.zeros(n, dtype=torch.float32, device=device)
        if param_dtype == torch.bfloat16:
            if not self._gpu:
                raise ValueError("bf16 shadow params need a GPU")
            self.shadow = torch.empty(n, dtype=torch.bfloat16, device=device)
            self.grad_flat = torch.zeros(n, dtype=torch.bfloat16, device=device)
            param_src = self.shadow
        else:
            self.shadow = None
            self.grad_flat = torch.zeros(n, dtype=torch.float32, device=device)
            param_src = self.values
        off = 0
        for p in self.params:
            sz = p.numel()
            p.data = param_src[off:off + sz].view(p.shape)
            p.grad = self.grad_flat[off:off + sz].view(p.shape)
            off += sz

        self._start()
        if self.is_master:
            # seed the shared state with this rank's init (master's weights
            # win; other ranks receive them via snapshot/gossip)
            self._add_flat(init_flat)
        if self.shadow is not None:
            # initial shadow refresh (post-join: values now hold the state)
            self.shadow.copy_(self.values)
        self.rank = rank
        self.world = world


def _check_max_grad_norm(max_grad_norm: Optional[float]) -> Optional[float]:
    if max_grad_norm is None:
        return None
    c = float(max_grad_norm)
    if not (math.isfinite(c) and c > 0.0):
        raise ValueError("max_grad_norm must be finite and > 0 (or None)")
    return c


class _ClipMixin:
    """max_grad_norm handling shared by the two optimizers: this rank's own
    global L2 norm (each rank takes its own step, so each clips its own
    gradient), torch's clip_grad_norm_ coefficient, and a step that is
    skipped on the device when the gradient holds an inf or NaN."""

    def _clip_state(self) -> Optional[torch.Tensor]:
        if self.max_grad_norm is None:
            return None
        return self.shared.grad_clip_coef(self.shared.grad_flat,
                                          self.max_grad_norm)

    def grad_stats(self) -> Optional[dict]:
        """{"grad_norm", "clip_coef", "skipped", "skipped_steps"} of the
        latest step (syncs), or None when clipping is off or no step ran."""
        if self.max_grad_norm is None or self.shared._clip_state is None:
            return None
        d = self.shared.decode_clip_state(self.shared._clip_state)
        del d["sumsq"]
        return d


def no_decay_groups(model: torch.nn.Module, weight_decay: float) -> List[dict]:
    """param_groups for the usual AdamW policy: parameters with ndim < 2
    (biases, LayerNorm/RMSNorm gains) are not decayed, everything else
    decays with `weight_decay`."""
    decay, plain = [], []
    for name, p in model.named_parameters():
        if p.requires_grad:
            (plain if p.ndim < 2 else decay).append(name)
    groups = []
    if decay:
        groups.append({"params": decay, "weight_decay": float(weight_decay)})
    if plain:
        groups.append({"params": plain, "weight_decay": 0.0})
    return groups


class _GroupMixin:
    """param_groups handling shared by the two optimizers.  Each entry is a
    torch-style dict {"params": [...], "weight_decay": float, "lr_scale":
    float}: params are nn.Parameter objects or names from
    model.named_parameters(); omitted keys default to the optimizer's
    weight_decay and to 1.0; parameters that no entry lists form a last,
    default group.  A tied parameter is one parameter under all its names.
    The groups become one segment table in FlatParamShared.params order
    (engine.make_group_table) that the fused kernel reads."""

    def _init_groups(self, param_groups, default_wd: float, decays: bool):
        sh = self.shared
        self._groups = None
        if param_groups is None:
            self._group_info = [{
                "names": [ns[0] for ns in sh.param_names if ns],
                "numel": sh.n, "weight_decay": float(default_wd),
                "lr_scale": 1.0}]
            return
        by_id = {id(p): k for k, p in enumerate(sh.params)}
        by_name = {n: k for k, ns in enumerate(sh.param_names) for n in ns}
        owner = [None] * len(sh.params)
        info = []
        for gi, entry in enumerate(param_groups):
            unknown = set(entry) - {"params", "weight_decay", "lr_scale"}
            if unknown:
                raise ValueError(f"param group {gi}: unknown keys "
                                 f"{sorted(unknown)}")
            members = list(entry.get("params", ()))
            if not members:
                raise ValueError(f"param group {gi} is empty")
            for m in members:
                if isinstance(m, str):
                    if m not in by_name:
                        raise ValueError(f"param group {gi}: no parameter "
                                         f"named {m!r}")
                    k = by_name[m]
                elif id(m) in by_id:
                    k = by_id[id(m)]
                else:
                    raise ValueError(f"param group {gi}: a parameter that "
                                     "the model does not train")
                if owner[k] is not None:
                    raise ValueError(
                        f"parameter {sh.param_names[k][:1] or k} is listed "
                        "twice")
                owner[k] = gi
            info.append({"weight_decay": float(entry.get("weight_decay",
                                                         default_wd)),
                         "lr_scale": float(entry.get("lr_scale", 1.0))})
        if any(o is None for o in owner):
            info.append({"weight_decay": float(default_wd), "lr_scale": 1.0})
            owner = [len(info) - 1 if o is None else o for o in owner]
        if not decays and any(g["weight_decay"] != 0.0 for g in info):
            raise ValueError("the fused SGD step has no weight decay: a "
                             "group's weight_decay must be 0")
        for g in info:
            g["names"], g["numel"] = [], 0
        for k, p in enumerate(sh.params):
            g = info[owner[k]]
            g["names"].append(sh.param_names[k][0] if sh.param_names[k]
                              else str(k))
            g["numel"] += p.numel()
        self._group_info = info
        self._groups = sh.make_group_table(
            [p.numel() for p in sh.params], owner,
            [g["lr_scale"] for g in info], [g["weight_decay"] for g in info])

    @property
    def param_groups(self) -> List[dict]:
        """Read-only: one dict per group with names, numel, weight_decay and
        lr_scale (a copy; change values with set_group)."""
        return [dict(g, names=list(g["names"])) for g in self._group_info]

    def set_group(self, i: int, weight_decay: Optional[float] = None,
                  lr_scale: Optional[float] = None):
        """New weight_decay and/or lr_scale for group i, from the next step
        on (the table is rewritten in stream order)."""
        if self._groups is None:
            raise ValueError("set_group needs an optimizer built with "
                             "param_groups")
        g = dict(self._group_info[i])
        if weight_decay is not None:
            if not self._decays and float(weight_decay) != 0.0:
                raise ValueError("the fused SGD step has no weight decay")
            g["weight_decay"] = float(weight_decay)
        if lr_scale is not None:
            g["lr_scale"] = float(lr_scale)
        new = list(self._group_info)
        new[i] = g
        self.shared.update_group_table(
            self._groups, lr_scale=[x["lr_scale"] for x in new],
            weight_decay=[x["weight_decay"] for x in new])
        self._group_info = new


class AsyncSGD(_ClipMixin, _GroupMixin):
    """SGD-momentum whose update feeds the shared tensor through the fused
    kernel — the optimizer step IS the addFromTensor.

    max_grad_norm: clip this rank's gradient to that global L2 norm inside
    the fused step; a non-finite gradient skips the step (momentum, weights
    and link residuals untouched).

    param_groups: see _GroupMixin; only lr_scale applies, a group with a
    non-zero weight_decay is a ValueError."""

    _decays = False

    def __init__(self, shared: FlatParamShared, lr: float = 0.1,
                 momentum: float = 0.9,
                 max_grad_norm: Optional[float] = None, param_groups=None):
        self.shared = shared
        self.lr = lr
        self.momentum = momentum
        self.max_grad_norm = _check_max_grad_norm(max_grad_norm)
        self._init_groups(param_groups, 0.0, decays=False)

    def step(self):
        clip = self._clip_state()
        if self.shared.shadow is not None:
            self.shared.fused_sgd_bf16_step(self.shared.mom_flat,
                                            self.shared.grad_flat,
                                            self.shared.shadow, self.lr,
                                            self.momentum, clip_state=clip,
                                            groups=self._groups)
        else:
            self.shared.fused_sgd_step(self.shared.mom_flat,
                                       self.shared.grad_flat,
                                       self.lr, self.momentum,
                                       clip_state=clip, groups=self._groups)

    def zero_grad(self, set_to_none: bool = False):
        self.shared.grad_flat.zero_()


class AsyncAdamW(_ClipMixin, _GroupMixin):
    """AdamW whose update feeds the shared tensor through the fused kernel
    (torch.optim.AdamW semantics: decoupled weight decay on the pre-update
    master weight) — the optimizer step IS the addFromTensor.

    max_grad_norm: clip this rank's gradient to that global L2 norm inside
    the fused step; a non-finite gradient skips the step (m, v, weights,
    shadow and link residuals untouched).  Deviation from a host-side
    skip: `step_count`, and with it the bias correction, still advances on
    a skipped step, because the host cannot know about the skip without a
    sync.

    param_groups: per-group weight_decay and lr_scale, see _GroupMixin and
    no_decay_groups."""

    _decays = True

    def __init__(self, shared: FlatParamShared, lr: float = 3e-4,
                 betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.01,
                 max_grad_norm: Optional[float] = None, param_groups=None):
        self.shared = shared
        self.max_grad_norm = _check_max_grad_norm(max_grad_norm)
        self.lr = lr
        self.betas = betas
        self.eps = eps
        self.weight_decay = weight_decay
        self.step_count = 0
        self.vel_flat = torch.zeros(shared.n, dtype=torch.float32,
                                    device=shared.device)
        self._init_groups(param_groups, weight_decay, decays=True)

    def step(self):
        self.step_count += 1
        sh = self.shared
        clip = self._clip_state()
        if sh.shadow is not None:
            sh.fused_adamw_bf16_step(sh.mom_flat, self.vel_flat, sh.grad_flat,
                                     sh.shadow, self.step_count, self.lr,
                                     self.betas, self.eps, self.weight_decay,
                                     clip_state=clip, groups=self._groups)
        else:
            sh.fused_adamw_step(sh.mom_flat, self.vel_flat, sh.grad_flat,
                                self.step_count, self.lr, self.betas,
                                self.eps, self.weight_decay, clip_state=clip,
                                groups=self._groups)

    def zero_grad(self, set_to_none: bool = False):
        self.shared.grad_flat.zero_()


class AsyncDPTrainer:
    """One rank's training loop against the shared parameter tensor.

    max_grad_norm (default None: off) clips this rank's gradient to that
    global L2 norm inside the fused optimizer step and skips a step whose
    gradient is not finite; see AsyncSGD / AsyncAdamW and grad_stats().

    param_groups (default None: one rate and one decay for everything)
    gives tensors their own weight decay and learning-rate scale inside the
    same fused step, e.g. param_groups=no_decay_groups(model, 0.1); see
    _GroupMixin, opt.param_groups and opt.set_group()."""

    def __init__(self, model: torch.nn.Module, host: str = "127.0.0.1",
                 port_base: Optional[int] = None, rank: Optional[int] = None,
                 world: Optional[int] = None, lr: float = 0.1,
                 momentum: float = 0.9, amp_dtype: Optional[torch.dtype] = torch.bfloat16,
                 param_dtype: Optional[torch.dtype] = None,
                 optimizer: str = "sgd", betas=(0.9, 0.999),
                 eps: float = 1e-8, weight_decay: float = 0.0,
                 max_grad_norm: Optional[float] = None, param_groups=None,
                 **engine_kw):
        max_grad_norm = _check_max_grad_norm(max_grad_norm)
        rank = int(os.environ.get("RANK", 0)) if rank is None else rank
        world = int(os.environ.get("WORLD_SIZE", 1)) if world is None else world
        if port_base is None:
            port_base = int(os.environ.get("SHTENS_PORT_BASE", 21000))
        self.model = model
        if param_dtype is None:
            param_dtype = torch.float32
        self.shared = FlatParamShared(model, host, port_base, rank, world,
                                      param_dtype=param_dtype, **engine_kw)
        if optimizer == "adamw":
            self.opt = AsyncAdamW(self.shared, lr=lr, betas=betas, eps=eps,
                                  weight_decay=weight_decay,
                                  max_grad_norm=max_grad_norm,
                                  param_groups=param_groups)
        elif optimizer == "sgd":
            self.opt = AsyncSGD(self.shared, lr=lr, momentum=momentum,
                                max_grad_norm=max_grad_norm,
                                param_groups=param_groups)
        else:
            raise ValueError(f"unknown optimizer {optimizer!r}")
        self.amp_dtype = amp_dtype
        self.rank, self.world = rank, world
        self.device = self.shared.device

    def step(self, batch, targets) -> torch.Tensor:
        self.opt.zero_grad()
        use_amp = self.amp_dtype is not None and self.device.type == "cuda"
        with torch.autocast(device_type="cuda", dtype=self.amp_dtype,
                            enabled=use_amp):
            _, loss = self.model(batch, targets)
        loss.backward()
        self.opt.step()
        return loss.detach()

    def stats(self):
        return self.shared.stats()

    def grad_stats(self) -> Optional[dict]:
        """Norm and clipping of the latest step: {"grad_norm": fp32 global
        L2 norm before clipping (inf/nan on a skipped step), "clip_coef":
        the factor applied (0 on a skipped step), "skipped": whether the
        latest step was skipped, "skipped_steps": how many were so far}.
        Waits for the device.  None when max_grad_norm is None."""
        return self.opt.grad_stats()

    def close(self):
        self.shared.close()
