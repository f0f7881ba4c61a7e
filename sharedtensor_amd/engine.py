"""Python API of the MI355X-native shared-tensor engine.

Mirrors the reference's three-call surface (createOrFetch / copyToTensor /
addFromTensor, /root/reference/src/sharedtensor.c:347-453) on top of the
native engine (csrc/engine.cpp), and extends it with the features the
reference's README names as missing (README.md:29-47): table-of-tensors sync
with per-tensor scales, real GPU codec kernels, bandwidth limiting,
reconnection, observability.

All large buffers (replica, per-link residual deltas, message staging) are
torch tensors allocated here and handed to the engine as raw pointers, so the
replica lives in HBM3E, integrates with torch's allocator, and `values` can
be viewed zero-copy as model parameters.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Union

import torch

from . import _core

CODECS = {"1bit": 0, "fp8": 1, "int4": 2}


def _percentile(xs: List[float], q: float) -> Optional[float]:
    if not xs:
        return None
    s = sorted(xs)
    i = min(int(q * len(s)), len(s) - 1)
    return s[i]


class _SharedBase:
    """Engine lifecycle + buffer management shared by SharedTensor/SharedTable."""

    def __init__(self, host: str, port: int, sizes: Sequence[int],
                 device: torch.device, codec: str = "1bit", *,
                 snapshot_join: bool = True, use_rccl: bool = True,
                 reconnect: bool = False, preserve_subtree: bool = False,
                 keepalive_s: float = 1.0,
                 bw_limit: float = 0.0, sync_interval_s: float = 0.0,
                 expected_children: int = 2,
                 provision_up: bool = True, explicit_parent: str = "",
                 listen_port: int = 0, join_timeout_s: float = 60.0,
                 rms_sample_stride: int = 1, lagged_scale: bool = False,
                 delta_dtype: torch.dtype = torch.float32,
                 use_graphs: bool = False):
        if codec not in CODECS:
            raise ValueError(f"codec must be one of {list(CODECS)}")
        self.device = torch.device(device)
        self._gpu = self.device.type == "cuda"
        cfg = _core.Config()
        cfg.host = host
        cfg.port = int(port)
        cfg.device = (self.device.index or 0) if self._gpu else -1
        cfg.codec = CODECS[codec]
        cfg.snapshot_join = snapshot_join
        cfg.use_rccl = use_rccl
        cfg.reconnect = reconnect
        if preserve_subtree and not snapshot_join:
            raise ValueError("preserve_subtree requires snapshot_join")
        cfg.preserve_subtree = preserve_subtree
        cfg.keepalive_s = keepalive_s
        cfg.bw_limit = float(bw_limit)
        cfg.min_round_interval_s = float(sync_interval_s)
        cfg.expected_children = expected_children
        cfg.sizes = [int(s) for s in sizes]
        cfg.explicit_parent = explicit_parent
        cfg.listen_port = int(listen_port)
        cfg.join_timeout_s = join_timeout_s
        cfg.rms_sample_stride = rms_sample_stride
        cfg.lagged_scale = bool(lagged_scale)
        if delta_dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("delta_dtype must be float32 or bfloat16")
        if delta_dtype == torch.bfloat16 and not self._gpu:
            raise ValueError("bf16 residual deltas need a GPU engine")
        cfg.delta_bf16 = delta_dtype == torch.bfloat16
        self.delta_dtype = delta_dtype
        cfg.use_graphs = bool(use_graphs)
        self.codec = codec
        self.n = int(sum(sizes))
        self._cfg = cfg
        self._closed = False
        self._clip_state = None      # allocated by the first grad_clip_coef
        self._clip_scratch = None
        self._group_shapes = {}      # table data_ptr -> (S, G, table)

        msg = _core.msg_bytes(cfg)
        self.values = torch.zeros(self.n, dtype=torch.float32, device=self.device)
        self._eng = _core.Engine(cfg)
        self._eng.set_values(self.values.data_ptr())

        self._link_bufs = []
        links = []
        if provision_up:
            links.append(0)
        links += [1, 2][: max(0, min(2, expected_children))]
        for li in (0, 1, 2):
            if li not in links:
                continue
            delta = torch.zeros(self.n, dtype=self.delta_dtype,
                                device=self.device)
            if self._gpu:
                # zeros (one-time cost): the scales-area padding beyond 4*T
                # bytes is never written by any kernel, and uninitialized HBM
                # must not leak onto the wire (WIRE_FORMAT.md: pad is zero)
                send_buf = torch.zeros(msg, dtype=torch.uint8, device=self.device)
                recv_buf = torch.zeros(msg, dtype=torch.uint8, device=self.device)
                send_pin = torch.empty(8 + msg, dtype=torch.uint8, pin_memory=True)
                recv_pin = torch.empty(8 + msg, dtype=torch.uint8, pin_memory=True)
                bufs = (delta, send_buf, recv_buf, send_pin, recv_pin)
                self._eng.set_link_buffers(li, delta.data_ptr(), send_buf.data_ptr(),
                                           recv_buf.data_ptr(), send_pin.data_ptr(),
                                           recv_pin.data_ptr())
            else:
                send_pin = torch.zeros(8 + msg, dtype=torch.uint8)
                recv_pin = torch.zeros(8 + msg, dtype=torch.uint8)
                bufs = (delta, send_pin, recv_pin)
                self._eng.set_link_buffers(li, delta.data_ptr(), 0, 0,
                                           send_pin.data_ptr(), recv_pin.data_ptr())
            self._link_bufs.append(bufs)

    # -- lifecycle ---------------------------------------------------------
    def _start(self):
        self._eng.start()

    @property
    def is_master(self) -> bool:
        return self._eng.is_master()

    @property
    def listen_port(self) -> int:
        return self._eng.listen_port()

    def close(self):
        if not self._closed:
            self._closed = True
            self._eng.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- shared-memory ops -------------------------------------------------
    def _stream(self) -> int:
        if self._gpu:
            return torch.cuda.current_stream(self.device).cuda_stream
        return 0

    def _add_flat(self, flat: torch.Tensor):
        if flat.dtype != torch.float32 or not flat.is_contiguous():
            raise TypeError("expected a contiguous float32 tensor")
        self._eng.add_from(flat.data_ptr(), flat.numel(), self._stream())

    def _copy_flat(self, flat: torch.Tensor):
        if flat.dtype != torch.float32 or not flat.is_contiguous():
            raise TypeError("expected a contiguous float32 tensor")
        self._eng.copy_to(flat.data_ptr(), flat.numel(), self._stream())

    def grad_clip_coef(self, grad: torch.Tensor,
                       max_norm: float) -> torch.Tensor:
        """Global L2 norm of the flat gradient and torch's clip coefficient
        min(1, max_norm / (norm + 1e-6)), computed on the engine's device
        and stream with no host sync (HIP kernels k_grad_sumsq and
        k_grad_clip_finalize: fp64, no atomics, bitwise reproducible).

        Returns the 32-byte clip state as 8 int32 words on the engine's
        device; hand it to a fused step as `clip_state`.  The same tensor is
        written again by every call.  Layout: f64 sumsq | f32 norm | f32
        coef | u32 skip | u32 skipped_total | 8 bytes padding.  skip is 1
        when some gradient is inf or NaN (coef is then 0 and a fused step
        given this state changes nothing); skipped_total counts such calls.
        `decode_clip_state` turns it into python numbers (that one syncs)."""
        max_norm = float(max_norm)
        if not (max_norm > 0.0 and max_norm != float("inf")):
            raise ValueError("max_norm must be finite and > 0")
        if grad.numel() != self.n or not grad.is_contiguous():
            raise ValueError("grad must be the contiguous flat gradient")
        if grad.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError("grad must be float32 or bfloat16")
        if grad.device.type != self.device.type:
            raise ValueError("grad must live on the engine's device")
        if self._clip_state is None:
            self._clip_state = torch.zeros(8, dtype=torch.int32,
                                           device=self.device)
            self._clip_scratch = torch.empty(
                _core.GRAD_CLIP_MAX_BLOCKS if self._gpu else 1,
                dtype=torch.float64, device=self.device)
        self._eng.grad_clip_coef(grad.data_ptr(),
                                 grad.dtype == torch.bfloat16, self.n,
                                 max_norm, self._clip_scratch.data_ptr(),
                                 self._clip_state.data_ptr(), self._stream())
        return self._clip_state

    @staticmethod
    def decode_clip_state(state: torch.Tensor) -> dict:
        """The clip state as python numbers.  Copies to the host, which
        waits for the work queued before it."""
        w = state.detach().cpu()
        return {"sumsq": float(w[0:2].view(torch.float64)[0]),
                "grad_norm": float(w[2:3].view(torch.float32)[0]),
                "clip_coef": float(w[3:4].view(torch.float32)[0]),
                "skipped": bool(int(w[4]) & 0xFFFFFFFF),
                "skipped_steps": int(w[5]) & 0xFFFFFFFF}

    def _clip_ptr(self, clip_state: Optional[torch.Tensor]) -> int:
        if clip_state is None:
            return 0
        if (clip_state.dtype != torch.int32 or clip_state.numel() != 8
                or not clip_state.is_contiguous()
                or clip_state.device.type != self.device.type):
            raise TypeError("clip_state must be the 8-word int32 tensor that "
                            "grad_clip_coef returned")
        return clip_state.data_ptr()

    # -- parameter groups --------------------------------------------------
    def make_group_table(self, seg_sizes: Sequence[int],
                         seg_group: Sequence[int],
                         lr_scale: Sequence[float],
                         weight_decay: Sequence[float]) -> torch.Tensor:
        """Parameter-group table for the fused steps' `groups` argument: the
        flat buffer as consecutive segments of `seg_sizes` elements, segment
        s in group `seg_group[s]`, group g stepping with the rate
        fl32(lr * lr_scale[g]) and (AdamW) the decay weight_decay[g].

        Validated and coalesced (adjacent segments of one group merge) by
        _core.build_group_table, then placed on the engine's device as int32
        words.  Layout (csrc/common.h): i64 n | i32 S | i32 G | i64
        seg_end[S] | i32 seg_group[S] | f32 lr_scale[G] | f32
        weight_decay[G].  ValueError unless the sizes are positive and sum
        to n, group indices are in range, the per-group values are finite
        and >= 0, there is at least one group, and at most
        _core.GROUP_MAX_SEGMENTS segments remain after merging."""
        sizes = [int(x) for x in seg_sizes]
        if sum(sizes) != self.n:
            raise ValueError(f"segments cover {sum(sizes)} elements, the "
                             f"tensor has {self.n}")
        ends, end = [], 0
        for x in sizes:
            end += x
            ends.append(end)
        words = _core.build_group_table(self.n, ends,
                                        [int(g) for g in seg_group],
                                        [float(x) for x in lr_scale],
                                        [float(x) for x in weight_decay])
        table = torch.tensor(words, dtype=torch.int32).to(self.device)
        self._group_shapes[table.data_ptr()] = (int(words[2]), int(words[3]),
                                                table)
        return table

    def _groups_ptr(self, groups: Optional[torch.Tensor]) -> int:
        if groups is None:
            return 0
        if (not isinstance(groups, torch.Tensor)
                or self._group_shapes.get(groups.data_ptr(),
                                          (0, 0, None))[2] is not groups):
            raise TypeError("groups must be a table that this object's "
                            "make_group_table returned")
        return groups.data_ptr()

    def update_group_table(self, table: torch.Tensor,
                           lr_scale: Optional[Sequence[float]] = None,
                           weight_decay: Optional[Sequence[float]] = None):
        """Rewrites the per-group values of `table` (all G of either kind).
        The write is ordered on the engine's stream like the fused steps: a
        step queued earlier still reads the old values."""
        self._groups_ptr(table)
        S, G, _ = self._group_shapes[table.data_ptr()]
        for k, vals in enumerate((lr_scale, weight_decay)):
            if vals is None:
                continue
            v = torch.tensor([float(x) for x in vals], dtype=torch.float32)
            if v.numel() != G:
                raise ValueError(f"expected {G} per-group values")
            if not bool((torch.isfinite(v) & (v >= 0)).all()):
                raise ValueError("lr_scale and weight_decay must be finite "
                                 "and >= 0")
            at = 4 + 3 * S + k * G
            table[at:at + G].copy_(v.view(torch.int32))

    def fused_sgd_step(self, momentum_buf: torch.Tensor, grad: torch.Tensor,
                       lr: float, momentum: float = 0.9,
                       clip_state: Optional[torch.Tensor] = None,
                       groups: Optional[torch.Tensor] = None):
        """m = mu*m + g; u = -lr*m; {replica, link deltas} += u — one fused
        HBM pass (HIP kernel k_fused_sgd) instead of optimizer + addFromTensor.
        With `clip_state` (see grad_clip_coef) g is fl32(g * coef), or the
        step changes nothing when the state says skip.  With `groups` (see
        make_group_table) each segment steps with fl32(lr * lr_scale[g]),
        still in one pass (k_fused_sgd_grp); SGD has no weight decay."""
        if momentum_buf.numel() != self.n or grad.numel() != self.n:
            raise ValueError("size mismatch")
        self._eng.fused_sgd(momentum_buf.data_ptr(), grad.data_ptr(),
                            float(lr), float(momentum), self._stream(),
                            self._clip_ptr(clip_state),
                            self._groups_ptr(groups))

    def fused_sgd_bf16_step(self, momentum_buf: torch.Tensor,
                            grad_bf16: torch.Tensor, shadow_bf16: torch.Tensor,
                            lr: float, momentum: float = 0.9,
                            clip_state: Optional[torch.Tensor] = None,
                            groups: Optional[torch.Tensor] = None):
        """Mixed-precision fused step: bf16 grads in, fp32 master updated,
        bf16 shadow params refreshed, link deltas staged — one HBM pass
        (HIP kernel k_fused_sgd_bf16).  `clip_state`, `groups`: as
        fused_sgd_step; the scaled gradient stays fp32."""
        if grad_bf16.dtype != torch.bfloat16 or shadow_bf16.dtype != torch.bfloat16:
            raise TypeError("grad/shadow must be bfloat16")
        if not (momentum_buf.numel() == grad_bf16.numel()
                == shadow_bf16.numel() == self.n):
            raise ValueError("size mismatch")
        self._eng.fused_sgd_bf16(momentum_buf.data_ptr(), grad_bf16.data_ptr(),
                                 shadow_bf16.data_ptr(), float(lr),
                                 float(momentum), self._stream(),
                                 self._clip_ptr(clip_state),
                                 self._groups_ptr(groups))

    def fused_adamw_step(self, mom: torch.Tensor, vel: torch.Tensor,
                         grad: torch.Tensor, step: int, lr: float,
                         betas=(0.9, 0.999), eps: float = 1e-8,
                         weight_decay: float = 0.0,
                         clip_state: Optional[torch.Tensor] = None,
                         groups: Optional[torch.Tensor] = None):
        """torch.optim.AdamW-semantics update feeding the shared tensor:
        fp32 m/v, decoupled weight decay on the pre-update master weight,
        update applied to the replica AND staged into every link delta in
        one HBM pass (HIP kernel k_fused_adamw).  `clip_state`: as
        fused_sgd_step; a skipped step leaves m, v and the weights alone.
        `groups` (see make_group_table): each segment steps with
        fl32(lr * lr_scale[g]) and weight_decay[g]; `weight_decay` is then
        unused (HIP kernel k_fused_adamw_grp, still one pass)."""
        if not (mom.numel() == vel.numel() == grad.numel() == self.n):
            raise ValueError("size mismatch")
        if grad.dtype != torch.float32:
            raise TypeError("fused_adamw_step takes fp32 grads "
                            "(use fused_adamw_bf16_step)")
        self._eng.fused_adamw(mom.data_ptr(), vel.data_ptr(), grad.data_ptr(),
                              False, 0, float(lr), float(betas[0]),
                              float(betas[1]), float(eps),
                              float(weight_decay), int(step), self._stream(),
                              self._clip_ptr(clip_state),
                              self._groups_ptr(groups))

    def fused_adamw_bf16_step(self, mom: torch.Tensor, vel: torch.Tensor,
                              grad_bf16: torch.Tensor,
                              shadow_bf16: torch.Tensor, step: int, lr: float,
                              betas=(0.9, 0.999), eps: float = 1e-8,
                              weight_decay: float = 0.0,
                              clip_state: Optional[torch.Tensor] = None,
                              groups: Optional[torch.Tensor] = None):
        """Mixed-precision fused AdamW: bf16 grads in, fp32 master updated,
        bf16 shadow params refreshed (folding concurrent gossip), link
        deltas staged — one HBM pass.  `clip_state`, `groups`: as
        fused_adamw_step."""
        if grad_bf16.dtype != torch.bfloat16 or shadow_bf16.dtype != torch.bfloat16:
            raise TypeError("grad/shadow must be bfloat16")
        if not (mom.numel() == vel.numel() == grad_bf16.numel()
                == shadow_bf16.numel() == self.n):
            raise ValueError("size mismatch")
        self._eng.fused_adamw(mom.data_ptr(), vel.data_ptr(),
                              grad_bf16.data_ptr(), True,
                              shadow_bf16.data_ptr(), float(lr),
                              float(betas[0]), float(betas[1]), float(eps),
                              float(weight_decay), int(step), self._stream(),
                              self._clip_ptr(clip_state),
                              self._groups_ptr(groups))

    # -- observability -----------------------------------------------------
    def stats(self) -> dict:
        links = self._eng.link_stats()
        recv_scales = self._eng.recent_scales_recv()
        sent_scales = self._eng.recent_scales_sent()
        return {
            "is_master": self.is_master,
            "listen_port": self.listen_port,
            "links": links,
            "rounds_sent": sum(l["rounds_sent"] for l in links),
            "rounds_recv": sum(l["rounds_recv"] for l in links),
            "bytes_sent": sum(l["bytes_sent"] for l in links),
            "bytes_recv": sum(l["bytes_recv"] for l in links),
            # the per-round scale IS the live staleness measure: every packet
            # moves each element by exactly +-scale
            "staleness_p50": _percentile(recv_scales, 0.5),
            "staleness_p90": _percentile(recv_scales, 0.9),
            "sent_scale_p50": _percentile(sent_scales, 0.5),
            "reconnects": self._eng.reconnect_count(),
            "last_error": self._eng.last_error(),
        }

    def notify(self):
        self._eng.notify_dirty()


class SharedTensor(_SharedBase):
    """A distributed shared tensor (reference API parity).

    The first process to bind (host, port) becomes the master and seeds the
    shared state with `tensor`'s contents; later processes join the
    self-organizing binary tree and receive the state (snapshot fast-path or
    the reference's converging-delta bootstrap).
    """

    def __init__(self, host: str, port: int, tensor: torch.Tensor, **kw):
        if tensor.dtype != torch.float32:
            raise TypeError("shared tensor must be float32 (fp32 replica + "
                            "compressed wire deltas)")
        self.shape = tuple(tensor.shape)
        super().__init__(host, port, [tensor.numel()],
                         device=tensor.device, **kw)
        self._start()
        if self.is_master:
            self._add_flat(tensor.detach().contiguous().view(-1).float())

    # reference-style API -------------------------------------------------
    def copy_to_tensor(self, tensor: torch.Tensor):
        if tuple(tensor.shape) != self.shape:
            tensor = tensor.view(self.shape)
        flat = tensor.view(-1)
        if not flat.is_contiguous() or flat.dtype != torch.float32:
            raise TypeError("copy_to_tensor needs a contiguous float32 tensor")
        self._copy_flat(flat)

    def add_from_tensor(self, tensor: torch.Tensor):
        flat = tensor.detach().contiguous().view(-1)
        if flat.dtype != torch.float32:
            raise TypeError("add_from_tensor needs a float32 tensor")
        if flat.numel() != self.n:
            raise ValueError("size mismatch")
        self._add_flat(flat)

    # camelCase aliases matching the reference Lua API (example.lua:15,22)
    copyToTensor = copy_to_tensor
    addFromTensor = add_from_tensor

    def view(self) -> torch.Tensor:
        """Zero-copy view of the live replica (mutated by the gossip engine;
        reads are the async-approximate contract, README.md:20-24)."""
        return self.values.view(self.shape)

    # checkpointing: the reference's only "restore" is joining (the
    # accumulated-delta bootstrap); we add explicit save/restore on top
    def save(self, path: str):
        torch.save({"values": self.values.detach().cpu(),
                    "shape": self.shape, "codec": self.codec}, path)

    @classmethod
    def restore(cls, host: str, port: int, path: str,
                device="cpu", **kw) -> "SharedTensor":
        """Create/join a shared tensor seeded from a checkpoint.  If this
        process becomes master, the checkpointed values seed the tree;
        otherwise the live tree state wins (by reference join semantics)."""
        ckpt = torch.load(path, map_location="cpu", weights_only=True)
        seed = ckpt["values"].view(ckpt["shape"]).to(device)
        return cls(host, port, seed, **kw)


class SharedTable(_SharedBase):
    """Table-of-tensors sync with per-tensor scales (reference README.md:41).

    Shares a dict/list of named tensors as one engine instance; each packet
    carries one scale per member tensor, so small and large tensors converge
    at their own magnitudes.
    """

    def __init__(self, host: str, port: int,
                 tensors: Union[Dict[str, torch.Tensor], Sequence[torch.Tensor]],
                 **kw):
        if isinstance(tensors, dict):
            items = list(tensors.items())
        else:
            items = [(str(i), t) for i, t in enumerate(tensors)]
        if not items:
            raise ValueError("empty table")
        dev = items[0][1].device
        for k, t in items:
            if t.device != dev:
                raise ValueError("all table tensors must share a device")
            if t.dtype != torch.float32:
                raise TypeError(f"table tensor {k} must be float32")
        self.names = [k for k, _ in items]
        self.shapes = {k: tuple(t.shape) for k, t in items}
        sizes = [t.numel() for _, t in items]
        super().__init__(host, port, sizes, device=dev, **kw)
        self._offsets = {}
        off = 0
        for (k, t), s in zip(items, sizes):
            self._offsets[k] = (off, off + s)
            off += s
        self._start()
        if self.is_master:
            flat = torch.cat([t.detach().contiguous().view(-1) for _, t in items])
            self._add_flat(flat)

    def tensor_view(self, name: str) -> torch.Tensor:
        a, b = self._offsets[name]
        return self.values[a:b].view(self.shapes[name])

    def views(self) -> Dict[str, torch.Tensor]:
        return {k: self.tensor_view(k) for k in self.names}

    def add_from_tensors(self, tensors: Union[Dict[str, torch.Tensor], Sequence[torch.Tensor], torch.Tensor]):
        if isinstance(tensors, torch.Tensor):
            flat = tensors.detach().contiguous().view(-1)
        elif isinstance(tensors, dict):
            flat = torch.cat([tensors[k].detach().contiguous().view(-1) for k in self.names])
        else:
            flat = torch.cat([t.detach().contiguous().view(-1) for t in tensors])
        if flat.numel() != self.n:
            raise ValueError("size mismatch")
        self._add_flat(flat.float())

    def copy_to_tensors(self, out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        if out is None:
            out = {k: torch.empty(self.shapes[k], dtype=torch.float32,
                                  device=self.device) for k in self.names}
        for k in self.names:
            a, b = self._offsets[k]
            out[k].view(-1).copy_(self.values[a:b])
        return out

    @classmethod
    def from_module(cls, host: str, port: int, module: torch.nn.Module, **kw):
        params = {n: p.data for n, p in module.named_parameters()}
        return cls(host, port, params, **kw)


# public name for the flat multi-tensor-capable base (bench/paramsync use it
# directly when no shape semantics are needed)
SharedFlat = _SharedBase


def create_or_fetch(host: str, port: int, tensor: torch.Tensor, **kw) -> SharedTensor:
    """Reference entrypoint parity (sharedtensor.createOrFetch,
    sharedtensor.c:347-391)."""
    return SharedTensor(host, port, tensor, **kw)


createOrFetch = create_or_fetch
