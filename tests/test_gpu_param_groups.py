"""Parameter-group variants of the fused optimizer kernels (k_fused_*_grp)
through the raw bindings, and the param_groups option on the GPU.

Oracle: the ungrouped kernels, which test_gpu_optim_kernels.py and
test_gpu_grad_clip.py pin to derived bounds.  For each group g the
ungrouped kernel runs over the whole buffer from the same inputs with
lr_g = fl32(fl32(lr) * fl32(lr_scale[g])) and weight_decay[g]; the grouped
result must equal, bit for bit and in every buffer, the composition that
takes each segment's elements from its group's run.  Pointers are never
offset, so the pairing of bf16 residuals is the kernel's own.
"""
import functools

import numpy as np
import pytest
import torch

import kernel_bounds as kb
import sharedtensor_amd  # noqa: F401
from sharedtensor_amd import _core
from sharedtensor_amd.models.gpt2 import GPT2, GPT2Config
from sharedtensor_amd.parallel import no_decay_groups
from sharedtensor_amd.parallel.async_dp import AsyncDPTrainer
from sharedtensor_amd.utils import free_port
from test_gpu_codec_table import stream
from test_gpu_grad_clip import make_bufs, optim_dev, snapshot, tensors
from test_gpu_optim_kernels import (B1, B2, LR, MU, N_GRID, N_ODD,
                                    assert_all_updated, check_tail,
                                    gpu_bits_equal)

pytestmark = pytest.mark.gpu

F32 = np.float32
EPS = 1e-8
SIZES = [1, 63, 64, 65, 255, 257, 298]     # odd ends split bf16 pairs
PATTERN = [0, 1, 2, 1, 0, 2, 1]
SCALES = [1.0, 1.0, 0.25]
DECAYS = [0.01, 0.0, 0.1]
COEF = 0.37
KINDS = pytest.mark.parametrize(
    "kind,gdtype", [("adamw", torch.float32), ("adamw", torch.bfloat16),
                    ("sgd", torch.float32), ("sgd16", torch.bfloat16)],
    ids=["adamw32", "adamw16", "sgd", "sgd16"])
RES = pytest.mark.parametrize("bf16_res", [False, True], ids=["r32", "r16"])
CLIP = pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])


def make_table(n, sizes, pattern, scales, decays):
    assert sum(sizes) == n
    words = _core.build_group_table(n, list(np.cumsum(sizes)), list(pattern),
                                    list(scales), list(decays))
    return torch.tensor(words, dtype=torch.int32).cuda()


def clip_state(coef=COEF, skip=0):
    """A hand-built clip state (common.h ClipState)."""
    w = np.zeros(8, dtype=np.int32)
    w[0:2] = np.array([1.0], dtype=np.float64).view(np.int32)
    w[2:3] = np.array([1.0], dtype=F32).view(np.int32)
    w[3:4] = np.array([coef], dtype=F32).view(np.int32)
    w[4] = skip
    return torch.from_numpy(w).cuda()


def launch(kind, b, g, lr, wd, clip=None, table=None, step=3):
    n, bf16_res = b["n"], b["bf16_res"]
    dsts = [b["vals"].data_ptr()] + [d.data_ptr() for d in b["ds"]]
    cp = 0 if clip is None else clip.data_ptr()
    tp = 0 if table is None else table.data_ptr()
    if kind == "adamw":
        i1, i2 = kb.bias_corrections(B1, B2, step)
        _core.gpu_fused_adamw(
            b["m"].data_ptr(), b["v"].data_ptr(), g.data_ptr(),
            g.dtype == torch.bfloat16,
            0 if b["shadow"] is None else b["shadow"].data_ptr(), lr, B1, B2,
            EPS, wd, i1, i2, n, dsts, stream(), bf16_res, cp, tp)
    elif kind == "sgd":
        _core.gpu_fused_sgd(b["m"].data_ptr(), g.data_ptr(), lr, MU, n, dsts,
                            stream(), bf16_res, cp, tp)
    else:
        _core.gpu_fused_sgd_bf16(b["m"].data_ptr(), g.data_ptr(),
                                 b["shadow"].data_ptr(), lr, MU, n, dsts,
                                 stream(), bf16_res, cp, tp)
    torch.cuda.synchronize()
    for d in b["ds"]:
        check_tail(d, n)
    out = {"vals": b["vals"], "m": b["m"], "d": [d[:n] for d in b["ds"]],
           "shadow": b["shadow"]}
    if kind == "adamw":
        out["v"] = b["v"]
    return out


def group_of_element(n, sizes, pattern):
    seg = torch.repeat_interleave(torch.arange(len(sizes)),
                                  torch.tensor(sizes))
    assert seg.numel() == n
    return torch.tensor(pattern)[seg].cuda()


def check_composition(kind, gdtype, n, sizes, pattern, scales, decays,
                      bf16_res, clip, seed=31, fill_seed=None):
    """Grouped step == per-group ungrouped steps, composed; returns the
    grouped result."""
    w, m0, v0, g = optim_dev(n, seed)
    g = g.to(gdtype)
    shadow = kind != "sgd"
    state = clip_state() if clip else None
    if kind != "adamw":
        decays = [0.0] * len(scales)
    table = make_table(n, sizes, pattern, scales, decays)
    got = launch(kind, make_bufs(w, m0, v0, bf16_res, shadow, fill_seed), g,
                 LR, 123.0, state, table)
    elem_group = group_of_element(n, sizes, pattern)
    want = None
    for gi, (sc, wd) in enumerate(zip(scales, decays)):
        lr_g = float(F32(F32(LR) * F32(sc)))
        r = tensors(launch(kind,
                           make_bufs(w, m0, v0, bf16_res, shadow, fill_seed),
                           g, lr_g, wd, state))
        if want is None:
            want = {k: t.clone() for k, t in r.items()}
        else:
            mask = elem_group == gi
            for k, t in r.items():
                want[k][mask] = t[mask]
    have = tensors(got)
    assert set(have) == set(want)
    for k in want:
        gpu_bits_equal(have[k], want[k],
                       f"{kind} {k} bf16_res={bf16_res} clip={clip}")
    return got


@CLIP
@RES
@KINDS
def test_grouped_is_the_composition_of_ungrouped(kind, gdtype, bf16_res, clip):
    assert sum(SIZES) == N_ODD
    got = check_composition(kind, gdtype, N_ODD, SIZES, PATTERN, SCALES,
                            DECAYS, bf16_res, clip)
    assert int((got["d"][0] == 0).sum()) < 16


@RES
@KINDS
def test_composition_on_filled_residuals(kind, gdtype, bf16_res):
    """Residuals and shadow that already hold data: a bf16 pair split
    between two groups keeps its other half."""
    check_composition(kind, gdtype, N_ODD, SIZES, PATTERN, SCALES, DECAYS,
                      bf16_res, False, fill_seed=9)


@functools.lru_cache(maxsize=None)
def grid_layout():
    """Segment sizes over N_GRID: 1500 segments of 1 to 7 elements first (cut
    further where a boundary below falls inside one), boundaries at T-1, T,
    T+1 and 2T for the tile size T, one element either side of the point
    where the grid starts its second pass, at that point's next tile, and
    at n-1."""
    T, blocks = _core.GROUP_TILE, _core.GROUP_GRID_BLOCKS
    wrap = T * blocks
    assert T == 256 and wrap < N_GRID - T
    ends = set(np.cumsum([1 + i % 7 for i in range(1500)]).tolist())
    ends |= {T - 1, T, T + 1, 2 * T, wrap - 1, wrap + 1, wrap + T,
             N_GRID - 1, N_GRID}
    ends = sorted(ends)
    sizes = np.diff([0] + ends).tolist()
    assert min(sizes) >= 1 and len(sizes) <= _core.GROUP_MAX_SEGMENTS
    assert len(sizes) >= 1500 and max(sizes[:1500]) <= 7
    pattern = [i % 3 for i in range(len(sizes))]
    return sizes, pattern


@pytest.mark.parametrize("kind,gdtype,bf16_res,clip", [
    ("adamw", torch.bfloat16, True, False),
    ("adamw", torch.float32, False, True),
    ("sgd", torch.float32, True, True),
    ("sgd16", torch.bfloat16, False, False),
], ids=["adamw16-r16", "adamw32-r32-clip", "sgd-r16-clip", "sgd16-r32"])
def test_boundaries_against_the_launch_geometry(kind, gdtype, bf16_res, clip):
    sizes, pattern = grid_layout()
    got = check_composition(kind, gdtype, N_GRID, sizes, pattern,
                            [1.0, 0.5, 0.25], [0.01, 0.0, 0.1], bf16_res,
                            clip, seed=32)
    if not bf16_res:
        assert_all_updated(got["d"][0])
    else:
        u = got["d"][0].float()
        assert (u[_core.GROUP_GRID_BLOCKS * _core.GROUP_TILE:] != 0).all()
        assert int((u == 0).sum()) < 16


@RES
@KINDS
def test_one_group_of_scale_one_is_the_ungrouped_kernel(kind, gdtype,
                                                        bf16_res):
    w, m0, v0, g = optim_dev(N_ODD, 33)
    g = g.to(gdtype)
    wd = 0.01 if kind == "adamw" else 0.0
    table = make_table(N_ODD, [N_ODD], [0], [1.0], [wd])
    shadow = kind != "sgd"
    a = tensors(launch(kind, make_bufs(w, m0, v0, bf16_res, shadow), g, LR,
                       55.0, None, table))
    b = tensors(launch(kind, make_bufs(w, m0, v0, bf16_res, shadow), g, LR,
                       wd))
    for k in b:
        gpu_bits_equal(a[k], b[k], f"{kind} {k}")


@KINDS
def test_skip_touches_nothing(kind, gdtype):
    w, m0, v0, g = optim_dev(N_ODD, 34)
    g = g.to(gdtype)
    table = make_table(N_ODD, SIZES, PATTERN, SCALES,
                       DECAYS if kind == "adamw" else [0.0] * 3)
    for bf16_res in (False, True):
        b = make_bufs(w, m0, v0, bf16_res, kind != "sgd", fill_seed=3)
        snap = snapshot(b)
        launch(kind, b, g, LR, 0.0, clip_state(0.0, skip=1), table)
        for i, (x, s) in enumerate(zip(snapshot(b), snap)):
            gpu_bits_equal(x, s, f"{kind}: buffer {i} untouched")


@KINDS
def test_lr_scale_zero_freezes_weights_not_state(kind, gdtype):
    w, m0, v0, g = optim_dev(N_ODD, 35)
    g = g.to(gdtype)
    table = make_table(N_ODD, SIZES, PATTERN, [1.0, 0.0, 1.0],
                       DECAYS if kind == "adamw" else [0.0] * 3)
    frozen = group_of_element(N_ODD, SIZES, PATTERN) == 1
    for bf16_res in (False, True):
        b = make_bufs(w, m0, v0, bf16_res, kind != "sgd", fill_seed=4)
        before = [t.clone() for t in (b["vals"], *b["ds"])]
        r = launch(kind, b, g, LR, 0.0, None, table)
        n = w.numel()
        for x, s in zip((r["vals"], *r["d"]), before):
            assert (x[:n][frozen] == s[:n][frozen]).all()
            if x.dtype == torch.float32:     # a bf16 sum may absorb a small u
                assert (x[:n][~frozen] != s[:n][~frozen]).float().mean() > 0.9
        assert (r["m"] != m0).all()
        if kind == "adamw":
            assert (r["v"] != v0).all()


def test_five_steps_match_torch_adamw_param_groups():
    n = (1 << 20) + 3
    sizes = [3, 70001, 256 * 1000, 500001, n - 3 - 70001 - 256000 - 500001]
    pattern, scales, decays = [0, 1, 2, 0, 1], [1.0, 0.5, 2.0], [0.01, 0.0, 0.1]
    gen = torch.Generator().manual_seed(8)
    init = torch.randn(n, generator=gen).cuda()
    grads = [torch.randn(n, generator=gen).cuda() for _ in range(5)]
    ps = [torch.nn.Parameter(x.clone()) for x in init.split(sizes)]
    opt = torch.optim.AdamW(
        [{"params": [p for p, k in zip(ps, pattern) if k == gi],
          "lr": LR * scales[gi], "weight_decay": decays[gi]}
         for gi in range(3)], betas=(B1, B2), eps=EPS)
    for g in grads:
        for p, gp in zip(ps, g.split(sizes)):
            p.grad = gp.clone()
        opt.step()
    want = torch.cat([p.detach() for p in ps])

    table = make_table(n, sizes, pattern, scales, decays)
    b = make_bufs(init, torch.zeros_like(init), torch.zeros_like(init), False,
                  False)
    for step, g in enumerate(grads, start=1):
        launch("adamw", b, g, LR, 0.0, None, table, step=step)
    torch.testing.assert_close(b["vals"], want, rtol=1e-5, atol=1e-6)


def test_no_decay_groups_on_the_shadow_path():
    torch.cuda.set_device(0)
    torch.manual_seed(7)
    model = GPT2(GPT2Config.tiny()).to("cuda:0")
    lr, wd = 1e-2, 0.1
    tr = AsyncDPTrainer(model, port_base=free_port(), rank=0, world=1, lr=lr,
                        optimizer="adamw", weight_decay=wd,
                        amp_dtype=torch.bfloat16, param_dtype=torch.bfloat16,
                        param_groups=no_decay_groups(model, wd))
    try:
        sh = tr.shared
        before = sh.values.clone().cpu().numpy()
        sh.grad_flat.zero_()
        tr.opt.step()
        torch.cuda.synchronize()
        after = sh.values.cpu().numpy()
        off, small, big = 0, 0, 0
        for p in sh.params:
            a, b = before[off:off + p.numel()], after[off:off + p.numel()]
            off += p.numel()
            if p.ndim < 2:
                small += 1
                assert a.tobytes() == b.tobytes()
            else:
                big += 1
                want = a + -F32(lr) * (F32(0) + F32(wd) * a)
                assert want.dtype == F32
                np.testing.assert_array_equal(b, want)
                assert (a != b).any()
        assert small > 0 and big > 0 and off == sh.n
        gpu_bits_equal(sh.shadow, sh.values.to(torch.bfloat16),
                       "shadow == bf16(values)")
    finally:
        tr.close()
