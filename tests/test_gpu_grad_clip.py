"""Global-norm gradient clipping kernels through the raw bindings:
k_grad_sumsq / k_grad_clip_finalize (gpu_grad_clip_coef) and the clip_state
argument of the three fused optimizer kernels.

Bounds.  sumsq: squares of fp32 or bf16 values are exact in fp64 and all
terms are non-negative, so every summation order of n terms stays within
n * 2^-53 * ref of the exact sum ref (math.fsum of the exact squares).
norm and coef: one fp32 rounding of a value recomputed in fp64 from the
device's own sumsq, so 1 fp32 ulp.  A clipped step uses fl32(g * coef),
rounded once, wherever the unclipped step uses g, so it equals the
unclipped kernel on gradients scaled beforehand bit for bit.

Gradient buffers are surrounded by NaN, so a read outside [0, n) shows as a
non-finite sum.
"""
import functools
import math

import numpy as np
import pytest
import torch

import kernel_bounds as kb
import sharedtensor_amd  # noqa: F401
from sharedtensor_amd import _core
from test_gpu_codec_table import stream
from test_gpu_optim_kernels import (B1, B2, LR, MU, N_GRID, N_ODD,
                                    assert_all_updated, check_invariants,
                                    check_tail, gpu_bits_equal, res_buf)

pytestmark = pytest.mark.gpu

NS = [1, 7, 1003, N_GRID]
EPS, WD = 1e-8, 0.01
FLT_MAX = float(np.finfo(np.float32).max)
DTYPES = pytest.mark.parametrize("gdtype", [torch.float32, torch.bfloat16],
                                 ids=["g32", "g16"])
OFFSETS = pytest.mark.parametrize("off", [0, 1], ids=["aligned", "off1"])


# ------------------------------------------------------------------ helpers

@functools.lru_cache(maxsize=None)
def scratch():
    assert _core.GRAD_CLIP_MAX_BLOCKS == 2048
    return torch.empty(2048, dtype=torch.float64, device="cuda")


def new_state():
    return torch.zeros(8, dtype=torch.int32, device="cuda")


def place(g, off):
    """g on the device at element offset `off` of a NaN-filled buffer."""
    n = g.numel()
    buf = torch.full((n + off + 16,), float("nan"), dtype=g.dtype,
                     device="cuda")
    view = buf[off:off + n]
    view.copy_(g)
    assert view.data_ptr() == buf.data_ptr() + off * g.element_size()
    return view


def clip_coef(g, max_norm, state=None):
    """Runs the reduction on the device tensor g; returns (state, decoded)."""
    state = new_state() if state is None else state
    bf16 = g.dtype == torch.bfloat16
    _core.gpu_grad_clip_coef(0 if bf16 else g.data_ptr(),
                             g.data_ptr() if bf16 else 0, g.numel(),
                             max_norm, scratch().data_ptr(), state.data_ptr(),
                             stream())
    torch.cuda.synchronize()
    return state, decode(state)


def decode(state):
    w = state.cpu().numpy().copy()
    return {"sumsq": float(w[0:2].view(np.float64)[0]),
            "norm": w[2:3].view(np.float32)[0],
            "coef": w[3:4].view(np.float32)[0],
            "skip": int(w[4:5].view(np.uint32)[0]),
            "skipped_total": int(w[5:6].view(np.uint32)[0]),
            "pad": (int(w[6]), int(w[7]))}


def within_ulp32(got, ref):
    """fp32 `got` against the fp64 value `ref` it should be the rounding of."""
    if ref > FLT_MAX:
        return got == np.float32("inf")
    return abs(float(got) - ref) <= float(np.spacing(np.float32(ref)))


def check_norm_coef(st, max_norm):
    nrm = math.sqrt(st["sumsq"])
    assert within_ulp32(st["norm"], nrm), (st["norm"], nrm)
    coef = min(1.0, max_norm / (nrm + 1e-6))
    assert within_ulp32(st["coef"], coef), (st["coef"], coef)
    if max_norm >= nrm + 1e-6:
        assert st["coef"] == np.float32(1.0)
    assert st["pad"] == (0, 0)


@functools.lru_cache(maxsize=None)
def family_grad(family, n, bf16):
    """The family's gradient in its dtype (CPU) and the exact sum of its
    squares, computed once per (family, n, dtype)."""
    g = kb.optim_inputs(family, n)[3]
    if bf16:
        g = g.to(torch.bfloat16)
    gd = g.double()
    return g, math.fsum((gd * gd).tolist())


# ------------------------------------------------------------ norm and state

@OFFSETS
@DTYPES
@pytest.mark.parametrize("n", NS)
def test_every_element_counted_once(n, gdtype, off):
    ones = place(torch.ones(n, dtype=gdtype, device="cuda"), off)
    _, st = clip_coef(ones, 1.0)
    assert st["sumsq"] == float(n) and st["skip"] == 0
    check_norm_coef(st, 1.0)

    pos = sorted({p for p in (0, 1, 7, 8, 255, 256, n - 2, n - 1)
                  if 0 <= p < n})
    g = torch.zeros(n, dtype=gdtype, device="cuda")
    g[pos] = 1.0
    _, st = clip_coef(place(g, off), 1.0)
    assert st["sumsq"] == float(len(pos)) and st["skip"] == 0


@OFFSETS
@DTYPES
@pytest.mark.parametrize("family", ["randn", "g_huge"])
@pytest.mark.parametrize("n", NS)
def test_sumsq_accuracy_state_and_reproducibility(n, family, gdtype, off):
    g_cpu, ref = family_grad(family, n, gdtype == torch.bfloat16)
    g = place(g_cpu, off)
    max_norm = math.sqrt(ref) / 8                 # clipped: coef near 1/8
    state, st = clip_coef(g, max_norm)
    print(f"sumsq n={n} {family} {gdtype} off={off}: got {st['sumsq']!r} "
          f"ref {ref!r} rel {abs(st['sumsq'] - ref) / ref:.3g} "
          f"bound {n * 2.0 ** -53:.3g}")
    assert math.isfinite(st["sumsq"]) and st["skip"] == 0
    assert st["skipped_total"] == 0
    assert abs(st["sumsq"] - ref) <= n * 2.0 ** -53 * ref
    check_norm_coef(st, max_norm)
    assert st["coef"] < 1
    # run to run: the same bits
    state2, _ = clip_coef(g, max_norm)
    assert torch.equal(state, state2)
    # the clamp: exactly 1 from max_norm = norm + 1e-6 upwards
    for c in (2 * math.sqrt(ref), math.sqrt(st["sumsq"]) + 1e-6):
        if math.isfinite(c):
            _, st1 = clip_coef(g, c)
            check_norm_coef(st1, c)
            assert st1["coef"] == np.float32(1.0)


@DTYPES
def test_norm_beyond_fp32_is_no_skip(gdtype):
    """Finite gradients whose norm overflows fp32: sumsq is finite in fp64,
    the step is not skipped and coef is the rounding of the fp64 quotient."""
    g = torch.full((7,), 3e38, dtype=gdtype)
    g[1::2] *= -1
    gd = g.double()
    ref = math.fsum((gd * gd).tolist())
    _, st = clip_coef(place(g, 0), 1e3)
    assert st["sumsq"] == ref            # 7 equal terms: every sum is exact
    assert st["norm"] == np.float32("inf") and st["skip"] == 0
    check_norm_coef(st, 1e3)
    assert 1e-37 < st["coef"] < 1e-35    # a normal fp32 number


@pytest.mark.parametrize("bad", [0.0, -1.0, float("inf"), float("nan")])
def test_bad_max_norm_raises_before_any_launch(bad):
    g = torch.ones(8, device="cuda")
    state = new_state()
    with pytest.raises(ValueError):
        _core.gpu_grad_clip_coef(g.data_ptr(), 0, 8, bad,
                                 scratch().data_ptr(), state.data_ptr(),
                                 stream())
    torch.cuda.synchronize()
    assert (state == 0).all()


# ---------------------------------------------------------- fused optimizers

@functools.lru_cache(maxsize=None)
def optim_dev(n, seed):
    w, m0, v0, g, _ = kb.optim_inputs("randn", n, seed=seed)
    return w.cuda(), m0.cuda(), v0.cuda(), g.cuda()


def make_bufs(w, m0, v0, bf16_res, shadow, fill_seed=None):
    """Fresh state for one step.  fill_seed: residuals and shadow hold
    random data instead of zeros."""
    n = w.numel()
    ds = [res_buf(n, bf16_res) for _ in range(3)]
    sh = torch.zeros(n, dtype=torch.bfloat16, device="cuda") if shadow else None
    if fill_seed is not None:
        gen = torch.Generator(device="cuda").manual_seed(fill_seed)
        for d in ds:
            d[:n] = torch.randn(n, generator=gen, device="cuda").to(d.dtype)
        if shadow:
            sh.copy_(torch.randn(n, generator=gen, device="cuda"))
    return {"vals": w.clone(), "m": m0.clone(), "v": v0.clone(), "ds": ds,
            "shadow": sh, "n": n, "bf16_res": bf16_res}


def launch(kind, b, g, clip=None, step=3):
    """kind: adamw (fp32 or bf16 g), sgd (fp32 g), sgd16 (bf16 g)."""
    n, bf16_res = b["n"], b["bf16_res"]
    dsts = [b["vals"].data_ptr()] + [d.data_ptr() for d in b["ds"]]
    kw = {} if clip is None else {"clip_state": clip.data_ptr()}
    if kind == "adamw":
        i1, i2 = kb.bias_corrections(B1, B2, step)
        _core.gpu_fused_adamw(
            b["m"].data_ptr(), b["v"].data_ptr(), g.data_ptr(),
            g.dtype == torch.bfloat16,
            0 if b["shadow"] is None else b["shadow"].data_ptr(), LR, B1, B2,
            EPS, WD, i1, i2, n, dsts, stream(), bf16_res, **kw)
    elif kind == "sgd":
        assert g.dtype == torch.float32
        _core.gpu_fused_sgd(b["m"].data_ptr(), g.data_ptr(), LR, MU, n, dsts,
                            stream(), bf16_res, **kw)
    else:
        assert g.dtype == torch.bfloat16
        _core.gpu_fused_sgd_bf16(b["m"].data_ptr(), g.data_ptr(),
                                 b["shadow"].data_ptr(), LR, MU, n, dsts,
                                 stream(), bf16_res, **kw)
    torch.cuda.synchronize()
    for d in b["ds"]:
        check_tail(d, n)
    out = {"vals": b["vals"], "m": b["m"], "d": [d[:n] for d in b["ds"]],
           "shadow": b["shadow"]}
    if kind == "adamw":
        out["v"] = b["v"]
    return out


def tensors(r):
    t = {"vals": r["vals"], "m": r["m"], "d1": r["d"][0], "d2": r["d"][1],
         "d3": r["d"][2]}
    if "v" in r:
        t["v"] = r["v"]
    if r["shadow"] is not None:
        t["shadow"] = r["shadow"]
    return t


def snapshot(b):
    return [t.clone() for t in (b["vals"], b["m"], b["v"], *b["ds"])
            ] + ([] if b["shadow"] is None else [b["shadow"].clone()])


def assert_unchanged(b, snap, what):
    for i, (a, s) in enumerate(zip(snapshot(b), snap)):
        gpu_bits_equal(a, s, f"{what}: buffer {i} untouched")


def clipped_equals_prescaled(kind, n, gdtype, step=3, shadow=True):
    w, m0, v0, g = optim_dev(n, 21)
    g = g.to(gdtype)
    max_norm = 0.1 * math.sqrt(n)              # |g| ~ sqrt(n): coef ~ 0.1
    state, st = clip_coef(g, max_norm)
    assert st["skip"] == 0 and 0.01 <= st["coef"] <= 0.5
    coef_dev = state[3:4].view(torch.float32)  # the device's own coef
    g_pre = g.float() * coef_dev               # fp32, one rounding
    assert g_pre.dtype == torch.float32
    ref_kind = "sgd" if kind == "sgd16" else kind
    ref_shadow = shadow and kind == "adamw"
    got, ref = {}, {}
    for bf16_res in (False, True):
        got[bf16_res] = launch(kind, make_bufs(w, m0, v0, bf16_res, shadow),
                               g, clip=state, step=step)
        ref[bf16_res] = launch(ref_kind,
                               make_bufs(w, m0, v0, bf16_res, ref_shadow),
                               g_pre, step=step)
        a, b = tensors(got[bf16_res]), tensors(ref[bf16_res])
        for k in b:
            gpu_bits_equal(a[k], b[k], f"{kind} {k} bf16_res={bf16_res}")
        if kind == "sgd16":
            gpu_bits_equal(a["shadow"], b["vals"].to(torch.bfloat16),
                           "sgd16 shadow == bf16(values of k_fused_sgd)")
    check_invariants(w, got[False], got[True],
                     has_shadow=shadow and kind != "sgd")
    if n == N_GRID:
        assert_all_updated(got[False]["d"][0])
    else:
        assert int((got[False]["d"][0] == 0).sum()) < 16
    # not the unclipped step
    plain = launch(kind, make_bufs(w, m0, v0, False, shadow), g, step=step)
    assert (plain["m"] != got[False]["m"]).float().mean() > 0.99


@DTYPES
@pytest.mark.parametrize("shadow", [True, False], ids=["shadow", "noshadow"])
@pytest.mark.parametrize("step", [1, 3])
def test_adamw_clipped_is_unclipped_on_prescaled(step, shadow, gdtype):
    clipped_equals_prescaled("adamw", N_ODD, gdtype, step=step, shadow=shadow)


@pytest.mark.parametrize("kind,gdtype", [("sgd", torch.float32),
                                         ("sgd16", torch.bfloat16)],
                         ids=["sgd", "sgd16"])
@pytest.mark.parametrize("n", [N_ODD, N_GRID])
def test_sgd_clipped_is_unclipped_on_prescaled(n, kind, gdtype):
    clipped_equals_prescaled(kind, n, gdtype)


@DTYPES
def test_adamw_clipped_grid_stride(gdtype):
    clipped_equals_prescaled("adamw", N_GRID, gdtype)


@pytest.mark.parametrize("kind,gdtype", [("adamw", torch.float32),
                                         ("adamw", torch.bfloat16),
                                         ("sgd", torch.float32),
                                         ("sgd16", torch.bfloat16)],
                         ids=["adamw32", "adamw16", "sgd", "sgd16"])
def test_coef_one_is_a_no_op(kind, gdtype):
    w, m0, v0, g = optim_dev(N_ODD, 22)
    g = g.to(gdtype)
    state, st = clip_coef(g, 1e6)
    assert st["coef"] == np.float32(1.0) and st["skip"] == 0
    for bf16_res in (False, True):
        a = tensors(launch(kind, make_bufs(w, m0, v0, bf16_res, True), g,
                           clip=state))
        b = tensors(launch(kind, make_bufs(w, m0, v0, bf16_res, True), g))
        for k in b:
            gpu_bits_equal(a[k], b[k], f"{kind} {k} bf16_res={bf16_res}")


@pytest.mark.parametrize("bf16_res", [False, True], ids=["r32", "r16"])
@pytest.mark.parametrize("bad,at", [(float("inf"), N_ODD - 1),
                                    (float("nan"), 0)], ids=["inf", "nan"])
@DTYPES
def test_non_finite_gradient_skips_the_step(gdtype, bad, at, bf16_res):
    """The kernels return before touching anything; nothing faults."""
    n = N_ODD
    w, m0, v0, g = optim_dev(n, 23)
    g = g.to(gdtype)
    g_bad = g.clone()
    g_bad[at] = bad
    kinds = ["adamw", "sgd" if gdtype == torch.float32 else "sgd16"]
    state = new_state()
    _, st = clip_coef(g_bad, 1.0, state)
    assert st["skip"] == 1 and st["coef"] == 0 and st["skipped_total"] == 1
    assert not math.isfinite(st["sumsq"])
    bufs = {k: make_bufs(w, m0, v0, bf16_res, True, fill_seed=5) for k in kinds}
    snaps = {k: snapshot(bufs[k]) for k in kinds}
    for k in kinds:
        launch(k, bufs[k], g_bad, clip=state)
        assert_unchanged(bufs[k], snaps[k], k)
    # a second bad step counts, and still touches nothing
    _, st = clip_coef(g_bad, 1.0, state)
    assert st["skip"] == 1 and st["skipped_total"] == 2
    for k in kinds:
        launch(k, bufs[k], g_bad, clip=state)
        assert_unchanged(bufs[k], snaps[k], k)
    # a finite step runs, and the count stays
    _, st = clip_coef(g, 1.0, state)
    assert st["skip"] == 0 and st["skipped_total"] == 2 and 0 < st["coef"] < 1
    for k in kinds:
        launch(k, bufs[k], g, clip=state)
        after = snapshot(bufs[k])
        for i, (a, s) in enumerate(zip(after, snaps[k])):
            if k != "adamw" and i == 2:
                continue                       # SGD has no second moment
            if k == "sgd" and i == 6:
                continue                       # nor, with fp32 gradients, a shadow
            same = (a.view(torch.int16 if a.dtype == torch.bfloat16
                           else torch.int32)
                    == s.view(torch.int16 if s.dtype == torch.bfloat16
                              else torch.int32))
            if a.dtype == torch.bfloat16:
                # a bf16 residual or shadow of magnitude ~1 can absorb a
                # small update: most, not all, elements move
                assert same[:n].float().mean() < 0.9, (k, i)
            else:
                assert same.float().mean() < 0.01, (k, i)
