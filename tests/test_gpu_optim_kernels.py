"""Fused optimizer kernels (AdamW, SGD momentum, SGD with bf16 gradients)
and the snapshot / delta-scatter kernels, through the raw bindings.

Two kinds of check.  Exact invariants: the update u is staged identically
into every link residual, the replica moves by exactly u, the bf16 shadow
is exactly the rounding of the replica, bf16 residuals hold exactly the
rounding of u, and the optimizer state does not depend on the residual
type.  And a derived bound: m, v and u against the fp64 single-step
reference of kernel_bounds.py, within the running-error bound of the
kernel's fp32 operation chain (validated on the CPU by
test_kernel_bounds_cpu.py; never widened to make the GPU pass).
"""
import numpy as np
import pytest
import torch

import codec_reference as cr
import kernel_bounds as kb
import sharedtensor_amd  # noqa: F401
from sharedtensor_amd import _core
from test_gpu_codec_table import assert_bits_equal, stream

pytestmark = pytest.mark.gpu

N_ODD = 1003                       # the last bf16 pair is split
N_GRID = 8_388_608 + 64 * 5 + 17   # past the 32768 x 256 grid cap
LR, B1, B2, MU = 2e-2, 0.9, 0.95, 0.9
SENT = 0x4049


def res_buf(n, bf16):
    """Zeroed residual buffer; bf16: even length with sentinels past n."""
    if not bf16:
        return torch.zeros(n, device="cuda")
    total = n + 1 + (n + 1) % 2
    b = torch.zeros(total, dtype=torch.int16, device="cuda")
    b[n:] = SENT
    return b.view(torch.bfloat16)


def check_tail(b, n):
    if b.dtype == torch.bfloat16:
        assert (b.view(torch.int16)[n:] == SENT).all()


def gpu_bits_equal(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    view = torch.int16 if a.dtype == torch.bfloat16 else torch.int32
    bad = a.contiguous().view(view) != b.contiguous().view(view)
    if bad.any():
        i = int(bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {a.numel()} differ; "
                             f"first at {i}: {float(a[i])!r} vs {float(b[i])!r}")


def assert_all_updated(u):
    """The invariants alone would accept a kernel that skips elements (u = 0
    there and the replica unchanged): the elements of the second grid-stride
    iteration all moved, and an exactly zero update stays a rare accident."""
    assert (u[32768 * 256:] != 0).all()
    assert int((u == 0).sum()) < 16


def run_adamw(w, m0, v0, g, eps, wd, step, bf16_res, with_shadow=True):
    n = w.numel()
    vals, mom, vel = w.clone().cuda(), m0.clone().cuda(), v0.clone().cuda()
    grad = g.cuda()
    ds = [res_buf(n, bf16_res) for _ in range(3)]
    shadow = (torch.zeros(n, dtype=torch.bfloat16, device="cuda")
              if with_shadow else None)
    i1, i2 = kb.bias_corrections(B1, B2, step)
    _core.gpu_fused_adamw(mom.data_ptr(), vel.data_ptr(), grad.data_ptr(),
                          grad.dtype == torch.bfloat16,
                          shadow.data_ptr() if with_shadow else 0, LR, B1, B2,
                          eps, wd, i1, i2, n,
                          [vals.data_ptr()] + [d.data_ptr() for d in ds],
                          stream(), bf16_res)
    torch.cuda.synchronize()
    for d in ds:
        check_tail(d, n)
    return {"vals": vals, "m": mom, "v": vel, "d": [d[:n] for d in ds],
            "shadow": shadow, "ibc": (i1, i2)}


def check_invariants(before_vals, r32, r16, has_shadow=True):
    """r32 / r16: the same step with fp32 and with bf16 residuals."""
    d1, d2, d3 = r32["d"]
    gpu_bits_equal(d1, d2, "d1 == d2")
    gpu_bits_equal(d1, d3, "d1 == d3")
    gpu_bits_equal(r32["vals"], before_vals + d1, "values == fl32(before + u)")
    if has_shadow:
        gpu_bits_equal(r32["shadow"], r32["vals"].to(torch.bfloat16),
                       "shadow == bf16(values)")
        gpu_bits_equal(r16["shadow"], r32["shadow"], "shadow across residual types")
    for d in r16["d"]:
        gpu_bits_equal(d, d1.to(torch.bfloat16), "bf16 residual == bf16(u)")
    gpu_bits_equal(r16["m"], r32["m"], "mom across residual types")
    gpu_bits_equal(r16["vals"], r32["vals"], "values across residual types")
    if "v" in r32:
        gpu_bits_equal(r16["v"], r32["v"], "vel across residual types")


@pytest.mark.parametrize("gdtype", [torch.float32, torch.bfloat16],
                         ids=["g32", "g16"])
@pytest.mark.parametrize("n", [N_ODD, N_GRID])
def test_adamw_exact_invariants(n, gdtype):
    w, m0, v0, g, wd = kb.optim_inputs("randn", n, seed=1)
    g = g.to(gdtype)
    r32 = run_adamw(w, m0, v0, g, 1e-8, wd, 3, False)
    r16 = run_adamw(w, m0, v0, g, 1e-8, wd, 3, True)
    check_invariants(w.cuda(), r32, r16)
    assert_all_updated(r32["d"][0])


def check_adamw_bound(w, m0, v0, g, eps, wd, step, family):
    r = run_adamw(w, m0, v0, g, eps, wd, step, False)
    i1, i2 = r["ibc"]
    args = (w, m0, v0, g.float(), LR, B1, B2, eps, wd, i1, i2)
    ref = kb.adamw_formula(*args)
    slack = kb.adamw_slack(*args)
    got = {"m": r["m"].cpu(), "v": r["v"].cpu(), "u": r["d"][0].cpu()}
    fin = torch.isfinite(g.float())
    for k in ("m", "v", "u"):
        assert not torch.isfinite(got[k][~fin]).any(), k
        assert not torch.isfinite(ref[k][~fin]).any(), k
        kb.assert_within(got[k][fin], ref[k][fin], slack[k][fin], "adamw", k,
                         family)
    return got, ref


@pytest.mark.parametrize("step", [1, 10000])
@pytest.mark.parametrize("eps", [1e-8, 1e-6])
@pytest.mark.parametrize("family", kb.OPTIM_FAMILIES)
def test_adamw_within_derived_bound(family, eps, step):
    w, m0, v0, g, wd = kb.optim_inputs(family, N_ODD)
    got, ref = check_adamw_bound(w, m0, v0, g, eps, wd, step,
                                 f"{family}/eps={eps:g}/step={step}")
    if family == "zero_g_zero_state":
        # m = v = 0: the Adam quotient is 0 / eps and u = -lr * (wd * w),
        # decay against the weight before the update
        f = np.float32
        want = -f(LR) * (f(wd) * w.numpy())
        assert want.dtype == np.float32
        np.testing.assert_array_equal(got["u"].numpy(), want)
        assert (got["m"] == 0).all() and (got["v"] == 0).all()
    if family == "g_huge":
        assert torch.isinf(got["v"]).all() and torch.isfinite(got["u"]).all()


@pytest.mark.parametrize("step", [1, 10000])
def test_adamw_every_bf16_gradient(step):
    g = kb.all_bf16()
    n = g.numel()
    w, m0, v0, _, wd = kb.optim_inputs("randn", n, seed=2)
    check_adamw_bound(w, m0, v0, g, 1e-8, wd, step, f"all-bf16/step={step}")


# --------------------------------------------------------------------- SGD

def run_sgd(w, m0, g, bf16_res):
    n = w.numel()
    vals, mom, grad = w.clone().cuda(), m0.clone().cuda(), g.cuda()
    ds = [res_buf(n, bf16_res) for _ in range(3)]
    out = {"vals": vals, "m": mom, "d": [d[:n] for d in ds], "shadow": None}
    dsts = [vals.data_ptr()] + [d.data_ptr() for d in ds]
    if g.dtype == torch.bfloat16:
        out["shadow"] = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
        _core.gpu_fused_sgd_bf16(mom.data_ptr(), grad.data_ptr(),
                                 out["shadow"].data_ptr(), LR, MU, n, dsts,
                                 stream(), bf16_res)
    else:
        _core.gpu_fused_sgd(mom.data_ptr(), grad.data_ptr(), LR, MU, n, dsts,
                            stream(), bf16_res)
    torch.cuda.synchronize()
    for d in ds:
        check_tail(d, n)
    return out


def check_sgd_bound(r, m0, g, family):
    ref = kb.sgd_formula(m0, g.float(), LR, MU)
    slack = kb.sgd_slack(m0, g.float(), LR, MU)
    fin = torch.isfinite(g.float())
    for k, got in (("m", r["m"].cpu()), ("u", r["d"][0].cpu())):
        assert not torch.isfinite(got[~fin]).any(), k
        kb.assert_within(got[fin], ref[k][fin], slack[k][fin], "sgd", k, family)


@pytest.mark.parametrize("gdtype", [torch.float32, torch.bfloat16],
                         ids=["g32", "g16"])
@pytest.mark.parametrize("n", [N_ODD, N_GRID])
def test_sgd_invariants_and_bound(n, gdtype):
    w, m0, _, g, _ = kb.optim_inputs("randn", n, seed=3)
    g = g.to(gdtype)
    r32 = run_sgd(w, m0, g, False)
    r16 = run_sgd(w, m0, g, True)
    check_invariants(w.cuda(), r32, r16, has_shadow=gdtype == torch.bfloat16)
    assert_all_updated(r32["d"][0])
    check_sgd_bound(r32, m0, g, f"randn/n={n}/{gdtype}")


def test_sgd_bf16_every_gradient():
    g = kb.all_bf16()
    w, m0, _, _, _ = kb.optim_inputs("randn", g.numel(), seed=4)
    r = run_sgd(w, m0, g, False)
    check_sgd_bound(r, m0, g, "all-bf16")
    fin = torch.isfinite(g.float()).cuda()
    gpu_bits_equal(r["shadow"][fin], r["vals"].to(torch.bfloat16)[fin],
                   "shadow == bf16(values)")


# ------------------------------------------------- snapshot / delta scatter

def _with_zeros(x):
    x = x.clone()
    x[::5] = 0.0
    x[2::10] = -0.0
    return x


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("n", [N_ODD, N_GRID])
def test_snapshot_capture(n, bf16):
    gen = torch.Generator().manual_seed(50 + bf16)
    values = _with_zeros(torch.randn(n, generator=gen)).cuda()
    delta0 = torch.randn(n, generator=gen)
    delta0[::15] = -0.0                       # a -0.0 residual under values == 0
    delta0[7::30] = -0.0                      # and one under values != 0
    dt = torch.bfloat16 if bf16 else torch.float32
    delta = res_buf(n, bf16)
    delta[:n] = delta0.to(dt)
    before = delta[:n].clone()
    out = torch.full((n,), 7.0, device="cuda")
    values0 = values.clone()
    _core.gpu_snapshot_capture(values.data_ptr(), delta.data_ptr(),
                               out.data_ptr(), n, stream(), bf16)
    torch.cuda.synchronize()
    gpu_bits_equal(out, values0, "out == values")
    gpu_bits_equal(values, values0, "values unchanged")
    # fp32: one rounding of before - v.  bf16: the packed atomic adds
    # bf16(-v) and rounds the exact sum once; the fp32 sum of two bf16
    # numbers is exact, or so close to the larger one that its bf16 rounding
    # is the same
    want = (before.float() + (-values0).to(dt).float()).to(dt)
    zero = values0 == 0
    want[zero] = before[zero]                 # untouched, -0.0 included
    gpu_bits_equal(delta[:n], want, "delta -= values")
    assert (delta[:n][zero].view(torch.int16 if bf16 else torch.int32)
            == before[zero].view(torch.int16 if bf16 else torch.int32)).all()
    check_tail(delta, n)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("n,ndst", [(N_ODD, 1), (N_ODD, 2), (N_ODD, 3),
                                    (N_GRID, 3)])
def test_add_delta_scatter(n, ndst, bf16):
    gen = torch.Generator().manual_seed(60 + ndst)
    dt = torch.bfloat16 if bf16 else torch.float32
    src0 = _with_zeros(torch.randn(n, generator=gen)).to(dt)
    src = res_buf(n, bf16)
    src[:n] = src0.cuda()
    vals0 = torch.randn(n, generator=gen)
    vals0[::10] = -0.0                        # under a zero source: skipped
    vals = vals0.clone().cuda()
    fwd = [res_buf(n, bf16) for _ in range(ndst - 1)]
    _core.gpu_add_delta_scatter(src.data_ptr(), n,
                                [vals.data_ptr()] + [f.data_ptr() for f in fwd],
                                stream(), bf16)
    torch.cuda.synchronize()
    s32 = src0.float().cuda()
    want = vals0.cuda() + s32
    want[s32 == 0] = vals0.cuda()[s32 == 0]
    gpu_bits_equal(vals, want, "values += src")
    gpu_bits_equal(src[:n], src0.cuda(), "source unchanged")
    for f in fwd:
        # zeroed destination: exactly the source where it is non-zero
        wantf = src0.cuda().clone()
        wantf[s32 == 0] = 0.0
        gpu_bits_equal(f[:n], wantf, "forward += src")
        check_tail(f, n)
    check_tail(src, n)
