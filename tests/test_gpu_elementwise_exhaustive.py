"""GELU and SwiGLU kernels over every bf16 bit pattern, at the sizes where
their grid-stride loop starts to iterate, on empty and on misaligned inputs,
against the fp64 reference and derived bounds of tests/kernel_bounds.py."""
import pytest
import torch

import kernel_bounds as kb
from sharedtensor_amd import _core
from sharedtensor_amd.ops import fused_gelu, fused_swiglu

pytestmark = pytest.mark.gpu

# 16384 blocks x 256 threads x 8 bf16: what one sweep of the loop covers
SWEEP = 16384 * 256 * 8
SIZES = [8, 8 * 255, 8 * 257, SWEEP + 8, 2 * SWEEP + 8 * 257]
SLICE = 1 << 22
SWIGLU_X3 = [1.0, -1.5, 2.0 ** -100, 3e38, 0.0]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dy(kind, n):
    if kind == "ones":
        return torch.ones(n, device="cuda", dtype=torch.bfloat16)
    return kb.dy_pattern(n, device="cuda")


def run_gelu(x, dy):
    xf = x.clone().requires_grad_(True)
    y = fused_gelu.fused_gelu(xf)
    y.backward(dy)
    torch.cuda.synchronize()
    return {"y": y.detach(), "dx": xf.grad}


def run_swiglu(x1, x3, dy):
    a = x1.clone().requires_grad_(True)
    b = x3.clone().requires_grad_(True)
    y = fused_swiglu.fused_swiglu(a, b)
    y.backward(dy)
    torch.cuda.synchronize()
    return {"y": y.detach(), "dx1": a.grad, "dx3": b.grad}


@pytest.mark.parametrize("dy_kind", ["ones", "pattern"])
def test_gelu_every_bf16(dy_kind):
    x = kb.all_bf16("cuda")
    dy = _dy(dy_kind, x.numel())
    got = run_gelu(x, dy)
    ref = kb.gelu_formula(x, dy)
    slack = kb.gelu_slack(x, dy)
    nan_x = torch.isnan(x)
    finite_x = torch.isfinite(x)
    assert torch.isnan(got["y"][nan_x]).all()
    assert torch.isnan(got["dx"][nan_x]).all()
    # every finite x has a finite reference, so the bound below judges it
    assert torch.isfinite(ref["dx"][finite_x]).all()
    assert torch.isfinite(ref["y"][finite_x]).all()
    bad = finite_x & ~torch.isfinite(got["dx"].float())
    assert not bad.any(), (
        f"dx not finite at {int(bad.sum())} finite x, first x = "
        f"{float(x[bad][0])!r}")
    for k in ("y", "dx"):
        kb.assert_bf16(got[k], ref[k], slack[k], "gelu", k,
                       "all-bf16/dy=" + dy_kind)


@pytest.mark.parametrize("x3v", SWIGLU_X3)
@pytest.mark.parametrize("dy_kind", ["ones", "pattern"])
def test_swiglu_every_bf16_x1(dy_kind, x3v):
    x1 = kb.all_bf16("cuda")
    x3 = torch.full_like(x1, x3v)
    dy = _dy(dy_kind, x1.numel())
    got = run_swiglu(x1, x3, dy)
    ref = kb.swiglu_formula(x1, x3, dy)
    slack = kb.swiglu_slack(x1, x3, dy)
    nan_x = torch.isnan(x1)
    for k in ("y", "dx1", "dx3"):
        assert torch.isnan(got[k][nan_x]).all(), k
        kb.assert_bf16(got[k], ref[k], slack[k], "swiglu", k,
                       f"all-bf16/x3={x3v:g}/dy={dy_kind}")


def test_swiglu_exp_saturation():
    """|x1| up to 100: exp(-x1) leaves the fp32 range on both sides."""
    g = torch.Generator(device="cuda").manual_seed(5)
    n = 1 << 16
    x1 = (torch.rand(n, device="cuda", generator=g) * 200 - 100).to(
        torch.bfloat16)
    x3 = torch.randn(n, device="cuda", generator=g).to(torch.bfloat16)
    dy = torch.randn(n, device="cuda", generator=g).to(torch.bfloat16)
    got = run_swiglu(x1, x3, dy)
    ref = kb.swiglu_formula(x1, x3, dy)
    slack = kb.swiglu_slack(x1, x3, dy)
    for k in ("y", "dx1", "dx3"):
        assert torch.isfinite(got[k].float()).all(), k
        kb.assert_bf16(got[k], ref[k], slack[k], "swiglu", k, "|x1|<=100")


def _poisoned(n):
    """An output buffer no kernel result equals: NaN everywhere, so an
    element the kernel never wrote fails the bound."""
    return torch.full((n,), float("nan"), device="cuda", dtype=torch.bfloat16)


def _check_sliced(got, refs, op, n, formula, slack_fn):
    """fp64 reference on the GPU, a slice at a time."""
    worst = {k: 0.0 for k in got}
    for lo in range(0, n, SLICE):
        sl = slice(lo, min(n, lo + SLICE))
        args = [t[sl] for t in refs]
        ref = formula(*args)
        slack = slack_fn(*args)
        for k in got:
            bad, w = kb.violations(got[k][sl], ref[k], slack[k])
            worst[k] = max(worst[k], w)
            assert not bad.any(), (
                f"{op} {k} n={n}: {int(bad.sum())} elements outside the "
                f"bound in [{lo}, {sl.stop}), first at "
                f"{lo + int(bad.nonzero()[0])}")
    for k, w in worst.items():
        kb.report(op, k, f"randn/n={n}", w)


@pytest.mark.parametrize("n", SIZES)
def test_gelu_sizes(n):
    """A partial last block (n/8 no multiple of 256), and the smallest sizes
    at which the grid-stride loop makes a second and a third sweep."""
    g = torch.Generator(device="cuda").manual_seed(n % 1000)
    x = (torch.randn(n, device="cuda", generator=g) * 3).to(torch.bfloat16)
    dy = torch.randn(n, device="cuda", generator=g).to(torch.bfloat16)
    y, dx = _poisoned(n), _poisoned(n)
    _core.gelu_fwd(x.data_ptr(), y.data_ptr(), n, _stream())
    _core.gelu_bwd(dy.data_ptr(), x.data_ptr(), dx.data_ptr(), n, _stream())
    torch.cuda.synchronize()
    _check_sliced({"y": y, "dx": dx}, (x, dy), "gelu", n, kb.gelu_formula,
                  kb.gelu_slack)
    del x, dy, y, dx
    torch.cuda.empty_cache()


@pytest.mark.parametrize("n", SIZES)
def test_swiglu_sizes(n):
    g = torch.Generator(device="cuda").manual_seed(n % 1000 + 1)
    x1 = (torch.randn(n, device="cuda", generator=g) * 2).to(torch.bfloat16)
    x3 = torch.randn(n, device="cuda", generator=g).to(torch.bfloat16)
    dy = torch.randn(n, device="cuda", generator=g).to(torch.bfloat16)
    y, dx1, dx3 = _poisoned(n), _poisoned(n), _poisoned(n)
    _core.swiglu_fwd(x1.data_ptr(), x3.data_ptr(), y.data_ptr(), n, _stream())
    _core.swiglu_bwd(dy.data_ptr(), x1.data_ptr(), x3.data_ptr(),
                     dx1.data_ptr(), dx3.data_ptr(), n, _stream())
    torch.cuda.synchronize()
    _check_sliced({"y": y, "dx1": dx1, "dx3": dx3}, (x1, x3, dy), "swiglu", n,
                  kb.swiglu_formula, kb.swiglu_slack)
    del x1, x3, dy, y, dx1, dx3
    torch.cuda.empty_cache()


@pytest.mark.parametrize("shape", [(0,), (0, 3072), (4, 0, 8)])
def test_empty_input(shape):
    x = torch.empty(shape, device="cuda", dtype=torch.bfloat16,
                    requires_grad=True)
    y = fused_gelu.fused_gelu(x)
    y.float().sum().backward()
    assert y.shape == shape and x.grad.shape == shape
    a = torch.empty(shape, device="cuda", dtype=torch.bfloat16,
                    requires_grad=True)
    b = torch.empty(shape, device="cuda", dtype=torch.bfloat16,
                    requires_grad=True)
    y = fused_swiglu.fused_swiglu(a, b)
    y.float().sum().backward()
    torch.cuda.synchronize()
    assert y.shape == shape and a.grad.shape == shape == b.grad.shape


def _offset_view(src, off=4):
    """A contiguous copy of `src` starting `off` elements (8 bytes) into an
    allocation: not 16-byte aligned."""
    buf = torch.empty(src.numel() + 8, dtype=src.dtype, device=src.device)
    v = buf[off:off + src.numel()].view(src.shape)
    v.copy_(src)
    assert v.data_ptr() % 16 == 8 and v.is_contiguous()
    return v


def test_misaligned_views_give_the_same_values():
    g = torch.Generator(device="cuda").manual_seed(3)
    x, x3, dy = ((torch.randn(33, 72, device="cuda", generator=g) * 2).to(
        torch.bfloat16) for _ in range(3))
    base = run_gelu(x, dy)
    for args in ((_offset_view(x), dy), (x, _offset_view(dy))):
        got = run_gelu(*args)
        for k in base:
            assert torch.equal(base[k], got[k]), k
    base = run_swiglu(x, x3, dy)
    for args in ((_offset_view(x), x3, dy), (x, _offset_view(x3), dy),
                 (x, x3, _offset_view(dy))):
        got = run_swiglu(*args)
        for k in base:
            assert torch.equal(base[k], got[k]), k


def test_core_rejects_misaligned_pointers():
    n = 64
    x = torch.ones(n, device="cuda", dtype=torch.bfloat16)
    xo = _offset_view(x)
    y = torch.zeros(n, device="cuda", dtype=torch.bfloat16)
    y2 = torch.zeros(n, device="cuda", dtype=torch.bfloat16)
    s = _stream()
    with pytest.raises(RuntimeError, match="aligned"):
        _core.gelu_fwd(xo.data_ptr(), y.data_ptr(), n, s)
    with pytest.raises(RuntimeError, match="aligned"):
        _core.gelu_bwd(xo.data_ptr(), x.data_ptr(), y.data_ptr(), n, s)
    with pytest.raises(RuntimeError, match="aligned"):
        _core.swiglu_fwd(x.data_ptr(), xo.data_ptr(), y.data_ptr(), n, s)
    with pytest.raises(RuntimeError, match="aligned"):
        _core.swiglu_bwd(xo.data_ptr(), x.data_ptr(), x.data_ptr(),
                         y.data_ptr(), y2.data_ptr(), n, s)
    torch.cuda.synchronize()
    assert not y.any() and not y2.any()  # nothing was launched
