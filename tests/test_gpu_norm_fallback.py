"""Block-per-row LayerNorm / RMSNorm kernels and colsum (csrc/ln_kernels.hip)
against the fp64 reference and derived bounds of tests/kernel_bounds.py.

The kernels are templated on bf16 pairs per thread, cpt = ceil(C/2/256) in
buckets 1, 2, 3, 4, 8, and the dw kernels on elements per thread, ecpt =
ceil(C/256) in buckets 1, 2, 3, 4, 8, 16.  WIDTHS sits on both sides of every
bucket boundary, with ragged tails (C/2 no multiple of 64) and last
iterations one lane wide.  None of them is a width the wave-per-row add+LN
kernels take, so fused_layer_norm runs the kernels under test."""
import pytest
import torch

import kernel_bounds as kb
from sharedtensor_amd import _core
from sharedtensor_amd.ops import fused_ln, fused_rms

pytestmark = pytest.mark.gpu

EPS = kb.EPS
WIDTHS = [2, 64, 66, 510, 514, 1022, 1026, 1280, 1534, 1538, 2046, 2050,
          4094]
DW_GRID = 2048  # the dw kernels' grid cap: rows beyond it make them loop


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _poisoned(like, dtype=None, n=None):
    """An output buffer filled with NaN: torch.empty may hand back the block
    that still holds the previous, correct result, and an element the kernel
    never stored would then pass."""
    shape = like.shape if n is None else (n,)
    return torch.full(shape, float("nan"), device="cuda",
                      dtype=dtype or like.dtype)


def core_ln(x, w, b, dy):
    """_core.ln_fwd + ln_bwd on 2-D inputs: every raw output."""
    R, C = x.shape
    y = _poisoned(x)
    mean = _poisoned(x, torch.float32, R)
    rstd = _poisoned(x, torch.float32, R)
    _core.ln_fwd(x.data_ptr(), w.data_ptr(),
                 b.data_ptr() if b is not None else 0, y.data_ptr(),
                 mean.data_ptr(), rstd.data_ptr(), R, C, EPS, _stream())
    dx = _poisoned(x)
    dg = torch.zeros(C, dtype=torch.float32, device="cuda")
    db = torch.zeros(C, dtype=torch.float32, device="cuda")
    _core.ln_bwd(dy.data_ptr(), x.data_ptr(), w.data_ptr(), mean.data_ptr(),
                 rstd.data_ptr(), dx.data_ptr(), dg.data_ptr(), db.data_ptr(),
                 R, C, _stream())
    torch.cuda.synchronize()
    return {"y": y, "mean": mean, "rstd": rstd, "dx": dx, "dgamma": dg,
            "dbeta": db}


def core_rms(x, w, dy):
    R, C = x.shape
    y = _poisoned(x)
    rstd = _poisoned(x, torch.float32, R)
    _core.rms_fwd(x.data_ptr(), w.data_ptr(), y.data_ptr(), rstd.data_ptr(),
                  R, C, EPS, _stream())
    dx = _poisoned(x)
    dg = torch.zeros(C, dtype=torch.float32, device="cuda")
    _core.rms_bwd(dy.data_ptr(), x.data_ptr(), w.data_ptr(), rstd.data_ptr(),
                  dx.data_ptr(), dg.data_ptr(), R, C, _stream())
    torch.cuda.synchronize()
    return {"y": y, "rstd": rstd, "dx": dx, "dgamma": dg}


def check_ln(x, w, b, dy, family):
    C = x.shape[-1]
    assert not _core.add_ln_supported(C)  # the fallback is what runs
    kb.check_ln_wrapper(fused_ln.fused_layer_norm, x, w, b, dy, family)
    got = core_ln(x, w, b, dy)
    ref = kb.ln_formula(x, w, b, dy)
    slack = kb.ln_slack(x, w, b, dy)
    for k in ("mean", "rstd", "dgamma", "dbeta"):
        kb.assert_f32(got[k], ref[k], slack[k], "ln", k, family)
    for k in ("y", "dx"):  # raw kernel output, same bound
        kb.assert_bf16(got[k], ref[k], slack[k], "ln-core", k, family)


def check_rms(x, w, dy, family):
    kb.check_rms_wrapper(fused_rms.fused_rms_norm, x, w, dy, family)
    got = core_rms(x, w, dy)
    ref = kb.rms_formula(x, w, dy)
    slack = kb.rms_slack(x, w, dy)
    for k in ("rstd", "dgamma"):
        kb.assert_f32(got[k], ref[k], slack[k], "rms", k, family)
    for k in ("y", "dx"):
        kb.assert_bf16(got[k], ref[k], slack[k], "rms-core", k, family)


@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("R", [1, 5])
def test_ln_widths(R, C):
    x, w, b, dy = kb.norm_inputs("randn2", R, C, device="cuda")
    check_ln(x, w, b, dy, f"randn2/C={C}")


@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("R", [1, 5])
def test_rms_widths(R, C):
    x, w, _, dy = kb.norm_inputs("randn2", R, C, device="cuda")
    check_rms(x, w, dy, f"randn2/C={C}")


@pytest.mark.parametrize("C", [66, 4094])
@pytest.mark.parametrize("family", kb.NORM_FAMILIES)
def test_ln_input_families(family, C):
    x, w, b, dy = kb.norm_inputs(family, 5, C, device="cuda")
    check_ln(x, w, b, dy, family)


@pytest.mark.parametrize("C", [66, 4094])
@pytest.mark.parametrize("family", kb.NORM_FAMILIES)
def test_rms_input_families(family, C):
    x, w, _, dy = kb.norm_inputs(family, 5, C, device="cuda")
    check_rms(x, w, dy, family)


def _sentinel_inputs(R, C):
    """dy of the last row and of row DW_GRID is 64x the others: a dropped or
    doubled sweep of the dw kernels' row loop moves the column sums by far
    more than the bound."""
    x, w, b, dy = kb.norm_inputs("randn2", R, C, device="cuda")
    dy = dy.clone()
    dy[R - 1] *= 64
    dy[DW_GRID] *= 64
    return x, w, b, dy


@pytest.mark.parametrize("C", [66, 514])
@pytest.mark.parametrize("R", [2049, 4099])
def test_row_grid_stride(R, C):
    x, w, b, dy = _sentinel_inputs(R, C)
    check_ln(x, w, b, dy, f"sentinel/R={R}")
    check_rms(x, w, dy, f"sentinel/R={R}")


EXACT_SHAPES = [(4099, 66), (2049, 4094), (7, 2), (1, 4096)]


@pytest.mark.parametrize("R,C", EXACT_SHAPES)
def test_dbeta_exact_on_integer_dy(R, C):
    """Integer-valued dy in [-4, 4]: the fp32 column sum is exact in any
    order, so dbeta equals the fp64 sum bit for bit."""
    g = torch.Generator(device="cuda").manual_seed(R + C)
    dy = torch.randint(-4, 5, (R, C), device="cuda",
                       generator=g).to(torch.bfloat16)
    x, w, b, _ = kb.norm_inputs("randn2", R, C, device="cuda")
    got = core_ln(x, w, b, dy)
    assert torch.equal(got["dbeta"].double(), dy.double().sum(0))


def test_ln_without_bias():
    x, w, b, dy = kb.norm_inputs("randn2", 5, 514, device="cuda")
    got = kb.check_ln_wrapper(fused_ln.fused_layer_norm, x, w, None, dy,
                              "bias=None")
    assert "dbeta" not in got
    wf = w.clone().requires_grad_(True)
    y0 = fused_ln.fused_layer_norm(x, wf, None, EPS)
    y0.backward(dy)
    zero = torch.zeros_like(b).requires_grad_(True)
    yz = fused_ln.fused_layer_norm(x, w, zero, EPS)
    assert torch.equal(y0, yz)
    assert torch.equal(got["y"], yz)


def _same(op, base, got, x, w, b, dy):
    """y and dx bit for bit; the weight gradient, summed by fp32 atomics in
    whatever order the blocks finish, against the reference instead."""
    for a, c in zip(base[:2], got[:2]):
        assert torch.equal(a, c.reshape(a.shape))
    if op == "ln":
        ref = kb.ln_formula(x, w, b, dy)["dgamma"]
        slack = kb.ln_slack(x, w, b, dy)["dgamma"]
    else:
        ref = kb.rms_formula(x, w, dy)["dgamma"]
        slack = kb.rms_slack(x, w, dy)["dgamma"]
    kb.assert_bf16(got[2], ref, slack, op, "dgamma", "layout-variant")


@pytest.mark.parametrize("op", ["ln", "rms"])
def test_layout_variants(op):
    """Non-contiguous x, a 3-D input and a stride-0 dy give what the plain
    2-D contiguous call gives."""
    R, C = 6, 514
    x, w, b, dy = kb.norm_inputs("randn2", R, C, device="cuda")

    def run(xin, dyin):
        xf = xin.detach().requires_grad_(True)
        wf = w.clone().requires_grad_(True)
        if op == "ln":
            y = fused_ln.fused_layer_norm(xf, wf, b, EPS)
        else:
            y = fused_rms.fused_rms_norm(xf, wf, EPS)
        if dyin is None:
            y.sum().backward()          # stride-0 dy
        else:
            y.backward(dyin)
        return y.detach(), xf.grad, wf.grad

    base = run(x, dy)
    big = torch.empty(R, 2 * C, device="cuda", dtype=torch.bfloat16)
    big[:, ::2] = x
    big[:, 1::2] = 7.0
    nc = big[:, ::2]
    assert not nc.is_contiguous()
    _same(op, base, run(nc, dy), x, w, b, dy)
    _same(op, base, run(x.view(2, 3, C), dy.view(2, 3, C)), x, w, b, dy)
    ones = torch.ones_like(dy)
    _same(op, run(x, ones), run(x, None), x, w, b, ones)
    # and the stride-0 result is right, not merely the same
    if op == "ln":
        kb.check_ln_wrapper(fused_ln.fused_layer_norm, x, w, b, ones,
                            "dy=ones")
    else:
        kb.check_rms_wrapper(fused_rms.fused_rms_norm, x, w, ones, "dy=ones")


@pytest.mark.parametrize("R,C", [(5, 1280), (2049, 66)])
def test_y_and_dx_repeat_bit_for_bit(R, C):
    x, w, b, dy = kb.norm_inputs("randn2", R, C, device="cuda")
    a, c = core_ln(x, w, b, dy), core_ln(x, w, b, dy)
    for k in ("y", "dx", "mean", "rstd"):  # dgamma/dbeta go through atomics
        assert torch.equal(a[k], c[k]), k
    a, c = core_rms(x, w, dy), core_rms(x, w, dy)
    for k in ("y", "dx", "rstd"):
        assert torch.equal(a[k], c[k]), k


@pytest.mark.parametrize("shape", [(0, 66), (2, 0, 1280)])
def test_empty_input(shape):
    C = shape[-1]
    for op in ("ln", "rms"):
        x = torch.empty(shape, device="cuda", dtype=torch.bfloat16,
                        requires_grad=True)
        w = torch.ones(C, device="cuda", dtype=torch.bfloat16,
                       requires_grad=True)
        b = torch.zeros(C, device="cuda", dtype=torch.bfloat16,
                        requires_grad=True)
        if op == "ln":
            y = fused_ln.fused_layer_norm(x, w, b, EPS)
        else:
            y = fused_rms.fused_rms_norm(x, w, EPS)
        y.float().sum().backward()
        torch.cuda.synchronize()
        assert y.shape == shape and y.dtype == torch.bfloat16
        assert x.grad.shape == shape
        assert torch.equal(w.grad, torch.zeros_like(w))
        if op == "ln":
            assert torch.equal(b.grad, torch.zeros_like(b))


def test_empty_colsum():
    o = torch.zeros(66, dtype=torch.float32, device="cuda")
    x = torch.empty(0, 66, device="cuda", dtype=torch.bfloat16)
    _core.colsum_bf16(x.data_ptr(), o.data_ptr(), 0, 66, _stream())
    torch.cuda.synchronize()
    assert torch.equal(o, torch.zeros_like(o))


def _offset_view(src, off=1):
    """A contiguous copy of `src` starting `off` elements into a 256-byte
    aligned allocation: 2-byte aligned only for off = 1."""
    buf = torch.empty(src.numel() + 8, dtype=src.dtype, device=src.device)
    v = buf[off:off + src.numel()].view(src.shape)
    v.copy_(src)
    assert v.data_ptr() % 4 == 2 and v.is_contiguous()
    return v


@pytest.mark.parametrize("op", ["ln", "rms"])
def test_misaligned_views_give_the_same_values(op):
    x, w, b, dy = kb.norm_inputs("randn2", 5, 66, device="cuda")

    def run(xin, win, dyin):
        xf = xin.detach().requires_grad_(True)
        wf = win.detach().requires_grad_(True)
        if op == "ln":
            y = fused_ln.fused_layer_norm(xf, wf, b, EPS)
        else:
            y = fused_rms.fused_rms_norm(xf, wf, EPS)
        y.backward(dyin)
        torch.cuda.synchronize()
        return y.detach(), xf.grad, wf.grad

    base = run(x, w, dy)
    for args in ((_offset_view(x), w, dy), (x, _offset_view(w), dy),
                 (x, w, _offset_view(dy))):
        _same(op, base, run(*args), x, w, b, dy)


def test_core_rejects_misaligned_pointers():
    x, w, b, dy = kb.norm_inputs("randn2", 5, 66, device="cuda")
    s = _stream()
    y, dx = torch.empty_like(x), torch.empty_like(x)
    mean = torch.empty(5, dtype=torch.float32, device="cuda")
    rstd = torch.ones(5, dtype=torch.float32, device="cuda")
    dg = torch.zeros(66, dtype=torch.float32, device="cuda")
    db = torch.zeros(66, dtype=torch.float32, device="cuda")
    xo, dyo = _offset_view(x), _offset_view(dy)
    with pytest.raises(RuntimeError, match="aligned"):
        _core.ln_fwd(xo.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(),
                     mean.data_ptr(), rstd.data_ptr(), 5, 66, EPS, s)
    with pytest.raises(RuntimeError, match="aligned"):
        _core.rms_fwd(xo.data_ptr(), w.data_ptr(), y.data_ptr(),
                      rstd.data_ptr(), 5, 66, EPS, s)
    with pytest.raises(RuntimeError, match="aligned"):
        _core.ln_bwd(dyo.data_ptr(), x.data_ptr(), w.data_ptr(),
                     mean.data_ptr(), rstd.data_ptr(), dx.data_ptr(),
                     dg.data_ptr(), db.data_ptr(), 5, 66, s)
    with pytest.raises(RuntimeError, match="aligned"):
        _core.rms_bwd(dyo.data_ptr(), x.data_ptr(), w.data_ptr(),
                      rstd.data_ptr(), dx.data_ptr(), dg.data_ptr(), 5, 66, s)
    torch.cuda.synchronize()
    # nothing was launched: the weight gradients are still zero
    assert not dg.any() and not db.any()
