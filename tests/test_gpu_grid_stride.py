"""Every elementwise codec kernel past the grid cap of 32768 x 256 threads:
n = 8,388,608 + 337 elements, so 337 threads run a second grid-stride
iteration and the rest must stop after one.

Whole-buffer checks run on the GPU with torch ops; windows at the start,
across the end of the first grid pass, and at 16 random places go through
the CPU oracle with the kernel's own scale.  The optimizer, snapshot and
delta-scatter kernels are held at this size in test_gpu_optim_kernels.py.
"""
import numpy as np
import pytest
import torch

import codec_reference as cr
import sharedtensor_amd  # noqa: F401
from sharedtensor_amd import _core
from sharedtensor_amd.ops import oracle as oc
from test_gpu_codec_table import assert_bits_equal, stream
from test_gpu_optim_kernels import N_GRID, check_tail, gpu_bits_equal, res_buf

pytestmark = pytest.mark.gpu

CAP = 32768 * 256
WIN = 4096


def windows():
    rng = np.random.default_rng(12)
    starts = rng.integers(0, (N_GRID - WIN) // 64, 16) * 64
    return [(0, WIN), (CAP - WIN, N_GRID)] + [(int(a), int(a) + WIN)
                                              for a in starts]


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("codec", [0, 1, 2], ids=["1bit", "fp8", "int4"])
def test_codec_second_grid_iteration(codec, bf16):
    n = N_GRID
    torch.manual_seed(100 + codec)
    dt = torch.bfloat16 if bf16 else torch.float32
    d = res_buf(n, bf16)
    d[:n] = (torch.randn(n, device="cuda") * 3).to(dt)   # RMS far from 2^k
    before = d[:n].clone()
    before_cpu = before.float().cpu()
    if codec == 0:
        cr.assert_rms_standoff(before_cpu.numpy(), 1, "grid-stride input")
    dc = _core.DevCodec(codec, [n], 0, delta_bf16=bf16)
    scales = torch.full((1,), -1.0, dtype=torch.float32, device="cuda")
    payload = torch.full((_core.payload_bytes(codec, n),), 0xAA,
                         dtype=torch.uint8, device="cuda")
    vals = torch.zeros(n, device="cuda")
    fwd = res_buf(n, bf16)
    s = stream()
    dc.reduce_scales(d.data_ptr(), scales.data_ptr(), 1, s)
    dc.quantize(d.data_ptr(), scales.data_ptr(), payload.data_ptr(), s)
    dc.apply(payload.data_ptr(), scales.data_ptr(),
             [vals.data_ptr(), fwd.data_ptr()], s)
    torch.cuda.synchronize()
    scale = scales.item()
    assert scale == oc.compute_scale(codec, before_cpu) and scale > 0

    # whole buffer, on the GPU: vals is what was sent (added to +0.0)
    dec = vals
    gpu_bits_equal(d[:n], (before.float() - dec).to(dt), "residual == d - sent")
    gpu_bits_equal(fwd[:n], dec.to(dt), "forward == sent")
    assert (dec.to(dt).float() == dec).all()
    if codec == 0:
        assert (dec.abs() == scale).all()
    check_tail(d, n)
    check_tail(fwd, n)

    per_byte = {0: 8, 1: 1, 2: 2}[codec]
    pay = payload.cpu().numpy()
    res_cpu, dec_cpu = d[:n].cpu(), dec.cpu()
    for a, b in windows():
        _, p_o, r_o = oc.encode(codec, before_cpu[a:b], scale)
        got = pay[a // per_byte: a // per_byte + len(p_o)].tobytes()
        assert got == p_o, f"payload window [{a}, {b})"
        assert_bits_equal(res_cpu[a:b], r_o.to(dt), f"residual window [{a}, {b})")
        want = torch.zeros(b - a) + oc.decode(codec, p_o, scale, b - a)
        assert_bits_equal(dec_cpu[a:b], want, f"decoded window [{a}, {b})")


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_add_scatter_second_grid_iteration(bf16):
    n = N_GRID
    torch.manual_seed(200)
    dt = torch.bfloat16 if bf16 else torch.float32
    src = torch.randn(n, device="cuda")
    src[::9] = 0.0
    vals0 = torch.randn(n, device="cuda")
    vals = vals0.clone()
    ds = [res_buf(n, bf16) for _ in range(3)]
    ptrs = [vals.data_ptr()] + [x.data_ptr() for x in ds]
    _core.gpu_add_scatter(src.data_ptr(), n, 0.0, ptrs, stream(), bf16)
    torch.cuda.synchronize()
    gpu_bits_equal(vals, vals0, "alpha = 0 leaves values")
    for x in ds:
        assert (x[:n].view(torch.int16 if bf16 else torch.int32) == 0).all()
        check_tail(x, n)
    _core.gpu_add_scatter(src.data_ptr(), n, 2.5, ptrs, stream(), bf16)
    torch.cuda.synchronize()
    v = 2.5 * src                  # one rounding, as in the kernel
    gpu_bits_equal(vals, vals0 + v, "values += alpha * src")
    for x in ds:
        gpu_bits_equal(x[:n], (torch.zeros_like(v) + v).to(dt),
                       "residual += alpha * src")
        check_tail(x, n)
