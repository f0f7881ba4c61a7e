"""Codec kernels in table mode: several tensors of sizes that leave padding,
start tensors in the middle of a wave (int4: one thread holds two elements)
and at odd element offsets (bf16 residuals: packed-pair atomics), and a
list long enough that every thread's second grid-stride iteration lands in
another tensor than its first (the mid-loop statistics flush).

Everything is compared bitwise with ops/oracle.py: scales, payload bytes,
residuals, decoded values, and the lagged-scale statistics that the
quantize kernels accumulate for the next round.  Neighbouring tensors
differ by a factor 100 in magnitude, so a value leaking across a boundary
moves a power-of-two scale.
"""
import numpy as np
import pytest
import torch

import codec_reference as cr
import sharedtensor_amd  # noqa: F401
from sharedtensor_amd import _core
from sharedtensor_amd.ops import oracle as oc

pytestmark = pytest.mark.gpu

SENTINEL16 = 0x4049          # bf16 3.140625


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev_buffer(flat: torch.Tensor, bf16: bool) -> torch.Tensor:
    """fp32: the tensor itself.  bf16: an even number of elements, at least
    one sentinel past n."""
    if not bf16:
        return flat.clone().cuda()
    n = flat.numel()
    total = n + 1 + (n + 1) % 2
    buf = torch.full((total,), SENTINEL16, dtype=torch.int16).view(torch.bfloat16)
    buf[:n] = flat.to(torch.bfloat16)
    return buf.cuda()


def assert_sentinel(buf: torch.Tensor, n: int, what: str):
    if buf.dtype == torch.bfloat16:
        tail = cr.bits16(buf.cpu())[n:]
        assert (tail == SENTINEL16).all(), (what, tail.tolist())


def assert_bits_equal(got: torch.Tensor, want: torch.Tensor, what: str):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    view = cr.bits16 if got.dtype == torch.bfloat16 else cr.bits32
    bad = (view(got) != view(want)).nonzero()
    assert bad.numel() == 0, (
        f"{what}: {bad.shape[0]} of {got.numel()} differ; first at "
        f"{int(bad[0])}: got {float(got[int(bad[0])])!r}, want "
        f"{float(want[int(bad[0])])!r}")


def expected(codec, parts, bf16):
    """Oracle scales, payload, decoded values, residual as stored, and the
    fp32 residual the statistics see."""
    scales_o, payload_o, res_o = oc.encode_table(codec, parts)
    sizes = [p.numel() for p in parts]
    dec = oc.decode_table(codec, payload_o, scales_o, sizes)
    # what the kernel accumulates: fl32(v - sent), before any bf16 rounding
    stat_res = [p - d for p, d in zip(parts, dec)]
    for r, s in zip(res_o, stat_res):
        assert torch.equal(cr.bits32(r), cr.bits32(s))
    stored = torch.cat(stat_res)
    if bf16:
        stored = cr.bf16_rne(stored)
    return scales_o, payload_o, torch.cat(dec), stored, stat_res


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("codec", [0, 1, 2], ids=["1bit", "fp8", "int4"])
@pytest.mark.parametrize("mag", sorted(cr.MAGS))
@pytest.mark.parametrize("name", sorted(cr.SIZE_LISTS))
def test_table_bitwise_and_lagged_stats(name, mag, codec, bf16):
    sizes = cr.SIZE_LISTS[name]
    T, n = len(sizes), sum(sizes)
    parts = cr.table_parts(name, mag, bf16)
    scales_o, payload_o, dec_o, stored_o, stat_res = expected(codec, parts, bf16)
    if codec == 0:
        for t in range(T):
            cr.assert_rms_standoff(parts[t].numpy(), 1, f"t{t}")
            cr.assert_rms_standoff(stat_res[t].numpy(), 1, f"t{t} residual")

    d = dev_buffer(torch.cat(parts), bf16)
    dc = _core.DevCodec(codec, sizes, 0, delta_bf16=bf16)
    pb = sum(_core.payload_bytes(codec, s) for s in sizes)
    assert pb == len(payload_o)
    scales = torch.full((T,), -1.0, dtype=torch.float32, device="cuda")
    payload = torch.full((pb,), 0xAA, dtype=torch.uint8, device="cuda")
    stats = torch.zeros(T, dtype=torch.float64, device="cuda")     # 8 B each
    lagged = torch.full((T,), -1.0, dtype=torch.float32, device="cuda")
    fresh = torch.full((T,), -1.0, dtype=torch.float32, device="cuda")
    s = stream()
    dc.reduce_scales(d.data_ptr(), scales.data_ptr(), 1, s)
    dc.quantize(d.data_ptr(), scales.data_ptr(), payload.data_ptr(), s,
                stats.data_ptr())
    dc.finalize_scales(stats.data_ptr(), lagged.data_ptr(), s)
    dc.reduce_scales(d.data_ptr(), fresh.data_ptr(), 1, s)
    torch.cuda.synchronize()

    want_scales = torch.tensor(scales_o, dtype=torch.float32)
    assert_bits_equal(scales.cpu(), want_scales, "scales")
    assert (want_scales > 0).all()
    assert payload.cpu().numpy().tobytes() == payload_o, "payload"
    assert_bits_equal(d.cpu()[:n], stored_o, "residual")
    assert_sentinel(d, n, "residual")

    # next round's scales from the statistics fused into quantize
    want_lag = torch.tensor([oc.compute_scale(codec, r) for r in stat_res],
                            dtype=torch.float32)
    assert_bits_equal(lagged.cpu(), want_lag, "lagged scales")
    if not bf16:
        assert_bits_equal(fresh.cpu(), want_lag, "fresh reduce of the residual")
    else:
        print(f"LAGGED-vs-FRESH bf16 {name}/{mag}/codec{codec}: "
              f"{'equal' if torch.equal(fresh.cpu(), lagged.cpu()) else 'differ'}")

    # apply: fp32 replica + two residual-typed forwards
    vals = torch.zeros(n, dtype=torch.float32, device="cuda")
    f1 = dev_buffer(torch.zeros(n), bf16)
    f2 = dev_buffer(torch.zeros(n), bf16)
    dc.apply(payload.data_ptr(), scales.data_ptr(),
             [vals.data_ptr(), f1.data_ptr(), f2.data_ptr()], s)
    torch.cuda.synchronize()
    # added to +0.0: an fp8 code 0x80 decodes to -0.0 and 0.0 + -0.0 is +0.0
    applied = torch.zeros(n) + dec_o
    assert_bits_equal(vals.cpu(), applied, "applied values")
    want_f = cr.bf16_rne(applied) if bf16 else applied
    if bf16:   # the debit quanta are exact in bf16
        assert torch.equal(want_f.float(), dec_o)
    for f, what in ((f1, "forward 1"), (f2, "forward 2")):
        assert_bits_equal(f.cpu()[:n], want_f, what)
        assert_sentinel(f, n, what)


@pytest.mark.parametrize("stride", cr.SAMPLED_STRIDES)
@pytest.mark.parametrize("mag", sorted(cr.MAGS))
@pytest.mark.parametrize("name", cr.SAMPLED_LISTS)
def test_sampled_scale(name, mag, stride):
    """reduce_scales(stride) samples every stride-th element of each tensor,
    counted from the tensor's own start."""
    sizes = cr.ALL_LISTS[name]
    parts = cr.table_parts(name, mag, False)
    want, want_cpp = [], []
    for t, p in enumerate(parts):
        cr.assert_rms_standoff(p.numpy(), stride, f"t{t}")
        assert p[::stride].numel() == -(-p.numel() // stride)
        want.append(oc.pow2_floor(cr.rms64(p.numpy(), stride)))
        want_cpp.append(_core.cpu_scale(0, p.data_ptr(), p.numel(), stride))
    assert want == want_cpp
    d = torch.cat(parts).cuda()
    dc = _core.DevCodec(0, sizes, 0)
    scales = torch.full((len(sizes),), -1.0, dtype=torch.float32, device="cuda")
    dc.reduce_scales(d.data_ptr(), scales.data_ptr(), stride, stream())
    torch.cuda.synchronize()
    assert_bits_equal(scales.cpu(), torch.tensor(want, dtype=torch.float32),
                      f"scales at stride {stride}")
