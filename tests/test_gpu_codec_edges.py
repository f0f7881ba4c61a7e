"""Codec kernels at the values where quantizers go wrong: exact rounding
ties, saturation under a stale (explicit) scale, zeros of both signs,
non-finite, subnormal and near-overflow residuals, scales at the exact
power-of-two boundaries, and the decode of every payload byte.

Expected values come from ops/oracle.py and, for fp8, also from the
table-built e4m3 reference in codec_reference.py.  "Explicit scale" means
the test writes the scale buffer itself instead of calling reduce_scales,
which is the lagged-scale situation: only there can |v / s| exceed the
codec's range or sit on a tie.
"""
import numpy as np
import pytest
import torch

import codec_reference as cr
import sharedtensor_amd  # noqa: F401
from sharedtensor_amd import _core
from sharedtensor_amd.ops import oracle as oc
from test_gpu_codec_table import (assert_bits_equal, assert_sentinel,
                                  dev_buffer, stream)

pytestmark = pytest.mark.gpu

F = np.float32
# 2^-130 is a subnormal fp32 scale, whose reciprocal is not an fp32 number.
# Its quanta (down to 2^-139) lie below bf16's smallest subnormal 2^-133, so
# it is an fp32-residual case; bf16 residuals take 2^-110 in its place, the
# region where every quantum and every residual is still a normal bf16.
BF16_SMALL_SCALE = 2.0 ** -110
SCALES = [2.0 ** -130, 2.0 ** -20, 1.0, 2.0 ** 100]
SCALE_IDS = ["2^-130", "2^-20", "1", "2^100"]
RESIDUALS = [False, True]
RES_IDS = ["f32", "bf16"]


def bf16_representable(v: np.ndarray) -> np.ndarray:
    t = torch.from_numpy(v)
    return (t.to(torch.bfloat16).float() == t).numpy() | np.isnan(v)


def pad_to(v: np.ndarray, lo=64) -> np.ndarray:
    return np.concatenate([v, np.zeros(max(lo - v.size, 0), F)]).astype(F)


def quantize_explicit(codec, v, scale, bf16):
    """Run quantize on fp32 values v with the scale buffer set to `scale`.
    Returns payload bytes, the residual buffer (device dtype, n elements)."""
    n = v.size
    d = dev_buffer(torch.from_numpy(v), bf16)
    dc = _core.DevCodec(codec, [n], 0, delta_bf16=bf16)
    scales = torch.tensor([scale], dtype=torch.float32, device="cuda")
    assert scales.item() == scale
    payload = torch.full((_core.payload_bytes(codec, n),), 0xAA,
                         dtype=torch.uint8, device="cuda")
    dc.quantize(d.data_ptr(), scales.data_ptr(), payload.data_ptr(), stream())
    torch.cuda.synchronize()
    assert_sentinel(d, n, "residual")
    return payload.cpu().numpy().tobytes(), d.cpu()[:n]


def check_explicit(codec, ratios, scale, bf16):
    """v = fl32(ratio * scale); the ratio actually quantized is v / scale,
    exact in fp64 because the scale is a power of two."""
    v = (np.asarray(ratios, np.float64) * scale).astype(F)
    if bf16:
        v = v[bf16_representable(v)]
    v = pad_to(v)
    n = v.size
    assert 64 <= n <= 4096
    payload, res = quantize_explicit(codec, v, scale, bf16)
    s_o, payload_o, res_o = oc.encode(codec, torch.from_numpy(v), scale)
    assert s_o == scale
    got = np.frombuffer(payload, np.uint8)
    want = np.frombuffer(payload_o, np.uint8)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(i, hex(got[i]), hex(want[i])) for i in bad[:8]]
    if codec == 1:
        x = v.astype(np.float64) / scale
        codes = cr.e4m3_encode(x)
        bad = np.nonzero(got[:n] != codes)[0]
        assert bad.size == 0, [(float(x[i]), hex(got[i]), hex(codes[i]))
                               for i in bad[:8]]
        sent = (cr.e4m3_decode(codes) * scale).astype(F)
        assert np.array_equal(sent.astype(np.float64),
                              cr.e4m3_decode(codes) * scale)
        np.testing.assert_array_equal((v - sent).view(np.int32),
                                      res_o.numpy().view(np.int32))
    want_res = cr.bf16_rne(res_o) if bf16 else res_o
    assert_bits_equal(res, want_res, "residual")


def both_signs(x):
    x = np.asarray(x, np.float64)
    return np.concatenate([x, -x])


def fp8_ratios():
    return both_signs(np.concatenate([
        cr.with_neighbours(cr.e4m3_midpoints()),
        cr.with_neighbours([448.0])[:2],            # 448 and the next above
        [1e4],
        cr.with_neighbours([2.0 ** -10]),           # tie to zero
    ]).astype(np.float64))


def int4_ratios():
    ties = np.arange(-8, 8, dtype=np.float64) + 0.5
    return np.concatenate([cr.with_neighbours(ties).astype(np.float64),
                           both_signs([7.49, 7.5, 100.0])])


@pytest.mark.parametrize("bf16", RESIDUALS, ids=RES_IDS)
@pytest.mark.parametrize("scale", SCALES, ids=SCALE_IDS)
def test_fp8_ties_and_saturation(scale, bf16):
    if bf16 and scale == SCALES[0]:
        scale = BF16_SMALL_SCALE
    check_explicit(1, fp8_ratios(), scale, bf16)


@pytest.mark.parametrize("bf16", RESIDUALS, ids=RES_IDS)
@pytest.mark.parametrize("scale", SCALES, ids=SCALE_IDS)
def test_int4_ties_and_saturation(scale, bf16):
    if bf16 and scale == SCALES[0]:
        scale = BF16_SMALL_SCALE
    check_explicit(2, int4_ratios(), scale, bf16)


@pytest.mark.parametrize("bf16", RESIDUALS, ids=RES_IDS)
@pytest.mark.parametrize("scale", [0.5, 2.0 ** -120, 2.0 ** 100])
def test_1bit_zeros_and_subnormals(scale, bf16):
    """A zero of either sign is "not positive": bit 1 (-scale was sent) and
    the residual becomes +scale."""
    tiny32, tiny16 = 2.0 ** -149, 2.0 ** -133
    v = np.tile(np.array([0.0, -0.0, tiny32, -tiny32, tiny16, -tiny16], F), 16)
    if bf16:
        v = v[bf16_representable(v)]
    n = v.size
    payload, res = quantize_explicit(0, v, scale, bf16)
    _, payload_o, res_o = oc.encode(0, torch.from_numpy(v), scale)
    assert payload == payload_o
    assert_bits_equal(res, cr.bf16_rne(res_o) if bf16 else res_o, "residual")
    bits = np.unpackbits(np.frombuffer(payload, np.uint8), bitorder="little")[:n]
    zero = v == 0
    assert (bits[zero] == 1).all()
    assert (res.float().numpy()[zero] == F(scale)).all()
    assert (bits[v > 0] == 0).all() and (bits[v < 0] == 1).all()


@pytest.mark.parametrize("bf16", RESIDUALS, ids=RES_IDS)
@pytest.mark.parametrize("codec", [0, 1, 2], ids=["1bit", "fp8", "int4"])
def test_zero_scale_keepalive_in_table(codec, bf16):
    """An all-zero tensor (zeros of both signs) between two live ones: scale
    0, zero payload region, residual and destinations untouched.  Its first
    element sits at an odd offset, so with bf16 residuals it shares a packed
    pair with the last element of the tensor before it."""
    sizes = [101, 64, 129]
    g = torch.Generator().manual_seed(40 + codec)
    parts = [torch.randn(s, generator=g) for s in sizes]
    parts[1] = torch.zeros(64)
    parts[1][::3] = -0.0
    if bf16:
        parts = [p.to(torch.bfloat16).float() for p in parts]
    n = sum(sizes)
    lo, hi = sizes[0], sizes[0] + sizes[1]
    d = dev_buffer(torch.cat(parts), bf16)
    before = d.cpu()[:n].clone()
    dc = _core.DevCodec(codec, sizes, 0, delta_bf16=bf16)
    scales = torch.full((3,), -1.0, dtype=torch.float32, device="cuda")
    pb = [_core.payload_bytes(codec, s) for s in sizes]
    payload = torch.full((sum(pb),), 0xAA, dtype=torch.uint8, device="cuda")
    s = stream()
    dc.reduce_scales(d.data_ptr(), scales.data_ptr(), 1, s)
    dc.quantize(d.data_ptr(), scales.data_ptr(), payload.data_ptr(), s)
    torch.cuda.synchronize()
    scales_o, payload_o, res_o = oc.encode_table(codec, parts)
    assert scales_o[1] == 0.0 and scales_o[0] > 0 and scales_o[2] > 0
    assert scales.cpu().tolist() == scales_o
    assert payload.cpu().numpy().tobytes() == payload_o
    assert (payload.cpu()[pb[0]: pb[0] + pb[1]] == 0).all()
    want = torch.cat(res_o)
    assert_bits_equal(d.cpu()[:n], cr.bf16_rne(want) if bf16 else want,
                      "residual")
    assert_bits_equal(d.cpu()[lo:hi], before[lo:hi], "keepalive residual")
    assert_sentinel(d, n, "residual")

    init = torch.randn(n, generator=g)
    init[lo:hi:2] = -0.0
    vals = init.clone().cuda()
    fwd = dev_buffer(init, bf16)
    fwd0 = fwd.cpu().clone()
    dc.apply(payload.data_ptr(), scales.data_ptr(),
             [vals.data_ptr(), fwd.data_ptr()], s)
    torch.cuda.synchronize()
    assert_bits_equal(vals.cpu()[lo:hi], init[lo:hi], "keepalive values")
    assert_bits_equal(fwd.cpu()[lo:hi], fwd0[lo:hi], "keepalive forward")
    dec = torch.cat(oc.decode_table(codec, payload_o, scales_o, sizes))
    want_vals = init + dec
    want_vals[lo:hi] = init[lo:hi]          # skipped, not "+ 0.0"
    assert_bits_equal(vals.cpu(), want_vals, "values")
    assert_sentinel(fwd, n, "forward")


@pytest.mark.parametrize("bf16", RESIDUALS, ids=RES_IDS)
@pytest.mark.parametrize("codec", [0, 1, 2], ids=["1bit", "fp8", "int4"])
@pytest.mark.parametrize("poison", ["nan", "inf", "-inf"])
def test_non_finite_element_is_never_sent(poison, codec, bf16):
    n = 1000
    g = torch.Generator().manual_seed(7)
    v = torch.randn(n, generator=g)
    v[613] = float(poison)
    if bf16:
        v = v.to(torch.bfloat16).float()
    d = dev_buffer(v, bf16)
    before = d.cpu().clone()
    dc = _core.DevCodec(codec, [n], 0, delta_bf16=bf16)
    scales = torch.full((1,), -1.0, dtype=torch.float32, device="cuda")
    payload = torch.full((_core.payload_bytes(codec, n),), 0xAA,
                         dtype=torch.uint8, device="cuda")
    dc.reduce_scales(d.data_ptr(), scales.data_ptr(), 1, stream())
    dc.quantize(d.data_ptr(), scales.data_ptr(), payload.data_ptr(), stream())
    torch.cuda.synchronize()
    assert oc.compute_scale(codec, v) == 0.0
    assert scales.item() == 0.0
    assert (payload.cpu() == 0).all()
    assert_bits_equal(d.cpu(), before, "residual")


FLT_MIN = 1.1754943508222875e-38


def _tiny_huge_cases():
    g = torch.Generator().manual_seed(3)
    sign = torch.where(torch.rand(4096, generator=g) < 0.5, -1.0, 1.0)
    return {
        "flt_min": torch.tensor([FLT_MIN]),
        "-flt_min": torch.tensor([-FLT_MIN]),
        "mixed_tiny": torch.tensor([FLT_MIN, -3e-38, 2e-38, 0.0]),
        "uniform_3e-38": (torch.rand(4096, generator=g) * 2 - 1) * 3e-38,
        "subnormal_1e-42": (1e-42 * (1 + torch.rand(4096, generator=g))
                            * sign).float(),
        "huge_3e38": 3e38 * sign,
    }


@pytest.mark.parametrize("codec", [0, 1, 2], ids=["1bit", "fp8", "int4"])
@pytest.mark.parametrize("case", ["flt_min", "-flt_min", "mixed_tiny",
                                  "uniform_3e-38", "subnormal_1e-42",
                                  "huge_3e38"])
def test_tiny_and_huge_values(case, codec):
    v = _tiny_huge_cases()[case].float()
    n = v.numel()
    d = v.clone().cuda()
    dc = _core.DevCodec(codec, [n], 0)
    scales = torch.full((1,), -1.0, dtype=torch.float32, device="cuda")
    payload = torch.full((_core.payload_bytes(codec, n),), 0xAA,
                         dtype=torch.uint8, device="cuda")
    dc.reduce_scales(d.data_ptr(), scales.data_ptr(), 1, stream())
    dc.quantize(d.data_ptr(), scales.data_ptr(), payload.data_ptr(), stream())
    vals = torch.zeros(n, device="cuda")
    dc.apply(payload.data_ptr(), scales.data_ptr(), [vals.data_ptr()], stream())
    torch.cuda.synchronize()
    scale_o, payload_o, res_o = oc.encode(codec, v)
    assert scale_o > 0
    assert scales.item() == scale_o
    assert payload.cpu().numpy().tobytes() == payload_o
    assert_bits_equal(d.cpu(), res_o, "residual")
    assert_bits_equal(vals.cpu(), oc.decode(codec, payload_o, scale_o, n),
                      "applied")


@pytest.mark.parametrize("k", [-140, -126, 0, 100])
def test_scale_boundaries(k):
    """RMS exactly 2^k; absmax exactly 448 * 2^k and 7 * 2^k and the next
    fp32 above them."""
    n = 256
    p2 = F(2.0) ** F(k)
    assert float(p2) == 2.0 ** k
    sign = np.where(np.arange(n) % 3 == 0, -1, 1).astype(F)

    def scale_of(codec, v):
        d = torch.from_numpy(v.astype(F)).cuda()
        dc = _core.DevCodec(codec, [n], 0)
        out = torch.full((1,), -1.0, dtype=torch.float32, device="cuda")
        dc.reduce_scales(d.data_ptr(), out.data_ptr(), 1, stream())
        torch.cuda.synchronize()
        assert out.item() == oc.compute_scale(codec, torch.from_numpy(v))
        return out.item()

    assert scale_of(0, sign * p2) == 2.0 ** k
    for codec, top in ((1, 448.0), (2, 7.0)):
        if k + 9 > 127:
            continue
        v = (sign * F(1e-3) * p2).astype(F)
        v[77] = -F(top) * p2
        if float(v[77]) != -top * 2.0 ** k:      # not an fp32 number
            continue
        assert scale_of(codec, v) == 2.0 ** k
        v[77] = np.nextafter(v[77], F(-np.inf))
        assert scale_of(codec, v) == 2.0 ** (k + 1)


@pytest.mark.parametrize("bf16", RESIDUALS, ids=RES_IDS)
@pytest.mark.parametrize("ndst", [1, 2, 3])
@pytest.mark.parametrize("scale", [1.0, 2.0 ** -3])
@pytest.mark.parametrize("codec", [1, 2], ids=["fp8", "int4"])
def test_decode_every_byte(codec, scale, ndst, bf16):
    raw = np.arange(256, dtype=np.uint8)
    n = 256 if codec == 1 else 512
    if codec == 1:
        want = cr.E4M3 * scale
    else:
        nib = np.stack([raw & 0xF, raw >> 4], axis=1).reshape(-1).astype(np.int64)
        want = np.where(nib > 7, nib - 16, nib) * scale      # nibble 8 is -8
        assert want.min() == -8 * scale
    orc = oc.decode(codec, raw.tobytes(), scale, n).double().numpy()
    np.testing.assert_array_equal(orc, want)                  # NaN == NaN here
    payload = torch.from_numpy(raw).cuda()
    dc = _core.DevCodec(codec, [n], 0, delta_bf16=bf16)
    scales = torch.tensor([scale], dtype=torch.float32, device="cuda")
    vals = torch.zeros(n, device="cuda")
    fwd = [dev_buffer(torch.zeros(n), bf16) for _ in range(ndst - 1)]
    dc.apply(payload.data_ptr(), scales.data_ptr(),
             [vals.data_ptr()] + [f.data_ptr() for f in fwd], stream())
    torch.cuda.synchronize()
    nan = np.isnan(want)
    assert nan.sum() == (2 if codec == 1 else 0)
    for t in [vals] + [f[:n] for f in fwd]:
        got = t.cpu().double().numpy()
        assert np.isnan(got[nan]).all()
        np.testing.assert_array_equal(got[~nan], want[~nan])
    for f in fwd:
        assert_sentinel(f, n, "forward")
