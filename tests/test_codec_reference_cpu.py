"""CPU self-test of tests/codec_reference.py.

The table-built e4m3 encoder, ops/oracle.py (torch.float8_e4m3fn) and the
C++ converters must agree wherever e4m3 rounding can go wrong: every code,
every midpoint between adjacent codes and its fp32 neighbours, saturation,
zeros of both signs and the tie at half the smallest subnormal.  And every
cell of the GPU table tests must satisfy the input condition those tests
assert (reference RMS clear of a power of two), before and after quantizing.
"""
import numpy as np
import pytest
import torch

import codec_reference as cr
from sharedtensor_amd import _core
from sharedtensor_amd.ops import oracle as oc


def _points():
    mids = cr.e4m3_midpoints()
    finite = cr.E4M3[np.isfinite(cr.E4M3)]
    extra = [448.0, 464.0, 480.0, 1e4, 0.0, 2.0 ** -9, 2.0 ** -10]
    pos = np.concatenate([finite, cr.with_neighbours(mids),
                          cr.with_neighbours(extra)])
    return np.concatenate([pos, -pos]).astype(np.float32)


def test_table_is_the_format():
    t = cr.E4M3
    assert t[0x00] == 0.0 and np.signbit(t[0x80]) and t[0x80] == 0.0
    assert t[0x01] == 2.0 ** -9 and t[0x07] == 7 * 2.0 ** -9
    assert t[0x08] == 2.0 ** -6 and t[0x38] == 1.0 and t[0x7E] == 448.0
    assert np.isnan(t[0x7F]) and np.isnan(t[0xFF])
    assert np.array_equal(t[0x80:0xFF], -t[0x00:0x7F])
    assert np.isfinite(t).sum() == 254


def test_all_codes_decode_alike():
    for code in range(256):
        mine = _core.e4m3_to_f32(code)
        ref = cr.E4M3[code]
        if np.isnan(ref):
            assert np.isnan(mine), code
        else:
            assert mine == ref and np.signbit(mine) == np.signbit(ref), code
    tor = torch.arange(256, dtype=torch.int32).to(torch.uint8).view(
        torch.float8_e4m3fn).double().numpy()
    np.testing.assert_array_equal(tor, cr.E4M3)      # NaN == NaN here


def test_encoders_agree_on_codes_midpoints_and_saturation():
    x = _points()
    ref = cr.e4m3_encode(x)
    cpp = np.array([_core.f32_to_e4m3(float(v)) for v in x], dtype=np.uint8)
    _, payload, _ = oc.encode_fp8(torch.from_numpy(x), 1.0)
    orc = np.frombuffer(payload, dtype=np.uint8)[: x.size]
    bad = np.nonzero((ref != cpp) | (ref != orc))[0]
    assert bad.size == 0, [(float(x[i]), hex(ref[i]), hex(cpp[i]), hex(orc[i]))
                           for i in bad[:8]]
    # every finite code encodes to itself, the sign of zero included
    fin = np.nonzero(np.isfinite(cr.E4M3))[0]
    np.testing.assert_array_equal(cr.e4m3_encode(cr.E4M3[fin]), fin)
    # ties go to the even code; half the smallest subnormal ties to zero
    assert cr.e4m3_encode([2.0 ** -10, -2.0 ** -10]).tolist() == [0x00, 0x80]
    assert cr.e4m3_encode([3 * 2.0 ** -10]).tolist() == [0x02]
    assert cr.e4m3_encode([464.0, 480.0, 1e4, -1e4]).tolist() == [
        0x7E, 0x7E, 0x7E, 0xFE]
    assert cr.e4m3_encode([float("nan")]).tolist() == [0x7F]
    assert _core.f32_to_e4m3(float("nan")) == 0x7F


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("mag", sorted(cr.MAGS))
@pytest.mark.parametrize("name", sorted(cr.ALL_LISTS))
def test_table_inputs_stand_off_powers_of_two(name, mag, bf16):
    """What test_gpu_codec_table asserts before each 1-bit launch, checked
    here for every cell so that no cell can be lost to its input."""
    parts = cr.table_parts(name, mag, bf16)
    _, _, res = oc.encode_table(oc.CODEC_1BIT, parts)
    for t, (p, r) in enumerate(zip(parts, res)):
        cr.assert_rms_standoff(p.numpy(), 1, f"{name}/{mag}/t{t}")
        cr.assert_rms_standoff(r.numpy(), 1, f"{name}/{mag}/t{t} residual")
    if not bf16 and name in cr.SAMPLED_LISTS:
        for stride in cr.SAMPLED_STRIDES:
            for t, p in enumerate(parts):
                cr.assert_rms_standoff(p.numpy(), stride,
                                       f"{name}/{mag}/t{t}/stride{stride}")
