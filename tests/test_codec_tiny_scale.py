"""Residuals near FLT_MIN give a power-of-two scale below 2^-127, whose
fp32 reciprocal is inf; the C++ CPU codec must still match the oracle."""
import numpy as np
import pytest
import torch

from sharedtensor_amd import _core
from sharedtensor_amd.ops import oracle as oc

FLT_MIN = 1.1754943508222875e-38


@pytest.mark.parametrize("codec", [0, 1, 2])
@pytest.mark.parametrize("vals", [[FLT_MIN], [-FLT_MIN],
                                  [FLT_MIN, -3e-38, 2e-38, 0.0]])
def test_cpu_codec_matches_oracle_at_tiny_scale(vals, codec):
    d = torch.tensor(vals, dtype=torch.float32)
    n = d.numel()
    d2 = d.clone()
    scale_o, payload_o, res_o = oc.encode(codec, d)
    buf = torch.zeros(_core.payload_bytes(codec, n), dtype=torch.uint8)
    scale_c, _ = _core.cpu_encode(codec, d2.data_ptr(), n, -1.0,
                                  buf.data_ptr())
    assert scale_c == scale_o
    assert buf.numpy().tobytes() == payload_o
    np.testing.assert_array_equal(d2.numpy(), res_o.numpy())
