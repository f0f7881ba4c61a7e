"""Compiler resource report of the parameter-group optimizer kernels (no GPU
needed: hipcc cross-compiles for gfx950).

The grouped kernels move the bytes of the ungrouped ones and must hide
their latency as well: no scratch, an occupancy not below that of the
ungrouped kernel with the same template arguments (compiled here the same
way), and the 3 KB of LDS that stage one tile's segments (3 arrays of
GROUP_TILE = 256 four-byte entries), far from limiting the blocks per CU.
"""
import re

import pytest

from resource_report import kernel_resources

LDS_CAP = 3 * 256 * 4


def _key(mangled):
    """(kernel, template arguments) of a mangled fused-optimizer kernel:
    the name is length-prefixed, the arguments run up to the 'EEv' that
    closes them."""
    m = re.match(r"_ZN5shamd\d+(k_fused_(?:adamw|sgd_bf16|sgd))(_grp)?I(.+?)EEv",
                 mangled)
    return (m.group(1), m.group(3), bool(m.group(2))) if m else None


@pytest.fixture(scope="module")
def reports(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("resource_usage")
    return (kernel_resources("optim_group_kernels.hip", tmp),
            kernel_resources("hip_kernels.hip", tmp))


def test_grouped_kernels_no_scratch_same_occupancy_small_lds(reports):
    grouped, plain = reports
    base = {}
    for name, res in plain.items():
        k = _key(name)
        if k:
            assert not k[2], name
            base[k[:2]] = res
    seen = set()
    for name, res in grouped.items():
        k = _key(name)
        assert k and k[2], name              # the file holds nothing else
        seen.add(k[:2])
        assert res["ScratchSize"] == 0, (name, res)
        assert res["Occupancy"] >= base[k[:2]]["Occupancy"], (
            name, res, base[k[:2]])
        assert 0 < res["LDS"] <= LDS_CAP, (name, res)
    # AdamW: 2 residual types x 2 gradient types x clip; SGD: 2 x clip each
    assert len(seen) == 8 + 4 + 4 and seen == set(base)
