"""ops/fused_wgrad.py without a GPU, for the pipelined 256 x 256 variant
(k_wgrad256p): its table entries, the split at the workload's shapes, what
``can_use`` rejects, and a model of the global-side swizzle of its
direct-to-LDS loads."""
import pytest
import torch

from sharedtensor_amd.ops import fused_wgrad as fw

V256P = 4


def test_variant_table():
    assert fw.VARIANTS[V256P] == (256, 256, 1)
    assert V256P in fw.COLSUM_VARIANTS
    assert fw.VARIANTS[3] == (256, 256, 1) and 3 in fw.COLSUM_VARIANTS


@pytest.mark.parametrize("N,K,split", [(3072, 768, 7), (768, 3072, 7),
                                       (2304, 768, 9), (768, 768, 28)])
def test_choose_split_at_the_workload(N, K, split):
    tn, tk, per_cu = fw.VARIANTS[V256P]
    tiles = (N // tn) * (K // tk)
    assert fw.choose_split(tiles, 65536 // fw.STEP, per_cu) == split


def test_can_use_wants_multiples_of_256_and_64():
    z = lambda *s: torch.zeros(*s, dtype=torch.bfloat16)
    assert not fw.can_use(z(64, 256), z(64, 256), V256P)  # CPU

    class OnDevice(torch.Tensor):
        is_cuda = True

    mk = lambda *s: z(*s).as_subclass(OnDevice)
    assert fw.can_use(mk(64, 256), mk(64, 512), V256P)
    assert not fw.can_use(mk(64, 384), mk(64, 512), V256P)   # N % 256
    assert not fw.can_use(mk(64, 256), mk(64, 640), V256P)   # K % 256
    assert not fw.can_use(mk(96, 256), mk(96, 256), V256P)   # M % 64


def _p_off(row, ch):
    # csrc/wgrad_kernels.hip, p_off()
    return row * 256 + ((ch ^ (((row & 3) << 2) | ((row >> 2) & 3))) << 4)


def test_global_side_swizzle_covers_a_slot_once_and_lands_on_p_off():
    """k_wgrad256p, `lrow`, `lch` and the `dma` lambda: load i of wave w
    fills half panel i >> 1, rows 16 (i & 1) + 4 w .. + 3; lane l writes
    LDS at that base + 16 l and fetches chunk lch of row 16 (i & 1) + lrow."""
    HPANEL = 32 * 256
    seen = {}
    for wave in range(4):
        for lane in range(64):
            lrow = 4 * wave + (lane >> 4)
            lch = (lane & 15) ^ (((lrow & 3) << 2) | ((lrow >> 2) & 3))
            for i in range(8):
                p, r16 = i >> 1, 16 * (i & 1)
                lds = p * HPANEL + r16 * 256 + wave * 1024 + 16 * lane
                row = r16 + lrow          # token row the global address uses
                key = (p, row, lch)
                assert key not in seen, key
                seen[key] = lds
                assert lds == p * HPANEL + _p_off(row, lch)
    assert len(seen) == 4 * 32 * 16
    assert set(seen) == {(p, r, c) for p in range(4) for r in range(32)
                         for c in range(16)}
    # a slot is the lower or upper half of a k_wgrad256 stage: p_off of row
    # r + 32 is p_off of row r plus 32 rows
    assert all(_p_off(r + 32, c) == _p_off(r, c) + 32 * 256
               for r in range(32) for c in range(16))
