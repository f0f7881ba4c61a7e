"""ops/fused_wgrad.py without a GPU, for the 256 x 256 variant: the split it
chooses at the workload's shapes, what ``can_use`` and ``wgrad`` reject, and
the CPU model graph, which the flag and a bias routed to the kernel leave
as it is."""
import pytest
import torch

from sharedtensor_amd.ops import fused_wgrad as fw

V256 = 3


def test_variant_table():
    assert fw.VARIANTS[V256] == (256, 256, 1)
    assert V256 in fw.COLSUM_VARIANTS
    assert not fw.COLSUM_VARIANTS & {0, 1, 2}
    # the older variants keep their indices, tiles and sizing
    assert [fw.VARIANTS[v] for v in (0, 1, 2)] == \
        [(128, 128, 2), (128, 128, 2), (256, 128, 1)]


@pytest.mark.parametrize("N,K,split", [(3072, 768, 7), (768, 3072, 7),
                                       (2304, 768, 9), (768, 768, 28)])
def test_choose_split_at_the_workload(N, K, split):
    tn, tk, per_cu = fw.VARIANTS[V256]
    tiles = (N // tn) * (K // tk)
    got = fw.choose_split(tiles, 65536 // fw.STEP, per_cu)
    assert got == split
    assert tiles * got <= fw.NUM_CU < tiles * (got + 1)


def test_can_use_wants_multiples_of_256():
    # can_use asks for CUDA tensors first; let the CPU ones through so that
    # the tile test is what decides
    z = lambda *s: torch.zeros(*s, dtype=torch.bfloat16)
    assert not fw.can_use(z(64, 256), z(64, 256), V256)  # CPU

    class OnDevice(torch.Tensor):
        is_cuda = True

    mk = lambda *s: z(*s).as_subclass(OnDevice)
    assert fw.can_use(mk(64, 256), mk(64, 512), V256)
    assert not fw.can_use(mk(64, 384), mk(64, 512), V256)   # N % 256
    assert not fw.can_use(mk(64, 256), mk(64, 640), V256)   # K % 256
    assert not fw.can_use(mk(64, 128), mk(64, 128), V256)
    assert fw.can_use(mk(64, 128), mk(64, 128), 1)
    assert not fw.can_use(mk(96, 256), mk(96, 256), V256)   # M % 64


def test_cpu_model_graph_unchanged_by_flag(monkeypatch):
    from sharedtensor_amd.models import gpt2
    monkeypatch.delenv("SHTENS_FUSED_WGRAD", raising=False)
    calls = []
    monkeypatch.setattr(fw, "linear_wgrad", lambda *a, **k: calls.append(1))
    # every shape wired to the new variant: only the device keeps the CPU
    # model off the op
    monkeypatch.setattr(fw, "TUNED", {(192, 64): V256, (64, 64): V256,
                                      (256, 64): V256, (64, 256): V256})
    torch.manual_seed(1)
    model = gpt2.GPT2(gpt2.GPT2Config.tiny())
    idx = torch.randint(0, 256, (2, 64))
    tgt = torch.randint(0, 256, (2, 64))

    def run(flag):
        monkeypatch.setattr(gpt2, "FUSE_WGRAD", flag)
        model.zero_grad(set_to_none=True)
        _, loss = model(idx, tgt)
        loss.backward()
        names, seen, stack = [], set(), [loss.grad_fn]
        while stack:
            fn = stack.pop()
            if fn is None or fn in seen:
                continue
            seen.add(fn)
            names.append(type(fn).__name__)
            stack.extend(f for f, _ in fn.next_functions)
        return loss.detach().clone(), sorted(names), \
            [p.grad.clone() for p in model.parameters()]

    l_on, g_on, p_on = run(True)
    l_off, g_off, p_off = run(False)
    assert not calls
    assert g_on == g_off and torch.equal(l_on, l_off)
    assert all(torch.equal(a, b) for a, b in zip(p_on, p_off))
