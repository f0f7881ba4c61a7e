"""ops/fused_wgrad.py without a GPU: the plain-torch path of ``linear_wgrad``
equals ``F.linear``'s own gradients, the model graph on the CPU does not
change with the flag, and the split arithmetic (the same the kernel does)
covers every 64-token step exactly once."""
import pytest
import torch
import torch.nn.functional as F

from sharedtensor_amd.ops import fused_wgrad as fw


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("shape", [(3, 5, 16), (7, 16)])
def test_fallback_equals_linear_autograd(shape, bias):
    torch.manual_seed(0)
    x = torch.randn(*shape, requires_grad=True)
    w = torch.randn(24, 16, requires_grad=True)
    b = torch.randn(24, requires_grad=True) if bias else None
    dy = torch.randn(*shape[:-1], 24)
    ins = (x, w) + ((b,) if bias else ())
    want = torch.autograd.grad(F.linear(x, w, b), ins, dy)
    y = fw.linear_wgrad(x, w, b)
    assert torch.equal(y, F.linear(x, w, b))
    got = torch.autograd.grad(y, ins, dy)
    for g, r in zip(got, want):
        assert g.shape == r.shape and g.dtype == r.dtype
        torch.testing.assert_close(g, r, rtol=1e-5, atol=1e-5)


def test_detached_bias_gets_no_gradient():
    x = torch.randn(4, 16, requires_grad=True)
    w = torch.randn(8, 16, requires_grad=True)
    b = torch.randn(8, requires_grad=True)
    fw.linear_wgrad(x, w, b.detach()).sum().backward()
    assert b.grad is None and w.grad is not None and x.grad is not None


def test_cpu_model_graph_unchanged_by_flag(monkeypatch):
    from sharedtensor_amd.models import gpt2
    monkeypatch.delenv("SHTENS_FUSED_WGRAD", raising=False)
    calls = []
    monkeypatch.setattr(fw, "linear_wgrad",
                        lambda *a, **k: calls.append(1))
    # every shape "tuned": only the device keeps the CPU model off the op
    monkeypatch.setattr(fw, "TUNED", {(192, 64): 0, (64, 64): 0,
                                      (256, 64): 0, (64, 256): 0})
    torch.manual_seed(1)
    model = gpt2.GPT2(gpt2.GPT2Config.tiny())
    idx = torch.randint(0, 256, (2, 64))
    tgt = torch.randint(0, 256, (2, 64))

    def run(flag):
        monkeypatch.setattr(gpt2, "FUSE_WGRAD", flag)
        model.zero_grad(set_to_none=True)
        _, loss = model(idx, tgt)
        loss.backward()
        names = []
        seen, stack = set(), [loss.grad_fn]
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


def test_wired_needs_cuda_bf16_and_a_tuned_shape():
    x = torch.zeros(2, 64, 768, dtype=torch.bfloat16)
    w = torch.zeros(768, 768, dtype=torch.bfloat16, requires_grad=True)
    assert (768, 768) in fw.TUNED
    assert not fw.wired(x, w)                       # CPU
    assert not fw.can_use(torch.zeros(64, 768, dtype=torch.bfloat16),
                          torch.zeros(64, 768, dtype=torch.bfloat16))
    with pytest.raises(ValueError):
        fw.wgrad(torch.zeros(64, 128), torch.zeros(64, 128))


@pytest.mark.parametrize("steps", [1, 5, 1024])
@pytest.mark.parametrize("split", [1, 3, 7, 8, 28])
def test_split_ranges_cover_every_step_once(steps, split):
    ranges = fw.split_ranges(steps, split)
    assert len(ranges) == split
    covered = []
    for begin, count in ranges:
        assert count >= 0
        covered.extend(range(begin, begin + count))
    assert covered == list(range(steps))            # in order, exactly once
    counts = [c for _, c in ranges]
    assert max(counts) - min(counts) <= 1
    assert counts == sorted(counts, reverse=True)   # longer ranges first


def test_split_ranges_examples():
    assert [c for _, c in fw.split_ranges(5, 3)] == [2, 2, 1]
    assert [c for _, c in fw.split_ranges(5, 8)] == [1, 1, 1, 1, 1, 0, 0, 0]


def test_choose_split_fills_but_never_exceeds_the_slots():
    for tiles in [9, 36, 108, 144, 600]:
        for per_cu in [1, 2, 3]:
            for steps in [1, 5, 1024]:
                s = fw.choose_split(tiles, steps, per_cu)
                assert 1 <= s <= max(1, steps)
                slots = fw.NUM_CU * per_cu
                if tiles <= slots:
                    assert tiles * s <= slots
                    assert s == steps or tiles * (s + 1) > slots
                else:
                    assert s == 1
    # the workload: attn.proj and attn.qkv at 1024 steps
    assert fw.choose_split(36, 1024, 2) == 14
    assert fw.choose_split(108, 1024, 2) == 4
