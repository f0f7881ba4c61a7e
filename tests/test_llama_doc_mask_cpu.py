"""Document masks of packed batches on the CPU path: the doc_start / doc_end
helper of ops/fused_gqa_attn.py against a plain loop, and Llama.forward with
doc_ids against the same model run with a hand-written fp32 attention under
the dense mask (absolute RoPE positions in both, as the model keeps them)."""
import pytest
import torch

from sharedtensor_amd.models import llama
from sharedtensor_amd.ops import fused_gqa_attn as fg

LAYOUTS = [[17], [129], [1] * 5, [20, 12, 33], [64, 64, 64],
           [70, 130, 1, 119], [200, 3]]


def _ids(*rows):
    return torch.tensor([[d for d, n in enumerate(row) for _ in range(n)]
                         for row in rows])


@pytest.mark.parametrize("layout", LAYOUTS, ids=str)
def test_doc_start_end_against_loop(layout):
    ids = _ids(layout, layout[::-1]) + 3  # ids need not start at 0
    start, end = fg.doc_start_end(ids)
    assert start.dtype == end.dtype == torch.int32
    for b, row in enumerate((layout, layout[::-1])):
        edges = [sum(row[:i]) for i in range(len(row) + 1)]
        for lo, hi in zip(edges, edges[1:]):
            assert (start[b, lo:hi] == lo).all() and (end[b, lo:hi] == hi).all()


@pytest.mark.parametrize("bad", [torch.tensor([[0, 1, 0]]),
                                 torch.zeros(4), torch.zeros(1, 4)])
def test_doc_start_end_rejects(bad):
    with pytest.raises(ValueError):
        fg.doc_start_end(bad)


def _model():
    torch.manual_seed(0)
    cfg = llama.LlamaConfig.tiny()
    return llama.Llama(cfg), torch.randint(0, cfg.vocab_size, (2, 48))


def test_doc_ids_against_hand_written_dense_mask(monkeypatch):
    model, idx = _model()
    ids = _ids([20, 1, 27], [5, 43])
    got, _ = model(idx, doc_ids=ids)
    vis = (ids[:, :, None] == ids[:, None, :]) & torch.ones(48, 48).bool().tril()

    def attention(q, k, v, **kw):
        g = q.shape[1] // k.shape[1]
        k, v = (t.repeat_interleave(g, dim=1) for t in (k, v))
        s = (q @ k.transpose(-1, -2)) / q.shape[-1] ** 0.5
        return torch.softmax(s.masked_fill(~vis[:, None], float("-inf")), -1) @ v

    monkeypatch.setattr(llama.F, "scaled_dot_product_attention", attention)
    ref, _ = model(idx)
    # fp32 on both sides, a few hundred operations per logit: 2^-24 each
    torch.testing.assert_close(got, ref, rtol=1e-4, atol=1e-6)
    # and the mask matters: the plain causal logits are not these
    monkeypatch.undo()
    assert not torch.allclose(model(idx)[0], ref, rtol=1e-2, atol=1e-4)


def test_no_doc_ids_is_the_plain_causal_call(monkeypatch):
    model, idx = _model()
    calls = []
    real = llama.F.scaled_dot_product_attention
    monkeypatch.setattr(
        llama.F, "scaled_dot_product_attention",
        lambda *a, **kw: (calls.append(kw), real(*a, **kw))[1])
    a, _ = model(idx)
    b, _ = model(idx, None, None)
    assert torch.equal(a, b)
    assert calls and all(kw.get("is_causal") and "attn_mask" not in kw
                         for kw in calls)
