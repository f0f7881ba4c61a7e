"""Cross-entropy options without a GPU: the plain-torch reference helper
against F.cross_entropy, the models' CPU fallback, and argument checks."""
import pytest
import torch
import torch.nn.functional as F

from sharedtensor_amd.models.gpt2 import GPT2, GPT2Config
from sharedtensor_amd.models.llama import Llama, LlamaConfig
from sharedtensor_amd.ops import fused_ce
from sharedtensor_amd.ops.fused_ce import cross_entropy_reference

# both sides are fp32 logsumexp compositions of ~1e3 terms that differ in
# operation order only: a few ulp (2^-23 ~ 1.2e-7) of values of order 1..10
ULP_TOL = dict(rtol=5e-6, atol=1e-6)


def _batch(R=12, V=37, seed=0, mask_every=3):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(R, V, generator=g) * 3
    t = torch.randint(0, V, (R,), generator=g)
    if mask_every:
        t[::mask_every] = -100
    return x, t


def _loss_and_grad(fn, x):
    xg = x.clone().requires_grad_(True)
    loss = fn(xg)
    loss.backward()
    return loss.detach(), xg.grad


@pytest.mark.parametrize("eps", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("ignore,mask_every", [(None, 0), (-100, 3), (-100, 0)])
def test_reference_equals_torch_for_zero_z(eps, ignore, mask_every):
    x, t = _batch(mask_every=mask_every)
    want = _loss_and_grad(lambda v: F.cross_entropy(
        v, t, ignore_index=-100 if ignore is None else ignore,
        label_smoothing=eps), x)
    got = _loss_and_grad(lambda v: cross_entropy_reference(
        v, t, ignore, eps, 0.0), x)
    torch.testing.assert_close(got[0], want[0], **ULP_TOL)
    torch.testing.assert_close(got[1], want[1], **ULP_TOL)


def test_reference_ignore_index_inside_the_vocabulary():
    x, t = _batch(mask_every=0)
    t[1] = 0
    t[5] = 0
    want = F.cross_entropy(x, t, ignore_index=0)
    torch.testing.assert_close(cross_entropy_reference(x, t, 0), want,
                               **ULP_TOL)


def test_reference_with_z_loss_equals_hand_composition():
    x, t = _batch()
    eps, z = 0.1, 0.1
    keep = t != -100

    def hand(v):
        lse = torch.logsumexp(v[keep], dim=-1)
        ce = F.cross_entropy(v[keep], t[keep], label_smoothing=eps)
        return ce + z * (lse ** 2).mean()

    want = _loss_and_grad(hand, x)
    got = _loss_and_grad(
        lambda v: cross_entropy_reference(v, t, -100, eps, z), x)
    torch.testing.assert_close(got[0], want[0], **ULP_TOL)
    torch.testing.assert_close(got[1], want[1], **ULP_TOL)
    assert not bool(got[1][~keep].any())


def test_reference_ignored_rows_do_not_reach_the_result():
    x, t = _batch()
    want = _loss_and_grad(lambda v: cross_entropy_reference(v, t, -100), x)
    for fill in (float("nan"), 1e30):
        y = x.clone()
        y[t == -100] = fill
        got = _loss_and_grad(lambda v: cross_entropy_reference(v, t, -100), y)
        assert torch.equal(got[0], want[0])
        assert torch.equal(got[1], want[1])


def test_reference_all_ignored_and_bad_targets():
    x, t = _batch(mask_every=0)
    loss, grad = _loss_and_grad(lambda v: cross_entropy_reference(
        v, torch.full_like(t, -100), -100), x)
    assert torch.isnan(loss) and not bool(grad.any())

    bad = t.clone()
    bad[2] = x.shape[1]
    bad[7] = -5
    loss, grad = _loss_and_grad(
        lambda v: cross_entropy_reference(v, bad, -100), x)
    assert torch.isnan(loss)
    assert not bool(grad[2].any()) and not bool(grad[7].any())
    as_ignored = bad.clone()
    as_ignored[[2, 7]] = -100
    _, want = _loss_and_grad(
        lambda v: cross_entropy_reference(v, as_ignored, -100), x)
    assert torch.equal(grad, want)


def _masked_tokens(vocab, seed):
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, vocab, (2, 17), generator=g)
    x, y = idx[:, :-1].contiguous(), idx[:, 1:].clone()
    y[:, ::2] = -100
    return x, y


@pytest.mark.parametrize("make", [
    lambda **kw: GPT2(GPT2Config(vocab_size=256, n_layer=2, n_head=2,
                                 n_embd=64, block_size=64, **kw)),
    lambda **kw: Llama(LlamaConfig(vocab_size=256, n_layer=2, n_head=4,
                                   n_kv_head=2, dim=64, ffn_dim=128,
                                   block_size=64, **kw)),
], ids=["gpt2", "llama"])
def test_models_give_the_masked_mean_on_cpu(make):
    torch.manual_seed(0)
    model = make(ignore_index=-100)
    x, y = _masked_tokens(256, 1)
    logits, loss = model(x, y)
    want = F.cross_entropy(logits.reshape(-1, 256).float(), y.reshape(-1),
                           ignore_index=-100)
    torch.testing.assert_close(loss, want, **ULP_TOL)

    torch.manual_seed(0)
    smooth = make(ignore_index=-100, label_smoothing=0.1, z_loss=1e-2)
    logits, loss = smooth(x, y)
    want = cross_entropy_reference(logits.reshape(-1, 256).float(),
                                   y.reshape(-1), -100, 0.1, 1e-2)
    assert torch.equal(loss, want)


def test_default_configs_keep_the_plain_mean():
    x, y = _masked_tokens(256, 2)
    y = y.clamp_min(0)
    torch.manual_seed(0)
    logits, loss = GPT2(GPT2Config.tiny())(x, y)
    assert torch.equal(loss, F.cross_entropy(logits.view(-1, 256),
                                             y.reshape(-1)))
    torch.manual_seed(0)
    logits, loss = Llama(LlamaConfig.tiny())(x, y)
    assert torch.equal(loss, F.cross_entropy(logits.view(-1, 256).float(),
                                             y.reshape(-1)))
    for cfg in (GPT2Config.tiny(), LlamaConfig.tiny()):
        assert (cfg.ignore_index, cfg.label_smoothing, cfg.z_loss) \
            == (None, 0.0, 0.0)


@pytest.mark.parametrize("kw", [
    dict(label_smoothing=1.0), dict(label_smoothing=-0.1),
    dict(label_smoothing=float("nan")), dict(z_loss=-1e-4),
    dict(z_loss=float("inf")), dict(z_loss=float("nan")),
])
def test_bad_options_raise(kw):
    x, t = _batch()
    with pytest.raises(ValueError):
        cross_entropy_reference(x, t, **kw)
    # checked before the tensors are looked at: no GPU needed
    with pytest.raises(ValueError):
        fused_ce.fused_cross_entropy(x, t, **kw)
