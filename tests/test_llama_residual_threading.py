"""Llama threads the pending residual delta through its blocks so the add can
ride inside the next RMSNorm.  That must change neither the parameter layout
(the flat shared replica follows `parameters()` order) nor, off the fused
path, a single value."""
import torch
import torch.nn.functional as F

from sharedtensor_amd.models.llama import Llama, LlamaConfig


def _block(i):
    p = f'blocks.{i}.'
    return [
        (p + 'attn_norm.weight', (64,)),
        (p + 'attn.wq.weight', (64, 64)),
        (p + 'attn.wk.weight', (32, 64)),
        (p + 'attn.wv.weight', (32, 64)),
        (p + 'attn.wo.weight', (64, 64)),
        (p + 'mlp_norm.weight', (64,)),
        (p + 'mlp.w1.weight', (128, 64)),
        (p + 'mlp.w3.weight', (128, 64)),
        (p + 'mlp.w2.weight', (64, 128)),
    ]


TINY_PARAMS = ([('tok.weight', (256, 64))] + _block(0) + _block(1)
               + [('norm.weight', (64,)), ('lm_head.weight', (256, 64))])


def test_parameter_names_shapes_and_order_unchanged():
    model = Llama(LlamaConfig.tiny())
    got = [(n, tuple(p.shape)) for n, p in model.named_parameters()]
    assert got == TINY_PARAMS


def _old_form_loss(model, idx, targets):
    """The model before the delta was threaded, written out.  The
    sub-modules are called one by one, so a block whose forward changed its
    signature or return value cannot hide behind this reference."""
    x = model.tok(idx)
    cos, sin = model._rope_cache(idx.device, x.dtype)
    for blk in model.blocks:
        x = x + blk.attn(blk.attn_norm(x), cos, sin)
        x = x + blk.mlp(blk.mlp_norm(x))
    logits = model.lm_head(model.norm(x))
    return F.cross_entropy(logits.float().view(-1, logits.size(-1)),
                           targets.reshape(-1))


def test_cpu_forward_and_grads_equal_old_formulation():
    torch.manual_seed(3)
    cfg = LlamaConfig.tiny()
    model = Llama(cfg)
    with torch.no_grad():  # all-ones norm weights would hide a swapped norm
        for n, p in model.named_parameters():
            if n.endswith("norm.weight"):
                p.normal_(mean=1.0, std=0.2)
    tok = torch.randint(0, cfg.vocab_size, (2, 33))
    idx, tgt = tok[:, :-1], tok[:, 1:]

    want = _old_form_loss(model, idx, tgt)
    model.zero_grad()
    want.backward()
    g_old = [p.grad.clone() for p in model.parameters()]

    model.zero_grad()
    _, loss = model(idx, tgt)
    assert loss.item() == want.item()
    loss.backward()
    for (n, p), a in zip(model.named_parameters(), g_old):
        assert torch.equal(a, p.grad), n


def test_block_returns_stream_and_pending_mlp_output():
    """`LlamaBlock.forward(x, cos, sin, delta)` -> (x, m): the stream after
    the attention add, and the MLP output the next norm still has to add."""
    torch.manual_seed(5)
    cfg = LlamaConfig.tiny()
    model = Llama(cfg)
    blk = model.blocks[0]
    x = torch.randn(2, 16, cfg.dim)
    d = torch.randn(2, 16, cfg.dim)
    cos, sin = model._rope_cache(x.device, x.dtype)
    for delta in (None, d):
        x0 = x if delta is None else x + delta
        x1 = x0 + blk.attn(blk.attn_norm(x0), cos, sin)
        m = blk.mlp(blk.mlp_norm(x1))
        got_x, got_m = blk(x, cos, sin, delta)
        assert torch.equal(got_x, x1) and torch.equal(got_m, m)
