"""GPT-2 threads the pending residual delta through its blocks so the add
can ride inside the next LayerNorm.  That must change neither the parameter
layout (the flat shared replica follows `parameters()` order) nor, off the
fused path, a single value."""
import torch

from sharedtensor_amd.models.gpt2 import GPT2, GPT2Config

TINY_PARAMS = [
    ('wte.weight', (256, 64)),
    ('wpe.weight', (64, 64)),
    ('blocks.0.ln1.weight', (64,)),
    ('blocks.0.ln1.bias', (64,)),
    ('blocks.0.attn.qkv.weight', (192, 64)),
    ('blocks.0.attn.qkv.bias', (192,)),
    ('blocks.0.attn.proj.weight', (64, 64)),
    ('blocks.0.attn.proj.bias', (64,)),
    ('blocks.0.ln2.weight', (64,)),
    ('blocks.0.ln2.bias', (64,)),
    ('blocks.0.mlp.fc.weight', (256, 64)),
    ('blocks.0.mlp.fc.bias', (256,)),
    ('blocks.0.mlp.proj.weight', (64, 256)),
    ('blocks.0.mlp.proj.bias', (64,)),
    ('blocks.1.ln1.weight', (64,)),
    ('blocks.1.ln1.bias', (64,)),
    ('blocks.1.attn.qkv.weight', (192, 64)),
    ('blocks.1.attn.qkv.bias', (192,)),
    ('blocks.1.attn.proj.weight', (64, 64)),
    ('blocks.1.attn.proj.bias', (64,)),
    ('blocks.1.ln2.weight', (64,)),
    ('blocks.1.ln2.bias', (64,)),
    ('blocks.1.mlp.fc.weight', (256, 64)),
    ('blocks.1.mlp.fc.bias', (256,)),
    ('blocks.1.mlp.proj.weight', (64, 256)),
    ('blocks.1.mlp.proj.bias', (64,)),
    ('ln_f.weight', (64,)),
    ('ln_f.bias', (64,)),
]


def test_parameter_names_shapes_and_order_unchanged():
    model = GPT2(GPT2Config.tiny())
    got = [(n, tuple(p.shape)) for n, p in model.named_parameters()]
    assert got == TINY_PARAMS


def _old_form_loss(model, idx, targets):
    pos = torch.arange(idx.shape[1])
    x = model.wte(idx) + model.wpe(pos)
    for blk in model.blocks:
        x = x + blk.attn(blk.ln1(x))
        x = x + blk.mlp(blk.ln2(x))
    logits = model.lm_head(model.ln_f(x))
    return torch.nn.functional.cross_entropy(
        logits.view(-1, logits.size(-1)), targets.reshape(-1))


def test_cpu_forward_equals_old_formulation(monkeypatch):
    import sharedtensor_amd.models.gpt2 as gpt2
    torch.manual_seed(3)
    cfg = GPT2Config.tiny()
    model = GPT2(cfg)
    with torch.no_grad():  # zero-initialised biases would hide a dropped one
        for n, p in model.named_parameters():
            if n.endswith("bias"):
                p.normal_(std=0.1)
    tok = torch.randint(0, cfg.vocab_size, (2, 33))
    idx, tgt = tok[:, :-1], tok[:, 1:]
    want = _old_form_loss(model, idx, tgt)
    for flag in (False, True):  # the flag only acts on the fused GPU path
        monkeypatch.setattr(gpt2, "FUSE_PROJ_BIAS", flag)
        _, loss = model(idx, tgt)
        assert loss.item() == want.item()

    # and the gradients, since the residual branch points moved
    model.zero_grad()
    want.backward()
    g_old = [p.grad.clone() for p in model.parameters()]
    model.zero_grad()
    monkeypatch.setattr(gpt2, "FUSE_PROJ_BIAS", False)
    model(idx, tgt)[1].backward()
    for a, p in zip(g_old, model.parameters()):
        assert torch.equal(a, p.grad)
