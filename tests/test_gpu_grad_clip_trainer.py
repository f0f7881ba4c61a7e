"""max_grad_norm end to end on the GPU: the tiny GPT-2 with bf16 shadow
parameters and fused AdamW, one rank."""
import pytest
import torch

from sharedtensor_amd.models.gpt2 import GPT2, GPT2Config
from sharedtensor_amd.parallel.async_dp import AsyncAdamW, AsyncDPTrainer
from sharedtensor_amd.utils import free_port

pytestmark = pytest.mark.gpu


@pytest.fixture
def trainer():
    torch.cuda.set_device(0)
    torch.manual_seed(1234)
    model = GPT2(GPT2Config.tiny()).to("cuda:0")
    tr = AsyncDPTrainer(model, port_base=free_port(), rank=0, world=1,
                        lr=1e-3, optimizer="adamw", weight_decay=0.01,
                        amp_dtype=torch.bfloat16, param_dtype=torch.bfloat16,
                        max_grad_norm=0.05)
    yield tr
    tr.close()


def batch():
    gen = torch.Generator().manual_seed(7)
    x = torch.randint(0, 256, (2, 33), generator=gen).cuda()
    return x[:, :-1], x[:, 1:]


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def test_clipping_path(trainer):
    tr = trainer
    assert isinstance(tr.opt, AsyncAdamW)
    assert tr.shared.grad_flat.dtype == torch.bfloat16
    assert tr.grad_stats() is None                   # no step yet
    before = tr.shared.values.clone()
    for _ in range(2):
        loss = tr.step(*batch())
        assert torch.isfinite(loss)
        gs = tr.grad_stats()
        print("grad_stats", gs)
        assert gs["grad_norm"] > 0.05 and gs["clip_coef"] < 1
        assert not gs["skipped"] and gs["skipped_steps"] == 0
        # torch's own norm of the same bf16 gradients (fp32 accumulation)
        ref = float(torch.linalg.vector_norm(tr.shared.grad_flat.float()))
        assert abs(gs["grad_norm"] - ref) <= 1e-4 * ref
        assert abs(gs["clip_coef"] * (gs["grad_norm"] + 1e-6) - 0.05) < 1e-6
    assert (tr.shared.values != before).float().mean() > 0.5
    assert torch.equal(bits(tr.shared.shadow),
                       bits(tr.shared.values.to(torch.bfloat16)))


def test_skip_path(trainer):
    tr, sh = trainer, trainer.shared
    tr.step(*batch())
    bufs = (sh.values, sh.shadow, sh.mom_flat, tr.opt.vel_flat)
    snap = [b.clone() for b in bufs]
    sh.grad_flat[12345 % sh.n] = float("inf")
    tr.opt.step()
    gs = tr.grad_stats()
    assert gs["skipped"] and gs["skipped_steps"] == 1 and gs["clip_coef"] == 0
    for b, s in zip(bufs, snap):
        assert torch.equal(bits(b), bits(s))
    # training goes on from the untouched state
    loss = tr.step(*batch())
    assert torch.isfinite(loss)
    gs = tr.grad_stats()
    assert not gs["skipped"] and gs["skipped_steps"] == 1
    assert not torch.equal(bits(sh.values), bits(snap[0]))
