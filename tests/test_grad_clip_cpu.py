"""Global-norm gradient clipping on a CPU engine: the clip state of
grad_clip_coef, the clipped and the skipped fused steps, and the trainer
option max_grad_norm.

Bounds.  sumsq: every square of an fp32 value is exact in fp64 and all terms
are non-negative, so any summation order of n terms stays within
n * 2^-53 * sum of the exact sum (math.fsum).  norm and coef: one fp32
rounding of a value recomputed in fp64 from the engine's own sumsq, so 1
fp32 ulp.  The clipped step uses fl32(g * coef), rounded once, wherever the
unclipped step uses g.
"""
import math

import numpy as np
import pytest
import torch

import kernel_bounds as kb
from sharedtensor_amd.models.gpt2 import GPT2, GPT2Config
from sharedtensor_amd.parallel.async_dp import (AsyncAdamW, AsyncDPTrainer,
                                                AsyncSGD, FlatParamShared)
from sharedtensor_amd.utils import free_port

F32 = np.float32


def decode(state):
    w = state.detach().cpu().numpy().copy()
    assert w.dtype == np.int32 and w.shape == (8,)
    return {"sumsq": float(w[0:2].view(np.float64)[0]),
            "norm": w[2:3].view(np.float32)[0],
            "coef": w[3:4].view(np.float32)[0],
            "skip": int(w[4:5].view(np.uint32)[0]),
            "skipped_total": int(w[5:6].view(np.uint32)[0])}


def ulp32(x):
    """Spacing of fp32 at |x| (array or scalar), as fp64."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(F32)
                      ).astype(np.float64)


def check_state(st, g, max_norm):
    """The state against the fp64 reference; returns coef."""
    gd = g.detach().double().cpu().numpy()
    n = gd.size
    ref = math.fsum((gd * gd).tolist())
    assert st["skip"] == 0
    assert abs(st["sumsq"] - ref) <= n * 2.0 ** -53 * ref, (st["sumsq"], ref)
    nrm = math.sqrt(st["sumsq"])
    assert abs(float(st["norm"]) - nrm) <= ulp32(nrm)
    coef = min(1.0, max_norm / (nrm + 1e-6))
    assert abs(float(st["coef"]) - coef) <= ulp32(coef)
    if max_norm >= nrm + 1e-6:
        assert st["coef"] == F32(1.0)
    return st["coef"]


@pytest.fixture
def shared():
    torch.manual_seed(11)
    lin = torch.nn.Linear(37, 29)          # n = 1102, no multiple of anything
    with torch.no_grad():
        # magnitudes in [0.5, 2): see test_fused_sgd_clipped
        for p in lin.parameters():
            sign = torch.where(torch.rand_like(p) < 0.5, -1.0, 1.0)
            p.copy_(sign * (0.5 + 1.5 * torch.rand_like(p)))
    sh = FlatParamShared(lin, "127.0.0.1", free_port(), 0, 1,
                         expected_children=1)
    yield sh
    sh.close()


def set_grad(sh, seed, scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    sh.grad_flat.copy_(torch.randn(sh.n, generator=gen) * scale)
    return sh.grad_flat


@pytest.mark.parametrize("max_norm", [0.5, 3.0, 1e4])
def test_state_against_fp64_reference(shared, max_norm):
    g = set_grad(shared, 1)
    state = shared.grad_clip_coef(g, max_norm)
    assert state.dtype == torch.int32 and state.numel() == 8
    st = decode(state)
    coef = check_state(st, g, max_norm)
    assert (coef < 1) == (max_norm < 30)     # |g| is about sqrt(1102) = 33
    assert st["skipped_total"] == 0
    # the same input gives the same bits, and the buffer is reused
    again = shared.grad_clip_coef(g, max_norm)
    assert again.data_ptr() == state.data_ptr()
    assert decode(again) == st


def test_fused_sgd_clipped(shared):
    """values_after is within 1 fp32 ulp of values_before - lr*fl32(g*coef).
    With momentum 0 and a zero momentum buffer m is exactly g' = fl32(g*coef);
    u = fl32(-lr*g') and values = fl32(before + u) round once each.  The
    weights have magnitude >= 0.5 and |u| <= 0.05 * 6 * coef < 0.06, so
    ulp(u) <= ulp(values)/8 and both roundings together stay below one ulp
    of the result."""
    lr = 0.05
    g = set_grad(shared, 2)
    before = shared.values.clone()
    state = shared.grad_clip_coef(g, 4.0)
    coef = check_state(decode(state), g, 4.0)
    assert 0.01 < coef < 0.5
    delta = shared._link_bufs[0][0]
    delta.zero_()                # it held the seeded weights, still unsent
    shared.fused_sgd_step(shared.mom_flat, g, lr, 0.0, clip_state=state)
    gp = g.numpy() * coef
    assert gp.dtype == np.float32
    np.testing.assert_array_equal(shared.mom_flat.numpy(), gp)
    ref = before.double().numpy() - float(F32(lr)) * gp.astype(np.float64)
    err = np.abs(shared.values.double().numpy() - ref)
    assert (err <= ulp32(ref)).all(), float((err / ulp32(ref)).max())
    # the staged update is the same u
    np.testing.assert_array_equal(delta.numpy(), F32(-lr) * gp)


@pytest.mark.parametrize("opt", ["sgd", "adamw"])
@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_skip_touches_nothing_and_counts(shared, opt, bad):
    gen = torch.Generator().manual_seed(3)
    shared.mom_flat.copy_(torch.randn(shared.n, generator=gen))
    vel = torch.randn(shared.n, generator=gen) ** 2
    delta = shared._link_bufs[0][0]
    delta.copy_(torch.randn(shared.n, generator=gen))

    def step(state):
        if opt == "sgd":
            shared.fused_sgd_step(shared.mom_flat, shared.grad_flat, 0.05,
                                  0.9, clip_state=state)
        else:
            shared.fused_adamw_step(shared.mom_flat, vel, shared.grad_flat, 1,
                                    0.05, weight_decay=0.01,
                                    clip_state=state)

    def snap():
        return [t.clone().view(torch.int32)
                for t in (shared.values, shared.mom_flat, vel, delta)]

    before = snap()
    for k in (1, 2):
        g = set_grad(shared, 4 + k)
        g[shared.n - 1 if k == 1 else 0] = bad
        state = shared.grad_clip_coef(g, 1.0)
        st = decode(state)
        assert st["skip"] == 1 and st["coef"] == 0 and st["skipped_total"] == k
        assert not math.isfinite(st["sumsq"])
        step(state)
        for a, b in zip(snap(), before):
            assert torch.equal(a, b)
    g = set_grad(shared, 9)
    state = shared.grad_clip_coef(g, 1.0)
    st = decode(state)
    assert st["skip"] == 0 and st["skipped_total"] == 2
    step(state)
    after = snap()
    names = ["values", "mom", "vel", "delta"]
    for name, a, b in zip(names, after, before):
        if name == "vel" and opt == "sgd":
            continue
        assert (a != b).float().mean() > 0.99, name


def test_fused_adamw_clipped_within_bound(shared):
    n = shared.n
    w, m0, v0, g, wd = kb.optim_inputs("randn", n, seed=5)
    lr, b1, b2, eps, step = 2e-2, 0.9, 0.95, 1e-8, 3
    shared.values.copy_(w)
    shared.mom_flat.copy_(m0)
    vel = v0.clone()
    shared.grad_flat.copy_(g)
    delta = shared._link_bufs[0][0]
    delta.zero_()
    state = shared.grad_clip_coef(shared.grad_flat, 6.0)
    coef = check_state(decode(state), g, 6.0)
    assert 0.01 < coef < 0.5
    shared.fused_adamw_step(shared.mom_flat, vel, shared.grad_flat, step, lr,
                            (b1, b2), eps, wd, clip_state=state)
    gp = torch.from_numpy(g.numpy() * coef)
    assert gp.dtype == torch.float32
    i1, i2 = kb.bias_corrections(b1, b2, step)
    args = (w, m0, v0, gp, lr, b1, b2, eps, wd, i1, i2)
    ref, slack = kb.adamw_formula(*args), kb.adamw_slack(*args)
    got = {"m": shared.mom_flat, "v": vel, "u": delta}
    for k in ("m", "v", "u"):
        kb.assert_within(got[k], ref[k], slack[k], "adamw-clipped-cpu", k,
                         "randn")


# ------------------------------------------------------------------ trainer

LR_TR = 2.0 ** -7      # a power of two: u = -lr * g' is exact


def make_trainer(**kw):
    torch.manual_seed(1234)
    model = GPT2(GPT2Config.tiny())
    return AsyncDPTrainer(model, port_base=free_port(), rank=0, world=1,
                          lr=LR_TR, amp_dtype=None, optimizer="sgd",
                          momentum=0.0, **kw)


def batch():
    gen = torch.Generator().manual_seed(7)
    x = torch.randint(0, 256, (2, 33), generator=gen)
    return x[:, :-1], x[:, 1:]


@pytest.fixture(scope="module")
def twin():
    """One unclipped step: its gradient norm and its resulting weights."""
    tr = make_trainer()
    try:
        before = tr.shared.values.clone()
        tr.step(*batch())
        assert tr.grad_stats() is None
        g = tr.shared.grad_flat.double()
        return {"before": before, "after": tr.shared.values.clone(),
                "grad": tr.shared.grad_flat.clone(),
                "norm": math.sqrt(math.fsum((g * g).tolist()))}
    finally:
        tr.close()


def test_trainer_clips(twin):
    """The parameter moves by -lr * fl32(coef * g) within 1 fp32 ulp of the
    parameter: lr is a power of two, so u is exact and only
    values = fl32(before + u) rounds (half an ulp of the result)."""
    c = twin["norm"] / 4
    tr = make_trainer(max_grad_norm=c)
    try:
        assert isinstance(tr.opt, AsyncSGD) and tr.opt.max_grad_norm == c
        assert tr.grad_stats() is None            # no step yet
        before = tr.shared.values.clone()
        assert torch.equal(before, twin["before"])
        tr.step(*batch())
        gs = tr.grad_stats()
        assert set(gs) == {"grad_norm", "clip_coef", "skipped",
                           "skipped_steps"}
        g = tr.shared.grad_flat
        assert torch.equal(g, twin["grad"])
        gd = g.double()
        norm = math.sqrt(math.fsum((gd * gd).tolist()))
        assert abs(gs["grad_norm"] - norm) <= ulp32(norm)
        assert gs["clip_coef"] < 1 and not gs["skipped"]
        assert gs["skipped_steps"] == 0
        assert abs(gs["clip_coef"] - c / (norm + 1e-6)) <= ulp32(0.25)
        gp = g.numpy() * F32(gs["clip_coef"])
        ref = before.double().numpy() - LR_TR * gp.astype(np.float64)
        after = tr.shared.values.double().numpy()
        err = np.abs(after - ref)
        assert (err <= ulp32(after)).all()
        assert (after != before.double().numpy()).mean() > 0.5
    finally:
        tr.close()


def test_trainer_without_clipping_is_the_twin(twin):
    tr = make_trainer(max_grad_norm=None)
    try:
        assert tr.opt.max_grad_norm is None
        tr.step(*batch())
        assert tr.grad_stats() is None
        assert torch.equal(tr.shared.values.view(torch.int32),
                           twin["after"].view(torch.int32))
    finally:
        tr.close()


def test_trainer_adamw_skips_non_finite_step():
    torch.manual_seed(5)
    tr = AsyncDPTrainer(GPT2(GPT2Config.tiny()), port_base=free_port(),
                        rank=0, world=1, lr=1e-3, amp_dtype=None,
                        optimizer="adamw", max_grad_norm=1.0)
    try:
        assert isinstance(tr.opt, AsyncAdamW)
        tr.step(*batch())
        sh = tr.shared
        snap = [t.clone() for t in (sh.values, sh.mom_flat, tr.opt.vel_flat)]
        sh.grad_flat[17] = float("inf")
        tr.opt.step()
        gs = tr.grad_stats()
        assert gs["skipped"] and gs["skipped_steps"] == 1
        assert gs["clip_coef"] == 0
        for a, b in zip((sh.values, sh.mom_flat, tr.opt.vel_flat), snap):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        assert tr.opt.step_count == 2    # documented: the host still counts
        loss = tr.step(*batch())
        assert torch.isfinite(loss)
        gs = tr.grad_stats()
        assert not gs["skipped"] and gs["skipped_steps"] == 1
    finally:
        tr.close()


@pytest.mark.parametrize("bad", [0, -1, float("inf"), float("nan")])
def test_bad_max_grad_norm_raises(bad, shared):
    with pytest.raises(ValueError):
        AsyncSGD(shared, max_grad_norm=bad)
    with pytest.raises(ValueError):
        AsyncAdamW(shared, max_grad_norm=bad)
    with pytest.raises(ValueError):
        shared.grad_clip_coef(shared.grad_flat, bad)
    with pytest.raises(ValueError):       # the native check, before any work
        shared._eng.grad_clip_coef(shared.grad_flat.data_ptr(), False,
                                   shared.n, float(bad), 0, 0, 0)
    with pytest.raises(ValueError):
        # raised before the engine is created: nothing to close
        AsyncDPTrainer(torch.nn.Linear(2, 2), port_base=1, rank=0, world=1,
                       max_grad_norm=bad)
