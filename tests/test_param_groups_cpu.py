"""Parameter groups of the fused optimizer steps on a CPU engine: the group
table (validation, coalescing, layout), grouped AdamW and SGD against
torch.optim with the equivalent param groups, and the param_groups option
of the optimizers and the trainer.

Tolerances: rtol 1e-5 / atol 1e-6 against torch.optim, those of
tests/test_adamw.py.  The mapping tests are exact: with zero gradients and
zero state AdamW's update is fl32(-lr * (0 + wd * w)), computed here in
numpy fp32, and a group without decay must not move at all.
"""
import numpy as np
import pytest
import torch

from sharedtensor_amd import _core
from sharedtensor_amd.engine import SharedFlat
from sharedtensor_amd.models.gpt2 import GPT2, GPT2Config
from sharedtensor_amd.models.llama import Llama, LlamaConfig
from sharedtensor_amd.parallel import no_decay_groups
from sharedtensor_amd.parallel.async_dp import (AsyncAdamW, AsyncDPTrainer,
                                                AsyncSGD, FlatParamShared)
from sharedtensor_amd.utils import free_port

F32 = np.float32
SIZES = [1, 63, 64, 65, 255, 257, 298]
PATTERN = [0, 1, 2, 1, 0, 2, 1]
SCALES = [1.0, 1.0, 0.25]
DECAYS = [0.01, 0.0, 0.1]
N = sum(SIZES)
LR, BETAS, EPS, MU = 2e-2, (0.9, 0.95), 1e-8, 0.9


def ends_of(sizes):
    return list(np.cumsum(sizes))


def decode(words):
    """The table's int32 words as python values, by the documented layout."""
    w = np.asarray(words, dtype=np.int32)
    n = int(w[0:2].view(np.int64)[0])
    S, G = int(w[2]), int(w[3])
    assert w.size == 4 + 3 * S + 2 * G
    return {"n": n, "S": S, "G": G,
            "seg_end": w[4:4 + 2 * S].view(np.int64).tolist(),
            "seg_group": w[4 + 2 * S:4 + 3 * S].tolist(),
            "lr_scale": w[4 + 3 * S:4 + 3 * S + G].view(F32).tolist(),
            "weight_decay": w[4 + 3 * S + G:].view(F32).tolist()}


# ------------------------------------------------------------------- table

def test_table_layout():
    assert N == 1003
    t = decode(_core.build_group_table(N, ends_of(SIZES), PATTERN, SCALES,
                                       DECAYS))
    assert t == {"n": N, "S": 7, "G": 3, "seg_end": ends_of(SIZES),
                 "seg_group": PATTERN, "lr_scale": [F32(x) for x in SCALES],
                 "weight_decay": [float(F32(x)) for x in DECAYS]}


def test_table_coalesces_adjacent_segments_of_one_group():
    t = decode(_core.build_group_table(10, [1, 3, 6, 7, 10], [0, 0, 1, 0, 0],
                                       [1.0, 2.0], [0.0, 0.5]))
    assert t["S"] == 3 and t["seg_end"] == [3, 6, 10]
    assert t["seg_group"] == [0, 1, 0]
    # the cap counts what is left after merging
    many = _core.GROUP_MAX_SEGMENTS + 5
    t = decode(_core.build_group_table(many, list(range(1, many + 1)),
                                       [0] * many, [1.0], [0.0]))
    assert t["S"] == 1 and t["seg_end"] == [many]


@pytest.mark.parametrize("args", [
    (10, [3, 3, 10], [0, 1, 0], [1, 1], [0, 0]),        # not ascending
    (10, [5, 3, 10], [0, 1, 0], [1, 1], [0, 0]),        # descending
    (10, [0, 10], [0, 1], [1, 1], [0, 0]),              # empty first segment
    (10, [3, 9], [0, 1], [1, 1], [0, 0]),               # ends before n
    (10, [3, 11], [0, 1], [1, 1], [0, 0]),              # ends after n
    (10, [3, 10], [0, 2], [1, 1], [0, 0]),              # group out of range
    (10, [3, 10], [0, -1], [1, 1], [0, 0]),             # negative group
    (10, [3, 10], [0, 1], [1, -0.5], [0, 0]),           # negative lr_scale
    (10, [3, 10], [0, 1], [1, float("nan")], [0, 0]),   # NaN lr_scale
    (10, [3, 10], [0, 1], [1, float("inf")], [0, 0]),   # inf lr_scale
    (10, [3, 10], [0, 1], [1, 1e39], [0, 0]),           # inf once it is fp32
    (10, [3, 10], [0, 1], [1, 1], [0, -1e-3]),          # negative decay
    (10, [3, 10], [0, 1], [1, 1], [0, float("nan")]),   # NaN decay
    (10, [3, 10], [0, 1], [1, 1], [float("inf"), 0]),   # inf decay
    (10, [10], [0], [], []),                            # no group
    (10, [], [], [1], [0]),                             # no segment
    (10, [3, 10], [0], [1], [0]),                       # lengths differ
    (10, [3, 10], [0, 1], [1, 1], [0]),                 # lengths differ
], ids=lambda a: None)
def test_table_rejects(args):
    with pytest.raises(ValueError):
        _core.build_group_table(*args)


def test_table_rejects_too_many_segments():
    cap = _core.GROUP_MAX_SEGMENTS
    assert cap >= 8 * 291                     # Llama-3-8B's tensors, 8 times

    def alternating(S):
        return (S, list(range(1, S + 1)), [i % 2 for i in range(S)],
                [1.0, 1.0], [0.0, 0.0])
    assert decode(_core.build_group_table(*alternating(cap)))["S"] == cap
    with pytest.raises(ValueError):
        _core.build_group_table(*alternating(cap + 1))


@pytest.fixture
def flat():
    sh = SharedFlat("127.0.0.1", free_port(), [N], device="cpu",
                    provision_up=False, expected_children=0)
    sh._start()
    yield sh
    sh.close()


def test_make_group_table_checks_the_total(flat):
    table = flat.make_group_table(SIZES, PATTERN, SCALES, DECAYS)
    assert table.dtype == torch.int32 and decode(table.numpy())["n"] == N
    with pytest.raises(ValueError):
        flat.make_group_table(SIZES[:-1] + [SIZES[-1] + 1], PATTERN, SCALES,
                              DECAYS)
    with pytest.raises(ValueError):
        flat.make_group_table(SIZES[:-1], PATTERN[:-1], SCALES, DECAYS)
    with pytest.raises(TypeError):            # not a table of this object
        flat.fused_sgd_step(torch.zeros(N), torch.zeros(N), LR, MU,
                            groups=table.clone())


def test_update_group_table(flat):
    table = flat.make_group_table(SIZES, PATTERN, SCALES, DECAYS)
    flat.update_group_table(table, lr_scale=[3.0, 2.0, 1.0])
    t = decode(table.numpy())
    assert t["lr_scale"] == [3.0, 2.0, 1.0]
    assert t["weight_decay"] == [float(F32(x)) for x in DECAYS]
    flat.update_group_table(table, weight_decay=[0.5, 0.25, 0.0])
    t = decode(table.numpy())
    assert t["lr_scale"] == [3.0, 2.0, 1.0]
    assert t["weight_decay"] == [0.5, 0.25, 0.0]
    assert t["seg_end"] == ends_of(SIZES) and t["seg_group"] == PATTERN
    for bad in ([1.0, 1.0], [1.0, 1.0, -1.0], [1.0, float("nan"), 1.0]):
        with pytest.raises(ValueError):
            flat.update_group_table(table, lr_scale=bad)


# ----------------------------------------------------- against torch.optim

def torch_groups(p_segments, lr, with_decay):
    groups = []
    for g in range(len(SCALES)):
        d = {"params": [p for p, k in zip(p_segments, PATTERN) if k == g],
             "lr": lr * SCALES[g]}
        if with_decay:
            d["weight_decay"] = DECAYS[g]
        groups.append(d)
    return groups


def test_grouped_adamw_matches_torch_param_groups(flat):
    torch.manual_seed(3)
    init = torch.randn(N)
    grads = [torch.randn(N) for _ in range(5)]
    ps = [torch.nn.Parameter(x.clone()) for x in init.split(SIZES)]
    opt = torch.optim.AdamW(torch_groups(ps, LR, True), betas=BETAS, eps=EPS)
    for g in grads:
        for p, gp in zip(ps, g.split(SIZES)):
            p.grad = gp.clone()
        opt.step()
    want = torch.cat([p.detach() for p in ps])

    table = flat.make_group_table(SIZES, PATTERN, SCALES, DECAYS)
    flat._add_flat(init.clone())
    mom, vel = torch.zeros(N), torch.zeros(N)
    for step, g in enumerate(grads, start=1):
        # weight_decay is ignored under groups: 7.0 would be far off
        flat.fused_adamw_step(mom, vel, g, step, LR, BETAS, EPS, 7.0,
                              groups=table)
    torch.testing.assert_close(flat.values, want, rtol=1e-5, atol=1e-6)
    # the groups matter: one rate and one decay for all is far away
    ungrouped = torch.nn.Parameter(init.clone())
    o2 = torch.optim.AdamW([ungrouped], lr=LR, betas=BETAS, eps=EPS,
                           weight_decay=DECAYS[0])
    for g in grads:
        ungrouped.grad = g.clone()
        o2.step()
    assert (flat.values - ungrouped.detach()).abs().max() > 1e-2


def test_grouped_sgd_matches_torch_param_groups(flat):
    torch.manual_seed(4)
    init = torch.randn(N)
    grads = [torch.randn(N) for _ in range(5)]
    ps = [torch.nn.Parameter(x.clone()) for x in init.split(SIZES)]
    opt = torch.optim.SGD(torch_groups(ps, LR, False), lr=LR, momentum=MU)
    for g in grads:
        for p, gp in zip(ps, g.split(SIZES)):
            p.grad = gp.clone()
        opt.step()
    want = torch.cat([p.detach() for p in ps])

    table = flat.make_group_table(SIZES, PATTERN, SCALES, [0.0] * 3)
    flat._add_flat(init.clone())
    mom = torch.zeros(N)
    for g in grads:
        flat.fused_sgd_step(mom, g, LR, MU, groups=table)
    torch.testing.assert_close(flat.values, want, rtol=1e-5, atol=1e-6)
    moved = (flat.values - init).abs().split(SIZES)
    assert moved[2].mean() < 0.5 * moved[3].mean()      # lr_scale 0.25 vs 1


def test_lr_scale_zero_freezes_the_weights_not_the_state(flat):
    torch.manual_seed(5)
    init, g = torch.randn(N), torch.randn(N)
    table = flat.make_group_table(SIZES, PATTERN, [1.0, 0.0, 1.0], DECAYS)
    flat._add_flat(init.clone())
    mom, vel = torch.zeros(N), torch.zeros(N)
    flat.fused_adamw_step(mom, vel, g, 1, LR, BETAS, EPS, 0.0, groups=table)
    for k, (a, b, m) in enumerate(zip(flat.values.split(SIZES),
                                      init.split(SIZES), mom.split(SIZES))):
        assert (m != 0).all()
        assert torch.equal(a, b) == (PATTERN[k] == 1)


# ------------------------------------------------- optimizers and trainer

def make_trainer(model, **kw):
    kw.setdefault("optimizer", "adamw")
    return AsyncDPTrainer(model, port_base=free_port(), rank=0, world=1,
                          lr=1e-2, amp_dtype=None, **kw)


@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_no_decay_groups_through_the_trainer(family):
    torch.manual_seed(7)
    model = (GPT2(GPT2Config.tiny()) if family == "gpt2"
             else Llama(LlamaConfig.tiny()))
    lr, wd = 1e-2, 0.1
    tr = make_trainer(model, weight_decay=wd,
                      param_groups=no_decay_groups(model, wd))
    try:
        sh = tr.shared
        before = sh.values.clone().numpy()
        sh.grad_flat.zero_()
        tr.opt.step()
        after = sh.values.numpy()
        off, n_small, n_big = 0, 0, 0
        for p in sh.params:
            a, b = before[off:off + p.numel()], after[off:off + p.numel()]
            off += p.numel()
            if p.ndim < 2:
                n_small += 1
                assert a.tobytes() == b.tobytes()
            else:
                n_big += 1
                u = -F32(lr) * (F32(0) + F32(wd) * a)
                want = a + u
                assert u.dtype == F32 and want.dtype == F32
                np.testing.assert_array_equal(b, want)
                assert (a != b).any()
        assert off == sh.n and n_small > 0 and n_big > 0
        # the gains are 1.0: under the single decay they would have moved
        gains = [p for p in sh.params if p.ndim < 2 and bool((p == 1).all())]
        assert gains
        groups = tr.opt.param_groups
        assert [g["weight_decay"] for g in groups] == [wd, 0.0]
        assert sum(g["numel"] for g in groups) == sh.n
        by_name = dict(model.named_parameters())
        assert all(by_name[nm].ndim < 2 for nm in groups[1]["names"])
        assert all(by_name[nm].ndim >= 2 for nm in groups[0]["names"])
    finally:
        tr.close()


def test_tied_parameter_is_one_parameter():
    model = GPT2(GPT2Config.tiny())
    assert model.lm_head.weight is model.wte.weight
    tr = make_trainer(model, weight_decay=0.1, param_groups=[
        {"params": ["lm_head.weight"], "lr_scale": 0.5}])
    try:
        g0, rest = tr.opt.param_groups
        assert g0["numel"] == model.lm_head.weight.numel()
        assert g0["lr_scale"] == 0.5 and g0["weight_decay"] == 0.1
        assert rest["lr_scale"] == 1.0 and rest["weight_decay"] == 0.1
        assert g0["numel"] + rest["numel"] == tr.shared.n
    finally:
        tr.close()
    model = GPT2(GPT2Config.tiny())
    with pytest.raises(ValueError):           # both names of the tied tensor
        make_trainer(model, param_groups=[
            {"params": ["lm_head.weight", "wte.weight"]}])


@pytest.fixture
def lin_shared():
    torch.manual_seed(11)
    lin = torch.nn.Linear(37, 29)
    sh = FlatParamShared(lin, "127.0.0.1", free_port(), 0, 1,
                         expected_children=0)
    yield lin, sh
    sh.close()


def test_param_groups_errors(lin_shared):
    lin, sh = lin_shared
    with pytest.raises(ValueError):           # listed twice, by object + name
        AsyncAdamW(sh, param_groups=[{"params": [lin.weight]},
                                     {"params": ["weight"]}])
    with pytest.raises(ValueError):           # twice in one group
        AsyncAdamW(sh, param_groups=[{"params": ["bias", "bias"]}])
    with pytest.raises(ValueError):           # unknown name
        AsyncAdamW(sh, param_groups=[{"params": ["no.such.weight"]}])
    with pytest.raises(ValueError):           # a parameter of another model
        AsyncAdamW(sh, param_groups=[
            {"params": [torch.nn.Parameter(torch.zeros(3))]}])
    with pytest.raises(ValueError):           # empty group
        AsyncAdamW(sh, param_groups=[{"params": []}])
    with pytest.raises(ValueError):           # negative decay
        AsyncAdamW(sh, param_groups=[{"params": ["bias"],
                                      "weight_decay": -0.1}])
    with pytest.raises(ValueError):           # SGD does not decay
        AsyncSGD(sh, param_groups=[{"params": ["bias"],
                                    "weight_decay": 0.1}])
    opt = AsyncSGD(sh, param_groups=[{"params": ["bias"], "lr_scale": 2.0}])
    assert [g["weight_decay"] for g in opt.param_groups] == [0.0, 0.0]
    with pytest.raises(ValueError):
        opt.set_group(0, weight_decay=0.1)


def test_set_group_changes_the_next_step_only(lin_shared):
    lin, sh = lin_shared
    lr, wd = 1e-2, 0.1
    opt = AsyncAdamW(sh, lr=lr, weight_decay=wd,
                     param_groups=[{"params": ["bias"], "weight_decay": 0.0}])
    assert [g["names"] for g in opt.param_groups] == [["bias"], ["weight"]]
    nw = lin.weight.numel()

    def step():
        before = sh.values.clone().numpy()
        sh.grad_flat.zero_()
        opt.step()
        return before, sh.values.numpy().copy()

    a, b = step()
    np.testing.assert_array_equal(b[nw:], a[nw:])                  # bias
    np.testing.assert_array_equal(
        b[:nw], a[:nw] + -F32(lr) * (F32(0) + F32(wd) * a[:nw]))
    opt.set_group(0, weight_decay=0.5)
    opt.set_group(1, lr_scale=0.25)
    assert opt.param_groups[0]["weight_decay"] == 0.5
    assert opt.param_groups[1]["lr_scale"] == 0.25
    assert opt.param_groups[1]["weight_decay"] == wd
    np.testing.assert_array_equal(sh.values.numpy(), b)     # nothing moved
    a, b = step()
    np.testing.assert_array_equal(
        b[nw:], a[nw:] + -F32(lr) * (F32(0) + F32(0.5) * a[nw:]))
    lr_w = F32(lr) * F32(0.25)
    np.testing.assert_array_equal(
        b[:nw], a[:nw] + -lr_w * (F32(0) + F32(wd) * a[:nw]))


@pytest.mark.parametrize("optimizer", ["adamw", "sgd"])
def test_default_is_one_group_and_the_ungrouped_path(optimizer, monkeypatch):
    model = GPT2(GPT2Config.tiny())
    tr = make_trainer(model, optimizer=optimizer,
                      weight_decay=0.01 if optimizer == "adamw" else 0.0)
    try:
        (g,) = tr.opt.param_groups
        assert g["numel"] == tr.shared.n and g["lr_scale"] == 1.0
        assert g["weight_decay"] == (0.01 if optimizer == "adamw" else 0.0)
        assert len(g["names"]) == len(tr.shared.params)
        with pytest.raises(ValueError):
            tr.opt.set_group(0, lr_scale=0.5)
        seen = []
        name = "fused_adamw" if optimizer == "adamw" else "fused_sgd"
        real_step = getattr(tr.shared, name + "_step")
        engine = tr.shared._eng
        real_eng = getattr(engine, name)

        class Eng:
            def __getattr__(self, attr):
                return getattr(engine, attr)

        def spy_step(*a, **kw):
            seen.append(("step", kw.get("groups", "missing")))
            return real_step(*a, **kw)

        def spy_eng(*a):
            seen.append(("engine", a[-1]))
            return real_eng(*a)

        eng = Eng()
        setattr(eng, name, spy_eng)
        monkeypatch.setattr(tr.shared, name + "_step", spy_step)
        monkeypatch.setattr(tr.shared, "_eng", eng)
        tr.opt.step()
        # None from the optimizer, the null pointer into the engine
        assert seen == [("step", None), ("engine", 0)]
    finally:
        monkeypatch.undo()
        tr.close()
