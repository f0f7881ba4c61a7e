"""CPU self-test of tests/kernel_bounds.py: the reference formulas evaluated
in fp32 and rounded to bf16 must meet the bound the GPU tests hold the
kernels to, with no exceptions, for every input family; and the bound must
still reject the errors it exists to find (one-pass LayerNorm variance on a
shifted row, a 1 % error in a constant)."""
import numpy as np
import pytest
import torch

import kernel_bounds as kb


def _bf16(t):
    return t.to(torch.bfloat16)


def test_bf16_ulp():
    v = torch.tensor([1.0, 0.999, 1.999, 2.0, 2.0 ** -126, 2.0 ** -130, 0.0,
                      3e38], dtype=torch.float64)
    want = [2.0 ** -7, 2.0 ** -8, 2.0 ** -7, 2.0 ** -6, 2.0 ** -133,
            2.0 ** -126, 2.0 ** -126, 2.0 ** 120]
    assert kb.bf16_ulp(v).tolist() == want
    # agrees with the spacing torch's own bf16 has
    x = torch.tensor([0.3, 5.0, 1e-3, 7e4], dtype=torch.float64)
    b = _bf16(x)
    nxt = (b.view(torch.int16) + 1).view(torch.bfloat16)
    assert torch.equal(kb.bf16_ulp(b), (nxt.double() - b.double()))


def test_bound_accepts_flush_and_overflow_only_where_it_may():
    ref = torch.tensor([2.0 ** -130, 3.3e38, 3.4e38, 1.0, 1.0],
                       dtype=torch.float64)
    inf = float("inf")
    got = torch.tensor([0.0, 3.3e38, inf, inf, float("nan")],
                       dtype=torch.float64)
    bad, _ = kb.violations(got, ref, torch.zeros(5, dtype=torch.float64))
    assert bad.tolist() == [False, False, False, True, True]


@pytest.mark.parametrize("C", [2, 66, 1280, 4094])
@pytest.mark.parametrize("family", kb.NORM_FAMILIES)
def test_fp32_reference_meets_bound_norms(family, C):
    R = 5
    x, w, b, dy = kb.norm_inputs(family, R, C)
    for op, formula, slack_fn, args in (
            ("ln", kb.ln_formula, kb.ln_slack, (x, w, b, dy)),
            ("rms", kb.rms_formula, kb.rms_slack, (x, w, dy))):
        ref = formula(*args)
        f32 = formula(*args, dtype=torch.float32)
        slack = slack_fn(*args)
        for k in ("y", "dx"):
            kb.assert_bf16(_bf16(f32[k]), ref[k], slack[k], op + "-fp32cpu",
                           k, family)
        for k in ref.keys() - {"y", "dx"}:
            kb.assert_f32(f32[k], ref[k], slack[k], op + "-fp32cpu", k,
                          family)


@pytest.mark.parametrize("C", [2, 66, 514, 1280, 4094])
@pytest.mark.parametrize("family", kb.NORM_FAMILIES)
def test_kernel_order_two_pass_stats_meet_bound(family, C):
    """mean / rstd in the kernel's own thread layout and summation order."""
    x, w, b, _ = kb.norm_inputs(family, 5, C)
    ref = kb.ln_formula(x, w, b)
    slack = kb.ln_slack(x, w, b)
    m, rs = kb.emu_ln_stats(x, one_pass=False)
    kb.assert_f32(m, ref["mean"], slack["mean"], "ln-emu", "mean", family)
    kb.assert_f32(rs, ref["rstd"], slack["rstd"], "ln-emu", "rstd", family)


@pytest.mark.parametrize("C", [66, 4094])
def test_one_pass_variance_violates_bound_on_shifted_row(C):
    """The row 100.0 with every 317th element 100.5: E[x^2] - m^2 in the
    kernel's fp32 summation order puts rstd off by +12.8 % at C = 66 and by
    far more at C = 4094 (the difference cancels to <= 0 and the old guard
    falls back to eps alone); sum((x - m)^2) meets the bound."""
    x, w, b, _ = kb.norm_inputs("shifted", 1, C)
    ref = kb.ln_formula(x, w, b)
    slack = kb.ln_slack(x, w, b)
    tol = slack["rstd"] + kb.U * ref["rstd"]

    _, rs1 = kb.emu_ln_stats(x, one_pass=True)
    rel1 = float((rs1.double() - ref["rstd"]) / ref["rstd"])
    print(f"C={C}: one-pass rstd off by {100 * rel1:+.2f} %")
    assert abs(rel1) > 0.05
    assert float((rs1.double() - ref["rstd"]).abs()) > 10 * float(tol)

    m2, rs2 = kb.emu_ln_stats(x, one_pass=False)
    rel2 = float((rs2.double() - ref["rstd"]) / ref["rstd"])
    print(f"C={C}: two-pass rstd off by {100 * rel2:+.2e} %")
    assert float((rs2.double() - ref["rstd"]).abs()) <= float(tol)

    # and through to y: the bound rejects one, accepts the other
    def y_from(m, rs):
        y = (x.float() - m[:, None]) * rs[:, None] * w.float() + b.float()
        return _bf16(y)
    m1, _ = kb.emu_ln_stats(x, one_pass=True)
    bad1, _ = kb.violations(y_from(m1, rs1), ref["y"], slack["y"])
    bad2, _ = kb.violations(y_from(m2, rs2), ref["y"], slack["y"])
    assert bad1.any() and not bad2.any()


def test_bound_rejects_small_norm_errors():
    """A 1 % error in rstd, a dropped row in dgamma: the old tolerances
    (atol 2e-2 on y, 3e-1 on dgamma) let both pass."""
    x, w, b, dy = kb.norm_inputs("randn2", 7, 66)
    ref = kb.rms_formula(x, w, dy)
    slack = kb.rms_slack(x, w, dy)
    bad, _ = kb.violations(_bf16(ref["y"] * 1.01), ref["y"], slack["y"])
    assert bad.any()
    short = kb.rms_formula(x[:6], w, dy[:6])["dgamma"]
    with pytest.raises(AssertionError):
        kb.assert_f32(short, ref["dgamma"], slack["dgamma"], "rms", "dgamma",
                      "dropped-row")


@pytest.mark.parametrize("dy_kind", ["ones", "pattern"])
def test_fp32_reference_meets_bound_gelu_exhaustive(dy_kind):
    x = kb.all_bf16()
    dy = torch.ones_like(x) if dy_kind == "ones" else kb.dy_pattern(x.numel())
    ref = kb.gelu_formula(x, dy)
    f32 = kb.gelu_formula(x, dy, dtype=torch.float32, clamp=True)
    slack = kb.gelu_slack(x, dy)
    finite_x = torch.isfinite(x.float())
    assert torch.isfinite(f32["dx"][finite_x]).all()
    assert torch.isfinite(ref["dx"][finite_x]).all()
    for k in ("y", "dx"):
        kb.assert_bf16(_bf16(f32[k]), ref[k], slack[k], "gelu-fp32cpu", k,
                       "all-bf16/dy=" + dy_kind)


def test_bound_rejects_wrong_gelu_constant(monkeypatch):
    x = kb.all_bf16()
    dy = torch.ones_like(x)
    ref = kb.gelu_formula(x, dy)
    slack = kb.gelu_slack(x, dy)
    monkeypatch.setattr(kb, "GK", 0.79)
    wrong = kb.gelu_formula(x, dy, dtype=torch.float32, clamp=True)
    for k in ("y", "dx"):
        bad, _ = kb.violations(_bf16(wrong[k]), ref[k], slack[k])
        assert bad.sum() > 100, k


SWIGLU_X3 = [1.0, -1.5, 2.0 ** -100, 3e38, 0.0]


@pytest.mark.parametrize("x3v", SWIGLU_X3)
def test_fp32_reference_meets_bound_swiglu(x3v):
    x1 = kb.all_bf16()
    x3 = torch.full_like(x1, x3v)
    for dy_kind in ("ones", "pattern"):
        dy = (torch.ones_like(x1) if dy_kind == "ones"
              else kb.dy_pattern(x1.numel()))
        ref = kb.swiglu_formula(x1, x3, dy)
        f32 = kb.swiglu_formula(x1, x3, dy, dtype=torch.float32)
        slack = kb.swiglu_slack(x1, x3, dy)
        for k in ("y", "dx1", "dx3"):
            kb.assert_bf16(_bf16(f32[k]), ref[k], slack[k], "swiglu-fp32cpu",
                           k, f"all-bf16/x3={x3v:g}/dy={dy_kind}")


def test_fp32_reference_meets_bound_swiglu_saturation():
    g = torch.Generator().manual_seed(5)
    x1 = _bf16((torch.rand(1 << 16, generator=g) * 200 - 100))
    x3 = _bf16(torch.randn(1 << 16, generator=g))
    dy = _bf16(torch.randn(1 << 16, generator=g))
    ref = kb.swiglu_formula(x1, x3, dy)
    f32 = kb.swiglu_formula(x1, x3, dy, dtype=torch.float32)
    slack = kb.swiglu_slack(x1, x3, dy)
    for k in ("y", "dx1", "dx3"):
        kb.assert_bf16(_bf16(f32[k]), ref[k], slack[k], "swiglu-fp32cpu", k,
                       "|x1|<=100")


def test_exact_sum_inputs_are_exact():
    """Integer-valued bf16 in [-4, 4]: an fp32 sum over 4099 rows stays
    below 2^24, so every summation order gives the fp64 sum bit for bit."""
    g = torch.Generator().manual_seed(1)
    x = _bf16(torch.randint(-4, 5, (4099, 66), generator=g).float())
    ref = x.double().sum(0)
    assert ref.abs().max() * 1 <= 4 * 4099 < 2 ** 24
    for perm in (torch.arange(4099), torch.randperm(4099, generator=g)):
        acc = np.zeros(66, np.float32)
        for r in x.float()[perm].numpy():
            acc = acc + r
        assert np.array_equal(acc.astype(np.float64), ref.numpy())


# ------------------------------------------------------- fused optimizers

LR, B1, B2, MU = 2e-2, 0.9, 0.95, 0.9


def _adamw_args(family, eps, step, n=1003, g=None):
    w, m0, v0, g0, wd = kb.optim_inputs(family, n)
    i1, i2 = kb.bias_corrections(B1, B2, step)
    return (w, m0, v0, g0 if g is None else g, LR, B1, B2, eps, wd, i1, i2)


@pytest.mark.parametrize("step", [1, 10000])
@pytest.mark.parametrize("eps", [1e-8, 1e-6])
@pytest.mark.parametrize("family", kb.OPTIM_FAMILIES)
def test_fp32_reference_meets_bound_adamw(family, eps, step):
    args = _adamw_args(family, eps, step)
    ref = kb.adamw_formula(*args)
    f32 = kb.adamw_formula(*args, dtype=torch.float32)
    slack = kb.adamw_slack(*args)
    for k in ("m", "v", "u"):
        assert f32[k].dtype == torch.float32
        kb.assert_within(f32[k], ref[k], slack[k], "adamw-fp32cpu", k,
                         f"{family}/eps={eps:g}/step={step}")
    if family == "g_huge":          # fp32 range is part of the reference
        assert torch.isinf(ref["v"]).all() and torch.isfinite(ref["u"]).all()
    if family == "zero_g_zero_state":
        wd = args[8]
        assert torch.equal(ref["u"], -kb.f32(LR) * (kb.f32(wd) * args[0].double()))


@pytest.mark.parametrize("step", [1, 10000])
def test_fp32_reference_meets_bound_adamw_all_bf16(step):
    g = kb.all_bf16().float()
    args = _adamw_args("randn", 1e-8, step, n=g.numel(), g=g)
    ref = kb.adamw_formula(*args)
    f32 = kb.adamw_formula(*args, dtype=torch.float32)
    slack = kb.adamw_slack(*args)
    fin = torch.isfinite(g)
    for k in ("m", "v", "u"):
        assert not torch.isfinite(ref[k][~fin]).any()
        assert not torch.isfinite(f32[k][~fin]).any()
        kb.assert_within(f32[k][fin], ref[k][fin], slack[k][fin],
                         "adamw-fp32cpu", k, f"all-bf16/step={step}")


def test_bias_corrections():
    i1, i2 = kb.bias_corrections(B1, B2, 1)
    assert abs(i1 - 10.0) < 1e-5 and abs(i2 - 20.0) < 1e-4
    i1, i2 = kb.bias_corrections(B1, B2, 10000)
    assert i1 == 1.0 and i2 == 1.0


def test_adamw_bound_rejects_wrong_formulas():
    """Decay against the updated weight, a dropped bias correction, a 1e-6
    relative error in m: each leaves the bound."""
    args = list(_adamw_args("zero_g_zero_state", 1e-8, 1))
    ref = kb.adamw_formula(*args)
    slack = kb.adamw_slack(*args)
    w, wd = args[0].double(), kb.f32(args[8])
    u_post = -kb.f32(LR) * wd * (w + ref["u"])      # decay on w + u
    assert ((u_post - ref["u"]).abs() > slack["u"]).sum() > 900
    args = list(_adamw_args("randn", 1e-8, 1))
    ref = kb.adamw_formula(*args)
    slack = kb.adamw_slack(*args)
    no_bc2 = kb.adamw_formula(*args[:10], 1.0)
    assert ((no_bc2["u"] - ref["u"]).abs() > slack["u"]).sum() > 900
    with pytest.raises(AssertionError):
        kb.assert_within(ref["m"] * (1 + 1e-6), ref["m"], slack["m"], "adamw",
                         "m", "perturbed")


@pytest.mark.parametrize("g16", [False, True])
def test_fp32_reference_meets_bound_sgd(g16):
    n = 65536
    _, m0, _, g, _ = kb.optim_inputs("randn", n)
    if g16:
        g = kb.all_bf16().float()
    ref = kb.sgd_formula(m0, g, LR, MU)
    f32 = kb.sgd_formula(m0, g, LR, MU, dtype=torch.float32)
    slack = kb.sgd_slack(m0, g, LR, MU)
    fin = torch.isfinite(g)
    for k in ("m", "u"):
        kb.assert_within(f32[k][fin], ref[k][fin], slack[k][fin],
                         "sgd-fp32cpu", k, "all-bf16" if g16 else "randn")
    with pytest.raises(AssertionError):
        kb.assert_within(ref["u"][fin] * (1 + 1e-6), ref["u"][fin],
                         slack["u"][fin], "sgd", "u", "perturbed")
