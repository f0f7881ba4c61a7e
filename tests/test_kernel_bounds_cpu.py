"""CPU self-test of tests/kernel_bounds.py: the reference formulas evaluated
in fp32 and rounded to bf16 must meet the bound the GPU tests hold the
kernels to, with no exceptions, for every input family; and the bound must
still reject the errors it exists to find (one-pass LayerNorm variance on a
shifted row, a 1 % error in a constant).  For the wave-per-row add+LayerNorm
and add+RMSNorm kernels the fp32 evaluation is one in the kernels' own lane
layout and summation order, and the mutants are listed with their tests."""
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


# --------------------------- wave-per-row add+LayerNorm and add+RMSNorm

# the narrowest and the widest instantiation of each kernel, and the widths
# of GPT-2-small and Llama-1B
WAVE_WIDTHS = {"ln": [256, 768, 1024], "rms": [512, 2048, 4096]}
WAVE_CASES = [(op, C) for op in ("ln", "rms") for C in WAVE_WIDTHS[op]]


def _wave_case(op, family, R, C, sentinel=()):
    """Inputs of one backward call as the GPU test builds them: x_new is the
    family's x itself (the delta = None call)."""
    t = kb.add_norm_inputs(op, family, R, C)
    x, w, dy = t["x"], t["w"], t["dy"]
    b = t["b"] if op == "ln" else None
    dres = kb.add_norm_dres(op, family, x, w, dy)
    for r in sentinel:
        dy, dres = dy.clone(), dres.clone()
        dy[r] *= 64
        dres[r] *= 64
    return x, w, b, dy, dres


def _wave_judge(op, got, args, family):
    try:
        kb.check_add_norm(op, got, *args, family, tag=f"add_{op}-emu")
    except AssertionError:
        return False
    return True


def test_wave_depths_are_the_ones_read_off_the_code():
    assert kb.wave_depths("ln", 768) == {"mean": 3 + 2 + 6 + 2,
                                         "var": 12 + 6 + 2, "row": 12 + 6 + 2}
    assert kb.wave_depths("ln", 1024)["var"] == 24 > kb.n_red(1024) == 14
    assert kb.wave_depths("rms", 4096)["var"] == 72 > kb.n_red(4096) == 26
    assert kb.wave_depths("rms", 512) == {"var": 16, "row": 16}


def test_default_depth_leaves_the_block_per_row_slack_as_it_was():
    x, w, b, dy = kb.norm_inputs("randn2", 5, 1280)
    n = kb.n_red(1280)
    a, c = kb.ln_slack(x, w, b, dy), kb.ln_slack(x, w, b, dy, depth=n)
    assert a.keys() == c.keys() and all(torch.equal(a[k], c[k]) for k in a)
    a, c = kb.rms_slack(x, w, dy), kb.rms_slack(x, w, dy, depth=n)
    assert a.keys() == c.keys() and all(torch.equal(a[k], c[k]) for k in a)
    # and a deeper sum widens it
    a, d = kb.ln_slack(x, w, b, dy), kb.ln_slack(x, w, b, dy, depth=2 * n)
    assert (d["mean"] > a["mean"]).all() and (d["dx"] > a["dx"]).all()


@pytest.mark.parametrize("op,C", WAVE_CASES)
@pytest.mark.parametrize("family", kb.ADD_NORM_FAMILIES)
def test_kernel_order_add_norm_meets_bound(family, op, C):
    """Every output of the wave-per-row kernels, evaluated in fp32 in their
    lane layout, butterfly and column-sum order, with and without d_x_new."""
    x, w, b, dy, dres = _wave_case(op, family, 5, C)
    for r in (dres, None):
        got = kb.emu_add_norm(op, x, w, b, dy, r)
        kb.check_add_norm(op, got, x, w, b, dy, r, family,
                          tag=f"add_{op}-emu")
    if family in ("constant", "shifted"):
        # the delta of add_norm_inputs reaches these rows exactly
        t = kb.add_norm_inputs(op, family, 5, C)
        for extra in (0.0, t["dbias"].float()):
            x0 = (x.float() - t["delta"].float() - extra).bfloat16()
            assert torch.equal(
                (x0.float() + t["delta"].float() + extra).bfloat16(), x)


@pytest.mark.parametrize("op,C", [("ln", 256), ("rms", 512)])
def test_kernel_order_add_norm_meets_bound_over_the_row_loop(op, C):
    """4099 rows on a grid of 1024 blocks: a lane adds two rows, the reducer
    1024 partial rows; rows 4096 and 4098 carry 64 times the gradient."""
    R = 4099
    args = _wave_case(op, "randn2", R, C, sentinel=(R - 1, 4096))
    got = kb.emu_add_norm(op, *args)
    kb.check_add_norm(op, got, *args, "sentinel", tag=f"add_{op}-emu")


@pytest.mark.parametrize("op,C", WAVE_CASES)
def test_bound_rejects_dx_rounded_before_the_residual_add(op, C):
    args = _wave_case(op, "dres_cancel", 5, C)
    ref = kb.add_norm_formula(op, *args)
    slack = kb.add_norm_slack(op, *args)
    good = kb.emu_add_norm(op, *args)["dx_total"]
    early = kb.emu_add_norm(op, *args, round_first=True)["dx_total"]
    bad0, _ = kb.violations(good, ref["dx_total"], slack["dx_total"])
    bad1, _ = kb.violations(early, ref["dx_total"], slack["dx_total"])
    print(f"{op} C={C}: rounded first, {int(bad1.sum())} of {bad1.numel()} "
          "outside")
    assert not bad0.any() and bad1.sum() > bad1.numel() // 2
    # the column sum of the residues notices too
    if op == "ln":
        dd = kb.emu_add_norm(op, *args, round_first=True)["ddbias"]
        bad, _ = kb.violations(dd, ref["ddbias"], slack["ddbias"])
        assert bad.sum() > C // 2


def test_bound_rejects_the_reciprocal_of_another_width():
    """1 / 1024 at C = 768 (LayerNorm), 1 / 4096 at C = 2048 (RMSNorm)."""
    for op, C, wrong in (("ln", 768, 1024), ("rms", 2048, 4096)):
        args = _wave_case(op, "randn2", 5, C)
        assert _wave_judge(op, kb.emu_add_norm(op, *args), args, "randn2")
        got = kb.emu_add_norm(op, *args, inv_c=1.0 / wrong)
        for k in got.keys() - {"dbeta"}:   # dbeta is sum(dy): no 1 / C in it
            assert not _wave_judge(op, {k: got[k]}, args, "1/C:" + k), k


@pytest.mark.parametrize("C", WAVE_WIDTHS["ln"])
def test_bound_rejects_one_pass_variance_in_wave_order(C):
    """Held by the fp32 bound on rstd.  Through y the error shows only where
    it exceeds the bf16 ulp y is allowed anyway: it does at C = 768 (rstd off
    by several per cent), not at 256 and 1024, where the sums of squares
    happen to stay nearly exact."""
    args = _wave_case("ln", "shifted", 5, C)
    ref = kb.add_norm_formula("ln", *args)["rstd"]
    assert _wave_judge("ln", kb.emu_add_norm("ln", *args), args, "shifted")
    got = kb.emu_add_norm("ln", *args, one_pass=True)
    rel = float(((got["rstd"].double() - ref) / ref).abs().max())
    print(f"C={C}: one-pass rstd off by {100 * rel:.3g} %")
    assert not _wave_judge("ln", {"rstd": got["rstd"]}, args, "one-pass")
    if C == 768:
        for k in ("y", "dx_total"):
            assert not _wave_judge("ln", {k: got[k]}, args, "one-pass:" + k)


# RMSNorm at C = 4096 is left out: the sum of squares is 72 deep there and the
# derived rstd slack (41 U = 2.4e-6 relative) is wider than what eps moves
@pytest.mark.parametrize("op,C", [c for c in WAVE_CASES if c != ("rms", 4096)])
def test_bound_rejects_dropped_eps_on_constant_rows(op, C):
    """LayerNorm: the variance is exactly 0, so rstd is inf without eps.
    RMSNorm: eps = 1e-5 against a mean square of 2.25 moves rstd of row 0 by
    2.2e-6 relative."""
    args = _wave_case(op, "constant", 5, C)
    assert _wave_judge(op, kb.emu_add_norm(op, *args), args, "constant")
    got = kb.emu_add_norm(op, *args, eps=0.0)
    assert not _wave_judge(op, {"rstd": got["rstd"]}, args, "no-eps")
    if op == "ln":
        assert not _wave_judge(op, {"y": got["y"]}, args, "no-eps")


@pytest.mark.parametrize("op,C", [("ln", 256), ("ln", 1024), ("rms", 512)])
@pytest.mark.parametrize("weight", [0.0, 2.0], ids=["dropped", "doubled"])
@pytest.mark.parametrize("R", [5, 4099])
def test_bound_rejects_a_sentinel_row_dropped_or_doubled(R, weight, op, C):
    last = R - 1
    other = 4096 if R > 4096 else 2
    args = _wave_case(op, "randn2", R, C, sentinel=(last, other))
    sums = ("dgamma", "dbeta", "ddbias") if op == "ln" else ("dgamma",)
    for r in (last, other):
        rw = np.ones(R, np.float32)
        rw[r] = weight
        got = kb.emu_add_norm(op, *args, row_weight=rw)
        ref = kb.add_norm_formula(op, *args)
        slack = kb.add_norm_slack(op, *args)
        for k in sums:
            bad, _ = kb.violations(got[k], ref[k], slack[k])
            assert bad.sum() > C // 2, (k, r, int(bad.sum()))


@pytest.mark.parametrize("op,C", WAVE_CASES)
def test_bound_rejects_dgamma_from_dy_times_w(op, C):
    args = _wave_case(op, "randn2", 5, C)
    ref = kb.add_norm_formula(op, *args)
    slack = kb.add_norm_slack(op, *args)
    got = kb.emu_add_norm(op, *args, dgamma_dyw=True)["dgamma"]
    bad, _ = kb.violations(got, ref["dgamma"], slack["dgamma"])
    assert bad.sum() > C // 2


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


# ----------------------------------------------------- fused cross-entropy

CE_OPTION_SETS = {
    "plain": dict(),
    "ignore": dict(ignore_index=-100),
    "eps": dict(eps=0.1),
    "z": dict(z=1e-4),
    "all": dict(ignore_index=-100, eps=0.1, z=1e-4),
}
GRAD_TOL = dict(rtol=5e-2, atol=1e-4)   # what the CE tests used to rely on


def _ce_case(family, V, opts, R=8):
    x, t = kb.ce_inputs(family, R, V)
    if "ignore_index" in opts:
        t = t.clone()
        t[1::3] = -100
    return x, t


def _ce_judge(got, x, t, family, **opts):
    """ce_check on fp32 CPU results; True when every output is accepted."""
    try:
        kb.ce_check(got, x, t, "ce-fp32cpu", family, **opts)
    except AssertionError:
        return False
    return True


def _ce_f32(x, t, **opts):
    f = kb.ce_formula(x, t, dtype=torch.float32, **opts)
    assert f["dlogits"].dtype == torch.float32
    return {"lse": f["lse"], "loss": f["loss"], "mean": f["mean"],
            "dlogits": _bf16(f["dlogits"])}, f


@pytest.mark.parametrize("V", [13, 1003, 50257])
@pytest.mark.parametrize("opts", CE_OPTION_SETS.values(),
                         ids=CE_OPTION_SETS.keys())
@pytest.mark.parametrize("family", kb.CE_FAMILIES)
def test_fp32_reference_meets_bound_ce(family, opts, V):
    x, t = _ce_case(family, V, opts)
    got, f = _ce_f32(x, t, **opts)
    got["m"] = f["m"]
    for g in (1.0, 0.37):
        if g != 1.0:
            got = {"dlogits": _bf16(kb.ce_formula(
                x, t, g=g, dtype=torch.float32, **opts)["dlogits"])}
        # the tightest layout: the bound of every kernel is at least this
        kb.ce_check(got, x, t, "ce-fp32cpu", f"{family}/V={V}", g=g,
                    BLK=1024, NCHUNK=7, **opts)


@pytest.mark.parametrize("family", kb.CE_FAMILIES)
def test_kernel_order_expsum_meets_bound_ce(family):
    """lse in the <1024, 7> thread layout and summation order at V = 50257,
    and in the 16-chunk one (same row, fewer chunks used)."""
    x, t = kb.ce_inputs(family, 8, 50257)
    for nchunk in (7, 16):
        m, tot, lse = kb.emu_ce_expsum(x, 1024, nchunk)
        loss = (lse.double() - x.double().gather(1, t[:, None]).squeeze(1))
        kb.ce_check({"m": m, "lse": lse, "loss": loss.float()}, x, t,
                    "ce-emu", family, BLK=1024, NCHUNK=nchunk)


def test_n_ce_counts_the_layouts():
    # 7 chunks + expsum8 tree + edge + 6 shuffles + 15 LDS adds
    assert kb.n_ce(50257, 1024, 7) == 7 + 3 + 1 + 6 + 15
    assert kb.n_ce(13, 1024, 7) == 1 + 3 + 1 + 6 + 15
    assert kb.n_ce(131072, 1024, 16) == 16 + 3 + 1 + 6 + 15
    assert kb.n_ce(50257, 256) == 25 + 3 + 1 + 6 + 3
    assert kb.n_ce(50257, 512) == 13 + 3 + 1 + 6 + 7
    assert kb.n_ce_sx(50257, 1024, 7) == 56 + 1 + 6 + 15


def test_ce_row_kinds_follow_the_reference_semantics():
    x, t = kb.ce_inputs("randn3", 8, 13)
    t = t.clone()
    t[2], t[5], t[6] = -100, 13, -3
    ref = kb.ce_formula(x, t, ignore_index=-100, eps=0.1, z=1e-4)
    assert ref["n_valid"] == 5 and torch.isnan(ref["mean"])
    assert ref["loss"][2] == 0 and ref["lse"][2] == 0
    assert torch.isnan(ref["loss"][[5, 6]]).all()
    assert kb.is_plus_zero(ref["dlogits"][[2, 5, 6]])
    none = kb.ce_formula(x, torch.full((8,), -100), ignore_index=-100)
    assert none["n_valid"] == 0 and torch.isnan(none["mean"])
    assert kb.is_plus_zero(none["dlogits"])
    assert kb.f32_inv(0) == float("inf")
    # against the project's own statement of the semantics
    from sharedtensor_amd.ops.fused_ce import cross_entropy_reference
    t[5], t[6] = 1, 2
    ref = kb.ce_formula(x, t, ignore_index=-100, eps=0.1, z=1e-4)
    lt = x.float().requires_grad_(True)
    want = cross_entropy_reference(lt, t, ignore_index=-100,
                                   label_smoothing=0.1, z_loss=1e-4)
    want.backward()
    torch.testing.assert_close(ref["mean"].float(), want.detach(),
                               rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(ref["dlogits"].float(), lt.grad, rtol=1e-4,
                               atol=1e-7)


def test_ce_bound_rejects_what_the_old_tolerance_accepted():
    """A head element written as 0, and the -eps/V term dropped, both at
    V = 50257: torch.testing.assert_close with the tolerance the CE tests
    used lets them through; the bound does not."""
    R, V = 8, 50257
    x, t = kb.ce_inputs("randn3", R, V)
    got, f = _ce_f32(x, t)
    ref = kb.ce_formula(x, t)
    assert _ce_judge(got, x, t, "randn3")
    # row 1 starts 2 bytes past a 16-byte boundary: elements 0..6 are its head
    j = 0 if int(t[1]) != 0 else 1
    zeroed = dict(got, dlogits=got["dlogits"].clone())
    zeroed["dlogits"][1, j] = 0.0
    torch.testing.assert_close(zeroed["dlogits"].float(),
                               ref["dlogits"].float(), **GRAD_TOL)
    assert not _ce_judge(zeroed, x, t, "head-zero")

    opts = dict(eps=0.1)
    got, f = _ce_f32(x, t, **opts)
    ref = kb.ce_formula(x, t, **opts)
    assert _ce_judge(got, x, t, "randn3", **opts)
    gs = kb.f32_inv(R)
    no_b = dict(got, dlogits=_bf16(f["dlogits"] + gs * kb.f32(0.1) / V))
    torch.testing.assert_close(no_b["dlogits"].float(),
                               ref["dlogits"].float(), **GRAD_TOL)
    assert not _ce_judge(no_b, x, t, "no-eps/V", **opts)


def test_ce_bound_rejects_gradient_mutants():
    R, V = 8, 50257
    x, t = kb.ce_inputs("randn3", R, V)
    got, f = _ce_f32(x, t)
    gs = kb.f32_inv(R)

    def mutant(d):
        return dict(got, dlogits=_bf16(d))

    # one body chunk's eight gradients doubled (row 0 has no head)
    d = f["dlogits"].clone()
    d[0, 8 * 1500:8 * 1501] *= 2
    assert not _ce_judge(mutant(d), x, t, "chunk-doubled")
    # the target's -1 one element late
    d = f["dlogits"].clone()
    r = next(i for i in range(R) if int(t[i]) + 1 < V)
    d[r, t[r]] += gs
    d[r, t[r] + 1] -= gs
    assert not _ce_judge(mutant(d), x, t, "hot-late")
    # inv_r = 1 / (R + 1)
    d = f["dlogits"] * (R / (R + 1.0))
    assert not _ce_judge(mutant(d), x, t, "inv_r")


def test_ce_bound_rejects_dropped_z_factor():
    """z = 1e-4 at lse ~ 15 makes the factor 1 + 2*z*lse = 1.003, three
    quarters of the smallest relative bf16 ulp: together with the final
    rounding it leaves the bound in a part of the elements."""
    R, V = 8, 50257
    x, t = kb.ce_inputs("randn3", R, V)
    opts = dict(z=1e-4)
    got, f = _ce_f32(x, t, **opts)
    assert _ce_judge(got, x, t, "randn3", **opts)
    plain = kb.ce_formula(x, t, dtype=torch.float32)["dlogits"]
    ref = kb.ce_formula(x, t, **opts)
    slack = kb.ce_slack(x, t, BLK=1024, NCHUNK=7, **opts)
    bad, _ = kb.violations(_bf16(plain), ref["dlogits"], slack["dlogits"])
    print(f"dropped 2*z*lse: {int(bad.sum())} of {bad.numel()} outside")
    assert bad.sum() > 1000
    assert not _ce_judge(dict(got, dlogits=_bf16(plain)), x, t, "no-z",
                         **opts)


def test_ce_bound_rejects_lse_and_mean_mutants():
    R, V = 8, 50257
    x, t = kb.ce_inputs("randn3", R, V)
    got, f = _ce_f32(x, t)
    # lse off by 2^-10 in one row, and the loss with it
    for k in ("lse", "loss"):
        off = {k: got[k].clone()}
        off[k][5] += 2.0 ** -10
        assert _ce_judge({k: got[k]}, x, t, "randn3")
        assert not _ce_judge(off, x, t, k + "+2^-10")
    # the mean over R instead of n_valid: in the scalar and in the gradient
    opts = dict(ignore_index=-100)
    x, t = _ce_case("randn3", V, opts)
    got, f = _ce_f32(x, t, **opts)
    n_valid = int((t != -100).sum())
    assert n_valid == 5
    assert _ce_judge(got, x, t, "randn3", **opts)
    wrong = dict(got, mean=(f["loss"].sum() / R))
    assert not _ce_judge(wrong, x, t, "mean/R", **opts)
    wrong = dict(got, dlogits=_bf16(f["dlogits"] * (n_valid / R)))
    assert not _ce_judge(wrong, x, t, "inv_count=1/R", **opts)
