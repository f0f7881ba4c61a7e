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
