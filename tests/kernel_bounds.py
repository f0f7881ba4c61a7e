"""fp64 references and derived error bounds for the bf16 model kernels
(block-per-row LayerNorm / RMSNorm, colsum, GELU, SwiGLU), for the fused
fp32 optimizers (AdamW, SGD momentum) and, at the end of the file, for the
fused cross-entropy kernels.

Reference: the same formula evaluated in fp64 on the bf16 inputs; backward
references use fp64 statistics, never the kernel's saved mean / rstd.

Bound for a bf16 output element:

    |got - ref| <= 1 bf16 ulp at |ref| + slack

One ulp = half an ulp for the final round-to-nearest-even + half an ulp for
a rounding that fp32 error flipped.  Below the smallest normal bf16 (2^-126)
the allowance is 2^-126 itself, so a flushed subnormal is accepted.  `slack`
is the running-error bound of an fp32 evaluation, n * 2^-24 * sum|terms|,
computed here in fp64 next to the reference: it is derived from the formula
and the reduction depth, not measured.  fp32 outputs (mean, rstd, dgamma,
dbeta, colsum) are held to the slack alone.

Reduction depth.  A row statistic is summed by 256 threads: each adds its
ceil(C/512) bf16 pairs serially (2 adds per pair), then 6 shuffle levels and
3 LDS adds, then one divide: n_red(C) = 2*ceil(C/512) + 10.  Column sums
over R rows are bounded for any order (serial, atomics): n = R + 3.

Transcendentals.  tanhf is given 4 fp32 ulps of its value.  The fast exp is
exp2(x * log2(e)) with the product rounded to fp32, a relative error of
|x| * 2^-24 in the result, plus 3 ulps for the exp2 and the constant.  A
sigmoid below the smallest normal fp32 may flush or saturate to 0 (exp
overflows to inf at x < -88.7), an absolute error of 2^-126 that the
multiplications by x1, x3 and dy then scale.

Every formula below takes a dtype, so the CPU self-test can run the very
same code in fp32, round to bf16 and push it through the bound: a bound the
fp32 evaluation of the reference cannot meet would be one no kernel can.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24            # fp32 unit roundoff
ETA = 2.0 ** -126         # smallest normal fp32 (and bf16)
BF16_MIN_NORMAL = 2.0 ** -126
BF16_MAX = float(torch.finfo(torch.bfloat16).max)
TANH_ULPS = 4.0
GK = math.sqrt(2.0 / math.pi)
GC = 0.044715
EPS = 1e-5
EPS32 = float(np.float32(EPS))  # what the kernel receives


def n_red(C: int) -> int:
    return 2 * math.ceil(C / 512) + 10


# ------------------------------------------------------------------ bound

def bf16_ulp(ref: torch.Tensor) -> torch.Tensor:
    """Spacing of bf16 (8 significant bits) at |ref|; 2^-126 below the
    smallest normal."""
    a = ref.double().abs()
    _, e = torch.frexp(a.clamp_min(BF16_MIN_NORMAL))  # a = m * 2^e, m in [.5, 1)
    ulp = torch.ldexp(torch.ones_like(a), e - 8)
    return torch.where(a < BF16_MIN_NORMAL,
                       torch.full_like(a, BF16_MIN_NORMAL), ulp)


def violations(got, ref, slack, ulps=1.0):
    """Boolean mask of elements outside the bound, and the largest error in
    bf16 ulps over the finite elements.  A NaN reference is not judged, an
    infinite one must be met exactly, and a finite one within reach of the
    bf16 maximum may come out as the infinity of its sign."""
    got = got.double()
    ref = ref.double()
    ulp = bf16_ulp(ref)
    tol = ulps * ulp + slack
    err = (got - ref).abs()
    ok = err <= tol
    inf = torch.full_like(ref, float("inf")).copysign(ref)
    ok |= (ref.abs() + tol >= BF16_MAX) & (got == inf)
    ok = torch.where(torch.isinf(ref), got == ref, ok)
    ok |= torch.isnan(ref)
    # reported figure: elements whose slack is below one ulp, where the
    # bf16 ulp is the meaningful unit (an ill-conditioned element, such as
    # silu(-90) * 3e38, is judged by its slack and says nothing in ulps)
    judged = torch.isfinite(ref) & torch.isfinite(got) & (slack <= ulp)
    worst = float((err / ulp)[judged].max()) if judged.any() else 0.0
    return ~ok, worst


def report(op, out, family, worst, unit="bf16ulp"):
    print(f"MAXERR op={op} out={out} family={family} {worst:.4g} {unit}")


def assert_bf16(got, ref, slack, op, out, family, ulps=1.0):
    bad, worst = violations(got, ref, slack, ulps)
    report(op, out, family, worst)
    if bad.any():
        i = tuple(int(v) for v in bad.nonzero()[0])
        g, r = float(got[i]), float(ref[i])
        s = float(slack[i]) if slack.dim() else float(slack)
        raise AssertionError(
            f"{op} {out} [{family}]: {int(bad.sum())} of {bad.numel()} "
            f"elements outside 1 ulp + slack; first at {i}: got {g!r}, "
            f"ref {r!r}, ulp {float(bf16_ulp(ref[i])):.3g}, slack {s:.3g}")
    return worst


def assert_f32(got, ref, slack, op, out, family):
    """fp32 output: slack plus the one fp32 rounding of the stored value."""
    got = got.double()
    ref = ref.double()
    tol = slack + U * ref.abs() + 2.0 ** -149
    err = (got - ref).abs()
    worst = float((err / tol).max()) if err.numel() else 0.0
    report(op, out, family, worst, unit="of-slack")
    bad = ~(err <= tol)
    if bad.any():
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(
            f"{op} {out} [{family}]: {int(bad.sum())} of {bad.numel()} "
            f"outside the fp32 bound; first at {i}: got {float(got[i])!r}, "
            f"ref {float(ref[i])!r}, tol {float(tol[i]):.3g}")
    return worst


# ------------------------------------------------------------ norm formulas

def rms_formula(x, w, dy=None, dtype=torch.float64, eps=EPS32):
    x, w = x.to(dtype), w.to(dtype)
    rs = torch.rsqrt((x * x).mean(-1, keepdim=True) + eps)
    out = {"y": x * rs * w, "rstd": rs.squeeze(-1)}
    if dy is not None:
        g = dy.to(dtype) * w
        t = rs * rs * (g * x).mean(-1, keepdim=True)
        out["dx"] = rs * (g - x * t)
        out["dgamma"] = (dy.to(dtype) * x * rs).sum(0)
    return out


def rms_slack(x, w, dy=None, eps=EPS32):
    """Running-error bounds for rms_formula evaluated in fp32."""
    x, w = x.double(), w.double()
    R, C = x.shape
    n = n_red(C)
    rs = torch.rsqrt((x * x).mean(-1, keepdim=True) + eps)
    # sum of squares: all terms positive, relative error (n + 2)u; the
    # inverse square root halves it; 4u for add, divide and rsqrt
    d_rs = (0.5 * (n + 2) + 4) * U
    y = x * rs * w
    out = {"y": y.abs() * (d_rs + 3 * U), "rstd": (rs * d_rs).squeeze(-1)}
    if dy is not None:
        dy = dy.double()
        g = dy * w
        gx = g * x
        t = rs * rs * gx.mean(-1, keepdim=True)
        t_err = (rs * rs * (n + 3) * U * gx.abs().mean(-1, keepdim=True)
                 + t.abs() * (2 * d_rs + 3 * U))
        mag = g.abs() + (x * t).abs()
        dx = rs * (g - x * t)
        out["dx"] = (rs * (3 * U * mag + x.abs() * t_err) + d_rs * rs * mag
                     + U * dx.abs())
        out["dgamma"] = ((R + 3) * U + d_rs) * (dy * x * rs).abs().sum(0)
    return out


def ln_formula(x, w, b=None, dy=None, dtype=torch.float64, eps=EPS32):
    x, w = x.to(dtype), w.to(dtype)
    m = x.mean(-1, keepdim=True)
    d = x - m
    rs = torch.rsqrt((d * d).mean(-1, keepdim=True) + eps)
    h = d * rs
    y = h * w
    if b is not None:
        y = y + b.to(dtype)
    out = {"y": y, "mean": m.squeeze(-1), "rstd": rs.squeeze(-1)}
    if dy is not None:
        dy = dy.to(dtype)
        g = dy * w
        t1 = g.mean(-1, keepdim=True)
        t2 = (g * h).mean(-1, keepdim=True)
        out["dx"] = rs * (g - t1 - h * t2)
        out["dgamma"] = (dy * h).sum(0)
        out["dbeta"] = dy.sum(0)
    return out


def ln_slack(x, w, b=None, dy=None, eps=EPS32):
    """Running-error bounds for ln_formula evaluated in fp32 (two-pass
    variance)."""
    x, w = x.double(), w.double()
    R, C = x.shape
    n = n_red(C)
    m = x.mean(-1, keepdim=True)
    d = x - m
    var = (d * d).mean(-1, keepdim=True)
    rs = torch.rsqrt(var + eps)
    h = d * rs
    m_err = n * U * x.abs().mean(-1, keepdim=True)
    # (x - m)^2 with m off by m_err, then a sum of positive terms
    var_err = (2 * m_err * d.abs().mean(-1, keepdim=True) + m_err * m_err
               + (n + 3) * U * var)
    rs_err = 0.5 * rs ** 3 * var_err + 3 * U * rs
    h_err = rs * (m_err + U * d.abs()) + d.abs() * rs_err + U * h.abs()
    babs = b.double().abs() if b is not None else 0.0
    out = {"y": w.abs() * h_err + 3 * U * ((h * w).abs() + babs),
           "mean": m_err.squeeze(-1), "rstd": rs_err.squeeze(-1)}
    if dy is not None:
        dy = dy.double()
        g = dy * w
        t1 = g.mean(-1, keepdim=True)
        t2 = (g * h).mean(-1, keepdim=True)
        t1_err = (n + 1) * U * g.abs().mean(-1, keepdim=True)
        t2_err = ((n + 3) * U * (g * h).abs().mean(-1, keepdim=True)
                  + (g.abs() * h_err).mean(-1, keepdim=True))
        inner = g - t1 - h * t2
        inner_err = (t1_err + h.abs() * t2_err + t2.abs() * h_err
                     + 4 * U * (g.abs() + t1.abs() + (h * t2).abs()))
        out["dx"] = (rs * inner_err + rs_err * inner.abs()
                     + U * (rs * inner).abs())
        out["dgamma"] = ((dy.abs() * h_err).sum(0)
                         + (R + 3) * U * (dy * h).abs().sum(0))
        out["dbeta"] = (R + 1) * U * dy.abs().sum(0)
    return out


# ------------------------------------------------- kernel-order emulation

def emu_block_sum(v: np.ndarray) -> np.ndarray:
    """The kernels' block_sum in fp32: v is (..., BLK) per-thread partials
    (BLK = 256, 512 or 1024); a shuffle-down tree inside each 64-lane wave,
    then the wave results in wave order, ((w0+w1)+w2)+w3 ..."""
    waves = v.shape[-1] // 64
    a = v.astype(np.float32).reshape(v.shape[:-1] + (waves, 64)).copy()
    w = 32
    while w:
        a[..., :w] = a[..., :w] + a[..., w:2 * w]
        w >>= 1
    l = a[..., 0]
    t = l[..., 0]
    for i in range(1, waves):
        t = t + l[..., i]
    return t


def emu_ln_stats(x: torch.Tensor, one_pass: bool, eps=EPS32):
    """mean and rstd of each row of bf16 x as k_ln_fwd's thread layout and
    fp32 summation order give them: thread t owns the bf16 pairs t, t+256,
    ...; `one_pass` is the E[x^2] - m^2 form the kernel used to have."""
    f = np.float32
    xs = x.float().numpy().astype(f)
    R, C = xs.shape
    C2 = C // 2
    cpt = (C2 + 255) // 256
    pad = np.zeros((R, cpt * 256, 2), f)
    pad[:, :C2] = xs.reshape(R, C2, 2)
    valid = (np.arange(cpt * 256) < C2).reshape(cpt, 256)
    lo = pad[..., 0].reshape(R, cpt, 256)
    hi = pad[..., 1].reshape(R, cpt, 256)
    s = np.zeros((R, 256), f)
    ss = np.zeros((R, 256), f)
    for k in range(cpt):
        s = s + (lo[:, k] + hi[:, k])
        ss = ss + (lo[:, k] * lo[:, k] + hi[:, k] * hi[:, k])
    m = emu_block_sum(s) / f(C)
    if one_pass:
        var = emu_block_sum(ss) / f(C) - m * m
        arg = np.where(var > 0, var + f(eps), f(eps)).astype(f)
    else:
        ss = np.zeros((R, 256), f)
        for k in range(cpt):
            d0 = lo[:, k] - m[:, None]
            d1 = hi[:, k] - m[:, None]
            ss = ss + np.where(valid[k], d0 * d0 + d1 * d1, f(0)).astype(f)
        arg = (emu_block_sum(ss) / f(C) + f(eps)).astype(f)
    rs = (f(1) / np.sqrt(arg)).astype(f)
    return torch.from_numpy(m), torch.from_numpy(rs)


# --------------------------------------------------------- norm input sets

NORM_FAMILIES = ["randn2", "shifted", "constant", "outlier", "zero_dy",
                 "w_zeros"]


def norm_inputs(family, R, C, seed=0, device="cpu"):
    """bf16 x (R, C), w, b (C), dy (R, C).  Generated on the CPU so the CPU
    self-test and the GPU tests see the same numbers."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * R + C)

    def rn(*shape, scale=1.0):
        return torch.randn(*shape, generator=g) * scale
    x = rn(R, C, scale=2.0)
    w, b, dy = rn(C), rn(C), rn(R, C)
    if family == "shifted":      # |mean| >> std: E[x^2] - m^2 cancels
        x = torch.full((R, C), 100.0)
        x[:, ::317] = 100.5
    elif family == "constant":   # variance exactly 0
        x = (1.5 * torch.arange(1, R + 1.0))[:, None].expand(R, C).clone()
    elif family == "outlier":
        x = rn(R, C)
        x[:, C // 3] = 1e4
    elif family == "zero_dy":
        dy = torch.zeros(R, C)
    elif family == "w_zeros":
        w[::3] = 0.0
    elif family != "randn2":
        raise ValueError(family)
    return tuple(t.to(torch.bfloat16).to(device) for t in (x, w, b, dy))


# -------------------------------------------------------------- elementwise

def all_bf16(device="cpu"):
    """Every bf16 bit pattern, in bit order (65536 values)."""
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    return bits.view(torch.bfloat16).to(device)


def dy_pattern(n, device="cpu"):
    """A fixed second dy: finite, both signs, zeros, 2^-20 .. 2^20."""
    i = torch.arange(n, dtype=torch.float64)
    mant = ((i * 37) % 17 - 8) / 8.0            # -1 .. 1, 0 included
    expo = torch.exp2(((i * 11) % 41) - 20)
    return (mant * expo).to(torch.bfloat16).to(device)


def gelu_formula(x, dy=None, dtype=torch.float64, clamp=False):
    """tanh-approximate GELU.  `clamp` evaluates the derivative at x clamped
    to [-10, 10], where it has long reached 1 or 0: what an fp32 evaluation
    has to do, since x*x overflows for |x| > 1.8e19."""
    x = x.to(dtype)
    t = torch.tanh(GK * (x + GC * x * x * x))
    out = {"y": 0.5 * x * (1 + t)}
    if dy is not None:
        xc = torch.where(x.isnan(), x, x.clamp(-10, 10)) if clamp else x
        x2 = xc * xc
        inner = GK * xc * (1 + GC * x2)
        tc = torch.tanh(inner)
        # fp64 reference: 1/cosh^2 has no cancellation; fp32: as the kernel
        sech2 = (1 - tc * tc) if clamp else 1 / torch.cosh(inner) ** 2
        grad = 0.5 * (1 + tc) + 0.5 * xc * sech2 * GK * (1 + 3 * GC * x2)
        out["dx"] = dy.to(dtype) * grad
    return out


def gelu_slack(x, dy=None):
    x = x.double()
    inner = GK * (x + GC * x * x * x)
    t = torch.tanh(inner)
    sech2 = 1 / torch.cosh(inner) ** 2
    t_err = sech2 * 7 * U * inner.abs() + TANH_ULPS * U * t.abs()
    t_err = torch.where(torch.isfinite(t_err), t_err, TANH_ULPS * U)
    y = 0.5 * x * (1 + t)
    out = {"y": 0.5 * x.abs() * (t_err + U * (1 + t.abs())) + 2 * U * y.abs()}
    if dy is not None:
        # the bound is the one at min(|x|, 10): beyond that the derivative
        # is constant to 1e-36 and no evaluation has to be less accurate
        xc = x.clamp(-10, 10)
        ic = GK * xc * (1 + GC * xc * xc)
        tc = torch.tanh(ic)
        s2 = 1 / torch.cosh(ic) ** 2
        tc_err = s2 * 7 * U * ic.abs() + TANH_ULPS * U * tc.abs()
        a_err = 0.5 * (tc_err + U * (1 + tc.abs()))
        s2_err = 2 * tc.abs() * tc_err + 2 * U       # 1 - t*t, absolute
        p = 0.5 * xc * GK * (1 + 3 * GC * xc * xc)
        b_err = p.abs() * s2_err + 7 * U * (p * s2).abs()
        grad = 0.5 * (1 + tc) + p * s2
        out["dx"] = dy.double().abs() * (a_err + b_err + 2 * U * grad.abs())
    return out


def swiglu_formula(x1, x3, dy=None, dtype=torch.float64):
    a, b = x1.to(dtype), x3.to(dtype)
    sg = 1 / (1 + torch.exp(-a))
    out = {"y": a * sg * b}
    if dy is not None:
        g = dy.to(dtype)
        # bounded factors first: silu'(a) and silu(a) underflow to 0 where
        # dy * x3 or dy * x1 alone would overflow to inf, and inf * 0 = NaN
        out["dx1"] = g * (b * (sg * (1 + a * (1 - sg))))
        out["dx3"] = g * (a * sg)
    return out


def swiglu_slack(x1, x3, dy=None):
    a, b = x1.double(), x3.double()
    sg = 1 / (1 + torch.exp(-a))
    nsg = 1 / (1 + torch.exp(a))                 # 1 - sg without cancellation
    sg_err = sg * nsg * (a.abs() + 3) * U + 2 * U * sg + ETA
    ab = (a * b).abs()
    y = a * sg * b
    out = {"y": ab * sg_err + 2 * U * y.abs()}
    if dy is not None:
        g = dy.double()
        q = 1 + a * nsg
        q_err = a.abs() * (sg_err + U * nsg) + 2 * U * (1 + (a * nsg).abs())
        gb = (g * b).abs()
        out["dx1"] = (gb * (sg_err * q.abs() + sg * q_err)
                      + 3 * U * (g * b * sg * q).abs())
        out["dx3"] = (g * a).abs() * sg_err + 2 * U * (g * a * sg).abs()
    for k, v in out.items():                      # inf * 0 in the bound itself
        out[k] = torch.where(torch.isnan(v), torch.full_like(v, float("inf")),
                             v)
    return out


# ----------------------------------------------- wrapper-level norm checks

def check_ln_wrapper(fused_layer_norm, x, w, b, dy, family, eps=EPS):
    """fused_layer_norm forward + backward on 2-D bf16 inputs against the
    fp64 reference: y, dx, and the bf16 weight gradients, each 1 ulp +
    slack.  Returns the kernel's outputs."""
    xf = x.clone().requires_grad_(True)
    wf = w.clone().requires_grad_(True)
    bf = b.clone().requires_grad_(True) if b is not None else None
    y = fused_layer_norm(xf, wf, bf, eps)
    y.backward(dy)
    ref = ln_formula(x, w, b, dy)
    slack = ln_slack(x, w, b, dy)
    got = {"y": y.detach(), "dx": xf.grad, "dgamma": wf.grad}
    if b is not None:
        got["dbeta"] = bf.grad
    for k, v in got.items():
        assert v.dtype == torch.bfloat16 and v.shape == ref[k].shape, k
        assert_bf16(v, ref[k], slack[k], "ln", k, family)
    return got


def check_rms_wrapper(fused_rms_norm, x, w, dy, family, eps=EPS):
    xf = x.clone().requires_grad_(True)
    wf = w.clone().requires_grad_(True)
    y = fused_rms_norm(xf, wf, eps)
    y.backward(dy)
    ref = rms_formula(x, w, dy)
    slack = rms_slack(x, w, dy)
    got = {"y": y.detach(), "dx": xf.grad, "dgamma": wf.grad}
    for k, v in got.items():
        assert v.dtype == torch.bfloat16 and v.shape == ref[k].shape, k
        assert_bf16(v, ref[k], slack[k], "rms", k, family)
    return got


# ------------------------------------------------------- fused optimizers
#
# k_fused_adamw / k_fused_sgd* evaluate, per element and in fp32,
#
#   m = b1*m0 + (1 - b1)*g
#   v = b2*v0 + (1 - b2)*g*g
#   u = -lr * (m*ibc1 / (sqrt(v*ibc2) + eps) + wd*w)          (AdamW)
#
#   m = mu*m0 + g;  u = -lr*m                                  (SGD momentum)
#
# The references below evaluate the same expressions in fp64 on the fp32
# values the kernel receives (hyperparameters rounded to fp32 first).  The
# bounds count the roundings on the path to each term, k of them giving
# gamma(k) = k*U / (1 - k*U) times the term's magnitude; a rounding that
# lands below 2^-126 adds at most SUB = 2^-149 instead.  A contracted
# multiply-add drops one of the counted roundings, so the bound holds with
# or without contraction.  Division and square root are taken as correctly
# rounded (the build passes no fast-math flag), one rounding each.
#
# fp32 range is part of the reference: a term beyond FLT_MAX is +-inf, as
# it is in any fp32 evaluation (g = 1e20 makes (1 - b2)*g*g overflow, v is
# inf and the Adam quotient is 0); so are the products m*ibc1 and v*ibc2.
# Within the bound of FLT_MAX either outcome is accepted.

FLT_MAX = float(torch.finfo(torch.float32).max)
SUB = 2.0 ** -149


def gamma(k):
    return k * U / (1 - k * U)


def f32(x) -> float:
    """A python scalar as the kernel receives it."""
    return float(np.float32(x))


def _overflow(t):
    inf = torch.full_like(t, float("inf")).copysign(t)
    return torch.where(t.abs() > FLT_MAX, inf, t)


def adamw_formula(w, m0, v0, g, lr, b1, b2, eps, wd, ibc1, ibc2,
                  dtype=torch.float64):
    """One AdamW step: new m, v and the update u."""
    w, m0, v0, g = (t.to(dtype) for t in (w, m0, v0, g))
    lr, b1, b2, eps, wd, ibc1, ibc2 = (
        torch.tensor(f32(s), dtype=dtype)
        for s in (lr, b1, b2, eps, wd, ibc1, ibc2))
    one = torch.tensor(1.0, dtype=dtype)
    m = b1 * m0 + (one - b1) * g
    v = b2 * v0 + (one - b2) * g * g
    if dtype == torch.float64:
        m, v = _overflow(m), _overflow(v)
    num, vh = m * ibc1, v * ibc2
    if dtype == torch.float64:      # the two intermediates that can overflow
        num, vh = _overflow(num), _overflow(vh)
    u = -lr * (num / (torch.sqrt(vh) + eps) + wd * w)
    return {"m": m, "v": v, "u": u}


def adamw_slack(w, m0, v0, g, lr, b1, b2, eps, wd, ibc1, ibc2):
    w, m0, v0, g = (t.double() for t in (w, m0, v0, g))
    lr, b1, b2, eps, wd, ibc1, ibc2 = (
        f32(s) for s in (lr, b1, b2, eps, wd, ibc1, ibc2))
    ref = adamw_formula(w, m0, v0, g, lr, b1, b2, eps, wd, ibc1, ibc2)
    m, v = ref["m"], ref["v"]
    # m: b1*m0 is rounded as a product and in the sum; (1 - b1)*g also in
    # the subtraction
    dm = (gamma(2) * (b1 * m0).abs() + gamma(3) * ((1 - b1) * g).abs()
          + 3 * SUB)
    # v: (1 - b2), *g, *g and the sum
    dv = (gamma(2) * (b2 * v0).abs() + gamma(4) * ((1 - b2) * g * g).abs()
          + 4 * SUB)
    num = _overflow(m * ibc1)
    dnum = ibc1 * dm + gamma(1) * num.abs() + SUB
    vh = _overflow(v * ibc2)
    dvh = ibc2 * dv + gamma(1) * vh.abs() + SUB
    s = torch.sqrt(vh)
    # |sqrt(a + d) - sqrt(a)| = |d| / (sqrt(a + d) + sqrt(a))
    #                        <= min(|d| / sqrt(a), sqrt(|d|))
    ds = torch.minimum(dvh / s.clamp_min(1e-300), torch.sqrt(dvh))
    ds = ds + gamma(1) * s
    den = s + eps
    dden = ds + gamma(1) * den
    den_lo = (den - dden).clamp_min(1e-300)
    q = num / den
    dq = dnum / den_lo + num.abs() * dden / (den * den_lo) + gamma(1) * q.abs()
    dw = wd * w
    ddw = gamma(1) * dw.abs() + SUB
    dsum = dq + ddw + gamma(1) * (q.abs() + dw.abs() + dq + ddw)
    u = ref["u"]
    du = lr * dsum + gamma(1) * (u.abs() + lr * dsum) + SUB
    # v or v*ibc2 = inf: the quotient is exactly 0 and only wd*w remains
    vinf = torch.isinf(vh) & torch.isfinite(num)
    du_inf = lr * ddw + gamma(2) * (lr * dw).abs() + SUB
    du = torch.where(vinf, du_inf, du)
    dv = torch.where(torch.isinf(v), torch.zeros_like(dv), dv)
    return {"m": dm, "v": dv, "u": du}


def sgd_formula(m0, g, lr, mu, dtype=torch.float64):
    """One SGD-momentum step: new m and the update u."""
    m0, g = m0.to(dtype), g.to(dtype)
    lr, mu = (torch.tensor(f32(s), dtype=dtype) for s in (lr, mu))
    m = mu * m0 + g
    if dtype == torch.float64:
        m = _overflow(m)
    return {"m": m, "u": -lr * m}


def sgd_slack(m0, g, lr, mu):
    m0, g = m0.double(), g.double()
    lr, mu = f32(lr), f32(mu)
    # the product and the sum round mu*m0, the sum alone rounds g
    dm = gamma(2) * (mu * m0).abs() + gamma(1) * g.abs() + 2 * SUB
    m = mu * m0 + g
    du = lr * dm + gamma(1) * (lr * (m.abs() + dm)) + SUB
    return {"m": dm, "u": du}


def assert_within(got, ref, slack, op, out, family):
    """fp32 output whose final rounding the slack already counts.  Finite
    references: |got - ref| <= slack.  Infinite: the same infinity.  NaN:
    NaN.  Within the slack of FLT_MAX: the bound or the infinity."""
    got, ref, slack = got.double(), ref.double(), slack.double()
    err = (got - ref).abs()
    fin = torch.isfinite(ref)
    ok = fin & (err <= slack)
    inf = torch.full_like(ref, float("inf")).copysign(ref)
    ok |= fin & (ref.abs() + slack >= FLT_MAX) & (got == inf)
    ok |= torch.isinf(ref) & (got == ref)
    ok |= torch.isnan(ref) & torch.isnan(got)
    judged = fin & torch.isfinite(got) & (slack > 0)
    worst = float((err / slack)[judged].max()) if judged.any() else 0.0
    report(op, out, family, worst, unit="of-bound")
    if not ok.all():
        bad = ~ok
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError(
            f"{op} {out} [{family}]: {int(bad.sum())} of {bad.numel()} outside "
            f"the bound; first at {i}: got {float(got.flatten()[i])!r}, ref "
            f"{float(ref.flatten()[i])!r}, bound {float(slack.flatten()[i]):.3g}")
    return worst


OPTIM_FAMILIES = ["randn", "zero_g_zero_state", "g_huge", "g_tiny", "wd0"]


def optim_inputs(family, n, seed=0):
    """fp32 w, m0, v0 (>= 0), g and the weight decay of the family."""
    gen = torch.Generator().manual_seed(77 * seed + n)
    w = torch.randn(n, generator=gen)
    m0 = torch.randn(n, generator=gen)
    v0 = torch.randn(n, generator=gen) ** 2
    g = torch.randn(n, generator=gen)
    sign = torch.where(torch.arange(n) % 2 == 0, 1.0, -1.0)
    wd = 0.01
    if family == "zero_g_zero_state":
        g, m0, v0 = torch.zeros(n), torch.zeros(n), torch.zeros(n)
    elif family == "g_huge":
        g = 1e20 * sign
    elif family == "g_tiny":
        g = 1e-30 * sign
    elif family == "wd0":
        wd = 0.0
    elif family != "randn":
        raise ValueError(family)
    return w, m0, v0, g, wd


def bias_corrections(b1, b2, step):
    """1 / (1 - beta^step) in fp32, as Engine::fused_adamw computes them."""
    f = np.float32
    return (float(f(1) / (f(1) - np.power(f(b1), f(step)))),
            float(f(1) / (f(1) - np.power(f(b2), f(step)))))


# ------------------------------------------------------ fused cross-entropy
#
# The kernels (csrc/ce_kernels.hip) evaluate
# per row of bf16 logits, in fp32,
#
#   m    = max_j x_j                                   (exact)
#   tot  = sum_j __expf(x_j - m)                       (>= 1, all terms >= 0)
#   lse  = __logf(tot) + m
#   loss = lse - x_t                                   (plain)
#        = (1-eps)*(lse - x_t) + eps*(lse - sx/V) + z*lse*lse,  sx = sum_j x_j
#   dx_j = g*inv_count*[(1 + 2*z*lse)*__expf(x_j - lse) - (1-eps)[j == t]
#                       - eps/V]
#
# ce_formula is that chain in a chosen dtype; ce_slack bounds its fp32
# evaluation in the kernels' reduction layout.
#
# Reduction depth of tot, n_ce(V, BLK, NCHUNK): a thread adds its chunks
# serially (ceil(nbody / BLK) of them, at most NCHUNK in the register
# kernels), each chunk is the 3-level tree of ce_expsum8, one more add brings
# the edge element in, then block_sum<BLK>: 6 shuffle levels and BLK/64 - 1
# LDS adds.  All terms are positive, so tot is off by at most n_ce * U
# relative, plus the per-term error of the exp.
#
# Transcendentals.  __expf is the fast exp of the module docstring: the
# argument x - m (or x - lse) is itself rounded (U*|arg|), the product with
# log2(e) is rounded (U*|arg| again) and the exp2 and the constant get
# EXP_ULPS = 3 ulps: relative error (2*|arg| + 3) * U.  For __logf neither the
# HIP headers nor the installed documentation state an accuracy (the headers
# only map it to the native log of the device library), so the figure is
# reasoned, not looked up, and not calibrated on the kernel: the native log is
# the hardware log2 (1 ulp by the instruction-set manual) times the fp32
# constant ln 2 (half an ulp in the constant, half an ulp in the product),
# 2 ulps in all; LOG_ULPS = 3 leaves one ulp for the hardware figure being
# meant at the magnitude of the result.  The ulps are taken at
# max(|log tot|, 1): close to tot = 1 the result is far smaller than the
# exponent-plus-table evaluation's last place.  The gradient bound hardly
# depends on LOG_ULPS: even 16 ulps on log(tot) <= 12 move exp(x - lse) by
# less than 1e-5 relative against a bf16 ulp of 4e-3; only the fp32 loss and
# lse bounds feel it.  A probability below the smallest normal fp32 may be
# flushed to 0: ETA, scaled by the coefficient.
#
# Constants taken from documentation: U, ETA (IEEE formats), the hardware
# log2 / exp2 ulp.  Derived here: n_ce, n_ce_sx, EXP_ULPS' use, LOG_ULPS, the
# rounding counts CE_COEF_ROUNDINGS and CE_DIV_ULPS.

EXP_ULPS = 3.0
LOG_ULPS = 3.0
# sx / V: correctly rounded by default; 3 covers a build whose fp32 division
# is the 2.5-ulp one
CE_DIV_ULPS = 3.0
# roundings on the way to one gradient term, the longest path: g*inv_count
# (1) and inv_count itself (1); a = gscale*(1 + 2*z*lse): z*lse, 1 + ., the
# product (3); nb = gscale*(eps/V): quotient and product; the fused
# multiply-add (1) and the subtraction of c at the target (1)
CE_COEF_ROUNDINGS = 7


def _ce_chunks(V, BLK, NCHUNK):
    c = max(1, math.ceil((V // 8) / BLK))
    return c if NCHUNK is None else min(c, NCHUNK)


def n_ce(V, BLK, NCHUNK=None):
    """Adds on the longest path of the exp-sum: NCHUNK None is the stride
    loop of the two-pass kernels."""
    return _ce_chunks(V, BLK, NCHUNK) + 3 + 1 + 6 + (BLK // 64 - 1)


def n_ce_sx(V, BLK, NCHUNK=None):
    """The same for sum_j x_j through ce_sum8: four dot2 per chunk, two fp32
    roundings each, chained on the accumulator."""
    return 8 * _ce_chunks(V, BLK, NCHUNK) + 1 + 6 + (BLK // 64 - 1)


def _ce_layouts(V):
    cap7 = 1024 * 7 * 8
    return [(1024, 7 if V <= cap7 else 16), (256, None), (512, None)]


def _ce_rows(x, t, ignore_index):
    V = x.shape[1]
    t = t.to(device=x.device, dtype=torch.int64)
    in_range = (t >= 0) & (t < V)
    ignored = (t == ignore_index) if ignore_index is not None \
        else torch.zeros_like(in_range)
    return t, in_range & ~ignored, ~in_range & ~ignored


def f32_inv(n) -> float:
    """fl32(1 / n) as the device computes it; inf at n = 0."""
    with np.errstate(divide="ignore"):
        return float(np.float32(1) / np.float32(n))


def ce_formula(x, t, g=1.0, ignore_index=None, eps=0.0, z=0.0,
               dtype=torch.float64, lse=None):
    """Cross-entropy of bf16 logits x (R, V) with targets t (R,): per-row m,
    lse and loss, the mean over the valid rows and dlogits for the upstream
    gradient g.  Row kinds as cross_entropy_reference (ops/fused_ce.py): an
    ignored row has loss 0, lse 0 and a +0 gradient row; an out-of-range,
    not ignored one has loss NaN and a +0 gradient row.  `lse`: the fp32
    row_lse a raw backward kernel is given; the gradient then uses it."""
    R, V = x.shape
    x = x.to(dtype)
    eps, z, g = f32(eps), f32(z), f32(g)
    t, valid, bad = _ce_rows(x, t, ignore_index)
    m = x.max(-1).values
    tot = torch.exp(x - m[:, None]).sum(-1)
    own = torch.log(tot) + m
    xt = x.gather(1, t.clamp(0, V - 1)[:, None]).squeeze(1)
    if eps != 0.0 or z != 0.0:
        sx = x.sum(-1)
        loss = (1.0 - eps) * (own - xt) + eps * (own - sx / V) + z * own * own
    else:
        loss = own - xt
    zero = torch.zeros((), dtype=dtype, device=x.device)
    nan = torch.full((), float("nan"), dtype=dtype, device=x.device)
    loss = torch.where(bad, nan, torch.where(valid, loss, zero))
    n_valid = int(valid.sum())
    inv = f32_inv(n_valid)
    mean = loss.sum() / n_valid if n_valid else loss.sum() * nan
    used = own if lse is None else lse.to(device=x.device, dtype=dtype)
    p = torch.exp(x - used[:, None])
    hot = torch.arange(V, device=x.device)[None, :] == t[:, None]
    d = (1.0 + 2.0 * z * used)[:, None] * p - (1.0 - eps) * hot.to(dtype) \
        - eps / V
    d = torch.where(valid[:, None], (g * inv) * d if n_valid else d, zero)
    return {"m": m, "lse": torch.where(valid, own, zero), "loss": loss,
            "mean": mean, "dlogits": d, "valid": valid, "bad": bad,
            "n_valid": n_valid}


def ce_slack(x, t, g=1.0, ignore_index=None, eps=0.0, z=0.0, lse=None,
             BLK=None, NCHUNK=None):
    """Running-error bounds of ce_formula in fp32.  BLK / NCHUNK name the
    kernel layout; without them the deepest of the layouts a call can take."""
    R, V = x.shape
    x = x.double()
    eps, z, g = f32(eps), f32(z), f32(g)
    if BLK is None:
        n = max(n_ce(V, b, c) for b, c in _ce_layouts(V))
        nsx = max(n_ce_sx(V, b, c) for b, c in _ce_layouts(V))
    else:
        n, nsx = n_ce(V, BLK, NCHUNK), n_ce_sx(V, BLK, NCHUNK)
    t, valid, bad = _ce_rows(x, t, ignore_index)
    fin = torch.isfinite(x)
    zero = torch.zeros((), dtype=torch.float64, device=x.device)

    m = x.max(-1).values
    xm = x - m[:, None]
    e = torch.exp(xm)
    tot = e.sum(-1)
    axm = torch.where(fin, xm.abs(), zero)       # exp(-inf) is exactly 0
    d_tot = (n * U + ((2 * axm + EXP_ULPS) * U * e).sum(-1) / tot
             + V * ETA / tot)
    logt = torch.log(tot)
    own = logt + m
    d_lse = d_tot + LOG_ULPS * U * logt.abs().clamp_min(1.0) + U * own.abs()
    xt = x.gather(1, t.clamp(0, V - 1)[:, None]).squeeze(1)
    if eps != 0.0 or z != 0.0:
        sx = x.sum(-1)
        sabs = torch.where(fin, x.abs(), zero).sum(-1)
        d_sx = nsx * U * sabs + V * ETA
        A = (1.0 - eps) * (own - xt)
        B = eps * (own - sx / V)
        C = z * own * own
        d_loss = ((1.0 - eps) * d_lse + 3 * U * A.abs()
                  + eps * (d_lse + d_sx / V + CE_DIV_ULPS * U * (sx / V).abs()
                           + U * (own - sx / V).abs()) + U * B.abs()
                  + 2 * z * own.abs() * d_lse + 2 * U * C.abs()
                  + 2 * U * (A.abs() + B.abs() + C.abs()))
    else:
        d_loss = d_lse          # the subtraction's rounding is assert_f32's
    inf = torch.full((), float("inf"), dtype=torch.float64, device=x.device)
    d_loss = torch.where(torch.isfinite(d_loss), d_loss, inf)
    d_loss = torch.where(valid, d_loss, zero)
    d_lse_out = torch.where(valid, d_lse, zero)

    ref = ce_formula(x, t, g, ignore_index, eps, z, lse=None)
    n_valid = ref["n_valid"]
    if n_valid and not bool(bad.any()):
        lv = torch.where(valid, ref["loss"], zero)
        d_mean = ((d_loss + U * lv.abs()).sum() / n_valid
                  + (R + 3) * U * lv.abs().sum() / n_valid
                  + 2 * U * ref["mean"].abs())
    else:
        d_mean = zero

    used = own if lse is None else lse.to(device=x.device).double()
    d_used = d_lse if lse is None else torch.zeros_like(d_lse)
    xl = x - used[:, None]
    p = torch.exp(xl)
    axl = torch.where(fin, xl.abs(), zero)
    dp = p * (d_used[:, None] + (2 * axl + EXP_ULPS) * U) + ETA
    gs = abs(g * f32_inv(n_valid)) if n_valid else 0.0
    a = gs * (1.0 + 2.0 * z * used.abs())[:, None]
    hot = (torch.arange(V, device=x.device)[None, :] == t[:, None]).double()
    mag = a * p + gs * eps / V + gs * (1.0 - eps) * hot
    d = (a * dp + gs * 2.0 * z * d_used[:, None] * p
         + CE_COEF_ROUNDINGS * U * mag)
    d = torch.where(valid[:, None], d, zero)
    return {"m": torch.zeros_like(m), "lse": d_lse_out, "loss": d_loss,
            "mean": d_mean, "dlogits": d}


def assert_f32_rows(got, ref, slack, op, out, family):
    """assert_f32 for per-row values that may be NaN or infinite by design
    (an out-of-range target; a -inf logit under label smoothing): the same
    rows must be NaN, infinities must match, the rest meets the bound."""
    got, ref = got.double().cpu(), ref.double().cpu()
    slack = slack.double().cpu() if torch.is_tensor(slack) else slack
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), \
        f"{op} {out} [{family}]: NaN rows differ: got {got}, ref {ref}"
    inf = torch.isinf(ref)
    assert torch.equal(got[inf], ref[inf]), f"{op} {out} [{family}]: inf rows"
    fin = torch.isfinite(ref)
    s = slack[fin] if torch.is_tensor(slack) and slack.dim() else slack
    return assert_f32(got[fin], ref[fin], s, op, out, family)


def is_plus_zero(t) -> bool:
    """Every element is +0 bit for bit (bf16 or fp32)."""
    bits = torch.int16 if t.element_size() == 2 else torch.int32
    return not bool(t.contiguous().view(bits).any())


def ce_check(got, x, t, op, family, g=1.0, ignore_index=None, eps=0.0,
             z=0.0, lse=None, BLK=None, NCHUNK=None):
    """Judge whatever of m / lse / loss / mean / dlogits `got` holds against
    the fp64 reference, on the device x lives on.  Rows that are not valid
    are held to their exact values.  Returns (ref, slack)."""
    kw = dict(g=g, ignore_index=ignore_index, eps=eps, z=z, lse=lse)
    ref = ce_formula(x, t, **kw)
    slack = ce_slack(x, t, BLK=BLK, NCHUNK=NCHUNK, **kw)
    valid, bad = ref["valid"], ref["bad"]
    for k in ("m", "lse", "loss"):
        if k not in got:
            continue
        v = got[k]
        assert v.dtype == torch.float32 and v.shape == ref[k].shape, k
        if k == "m":
            assert torch.equal(v.double()[valid], ref[k][valid]), \
                f"{op} m [{family}]: not the row maximum"
            report(op, "m", family, 0.0, unit="of-slack")
            continue
        assert_f32_rows(v, ref[k], slack[k], op, k, family)
        assert is_plus_zero(v[~valid & ~bad]), f"{op} {k}: ignored rows"
        if k == "lse":
            assert is_plus_zero(v[bad]), f"{op} lse: out-of-range rows"
    if "mean" in got:
        assert_f32_rows(got["mean"].reshape(1), ref["mean"].reshape(1),
                        slack["mean"].reshape(1), op, "mean", family)
    if "dlogits" in got:
        d = got["dlogits"]
        assert d.dtype == torch.bfloat16 and d.shape == ref["dlogits"].shape
        assert_bf16(d, ref["dlogits"], slack["dlogits"], op, "dlogits",
                    family)
        assert is_plus_zero(d[~valid]), f"{op} dlogits: rows not valid"
    return ref, slack


def seam_targets(R, V, offset=0):
    """Targets at element 0, at V-1, in a head and in a tail element of rows
    that have one (`offset` = element offset of the matrix from a 16-byte
    boundary); random elsewhere.  int64, on the CPU."""
    g = torch.Generator().manual_seed(R * 7919 + V)
    t = torch.randint(0, V, (R,), generator=g)
    want = ["first", "last", "head", "tail"]
    for r in range(R):
        head = min((-(offset + r * V)) % 8, V)
        tail = (V - head) % 8
        if "head" in want and head > 1 and r > 0:
            t[r] = head - 1
            want.remove("head")
        elif "tail" in want and tail > 1 and r > 0:
            t[r] = V - tail
            want.remove("tail")
        elif "first" in want:
            t[r] = 0
            want.remove("first")
        elif "last" in want:
            t[r] = V - 1
            want.remove("last")
    return t


CE_FAMILIES = ["randn3", "tiny", "wide", "flat", "peaked_target",
               "peaked_other", "masked", "shifted", "neg_zero_mix"]


def ce_inputs(family, R, V, seed=0, offset=0):
    """bf16 logits (R, V) and int64 seam targets (R,), on the CPU."""
    gen = torch.Generator().manual_seed(1000 * seed + 31 * R + V)
    t = seam_targets(R, V, offset)
    rows = torch.arange(R)
    rn = torch.randn(R, V, generator=gen)
    if family == "randn3":
        x = rn * 3
    elif family == "tiny":
        x = rn * 1e-3
    elif family == "wide":           # most exps underflow
        x = rn * 30
    elif family == "flat":           # one constant per row
        x = (1.5 * (rows - R // 2).float())[:, None].expand(R, V).clone()
    elif family in ("peaked_target", "peaked_other"):
        x = rn * 0.1                 # 1 - p cancels at the peak
        at = t if family == "peaked_target" else (t + V // 2) % V
        x[rows, at] = 80.0
    elif family == "masked":         # masked vocabulary
        x = rn * 3
        drop = torch.rand(R, V, generator=gen) < 0.5
        drop[R // 2] = True          # a row with the target alone
        drop[rows, t] = False
        x[drop] = float("-inf")
    elif family == "shifted":        # x - m exact, ulp(lse) = 2^-9
        x = rn + 3e4
    elif family == "neg_zero_mix":   # +-0 and bf16 subnormals
        bits = torch.randint(0, 0x80, (R, V), generator=gen)
        bits = torch.where(torch.rand(R, V, generator=gen) < 0.5,
                           torch.zeros_like(bits), bits)
        bits = bits | (torch.randint(0, 2, (R, V), generator=gen) << 15)
        x = bits.to(torch.int32).to(torch.int16).view(torch.bfloat16).float()
    else:
        raise ValueError(family)
    return x.to(torch.bfloat16), t


def emu_ce_expsum(x, BLK=1024, NCHUNK=7):
    """tot = sum_j exp(x_j - m) of each row of bf16 x (matrix on a 16-byte
    boundary) in k_ce_fwd_grad<BLK, NCHUNK>'s thread layout and fp32 order:
    thread t holds chunks t, t + BLK, ...; edge element e rides in thread
    BLK - 1 - e; ce_expsum8's tree inside a chunk; then block_sum.  Returns
    (m, tot, lse) in fp32."""
    f = np.float32
    xs = x.float().numpy().astype(f)
    R, V = xs.shape
    ms, tots = np.zeros(R, f), np.zeros(R, f)
    for r in range(R):
        row = xs[r]
        head = min((-(r * V)) % 8, V)
        nbody = (V - head) // 8
        tail = V - head - 8 * nbody
        assert nbody <= BLK * NCHUNK
        m = row.max()
        ex = np.exp((row - m).astype(f)).astype(f)
        s = np.zeros(BLK, f)
        edges = np.concatenate([ex[:head], ex[V - tail:]]) if tail \
            else ex[:head]
        s[BLK - 1 - np.arange(edges.size)] = edges
        body = np.zeros((BLK * NCHUNK, 8), f)
        body[:nbody] = ex[head:head + 8 * nbody].reshape(nbody, 8)
        p = body[:, 0::2] + body[:, 1::2]
        c8 = ((p[:, 0] + p[:, 1]) + (p[:, 2] + p[:, 3])).reshape(NCHUNK, BLK)
        for k in range(NCHUNK):
            s = np.where(k * BLK + np.arange(BLK) < nbody, s + c8[k], s)
        ms[r], tots[r] = m, emu_block_sum(s.astype(f))
    lse = (np.log(tots).astype(f) + ms).astype(f)
    return (torch.from_numpy(ms), torch.from_numpy(tots),
            torch.from_numpy(lse))
