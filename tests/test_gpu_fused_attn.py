"""The causal bf16 attention forward kernel (csrc/attn_kernels.hip) and its
autograd Function (ops/fused_attn.py) against softmax attention in fp64.

Tolerance.  Nothing is fixed in advance: on every case the error of the fused
kernel against fp64 may be at most 1.5x the error of the aten
efficient-attention op on the same inputs (the equivalence margin of
profiles/r03, r04, r07).  Both arms round P and the output to bf16 and
accumulate scores in fp32, so those errors are measured by the aten arm and
are no part of any floor.  A floor takes over only where the aten error is
about zero (T = 1, where out is v itself), and it counts the fp32 operations
alone.  With eps32 = 2^-24 (half an ulp of fp32):

* out: a numerator of T products accumulated in fp32 on top of the 64-term
  scores, the hardware exp2 within 2^-21 relative on numerator and
  denominator alike; relative to sum_k p_k |v_k| / l, which fp64 gives per
  element as (P |v|):
      floor_out[i] = (P |v|)[i] ((T + 64) eps32 + 2^-20)
  taken as its maximum for max-abs and as ||floor_out||_2 / ||ref||_2 for the
  relative L2;
* lse = ln2 (m + log2 l) is one fp32 number produced by an add and a
  multiply: floor_lse = 2 eps32 max(1, max |lse|).

Gradients reach us through the aten backward, which reads our out and lse;
the current path's gradients are bf16 and never exact, so they are held to
the 1.5x rule with no floor at all.

Each case prints its figures; test_maxerr_report prints one MAXERR line per
output and input family (the record is profiles/r08/attn_maxerr.txt).
"""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -24
MARGIN = 1.5
SCALE = 1.0 / 8.0

SHAPES = [(2, 3, 1), (2, 3, 17), (2, 3, 64), (2, 3, 96), (2, 3, 128),
          (2, 3, 192), (2, 3, 320), (1, 2, 1024)]
FAMILIES = ["gauss", "pm80", "lastmax", "equalkeys"]
LAYOUTS = ["packed", "separate"]


def _fa():
    from sharedtensor_amd.ops import fused_attn
    return fused_attn


def _priority():
    from torch.nn.attention import SDPBackend, sdpa_kernel
    return sdpa_kernel([SDPBackend.EFFICIENT_ATTENTION,
                        SDPBackend.FLASH_ATTENTION, SDPBackend.MATH],
                       set_priority=True)


def _make_qkv(B, H, T, family, seed):
    """(B, T, H, 64) fp32 values of q, k, v for one input family."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    q, k, v = (torch.randn(B, T, H, 64, device="cuda", generator=g)
               for _ in range(3))
    if family == "pm80":
        # raw scores (before the 1/8) whose extremes over the visible keys
        # reach +-80: the max must be subtracted before exp, not after
        s = torch.einsum("bthd,bshd->bhts", q.bfloat16().double(),
                         k.bfloat16().double())
        vis = torch.ones(T, T, device="cuda", dtype=torch.bool).tril()
        q = q * (80.0 / s.masked_fill(~vis, 0.0).abs().max().clamp_min(1e-3))
    elif family == "lastmax":
        # keys grow with the position and the last key is aligned with the
        # last query: the row maximum sits in the last KV tile, every
        # earlier tile gets rescaled
        grow = 0.5 + 2.0 * torch.arange(T, device="cuda").float() / T
        k = k * grow.view(1, T, 1, 1)
        k[:, T - 1] = 4.0 * q[:, T - 1]
    elif family == "equalkeys":
        k = k[:, :1].expand(B, T, H, 64).clone()
    return q, k, v


def _layout(q, k, v, layout):
    """bf16 (B, H, T, 64) views as the model builds them."""
    B, T, H, _ = q.shape
    if layout == "packed":
        qkv = torch.cat([t.reshape(B, T, H * 64) for t in (q, k, v)],
                        dim=2).bfloat16()
        return tuple(t.view(B, T, H, 64).transpose(1, 2)
                     for t in qkv.split(H * 64, dim=2))
    return tuple(t.bfloat16().transpose(1, 2).contiguous() for t in (q, k, v))


def _ref64(q, k, v):
    q, k, v = q.double(), k.double(), v.double()
    T = q.shape[2]
    s = (q @ k.transpose(-1, -2)) * SCALE
    vis = torch.ones(T, T, device=q.device, dtype=torch.bool).tril()
    s = s.masked_fill(~vis, float("-inf"))
    return torch.softmax(s, dim=-1) @ v, torch.logsumexp(s, dim=-1)


def _errs(x, ref):
    d = x.double() - ref
    return d.abs().max().item(), (d.norm() / ref.norm().clamp_min(1e-300)).item()


CANARY_BF16 = -12345.0
CANARY_F32 = -7.0e33
GUARD = 256  # elements before and after; keeps out 16-byte aligned


def _guarded(shape, dtype, canary):
    n = math.prod(shape)
    buf = torch.full((n + 2 * GUARD,), canary, dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + n].view(shape)


@functools.lru_cache(maxsize=None)
def _case(B, H, T, family, layout):
    fa = _fa()
    seed = 1000 * T + 10 * FAMILIES.index(family) + LAYOUTS.index(layout)
    q, k, v = _layout(*_make_qkv(B, H, T, family, seed), layout)
    o_ref, l_ref = _ref64(q, k, v)
    with _priority():
        a_out, a_lse, _, _ = \
            torch.ops.aten._scaled_dot_product_efficient_attention(
                q, k, v, None, True, 0.0, True, scale=SCALE)
    obuf, out = _guarded((B, T, H, 64), torch.bfloat16, CANARY_BF16)
    lbuf, lse = _guarded((B, H, T), torch.float32, CANARY_F32)
    fa.attn_forward(q, k, v, SCALE, out=out, lse=lse)
    torch.cuda.synchronize()
    T_ = q.shape[2]
    vis = torch.ones(T_, T_, device="cuda", dtype=torch.bool).tril()
    sc = ((q.double() @ k.double().transpose(-1, -2)) * SCALE).masked_fill(
        ~vis, float("-inf"))
    pv = torch.softmax(sc, dim=-1) @ v.double().abs()
    floor_el = pv * ((T + 64) * EPS32 + 2.0 ** -20)
    floor_out = floor_el.max().item()
    floor_l2 = (floor_el.norm() / o_ref.norm().clamp_min(1e-300)).item()
    floor_lse = 2 * EPS32 * max(1.0, l_ref.abs().max().item())
    return dict(q=q, k=k, v=v, o_ref=o_ref, l_ref=l_ref, a_out=a_out,
                a_lse=a_lse, out=out, lse=lse, obuf=obuf, lbuf=lbuf,
                floor_out=floor_out, floor_l2=floor_l2, floor_lse=floor_lse)


def _figures(c):
    f_abs, f_l2 = _errs(c["out"].transpose(1, 2), c["o_ref"])
    a_abs, a_l2 = _errs(c["a_out"], c["o_ref"])
    f_lse, _ = _errs(c["lse"], c["l_ref"])
    a_lse, _ = _errs(c["a_lse"], c["l_ref"])
    return dict(f_abs=f_abs, f_l2=f_l2, a_abs=a_abs, a_l2=a_l2, f_lse=f_lse,
                a_lse=a_lse)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("B,H,T", SHAPES)
def test_forward_against_fp64(B, H, T, family, layout):
    c = _case(B, H, T, family, layout)
    out, lse = c["out"], c["lse"]
    # shape, dtype and padding of lse are the aten op's
    assert lse.shape == c["a_lse"].shape and lse.dtype == c["a_lse"].dtype
    assert lse.stride() == c["a_lse"].stride()
    assert out.transpose(1, 2).shape == c["a_out"].shape
    assert out.transpose(1, 2).stride() == c["a_out"].stride()
    assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all()
    # guards untouched
    for buf, canary in ((c["obuf"], CANARY_BF16), (c["lbuf"], CANARY_F32)):
        ref = torch.full((GUARD,), canary, dtype=buf.dtype, device="cuda")
        assert torch.equal(buf[:GUARD], ref) and torch.equal(buf[-GUARD:], ref)
    f = _figures(c)
    floor_l2 = c["floor_l2"]
    print(f"ATTN T={T} {family} {layout}: out maxabs fused {f['f_abs']:.3e} "
          f"aten {f['a_abs']:.3e} floor {c['floor_out']:.3e} | rel-l2 fused "
          f"{f['f_l2']:.3e} aten {f['a_l2']:.3e} floor {floor_l2:.3e} | lse "
          f"fused {f['f_lse']:.3e} aten {f['a_lse']:.3e} floor "
          f"{c['floor_lse']:.3e}")
    assert f["f_abs"] <= max(MARGIN * f["a_abs"], c["floor_out"])
    assert f["f_l2"] <= max(MARGIN * f["a_l2"], floor_l2)
    assert f["f_lse"] <= max(MARGIN * f["a_lse"], c["floor_lse"])


def test_equal_keys_is_running_mean():
    """All keys equal: softmax is uniform over the visible keys, so out is
    the running mean of v, computed here without any softmax; same rule."""
    c = _case(2, 3, 192, "equalkeys", "packed")
    v = c["v"].double()
    cnt = torch.arange(1, 193, device="cuda").double().view(1, 1, 192, 1)
    mean = v.cumsum(dim=2) / cnt
    f_abs, f_l2 = _errs(c["out"].transpose(1, 2), mean)
    a_abs, a_l2 = _errs(c["a_out"], mean)
    print(f"ATTN running mean: maxabs fused {f_abs:.3e} aten {a_abs:.3e} | "
          f"rel-l2 fused {f_l2:.3e} aten {a_l2:.3e}")
    assert f_abs <= max(MARGIN * a_abs, c["floor_out"])
    assert f_l2 <= max(MARGIN * a_l2, c["floor_l2"])


def test_maxerr_report():
    for fam in FAMILIES:
        worst = dict(f_abs=0.0, a_abs=0.0, f_l2=0.0, a_l2=0.0, f_lse=0.0,
                     a_lse=0.0)
        for (B, H, T) in SHAPES:
            for lay in LAYOUTS:
                f = _figures(_case(B, H, T, fam, lay))
                worst = {k: max(worst[k], f[k]) for k in worst}
        print(f"MAXERR attn_fwd out {fam}: maxabs fused {worst['f_abs']:.3e} "
              f"aten {worst['a_abs']:.3e} rel-l2 fused {worst['f_l2']:.3e} "
              f"aten {worst['a_l2']:.3e}")
        print(f"MAXERR attn_fwd lse {fam}: maxabs fused {worst['f_lse']:.3e} "
              f"aten {worst['a_lse']:.3e}")


@pytest.mark.parametrize("family", ["gauss", "lastmax"])
@pytest.mark.parametrize("B,H,T", [(2, 3, 17), (2, 3, 192), (1, 2, 1024)])
def test_backward_against_fp64(B, H, T, family):
    fa = _fa()
    c = _case(B, H, T, family, "packed")
    g = torch.Generator(device="cuda").manual_seed(T)
    do = torch.randn(B, H, T, 64, device="cuda", generator=g).bfloat16()

    def grads(fn, dtype):
        xs = [c[n].detach().to(dtype).requires_grad_() for n in "qkv"]
        fn(*xs).backward(do.to(dtype))
        return [x.grad for x in xs]

    ref = grads(lambda q, k, v: _ref64(q, k, v)[0], torch.float64)
    fused = grads(lambda q, k, v: fa.fused_causal_attention(q, k, v, SCALE),
                  torch.bfloat16)

    def sdpa(q, k, v):
        with _priority():
            return torch.nn.functional.scaled_dot_product_attention(
                q, k, v, is_causal=True, scale=SCALE)
    cur = grads(sdpa, torch.bfloat16)
    for name, r, f, a in zip(("dq", "dk", "dv"), ref, fused, cur):
        assert f.stride() == a.stride() and f.dtype == a.dtype
        f_abs, f_l2 = _errs(f, r)
        a_abs, a_l2 = _errs(a, r)
        print(f"ATTN bwd T={T} {family} {name}: maxabs fused {f_abs:.3e} "
              f"current {a_abs:.3e} | rel-l2 fused {f_l2:.3e} current "
              f"{a_l2:.3e}")
        assert torch.isfinite(f.float()).all()
        assert f_abs <= MARGIN * a_abs
        assert f_l2 <= MARGIN * a_l2


def test_module_gradients_flag_on_and_off(monkeypatch):
    """One CausalSelfAttention, forward + backward, with the flag on and off,
    each against the same module in fp64."""
    from sharedtensor_amd.models import gpt2
    from sharedtensor_amd.ops import fused_attn
    monkeypatch.delenv("SHTENS_FUSED_ATTN", raising=False)
    cfg = gpt2.GPT2Config(vocab_size=64, n_layer=1, n_head=3, n_embd=192,
                          block_size=128)
    torch.manual_seed(3)
    mod = gpt2.CausalSelfAttention(cfg).cuda()
    torch.nn.init.normal_(mod.qkv.bias, std=0.1)
    mod = mod.bfloat16()
    x = torch.randn(2, 96, 192, device="cuda").bfloat16()
    dy = torch.randn(2, 96, 192, device="cuda").bfloat16()
    names = ["qkv.weight", "qkv.bias", "proj.weight"]

    calls = []
    real = fused_attn.fused_causal_attention
    monkeypatch.setattr(fused_attn, "fused_causal_attention",
                        lambda *a, **k: (calls.append(1), real(*a, **k))[1])

    def run(m, xx, dd, flag):
        monkeypatch.setattr(gpt2, "FUSE_ATTN_FWD", flag)
        m.zero_grad(set_to_none=True)
        m(xx).backward(dd)
        p = dict(m.named_parameters())
        return [p[n].grad.clone() for n in names]

    on = run(mod, x, dy, True)
    assert calls, "flag on: the fused Function did not run"
    n_on = len(calls)
    off = run(mod, x, dy, False)
    assert len(calls) == n_on, "flag off: the fused Function ran"
    import copy
    ref = run(copy.deepcopy(mod).double(), x.double(), dy.double(), True)
    assert len(calls) == n_on, "fp64 must keep the SDPA path"
    for name, r, f, a in zip(names, ref, on, off):
        f_abs, f_l2 = _errs(f, r)
        a_abs, a_l2 = _errs(a, r)
        print(f"ATTN module {name}: maxabs fused {f_abs:.3e} current "
              f"{a_abs:.3e} | rel-l2 fused {f_l2:.3e} current {a_l2:.3e}")
        assert f_abs <= MARGIN * a_abs
        assert f_l2 <= MARGIN * a_l2


def test_philox_state_is_what_aten_returns():
    """At dropout 0 the aten forward returns a philox seed and offset the
    backward never reads; the Function hands the backward tensors of the
    same shape, dtype and device."""
    fa = _fa()
    c = _case(2, 3, 17, "gauss", "packed")
    with _priority():
        res = torch.ops.aten._scaled_dot_product_efficient_attention(
            c["q"], c["k"], c["v"], None, True, 0.0, True, scale=SCALE)
    for ours, theirs in zip(fa._philox_state(), res[2:4]):
        assert ours.shape == theirs.shape
        assert ours.dtype == theirs.dtype
        assert ours.device == theirs.device


def test_can_use_rejections_on_device():
    fa = _fa()
    mk = lambda *s, dt=torch.bfloat16: torch.zeros(*s, device="cuda", dtype=dt)
    q = mk(2, 3, 16, 64)
    assert fa.can_use(q, q, q)
    f = mk(2, 3, 16, 64, dt=torch.float32)
    assert not fa.can_use(f, f, f)
    d32 = mk(2, 3, 16, 32)
    assert not fa.can_use(d32, d32, d32)
    kv = mk(2, 1, 16, 64)
    assert not fa.can_use(q, kv, kv)            # GQA
    assert not fa.can_use(q, mk(2, 3, 8, 64), mk(2, 3, 8, 64))  # Tq != Tk
    odd = mk(2, 3, 16, 68)[..., 2:66]           # stride 68, base off by 4 B
    assert not fa.can_use(odd, odd, odd)
    with pytest.raises(ValueError):
        fa.attn_forward(f, f, f)
