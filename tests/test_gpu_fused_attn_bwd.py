"""The causal bf16 attention backward kernels (csrc/attn_bwd_kernels.hip)
against fp64 autograd through plain softmax attention, fed the out and lse of
our forward and the same bf16 dout.

Tolerance.  Nothing is fixed in advance: for each of dq, dk and dv the
max-abs and the relative-L2 error against fp64 may be at most 1.5x the error
of the aten efficient-attention backward on the same q, k, v, out, lse and
dout.  Both arms round P, dS and the gradients to bf16; those errors are
measured by the aten arm.  A floor takes over only where the aten error is
about zero (T = 1: dq = dk = 0, dv = dout) and counts the fp32 operations
alone.  With eps32 = 2^-24 and everything in fp64 (tests/attn_bwd_floors.py):

* dS = P (dP - delta): dP and delta are 64-term fp32 sums whose exact values
  may cancel, so each costs 64 eps32 of sum_d |dO||v| and sum_d |dO||O|; the
  subtraction, the product, the fma in front of exp2 and the score's own
  64-term sum behind it are a handful more (4 eps32 on the same magnitude,
  the score's share going through P), and the hardware exp2 is within 2^-21,
  counted as 2^-20 like the forward's:
      A_ij = P_ij (sum_d |dO_id||v_jd| + sum_d |dO_id||O_id|)
      floor_dS = A (132 eps32 + 2^-20)
  and the kernels follow exactly this order (one sequential fma sum for
  delta, one mfma chain each for S and dP), so the counts stand as stated;
* dq = scale dS k and dk = scale dS^T q carry it on:
      floor_dq = scale floor_dS |k|,  floor_dk = scale floor_dS^T |q|;
* dv = P^T dO is a T-term fp32 sum on top of the 64-term scores:
      floor_dv = (P^T |dO|) ((T + 64) eps32 + 2^-20).

Max-abs uses the floor's maximum, relative L2 its norm over the reference's
norm, skipped where the reference is identically zero.
tests/test_fused_attn_bwd_cpu.py checks that an fp32 evaluation of these
formulas stays inside the floors at T = 1.

Each case prints its figures; test_maxerr_report prints one MAXERR line per
gradient and family (the record is profiles/r11/attn_bwd_maxerr.txt).
"""
import copy
import functools

import pytest
import torch

from attn_bwd_floors import EPS32, floors, reference
from test_gpu_fused_attn import (CANARY_BF16, CANARY_F32, GUARD, MARGIN, SCALE,
                                 _errs, _fa, _guarded, _layout, _make_qkv,
                                 _priority)

pytestmark = pytest.mark.gpu

SHAPES = [(2, 3, 1), (2, 3, 17), (2, 3, 64), (2, 3, 96), (2, 3, 128),
          (2, 3, 129), (2, 3, 192), (2, 3, 320)]
FAMILIES = ["gauss", "pm80", "lastmax"]
LAYOUTS = ["packed", "separate"]
GRADS = ("dq", "dk", "dv")


@functools.lru_cache(maxsize=None)
def _case(B, H, T, family, layout):
    fa = _fa()
    seed = 2000 * T + 10 * FAMILIES.index(family) + LAYOUTS.index(layout)
    q, k, v = _layout(*_make_qkv(B, H, T, family, seed), layout)
    g = torch.Generator(device="cuda").manual_seed(seed + 1)
    dout = torch.randn(B, T, H, 64, device="cuda",
                       generator=g).bfloat16().transpose(1, 2)
    out, lse = fa.attn_forward(q, k, v, SCALE)
    out = out.transpose(1, 2)
    ref = reference(q, k, v, dout, SCALE)
    fl = floors(ref, q, k, v, dout, SCALE)
    seed_, offset = fa._philox_state()
    with _priority():
        aten = torch.ops.aten._scaled_dot_product_efficient_attention_backward(
            dout, q, k, v, None, out, lse, seed_, offset, 0.0,
            [True, True, True, False], True, scale=SCALE)[:3]

    def run():
        bufs, views = zip(*(_guarded((B, T, H, 64), torch.bfloat16,
                                     CANARY_BF16) for _ in GRADS))
        dbuf, delta = _guarded((B, H, T), torch.float32, CANARY_F32)
        got = fa.attn_backward(q, k, v, out, lse, dout, SCALE,
                               *(x.transpose(1, 2) for x in views),
                               delta=delta)
        torch.cuda.synchronize()
        return got, delta, bufs + (dbuf,)

    got, delta, bufs = run()
    again, delta2, _ = run()
    return dict(ref=ref, fl=fl, aten=dict(zip(GRADS, aten)),
                got=dict(zip(GRADS, got)), again=dict(zip(GRADS, again)),
                delta=delta, delta2=delta2, bufs=bufs, out=out, dout=dout)


def _figures(c, name):
    f_abs, f_l2 = _errs(c["got"][name], c["ref"][name])
    a_abs, a_l2 = _errs(c["aten"][name], c["ref"][name])
    norm = c["ref"][name].norm().item()
    fl_l2 = (c["fl"][name].norm().item() / norm) if norm > 0 else None
    if norm == 0:  # no relative figure against an identically zero reference
        f_l2 = a_l2 = 0.0
    return dict(f_abs=f_abs, f_l2=f_l2, a_abs=a_abs, a_l2=a_l2,
                fl_abs=c["fl"][name].max().item(), fl_l2=fl_l2)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("B,H,T", SHAPES)
def test_backward_against_fp64(B, H, T, family, layout):
    c = _case(B, H, T, family, layout)
    for buf in c["bufs"]:  # guards untouched
        canary = CANARY_BF16 if buf.dtype == torch.bfloat16 else CANARY_F32
        g = torch.full((GUARD,), canary, dtype=buf.dtype, device="cuda")
        assert torch.equal(buf[:GUARD], g) and torch.equal(buf[-GUARD:], g)
    prod = (c["dout"].double() * c["out"].double())
    d_err = (c["delta"].double() - prod.sum(-1)).abs()
    assert (d_err <= 2 * 64 * EPS32 * prod.abs().sum(-1)).all(), d_err.max()
    assert torch.equal(c["delta"], c["delta2"])
    for name in GRADS:
        got = c["got"][name]
        assert got.shape == (B, H, T, 64) and got.dtype == torch.bfloat16
        assert torch.isfinite(got.float()).all()
        assert torch.equal(got, c["again"][name]), f"{name}: repeat differs"
        f = _figures(c, name)
        print(f"ATTN bwd T={T} {family} {layout} {name}: maxabs fused "
              f"{f['f_abs']:.3e} aten {f['a_abs']:.3e} floor "
              f"{f['fl_abs']:.3e} | rel-l2 fused {f['f_l2']:.3e} aten "
              f"{f['a_l2']:.3e} floor {f['fl_l2']}")
        assert f["f_abs"] <= max(MARGIN * f["a_abs"], f["fl_abs"])
        if f["fl_l2"] is not None:
            assert f["f_l2"] <= max(MARGIN * f["a_l2"], f["fl_l2"])


def test_maxerr_report():
    for fam in FAMILIES:
        for name in GRADS:
            w = dict(f_abs=0.0, a_abs=0.0, f_l2=0.0, a_l2=0.0)
            for (B, H, T) in SHAPES:
                for lay in LAYOUTS:
                    f = _figures(_case(B, H, T, fam, lay), name)
                    w = {k: max(w[k], f[k]) for k in w}
            print(f"MAXERR attn_bwd {name} {fam}: maxabs fused "
                  f"{w['f_abs']:.3e} aten {w['a_abs']:.3e} rel-l2 fused "
                  f"{w['f_l2']:.3e} aten {w['a_l2']:.3e}")


def test_module_gradients_flag_on_and_off(monkeypatch):
    """One CausalSelfAttention, forward + backward, with FUSE_ATTN_BWD on and
    off, each against the same module in fp64; attn_backward runs exactly
    when the flag says so."""
    from sharedtensor_amd.models import gpt2
    from sharedtensor_amd.ops import fused_attn
    monkeypatch.delenv("SHTENS_FUSED_ATTN", raising=False)
    monkeypatch.delenv("SHTENS_FUSED_ATTN_BWD", raising=False)
    monkeypatch.setattr(gpt2, "FUSE_ATTN_FWD", True)
    cfg = gpt2.GPT2Config(vocab_size=64, n_layer=1, n_head=3, n_embd=192,
                          block_size=256)
    torch.manual_seed(3)
    mod = gpt2.CausalSelfAttention(cfg).cuda()
    torch.nn.init.normal_(mod.qkv.bias, std=0.1)
    mod = mod.bfloat16()
    x = torch.randn(2, 160, 192, device="cuda").bfloat16()
    dy = torch.randn(2, 160, 192, device="cuda").bfloat16()
    names = ["qkv.weight", "qkv.bias", "proj.weight"]

    calls = []
    real = fused_attn.attn_backward
    monkeypatch.setattr(fused_attn, "attn_backward",
                        lambda *a, **k: (calls.append(1), real(*a, **k))[1])

    def run(m, xx, dd, flag):
        monkeypatch.setattr(gpt2, "FUSE_ATTN_BWD", flag)
        m.zero_grad(set_to_none=True)
        m(xx).backward(dd)
        p = dict(m.named_parameters())
        return [p[n].grad.clone() for n in names]

    on = run(mod, x, dy, True)
    assert len(calls) == 1, "flag on: attn_backward did not run once"
    off = run(mod, x, dy, False)
    ref = run(copy.deepcopy(mod).double(), x.double(), dy.double(), True)
    assert len(calls) == 1, "flag off or fp64: attn_backward ran"
    for name, r, f, a in zip(names, ref, on, off):
        f_abs, f_l2 = _errs(f, r)
        a_abs, a_l2 = _errs(a, r)
        print(f"ATTN bwd module {name}: maxabs fused {f_abs:.3e} aten "
              f"{a_abs:.3e} | rel-l2 fused {f_l2:.3e} aten {a_l2:.3e}")
        assert f_abs <= MARGIN * a_abs
        assert f_l2 <= MARGIN * a_l2


def test_can_use_backward_rejections_on_device():
    fa = _fa()
    mk = lambda *s, dt=torch.bfloat16: torch.zeros(*s, device="cuda", dtype=dt)
    q, lse = mk(2, 3, 16, 64), mk(2, 3, 16, dt=torch.float32)
    assert fa.can_use_backward(q, q, q, q, lse, q)
    f = mk(2, 3, 16, 64, dt=torch.float32)
    d32 = mk(2, 3, 16, 32)
    kv = mk(2, 1, 16, 64)
    odd = mk(2, 3, 16, 68)[..., 2:66]  # stride 68, base off by 4 B
    bad = [(f, f, f, f, lse, f),        # fp32
           (q, q, q, q, lse, f),        # fp32 dout
           (d32, d32, d32, d32, lse, d32),
           (q, kv, kv, q, lse, q),      # mismatched heads
           (q, q, q, odd, lse, q)]      # misaligned out
    for args in bad:
        assert not fa.can_use_backward(*args)
        with pytest.raises(ValueError):
            fa.attn_backward(*args, 0.125)
    # a dout that only breaks the stride rules is made contiguous once
    dq, _, _ = fa.attn_backward(q, q, q, q, lse, odd, 0.125)
    assert dq.shape == q.shape
