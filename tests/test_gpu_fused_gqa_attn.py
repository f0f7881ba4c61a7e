"""The causal bf16 grouped-query attention kernels (csrc/gqa_attn_kernels.hip,
csrc/gqa_attn_bwd_kernels.hip) and ops/fused_gqa_attn.py against fp64 softmax
attention over repeat_interleave'd K/V, with autograd.

Tolerance.  Nothing is fixed in advance: max-abs and relative-L2 error of out,
lse, dq, dk and dv against fp64 may be at most 1.5x (MARGIN of
test_gpu_fused_attn.py) the error of today's path written out: the aten
efficient-attention forward and backward on the expanded bf16 K/V, the
per-head bf16 dk and dv summed over the group.  A floor takes over only
where that error is about zero (T = 1) and counts the fp32 operations alone:

* out and lse: the floors of test_gpu_fused_attn.py, per query head;
* dq: attn_bwd_floors.floors per query head on the expanded tensors;
* dk: the same per-head floors summed over the group (the sum adds G - 1
  fp32 additions to chains of 64 and more terms already counted in 132 eps32);
* dv = sum_g P_g^T dO_g is one fp32 chain over the G heads, so G T replaces T
  in its term count: (sum_g P_g^T |dO_g|) ((G T + 64) eps32 + 2^-20);
* dk and dv each get 2^-9 |ref| on top: in the single-head case dv = dout at
  T = 1 is exact in bf16, here it is a sum of G bf16 values rounded to bf16
  once, and the arm's own sum may round the other way.

tests/test_fused_gqa_attn_cpu.py checks an fp32 evaluation against these
floors at T = 1.  The same cases assert untouched guard regions, delta within
2 * 64 eps32 sum |dO O| of fp64, and a bit-equal second run.

Each case prints its figures; test_maxerr_report prints one MAXERR line per
output and family (the record is profiles/r12/gqa_attn_maxerr.txt).
"""
import copy
import functools

import pytest
import torch

from attn_bwd_floors import EPS32, floors, reference
from test_gpu_fused_attn import (CANARY_BF16, CANARY_F32, GUARD, MARGIN, SCALE,
                                 _errs, _guarded, _make_qkv, _priority)

pytestmark = pytest.mark.gpu

B, HKV = 2, 2
GROUPS = [2, 4, 8]
LENGTHS = [1, 17, 64, 96, 129, 192, 320]
FAMILIES = ["gauss", "pm80", "lastmax"]
LAYOUTS = ["packed", "separate"]
OUTPUTS = ("out", "lse", "dq", "dk", "dv")


def _fg():
    from sharedtensor_amd.ops import fused_gqa_attn
    return fused_gqa_attn


def expand(t, G):
    return t.repeat_interleave(G, dim=1)


def group_sum(t, G):
    b, h, T, d = t.shape
    return t.view(b, h // G, G, T, d).sum(2)


def gqa_reference(q, k, v, dout, G, scale):
    """fp64 out, lse, P, dq, dk, dv; dk and dv summed over the group."""
    ref = reference(q, expand(k, G), expand(v, G), dout, scale)
    T = q.shape[2]
    vis = torch.ones(T, T, device=q.device, dtype=torch.bool).tril()
    s = (q.double() @ expand(k, G).double().transpose(-1, -2)) * scale
    ref["lse"] = torch.logsumexp(s.masked_fill(~vis, float("-inf")), dim=-1)
    ref["dk1"], ref["dv1"] = ref["dk"], ref["dv"]  # per query head
    ref["dk"], ref["dv"] = group_sum(ref["dk"], G), group_sum(ref["dv"], G)
    return ref


def gqa_floors(ref, q, k, v, dout, G, scale):
    """Element-wise floors of the five outputs (derived in the docstring)."""
    T = q.shape[2]
    ke, ve = expand(k, G), expand(v, G)
    one = floors(ref, q, ke, ve, dout, scale)
    p_do = group_sum(ref["P"].transpose(-1, -2) @ dout.double().abs(), G)
    return dict(
        out=(ref["P"] @ ve.double().abs()) * ((T + 64) * EPS32 + 2.0 ** -20),
        lse=torch.full_like(ref["lse"],
                            2 * EPS32 * max(1.0, ref["lse"].abs().max().item())),
        dq=one["dq"],
        dk=group_sum(one["dk"], G) + 2.0 ** -9 * ref["dk"].abs(),
        dv=p_do * ((G * T + 64) * EPS32 + 2.0 ** -20)
        + 2.0 ** -9 * ref["dv"].abs())


def _inputs(G, T, family, layout, seed):
    """bf16 q (B, Hq, T, 64) and k, v (B, HKV, T, 64) views."""
    hq = G * HKV
    q, k, v = _make_qkv(B, hq, T, "gauss", seed)  # (B, T, hq, 64) fp32
    k, v = k[:, :, :HKV].contiguous(), v[:, :, :HKV].contiguous()
    if family == "pm80":  # raw group scores reach +-80
        s = torch.einsum("bthd,bshd->bhts", q.bfloat16().double(),
                         k.bfloat16().double().repeat_interleave(G, dim=2))
        vis = torch.ones(T, T, device="cuda", dtype=torch.bool).tril()
        q = q * (80.0 / s.masked_fill(~vis, 0.0).abs().max().clamp_min(1e-3))
    elif family == "lastmax":  # row maximum in the last KV tile
        grow = 0.5 + 2.0 * torch.arange(T, device="cuda").float() / T
        k = k * grow.view(1, T, 1, 1)
        k[:, T - 1] = 4.0 * q[:, T - 1, ::G]
    if layout == "packed":
        qkv = torch.cat([t.reshape(B, T, -1) for t in (q, k, v)],
                        dim=2).bfloat16()
        parts = qkv.split([hq * 64, HKV * 64, HKV * 64], dim=2)
    else:  # three buffers, Llama's layout
        parts = [t.bfloat16() for t in (q, k, v)]
    return tuple(t.view(B, T, -1, 64).transpose(1, 2) for t in parts)


@functools.lru_cache(maxsize=None)
def _case(G, T, family, layout):
    fg = _fg()
    hq = G * HKV
    seed = 3000 * T + 100 * G + 10 * FAMILIES.index(family) \
        + LAYOUTS.index(layout)
    q, k, v = _inputs(G, T, family, layout, seed)
    g = torch.Generator(device="cuda").manual_seed(seed + 1)
    dout = torch.randn(B, T, hq, 64, device="cuda",
                       generator=g).bfloat16().transpose(1, 2)
    ref = gqa_reference(q, k, v, dout, G, SCALE)
    fl = gqa_floors(ref, q, k, v, dout, G, SCALE)
    # today's path: aten on expanded K/V, bf16 dk/dv summed over the group
    ke, ve = expand(k, G), expand(v, G)
    with _priority():
        a_out, a_lse, seed_, off = \
            torch.ops.aten._scaled_dot_product_efficient_attention(
                q, ke, ve, None, True, 0.0, True, scale=SCALE)
        a_dq, a_dk, a_dv, _ = \
            torch.ops.aten._scaled_dot_product_efficient_attention_backward(
                dout, q, ke, ve, None, a_out, a_lse, seed_, off, 0.0,
                [True, True, True, False], True, scale=SCALE)
    arm = dict(out=a_out, lse=a_lse, dq=a_dq, dk=group_sum(a_dk, G),
               dv=group_sum(a_dv, G))

    def run():
        shapes = dict(out=(B, T, hq, 64), dq=(B, T, hq, 64),
                      dk=(B, T, HKV, 64), dv=(B, T, HKV, 64))
        bufs, x = {}, {}
        for n, shp in shapes.items():
            bufs[n], x[n] = _guarded(shp, torch.bfloat16, CANARY_BF16)
        for n in ("lse", "delta"):
            bufs[n], x[n] = _guarded((B, hq, T), torch.float32, CANARY_F32)
        fg.gqa_forward(q, k, v, SCALE, out=x["out"], lse=x["lse"])
        x["out"] = x["out"].transpose(1, 2)
        x["dq"], x["dk"], x["dv"] = fg.gqa_backward(
            q, k, v, x["out"], x["lse"], dout, SCALE,
            *(x[n].transpose(1, 2) for n in ("dq", "dk", "dv")),
            delta=x["delta"])
        torch.cuda.synchronize()
        return x, bufs

    got, bufs = run()
    again, _ = run()
    return dict(ref=ref, fl=fl, arm=arm, got=got, again=again, bufs=bufs,
                dout=dout)


def _figures(c, name):
    ref = c["ref"][name]
    f_abs, f_l2 = _errs(c["got"][name], ref)
    a_abs, a_l2 = _errs(c["arm"][name], ref)
    norm = ref.norm().item()
    if norm == 0:  # no relative figure against an identically zero reference
        f_l2 = a_l2 = 0.0
    return dict(f_abs=f_abs, f_l2=f_l2, a_abs=a_abs, a_l2=a_l2,
                fl_abs=c["fl"][name].max().item(),
                fl_l2=c["fl"][name].norm().item() / norm if norm else 0.0)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("T", LENGTHS)
@pytest.mark.parametrize("G", GROUPS)
def test_gqa_against_fp64(G, T, family, layout):
    c = _case(G, T, family, layout)
    got = c["got"]
    for buf in c["bufs"].values():  # guards untouched
        canary = CANARY_BF16 if buf.dtype == torch.bfloat16 else CANARY_F32
        g = torch.full((GUARD,), canary, dtype=buf.dtype, device="cuda")
        assert torch.equal(buf[:GUARD], g) and torch.equal(buf[-GUARD:], g)
    prod = c["dout"].double() * got["out"].double()
    d_err = (got["delta"].double() - prod.sum(-1)).abs()
    assert (d_err <= 2 * 64 * EPS32 * prod.abs().sum(-1)).all(), d_err.max()
    for name in OUTPUTS + ("delta",):
        assert torch.isfinite(got[name].float()).all(), name
        assert torch.equal(got[name], c["again"][name]), f"{name}: repeat differs"
    for name in OUTPUTS:
        assert got[name].shape == c["ref"][name].shape, name
        f = _figures(c, name)
        print(f"GQA G={G} T={T} {family} {layout} {name}: maxabs fused "
              f"{f['f_abs']:.3e} arm {f['a_abs']:.3e} floor {f['fl_abs']:.3e}"
              f" | rel-l2 fused {f['f_l2']:.3e} arm {f['a_l2']:.3e} floor "
              f"{f['fl_l2']:.3e}")
        assert f["f_abs"] <= max(MARGIN * f["a_abs"], f["fl_abs"]), name
        assert f["f_l2"] <= max(MARGIN * f["a_l2"], f["fl_l2"]), name


def test_maxerr_report():
    for fam in FAMILIES:
        for name in OUTPUTS:
            w = dict(f_abs=0.0, a_abs=0.0, f_l2=0.0, a_l2=0.0)
            for G in GROUPS:
                for T in LENGTHS:
                    for lay in LAYOUTS:
                        f = _figures(_case(G, T, fam, lay), name)
                        w = {k: max(w[k], f[k]) for k in w}
            print(f"MAXERR gqa_attn {name} {fam}: maxabs fused "
                  f"{w['f_abs']:.3e} arm {w['a_abs']:.3e} rel-l2 fused "
                  f"{w['f_l2']:.3e} arm {w['a_l2']:.3e}")


def test_module_gradients_flag_on_and_off(monkeypatch):
    """One LlamaAttention (G = 4), forward + backward, with FUSE_GQA_ATTN on
    and off, each against a deep copy in fp64; gqa_backward runs exactly when
    the flag says so."""
    from sharedtensor_amd.models import llama
    fg = _fg()
    monkeypatch.delenv("SHTENS_FUSED_GQA_ATTN", raising=False)
    cfg = llama.LlamaConfig(vocab_size=64, n_layer=1, n_head=8, n_kv_head=2,
                            dim=512, ffn_dim=512, block_size=256)
    torch.manual_seed(3)
    mod = llama.LlamaAttention(cfg).cuda().bfloat16()
    cos, sin = llama.rope_freqs(64, 160, cfg.rope_theta, "cuda")
    x = torch.randn(2, 160, 512, device="cuda").bfloat16()
    dy = torch.randn(2, 160, 512, device="cuda").bfloat16()
    names = ["wq.weight", "wk.weight", "wv.weight", "wo.weight"]

    calls = []
    real = fg.gqa_backward
    monkeypatch.setattr(fg, "gqa_backward",
                        lambda *a, **k: (calls.append(1), real(*a, **k))[1])

    def run(m, xx, dd, flag):
        monkeypatch.setattr(llama, "FUSE_GQA_ATTN", flag)
        m.zero_grad(set_to_none=True)
        m(xx, cos, sin).backward(dd)
        p = dict(m.named_parameters())
        return [p[n].grad.clone() for n in names]

    on = run(mod, x, dy, True)
    assert len(calls) == 1, "flag on: gqa_backward did not run once"
    off = run(mod, x, dy, False)
    ref = run(copy.deepcopy(mod).double(), x.double(), dy.double(), True)
    assert len(calls) == 1, "flag off or fp64: gqa_backward ran"
    for name, r, f, a in zip(names, ref, on, off):
        f_abs, f_l2 = _errs(f, r)
        a_abs, a_l2 = _errs(a, r)
        print(f"GQA module {name}: maxabs fused {f_abs:.3e} current "
              f"{a_abs:.3e} | rel-l2 fused {f_l2:.3e} current {a_l2:.3e}")
        assert f_abs <= MARGIN * a_abs
        assert f_l2 <= MARGIN * a_l2


def test_can_use_rejections_on_device():
    fg = _fg()
    mk = lambda *s, dt=torch.bfloat16: torch.zeros(*s, device="cuda", dtype=dt)
    q, kv = mk(2, 8, 16, 64), mk(2, 2, 16, 64)
    assert fg.can_use(q, kv, kv)
    f8, f2 = (mk(2, h, 16, 64, dt=torch.float32) for h in (8, 2))
    odd = mk(2, 8, 16, 68)[..., 2:66]  # stride 68, base off by 4 B
    bad = [(f8, f2, f2),                                  # fp32
           (mk(2, 8, 16, 32), mk(2, 2, 16, 32), mk(2, 2, 16, 32)),
           (q, q, q),                                     # Hq == Hkv
           (mk(2, 6, 16, 64), kv, kv),                    # G = 3
           (mk(2, 5, 16, 64), kv, kv),                    # Hq % Hkv != 0
           (q, mk(2, 2, 8, 64), mk(2, 2, 8, 64)),         # Tq != Tk
           (odd, kv, kv)]                                 # misaligned view
    for args in bad:
        assert not fg.can_use(*args)
        with pytest.raises(ValueError):
            fg.gqa_forward(*args)
