"""csrc/gqa_attn_hd128_kernels.hip and ops/fused_gqa_attn.py at D = 128 against
fp64 attention over repeat_interleave'd K/V, under the rules of
test_gpu_fused_attn.py: MARGIN times the error of the aten path on expanded
K/V, the floor (128 score terms, not 64) only where that is about zero;
gradients MARGIN times SDPA enable_gqa's, no floor.  Tiles and position
blocks are those of head dim 64, so the lengths are the ones used there."""
import copy
import functools

import pytest
import torch

from sharedtensor_amd.ops import fused_gqa_attn as fg
from test_gpu_fused_attn import (CANARY_BF16, CANARY_F32, EPS32, GUARD, MARGIN,
                                 _errs, _guarded, _priority)
from test_gpu_fused_gqa_attn import expand, gqa_reference

pytestmark = pytest.mark.gpu

B, HKV, D = 2, 2, 128
SCALE = D ** -0.5
FAMILIES = ["gauss", "pm80", "lastmax"]
LAYOUTS = ["packed", "separate"]


@functools.lru_cache(maxsize=None)
def _inputs(G, T, family, layout):
    """bf16 q, dout (B, Hq, T, 128), k, v (B, HKV, T, 128) views and their
    fp64 reference; families and layouts of test_gpu_fused_gqa_attn.py."""
    hq = G * HKV
    g = torch.Generator(device="cuda").manual_seed(
        3000 * T + 100 * G + 10 * FAMILIES.index(family)
        + LAYOUTS.index(layout))
    q, k, v = (torch.randn(B, T, h, D, device="cuda", generator=g)
               for h in (hq, HKV, HKV))
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
        parts = qkv.split([hq * D, HKV * D, HKV * D], dim=2)
    else:  # three buffers, Llama's layout
        parts = [t.bfloat16() for t in (q, k, v)]
    q, k, v = (t.view(B, T, -1, D).transpose(1, 2) for t in parts)
    do = torch.randn(B, hq, T, D, device="cuda", generator=g).bfloat16()
    return q, k, v, do, gqa_reference(q, k, v, do, G, SCALE)


def _held(tag, fused, arm, ref, fl_abs=0.0, fl_l2=0.0):
    (f_abs, f_l2), (a_abs, a_l2) = _errs(fused, ref), _errs(arm, ref)
    print(f"GQA128 {tag}: maxabs, rel-l2 fused {f_abs:.3e} {f_l2:.3e} arm "
          f"{a_abs:.3e} {a_l2:.3e} floor {fl_abs:.3e} {fl_l2:.3e}")
    assert torch.isfinite(fused.float()).all(), tag
    assert f_abs <= max(MARGIN * a_abs, fl_abs), tag
    assert f_l2 <= max(MARGIN * a_l2, fl_l2), tag


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("T", [1, 17, 64, 96, 129, 192, 320])
@pytest.mark.parametrize("G", [2, 4, 8])
def test_forward_against_fp64(G, T, family, layout):
    q, k, v, _, ref = _inputs(G, T, family, layout)
    o_ref, l_ref = ref["out"], ref["lse"]
    ve = expand(v, G)
    with _priority():
        a_out, a_lse, _, _ = \
            torch.ops.aten._scaled_dot_product_efficient_attention(
                q, expand(k, G), ve, None, True, 0.0, True, scale=SCALE)

    def run():
        obuf, out = _guarded((B, T, G * HKV, D), torch.bfloat16, CANARY_BF16)
        lbuf, lse = _guarded((B, G * HKV, T), torch.float32, CANARY_F32)
        fg.gqa_forward(q, k, v, SCALE, out=out, lse=lse)
        torch.cuda.synchronize()
        return out.transpose(1, 2), lse, (obuf, lbuf)

    out, lse, bufs = run()
    out2, lse2, _ = run()
    assert torch.equal(out, out2) and torch.equal(lse, lse2), "repeat differs"
    for buf, canary in zip(bufs, (CANARY_BF16, CANARY_F32)):
        g = torch.full((GUARD,), canary, dtype=buf.dtype, device="cuda")
        assert torch.equal(buf[:GUARD], g) and torch.equal(buf[-GUARD:], g)
    for x, a in ((lse, a_lse), (out, a_out)):  # the aten op's layout
        assert (x.shape, x.dtype, x.stride()) == (a.shape, a.dtype, a.stride())
    fl = (ref["P"] @ ve.double().abs()) * ((T + D) * EPS32 + 2.0 ** -20)
    tag = f"G={G} T={T} {family} {layout}"
    _held(tag + " out", out, a_out, o_ref, fl.max().item(),
          (fl.norm() / o_ref.norm().clamp_min(1e-300)).item())
    fl_lse = 2 * EPS32 * max(1.0, l_ref.abs().max().item())
    _held(tag + " lse", lse, a_lse, l_ref, fl_lse,
          fl_lse * l_ref.numel() ** 0.5 / l_ref.norm().clamp_min(1e-300).item())


@pytest.mark.parametrize("T", [96, 129])
def test_gradients_through_the_function(T):
    G = 4
    q, k, v, do, ref = _inputs(G, T, "gauss", "separate")  # ref: fp64 autograd

    def grads(fn):
        xs = [x.detach().requires_grad_() for x in (q, k, v)]
        fn(*xs).backward(do)
        return [x.grad for x in xs]

    def sdpa(q, k, v):
        with _priority():
            return torch.nn.functional.scaled_dot_product_attention(
                q, k, v, is_causal=True, scale=SCALE, enable_gqa=True)

    fused = grads(lambda q, k, v: fg.fused_causal_gqa_attention(q, k, v, SCALE))
    for name, f, a in zip(("dq", "dk", "dv"), fused, grads(sdpa)):
        assert f.shape == ref[name].shape and f.dtype == torch.bfloat16
        _held(f"bwd T={T} {name}", f, a, ref[name])


def test_module_gradients_flag_on_and_off(monkeypatch):
    """One LlamaAttention at head dim 128, G = 4, against an fp64 deep copy;
    gqa_forward runs exactly when FUSE_GQA_ATTN_HD128 says so."""
    from sharedtensor_amd.models import llama
    monkeypatch.delenv("SHTENS_FUSED_GQA_ATTN_HD128", raising=False)
    cfg = llama.LlamaConfig(vocab_size=64, n_layer=1, n_head=8, n_kv_head=2,
                            dim=1024, ffn_dim=512, block_size=256)
    torch.manual_seed(3)
    mod = llama.LlamaAttention(cfg).cuda().bfloat16()
    cos, sin = llama.rope_freqs(D, 160, cfg.rope_theta, "cuda")
    x = torch.randn(2, 160, 1024, device="cuda").bfloat16()
    dy = torch.randn(2, 160, 1024, device="cuda").bfloat16()
    names = ["wq.weight", "wk.weight", "wv.weight", "wo.weight"]
    calls = []
    real = fg.gqa_forward
    monkeypatch.setattr(fg, "gqa_forward",
                        lambda *a, **k: (calls.append(1), real(*a, **k))[1])

    def run(m, xx, dd, flag):
        monkeypatch.setattr(llama, "FUSE_GQA_ATTN_HD128", flag)
        m.zero_grad(set_to_none=True)
        m(xx, cos, sin).backward(dd)
        p = dict(m.named_parameters())
        return [p[n].grad.clone() for n in names]

    on = run(mod, x, dy, True)
    assert len(calls) == 1, "flag on: gqa_forward did not run once"
    off = run(mod, x, dy, False)
    ref = run(copy.deepcopy(mod).double(), x.double(), dy.double(), True)
    assert len(calls) == 1, "flag off or fp64: gqa_forward ran"
    for name, r, f, a in zip(names, ref, on, off):
        _held(f"module {name}", f, a, r)


def test_can_use_on_device():
    mk = lambda *s, dt=torch.bfloat16: torch.zeros(*s, device="cuda", dtype=dt)
    q, kv = mk(2, 8, 16, D), mk(2, 2, 16, D)
    assert fg.can_use(q, kv, kv)
    lse = mk(2, 8, 16, dt=torch.float32)
    assert not fg.can_use_backward(q, kv, kv, q, lse, q)
    for d in (96, 256):
        assert not fg.can_use(*(mk(2, h, 16, d) for h in (8, 2, 2)))
    f8, f2 = (mk(2, h, 16, D, dt=torch.float32) for h in (8, 2))
    odd = mk(2, 8, 16, D + 4)[..., 2:D + 2]  # stride 132, base off by 4 B
    for args in [(mk(2, 6, 16, D), kv, kv),                  # G = 3
                 (q, mk(2, 2, 8, D), mk(2, 2, 8, D)),        # Tq != Tk
                 (f8, f2, f2),                               # fp32
                 (odd, kv, kv)]:                             # misaligned view
        assert not fg.can_use(*args)
        with pytest.raises(ValueError):
            fg.gqa_forward(*args)
