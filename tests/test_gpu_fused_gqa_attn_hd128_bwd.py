"""csrc/gqa_attn_hd128_bwd_kernels.hip and ops.fused_gqa_attn.gqa_backward_hd128
against fp64 attention over repeat_interleave'd K/V (gqa_reference: dk and dv
summed over the group), on the inputs of test_gpu_fused_gqa_attn_hd128.py.

Tolerance.  Nothing is fixed in advance: max-abs and relative-L2 error of dq,
dk and dv may be at most MARGIN (1.5, test_gpu_fused_attn.py) times the error
of today's path, the gradients of fused_causal_gqa_attention with its default
backward (aten on expanded K/V, bf16 dk and dv summed over the group) on the
same inputs and dout.  A floor takes over only where that error is about zero
(T = 1) and counts the fp32 operations alone, by the derivation in
test_gpu_fused_attn_bwd.py and test_gpu_fused_gqa_attn.py with 128-term sums
(one fma chain per lane half for delta, one MFMA chain each for S and dP):

* floor_dS = A (260 eps32 + 2^-20), 260 = 2 * 128 + 4,
  A = P (|dO| |V|^T + sum |dO| |O|);
* dq: scale floor_dS |K| per query head; dk: scale floor_dS^T |Q| summed over
  the group;
* floor_dv = (sum_g P_g^T |dO_g|) ((G T + 128) eps32 + 2^-20);
* dk and dv each get 2^-9 |ref| on top, for the single final rounding.

A gradient whose reference is identically zero (dq, dk at T = 1) has no
relative figure.  delta is held to 2 * 128 eps32 sum |dO O| of fp64.  Each case
also asserts untouched guard regions and a bit-equal second run, and prints
its figures (the worst per gradient and family:
profiles/r18/gqa_attn_hd128_bwd_maxerr.txt)."""
import copy

import pytest
import torch

from sharedtensor_amd.ops import fused_gqa_attn as fg
from test_gpu_fused_attn import (CANARY_BF16, CANARY_F32, EPS32, GUARD, MARGIN,
                                 _errs, _guarded)
from test_gpu_fused_gqa_attn import expand, group_sum
from test_gpu_fused_gqa_attn_hd128 import B, D, HKV, SCALE, _inputs

pytestmark = pytest.mark.gpu

NAMES = ("dq", "dk", "dv")


def _floors(ref, q, k, v, do, G):
    qa, ka, va, da = (t.double().abs() for t in (q, expand(k, G), expand(v, G),
                                                 do))
    a = ref["P"] * (da @ va.transpose(-1, -2)
                    + (da * ref["out"].abs()).sum(-1, keepdim=True))
    f_ds = a * (260 * EPS32 + 2.0 ** -20)
    p_do = group_sum(ref["P"].transpose(-1, -2) @ da, G)
    return dict(
        dq=SCALE * (f_ds @ ka),
        dk=group_sum(SCALE * (f_ds.transpose(-1, -2) @ qa), G)
        + 2.0 ** -9 * ref["dk"].abs(),
        dv=p_do * ((G * q.shape[2] + D) * EPS32 + 2.0 ** -20)
        + 2.0 ** -9 * ref["dv"].abs())


@pytest.mark.parametrize("layout", ["packed", "separate"])
@pytest.mark.parametrize("family", ["gauss", "pm80"])
@pytest.mark.parametrize("T", [1, 17, 64, 96, 129, 192, 320])
@pytest.mark.parametrize("G", [2, 4, 8])
def test_backward_against_fp64(G, T, family, layout):
    q, k, v, do, ref = _inputs(G, T, family, layout)
    hq = G * HKV
    xs = [x.detach().requires_grad_() for x in (q, k, v)]
    fg.fused_causal_gqa_attention(*xs, SCALE).backward(do)  # today's path
    arm = dict(zip(NAMES, (x.grad for x in xs)))
    out, lse = fg.gqa_forward(q, k, v, SCALE)
    out = out.transpose(1, 2)

    def run():
        bufs, x = {}, {}
        for n, h in zip(NAMES, (hq, HKV, HKV)):
            bufs[n], x[n] = _guarded((B, T, h, D), torch.bfloat16, CANARY_BF16)
        bufs["delta"], x["delta"] = _guarded((B, hq, T), torch.float32,
                                             CANARY_F32)
        x["dq"], x["dk"], x["dv"] = fg.gqa_backward_hd128(
            q, k, v, out, lse, do, SCALE,
            *(x[n].transpose(1, 2) for n in NAMES), delta=x["delta"])
        torch.cuda.synchronize()
        return x, bufs

    got, bufs = run()
    again, _ = run()
    for buf in bufs.values():  # guards untouched
        canary = CANARY_BF16 if buf.dtype == torch.bfloat16 else CANARY_F32
        g = torch.full((GUARD,), canary, dtype=buf.dtype, device="cuda")
        assert torch.equal(buf[:GUARD], g) and torch.equal(buf[-GUARD:], g)
    for n in NAMES + ("delta",):
        assert torch.isfinite(got[n].float()).all(), n
        assert torch.equal(got[n], again[n]), f"{n}: repeat differs"
    prod = do.double() * out.double()
    d_err = (got["delta"].double() - prod.sum(-1)).abs()
    assert (d_err <= 2 * D * EPS32 * prod.abs().sum(-1)).all(), d_err.max()

    fl = _floors(ref, q, k, v, do, G)
    for n in NAMES:
        assert got[n].shape == ref[n].shape, n
        (f_abs, f_l2), (a_abs, a_l2) = _errs(got[n], ref[n]), _errs(arm[n],
                                                                    ref[n])
        norm = ref[n].norm().item()
        fl_abs, fl_l2 = fl[n].max().item(), 0.0
        if norm == 0:  # no relative figure against an identically zero ref
            f_l2 = a_l2 = 0.0
        else:
            fl_l2 = fl[n].norm().item() / norm
        print(f"GQA128BWD G={G} T={T} {family} {layout} {n}: maxabs fused "
              f"{f_abs:.3e} arm {a_abs:.3e} floor {fl_abs:.3e} | rel-l2 fused "
              f"{f_l2:.3e} arm {a_l2:.3e} floor {fl_l2:.3e}")
        assert f_abs <= max(MARGIN * a_abs, fl_abs), n
        assert f_l2 <= max(MARGIN * a_l2, fl_l2), n


def test_module_gradients_flag_on_and_off(monkeypatch):
    """One LlamaAttention at head dim 128, G = 4, T = 160, against an fp64
    deep copy; gqa_backward_hd128 runs exactly when FUSE_GQA_ATTN_HD128_BWD
    says so."""
    from sharedtensor_amd.models import llama
    for env in ("SHTENS_FUSED_GQA_ATTN_HD128", "SHTENS_FUSED_GQA_ATTN_HD128_BWD"):
        monkeypatch.delenv(env, raising=False)
    monkeypatch.setattr(llama, "FUSE_GQA_ATTN_HD128", True)
    cfg = llama.LlamaConfig(vocab_size=64, n_layer=1, n_head=8, n_kv_head=2,
                            dim=1024, ffn_dim=512, block_size=256)
    torch.manual_seed(3)
    mod = llama.LlamaAttention(cfg).cuda().bfloat16()
    cos, sin = llama.rope_freqs(D, 160, cfg.rope_theta, "cuda")
    x = torch.randn(2, 160, 1024, device="cuda").bfloat16()
    dy = torch.randn(2, 160, 1024, device="cuda").bfloat16()
    names = ["wq.weight", "wk.weight", "wv.weight", "wo.weight"]
    calls = []
    real = fg.gqa_backward_hd128
    monkeypatch.setattr(fg, "gqa_backward_hd128",
                        lambda *a, **k: (calls.append(1), real(*a, **k))[1])

    def run(m, xx, dd, flag):
        monkeypatch.setattr(llama, "FUSE_GQA_ATTN_HD128_BWD", flag)
        m.zero_grad(set_to_none=True)
        m(xx, cos, sin).backward(dd)
        p = dict(m.named_parameters())
        return [p[n].grad.clone() for n in names]

    on = run(mod, x, dy, True)
    assert len(calls) == 1, "flag on: gqa_backward_hd128 did not run once"
    off = run(mod, x, dy, False)
    ref = run(copy.deepcopy(mod).double(), x.double(), dy.double(), True)
    assert len(calls) == 1, "flag off or fp64: gqa_backward_hd128 ran"
    for name, r, f, a in zip(names, ref, on, off):
        (f_abs, f_l2), (a_abs, a_l2) = _errs(f, r), _errs(a, r)
        print(f"GQA128BWD module {name}: maxabs own {f_abs:.3e} aten "
              f"{a_abs:.3e} | rel-l2 own {f_l2:.3e} aten {a_l2:.3e}")
        assert f_abs <= MARGIN * a_abs and f_l2 <= MARGIN * a_l2, name


def test_can_use_backward_hd128_on_device():
    mk = lambda *s, dt=torch.bfloat16: torch.zeros(*s, device="cuda", dtype=dt)
    q, kv = mk(2, 8, 16, D), mk(2, 2, 16, D)
    lse = mk(2, 8, 16, dt=torch.float32)
    assert fg.can_use_backward_hd128(q, kv, kv, q, lse, q)
    q64, kv64 = mk(2, 8, 16, 64), mk(2, 2, 16, 64)
    q6 = mk(2, 6, 16, D)
    f8, f2 = (mk(2, h, 16, D, dt=torch.float32) for h in (8, 2))
    odd = mk(2, 8, 16, D + 4)[..., 2:D + 2]  # stride 132, base off by 4 B
    lse_nc = mk(2, 8, 32, dt=torch.float32)[..., ::2]
    for args in [(q64, kv64, kv64, q64, lse, q64),               # D = 64
                 (q6, kv, kv, q6, mk(2, 6, 16, dt=torch.float32), q6),  # G = 3
                 (f8, f2, f2, f8, lse, f8),                      # fp32
                 (odd, kv, kv, q, lse, q),                       # misaligned q
                 (q, kv, kv, odd, lse, q),                       # and out
                 (q, kv, kv, q, lse_nc, q)]:                     # lse strided
        assert not fg.can_use_backward_hd128(*args)
        with pytest.raises(ValueError):
            fg.gqa_backward_hd128(*args)
