"""Fused bf16 RoPE (csrc/rope_kernels.hip): forward bit-equal to the eager
`apply_rope`, backward within one bf16 rounding of an fp64 reference."""
import functools

import pytest
import torch

from sharedtensor_amd import _core
from sharedtensor_amd.models.llama import (LlamaAttention, LlamaConfig,
                                           apply_rope, rope_freqs)
from sharedtensor_amd.ops import fused_rope

pytestmark = pytest.mark.gpu

THETA = 500000.0

# (B, Hq, Hkv, T, D, table rows)
SHAPES = [
    (2, 3, 1, 5, 8, 5),       # smallest vector case, odd T and H, GQA
    (1, 4, 2, 33, 64, 33),    # tail rows
    (2, 2, 2, 64, 128, 64),   # Llama-8B head dim, MHA
    (1, 2, 1, 7, 6, 7),       # scalar-pair path, D % 8 != 0
    (1, 4, 2, 9, 64, 64),     # table longer than T: wrong-row-stride catch
]
IDS = ["x".join(map(str, s)) for s in SHAPES]


def _model_layout(B, H, T, D):
    # as the model hands q/k over: (B,T,H,D) storage viewed as (B,H,T,D)
    return torch.randn(B, T, H, D, device="cuda").bfloat16().transpose(1, 2)


def grad_reference(g, cos, sin):
    """fp64 gradient of the rotation for upstream g (B,H,T,D) and its bound:
    r1 = g1*c + g2*s, r2 = g2*c - g1*s;
    |fused - r| <= 2^-8 |r| + 2^-22 (|ga*c| + |gb*s|) + 2^-133
    (half a bf16 ulp; three fp32 roundings under cancellation; the bf16
    subnormal floor)."""
    T = g.shape[2]
    c, s = cos[:T].double(), sin[:T].double()
    g1, g2 = g[..., 0::2].double(), g[..., 1::2].double()
    r1, r2 = g1 * c + g2 * s, g2 * c - g1 * s
    b1 = 2.0 ** -8 * r1.abs() + 2.0 ** -22 * ((g1 * c).abs() + (g2 * s).abs())
    b2 = 2.0 ** -8 * r2.abs() + 2.0 ** -22 * ((g2 * c).abs() + (g1 * s).abs())
    ref = torch.stack((r1, r2), dim=-1).flatten(-2)
    bound = torch.stack((b1, b2), dim=-1).flatten(-2) + 2.0 ** -133
    return ref, bound


def assert_grad_within_bound(grad, ref, bound):
    err = (grad.double() - ref).abs()
    bad = int((err > bound).sum())
    worst = float((err / bound).max())
    print(f"grad violations={bad}/{err.numel()} worst err/bound={worst:.3f}")
    assert bad == 0, (bad, err.numel(), worst)


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Inputs, upstream gradients and references for one shape; computed
    once and shared (nothing below writes to them)."""
    B, Hq, Hkv, T, D, rows = shape
    torch.manual_seed(sum(shape))
    q = _model_layout(B, Hq, T, D)
    k = _model_layout(B, Hkv, T, D)
    gq = torch.randn(B, Hq, T, D, device="cuda").bfloat16()
    gk = torch.randn(B, Hkv, T, D, device="cuda").bfloat16()
    cos, sin = rope_freqs(D, rows, THETA, "cuda")
    return dict(q=q, k=k, gq=gq, gk=gk, cos=cos, sin=sin,
                eager_q=apply_rope(q, cos, sin),
                eager_k=apply_rope(k, cos, sin),
                ref_q=grad_reference(gq, cos, sin),
                ref_k=grad_reference(gk, cos, sin))


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_forward_bit_equal_to_eager(shape):
    c = _case(shape)
    assert not c["q"].is_contiguous()  # the strided-read path is under test
    assert fused_rope.can_use(c["q"], c["k"], c["cos"], c["sin"])
    qr, kr = fused_rope.fused_rope_qk(c["q"], c["k"], c["cos"], c["sin"])
    for out, eager, x in ((qr, c["eager_q"], c["q"]),
                          (kr, c["eager_k"], c["k"])):
        assert out.dtype == torch.bfloat16 and out.shape == x.shape
        assert out.is_contiguous()
        assert torch.equal(out, eager)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_backward_against_fp64(shape):
    c = _case(shape)
    q = c["q"].detach().requires_grad_(True)
    k = c["k"].detach().requires_grad_(True)
    qr, kr = fused_rope.fused_rope_qk(q, k, c["cos"], c["sin"])
    dq, dk = torch.autograd.grad((qr, kr), (q, k), (c["gq"], c["gk"]))
    for g, x, (ref, bound) in ((dq, q, c["ref_q"]), (dk, k, c["ref_k"])):
        assert g.dtype == torch.bfloat16 and g.shape == x.shape
        # aliases (B,T,H,D)-contiguous storage: the view backward is free
        assert g.transpose(1, 2).is_contiguous()
        assert_grad_within_bound(g, ref, bound)


def test_backward_accepts_strided_upstream_gradient():
    """SDPA's backward may hand over gradients in any layout; a (B,T,H,D)
    upstream exercises the strided-read side of the inverse launch."""
    c = _case(SHAPES[1])
    q = c["q"].detach().requires_grad_(True)
    k = c["k"].detach().requires_grad_(True)
    qr, kr = fused_rope.fused_rope_qk(q, k, c["cos"], c["sin"])
    gq = c["gq"].transpose(1, 2).contiguous().transpose(1, 2)
    gk = torch.stack((c["gk"], c["gk"]), dim=-1)[..., 0]  # last stride 2
    assert gk.stride(-1) != 1 and not gq.is_contiguous()
    dq, dk = torch.autograd.grad((qr, kr), (q, k), (gq, gk))
    assert_grad_within_bound(dq, *c["ref_q"])
    assert_grad_within_bound(dk, *c["ref_k"])


def _bht(x):
    return (x.stride(0), x.stride(1), x.stride(2))


def _binding(q, k, cos, sin, inverse):
    qo = torch.empty(q.shape, dtype=q.dtype, device=q.device)
    ko = torch.empty(k.shape, dtype=k.dtype, device=k.device)
    s = torch.cuda.current_stream().cuda_stream
    _core.rope_qk(q.data_ptr(), k.data_ptr(), qo.data_ptr(), ko.data_ptr(),
                  cos.data_ptr(), sin.data_ptr(), q.shape[0], q.shape[1],
                  k.shape[1], q.shape[2], q.shape[3], _bht(q), _bht(k),
                  _bht(qo), _bht(ko), inverse, s)
    return qo, ko


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_inverse_round_trip_through_binding(shape):
    """forward then inverse returns the input to within 2 bf16 ulp.

    Each direction rounds each component once, by at most half a bf16 ulp
    of a value no larger than the pair's norm r (a rotation preserves r), so
    the ulp is taken at r: the forward error vector has norm <= ulp(r)/sqrt2,
    the inverse rotation preserves it, and the second rounding adds at most
    ulp(r) when the result crosses into the next binade — 1.71 ulp(r) in
    all.  (An ulp at each element's own magnitude cannot hold for any
    rounding implementation: a small component next to a large one loses
    its low bits in the rotated pair.)"""
    c = _case(shape)
    cos, sin = c["cos"], c["sin"]
    y_q, y_k = _binding(c["q"], c["k"], cos, sin, False)
    assert torch.equal(y_q, c["eager_q"]) and torch.equal(y_k, c["eager_k"])
    z_q, z_k = _binding(y_q, y_k, cos, sin, True)
    for z, x in ((z_q, c["q"]), (z_k, c["k"])):
        xd = x.double()
        r = (xd[..., 0::2] ** 2 + xd[..., 1::2] ** 2).sqrt()
        _, e = torch.frexp(r)                      # r = m * 2^e, m in [.5, 1)
        ulp = torch.ldexp(torch.ones_like(r), e - 8)
        ulp = torch.where(r > 0, ulp, torch.zeros_like(r))
        ulp = ulp.repeat_interleave(2, dim=-1)
        err = (z.double() - xd).abs()
        print(f"round trip worst err/ulp(r)={float((err / ulp).max()):.3f}")
        assert bool((err <= 2 * ulp).all())
    # k absent: q alone, same result, nothing read through the null pointer
    qo = torch.empty_like(y_q)
    _core.rope_qk(c["q"].data_ptr(), 0, qo.data_ptr(), 0, cos.data_ptr(),
                  sin.data_ptr(), *c["q"].shape[:2], 0, *c["q"].shape[2:],
                  _bht(c["q"]), (0, 0, 0), _bht(qo), (0, 0, 0), False,
                  torch.cuda.current_stream().cuda_stream)
    assert torch.equal(qo, y_q)


def test_binding_rejects_bad_arguments():
    x = torch.zeros(1, 1, 2, 7, dtype=torch.bfloat16, device="cuda")
    t = torch.zeros(2, 4, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    with pytest.raises(RuntimeError):  # odd D
        _core.rope_qk(x.data_ptr(), 0, x.data_ptr(), 0, t.data_ptr(),
                      t.data_ptr(), 1, 1, 0, 2, 7, _bht(x), (0, 0, 0),
                      _bht(x), (0, 0, 0), False, s)
    with pytest.raises(RuntimeError):  # null table
        _core.rope_qk(x.data_ptr(), 0, x.data_ptr(), 0, 0, t.data_ptr(), 1,
                      1, 0, 2, 6, _bht(x), (0, 0, 0), _bht(x), (0, 0, 0),
                      False, s)


def test_op_rejects_inputs_the_kernel_would_misread():
    """fused_rope_qk called directly (without can_use) raises before any
    launch on a dtype, table or shape the kernel cannot address."""
    c = _case(SHAPES[1])
    q, k, cos, sin = c["q"], c["k"], c["cos"], c["sin"]
    bad = [
        (q.float(), k, cos, sin),                  # fp32 activation
        (q, k.float(), cos, sin),
        (q, k, cos[:-1], sin[:-1]),                # table shorter than T
        (q, k, cos[:, :-1], sin[:, :-1]),          # wrong width, strided
        (q, k, cos.double(), sin.double()),
        (q, k[:, :, :-1], cos, sin),               # k does not share T
        (q[..., :7], k[..., :7], cos[:, :3], sin[:, :3]),  # odd D
        (q.cpu(), k.cpu(), cos.cpu(), sin.cpu()),
    ]
    for args in bad:
        with pytest.raises(ValueError):
            fused_rope.fused_rope_qk(*args)


def test_partial_gradients():
    c = _case(SHAPES[1])
    q = c["q"].detach().requires_grad_(True)
    k = c["k"].detach().requires_grad_(True)
    qr, _ = fused_rope.fused_rope_qk(q, k, c["cos"], c["sin"])
    (qr.float() * c["gq"].float()).sum().backward()
    assert_grad_within_bound(q.grad, *c["ref_q"])
    assert k.grad is None or not bool(k.grad.any())
    # and the other way round, with q not requiring a gradient at all
    k2 = c["k"].detach().requires_grad_(True)
    _, kr = fused_rope.fused_rope_qk(c["q"], k2, c["cos"], c["sin"])
    (dk,) = torch.autograd.grad(kr, k2, c["gk"])
    assert_grad_within_bound(dk, *c["ref_k"])


def _attn_setup():
    torch.manual_seed(3)
    cfg = LlamaConfig.tiny()
    attn = LlamaAttention(cfg).cuda().to(torch.bfloat16)
    x = torch.randn(2, 33, cfg.dim, device="cuda").bfloat16()
    cos, sin = rope_freqs(cfg.dim // cfg.n_head, cfg.block_size,
                          cfg.rope_theta, "cuda")
    return cfg, attn, x, cos, sin


def test_model_path(monkeypatch):
    cfg, attn, x, cos, sin = _attn_setup()
    B, T, _ = x.shape
    q = attn.wq(x).view(B, T, attn.n_head, attn.head_dim).transpose(1, 2)
    k = attn.wk(x).view(B, T, attn.n_kv, attn.head_dim).transpose(1, 2)
    assert fused_rope.can_use(q, k, cos, sin)

    calls = []
    real = fused_rope.fused_rope_qk
    monkeypatch.setattr(fused_rope, "fused_rope_qk",
                        lambda *a: (calls.append(1), real(*a))[1])
    y = attn(x, cos, sin)
    y.float().square().sum().backward()
    assert len(calls) == 1
    grads = {n: p.grad.clone() for n, p in attn.named_parameters()}
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())
    assert all(bool(g.any()) for g in grads.values())

    monkeypatch.setenv("SHTENS_NO_FUSED_ROPE", "1")
    assert not fused_rope.can_use(q, k, cos, sin)
    y_eager = attn(x, cos, sin)
    assert len(calls) == 1  # the knob routed this run through apply_rope
    assert torch.equal(y, y_eager)
    monkeypatch.delenv("SHTENS_NO_FUSED_ROPE")

    # fallbacks: fp32, CPU and an odd head dim are refused ...
    assert not fused_rope.can_use(q.float(), k.float(), cos, sin)
    assert not fused_rope.can_use(q.cpu(), k.cpu(), cos.cpu(), sin.cpu())
    assert not fused_rope.can_use(q[..., :7], k[..., :7], cos[:, :3],
                                  sin[:, :3])
    # ... and the module still runs where eager RoPE itself is defined
    # (an odd head dim has no pairing, fused or eager)
    a32 = LlamaAttention(cfg).cuda()
    assert a32(x.float(), cos, sin).dtype == torch.float32
    acpu = LlamaAttention(cfg)
    assert acpu(x.float().cpu(), cos.cpu(), sin.cpu()).shape == x.shape
    assert len(calls) == 1


def test_training_equivalence_small_llama(monkeypatch):
    """A few training steps with fused vs eager RoPE must track."""
    from sharedtensor_amd.models.llama import Llama
    losses = {}
    for tag in ("fused", "torch"):
        if tag == "torch":
            monkeypatch.setenv("SHTENS_NO_FUSED_ROPE", "1")
        torch.manual_seed(7)
        cfg = LlamaConfig.tiny()
        m = Llama(cfg).cuda().to(torch.bfloat16)
        opt = torch.optim.SGD(m.parameters(), lr=0.05)
        x = torch.randint(0, cfg.vocab_size, (2, 33), device="cuda")
        ls = []
        for _ in range(8):
            opt.zero_grad()
            _, loss = m(x[:, :-1], x[:, 1:])
            loss.float().backward()
            opt.step()
            ls.append(float(loss.detach()))
        losses[tag] = ls
    print(losses)
    for a, b in zip(losses["fused"], losses["torch"]):
        assert abs(a - b) < 0.15, (losses["fused"], losses["torch"])
