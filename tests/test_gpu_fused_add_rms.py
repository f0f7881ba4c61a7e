"""Fused residual-add + RMSNorm (csrc/add_rms_kernels.hip) against an fp32
torch reference and against the unfused sequence it replaces, and the Llama
model paths that use it (residual threading, loss through the fused CE)."""
import math

import pytest
import torch
import torch.nn.functional as F

from sharedtensor_amd import _core
from sharedtensor_amd.ops import fused_ce, fused_rms

pytestmark = pytest.mark.gpu

EPS = 1e-5
# 512 (smallest), 1536, 2048, 3072 and 4096 (largest) run the wave-per-row
# kernels (every multiple of 512), 64 and 768 the fallback.  The backward
# grid holds at most add_rms_max_blocks() blocks of ROWS_PER_BLOCK rows (a
# 64-lane wave per row, 256-thread blocks), so RAGGED rows make its row loop
# iterate with a ragged tail whatever the device's size.
WIDTHS = [512, 2048, 4096, 3072, 1536, 64, 768]
ROWS_PER_BLOCK = 4
RAGGED = _core.add_rms_max_blocks() * ROWS_PER_BLOCK + 3
ROWS = [1, 5, 1000, RAGGED]


def bf16_ulp(mag: float) -> float:
    """Spacing of bf16 (8 significant bits) at magnitude `mag`."""
    return 2.0 ** (math.floor(math.log2(max(mag, 1e-30))) - 7)


def make_inputs(R, C, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)

    def rn(*shape, scale=1.0):
        return (torch.randn(*shape, device="cuda", generator=g)
                * scale).to(torch.bfloat16)
    return {"x": rn(R, C, scale=2.0), "delta": rn(R, C), "w": rn(C),
            "dy": rn(R, C), "dres": rn(R, C)}


def reference(t, x_new, has_dres):
    """fp32 autograd through RMSNorm on the bf16 x_new."""
    xn = x_new.float().requires_grad_(True)
    w = t["w"].float().requires_grad_(True)
    y = xn * torch.rsqrt(xn.pow(2).mean(-1, keepdim=True) + EPS) * w
    loss = (y * t["dy"].float()).sum()
    if has_dres:
        loss = loss + (xn * t["dres"].float()).sum()
    loss.backward()
    return {"y": y.detach(), "dx": xn.grad, "dgamma": w.grad}


def run_fused(t, has_delta, has_dres):
    x = t["x"].clone().requires_grad_(True)
    delta = t["delta"].clone().requires_grad_(True) if has_delta else None
    w = t["w"].clone().requires_grad_(True)
    x_new, y = fused_rms.fused_add_rms_norm(x, delta, w, EPS)
    loss = (y.float() * t["dy"].float()).sum()
    if has_dres:
        loss = loss + (x_new.float() * t["dres"].float()).sum()
    loss.backward()
    torch.cuda.synchronize()
    if has_delta:  # one tensor serves both inputs
        assert torch.equal(x.grad, delta.grad)
    return {"x_new": x_new.detach(), "y": y.detach().float(),
            "dx": x.grad.float(), "dgamma": w.grad.float()}


def run_unfused(t, x_new, has_dres):
    """What the fused op replaces: the block-per-row RMSNorm kernels on
    x_new, then autograd's bf16 add of the residual-path gradient."""
    R, C = x_new.shape
    s = torch.cuda.current_stream().cuda_stream
    y = torch.empty_like(x_new)
    rstd = torch.empty(R, dtype=torch.float32, device="cuda")
    _core.rms_fwd(x_new.data_ptr(), t["w"].data_ptr(), y.data_ptr(),
                  rstd.data_ptr(), R, C, EPS, s)
    dx = torch.empty_like(x_new)
    dg = torch.zeros(C, dtype=torch.float32, device="cuda")
    _core.rms_bwd(t["dy"].data_ptr(), x_new.data_ptr(), t["w"].data_ptr(),
                  rstd.data_ptr(), dx.data_ptr(), dg.data_ptr(), R, C, s)
    if has_dres:
        dx = dx + t["dres"]
    torch.cuda.synchronize()
    return {"y": y.float(), "dx": dx.float(),
            "dgamma": dg.bfloat16().float()}


def check(R, C, has_delta, has_dres):
    t = make_inputs(R, C, seed=R * 131 + C)
    got = run_fused(t, has_delta, has_dres)
    want_x_new = t["x"] + t["delta"] if has_delta else t["x"]
    # one fp32 add, one round-to-nearest-even: bit for bit torch's sum
    assert torch.equal(got["x_new"], want_x_new)
    ref = reference(t, want_x_new, has_dres)
    old = run_unfused(t, want_x_new, has_dres)

    tol = {"y": (2e-2, 2e-2), "dx": (5e-2, 5e-2), "dgamma": (3e-2, 3e-1)}
    for name, (rtol, atol) in tol.items():
        err_new = (got[name] - ref[name]).abs().max().item()
        err_old = (old[name] - ref[name]).abs().max().item()
        ulp = bf16_ulp(ref[name].abs().max().item())
        print(f"R={R} C={C} {name}: fused err {err_new:.4g}, "
              f"unfused err {err_old:.4g}, ulp {ulp:.4g}")
        torch.testing.assert_close(got[name], ref[name], rtol=rtol, atol=atol,
                                   msg=lambda m, n=name: f"{n}: {m}")
        # the fused backward rounds dx once where the old path rounds twice
        assert err_new <= err_old + ulp, (name, err_new, err_old, ulp)


@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("R", ROWS)
def test_shapes(R, C):
    check(R, C, has_delta=True, has_dres=True)


# 1024, 2560 and 3584: the multiples of 512 that WIDTHS leaves out
@pytest.mark.parametrize("R,C", [(1000, 2048), (RAGGED, 512), (5, 4096),
                                 (5, 64), (5, 1024), (5, 2560), (5, 3584)])
@pytest.mark.parametrize("has_delta,has_dres",
                         [(True, False), (False, True), (False, False)])
def test_variants(R, C, has_delta, has_dres):
    """delta absent is plain RMSNorm; d_x_new absent is the final norm,
    whose residual output nobody uses."""
    check(R, C, has_delta, has_dres)


def test_supported_widths():
    for C in range(512, 4097, 512):
        assert _core.add_rms_supported(C), C
    for C in (0, 64, 256, 768, 1280, 4608, 8192):
        assert not _core.add_rms_supported(C), C


def test_host_validation():
    t = make_inputs(4, 512, seed=1)
    s = torch.cuda.current_stream().cuda_stream
    x, d, w = t["x"], t["delta"], t["w"]
    xn, y = torch.empty_like(x), torch.empty_like(x)
    rstd = torch.empty(4, dtype=torch.float32, device="cuda")
    with pytest.raises(RuntimeError):  # unsupported width
        _core.add_rms_fwd(x.data_ptr(), d.data_ptr(), w.data_ptr(),
                          xn.data_ptr(), y.data_ptr(), rstd.data_ptr(), 4,
                          768, EPS, s)
    with pytest.raises(RuntimeError):  # misaligned pointer
        _core.add_rms_fwd(x.data_ptr() + 8, d.data_ptr(), w.data_ptr(),
                          xn.data_ptr(), y.data_ptr(), rstd.data_ptr(), 3,
                          512, EPS, s)
    with pytest.raises(RuntimeError):  # delta without x_new
        _core.add_rms_fwd(x.data_ptr(), d.data_ptr(), w.data_ptr(), 0,
                          y.data_ptr(), rstd.data_ptr(), 4, 512, EPS, s)
    # R == 0 launches nothing and raises nothing
    _core.add_rms_fwd(x.data_ptr(), d.data_ptr(), w.data_ptr(),
                      xn.data_ptr(), y.data_ptr(), rstd.data_ptr(), 0, 512,
                      EPS, s)
    torch.cuda.synchronize()


def test_empty_input():
    x = torch.empty(0, 512, device="cuda", dtype=torch.bfloat16,
                    requires_grad=True)
    d = torch.empty_like(x, requires_grad=True)
    w = torch.ones(512, device="cuda", dtype=torch.bfloat16,
                   requires_grad=True)
    x_new, y = fused_rms.fused_add_rms_norm(x, d, w, EPS)
    (x_new.float().sum() + y.float().sum()).backward()
    assert x_new.shape == y.shape == (0, 512)
    assert torch.equal(w.grad, torch.zeros_like(w))


def test_only_residual_stream_used():
    """y unused: the gradient of x and delta is d_x_new itself."""
    t = make_inputs(37, 2048, seed=3)
    x = t["x"].clone().requires_grad_(True)
    delta = t["delta"].clone().requires_grad_(True)
    w = t["w"].clone().requires_grad_(True)
    x_new, _ = fused_rms.fused_add_rms_norm(x, delta, w, EPS)
    x_new.backward(t["dres"])
    torch.cuda.synchronize()
    assert torch.equal(x.grad, t["dres"]) and torch.equal(delta.grad, t["dres"])
    assert w.grad is None


def test_only_y_used():
    """The final norm: nothing comes down the residual stream."""
    t = make_inputs(37, 2048, seed=4)
    got = run_fused(t, True, False)
    ref = reference(t, t["x"] + t["delta"], False)
    torch.testing.assert_close(got["dx"], ref["dx"], rtol=5e-2, atol=5e-2)
    torch.testing.assert_close(got["dgamma"], ref["dgamma"], rtol=3e-2,
                               atol=3e-1)


@pytest.mark.parametrize("R,C", [(RAGGED, 2048), (RAGGED, 512), (1000, 4096)])
def test_backward_repeats_bit_for_bit(R, C):
    t = make_inputs(R, C, seed=11)
    a = run_fused(t, True, True)
    b = run_fused(t, True, True)
    for name in ("dx", "dgamma"):
        assert torch.equal(a[name], b[name]), name


def _offset_view(src, off=4):
    """A contiguous copy of `src` whose storage starts `off` elements (8
    bytes) into an allocation: not 16-byte aligned."""
    buf = torch.empty(src.numel() + 8, dtype=src.dtype, device=src.device)
    v = buf[off:off + src.numel()].view(src.shape)
    v.copy_(src)
    assert v.data_ptr() % 16 != 0 and v.is_contiguous()
    return v


def test_misaligned_views_give_the_same_values():
    t = make_inputs(33, 2048, seed=5)

    def run(x, delta, dy, dres):
        x = x.detach().requires_grad_(True)
        delta = delta.detach().requires_grad_(True)
        w = t["w"].clone().requires_grad_(True)
        x_new, y = fused_rms.fused_add_rms_norm(x, delta, w, EPS)
        torch.autograd.backward([y, x_new], [dy, dres])
        torch.cuda.synchronize()
        return (x_new.detach(), y.detach(), x.grad, delta.grad, w.grad)

    base = run(t["x"], t["delta"], t["dy"], t["dres"])
    # misaligned incoming gradients: backward clones them, same kernel
    got = run(t["x"], t["delta"], _offset_view(t["dy"]),
              _offset_view(t["dres"]))
    for a, b in zip(base, got):
        assert torch.equal(a, b)
    # misaligned inputs: add, then the block-per-row kernels
    got = run(_offset_view(t["x"]), _offset_view(t["delta"]), t["dy"],
              t["dres"])
    assert torch.equal(got[0], base[0])
    assert torch.equal(got[2], got[3])
    for a, b, (rtol, atol) in zip(base[1:], got[1:],
                                  [(2e-2, 2e-2), (5e-2, 5e-2), (5e-2, 5e-2),
                                   (3e-2, 3e-1)]):
        torch.testing.assert_close(a.float(), b.float(), rtol=rtol, atol=atol)


def _tiny_llama(dim=512, n_layer=2, vocab=256, ffn=1024):
    from sharedtensor_amd.models.llama import Llama, LlamaConfig
    cfg = LlamaConfig(vocab_size=vocab, n_layer=n_layer, n_head=4,
                      n_kv_head=2, dim=dim, ffn_dim=ffn, block_size=64)
    return Llama(cfg).cuda().to(torch.bfloat16), cfg


def test_knob_routes_block_away_from_fused_op(monkeypatch):
    calls = []
    real = fused_rms.fused_add_rms_norm

    def counting(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(fused_rms, "fused_add_rms_norm", counting)
    torch.manual_seed(2)
    model, cfg = _tiny_llama()
    blk = model.blocks[0]
    x = torch.randn(2, 16, cfg.dim, device="cuda").to(torch.bfloat16)
    d = torch.randn(2, 16, cfg.dim, device="cuda").to(torch.bfloat16)
    cos, sin = model._rope_cache(x.device, x.dtype)
    monkeypatch.delenv("SHTENS_NO_FUSED_ADD_RMS", raising=False)
    fx, fm = blk(x, cos, sin, d)
    assert len(calls) == 2  # both adds of the block ride in their norms
    monkeypatch.setenv("SHTENS_NO_FUSED_ADD_RMS", "1")
    ux, um = blk(x, cos, sin, d)
    assert len(calls) == 2  # add-then-norm: the fused op is not called
    torch.cuda.synchronize()
    assert torch.equal(fx, ux)  # x_new is bit for bit torch's sum
    torch.testing.assert_close(fm.float(), um.float(), rtol=5e-2, atol=5e-2)


def _train_losses(monkeypatch, knob):
    losses = {}
    for tag in ("fused", "knob"):
        with monkeypatch.context() as mp:
            mp.delenv("SHTENS_NO_FUSED_ADD_RMS", raising=False)
            mp.delenv("SHTENS_NO_FUSED_CE_LLAMA", raising=False)
            if tag == "knob":
                mp.setenv(knob, "1")
            torch.manual_seed(7)
            m, cfg = _tiny_llama()
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
    print(knob, losses)
    return losses


@pytest.mark.parametrize("knob", ["SHTENS_NO_FUSED_ADD_RMS",
                                  "SHTENS_NO_FUSED_CE_LLAMA"])
def test_training_equivalence(monkeypatch, knob):
    """8 SGD steps on a 2-layer, 512-wide Llama: the default path tracks the
    one the knob restores."""
    losses = _train_losses(monkeypatch, knob)
    assert all(math.isfinite(v) for v in losses["fused"])
    for a, b in zip(losses["fused"], losses["knob"]):
        assert abs(a - b) < 0.15, losses


def test_llama_loss_goes_through_fused_ce(monkeypatch):
    """R=6 rows of the Llama-3 vocabulary through the model's own loss path:
    the fused CE is called, and loss and dlogits match
    F.cross_entropy(logits.float())."""
    V = 128256
    assert V <= _core.ce_fwd_grad_max_v()
    calls = []
    real = fused_ce.fused_cross_entropy

    def counting(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(fused_ce, "fused_cross_entropy", counting)
    monkeypatch.delenv("SHTENS_NO_FUSED_CE_LLAMA", raising=False)
    torch.manual_seed(9)
    model, cfg = _tiny_llama(dim=64, n_layer=1, vocab=V, ffn=128)
    with torch.no_grad():  # spread the logits so softmax is not flat
        model.lm_head.weight.normal_(std=0.5)
    tok = torch.randint(0, V, (2, 4), device="cuda")
    idx, tgt = tok[:, :-1], tok[:, 1:]
    logits, loss = model(idx, tgt)
    assert logits.shape == (2, 3, V) and len(calls) == 1
    logits.retain_grad()
    loss.backward()
    torch.cuda.synchronize()

    lt = logits.detach().float().requires_grad_(True)
    loss_t = F.cross_entropy(lt.view(-1, V), tgt.reshape(-1))
    loss_t.backward()
    torch.testing.assert_close(loss.float(), loss_t, rtol=2e-3, atol=2e-3)
    torch.testing.assert_close(logits.grad.float(), lt.grad, rtol=5e-2,
                               atol=1e-4)

    # the knob restores the logits.float() path
    monkeypatch.setenv("SHTENS_NO_FUSED_CE_LLAMA", "1")
    _, loss_k = model(idx, tgt)
    assert len(calls) == 1
    torch.testing.assert_close(loss_k.float(), loss_t, rtol=1e-6, atol=1e-6)
