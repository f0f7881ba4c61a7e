"""Fused residual-add + LayerNorm (csrc/add_ln_kernels.hip) against an fp32
torch reference and against the unfused sequence it replaces."""
import math

import pytest
import torch
import torch.nn.functional as F

from sharedtensor_amd import _core
from sharedtensor_amd.ops import fused_ln

pytestmark = pytest.mark.gpu

EPS = 1e-5
# 768 and 512 run the wave-per-row kernels, 64 and 4096 the fallback.  8195
# rows exceed what the backward grid covers in one sweep (at most 1024
# blocks of 4 rows), so its row loop iterates with a ragged tail.
WIDTHS = [768, 512, 64, 4096]
ROWS = [1, 5, 1000, 8195]


def bf16_ulp(mag: float) -> float:
    """Spacing of bf16 (8 significant bits) at magnitude `mag`."""
    return 2.0 ** (math.floor(math.log2(max(mag, 1e-30))) - 7)


def make_inputs(R, C, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)

    def rn(*shape, scale=1.0):
        return (torch.randn(*shape, device="cuda", generator=g)
                * scale).to(torch.bfloat16)
    return {"x": rn(R, C, scale=2.0), "delta": rn(R, C), "w": rn(C),
            "b": rn(C), "dbias": rn(C), "dy": rn(R, C), "dres": rn(R, C)}


def expected_x_new(t, has_delta, has_dbias):
    if not has_delta:
        return t["x"]
    if has_dbias:
        return (t["x"].float() + t["delta"].float()
                + t["dbias"].float()).bfloat16()
    return t["x"] + t["delta"]


def reference(t, x_new, has_bias, has_dres):
    """fp32 autograd through F.layer_norm on the bf16 x_new."""
    C = x_new.shape[-1]
    xn = x_new.float().requires_grad_(True)
    w = t["w"].float().requires_grad_(True)
    b = t["b"].float().requires_grad_(True) if has_bias else None
    y = F.layer_norm(xn, (C,), w, b, EPS)
    loss = (y * t["dy"].float()).sum()
    if has_dres:
        loss = loss + (xn * t["dres"].float()).sum()
    loss.backward()
    return {"y": y.detach(), "dx": xn.grad, "dgamma": w.grad,
            "dbeta": b.grad if has_bias else None, "ddbias": xn.grad.sum(0)}


def run_fused(t, has_delta, has_dres, has_bias, has_dbias):
    x = t["x"].clone().requires_grad_(True)
    delta = t["delta"].clone().requires_grad_(True) if has_delta else None
    w = t["w"].clone().requires_grad_(True)
    b = t["b"].clone().requires_grad_(True) if has_bias else None
    db = t["dbias"].clone().requires_grad_(True) if has_dbias else None
    x_new, y = fused_ln.fused_add_layer_norm(x, delta, w, b, EPS, db)
    loss = (y.float() * t["dy"].float()).sum()
    if has_dres:
        loss = loss + (x_new.float() * t["dres"].float()).sum()
    loss.backward()
    torch.cuda.synchronize()
    if has_delta:  # one tensor serves both inputs
        assert torch.equal(x.grad, delta.grad)
    return {"x_new": x_new.detach(), "y": y.detach().float(),
            "dx": x.grad.float(), "dgamma": w.grad.float(),
            "dbeta": b.grad.float() if has_bias else None,
            "ddbias": db.grad.float() if has_dbias else None}


def run_unfused(t, x_new, has_bias, has_dres):
    """What the fused op replaces: the block-per-row LN kernels on x_new,
    then autograd's bf16 add of the residual-path gradient."""
    R, C = x_new.shape
    s = torch.cuda.current_stream().cuda_stream
    y = torch.empty_like(x_new)
    mean = torch.empty(R, dtype=torch.float32, device="cuda")
    rstd = torch.empty(R, dtype=torch.float32, device="cuda")
    _core.ln_fwd(x_new.data_ptr(), t["w"].data_ptr(),
                 t["b"].data_ptr() if has_bias else 0, y.data_ptr(),
                 mean.data_ptr(), rstd.data_ptr(), R, C, EPS, s)
    dx = torch.empty_like(x_new)
    dwdb = torch.zeros(2, C, dtype=torch.float32, device="cuda")
    _core.ln_bwd(t["dy"].data_ptr(), x_new.data_ptr(), t["w"].data_ptr(),
                 mean.data_ptr(), rstd.data_ptr(), dx.data_ptr(),
                 dwdb[0].data_ptr(), dwdb[1].data_ptr(), R, C, s)
    if has_dres:
        dx = dx + t["dres"]
    torch.cuda.synchronize()
    return {"y": y.float(), "dx": dx.float(),
            "dgamma": dwdb[0].bfloat16().float(),
            "dbeta": dwdb[1].bfloat16().float() if has_bias else None,
            "ddbias": dx.float().sum(0).bfloat16().float()}


def check(R, C, has_delta, has_dres, has_bias, has_dbias):
    t = make_inputs(R, C, seed=R * 131 + C)
    got = run_fused(t, has_delta, has_dres, has_bias, has_dbias)
    want_x_new = expected_x_new(t, has_delta, has_dbias)
    # one fp32 add, one round-to-nearest-even: bit for bit torch's sum
    assert torch.equal(got["x_new"], want_x_new)
    ref = reference(t, want_x_new, has_bias, has_dres)
    old = run_unfused(t, want_x_new, has_bias, has_dres)

    tol = {"y": (2e-2, 2e-2), "dx": (5e-2, 5e-2), "dgamma": (3e-2, 3e-1),
           "dbeta": (3e-2, 3e-1), "ddbias": (3e-2, 3e-1)}
    for name, (rtol, atol) in tol.items():
        if got[name] is None:
            continue
        torch.testing.assert_close(got[name], ref[name], rtol=rtol, atol=atol,
                                   msg=lambda m, n=name: f"{n}: {m}")
        err_new = (got[name] - ref[name]).abs().max().item()
        err_old = (old[name] - ref[name]).abs().max().item()
        ulp = bf16_ulp(ref[name].abs().max().item())
        print(f"R={R} C={C} {name}: fused err {err_new:.4g}, "
              f"unfused err {err_old:.4g}, ulp {ulp:.4g}")
        # the fused backward rounds once where the old path rounds twice
        assert err_new <= err_old + ulp, (name, err_new, err_old, ulp)


@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("R", ROWS)
def test_shapes(R, C):
    check(R, C, has_delta=True, has_dres=True, has_bias=True,
          has_dbias=False)


VARIANTS = [(d, r, b, db) for d in (True, False) for r in (True, False)
            for b in (True, False) for db in (True, False) if d or not db]


# 256 and 1024: the narrowest and the widest wave-per-row instantiation
@pytest.mark.parametrize("R,C", [(1000, 768), (8195, 512), (5, 64), (5, 256),
                                 (5, 1024)])
@pytest.mark.parametrize("has_delta,has_dres,has_bias,has_dbias", VARIANTS)
def test_variants(R, C, has_delta, has_dres, has_bias, has_dbias):
    check(R, C, has_delta, has_dres, has_bias, has_dbias)


def test_only_residual_stream_used():
    """y unused: the gradient of x and delta is d_x_new itself."""
    t = make_inputs(37, 768, seed=3)
    x = t["x"].clone().requires_grad_(True)
    delta = t["delta"].clone().requires_grad_(True)
    w = t["w"].clone().requires_grad_(True)
    db = t["dbias"].clone().requires_grad_(True)
    x_new, _ = fused_ln.fused_add_layer_norm(x, delta, w, t["b"], EPS, db)
    x_new.backward(t["dres"])
    torch.cuda.synchronize()
    assert torch.equal(x.grad, t["dres"]) and torch.equal(delta.grad, t["dres"])
    assert w.grad is None
    torch.testing.assert_close(db.grad.float(), t["dres"].float().sum(0),
                               rtol=3e-2, atol=3e-1)


@pytest.mark.parametrize("R,C", [(8195, 768), (1000, 512)])
def test_backward_repeats_bit_for_bit(R, C):
    t = make_inputs(R, C, seed=11)
    a = run_fused(t, True, True, True, True)
    b = run_fused(t, True, True, True, True)
    for name in ("dx", "dgamma", "dbeta", "ddbias"):
        assert torch.equal(a[name], b[name]), name


@pytest.mark.parametrize("fuse_proj_bias", [False, True])
def test_training_equivalence_width_768(monkeypatch, fuse_proj_bias):
    """8 SGD steps on a 2-layer, 768-wide GPT-2: the fused add+LN path
    tracks the plain torch path (`can_use` forced false)."""
    import sharedtensor_amd.models.gpt2 as gpt2
    monkeypatch.setattr(gpt2, "FUSE_PROJ_BIAS", fuse_proj_bias)
    losses = {}
    for tag in ("fused", "torch"):
        with monkeypatch.context() as mp:
            if tag == "torch":
                mp.setattr(fused_ln, "can_use", lambda *a: False)
            torch.manual_seed(7)
            cfg = gpt2.GPT2Config.tiny()
            cfg.n_embd, cfg.n_layer, cfg.n_head = 768, 2, 12
            m = gpt2.GPT2(cfg).cuda().to(torch.bfloat16)
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
        assert abs(a - b) < 0.15, losses
