"""The attention backward writing the packed (B, T, 3C) dqkv and summing its
columns for qkv.bias.grad in the store epilogue (csrc/attn_bwd_kernels.hip,
attn_bwd_tile.h), and the route through models/gpt2.py.

* dqkv and delta are bit-equal to dq, dk, dv and delta of the existing
  ``attn_backward`` into separate buffers: the arithmetic is the same, only
  addresses move.  Guards around every buffer stay untouched.
* db is held to the bound derived in colsum_bounds.py against the fp64 column
  sum of the bf16 dqkv the kernel wrote; one MAXERR line per shape (a record,
  profiles/r14/qkv_attn_bwd_maxerr.txt, not a threshold).
* the partials scratch is filled with NaN before each call; repeats are
  bit-equal.
"""
import functools

import pytest
import torch

from colsum_bounds import ATTN_EPILOGUE_ADDS, colsum_check, reduce_adds
from test_gpu_fused_attn import (CANARY_BF16, CANARY_F32, GUARD, SCALE, _fa,
                                 _guarded, _layout, _make_qkv)

pytestmark = pytest.mark.gpu

# both sides of the wave (32), tile (64) and workgroup (128) boundaries; a
# packed row stride (3 * 192) that differs from the head stride; B * H below
# (6, 9) and above (12) the 8 XCDs of grid_map
SHAPES = [(2, 3, 1), (2, 3, 17), (2, 3, 64), (2, 3, 96), (2, 3, 128),
          (2, 3, 129), (3, 3, 200), (1, 12, 257)]


def _core():
    from sharedtensor_amd import _core
    return _core


def _guards_ok(buf):
    canary = CANARY_BF16 if buf.dtype == torch.bfloat16 else CANARY_F32
    g = torch.full((GUARD,), canary, dtype=buf.dtype, device="cuda")
    return torch.equal(buf[:GUARD], g) and torch.equal(buf[-GUARD:], g)


@functools.lru_cache(maxsize=None)
def _case(B, H, T):
    fa = _fa()
    seed = 3000 * T + H
    q, k, v = _layout(*_make_qkv(B, H, T, "gauss", seed), "packed")
    g = torch.Generator(device="cuda").manual_seed(seed + 1)
    dout = torch.randn(B, T, H, 64, device="cuda",
                       generator=g).bfloat16().transpose(1, 2)
    out, lse = fa.attn_forward(q, k, v, SCALE)
    out = out.transpose(1, 2)
    C = H * 64

    sep_delta = torch.empty(B, H, T, dtype=torch.float32, device="cuda")
    sep = fa.attn_backward(q, k, v, out, lse, dout, SCALE, delta=sep_delta)

    nfl = _core().attn_bwd_colsum_floats(B, H, T)

    def run():
        gbuf, dqkv = _guarded((B, T, 3 * C), torch.bfloat16, CANARY_BF16)
        dbuf, delta = _guarded((B, H, T), torch.float32, CANARY_F32)
        bbuf, db = _guarded((3 * C,), torch.bfloat16, CANARY_BF16)
        pbuf, part = _guarded((nfl,), torch.float32, CANARY_F32)
        part.fill_(float("nan"))  # nothing stale may be read
        views = fa._heads(dqkv, H)
        fa.attn_backward(q, k, v, out, lse, dout, SCALE, *views, delta=delta,
                         partial=part, db=db)
        torch.cuda.synchronize()
        return dqkv, delta, db, (gbuf, dbuf, bbuf, pbuf)

    dqkv, delta, db, bufs = run()
    dqkv2, delta2, db2, _ = run()
    return dict(sep=sep, sep_delta=sep_delta, dqkv=dqkv, delta=delta, db=db,
                dqkv2=dqkv2, delta2=delta2, db2=db2, bufs=bufs)


def _db_worst(B, H, T, c):
    G = B * (-(-T // 128))
    return colsum_check(c["db"], c["dqkv"].reshape(B * T, -1),
                        ATTN_EPILOGUE_ADDS + reduce_adds(G),
                        f"db B={B} H={H} T={T}")


@pytest.mark.parametrize("B,H,T", SHAPES)
def test_packed_backward(B, H, T):
    c = _case(B, H, T)
    C = H * 64
    for buf in c["bufs"]:
        assert _guards_ok(buf)
    # gradient: bit-equal to the separate-buffer call
    for i, name in enumerate(("dq", "dk", "dv")):
        want = c["sep"][i].transpose(1, 2).reshape(B, T, C)
        got = c["dqkv"][:, :, i * C:(i + 1) * C]
        assert torch.equal(got, want), f"{name} differs from attn_backward"
    assert torch.equal(c["delta"], c["sep_delta"])
    # bias gradient: derived bound, NaN-filled scratch
    worst = _db_worst(B, H, T, c)
    print(f"MAXERR op=qkv_attn_bwd out=db B={B} H={H} T={T} "
          f"{worst:.4g} of-bound")
    # repeats
    assert torch.equal(c["dqkv"], c["dqkv2"])
    assert torch.equal(c["delta"], c["delta2"])
    assert torch.equal(c["db"], c["db2"])


def test_partial_and_db_go_together():
    fa = _fa()
    q, k, v = _layout(*_make_qkv(1, 3, 8, "gauss", 5), "packed")
    out, lse = fa.attn_forward(q, k, v, SCALE)
    out = out.transpose(1, 2)
    db = torch.empty(3 * 192, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(ValueError):
        fa.attn_backward(q, k, v, out, lse, out, SCALE, db=db)
    small = torch.empty(8, dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError):
        fa.attn_backward(q, k, v, out, lse, out, SCALE, partial=small, db=db)


def _module(n_embd, n_head):
    from sharedtensor_amd.models import gpt2
    cfg = gpt2.GPT2Config(vocab_size=64, n_layer=1, n_head=n_head,
                          n_embd=n_embd, block_size=256)
    torch.manual_seed(3)
    mod = gpt2.CausalSelfAttention(cfg).cuda()
    torch.nn.init.normal_(mod.qkv.bias, std=0.1)
    return mod.bfloat16()


def _run_module(monkeypatch, mod, x, dy, flag):
    """Forward + backward with SHTENS_FUSED_QKV_ATTN = flag; returns the
    output, the gradients, the packed gradient the qkv Linear received and
    how often the packed node ran."""
    from sharedtensor_amd.models import gpt2
    from sharedtensor_amd.ops import fused_attn
    monkeypatch.setenv("SHTENS_FUSED_QKV_ATTN", flag)
    for name in ("SHTENS_FUSED_ATTN", "SHTENS_FUSED_ATTN_BWD",
                 "SHTENS_FUSED_QKV_BGRAD"):
        monkeypatch.delenv(name, raising=False)
    calls, dqkv = [], []
    real_node = fused_attn.fused_qkv_causal_attention
    monkeypatch.setattr(fused_attn, "fused_qkv_causal_attention",
                        lambda *a, **k: (calls.append(1), real_node(*a, **k))[1])
    real_linear = gpt2._linear

    def linear(inp, weight, bias=None):
        y = real_linear(inp, weight, bias)
        if weight is mod.qkv.weight:
            y.register_hook(lambda g: dqkv.append(g.detach().clone()))
        return y

    monkeypatch.setattr(gpt2, "_linear", linear)
    mod.zero_grad(set_to_none=True)
    xx = x.clone().requires_grad_(True)
    y = mod(xx)
    y.backward(dy)
    torch.cuda.synchronize()
    monkeypatch.setattr(gpt2, "_linear", real_linear)
    monkeypatch.setattr(fused_attn, "fused_qkv_causal_attention", real_node)
    grads = {n: p.grad.clone() for n, p in mod.named_parameters()}
    return y.detach(), xx.grad, grads, dqkv[0], len(calls)


def test_module_gradients_flag_on_and_off(monkeypatch):
    B, T, H = 2, 96, 3
    mod = _module(64 * H, H)
    x = torch.randn(B, T, 64 * H, device="cuda").bfloat16()
    dy = torch.randn(B, T, 64 * H, device="cuda").bfloat16()
    y0, dx0, g0, dqkv0, n0 = _run_module(monkeypatch, mod, x, dy, "0")
    y1, dx1, g1, dqkv1, n1 = _run_module(monkeypatch, mod, x, dy, "1")
    assert (n0, n1) == (0, 1)
    assert torch.equal(y0, y1) and torch.equal(dx0, dx1)
    assert torch.equal(dqkv0, dqkv1)
    for name in ("qkv.weight", "proj.weight", "proj.bias"):
        assert torch.equal(g0[name], g1[name]), name
    G = B * (-(-T // 128))
    worst = colsum_check(g1["qkv.bias"], dqkv1.reshape(B * T, -1),
                         ATTN_EPILOGUE_ADDS + reduce_adds(G),
                         "module qkv.bias.grad")
    print(f"MAXERR op=qkv_attn_bwd out=module_db B={B} H={H} T={T} "
          f"{worst:.4g} of-bound")


def test_fallback_outside_can_use(monkeypatch):
    """Head dim 32: the kernels do not take it, the flag changes nothing."""
    B, T, H = 2, 40, 3
    mod = _module(32 * H, H)
    x = torch.randn(B, T, 32 * H, device="cuda").bfloat16()
    dy = torch.randn(B, T, 32 * H, device="cuda").bfloat16()
    y0, dx0, g0, dqkv0, n0 = _run_module(monkeypatch, mod, x, dy, "0")
    y1, dx1, g1, dqkv1, n1 = _run_module(monkeypatch, mod, x, dy, "1")
    assert (n0, n1) == (0, 0)
    assert torch.equal(y0, y1) and torch.equal(dx0, dx1)
    assert torch.equal(dqkv0, dqkv1)
    for name in g0:
        assert torch.equal(g0[name], g1[name]), name
