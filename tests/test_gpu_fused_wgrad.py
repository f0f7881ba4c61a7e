"""The split-K bf16 weight-gradient kernel (csrc/wgrad_kernels.hip) through
its raw binding, and ops/fused_wgrad.py at module level.

Reference: the fp64 product of the bf16 inputs.  Rule, as in
test_gpu_fused_attn.py: the kernel's max-abs and relative-L2 error against
fp64 may be at most 1.5x the error of ``torch.mm`` on the same inputs; a
floor takes over only where the library's error is (nearly) zero.  The floor
comes from the operation count alone, per element

    floor[n, k] = 2^-8 |ref[n, k]| + (M + 64) 2^-24 (|dY|^T |X|)[n, k]

(one bf16 rounding of the result, and M fp32 accumulations plus the split
sums of products that are exact in fp32), taken as its maximum for max-abs
and as ||floor||_2 / ||ref||_2 for the relative L2.

dW and the workspace sit inside sentinel-filled guard buffers; the workspace
is filled with NaN first, so a partial that is read before it is written
shows in the result.  Every case runs the kernel twice and wants equal bits.

Shapes are the smallest at which each mechanism can fail: one tile and one
step; uneven (2/2/1) and empty split ranges at 5 steps; N != K with unrelated
operands, where a transposed output or swapped operands cannot pass; the
workload's feature sizes and split at a short token count; a strided dY.
test_maxerr_report prints one MAXERR line per family (kept in profiles/r09/
as a record, not as a threshold).
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

MARGIN = 1.5
GUARD = 256


def _fw():
    from sharedtensor_amd.ops import fused_wgrad
    return fused_wgrad


def _inputs(M, N, K, family, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    if family == "selector":
        assert M <= N
        cols = torch.randperm(N, generator=g, device="cuda")[:M]
        dy = torch.zeros(M, N, device="cuda")
        dy[torch.arange(M, device="cuda"), cols] = 1.0
        x = torch.randn(M, K, generator=g, device="cuda")
        return dy.bfloat16(), x.bfloat16(), cols
    dy = torch.randn(M, N, generator=g, device="cuda")
    x = torch.randn(M, K, generator=g, device="cuda")
    if family == "cancel":
        # large values whose sign alternates along M: the sum cancels
        sign = 1.0 - 2.0 * (torch.arange(M, device="cuda") % 2).float()
        dy = (100.0 + dy) * sign[:, None]
        x = 50.0 + x
    return dy.bfloat16(), x.bfloat16(), None


@functools.lru_cache(maxsize=None)
def _case(M, N, K, family, seed=0):
    dy, x, cols = _inputs(M, N, K, family, seed)
    d64, x64 = dy.double(), x.double()
    ref = d64.t() @ x64
    mag = d64.abs().t() @ x64.abs()
    floor = 2.0 ** -8 * ref.abs() + (M + 64) * 2.0 ** -24 * mag
    lib = dy.t().mm(x)
    return dict(dy=dy, x=x, cols=cols, ref=ref, lib=lib,
                floor_abs=floor.max().item(),
                floor_l2=(floor.norm() / ref.norm().clamp_min(1e-300)).item())


def _errs(a, ref):
    d = a.double() - ref
    return d.abs().max().item(), (d.norm() / ref.norm().clamp_min(1e-300)).item()


def _guarded(n, dtype, canary):
    buf = torch.full((n + 2 * GUARD,), canary, dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, canary):
    ref = torch.full((GUARD,), canary, dtype=buf.dtype, device="cuda")
    return torch.equal(buf[:GUARD], ref) and torch.equal(buf[-GUARD:], ref)


def _run(dy, x, split, variant, ldw=None):
    """The kernel twice, inside guards, with a NaN-filled workspace; returns
    dW (N, K) after checking guards and bit-equality."""
    fw = _fw()
    N, K = dy.shape[1], x.shape[1]
    ldw = K if ldw is None else ldw
    tn, tk, per_cu = fw.VARIANTS[variant]
    if split is None:
        split = fw.choose_split((N // tn) * (K // tk), dy.shape[0] // fw.STEP,
                                per_cu)
    outs = []
    for _ in range(2):
        obuf, o = _guarded(N * ldw, torch.bfloat16, -7.0)
        out = o.view(N, ldw)[:, :K]
        wbuf, ws = _guarded(max(split * N * K, 8), torch.float32, 12345.0)
        ws.fill_(float("nan"))
        fw.wgrad(dy, x, out=out, split=split, variant=variant, ws=ws)
        torch.cuda.synchronize()
        assert _guards_intact(obuf, -7.0), "dW guard overwritten"
        assert _guards_intact(wbuf, 12345.0), "workspace guard overwritten"
        if ldw > K:  # the padding between rows belongs to the caller
            pad = o.view(N, ldw)[:, K:]
            assert torch.equal(pad, torch.full_like(pad, -7.0))
        outs.append(out.clone())
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), \
        "two calls on the same inputs differ"
    return outs[0]


def _check(c, got, tag):
    f_abs, f_l2 = _errs(got, c["ref"])
    a_abs, a_l2 = _errs(c["lib"], c["ref"])
    print(f"WGRAD {tag}: maxabs fused {f_abs:.3e} mm {a_abs:.3e} floor "
          f"{c['floor_abs']:.3e} | rel-l2 fused {f_l2:.3e} mm {a_l2:.3e} "
          f"floor {c['floor_l2']:.3e}")
    assert f_abs <= max(MARGIN * a_abs, c["floor_abs"])
    assert f_l2 <= max(MARGIN * a_l2, c["floor_l2"])
    return f_abs, f_l2, a_abs, a_l2


# (M, N, K, split); None is the split the op would choose
SMALL = [
    (64, 256, 256, 1),      # one tile, one step, direct bf16 store
    (320, 256, 256, 3),     # 5 steps as 2/2/1
    (320, 256, 256, 8),     # 5 steps over 8 splits: three empty ones
    (128, 512, 256, None),  # N != K, unrelated operands
    (128, 256, 768, None),
]
REAL = [
    (4096, 768, 768, None),   # attn.proj: the workload's split
    (4096, 2304, 768, None),  # attn.qkv
]


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("family", ["randn", "cancel"])
@pytest.mark.parametrize("M,N,K,split", SMALL)
def test_small_shapes_against_fp64(M, N, K, split, family, variant):
    c = _case(M, N, K, family)
    got = _run(c["dy"], c["x"], split, variant)
    _check(c, got, f"{family} M{M} N{N} K{K} split {split} v{variant}")


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("family", ["randn", "cancel"])
@pytest.mark.parametrize("M,N,K,split", REAL)
def test_real_feature_sizes_against_fp64(M, N, K, split, family, variant):
    c = _case(M, N, K, family)
    got = _run(c["dy"], c["x"], split, variant)
    _check(c, got, f"{family} M{M} N{N} K{K} split {split} v{variant}")


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("M,N,K,split", [(64, 256, 256, 1),
                                         (256, 256, 384, 3),
                                         (320, 512, 256, 8)])
def test_selector_copies_rows_bit_for_bit(M, N, K, split, variant):
    """dY has a single 1 per row, in distinct columns: dW's row cols[m] is
    row m of X exactly, every other row is zero."""
    c = _case(M, N, K, "selector")
    got = _run(c["dy"], c["x"], split, variant)
    want = torch.zeros(N, K, dtype=torch.bfloat16, device="cuda")
    want[c["cols"]] = c["x"]
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("variant", [0, 2])
def test_strided_operands_and_output(variant):
    """dY as a column slice of a wider buffer (the q part of a packed
    gradient), X with padded rows, dW with padded rows."""
    fw = _fw()
    M, N, K = 192, 256, 256
    c = _case(M, N, K, "randn", 5)
    wide = torch.randn(M, 3 * N, device="cuda").bfloat16()
    wide[:, N:2 * N] = c["dy"]
    dy = wide[:, N:2 * N]
    xw = torch.randn(M, K + 64, device="cuda").bfloat16()
    xw[:, :K] = c["x"]
    x = xw[:, :K]
    assert fw.can_use(dy, x, variant) and not dy.is_contiguous()
    got = _run(dy, x, 2, variant, ldw=K + 8)
    _check(c, got, f"strided v{variant}")
    dense = _run(c["dy"], c["x"], 2, variant)
    assert torch.equal(got.view(torch.int16), dense.view(torch.int16))


def test_maxerr_report():
    for family in ["randn", "cancel"]:
        worst = [0.0, 0.0, 0.0, 0.0]
        for M, N, K, split in SMALL + REAL:
            c = _case(M, N, K, family)
            got = _run(c["dy"], c["x"], split, 0)
            f = _errs(got, c["ref"]) + _errs(c["lib"], c["ref"])
            worst = [max(a, b) for a, b in zip(worst, f)]
        print(f"MAXERR wgrad {family}: maxabs fused {worst[0]:.3e} mm "
              f"{worst[2]:.3e} | rel-l2 fused {worst[1]:.3e} mm {worst[3]:.3e}")


def test_module_gradients_flag_on_and_off(monkeypatch):
    """A 2-layer GPT-2 (two heads of 64) at B=2, T=128 with the flag on and
    off on one batch; every parameter gradient against an fp32 run."""
    import copy
    from sharedtensor_amd.models import gpt2
    fw = _fw()
    for env in ("SHTENS_FUSED_WGRAD", "SHTENS_FUSED_QKV_BGRAD",
                "SHTENS_FUSED_GELU_BGRAD", "SHTENS_FUSED_ATTN"):
        monkeypatch.delenv(env, raising=False)
    cfg = gpt2.GPT2Config(vocab_size=512, n_layer=2, n_head=2, n_embd=128,
                          block_size=128)
    shapes = {(384, 128): 0, (128, 128): 1, (512, 128): 2, (128, 512): 0}
    monkeypatch.setattr(fw, "TUNED", shapes)
    torch.manual_seed(11)
    master = gpt2.GPT2(cfg).cuda()
    for n, p in master.named_parameters():
        if n.endswith("bias"):
            torch.nn.init.normal_(p, std=0.05)
    idx = torch.randint(0, cfg.vocab_size, (2, 128), device="cuda")
    tgt = torch.randint(0, cfg.vocab_size, (2, 128), device="cuda")

    calls = []
    real = fw.wgrad
    monkeypatch.setattr(fw, "wgrad",
                        lambda *a, **k: (calls.append(1), real(*a, **k))[1])

    def run(model, flag):
        monkeypatch.setattr(gpt2, "FUSE_WGRAD", flag)
        model.zero_grad(set_to_none=True)
        _, loss = model(idx, tgt)
        loss.backward()
        return {n: p.grad.clone() for n, p in model.named_parameters()}

    ref = run(copy.deepcopy(master), True)          # fp32: never wired
    assert not calls, "fp32 parameters must keep the library path"
    low = copy.deepcopy(master).bfloat16()
    on = run(low, True)
    assert len(calls) == 4 * cfg.n_layer, calls
    off = run(low, False)
    assert len(calls) == 4 * cfg.n_layer, "flag off: the kernel ran"
    for name, r in ref.items():
        f_abs, f_l2 = _errs(on[name], r.double())
        a_abs, a_l2 = _errs(off[name], r.double())
        print(f"WGRAD module {name}: maxabs fused {f_abs:.3e} current "
              f"{a_abs:.3e} | rel-l2 fused {f_l2:.3e} current {a_l2:.3e}")
        assert f_abs <= MARGIN * a_abs
        assert f_l2 <= MARGIN * a_l2


def test_can_use_rejections_on_device():
    fw = _fw()
    mk = lambda *s, dt=torch.bfloat16: torch.zeros(*s, device="cuda", dtype=dt)
    dy, x = mk(128, 256), mk(128, 384)
    assert fw.can_use(dy, x)
    assert not fw.can_use(mk(128, 256, dt=torch.float32), x)
    assert not fw.can_use(dy, mk(128, 384, dt=torch.float16))
    assert not fw.can_use(mk(100, 256), mk(100, 384))       # M % 64
    assert not fw.can_use(mk(128, 192), x)                  # N % 128
    assert not fw.can_use(dy, mk(128, 320))                 # K % 128
    assert fw.can_use(dy, x, 0) and not fw.can_use(mk(128, 384), x, 2)
    assert not fw.can_use(dy, mk(64, 384))                  # M differs
    assert not fw.can_use(mk(128, 260)[:, 4:260], x)        # base off by 8 B
    assert not fw.can_use(mk(256, 128).t(), mk(128, 384))   # column-major
    assert not fw.can_use(dy.cpu(), x.cpu())
    assert not fw.can_use(dy, x, 7)
    with pytest.raises(ValueError):
        fw.wgrad(mk(100, 256), mk(100, 384))
    from sharedtensor_amd import _core
    s = torch.cuda.current_stream().cuda_stream
    out = mk(256, 384)
    with pytest.raises(RuntimeError):  # the launcher checks again
        _core.wgrad_bf16(dy.data_ptr(), x.data_ptr(), out.data_ptr(), 0, 0,
                         128, 256, 384, 256, 384, 384, 2, 0, s)  # no ws
    with pytest.raises(RuntimeError):
        _core.wgrad_bf16(dy.data_ptr(), x.data_ptr(), out.data_ptr(), 0, 0,
                         100, 256, 384, 256, 384, 384, 1, 0, s)
