"""The pipelined 256 x 256 variant of the split-K weight-gradient kernel
(csrc/wgrad_kernels.hip, k_wgrad256p; variant 4 of ops/fused_wgrad.py).

Rules and helpers are those of test_gpu_fused_wgrad.py and
test_gpu_fused_wgrad256.py: fp64 reference, 1.5x ``torch.mm``'s error above
the operation-count floor, guards, NaN-filled workspaces, db and wsb, every
run twice with equal bits.  On top of that dW must have the bits of variant
3 at the same split: both kernels issue the same MFMAs in the same order on
every accumulator.  db is held to the fp64 floor, not to variant 3's bits:
its summation order differs.

The ring has four 32-token slots, two 64-token steps.  Step counts 1, 2, 3
and 5 (and 4, 6) at one tile cover a prologue longer than the work, the ring
wrap, and odd counts, which start the ring at slot 2.  The other shapes are
those of the 256 x 256 test.  A load of a half step at or past its split's
count cannot be observed from here; the last-row test below only sets up the
configuration in which it would leave the buffer.
"""
import pytest
import torch
import torch.nn.functional as F

from test_gpu_fused_wgrad import (MARGIN, _case, _check, _errs, _fw,
                                  _guarded, _guards_intact)
from test_gpu_fused_wgrad256 import _check_db

pytestmark = pytest.mark.gpu

V256, V256P = 3, 4


def _run(dy, x, split, variant=V256P, ldw=None, with_db=True):
    """The kernel twice inside guards, with NaN-filled workspaces and db;
    returns (dW, db) after checking guards and bit-equality."""
    fw = _fw()
    N, K = dy.shape[1], x.shape[1]
    ldw = K if ldw is None else ldw
    outs = []
    for _ in range(2):
        obuf, o = _guarded(N * ldw, torch.bfloat16, -7.0)
        out = o.view(N, ldw)[:, :K]
        wbuf, ws = _guarded(max(split * N * K, 8), torch.float32, 12345.0)
        ws.fill_(float("nan"))
        bbuf, db = _guarded(N, torch.bfloat16, -7.0)
        db.fill_(float("nan"))
        sbuf, wsb = _guarded(max(split * N, 8), torch.float32, 12345.0)
        wsb.fill_(float("nan"))
        fw.wgrad(dy, x, out=out, split=split, variant=variant, ws=ws,
                 db_out=db if with_db else None, wsb=wsb)
        torch.cuda.synchronize()
        assert _guards_intact(obuf, -7.0), "dW guard overwritten"
        assert _guards_intact(wbuf, 12345.0), "workspace guard overwritten"
        assert _guards_intact(bbuf, -7.0), "db guard overwritten"
        assert _guards_intact(sbuf, 12345.0), "db workspace guard overwritten"
        if ldw > K:  # the padding between rows belongs to the caller
            pad = o.view(N, ldw)[:, K:]
            assert torch.equal(pad, torch.full_like(pad, -7.0))
        if not with_db:
            assert torch.isnan(db).all() and torch.isnan(wsb).all(), \
                "db or its workspace written without db_out"
        outs.append((out.clone(), db.clone()))
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), \
            "two calls on the same inputs differ"
    return outs[0]


def _same_bits(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


# (M, N, K, split)
SHAPES = [(64 * s, 256, 256, 1) for s in (1, 2, 3, 4, 5, 6)] + [
    (320, 512, 256, 3),     # 5 steps as 2/2/1, N != K
    (320, 512, 256, 8),     # 5 steps over 8 splits: three empty ones
    (320, 256, 256, 2),     # the cancel family's shape
    (448, 3072, 768, 7),    # mlp.fc at 7 steps, the workload's split
    (448, 768, 3072, 7),    # mlp.proj
]


@pytest.mark.parametrize("family", ["randn", "cancel"])
@pytest.mark.parametrize("M,N,K,split", SHAPES)
def test_dw_and_db_against_fp64_and_variant3(M, N, K, split, family):
    c = _case(M, N, K, family)
    dw, db = _run(c["dy"], c["x"], split)
    tag = f"{family} M{M} N{N} K{K} split {split} v4"
    _check(c, dw, tag)
    _check_db(c, db, tag)
    dw3, _ = _run(c["dy"], c["x"], split, variant=V256)
    assert _same_bits(dw, dw3), "dW differs from variant 3"


@pytest.mark.parametrize("M,N,K,split", [(64, 256, 256, 1),
                                         (320, 512, 256, 8)])
def test_without_db_nothing_of_it_is_written(M, N, K, split):
    c = _case(M, N, K, "randn")
    dw, _ = _run(c["dy"], c["x"], split, with_db=False)
    with_db, _ = _run(c["dy"], c["x"], split)
    assert _same_bits(dw, with_db)
    dw3, _ = _run(c["dy"], c["x"], split, variant=V256, with_db=False)
    assert _same_bits(dw, dw3), "dW differs from variant 3"


@pytest.mark.parametrize("split", [1, 3, 8])
def test_selector_sums_rows_bit_for_bit(split):
    """As in test_gpu_fused_wgrad256.py: one 1 per dY row, M = 320 > N, so
    dW rows are exact sums of one or two X rows and db counts them."""
    M, N, K = 320, 256, 256
    g = torch.Generator(device="cuda").manual_seed(3)
    cols = torch.cat([torch.randperm(N, generator=g, device="cuda"),
                      torch.randperm(N, generator=g, device="cuda")[:M - N]])
    dy = torch.zeros(M, N, device="cuda")
    dy[torch.arange(M, device="cuda"), cols] = 1.0
    dy = dy.bfloat16()
    x = torch.randn(M, K, generator=g, device="cuda").bfloat16()
    dw, db = _run(dy, x, split)
    want = torch.zeros(N, K, device="cuda").index_add_(0, cols, x.float())
    assert _same_bits(dw, want.bfloat16())
    dw3, _ = _run(dy, x, split, variant=V256)
    assert _same_bits(dw, dw3), "dW differs from variant 3"
    count = torch.zeros(N, device="cuda").index_add_(
        0, cols, torch.ones(M, device="cuda"))
    assert torch.equal(db.float(), count)


def test_strided_operands_and_output():
    """dY as the middle column slice of a (M, 3N) buffer, X with padded rows,
    dW with padded rows: the global-side swizzle with ldy != N."""
    fw = _fw()
    M, N, K = 192, 256, 256
    c = _case(M, N, K, "randn", 5)
    wide = torch.randn(M, 3 * N, device="cuda").bfloat16()
    wide[:, N:2 * N] = c["dy"]
    dy = wide[:, N:2 * N]
    xw = torch.randn(M, K + 64, device="cuda").bfloat16()
    xw[:, :K] = c["x"]
    x = xw[:, :K]
    assert fw.can_use(dy, x, V256P) and not dy.is_contiguous()
    dw, db = _run(dy, x, 2, ldw=K + 8)
    _check(c, dw, "strided v4")
    _check_db(c, db, "strided v4")
    dense_dw, dense_db = _run(c["dy"], c["x"], 2)
    assert _same_bits(dw, dense_dw) and _same_bits(db, dense_db)
    dw3, _ = _run(c["dy"], c["x"], 2, variant=V256)
    assert _same_bits(dw, dw3)


def test_operands_end_at_the_end_of_a_buffer():
    """Each operand is the tail of a 12 MiB buffer of its own, and the last
    split (of 2, over 3 steps) ends on its last row.  A request above 10 MiB
    gets a segment of its own from the caching allocator, rounded to 2 MiB,
    so when no larger cached block is reused the operand's last byte is the
    segment's last byte: a prefetch past the split would leave it."""
    M, N, K = 192, 256, 256
    c = _case(M, N, K, "randn", 7)
    whole = 12 * 1024 * 1024 // 2
    dy = torch.empty(whole, dtype=torch.bfloat16,
                     device="cuda")[whole - M * N:].view(M, N)
    x = torch.empty(whole, dtype=torch.bfloat16,
                    device="cuda")[whole - M * K:].view(M, K)
    dy.copy_(c["dy"])
    x.copy_(c["x"])
    dw, db = _run(dy, x, 2)
    _check(c, dw, "last row v4")
    _check_db(c, db, "last row v4")
    dw3, _ = _run(dy, x, 2, variant=V256)
    assert _same_bits(dw, dw3), "dW differs from variant 3"


def test_linear_wgrad_with_bias_against_linear_autograd(monkeypatch):
    """linear_wgrad with a bias at (2, 64, 256) -> 256 wired to variant 4:
    dx, dw and db against F.linear's autograd, each held to 1.5x its error
    against fp64."""
    fw = _fw()
    N, K, M = 256, 256, 128
    monkeypatch.setattr(fw, "TUNED", {(N, K): V256P})
    calls = []
    real = fw.wgrad
    monkeypatch.setattr(
        fw, "wgrad", lambda *a, **k: (calls.append(k.get("db_out")),
                                      real(*a, **k))[1])
    g = torch.Generator(device="cuda").manual_seed(21)
    mk = lambda *s: torch.randn(*s, generator=g, device="cuda").bfloat16()
    x, w, b, dy = mk(2, 64, K), mk(N, K) * 0.05, mk(N), mk(2, 64, N)

    def grads(fn, dt):
        ins = [t.detach().to(dt).requires_grad_() for t in (x, w, b)]
        return torch.autograd.grad(fn(*ins), ins, dy.to(dt))

    ref = grads(F.linear, torch.float64)
    lib = grads(F.linear, torch.bfloat16)
    assert not calls
    got = grads(fw.linear_wgrad, torch.bfloat16)
    assert len(calls) == 1 and calls[0] is not None, \
        "db did not come from the kernel"
    d64, x64, w64 = (t.double().reshape(-1, t.shape[-1]) for t in (dy, x, w))
    floors = [
        2.0 ** -8 * ref[0].abs().reshape(M, K)
        + (N + 64) * 2.0 ** -24 * (d64.abs() @ w64.abs()),
        2.0 ** -8 * ref[1].abs() + (M + 64) * 2.0 ** -24 * (d64.abs().t()
                                                            @ x64.abs()),
        2.0 ** -8 * ref[2].abs() + (M + 64) * 2.0 ** -24 * d64.abs().sum(0),
    ]
    for name, gt, lb, rf, fl in zip(("dx", "dw", "db"), got, lib, ref, floors):
        assert gt.shape == lb.shape and gt.dtype == lb.dtype
        f_abs, f_l2 = _errs(gt, rf)
        a_abs, a_l2 = _errs(lb, rf)
        print(f"WGRAD256P module {name}: maxabs fused {f_abs:.3e} linear "
              f"{a_abs:.3e} | rel-l2 fused {f_l2:.3e} linear {a_l2:.3e}")
        assert f_abs <= max(MARGIN * a_abs, fl.max().item())
        assert f_l2 <= max(MARGIN * a_l2, (fl.norm() / rf.norm()).item())
