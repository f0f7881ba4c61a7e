"""The 256 x 256 variant of the split-K weight-gradient kernel and the column
sums of dY it takes on the way (csrc/wgrad_kernels.hip, k_wgrad256), through
ops/fused_wgrad.py.

Rules and helpers are those of test_gpu_fused_wgrad.py: fp64 reference; the
kernel's max-abs and relative-L2 error may be at most 1.5x ``torch.mm``'s,
with that file's operation-count floor; dW, the workspaces and db sit inside
sentinel guards; the workspaces and db are NaN-filled before every call, so a
partial read before it is written, or a db element nobody wrote, shows in the
result; every case runs twice and wants equal bits.

db is held to the fp64 column sum the same way: its error may be at most
1.5x that of ``dy.sum(0)``, above the floor, per element,

    floor_b[n] = 2^-8 |ref[n]| + (M + 64) 2^-24 sum_m |dY[m, n]|

(one bf16 rounding, M fp32 additions of values exact in fp32, the split sums).

Shapes are the smallest at which each mechanism can fail: one tile and one
step (the direct bf16 stores, db included); 5 steps over 3 splits (2/2/1) and
over 8 (three empty splits, db with split > steps) at N = 512, K = 256 with
unrelated operands; the selector and cancel families at M = 320; the
workload's feature sizes and split at 7 steps; row-strided operands.
"""
import pytest
import torch
import torch.nn.functional as F

from test_gpu_fused_wgrad import (MARGIN, _case, _check, _errs, _fw,
                                  _guarded, _guards_intact)

pytestmark = pytest.mark.gpu

V256 = 3


def _db_case(c):
    """fp64 column sum of the case's dY, dy.sum(0) and the floor (cached in
    the shared case dict)."""
    if "db_ref" not in c:
        d64 = c["dy"].double()
        M = d64.shape[0]
        ref = d64.sum(0)
        floor = 2.0 ** -8 * ref.abs() + (M + 64) * 2.0 ** -24 * d64.abs().sum(0)
        c["db_ref"] = ref
        c["db_lib"] = c["dy"].sum(0)
        c["db_floor_abs"] = floor.max().item()
        c["db_floor_l2"] = (floor.norm() / ref.norm().clamp_min(1e-300)).item()
    return c


def _check_db(c, got, tag):
    c = _db_case(c)
    f_abs, f_l2 = _errs(got, c["db_ref"])
    a_abs, a_l2 = _errs(c["db_lib"], c["db_ref"])
    print(f"WGRAD256 db {tag}: maxabs fused {f_abs:.3e} sum(0) {a_abs:.3e} "
          f"floor {c['db_floor_abs']:.3e} | rel-l2 fused {f_l2:.3e} sum(0) "
          f"{a_l2:.3e} floor {c['db_floor_l2']:.3e}")
    # a NaN (an element nobody wrote) fails both comparisons
    assert f_abs <= max(MARGIN * a_abs, c["db_floor_abs"])
    assert f_l2 <= max(MARGIN * a_l2, c["db_floor_l2"])


def _run(dy, x, split, ldw=None, with_db=True):
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
        fw.wgrad(dy, x, out=out, split=split, variant=V256, ws=ws,
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


# (M, N, K, split)
SHAPES = [
    (64, 256, 256, 1),      # one tile, one step: direct bf16 stores, db too
    (320, 512, 256, 3),     # 5 steps as 2/2/1, N != K
    (320, 512, 256, 8),     # 5 steps over 8 splits: three empty ones
    (320, 256, 256, 2),     # the cancel family's shape
    (448, 3072, 768, 7),    # mlp.fc at 7 steps, the workload's split
    (448, 768, 3072, 7),    # mlp.proj
]


@pytest.mark.parametrize("family", ["randn", "cancel"])
@pytest.mark.parametrize("M,N,K,split", SHAPES)
def test_dw_and_db_against_fp64(M, N, K, split, family):
    c = _case(M, N, K, family)
    dw, db = _run(c["dy"], c["x"], split)
    tag = f"{family} M{M} N{N} K{K} split {split}"
    _check(c, dw, tag)
    _check_db(c, db, tag)


@pytest.mark.parametrize("M,N,K,split", [(64, 256, 256, 1),
                                         (320, 512, 256, 8)])
def test_without_db_nothing_of_it_is_written(M, N, K, split):
    c = _case(M, N, K, "randn")
    dw, _ = _run(c["dy"], c["x"], split, with_db=False)
    with_db, _ = _run(c["dy"], c["x"], split)
    assert torch.equal(dw.view(torch.int16), with_db.view(torch.int16))


@pytest.mark.parametrize("split", [1, 3, 8])
def test_selector_sums_rows_bit_for_bit(split):
    """dY has a single 1 per row; the first 256 rows pick distinct columns,
    the last 64 pick 64 of them again (M = 320 > N = 256).  Row n of dW is
    the sum of the one or two X rows that picked n, which is exact in fp32
    up to one rounding that does not depend on the order, then rounded to
    bf16; db[n] is their count."""
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
    assert torch.equal(dw.view(torch.int16),
                       want.bfloat16().view(torch.int16))
    count = torch.zeros(N, device="cuda").index_add_(
        0, cols, torch.ones(M, device="cuda"))
    assert torch.equal(db.float(), count)


def test_strided_operands_and_output():
    """dY as a column slice of a wider buffer, X with padded rows, dW with
    padded rows: the padding stays, the bits equal the dense call's."""
    fw = _fw()
    M, N, K = 192, 256, 256
    c = _case(M, N, K, "randn", 5)
    wide = torch.randn(M, 3 * N, device="cuda").bfloat16()
    wide[:, N:2 * N] = c["dy"]
    dy = wide[:, N:2 * N]
    xw = torch.randn(M, K + 64, device="cuda").bfloat16()
    xw[:, :K] = c["x"]
    x = xw[:, :K]
    assert fw.can_use(dy, x, V256) and not dy.is_contiguous()
    dw, db = _run(dy, x, 2, ldw=K + 8)
    _check(c, dw, "strided v3")
    _check_db(c, db, "strided v3")
    dense_dw, dense_db = _run(c["dy"], c["x"], 2)
    assert torch.equal(dw.view(torch.int16), dense_dw.view(torch.int16))
    assert torch.equal(db.view(torch.int16), dense_db.view(torch.int16))


def test_db_only_from_variants_that_have_it():
    fw = _fw()
    c = _case(64, 256, 256, "randn")
    db = torch.empty(256, dtype=torch.bfloat16, device="cuda")
    for v in (0, 1, 2):
        with pytest.raises(ValueError):
            fw.wgrad(c["dy"], c["x"], variant=v, db_out=db)
    from sharedtensor_amd import _core
    s = torch.cuda.current_stream().cuda_stream
    out = torch.empty(256, 256, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(RuntimeError):  # the launcher checks again
        _core.wgrad_bf16(c["dy"].data_ptr(), c["x"].data_ptr(),
                         out.data_ptr(), 0, 0, 64, 256, 256, 256, 256, 256,
                         1, 1, s, db.data_ptr(), 0, 0)
    with pytest.raises(RuntimeError):  # split > 1 and no wsb
        ws = torch.empty(2 * 256 * 256, device="cuda")
        _core.wgrad_bf16(c["dy"].data_ptr(), c["x"].data_ptr(),
                         out.data_ptr(), ws.data_ptr(), ws.numel(), 64, 256,
                         256, 256, 256, 256, 2, V256, s, db.data_ptr(), 0, 0)
    assert not fw.can_use(c["dy"][:, :128], c["x"], V256)       # N % 256
    assert not fw.can_use(c["dy"], c["x"][:, :128], V256)       # K % 256


def test_linear_wgrad_with_bias_against_linear_autograd(monkeypatch):
    """linear_wgrad with a bias at M = 128 with the shape wired to the
    256 x 256 variant: dx, dw and db against F.linear's autograd, each held
    to 1.5x its error against fp64."""
    fw = _fw()
    N, K = 256, 512
    monkeypatch.setattr(fw, "TUNED", {(N, K): V256})
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
    M = 128
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
        print(f"WGRAD256 module {name}: maxabs fused {f_abs:.3e} linear "
              f"{a_abs:.3e} | rel-l2 fused {f_l2:.3e} linear {a_l2:.3e}")
        assert f_abs <= max(MARGIN * a_abs, fl.max().item())
        assert f_l2 <= max(MARGIN * a_l2, (fl.norm() / rf.norm()).item())
