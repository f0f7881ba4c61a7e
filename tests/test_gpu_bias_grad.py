"""k_gelu_bwd_colsum, k_pack3_colsum and their second stage
(csrc/bias_grad_kernels.hip) against fp64 references with derived bounds,
and the two autograd Functions inside a small GPT-2 block.

A bias gradient db[c] (bf16) is checked twice.

1. Against the fp64 column sum of the bf16 dx the kernel itself returned
   (that dx is bounded element by element against the reference first):

       gamma(R) * sum_r |dx[r, c]|  +  1 bf16 ulp at |ref|

   A dropped or doubled row, a sum over the unrounded fp32 dx or a
   lower-precision accumulation all exceed it.

2. Against the fp64 column sum of the reference's bf16-rounded dx:

       sum_r tol[r, c]  +  gamma(R) * sum_r |dx[r, c]|  +  1 bf16 ulp at |ref|

   tol is gelu_slack, the fp32 evaluation error of one element.  Where the
   reference lies within that slack of a bf16 rounding boundary the kernel's
   value may round to the other neighbour, and only those elements are
   granted one bf16 ulp more.  For the pack kernel the copy is bit-exact,
   tol is 0 and the two checks coincide.

* gamma(R) = R u / (1 - R u) bounds an fp32 sum of R terms in any order
  (row loop, LDS combine and second stage together add each term once).
* one bf16 ulp for the final rounding (half) and a rounding the fp32 error
  flipped (half), as in kernel_bounds.assert_bf16.

A column holding a NaN must come out NaN and no other column may.
"""
import pytest
import torch

import kernel_bounds as kb
from sharedtensor_amd import _core

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _partial(ncols):
    return torch.empty(_core.bias_grad_partial_floats(ncols),
                       dtype=torch.float32, device="cuda")


def run_gelu(dy, x):
    R, C = x.shape
    dx = torch.empty_like(x)
    db = torch.empty(C, dtype=BF, device="cuda")
    part = _partial(C)
    _core.gelu_bwd_colsum(dy.data_ptr(), x.data_ptr(), dx.data_ptr(),
                          db.data_ptr(), part.data_ptr(), R, C, _stream())
    torch.cuda.synchronize()
    return dx, db


def run_pack(srcs):
    R, C = srcs[0].shape
    dst = torch.empty(R, 3 * C, dtype=BF, device="cuda")
    db = torch.empty(3 * C, dtype=BF, device="cuda")
    part = _partial(3 * C)
    _core.pack3_colsum(srcs[0].data_ptr(), srcs[1].data_ptr(),
                       srcs[2].data_ptr(), dst.data_ptr(), db.data_ptr(),
                       part.data_ptr(), R, C, _stream())
    torch.cuda.synchronize()
    return dst, db


def colsum_tol(ref_dx_bf16, elem_tol, R):
    """The accumulation part of the bound (the final ulp is added by
    assert_bf16)."""
    a = ref_dx_bf16.double().abs().sum(0)
    return elem_tol.sum(0) + kb.gamma(R) * a


def check_db(db, dx_ref64, elem_tol, op, family):
    R = dx_ref64.shape[0]
    rounded = dx_ref64.to(BF)
    ref = rounded.double().sum(0)
    nan_col = torch.isnan(dx_ref64).any(0)
    assert torch.equal(torch.isnan(db), nan_col), (op, family)
    # a rounded reference of +-inf makes the column sum inf or NaN; the
    # families here stay finite outside their NaN columns
    assert bool(torch.isfinite(ref[~nan_col]).all())
    tol = colsum_tol(rounded.nan_to_num(0.0), elem_tol.nan_to_num(0.0), R)
    kb.assert_bf16(db, ref, tol, op, "db", family)


def flip_tol(ref, slack):
    """Per-element allowance between the kernel's rounded dx and the
    reference's: the slack, plus one bf16 ulp where the reference is within
    the slack of the midpoint between two bf16 values (an error of at most
    `slack` can move the rounding across it), nothing more elsewhere."""
    r = ref.nan_to_num(0.0)
    ulp = kb.bf16_ulp(r)
    to_mid = 0.5 * ulp - (r - r.to(BF).double()).abs()
    return slack + torch.where(to_mid <= slack, ulp, torch.zeros_like(ulp))


def gelu_rows_grid_stride(C):
    """Narrow C: more than two sweeps of the capped grid, plus one row."""
    sweep = _core.bias_grad_sweep_rows(1 << 40, C, False)
    return 2 * sweep + 1


GELU_SHAPES = [(1, 8), (3, 768), (257, 3072), (1031, 3072), (4099, 264),
               ("stride", 8)]
GELU_FAMILIES = ["randn", "zero_dy", "cancel", "clamp", "nan"]


def gelu_inputs(family, R, C):
    g = torch.Generator(device="cuda").manual_seed(31 * R + C)

    def rn(*shape, scale=1.0):
        return torch.randn(*shape, generator=g, device="cuda") * scale
    x = rn(R, C, scale=3.0)
    dy = rn(R, C)
    if family == "zero_dy":
        dy = torch.zeros(R, C, device="cuda")
    elif family == "cancel":
        # one x per column and dy = +-a(c) on alternating rows: the rounded
        # dx of a column are +-one value, their true sum is exactly 0
        # (an odd R gets a last row of dy = 0)
        x = rn(1, C, scale=3.0).expand(R, C).contiguous()
        sign = torch.where(torch.arange(R, device="cuda") % 2 == 0, 1.0, -1.0)
        if R % 2:
            sign[-1] = 0.0
        dy = sign[:, None] * (rn(1, C).abs() + 0.5)
    elif family == "clamp":
        vals = torch.tensor([-1e20, -10.5, -10.0, -9.98, -0.0, 9.98, 10.0,
                             10.5, 1e20], device="cuda")
        idx = torch.randint(0, len(vals), (R, C), generator=g, device="cuda")
        x = vals[idx]
    elif family == "nan":
        x[R // 2, 1] = float("nan")
        dy[R - 1, C - 3] = float("nan")
    elif family != "randn":
        raise ValueError(family)
    return dy.to(BF).contiguous(), x.to(BF).contiguous()


@pytest.mark.parametrize("family", GELU_FAMILIES)
@pytest.mark.parametrize("shape", GELU_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_gelu_bwd_colsum(shape, family):
    R, C = shape
    if R == "stride":
        R = gelu_rows_grid_stride(C)
    dy, x = gelu_inputs(family, R, C)
    dx, db = run_gelu(dy, x)
    ref = kb.gelu_formula(x, dy)["dx"]
    slack = kb.gelu_slack(x, dy)["dx"]
    fam = f"{family}/{R}x{C}"
    assert torch.equal(torch.isnan(dx), torch.isnan(ref)), fam
    kb.assert_bf16(dx, ref, slack, "gelu_bwd_colsum", "dx", fam)
    # 1. the sum of what the kernel wrote: accumulation error alone
    zero = torch.zeros_like(ref)
    check_db(db, dx.double(), zero, "gelu_bwd_colsum/own-dx", fam)
    # 2. the sum of the reference's rounded dx
    check_db(db, ref, flip_tol(ref, slack), "gelu_bwd_colsum", fam)
    if family == "cancel":
        assert float(ref.to(BF).double().sum(0).abs().max()) == 0.0
    if family == "nan":
        assert int(torch.isnan(db).sum()) == 2 and int(torch.isnan(dx).sum()) == 2


def test_gelu_bwd_colsum_matches_gelu_bwd_bits():
    """dx is the very value k_gelu_bwd writes (shared gelu_grad_f)."""
    dy, x = gelu_inputs("clamp", 257, 3072)
    dx, _ = run_gelu(dy, x)
    dx2 = torch.empty_like(x)
    _core.gelu_bwd(dy.data_ptr(), x.data_ptr(), dx2.data_ptr(), x.numel(),
                   _stream())
    torch.cuda.synchronize()
    assert torch.equal(dx.view(torch.int16), dx2.view(torch.int16))


PACK_SHAPES = [(R, C) for C in (8, 768) for R in (1, 5, 1031)] + [("stride", 8)]


@pytest.mark.parametrize("shape", PACK_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pack3_colsum(shape):
    R, C = shape
    if R == "stride":
        R = 2 * _core.bias_grad_sweep_rows(1 << 40, 3 * C, True) + 1
    g = torch.Generator(device="cuda").manual_seed(5 * R + C)
    srcs = [(torch.randn(R, C, generator=g, device="cuda") * (s + 1)).to(BF)
            for s in range(3)]
    dst, db = run_pack(srcs)
    want = torch.cat(srcs, dim=1)
    assert torch.equal(dst.view(torch.int16), want.view(torch.int16))
    zero = torch.zeros(R, 3 * C, dtype=torch.float64, device="cuda")
    check_db(db, want.double(), zero, "pack3_colsum", f"randn/{R}x{C}")


def test_pack3_copies_every_bit_pattern():
    """NaN payloads, infinities and subnormals pass through unchanged."""
    R, C = 3 * 1024, 64
    bits = torch.arange(3 * R * C, device="cuda", dtype=torch.int32)
    bits = (bits * 40503 % 65536).to(torch.int16).view(BF).view(3, R, C)
    srcs = [bits[s].contiguous() for s in range(3)]
    dst, _ = run_pack(srcs)
    want = torch.cat(srcs, dim=1)
    assert torch.equal(dst.view(torch.int16), want.view(torch.int16))


def test_column_sums_repeat_bit_for_bit():
    dy, x = gelu_inputs("randn", 1031, 3072)
    _, a = run_gelu(dy, x)
    _, b = run_gelu(dy, x)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    srcs = [dy[:, :768].contiguous(), x[:, :768].contiguous(),
            dy[:, 768:1536].contiguous()]
    _, a = run_pack(srcs)
    _, b = run_pack(srcs)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


def test_entry_points_check_shape_and_alignment():
    x = torch.zeros(4, 16, dtype=BF, device="cuda")
    part = _partial(16)
    db = torch.empty(48, dtype=BF, device="cuda")
    p = x.data_ptr()
    with pytest.raises(RuntimeError, match="multiple of 8"):
        _core.gelu_bwd_colsum(p, p, p, db.data_ptr(), part.data_ptr(), 4, 12,
                              _stream())
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        _core.gelu_bwd_colsum(p + 2, p, p, db.data_ptr(), part.data_ptr(), 2,
                              16, _stream())
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        _core.pack3_colsum(p, p, p + 8, p, db.data_ptr(), part.data_ptr(), 1,
                           16, _stream())
    with pytest.raises(RuntimeError, match="empty"):
        _core.pack3_colsum(p, p, p, p, db.data_ptr(), part.data_ptr(), 0, 16,
                           _stream())


# ------------------------------------------------------------ autograd level

def _block(seed=0, dtype=BF, device="cuda"):
    from sharedtensor_amd.models.gpt2 import Block, GPT2Config
    torch.manual_seed(seed)
    cfg = GPT2Config(vocab_size=256, n_layer=1, n_head=4, n_embd=256,
                     block_size=16)
    blk = Block(cfg)
    for p in blk.parameters():       # biases start at 0; make them count
        if p.dim() == 1:
            torch.nn.init.normal_(p, std=0.1)
    return blk.to(device).to(dtype)


def _run_block(blk, x, dy):
    for p in blk.parameters():
        p.grad = None
    xi = x.clone().requires_grad_(True)
    xo, m, _ = blk(xi)
    out = xo + m
    out.backward(dy)
    grads = {n: p.grad.clone() for n, p in blk.named_parameters()}
    grads["input"] = xi.grad.clone()
    return out.detach(), grads


def _graph_names(t):
    seen, names, todo = set(), [], [t.grad_fn]
    while todo:
        f = todo.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        names.append(type(f).__name__)
        todo.extend(n for n, _ in f.next_functions)
    return sorted(names)


def _bits_equal(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


def test_block_flags_on_against_off(monkeypatch):
    import torch.nn.functional as F
    import sharedtensor_amd.models.gpt2 as g
    from sharedtensor_amd.ops import fused_bias_grad as fb
    blk = _block()
    torch.manual_seed(1)
    x = torch.randn(2, 16, 256, device="cuda").to(BF)
    dy = torch.randn(2, 16, 256, device="cuda").to(BF)

    # capture what reaches and leaves the two Functions, and in the unfused
    # path what leaves GeluBackward
    cap = {}
    orig_gelu, orig_split, torch_gelu = (fb.bias_gelu_bgrad,
                                         fb.qkv_split_bgrad, F.gelu)

    def keep(key):
        return lambda gr: cap.__setitem__(key, gr.clone())

    def gelu_spy(pre, b):
        cap["pre"] = pre.detach().clone()
        pre.register_hook(keep("dpre"))
        h = orig_gelu(pre, b)
        h.register_hook(keep("dh"))
        return h

    def split_spy(qkv, b):
        qkv.register_hook(keep("dqkv"))
        return orig_split(qkv, b)

    def torch_gelu_spy(t, *a, **k):
        # the unfused path; our Function's forward runs with grad mode off
        if t.requires_grad and torch.is_grad_enabled():
            t.register_hook(keep("dpre_torch"))
        return torch_gelu(t, *a, **k)
    monkeypatch.setattr(fb, "bias_gelu_bgrad", gelu_spy)
    monkeypatch.setattr(fb, "qkv_split_bgrad", split_spy)
    monkeypatch.setattr(F, "gelu", torch_gelu_spy)

    def run(fc, qkv):
        cap.clear()
        monkeypatch.setattr(g, "FUSE_FC_BIAS_GRAD", fc)
        monkeypatch.setattr(g, "FUSE_QKV_BIAS_GRAD", qkv)
        with torch.autocast("cuda", BF):
            y, grads = _run_block(blk, x, dy)
        return y, grads, dict(cap)

    y_off, g_off, c_off = run(False, False)
    y_qkv, g_qkv, c_qkv = run(False, True)
    y_on, g_on, c_on = run(True, True)
    assert set(c_off) == {"dpre_torch"}     # neither Function ran
    assert set(c_qkv) == {"dpre_torch", "dqkv"}
    assert set(c_on) == {"pre", "dpre", "dh", "dqkv"}
    assert _bits_equal(y_qkv, y_off) and _bits_equal(y_on, y_off)

    def db_bound(d):
        """(exact column sum, accumulation bound + final ulp) of bf16 d."""
        d = d.reshape(-1, d.shape[-1]).double()
        ref = d.sum(0)
        return ref, kb.gamma(d.shape[0]) * d.abs().sum(0) + kb.bf16_ulp(ref)

    # qkv half alone: dqkv is a bit-exact copy, so every gradient but
    # qkv.bias is bit-identical to the unfused run; qkv.bias is the column
    # sum of that very dqkv, and so is torch's reduce in the unfused run:
    # each within the accumulation bound of the exact sum, twice that apart
    for name in g_off:
        if name != "attn.qkv.bias":
            assert _bits_equal(g_qkv[name], g_off[name]), name
    zero = torch.zeros(32, 768, dtype=torch.float64, device="cuda")
    d = c_qkv["dqkv"].reshape(32, 768)
    assert g_qkv["attn.qkv.bias"].dtype == BF
    check_db(g_qkv["attn.qkv.bias"], d.double(), zero, "block/qkv",
             "attn.qkv.bias")
    ref, tol = db_bound(d)
    diff = (g_qkv["attn.qkv.bias"].double()
            - g_off["attn.qkv.bias"].double()).abs()
    assert bool((diff <= 2 * tol).all())

    # both halves: dpre against the fp64 formula on the captured inputs,
    # each bias gradient against the column sum of the packed gradient this
    # very run produced
    pre = c_on["pre"].reshape(32, 1024)
    dh = c_on["dh"].reshape(32, 1024)
    dpre = c_on["dpre"].reshape(32, 1024)
    fref = kb.gelu_formula(pre, dh)["dx"]
    fslack = kb.gelu_slack(pre, dh)["dx"]
    kb.assert_bf16(dpre, fref, fslack, "block", "dpre", "both")
    zero = torch.zeros_like(fref)
    check_db(g_on["mlp.fc.bias"], dpre.double(), zero, "block/both",
             "mlp.fc.bias")
    check_db(g_on["mlp.fc.bias"], fref, flip_tol(fref, fslack), "block/both",
             "mlp.fc.bias/ref")
    check_db(g_on["attn.qkv.bias"],
             c_on["dqkv"].reshape(32, 768).double(),
             torch.zeros(32, 768, dtype=torch.float64, device="cuda"),
             "block/both", "attn.qkv.bias")
    # dh does not depend on the flags.  torch's GeluBackward meets the same
    # elementwise bound; where its dpre and ours agree to the bit, all that
    # follows is the same torch code on the same bits, so every gradient but
    # the two bias sums is bit-identical.  Where they differ by a rounding,
    # the elementwise bounds above are what holds for both.
    dpre_t = c_off["dpre_torch"].reshape(32, 1024)
    kb.assert_bf16(dpre_t, fref, fslack, "block", "dpre_torch", "off")
    n_diff = int((dpre.view(torch.int16) != dpre_t.view(torch.int16)).sum())
    print(f"DPRE elements differing from torch's: {n_diff} of {dpre.numel()}")
    if n_diff == 0:
        for name in g_off:
            if name not in ("attn.qkv.bias", "mlp.fc.bias"):
                assert _bits_equal(g_on[name], g_off[name]), name
        ref, tol = db_bound(dpre)
        diff = (g_on["mlp.fc.bias"].double()
                - g_off["mlp.fc.bias"].double()).abs()
        assert bool((diff <= 2 * tol).all())


def test_fallbacks_keep_the_parent_graph(monkeypatch):
    import sharedtensor_amd.models.gpt2 as g

    def names(blk, x, autocast):
        if autocast:
            with torch.autocast("cuda", BF):
                xo, m, _ = blk(x)
        else:
            xo, m, _ = blk(x)
        return _graph_names(xo + m)

    # fp32 parameters under autocast, and CPU: same graph with the flags on
    # as with them off, and no node of the fused Functions in it
    cases = [(_block(dtype=torch.float32), "cuda", True),
             (_block(dtype=torch.float32, device="cpu"), "cpu", False)]
    for blk, dev, autocast in cases:
        x = torch.randn(2, 16, 256, device=dev)
        monkeypatch.setattr(g, "FUSE_FC_BIAS_GRAD", True)
        monkeypatch.setattr(g, "FUSE_QKV_BIAS_GRAD", True)
        on = names(blk, x, autocast)
        monkeypatch.setattr(g, "FUSE_FC_BIAS_GRAD", False)
        monkeypatch.setattr(g, "FUSE_QKV_BIAS_GRAD", False)
        off = names(blk, x, autocast)
        monkeypatch.undo()
        assert on == off
        assert not [n for n in on if "BiasGelu" in n or "QkvSplit" in n]

    # bf16 on the GPU: the module flags decide, the environment overrides
    # either of them in both directions
    blk = _block()
    x = torch.randn(2, 16, 256, device="cuda").to(BF)
    monkeypatch.setattr(g, "FUSE_FC_BIAS_GRAD", True)
    monkeypatch.setattr(g, "FUSE_QKV_BIAS_GRAD", True)
    both = names(blk, x, True)
    assert any("BiasGelu" in n for n in both)
    assert any("QkvSplit" in n for n in both)
    monkeypatch.setenv("SHTENS_FUSED_GELU_BGRAD", "0")
    one = names(blk, x, True)
    assert not any("BiasGelu" in n for n in one)
    assert any("QkvSplit" in n for n in one)
    monkeypatch.setenv("SHTENS_FUSED_QKV_BGRAD", "0")
    assert not any("QkvSplit" in n for n in names(blk, x, True))
    monkeypatch.setattr(g, "FUSE_FC_BIAS_GRAD", False)
    monkeypatch.setenv("SHTENS_FUSED_GELU_BGRAD", "1")
    assert any("BiasGelu" in n for n in names(blk, x, True))
