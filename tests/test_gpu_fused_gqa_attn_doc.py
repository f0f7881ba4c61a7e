"""The document-masked grouped-query attention kernels
(csrc/gqa_attn_doc_kernels.hip, csrc/gqa_attn_doc_bwd_kernels.hip) and the
doc_ids path of ops/fused_gqa_attn.py against fp64 softmax attention with the
document mask over repeat_interleave'd K/V, with autograd.

Tolerance, as in test_gpu_fused_gqa_attn.py: nothing is fixed in advance.
Max-abs and relative-L2 error of out, lse, dq, dk and dv against fp64 may be
at most MARGIN (1.5) times the error of today's path: the aten
efficient-attention forward and backward on expanded bf16 K/V with the dense
mask (the additive bf16 form SDPA makes of a boolean attn_mask), per-head dk
and dv summed over the group.  The floors are gqa_floors of that file on the
masked P; they take over only where that error is zero, documents of length 1.

Layouts are lists of document lengths, one per batch row:
  [T]               one document: also bit-equal to the plain causal kernels
  [1] * 5           every row sees only itself (both rows: the floors' case)
  [20, 12, 33]      boundaries inside one 32-row wave and one 64-key tile:
                    tiles in which later rows of a wave see nothing
  [64, 64, 64]      boundaries on tile edges, no lower mask anywhere
  [70, 130, 1, 119] a document that spans tiles and starts mid-tile, one of
                    length 1; the last query block's first KV tile is not 0
  [200, 3]          dK/dV's query loop ends early for the first key block

Each case also asserts untouched guards (outputs, delta, doc_start, doc_end),
finite outputs, a bit-equal second run and delta within
2 * 64 eps32 sum |dO O|.  test_maxerr_report prints one MAXERR line per output
(the record is profiles/r20/).
"""
import functools

import pytest
import torch

from attn_bwd_floors import EPS32
from test_gpu_fused_attn import (CANARY_BF16, CANARY_F32, GUARD, MARGIN, SCALE,
                                 _errs, _guarded, _make_qkv, _priority)
from test_gpu_fused_gqa_attn import expand, gqa_floors, group_sum

pytestmark = pytest.mark.gpu

B, HKV = 2, 2
GROUPS = [2, 4, 8]
LAYOUTS = [([17], [17]), ([129], [129]), ([1] * 5, [1] * 5),
           ([20, 12, 33], [33, 20, 12]), ([64, 64, 64], [128, 64]),
           ([70, 130, 1, 119], [119, 1, 130, 70]), ([200, 3], [3, 200])]
OUTPUTS = ("out", "lse", "dq", "dk", "dv")
CANARY_I32 = -77


def _fg():
    from sharedtensor_amd.ops import fused_gqa_attn
    return fused_gqa_attn


def _doc_ids(layout):
    return torch.tensor([[d for d, n in enumerate(row) for _ in range(n)]
                         for row in layout], device="cuda")


def masked_reference(q, k, v, dout, vis, scale):
    """attn_bwd_floors.reference with the mask vis (B, 1, T, T), plus lse."""
    q, k, v = (t.detach().double().requires_grad_() for t in (q, k, v))
    s = ((q @ k.transpose(-1, -2)) * scale).masked_fill(~vis, float("-inf"))
    p = torch.softmax(s, dim=-1)
    out = p @ v
    out.backward(dout.double())
    return dict(out=out.detach(), P=p.detach(), dq=q.grad, dk=k.grad,
                dv=v.grad, lse=torch.logsumexp(s.detach(), dim=-1))


@functools.lru_cache(maxsize=None)
def _case(G, li):
    fg = _fg()
    layout = LAYOUTS[li]
    T, hq = sum(layout[0]), G * HKV
    seed = 5000 * li + 100 * G
    q, k, v = _make_qkv(B, hq, T, "gauss", seed)  # (B, T, hq, 64) fp32
    q, k, v = (t.bfloat16().transpose(1, 2)
               for t in (q, k[:, :, :HKV].contiguous(),
                         v[:, :, :HKV].contiguous()))
    g = torch.Generator(device="cuda").manual_seed(seed + 1)
    dout = torch.randn(B, T, hq, 64, device="cuda",
                       generator=g).bfloat16().transpose(1, 2)
    ids = _doc_ids(layout)
    start, end = fg.doc_start_end(ids)
    vis = ((ids[:, :, None] == ids[:, None, :])
           & torch.ones(T, T, device="cuda", dtype=torch.bool).tril())[:, None]
    ke, ve = expand(k, G), expand(v, G)
    ref = masked_reference(q, ke, ve, dout, vis, SCALE)
    ref["dk"], ref["dv"] = group_sum(ref["dk"], G), group_sum(ref["dv"], G)
    fl = gqa_floors(ref, q, k, v, dout, G, SCALE)
    # today's path: the bias SDPA makes of the mask, last dim padded to 16
    Tp = (T + 15) // 16 * 16
    bias = torch.full((B, 1, T, Tp), float("-inf"), device="cuda",
                      dtype=torch.bfloat16)
    bias[..., :T].masked_fill_(vis, 0.0)
    bias = bias[..., :T].expand(B, hq, T, T)
    with _priority():
        a_out, a_lse, seed_, off = \
            torch.ops.aten._scaled_dot_product_efficient_attention(
                q, ke, ve, bias, True, 0.0, False, scale=SCALE)
        a_dq, a_dk, a_dv, _ = \
            torch.ops.aten._scaled_dot_product_efficient_attention_backward(
                dout, q, ke, ve, bias, a_out, a_lse, seed_, off, 0.0,
                [True, True, True, False], False, scale=SCALE)
    arm = dict(out=a_out, lse=a_lse[..., :T], dq=a_dq, dk=group_sum(a_dk, G),
               dv=group_sum(a_dv, G))

    def run(doc):
        shapes = dict(out=(B, T, hq, 64), dq=(B, T, hq, 64),
                      dk=(B, T, HKV, 64), dv=(B, T, HKV, 64))
        bufs, x = {}, {}
        for n, shp in shapes.items():
            bufs[n], x[n] = _guarded(shp, torch.bfloat16, CANARY_BF16)
        for n in ("lse", "delta"):
            bufs[n], x[n] = _guarded((B, hq, T), torch.float32, CANARY_F32)
        kw = {}
        if doc:
            for n, val in (("doc_start", start), ("doc_end", end)):
                bufs[n], kw[n] = _guarded((B, T), torch.int32, CANARY_I32)
                kw[n].copy_(val)
        fg.gqa_forward(q, k, v, SCALE, out=x["out"], lse=x["lse"],
                       **({"doc_start": kw["doc_start"]} if doc else {}))
        x["out"] = x["out"].transpose(1, 2)
        x["dq"], x["dk"], x["dv"] = fg.gqa_backward(
            q, k, v, x["out"], x["lse"], dout, SCALE,
            *(x[n].transpose(1, 2) for n in ("dq", "dk", "dv")),
            delta=x["delta"], **kw)
        torch.cuda.synchronize()
        return x, bufs

    got, bufs = run(True)
    again, _ = run(True)
    plain = run(False)[0] if len(layout[0]) == len(layout[1]) == 1 else None
    return dict(ref=ref, fl=fl, arm=arm, got=got, again=again, bufs=bufs,
                plain=plain, dout=dout)


def _figures(c, name):
    ref = c["ref"][name]
    f_abs, f_l2 = _errs(c["got"][name], ref)
    a_abs, a_l2 = _errs(c["arm"][name], ref)
    norm = ref.norm().item()
    if norm == 0:  # dq and dk of length-1 documents: no relative figure
        f_l2 = a_l2 = 0.0
    return dict(f_abs=f_abs, f_l2=f_l2, a_abs=a_abs, a_l2=a_l2,
                fl_abs=c["fl"][name].max().item(),
                fl_l2=c["fl"][name].norm().item() / norm if norm else 0.0)


@pytest.mark.parametrize("li", range(len(LAYOUTS)),
                         ids=["-".join(map(str, l[0])) for l in LAYOUTS])
@pytest.mark.parametrize("G", GROUPS)
def test_doc_mask_against_fp64(G, li):
    c = _case(G, li)
    got = c["got"]
    canaries = {torch.bfloat16: CANARY_BF16, torch.float32: CANARY_F32,
                torch.int32: CANARY_I32}
    for n, buf in c["bufs"].items():  # guards untouched
        g = torch.full((GUARD,), canaries[buf.dtype], dtype=buf.dtype,
                       device="cuda")
        assert torch.equal(buf[:GUARD], g) and torch.equal(buf[-GUARD:], g), n
    prod = c["dout"].double() * got["out"].double()
    d_err = (got["delta"].double() - prod.sum(-1)).abs()
    assert (d_err <= 2 * 64 * EPS32 * prod.abs().sum(-1)).all(), d_err.max()
    for name in OUTPUTS + ("delta",):
        assert torch.isfinite(got[name].float()).all(), name
        assert torch.equal(got[name], c["again"][name]), f"{name}: repeat differs"
        if c["plain"] is not None:  # one document: the mask machinery is idle
            assert torch.equal(got[name], c["plain"][name]), f"{name}: != plain"
    for name in OUTPUTS:
        assert got[name].shape == c["ref"][name].shape, name
        f = _figures(c, name)
        print(f"GQADOC G={G} {LAYOUTS[li][0]} {name}: maxabs fused "
              f"{f['f_abs']:.3e} arm {f['a_abs']:.3e} floor {f['fl_abs']:.3e}"
              f" | rel-l2 fused {f['f_l2']:.3e} arm {f['a_l2']:.3e} floor "
              f"{f['fl_l2']:.3e}")
        assert f["f_abs"] <= max(MARGIN * f["a_abs"], f["fl_abs"]), name
        assert f["f_l2"] <= max(MARGIN * f["a_l2"], f["fl_l2"]), name


def test_maxerr_report():
    for name in OUTPUTS:
        w = dict(f_abs=0.0, a_abs=0.0, f_l2=0.0, a_l2=0.0)
        for G in GROUPS:
            for li in range(len(LAYOUTS)):
                f = _figures(_case(G, li), name)
                w = {k: max(w[k], f[k]) for k in w}
        print(f"MAXERR gqa_attn_doc {name}: maxabs fused {w['f_abs']:.3e} "
              f"arm {w['a_abs']:.3e} rel-l2 fused {w['f_l2']:.3e} arm "
              f"{w['a_l2']:.3e}")


def test_autograd_path_and_rejections():
    """fused_causal_gqa_attention(doc_ids=...) is the guarded case's numbers;
    head dim 128 and non-contiguous runs raise."""
    fg = _fg()
    c = _case(4, 3)
    T = sum(LAYOUTS[3][0])
    q, k, v = _make_qkv(B, 4 * HKV, T, "gauss", 5000 * 3 + 400)
    q, k, v = (t.bfloat16().transpose(1, 2).requires_grad_()
               for t in (q, k[:, :, :HKV].contiguous(),
                         v[:, :, :HKV].contiguous()))
    y = fg.fused_causal_gqa_attention(q, k, v, SCALE,
                                      doc_ids=_doc_ids(LAYOUTS[3]))
    y.backward(c["dout"])
    for name, t in (("out", y), ("dq", q.grad), ("dk", k.grad),
                    ("dv", v.grad)):
        assert torch.equal(t, c["got"][name]), name
    mk = lambda *s: torch.zeros(*s, device="cuda", dtype=torch.bfloat16)
    ids = torch.zeros(2, 16, device="cuda", dtype=torch.long)
    with pytest.raises(ValueError):  # head dim 128
        fg.fused_causal_gqa_attention(mk(2, 8, 16, 128), mk(2, 2, 16, 128),
                                      mk(2, 2, 16, 128), doc_ids=ids)
    ids[1, 3], ids[1, 9] = 1, 1  # 0 0 0 1 0 .. 1: runs of 0 and 1 come back
    with pytest.raises(ValueError):
        fg.fused_causal_gqa_attention(mk(2, 8, 16, 64), mk(2, 2, 16, 64),
                                      mk(2, 2, 16, 64), doc_ids=ids)
