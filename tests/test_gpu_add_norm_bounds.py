"""The wave-per-row add+LayerNorm and add+RMSNorm kernels
(csrc/add_ln_kernels.hip, csrc/add_rms_kernels.hip) against the fp64
reference and the derived bounds of tests/kernel_bounds.py: bf16 outputs 1 ulp
+ fp32 slack, mean / rstd the fp32 slack, with the reduction depths of
kb.wave_depths.  No tolerance in this file is a number taken from the kernels'
output.

The raw bindings are called directly.  Every output is filled with a NaN
pattern no kernel writes and sits between guard regions; every call gets its
own NaN-filled partials buffer of max_blocks * NS * C floats, so the reducer
reads nothing the backward kernel did not store in this call.  x_new is held
bit-equal to torch's sum first, and the reference is computed from it, with
fp64 statistics.

Widths: every instantiation (LN C = 256 NV, NV = 1..4; RMS C = 512 NV,
NV = 1..8).  Rows: 1, 2, 3, 5 leave waves of the last block idle, which reach
the combine with zeros; 4 * max_blocks + 3 makes the backward grid loop with
a ragged tail, the last row and the first row of the second sweep carrying 64
times the gradient."""
import functools
import itertools

import pytest
import torch

import kernel_bounds as kb
from sharedtensor_amd import _core
from sharedtensor_amd.ops import fused_ln, fused_rms

pytestmark = pytest.mark.gpu

EPS = kb.EPS
GUARD = 64                      # elements on either side
# NaN patterns no kernel writes (f32_to_bf16 turns every NaN into 0x7FC0)
FILL = {torch.bfloat16: 0x7FC1, torch.float32: 0x7FC00001}
LN_WIDTHS = [256, 512, 768, 1024]
RMS_WIDTHS = list(range(512, 4097, 512))
WIDTHS = {"ln": LN_WIDTHS, "rms": RMS_WIDTHS}
FAMILY_WIDTHS = {"ln": [256, 768, 1024], "rms": [512, 2048, 4096]}
MAX_BLOCKS = {"ln": _core.add_ln_max_blocks(),
              "rms": _core.add_rms_max_blocks()}
RAGGED = {op: 4 * n + 3 for op, n in MAX_BLOCKS.items()}


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Guarded:
    """A poisoned tensor of `shape` with GUARD poisoned elements on either
    side of it."""

    def __init__(self, shape, dtype):
        n = 1
        for s in shape:
            n *= s
        bits = torch.int16 if dtype == torch.bfloat16 else torch.int32
        self.fill = FILL[dtype]
        self.buf = torch.full((GUARD + n + GUARD,), self.fill, dtype=bits,
                              device="cuda")
        self.bits = self.buf[GUARD:GUARD + n]
        self.view = self.bits.view(dtype).view(shape)
        assert self.view.data_ptr() % 16 == 0

    def ptr(self):
        return self.view.data_ptr()

    def margins_intact(self):
        return bool((self.buf[:GUARD] == self.fill).all()
                    and (self.buf[-GUARD:] == self.fill).all())

    def untouched(self):
        return bool((self.buf == self.fill).all())

    def fully_written(self):
        return not bool((self.bits == self.fill).any())


def run(op, x, w, dy, delta=None, dbias=None, b=None, dres=None,
        ddbias=False):
    """One forward and one backward call through the raw bindings.  Returns
    the outputs the calls were given, after checking that exactly those were
    written, in full, that nothing around them and no input was, and that
    the backward kernel stored every partial the reducer read."""
    R, C = x.shape
    bf, f32 = torch.bfloat16, torch.float32
    o = {"x_new": Guarded((R, C), bf), "y": Guarded((R, C), bf),
         "rstd": Guarded((R,), f32), "dx_total": Guarded((R, C), bf),
         "dgamma": Guarded((C,), bf)}
    if op == "ln":
        o.update(mean=Guarded((R,), f32), dbeta=Guarded((C,), bf),
                 ddbias=Guarded((C,), bf))
    ns = 1 if op == "rms" else (3 if ddbias else 2)
    part = Guarded((MAX_BLOCKS[op] * ns * C,), f32)
    ins = [t for t in (x, w, dy, delta, dbias, b, dres) if t is not None]
    before = [t.clone() for t in ins]

    def p(t):
        return t.data_ptr() if t is not None else 0
    xn = o["x_new"].view if delta is not None else x
    s = _stream()
    if op == "ln":
        _core.add_ln_fwd(x.data_ptr(), p(delta), p(dbias), w.data_ptr(), p(b),
                         o["x_new"].ptr() if delta is not None else 0,
                         o["y"].ptr(), o["mean"].ptr(), o["rstd"].ptr(), R, C,
                         EPS, s)
        _core.add_ln_bwd(dy.data_ptr(), xn.data_ptr(), w.data_ptr(),
                         o["mean"].ptr(), o["rstd"].ptr(), p(dres),
                         o["dx_total"].ptr(), o["dgamma"].ptr(),
                         o["dbeta"].ptr(), o["ddbias"].ptr() if ddbias else 0,
                         part.ptr(), R, C, s)
    else:
        assert dbias is None and b is None and not ddbias
        _core.add_rms_fwd(x.data_ptr(), p(delta), w.data_ptr(),
                          o["x_new"].ptr() if delta is not None else 0,
                          o["y"].ptr(), o["rstd"].ptr(), R, C, EPS, s)
        _core.add_rms_bwd(dy.data_ptr(), xn.data_ptr(), w.data_ptr(),
                          o["rstd"].ptr(), p(dres), o["dx_total"].ptr(),
                          o["dgamma"].ptr(), part.ptr(), R, C, s)
    torch.cuda.synchronize()

    absent = set()
    if delta is None:
        absent.add("x_new")
    if op == "ln" and not ddbias:
        absent.add("ddbias")
    for k, g in o.items():
        if k in absent:     # a null pointer: its buffer stays poisoned
            assert g.untouched(), f"{k} was written"
        else:
            assert g.margins_intact(), f"write outside {k}"
            assert g.fully_written(), f"{k} has elements never stored"
    for t, t0 in zip(ins, before):
        assert torch.equal(t.view(torch.int16), t0.view(torch.int16)), \
            "an input changed"
    # partials: whole rows of ns * C floats from the start, one per block of
    # the grid, all finite; the rest is still poison
    assert part.margins_intact(), "write outside the partials"
    stored = part.bits != part.fill
    n = int(stored.sum())
    assert n > 0 and n % (ns * C) == 0 and bool(stored[:n].all()), n
    grid = n // (ns * C)
    assert grid <= min((R + 3) // 4, MAX_BLOCKS[op]), grid
    if R <= 4 * 64:         # fewer rows than any device keeps resident
        assert grid == (R + 3) // 4, grid
    assert bool(torch.isfinite(part.view[:n]).all())
    return {k: g.view for k, g in o.items() if k not in absent}


@functools.lru_cache(maxsize=None)
def _inputs(op, family, R, C):
    """The inputs of kb.add_norm_inputs on the device, shared between the
    tests and never modified."""
    t = kb.add_norm_inputs(op, family, R, C)
    return {k: v.cuda() for k, v in t.items()}


def case(op, family, R, C, delta=False, dbias=False, bias=True, dres=True,
         ddbias=False, sentinel=False):
    """Arguments of run() for one call, and the x_new torch's own sum gives.
    The family's x is the x_new aimed at: with a delta, x = bf16(x_new -
    delta).  `sentinel` scales dy and d_x_new of the last row and of the
    first row of the second sweep by 64."""
    t = _inputs(op, family, R, C)
    w, dy, x = t["w"], t["dy"], t["x"]
    kw = {"ddbias": ddbias}
    if delta and dbias:
        kw.update(delta=t["delta"], dbias=t["dbias"])
        x = (x.float() - t["delta"].float() - t["dbias"].float()).bfloat16()
        x_new = (x.float() + t["delta"].float()
                 + t["dbias"].float()).bfloat16()
    elif delta:
        kw.update(delta=t["delta"])
        x = (x.float() - t["delta"].float()).bfloat16()
        x_new = x + t["delta"]
    else:
        x_new = x
    if family in ("constant", "shifted"):   # the family survives the detour
        assert torch.equal(x_new, t["x"])
    if op == "ln" and bias:
        kw.update(b=t["b"])
    d = kb.add_norm_dres(op, family, x_new, w, dy)
    if sentinel:
        dy, d = dy.clone(), d.clone()
        for r in (R - 1, 4 * MAX_BLOCKS[op]):
            dy[r] *= 64
            d[r] *= 64
    if dres:
        kw.update(dres=d)
    return (op, x, w, dy), kw, x_new


def check(op, family, R, C, label=None, **variant):
    args, kw, x_new = case(op, family, R, C, **variant)
    got = run(*args, **kw)
    if "delta" in kw:
        # one fp32 sum, one round-to-nearest-even: bit for bit torch's
        assert torch.equal(got.pop("x_new"), x_new), "x_new is not x + delta"
    kb.check_add_norm(op, got, x_new, args[2], kw.get("b"), args[3],
                      kw.get("dres"), label or family)
    return got


FULL = {"ln": dict(delta=True, dbias=True, ddbias=True),
        "rms": dict(delta=True)}
OP_WIDTHS = [(op, C) for op in ("ln", "rms") for C in WIDTHS[op]]


@pytest.mark.parametrize("op,C", OP_WIDTHS)
@pytest.mark.parametrize("R", [1, 2, 3, 5])
def test_widths_and_idle_waves(R, op, C):
    check(op, "randn2", R, C, **FULL[op])


@pytest.mark.parametrize("op,C", [(op, C) for op in ("ln", "rms")
                                  for C in FAMILY_WIDTHS[op]])
@pytest.mark.parametrize("family", kb.ADD_NORM_FAMILIES)
def test_input_families(family, op, C):
    check(op, family, 5, C, **FULL[op])
    check(op, family, 5, C, ddbias=(op == "ln"))    # x_new is x itself


@pytest.mark.parametrize("op,C", [("ln", 256), ("ln", 1024), ("rms", 512),
                                  ("rms", 2048), ("rms", 4096)])
def test_row_loop_with_ragged_tail(op, C):
    check(op, "randn2", RAGGED[op], C, label="sentinel", sentinel=True,
          **FULL[op])


LN_VARIANTS = [dict(delta=d, dbias=db, bias=b, dres=r, ddbias=dd)
               for d, db, b, r, dd in itertools.product((False, True),
                                                        repeat=5)
               if d or not db]          # delta_bias needs a delta
RMS_VARIANTS = [dict(delta=d, dres=r)
                for d, r in itertools.product((False, True), repeat=2)]


def _vid(v):
    return "+".join(k for k, on in v.items() if on) or "none"


@pytest.mark.parametrize("v", LN_VARIANTS, ids=_vid)
@pytest.mark.parametrize("R", [5, RAGGED["ln"]])
def test_ln_pointer_variants(R, v):
    check("ln", "randn2", R, 768, label="variants", sentinel=R > 5, **v)


@pytest.mark.parametrize("v", RMS_VARIANTS, ids=_vid)
@pytest.mark.parametrize("R", [5, RAGGED["rms"]])
def test_rms_pointer_variants(R, v):
    check("rms", "randn2", R, 2048, label="variants", sentinel=R > 5, **v)


@pytest.mark.parametrize("R,C", [(5, 256), (5, 768), (5, 1024),
                                 (RAGGED["ln"], 256), (RAGGED["ln"], 1024)])
def test_dbeta_exact_on_integer_dy(R, C):
    """Integer dy in [-4, 4], in at most 32 rows: every partial sum is an
    integer of at most 128 in magnitude, exact in fp32 in any order and
    exact in bf16's 8 bits, so dbeta is the fp64 column sum bit for bit."""
    (op, x, w, _), kw, _ = case("ln", "randn2", R, C, ddbias=True)
    g = torch.Generator().manual_seed(R + C)
    dy = torch.zeros(R, C)
    rows = torch.arange(R) if R <= 32 else torch.cat([
        torch.tensor([0, 1, 4 * MAX_BLOCKS["ln"] - 1, 4 * MAX_BLOCKS["ln"],
                      R - 2, R - 1]),
        torch.randperm(R - 2, generator=g)[:26] + 1]).unique()
    assert rows.numel() <= 32
    dy[rows] = torch.randint(-4, 5, (rows.numel(), C), generator=g).float()
    dy = dy.bfloat16().cuda()
    want = dy.double().sum(0)
    assert float(want.abs().max()) <= 128
    got = run(op, x, w, dy, **kw)
    assert torch.equal(got["dbeta"].double(), want)


@pytest.mark.parametrize("op,R,C", [("ln", 5, 768), ("rms", 5, 2048),
                                    ("ln", RAGGED["ln"], 1024),
                                    ("rms", RAGGED["rms"], 4096)])
def test_two_runs_are_bit_equal(op, R, C):
    args, kw, _ = case(op, "randn2", R, C, sentinel=R > 5, **FULL[op])
    a, c = run(*args, **kw), run(*args, **kw)
    assert a.keys() == c.keys()
    for k in a:
        bits = torch.int16 if a[k].dtype == torch.bfloat16 else torch.int32
        assert torch.equal(a[k].view(bits), c[k].view(bits)), k


# ------------------------------------------------------- through the ops

def test_fused_layer_norm_takes_the_wave_kernels():
    C = 768
    assert _core.add_ln_supported(C)
    t = _inputs("ln", "randn2", 5, C)
    for b in (t["b"], None):
        kb.check_ln_wrapper(fused_ln.fused_layer_norm, t["x"], t["w"], b,
                            t["dy"], "op/delta=None",
                            depth=kb.wave_depths("ln", C))
    x_new, _ = fused_ln.fused_add_layer_norm(t["x"], None, t["w"], t["b"],
                                             EPS)
    assert x_new is t["x"]


def test_fused_rms_norm_without_delta():
    """delta = None hands a supported width to the block-per-row kernels;
    the wave depth is the wider of the two bounds at this width."""
    C = 2048
    assert _core.add_rms_supported(C)
    assert kb.wave_depths("rms", C)["var"] >= kb.n_red(C)
    t = _inputs("rms", "randn2", 5, C)

    def op(x, w, eps):
        x_new, y = fused_rms.fused_add_rms_norm(x, None, w, eps)
        assert x_new is x
        return y
    kb.check_rms_wrapper(op, t["x"], t["w"], t["dy"], "op/delta=None",
                         depth=kb.wave_depths("rms", C))


@pytest.mark.parametrize("op,C,dbias", [("ln", 768, False), ("ln", 768, True),
                                        ("rms", 2048, False)])
@pytest.mark.parametrize("R", [5, 261])
def test_fused_add_ops_with_autograd(R, op, C, dbias):
    """A mis-wired pointer in the Python layer: every gradient the Function
    returns against the reference, delta_bias included."""
    (_, x, w, dy), kw, want = case(op, "randn2", R, C, delta=True,
                                   dbias=dbias)
    leaf = {k: v.clone().requires_grad_(True)
            for k, v in dict(x=x, w=w, **{k: kw[k] for k in
                                          ("delta", "dbias", "b")
                                          if k in kw}).items()}
    if op == "ln":
        x_new, y = fused_ln.fused_add_layer_norm(
            leaf["x"], leaf["delta"], leaf["w"], leaf["b"], EPS,
            leaf.get("dbias"))
    else:
        x_new, y = fused_rms.fused_add_rms_norm(leaf["x"], leaf["delta"],
                                                leaf["w"], EPS)
    assert torch.equal(x_new, want)
    torch.autograd.backward([y, x_new], [dy, kw["dres"]])
    torch.cuda.synchronize()
    assert torch.equal(leaf["x"].grad, leaf["delta"].grad)
    got = {"y": y.detach(), "dx_total": leaf["x"].grad,
           "dgamma": leaf["w"].grad}
    if op == "ln":
        got["dbeta"] = leaf["b"].grad
    if dbias:
        got["ddbias"] = leaf["dbias"].grad
    kb.check_add_norm(op, got, want, w, kw.get("b"), dy, kw["dres"],
                      "op/autograd")
