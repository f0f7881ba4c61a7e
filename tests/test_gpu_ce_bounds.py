"""The fused cross-entropy kernels (csrc/ce_kernels.hip, all row policies)
through their raw bindings, against the fp64 reference and the derived bound
of tests/kernel_bounds.py: dlogits within 1 bf16 ulp + slack element by
element, per-row loss / row_lse within the fp32 slack, row_m exact.

Every output buffer is pre-filled with a sentinel (a NaN with payload 1 for
fp32, 0x7FC1 for dlogits) and sits inside a larger guard buffer: an element
the kernel did not write still holds the sentinel, a write outside the
matrix changes a margin, a read outside drags 1e30 into a row.

Cases and the branches they reach:

  test_kernels_meet_bound
      V in {1, 7, 8, 13, 1003, 8197, 50257, 57344}: k_ce_fwd_grad<1024, 7>
      (V < 8: edge elements only; 8197: first row with a second chunk slot;
      57344: all seven slots full); V in {57345, 131072}, R = 3:
      k_ce_fwd_grad<1024, 16>.  Offsets (logits, dlogits) from a 16-byte
      boundary (0,0) (3,3) (5,5): ce_store8 aligned; (3,5) (0,3):
      element-wise.  The same inputs through k_ce_fwd<256> and, with
      SHTENS_CE_BLOCK=512, k_ce_fwd<512> (row_m exact, lse and loss within
      bound and within the two slacks of the one-pass values), through
      k_ce_bwd<256|512, false> at g = 1 (bit-equal to the one-pass buffer)
      and through the option kernels with nothing ignored and EXTRA off
      (bit-equal to the plain kernels).
  test_two_pass_beyond_the_register_capacity
      V = 131073: one-pass launcher refuses, k_ce_fwd / k_ce_bwd run.
  test_backward_unroll_seam
      nbody in {767, 768, 769, 1024, 1324}, V aligned and odd: no thread /
      thread 0 only / every thread in the 4-way loop, with and without the
      remainder loop; g in {1, 2, 0.37, 0, -1}; row_lse an input.
      test_backward_unroll_seam_block_512: the same seam of k_ce_bwd<512>.
  test_skip_if_unit_strided_rows
      R = 2053 > the capped grid (2048 blocks; 1024 with the 512 knob): rows
      past the first sweep go through r += gridDim.x of
      k_ce_bwd<., true, plain | masked | masked + extra>, ignored
      rows among them; g = 2 within bound, g = 1 leaves the sentinel.
  test_options
      {ignore}, {eps}, {z}, {ignore, eps, z} x V in {13, 1003, 50257} over
      k_ce_fwd_grad, k_ce_fwd and k_ce_bwd with the masked policies (EXTRA
      off and on); the three row kinds (valid, ignored, out of range);
      ignored rows poisoned with NaN and 1e30 against zeros, bitwise.
  test_scan_state
      k_ce_opts_scan counts and inv_count for R around its 1024 threads.
  test_row_isolation
      a NaN / +inf row touches no other row.
  test_wrapper_mean
      fused_cross_entropy's scalar and gradient per path.

The plain (option-free) kernels do not validate targets, so no case feeds
them one out of range.
"""
import numpy as np
import pytest
import torch

import kernel_bounds as kb
from sharedtensor_amd import _core
from sharedtensor_amd.ops import fused_ce

pytestmark = pytest.mark.gpu

MAX_V = _core.ce_fwd_grad_max_v()  # largest V the one-pass kernel takes
MID_V = 1024 * 7 * 8               # last V of the 7-chunk instantiation
GUARD = 64                         # elements on either side
D_SENTINEL = 0x7FC1                # a bf16 NaN no kernel writes
F_SENTINEL = 0x7FC00001            # an fp32 NaN no kernel writes
IGN = -100
EPS, Z = 0.1, 1e-4


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits16(v):
    return int(torch.tensor(v).to(torch.bfloat16).view(torch.int16))


class Guarded:
    """n elements at `off` elements past a 16-byte boundary inside a buffer
    with GUARD elements of `fill` bits on either side (and in the view)."""

    def __init__(self, n, off, fill, dtype):
        bits = torch.int16 if dtype == torch.bfloat16 else torch.int32
        self.buf = torch.full((GUARD + 8 + n + GUARD,), fill, dtype=bits,
                              device="cuda")
        assert self.buf.data_ptr() % 16 == 0 and (GUARD * 2) % 16 == 0
        self.lo, self.hi, self.fill = GUARD + off, GUARD + off + n, fill
        self.view = self.buf[self.lo:self.hi].view(dtype)

    def margins_intact(self):
        return bool((self.buf[:self.lo] == self.fill).all()
                    and (self.buf[self.hi:] == self.fill).all())

    def untouched(self):
        return bool((self.buf == self.fill).all())

    def fully_written(self):
        return not bool((self.buf[self.lo:self.hi] == self.fill).any())


class Case:
    """bf16 logits in a 1e30-filled guard buffer, int32 targets."""

    def __init__(self, x, t, off_x=0):
        self.R, self.V = x.shape
        self.g = Guarded(x.numel(), off_x, _bits16(1e30), torch.bfloat16)
        self.x = self.g.view.view(self.R, self.V)
        self.x.copy_(x.cuda())
        self.before = self.g.buf.clone()
        self.t64 = t.cuda()
        self.t = self.t64.to(torch.int32)

    def outputs(self, names, off_d=None):
        out = {k: Guarded(self.R, 0, F_SENTINEL, torch.float32)
               for k in names}
        if off_d is not None:
            out["dlogits"] = Guarded(self.R * self.V, off_d, D_SENTINEL,
                                     torch.bfloat16)
        return out

    def finish(self, out, written=True):
        torch.cuda.synchronize()
        assert torch.equal(self.g.buf, self.before), "logits changed"
        res = {}
        for k, gd in out.items():
            assert gd.margins_intact(), f"{k}: write outside the buffer"
            if written:
                assert gd.fully_written(), f"{k}: elements left unwritten"
            else:
                assert gd.untouched(), f"{k}: written although g == 1"
            v = gd.view.clone()
            res[k] = v.view(self.R, self.V) if k == "dlogits" else v
        return res


def _kopts(o):
    ii = o.get("ignore_index")
    return dict(ignore_index=0 if ii is None else ii, has_ignore=ii is not None,
                label_smoothing=o.get("eps", 0.0), z_loss=o.get("z", 0.0))


def _scan(c, o):
    k = _kopts(o)
    state = torch.full((_core.CE_OPT_STATE_BYTES // 4,), float("nan"),
                       device="cuda")
    _core.ce_opts_scan(c.t.data_ptr(), c.R, c.V, k["ignore_index"],
                       k["has_ignore"], state.data_ptr(), _stream())
    return state


def fwd_grad(c, off_d=0, opts=None):
    out = c.outputs(("loss", "lse"), off_d)
    p = {k: g.view.data_ptr() for k, g in out.items()}
    if opts is None:
        _core.ce_fwd_grad(c.x.data_ptr(), c.t.data_ptr(), p["loss"], p["lse"],
                          p["dlogits"], 1.0 / c.R, c.R, c.V, _stream())
    else:
        state = _scan(c, opts)
        _core.ce_opts_fwd_grad(c.x.data_ptr(), c.t.data_ptr(), p["loss"],
                               p["lse"], p["dlogits"], state.data_ptr(), c.R,
                               c.V, stream=_stream(), **_kopts(opts))
    return c.finish(out)


def fwd(c, opts=None):
    out = c.outputs(("loss", "lse") + (("m",) if opts is None else ()))
    p = {k: g.view.data_ptr() for k, g in out.items()}
    if opts is None:
        _core.ce_fwd(c.x.data_ptr(), c.t.data_ptr(), p["loss"], p["m"],
                     p["lse"], c.R, c.V, _stream())
    else:
        _core.ce_opts_fwd(c.x.data_ptr(), c.t.data_ptr(), p["loss"], p["lse"],
                          c.R, c.V, stream=_stream(), **_kopts(opts))
    return c.finish(out)


def bwd(c, row_lse, g, off_d=0, opts=None, skip=False, written=True):
    out = c.outputs((), off_d)
    gdev = torch.tensor([g], dtype=torch.float32, device="cuda")
    lse = row_lse.contiguous()
    d = out["dlogits"].view.data_ptr()
    if opts is None:
        _core.ce_bwd(c.x.data_ptr(), c.t.data_ptr(), lse.data_ptr(), d,
                     gdev.data_ptr(), 1.0 / c.R, c.R, c.V, _stream(),
                     skip_if_unit=skip)
    else:
        state = _scan(c, opts)
        _core.ce_opts_bwd(c.x.data_ptr(), c.t.data_ptr(), lse.data_ptr(), d,
                          gdev.data_ptr(), state.data_ptr(), c.R, c.V,
                          stream=_stream(), skip_if_unit=skip, **_kopts(opts))
    return c.finish(out, written)["dlogits"]


def _same_bits(a, b):
    bits = torch.int16 if a.element_size() == 2 else torch.int32
    return torch.equal(a.contiguous().view(bits), b.contiguous().view(bits))


def _nchunk(V):
    return 7 if V <= MID_V else 16


def _agree(a, b, sa, sb, op, out, family):
    """Two kernels' fp32 values of one quantity: within the sum of their
    slacks (each is within its own of the exact value)."""
    fin = torch.isfinite(b)
    kb.assert_f32(a[fin], b[fin].double(),
                  (sa + sb)[fin] + kb.U * b[fin].double().abs(), op, out,
                  family)


# ------------------------------------------------------- plain kernels

_OFFS = [(0, 0), (3, 3), (5, 5), (3, 5), (0, 3)]
_CASES = ([(V, f) for V in (13, 1003) for f in kb.CE_FAMILIES]
          + [(50257, f) for f in ("randn3", "masked", "peaked_target",
                                  "peaked_other")]
          + [(V, "randn3") for V in (1, 7, 8, 8 * 1024 + 5, MID_V,
                                     MID_V + 1, MAX_V)]
          + [(MAX_V, "masked")])
_CASES = [(V, f) + _OFFS[i % len(_OFFS)] for i, (V, f) in enumerate(_CASES)]
_CASES += [(1003, "randn3", 3, 5), (50257, "randn3", 5, 3),
           (50257, "randn3", 3, 3)]


@pytest.mark.parametrize("V,family,off_x,off_d", _CASES)
def test_kernels_meet_bound(monkeypatch, V, family, off_x, off_d):
    R = 3 if V > MID_V else (9 if V == 1003 else 8)
    x, t = kb.ce_inputs(family, R, V, offset=off_x)
    c = Case(x, t, off_x)
    nc = _nchunk(V)

    one = fwd_grad(c, off_d)
    _, s1 = kb.ce_check(one, c.x, c.t64, f"ce_fwd_grad<{nc}>", family,
                        BLK=1024, NCHUNK=nc)

    for blk in (256, 512):
        if blk == 512:
            monkeypatch.setenv("SHTENS_CE_BLOCK", "512")
        two = fwd(c)
        _, s2 = kb.ce_check(two, c.x, c.t64, f"ce_fwd<{blk}>", family,
                            BLK=blk)
        for k in ("lse", "loss"):
            _agree(two[k], one[k], s2[k], s1[k], f"ce_fwd<{blk}>-vs-onepass",
                   k, family)
        # same row_lse, same formula: bit for bit
        d1 = bwd(c, one["lse"], 1.0, off_d)
        assert _same_bits(d1, one["dlogits"]), f"ce_bwd<{blk}> g=1"
    monkeypatch.delenv("SHTENS_CE_BLOCK")

    # option kernels, nothing ignored, EXTRA off: the plain chain exactly
    o = dict(ignore_index=IGN)
    one_o = fwd_grad(c, off_d, o)
    two, two_o = fwd(c), fwd(c, o)
    for k in ("loss", "lse", "dlogits"):
        assert _same_bits(one_o[k], one[k]), f"ce_opts_fwd_grad {k}"
    for k in ("loss", "lse"):
        assert _same_bits(two_o[k], two[k]), f"ce_opts_fwd {k}"
    assert _same_bits(bwd(c, one["lse"], 0.37, off_d, o),
                      bwd(c, one["lse"], 0.37, off_d)), "ce_opts_bwd"


@pytest.mark.parametrize("blk", [256, 512])
def test_two_pass_beyond_the_register_capacity(monkeypatch, blk):
    if blk == 512:
        monkeypatch.setenv("SHTENS_CE_BLOCK", "512")
    R, V = 3, MAX_V + 1
    x, t = kb.ce_inputs("randn3", R, V)
    c = Case(x, t)
    out = c.outputs(("loss", "lse"), 0)
    p = {k: g.view.data_ptr() for k, g in out.items()}
    with pytest.raises(RuntimeError):
        _core.ce_fwd_grad(c.x.data_ptr(), c.t.data_ptr(), p["loss"], p["lse"],
                          p["dlogits"], 1.0 / R, R, V, _stream())
    c.finish(out, written=False)
    two = fwd(c)
    kb.ce_check(two, c.x, c.t64, f"ce_fwd<{blk}>", "randn3/V=max+1", BLK=blk)
    for g in (1.0, 0.37):
        d = bwd(c, two["lse"], g)
        kb.ce_check({"dlogits": d}, c.x, c.t64, f"ce_bwd<{blk}>",
                    "randn3/V=max+1", g=g, lse=two["lse"])
    two_o = fwd(c, dict(eps=EPS, z=Z))
    kb.ce_check(two_o, c.x, c.t64, "ce_opts_fwd<256,extra>", "randn3/V=max+1",
                eps=EPS, z=Z, BLK=256)


GS = [1.0, 2.0, 0.37, 0.0, -1.0]


def _seam_case(V, blk):
    R = 8
    x, t = kb.ce_inputs("randn3", R, V)
    c = Case(x, t)
    ref = kb.ce_formula(c.x, c.t64)
    row_lse = ref["lse"].float()     # the fp32-rounded reference lse
    for g in GS:
        d = bwd(c, row_lse, g)
        kb.ce_check({"dlogits": d}, c.x, c.t64, f"ce_bwd<{blk}>",
                    f"seam/g={g:g}", g=g, lse=row_lse)
    one = fwd_grad(c)
    assert _same_bits(bwd(c, one["lse"], 1.0), one["dlogits"])
    o = dict(ignore_index=IGN, eps=EPS, z=Z)
    d = bwd(c, row_lse, 0.37, opts=o)
    kb.ce_check({"dlogits": d}, c.x, c.t64, "ce_opts_bwd<256,extra>",
                "seam/g=0.37", g=0.37, lse=row_lse, **o)


@pytest.mark.parametrize("odd", [0, 3], ids=["aligned", "odd"])
@pytest.mark.parametrize("nbody", [767, 768, 769, 1024, 1024 + 300])
def test_backward_unroll_seam(nbody, odd):
    _seam_case(8 * nbody + odd, 256)


def test_backward_unroll_seam_block_512(monkeypatch):
    monkeypatch.setenv("SHTENS_CE_BLOCK", "512")
    _seam_case(8 * (3 * 512 + 1 + 300) + 5, 512)


@pytest.mark.parametrize("kind", ["plain", "plain512", "ignore", "all"])
@pytest.mark.parametrize("V", [13, 1003])
def test_skip_if_unit_strided_rows(monkeypatch, V, kind):
    R = 2048 + 5
    x, t = kb.ce_inputs("randn3", R, V)
    opts = None
    if kind == "plain512":
        monkeypatch.setenv("SHTENS_CE_BLOCK", "512")
    elif kind != "plain":
        t = t.clone()
        t[5::7] = IGN
        t[2049] = t[R - 1] = IGN     # in the strided part
        opts = dict(ignore_index=IGN)
        if kind == "all":
            opts.update(eps=EPS, z=Z)
    kw = opts or {}
    c = Case(x, t)
    one = fwd_grad(c, 0, opts)
    kb.ce_check(one, c.x, c.t64, f"ce_fwd_grad/{kind}", "R=2053",
                BLK=1024, NCHUNK=7, **kw)
    d2 = bwd(c, one["lse"], 2.0, opts=opts, skip=True)
    kb.ce_check({"dlogits": d2}, c.x, c.t64, f"ce_bwd<skip>/{kind}",
                "R=2053/g=2", g=2.0, lse=one["lse"], **kw)
    # the rows of the second sweep on their own
    assert bool((d2[2048:].float().abs().sum(-1) > 0)[
        kb.ce_formula(c.x, c.t64, **kw)["valid"][2048:]].all())
    bwd(c, one["lse"], 1.0, opts=opts, skip=True, written=False)


# ----------------------------------------------------------- options

OPTION_SETS = {
    "ignore": dict(ignore_index=IGN),
    "eps": dict(eps=EPS),
    "z": dict(z=Z),
    "all": dict(ignore_index=IGN, eps=EPS, z=Z),
}
MASKS = ["none", "first", "last", "alternating", "all_but_one", "all"]


def _mask_rows(R, pattern):
    m = torch.zeros(R, dtype=torch.bool)
    if pattern == "first":
        m[0] = True
    elif pattern == "last":
        m[-1] = True
    elif pattern == "alternating":
        m[::2] = True
    elif pattern == "all_but_one":
        m[:] = True
        m[R // 2] = False
    elif pattern == "all":
        m[:] = True
    return m


def _run_opts(x, t, o, label, judge=True):
    c = Case(x, t)
    extra = "extra" if (o.get("eps") or o.get("z")) else "plain"
    one = fwd_grad(c, 0, o)
    two = fwd(c, o)
    d = bwd(c, one["lse"], 0.37, opts=o)
    if judge:
        kb.ce_check(one, c.x, c.t64, f"ce_opts_fwd_grad<7,{extra}>", label,
                    BLK=1024, NCHUNK=7, **o)
        kb.ce_check(two, c.x, c.t64, f"ce_opts_fwd<256,{extra}>", label,
                    BLK=256, **o)
        kb.ce_check({"dlogits": d}, c.x, c.t64, f"ce_opts_bwd<256,{extra}>",
                    label, g=0.37, lse=one["lse"], **o)
    return dict(one, loss2=two["loss"], lse2=two["lse"], d037=d)


@pytest.mark.parametrize("V", [13, 1003, 50257])
@pytest.mark.parametrize("name", OPTION_SETS.keys())
def test_options(name, V):
    o = OPTION_SETS[name]
    R = 8
    x, seam = kb.ce_inputs("randn3", R, V)
    has_ignore = "ignore_index" in o
    for pattern in (MASKS if has_ignore else ["none"]):
        masked = _mask_rows(R, pattern)
        t = torch.where(masked, torch.full_like(seam, IGN), seam)
        zeros = x.clone()
        zeros[masked] = 0.0
        base = _run_opts(zeros, t, o, f"{name}/{pattern}")
        if pattern == "all":
            assert kb.is_plus_zero(base["dlogits"])
            assert kb.is_plus_zero(base["loss"])
        for fill in (float("nan"), 1e30):
            if not masked.any():
                break
            poisoned = x.clone()
            poisoned[masked] = fill
            got = _run_opts(poisoned, t, o, f"{name}/{pattern}", judge=False)
            for k, v in got.items():
                assert _same_bits(v, base[k]), (pattern, fill, k)
    if has_ignore:
        # out of range and not ignored: loss NaN, +0 gradient row; and an
        # ignore_index inside the vocabulary
        t = seam.clone()
        t[0] = IGN
        t[1], t[R - 2] = V, -5
        got = _run_opts(x, t, o, f"{name}/out-of-range")
        assert torch.isnan(got["loss"][[1, R - 2]]).all()
        assert torch.isnan(got["loss2"][[1, R - 2]]).all()
        inside = dict(o, ignore_index=int(seam[2]))
        got = _run_opts(x, seam, inside, f"{name}/ignore-inside")
        assert kb.is_plus_zero(got["dlogits"][2]) and got["loss"][2] == 0


@pytest.mark.parametrize("inside", [False, True], ids=["outside", "inside"])
@pytest.mark.parametrize("R", [1, 1023, 1024, 1025, 70001])
def test_scan_state(R, inside):
    V = 50
    ign = 7 if inside else IGN
    g = torch.Generator().manual_seed(R)
    t = torch.randint(-3, V + 3, (R,), generator=g)  # bad ones of both signs
    t[torch.rand(R, generator=g) < 0.3] = ign
    for has_ignore, tt in ((True, t), (False, t),
                           (True, torch.full((R,), ign))):
        state = torch.full((4,), float("nan"), device="cuda")
        _core.ce_opts_scan(tt.to(torch.int32).cuda().data_ptr(), R, V, ign,
                           has_ignore, state.data_ptr(), _stream())
        torch.cuda.synchronize()
        ignored = (tt == ign) if has_ignore else torch.zeros(R, dtype=bool)
        in_range = (tt >= 0) & (tt < V)
        n_valid = int((in_range & ~ignored).sum())
        n_bad = int((~in_range & ~ignored).sum())
        ints = state.view(torch.int32).cpu().numpy()
        assert (int(ints[1]), int(ints[2]), int(ints[3])) == (n_valid, n_bad, 0)
        with np.errstate(divide="ignore"):
            want = np.float32(1) / np.float32(n_valid)
        assert ints[0] == want.view(np.int32), (state[0].item(), want)
        if n_valid == 0:
            assert state[0].item() == float("inf")


@pytest.mark.parametrize("fill", [float("nan"), float("inf")])
def test_row_isolation(fill):
    R, V = 9, 1003
    x, t = kb.ce_inputs("randn3", R, V)
    dirty = x.clone()
    dirty[4, 517] = fill
    others = torch.arange(R) != 4
    for o in (None, dict(ignore_index=IGN, eps=EPS, z=Z)):
        ca, cb = Case(x, t), Case(dirty, t)
        for run in (lambda c: fwd_grad(c, 0, o), lambda c: fwd(c, o)):
            a, b = run(ca), run(cb)
            assert torch.isnan(b["loss"][4])
            for k in a:
                assert _same_bits(a[k][others], b[k][others]), (fill, k)


@pytest.mark.parametrize("R,V", [(9, 1003), (8, 50257)])
@pytest.mark.parametrize("onepass", ["1", "0"])
@pytest.mark.parametrize("name", ["plain", "all"])
def test_wrapper_mean(monkeypatch, name, onepass, R, V):
    monkeypatch.setenv("SHTENS_CE_ONEPASS", onepass)
    x, t = kb.ce_inputs("randn3", R, V)
    o, kw = {}, {}
    if name == "all":
        t = t.clone()
        t[1::3] = IGN
        o = OPTION_SETS["all"]
        kw = dict(ignore_index=IGN, label_smoothing=EPS, z_loss=Z)
    lf = x.cuda().requires_grad_(True)
    loss = fused_ce.fused_cross_entropy(lf, t.cuda(), **kw)
    (loss * 0.37).backward()
    torch.cuda.synchronize()
    assert loss.dtype == torch.float32
    kb.ce_check({"mean": loss.detach()}, x.cuda(), t.cuda(),
                f"fused_cross_entropy/{name}/onepass={onepass}", "randn3", **o)
    # the gradient comes from the kernel's own row_lse: one-pass layout's
    # slack on lse bounds the two-pass one only from below, so the deepest
    kb.ce_check({"dlogits": lf.grad}, x.cuda(), t.cuda(),
                f"fused_cross_entropy/{name}/onepass={onepass}", "randn3",
                g=0.37, **o)
