"""Fused cross-entropy with ignore_index, label smoothing and z-loss
(csrc/ce_kernels.hip) against cross_entropy_reference on the same bf16
logits upcast to fp32.

Shapes and seam targets are those of test_gpu_fused_ce_onepass.py: every
16-byte phase, rows shorter than a chunk, both register instantiations and
the two-kernel fallback beyond the register capacity.
"""
import dataclasses

import pytest
import torch

import kernel_bounds as kb
from sharedtensor_amd import _core
from sharedtensor_amd.ops import fused_ce
from sharedtensor_amd.ops.fused_ce import cross_entropy_reference

pytestmark = pytest.mark.gpu

LOSS_TOL = dict(rtol=2e-3, atol=2e-3)
GRAD_TOL = dict(rtol=5e-2, atol=1e-4)

MAX_V = _core.ce_fwd_grad_max_v()  # largest V the one-pass kernel takes
MID_V = 1024 * 7 * 8               # last V of the 7-chunk instantiation

SHAPES = [(16, 50257), (7, 13), (8, 1024), (5, 1000), (4, MID_V + 1),
          (4, MAX_V + 1)]
MASKS = ["none", "first", "last", "alternating", "all_but_one", "all"]
OPTION_SETS = {
    "mask": dict(),
    "smooth": dict(label_smoothing=0.1),
    "z": dict(z_loss=0.1),                      # 2*z*lse is of order 2
    "all": dict(label_smoothing=0.1, z_loss=0.1),
}


def _seam_targets(R, V, offset=0):
    """Targets at element 0, at V-1, in a head and in a tail element of rows
    that have one (`offset` = element offset of the matrix from a 16-byte
    boundary); random elsewhere."""
    return kb.seam_targets(R, V, offset).cuda()


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
    return m.cuda()


def _logits(R, V, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(R, V, device="cuda", generator=g) * 3).to(torch.bfloat16)


def _reference(logits, targets, **opts):
    lt = logits.detach().clone().requires_grad_(True)
    loss = cross_entropy_reference(lt.float(), targets, **opts)
    loss.backward()
    return loss.detach(), lt.grad.float()


def _fused(logits, targets, scale=None, **opts):
    lf = logits.detach().requires_grad_(True)  # same storage and offset
    loss = fused_ce.fused_cross_entropy(lf, targets, **opts)
    (loss if scale is None else loss * scale).backward()
    torch.cuda.synchronize()
    return loss.detach(), lf.grad


def _is_plus_zero(t):
    return not bool(t.contiguous().view(torch.int16).any())


def _check(logits, targets, **opts):
    loss_t, grad_t = _reference(logits, targets, **opts)
    loss_f, grad_f = _fused(logits, targets, **opts)
    print(f"loss fused {loss_f.item():.6f} ref {loss_t.item():.6f} "
          f"max |dgrad| {(grad_f.float() - grad_t).abs().max().item():.3e}")
    torch.testing.assert_close(loss_f.float(), loss_t, equal_nan=True,
                               **LOSS_TOL)
    torch.testing.assert_close(grad_f.float(), grad_t, **GRAD_TOL)
    # element by element: 1 bf16 ulp + slack against the fp64 reference
    kb.ce_check({"mean": loss_f, "dlogits": grad_f}, logits, targets,
                "fused_cross_entropy/opts", f"V={logits.shape[1]}",
                ignore_index=opts.get("ignore_index"),
                eps=opts.get("label_smoothing", 0.0),
                z=opts.get("z_loss", 0.0))
    return loss_f, grad_f


@pytest.mark.parametrize("opts", OPTION_SETS.values(), ids=OPTION_SETS.keys())
@pytest.mark.parametrize("R,V", SHAPES)
def test_matches_reference(R, V, opts):
    logits = _logits(R, V, R + V)
    seam = _seam_targets(R, V)
    for pattern in MASKS:
        masked = _mask_rows(R, pattern)
        targets = torch.where(masked, torch.full_like(seam, -100), seam)
        assert targets.dtype == torch.int64
        loss, grad = _check(logits, targets, ignore_index=-100, **opts)
        assert _is_plus_zero(grad[masked]), pattern
        if pattern == "all":
            assert torch.isnan(loss) and _is_plus_zero(grad)
        else:
            assert torch.isfinite(loss), pattern


@pytest.mark.parametrize("opts", OPTION_SETS.values(), ids=OPTION_SETS.keys())
def test_ignore_index_inside_the_vocabulary(opts):
    R, V = 16, 50257
    logits = _logits(R, V, 3)
    targets = _seam_targets(R, V)
    targets[5] = 0
    masked = targets == 0
    assert int(masked.sum()) >= 2  # the seam target at element 0, and row 5
    _, grad = _check(logits, targets, ignore_index=0, **opts)
    assert _is_plus_zero(grad[masked])


@pytest.mark.parametrize("pattern", ["none", "alternating"])
@pytest.mark.parametrize("z", [0.0, 0.1])
def test_smoothing_term_at_a_small_vocabulary(pattern, z):
    # eps/V = 0.5/13 ~ 0.04 per element before the 1/n_valid, two orders of
    # magnitude above the gradient atol: a dropped -eps/V term fails here
    # (at V = 50257 it is below atol by construction)
    R, V = 7, 13
    logits = _logits(R, V, 17)
    masked = _mask_rows(R, pattern)
    seam = _seam_targets(R, V)
    targets = torch.where(masked, torch.full_like(seam, -100), seam)
    _check(logits, targets, ignore_index=-100, label_smoothing=0.5, z_loss=z)


@pytest.mark.parametrize("opts", [OPTION_SETS["mask"], OPTION_SETS["all"]],
                         ids=["mask", "all"])
@pytest.mark.parametrize("onepass", ["1", "0"])
def test_masked_rows_are_never_read(monkeypatch, onepass, opts):
    monkeypatch.setenv("SHTENS_CE_ONEPASS", onepass)
    R, V = 9, 1003
    logits = _logits(R, V, 11)
    masked = _mask_rows(R, "alternating")
    seam = _seam_targets(R, V)
    targets = torch.where(masked, torch.full_like(seam, -100), seam)
    loss, grad = _check(logits, targets, ignore_index=-100, **opts)
    for fill in (float("nan"), 1e30):
        poisoned = logits.clone()
        poisoned[masked] = fill
        loss_p, grad_p = _fused(poisoned, targets, ignore_index=-100, **opts)
        assert torch.equal(loss_p, loss), fill
        assert torch.equal(grad_p, grad), fill
        assert _is_plus_zero(grad_p[masked]), fill
        with torch.no_grad():
            loss_n = fused_ce.fused_cross_entropy(poisoned, targets,
                                                  ignore_index=-100, **opts)
        assert torch.isfinite(loss_n), fill


@pytest.mark.parametrize("R,V", [(16, 50257), (7, 13), (8, 1024),
                                 (4, MID_V + 1)])
def test_nothing_masked_is_bit_identical_to_the_default_call(R, V):
    # R < 2^24: 1.0f / R on the device is the host's float(1.0 / R)
    logits = _logits(R, V, R + V)
    targets = _seam_targets(R, V)
    _, grad_default = _fused(logits, targets)
    _, grad_opts = _fused(logits, targets, ignore_index=-100)
    assert torch.equal(grad_opts, grad_default)


@pytest.mark.parametrize("opts", [OPTION_SETS["mask"], OPTION_SETS["all"]],
                         ids=["mask", "all"])
def test_valid_rows_equal_the_compacted_batch(opts):
    # V = 1024: no head, no tail, every row on a 16-byte boundary, so a row
    # keeps its phase when the masked rows are taken out
    R, V = 8, 1024
    logits = _logits(R, V, 21)
    masked = _mask_rows(R, "alternating")
    seam = _seam_targets(R, V)
    targets = torch.where(masked, torch.full_like(seam, -100), seam)
    loss, grad = _fused(logits, targets, ignore_index=-100, **opts)
    loss_c, grad_c = _fused(logits[~masked].contiguous(), targets[~masked],
                            ignore_index=-100, **opts)
    assert torch.equal(grad[~masked], grad_c)
    # same per-row losses; only the order of the final fp32 sum may differ
    torch.testing.assert_close(loss, loss_c, rtol=1e-6, atol=0)


@pytest.mark.parametrize("opts", [OPTION_SETS["mask"], OPTION_SETS["all"]],
                         ids=["mask", "all"])
@pytest.mark.parametrize("onepass", ["1", "0"])
@pytest.mark.parametrize("R,V,offset", [(8, 1003, 3), (6, 50257, 5)])
def test_odd_offset_view_stays_inside_its_rows(monkeypatch, R, V, offset,
                                               onepass, opts):
    # the view sits in a 1e30-filled buffer: a read outside a row drags 1e30
    # into it, a store outside the view changes the buffer
    monkeypatch.setenv("SHTENS_CE_ONEPASS", onepass)
    buf = torch.full((R * V + 32,), 1e30, device="cuda", dtype=torch.bfloat16)
    logits = buf[offset:offset + R * V].view(R, V)
    logits.copy_(_logits(R, V, V + offset))
    assert logits.data_ptr() % 4 == 2 and logits.is_contiguous()
    before = buf.clone()

    targets = _seam_targets(R, V, offset)
    targets[0] = -100
    targets[R - 1] = -100
    _check(logits, targets, ignore_index=-100, **opts)
    assert torch.equal(buf, before)

    # out-of-range targets that are not ignore_index
    bad = targets.clone()
    bad[1] = V
    bad[R - 2] = -5
    as_ignored = bad.clone()
    as_ignored[1] = -100
    as_ignored[R - 2] = -100
    _, grad_t = _reference(logits, as_ignored, ignore_index=-100, **opts)
    loss_f, grad_f = _fused(logits, bad, ignore_index=-100, **opts)
    assert torch.isnan(loss_f)
    assert _is_plus_zero(grad_f[1]) and _is_plus_zero(grad_f[R - 2])
    torch.testing.assert_close(grad_f.float(), grad_t, **GRAD_TOL)
    with torch.no_grad():
        assert torch.isnan(fused_ce.fused_cross_entropy(
            logits, bad, ignore_index=-100, **opts))
    assert torch.equal(buf, before)


def _small():
    R, V = 9, 1003
    masked = _mask_rows(R, "alternating")
    seam = _seam_targets(R, V)
    return _logits(R, V, 11), torch.where(masked, torch.full_like(seam, -100),
                                          seam)


@pytest.mark.parametrize("opts", [OPTION_SETS["mask"], OPTION_SETS["all"]],
                         ids=["mask", "all"])
def test_upstream_grad_scaling(opts):
    logits, targets = _small()
    _, grad_t = _reference(logits, targets, ignore_index=-100, **opts)
    _, g3 = _fused(logits, targets, scale=3.0, ignore_index=-100, **opts)
    torch.testing.assert_close(g3.float(), 3.0 * grad_t, **GRAD_TOL)
    assert _is_plus_zero(g3[targets == -100])


@pytest.mark.parametrize("opts", [OPTION_SETS["mask"], OPTION_SETS["all"]],
                         ids=["mask", "all"])
def test_backward_twice_retain_graph(opts):
    logits, targets = _small()
    _, grad_t = _reference(logits, targets, ignore_index=-100, **opts)
    lf = logits.clone().requires_grad_(True)
    loss = fused_ce.fused_cross_entropy(lf, targets, ignore_index=-100, **opts)
    (g1,) = torch.autograd.grad(loss, lf, retain_graph=True)
    snap = g1.clone()
    (g2,) = torch.autograd.grad(loss, lf)
    torch.cuda.synchronize()
    assert g2.data_ptr() != g1.data_ptr()
    assert torch.equal(g1, snap)
    torch.testing.assert_close(g1.float(), grad_t, **GRAD_TOL)
    torch.testing.assert_close(g2.float(), g1.float(), **GRAD_TOL)
    # same row_lse, same coefficients, same formula: bit for bit
    assert torch.equal(g2, g1)


@pytest.mark.parametrize("opts", [OPTION_SETS["mask"], OPTION_SETS["all"]],
                         ids=["mask", "all"])
def test_no_grad_loss_equals_grad_path_loss(opts):
    logits, targets = _small()
    loss_g, _ = _check(logits, targets, ignore_index=-100, **opts)
    with torch.no_grad():
        loss_n = fused_ce.fused_cross_entropy(logits, targets,
                                              ignore_index=-100, **opts)
    assert not loss_n.requires_grad
    # the two kernels differ in the fp32 summation order inside lse and
    # sum_j x_j: a few ulp of sums of ~1e3 terms.  lse ~ 11 enters z*lse^2
    # with derivative 2*z*lse ~ 2, so a few 1e-6 of lse stay below 1e-5
    torch.testing.assert_close(loss_n, loss_g, rtol=1e-5, atol=1e-5)


def test_forward_and_backward_do_not_sync():
    logits, targets = _small()
    lf = logits.clone().requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = fused_ce.fused_cross_entropy(lf, targets, ignore_index=-100,
                                            label_smoothing=0.1, z_loss=0.1)
        (loss * 3.0).backward()
        with torch.no_grad():
            fused_ce.fused_cross_entropy(logits, targets, ignore_index=-100)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.isfinite(loss) and bool(torch.isfinite(lf.grad).all())


def _model(name):
    if name == "gpt2":
        from sharedtensor_amd.models.gpt2 import GPT2, GPT2Config
        return GPT2(dataclasses.replace(GPT2Config.tiny(), ignore_index=-100))
    from sharedtensor_amd.models.llama import Llama, LlamaConfig
    return Llama(dataclasses.replace(LlamaConfig.tiny(), ignore_index=-100))


@pytest.mark.parametrize("name", ["gpt2", "llama"])
def test_model_loss_is_the_masked_mean(name):
    torch.manual_seed(3)
    m = _model(name).cuda().to(torch.bfloat16)
    idx = torch.randint(0, m.cfg.vocab_size, (2, 33), device="cuda")
    x, y = idx[:, :-1], idx[:, 1:].clone()
    y[:, ::2] = -100  # half the targets
    logits, loss = m(x, y)
    assert logits.dtype == torch.bfloat16
    want = cross_entropy_reference(
        logits.detach().reshape(-1, m.cfg.vocab_size).float(), y.reshape(-1),
        ignore_index=-100)
    torch.testing.assert_close(loss.float(), want, **LOSS_TOL)
    loss.backward()
    torch.cuda.synchronize()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all())
               for p in m.parameters())
