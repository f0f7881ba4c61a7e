"""One-pass fused cross-entropy (k_ce_fwd_grad + skip_if_unit backward) vs
torch.nn.functional.cross_entropy on the same bf16 logits upcast to fp32.

Rows of an odd-V matrix start at every 16-byte phase, so each row is a head
of up to 7 elements, a body of 16-byte chunks and a tail of up to 7; the
shapes and targets below aim at those seams.
"""
import pytest
import torch

import kernel_bounds as kb
from sharedtensor_amd import _core
from sharedtensor_amd.ops import fused_ce

pytestmark = pytest.mark.gpu

LOSS_TOL = dict(rtol=2e-3, atol=2e-3)
GRAD_TOL = dict(rtol=5e-2, atol=1e-4)

MAX_V = _core.ce_fwd_grad_max_v()  # largest V the one-pass kernel takes
MID_V = 1024 * 7 * 8               # last V of the 7-chunk instantiation


def _seam_targets(R, V, offset=0):
    """Targets at element 0, at V-1, in a head and in a tail element of rows
    that have one (`offset` = element offset of the matrix from a 16-byte
    boundary); random elsewhere."""
    return kb.seam_targets(R, V, offset).cuda()


def _reference(logits, targets):
    lt = logits.detach().clone().requires_grad_(True)
    loss = torch.nn.functional.cross_entropy(lt.float(), targets)
    loss.backward()
    return loss.detach(), lt.grad.float()


def _check(logits, targets):
    loss_t, grad_t = _reference(logits, targets)
    lf = logits.detach().requires_grad_(True)  # same storage and offset
    loss_f = fused_ce.fused_cross_entropy(lf, targets)
    loss_f.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(loss_f)
    torch.testing.assert_close(loss_f.float(), loss_t, **LOSS_TOL)
    torch.testing.assert_close(lf.grad.float(), grad_t, **GRAD_TOL)
    # element by element: 1 bf16 ulp + slack against the fp64 reference
    kb.ce_check({"mean": loss_f.detach(), "dlogits": lf.grad}, logits,
                targets, "fused_cross_entropy", f"V={logits.shape[1]}")
    return loss_f.detach(), lf.grad


@pytest.mark.parametrize("R,V", [
    (16, 50257),      # every 16-byte phase twice at the real chunk count
    (7, 13),          # shorter than one chunk per thread
    (8, 1024),        # aligned: no head, no tail
    (5, 1000),        # even V, not a multiple of 8
    (4, MID_V),       # last V of the 7-chunk instantiation ...
    (4, MID_V + 1),   # ... first of the 16-chunk one
    (4, MAX_V),       # capacity
    (4, MAX_V + 1),   # beyond it: two-kernel fallback
])
def test_matches_torch(R, V):
    torch.manual_seed(R + V)
    logits = (torch.randn(R, V, device="cuda") * 3).to(torch.bfloat16)
    _check(logits, _seam_targets(R, V))


@pytest.mark.parametrize("R,V,offset", [(6, 1003, 3), (3, 50257, 5)])
def test_odd_offset_view_ignores_neighbours(R, V, offset):
    # a head or tail that reads a neighbour drags 1e30 into the row max; a
    # head or tail store past the row shows up in the next row's gradient
    torch.manual_seed(V + offset)
    buf = torch.full((R * V + 32,), 1e30, device="cuda", dtype=torch.bfloat16)
    logits = buf[offset:offset + R * V].view(R, V)
    logits.copy_((torch.randn(R, V, device="cuda") * 3).to(torch.bfloat16))
    assert logits.data_ptr() % 4 == 2 and logits.is_contiguous()
    before = buf.clone()
    _check(logits, _seam_targets(R, V, offset))
    assert torch.equal(buf, before)


def test_extreme_logit():
    torch.manual_seed(5)
    R, V = 6, 1003
    logits = torch.randn(R, V, device="cuda") * 0.1
    logits[2, 517] = 80.0
    logits[4, V - 1] = 80.0
    targets = _seam_targets(R, V)
    targets[4] = 3  # a row whose target is not the spike: loss near 80
    _, grad = _check(logits.to(torch.bfloat16), targets)
    assert bool(torch.isfinite(grad).all())


def _small():
    torch.manual_seed(11)
    R, V = 9, 1003
    logits = (torch.randn(R, V, device="cuda") * 3).to(torch.bfloat16)
    return logits, _seam_targets(R, V)


def test_upstream_grad_scaling():
    logits, targets = _small()
    _, g1 = _check(logits, targets)
    lf = logits.clone().requires_grad_(True)
    (fused_ce.fused_cross_entropy(lf, targets) * 3.0).backward()
    torch.cuda.synchronize()
    torch.testing.assert_close(lf.grad.float(), 3.0 * g1.float(), rtol=2e-2,
                               atol=1e-5)


def test_backward_twice_retain_graph():
    logits, targets = _small()
    _, grad_t = _reference(logits, targets)
    lf = logits.clone().requires_grad_(True)
    loss = fused_ce.fused_cross_entropy(lf, targets)
    (g1,) = torch.autograd.grad(loss, lf, retain_graph=True)
    snap = g1.clone()
    (g2,) = torch.autograd.grad(loss, lf)
    torch.cuda.synchronize()
    assert g2.data_ptr() != g1.data_ptr()
    # same row_lse, same formula: the classic kernel reproduces the
    # one-pass buffer bit for bit
    assert torch.equal(g2, g1)
    assert torch.equal(g1, snap)
    torch.testing.assert_close(g1.float(), grad_t, **GRAD_TOL)


def test_no_grad_loss_equals_grad_path_loss():
    logits, targets = _small()
    loss_g, _ = _check(logits, targets)
    with torch.no_grad():
        loss_n = fused_ce.fused_cross_entropy(logits, targets)
    assert not loss_n.requires_grad
    # the two kernels differ only in the fp32 summation order inside lse:
    # a few ulp of an exp-sum of ~1e3 positive terms, far below 1e-5
    torch.testing.assert_close(loss_n, loss_g, rtol=1e-5, atol=1e-5)


def test_two_kernel_path_by_env(monkeypatch):
    monkeypatch.setenv("SHTENS_CE_ONEPASS", "0")
    torch.manual_seed(13)
    R, V = 16, 50257
    logits = (torch.randn(R, V, device="cuda") * 3).to(torch.bfloat16)
    _check(logits, _seam_targets(R, V))
