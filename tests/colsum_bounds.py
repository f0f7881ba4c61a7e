"""Derived bound for bf16 column sums that come from fp32 partial sums with a
known summation tree (the attention backward's column-sum epilogue and
k_colsum_reduce), in the style of kernel_bounds.py.

Reference: the fp64 column sum of the very values the kernel summed.

An fp32 evaluation of a sum along any tree of height h (the largest number of
additions one term passes through) is off by at most gamma(h) * sum|x|,
gamma(h) = h U / (1 - h U), U = 2^-24.  Rounding that fp32 sum s to bf16 adds
at most half a bf16 ulp at |s| <= |ref| + slack.  So

    |got - ref| <= 0.5 * ulp_bf16(|ref| + slack) + slack,
    slack = gamma(h) * sum|x|.

Tree heights, every `+=` counted, the first one onto 0.f included:

* attention epilogue (attn_bwd_tile.h): a lane adds its 4 rows in pass order
  (4), the 8 lanes that share a chunk as a 3-level butterfly (3), the 4 waves
  in wave order (4): ATTN_EPILOGUE_ADDS = 11 for the 128 rows of a workgroup;
* k_colsum_reduce (bias_grad_kernels.hip): a row group adds its
  ceil(G / 64) rows in row order, 4 row groups are added in order, then the
  16 results in order: reduce_adds(G) = ceil(G / 64) + 4 + 16.
"""
import torch

from kernel_bounds import bf16_ulp, gamma

ATTN_EPILOGUE_ADDS = 11


def reduce_adds(G: int) -> int:
    return -(-G // 64) + 4 + 16


def colsum_check(got, terms, adds, what):
    """got: bf16 (N,); terms: (rows, N) values whose columns were summed;
    adds: height of the fp32 tree.  Returns the largest error over its
    bound."""
    assert got.dtype == torch.bfloat16 and got.shape == terms.shape[1:], what
    x = terms.double()
    ref = x.sum(0)
    slack = gamma(adds) * x.abs().sum(0)
    tol = 0.5 * bf16_ulp(ref.abs() + slack) + slack
    assert torch.isfinite(got.float()).all(), f"{what}: not finite"
    err = (got.double() - ref).abs()
    worst = float((err / tol).max())
    bad = err > tol
    assert not bad.any(), (
        f"{what}: {int(bad.sum())} of {bad.numel()} columns outside the "
        f"bound; first at {int(bad.nonzero()[0])}, worst {worst:.3g} of bound")
    return worst
