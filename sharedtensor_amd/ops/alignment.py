"""Pointer alignment for the vectorised kernels' tensor arguments."""
from __future__ import annotations


def aligned(t, nbytes: int):
    """``t`` if its storage starts on an ``nbytes`` boundary, else a copy
    that does.  contiguous() keeps an offset view of a larger buffer as it
    is; a copy aligns it.  None (an optional tensor) passes through."""
    if t is not None and t.data_ptr() % nbytes:
        return t.clone()
    return t
