"""Parallel training on the shared-tensor engine."""
from .async_dp import (AsyncAdamW, AsyncDPTrainer, AsyncSGD, FlatParamShared,
                       no_decay_groups)

__all__ = ["AsyncAdamW", "AsyncDPTrainer", "AsyncSGD", "FlatParamShared",
           "no_decay_groups"]
