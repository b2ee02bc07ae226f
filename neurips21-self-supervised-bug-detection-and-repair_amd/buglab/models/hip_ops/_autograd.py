"""What every autograd Function of buglab.models.hip_ops shares: handing saved buffers over once, and where a parameter's
gradient is accumulated."""
from __future__ import annotations

import torch

from ._streams import _direct_small

__all__ = ["_take_saved", "_grad_target"]


def _take_saved(ctx):
    """What a Function's forward kept in `ctx.saved`, handed over ONCE: backward drops the references at once (activations are
    freed as the backward pass proceeds), so a second backward through the same graph has nothing to read."""
    saved = ctx.saved
    if saved is None:
        raise RuntimeError("hip_ops: this graph's buffers were freed by its first backward pass; retain_graph=True / a second "
                           "backward through the same forward is not supported by the hip_ops Functions")
    ctx.saved = None
    return saved


def _grad_target(param):
    """(buffer the kernels accumulate into, what backward returns for it)."""
    d = _direct_small(param)
    if d is not None:
        return d, None
    z = torch.zeros_like(param)
    return z, z
