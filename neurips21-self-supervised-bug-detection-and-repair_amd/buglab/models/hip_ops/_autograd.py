"""What every autograd Function of buglab.models.hip_ops shares: handing saved buffers over once, and where a parameter's
gradient is accumulated."""
from __future__ import annotations

import contextlib

import torch

from ._cabi import load_library
from ._streams import _direct_small

__all__ = ["_take_saved", "_grad_target", "_seq_gemm_mode_code", "_in_seq_gemm_mode"]


def _seq_gemm_mode_code() -> int:
    """bl_seq_gemm_mode() now: what a Function's forward keeps for its backward."""
    return int(load_library().bl_seq_gemm_mode())


@contextlib.contextmanager
def _in_seq_gemm_mode(code: int):
    """Run a Function's backward in the sequence GEMM mode its forward ran in: the saved packed activations and the gradients
    belong to one arithmetic, so a set_seq_gemm_mode between the two passes changes nothing for graphs already built."""
    lib = load_library()
    now = int(lib.bl_seq_gemm_mode())
    if now != code:
        lib.bl_set_seq_gemm_mode(code)
    try:
        yield
    finally:
        if now != code:
            lib.bl_set_seq_gemm_mode(now)


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
