"""Optimiser kernels on flat buffers: ordered squared norm, clip + Adam (single device and data-parallel forms), the same
with a parameter average kept in the pass, and the buffer exchange that puts the average in the parameters' place."""
from __future__ import annotations

from typing import Optional

import torch

from ._cabi import _check, _f32, load_library, _p, _stream

__all__ = ["_SQNORM_SCRATCH", "sqnorm", "adam_clip_step", "adam_clip_step_dp", "adam_clip_step_ema", "adam_clip_step_dp_ema", "swap_buffers"]


# ------------------------------------------------------------------------------------------------
# optimiser on flat buffers
_SQNORM_SCRATCH: dict = {}


def sqnorm(flat_grad: torch.Tensor, out: torch.Tensor, scratch: Optional[torch.Tensor] = None):
    """sum(g^2) -> out[0], added in one fixed order (replicas with equal gradients clip by the same number).  `scratch`
    (bl_sqnorm_scratch_bytes()) defaults to one buffer per (device, stream)."""
    lib = load_library()
    if scratch is None:
        key = (flat_grad.device, _stream())
        scratch = _SQNORM_SCRATCH.get(key)
        if scratch is None:
            scratch = _SQNORM_SCRATCH[key] = torch.empty(lib.bl_sqnorm_scratch_bytes() // 4, dtype=torch.float32, device=flat_grad.device)
    _check(lib.bl_sqnorm(_f32(flat_grad).data_ptr(), flat_grad.numel(), out.data_ptr(), scratch.data_ptr(), _stream()), "bl_sqnorm")
    return out


def adam_clip_step(param, grad, m, v, sqn, *, prescale=1.0, clip=0.5, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, step=1):
    _check(
        load_library().bl_adam_clip_step(_f32(param).data_ptr(), _f32(grad).data_ptr(), _f32(m).data_ptr(), _f32(v).data_ptr(),
                                         param.numel(), _p(sqn), float(prescale), float(clip), float(lr), float(beta1), float(beta2),
                                         float(eps), int(step), _stream()),
        "bl_adam_clip_step")


def adam_clip_step_dp(param, grad, m, v, sqn, batch_total, *, clip=0.5, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, step=1):
    """Data-parallel form: grad = sum over ranks of B_rank * grad_rank, batch_total = device scalar sum of B_rank."""
    _check(
        load_library().bl_adam_clip_step_dp(_f32(param).data_ptr(), _f32(grad).data_ptr(), _f32(m).data_ptr(), _f32(v).data_ptr(),
                                            param.numel(), _p(sqn), _f32(batch_total).data_ptr(), float(clip), float(lr), float(beta1),
                                            float(beta2), float(eps), int(step), _stream()),
        "bl_adam_clip_step_dp")


def adam_clip_step_ema(param, grad, m, v, ema, sqn, *, one_minus_decay, prescale=1.0, clip=0.5, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8,
                       step=1):
    """adam_clip_step, and in the same pass ema += one_minus_decay * (p_new - ema) (one fma per element, buglab.runtime._averaging)."""
    _check(
        load_library().bl_adam_clip_step_ema(_f32(param).data_ptr(), _f32(grad).data_ptr(), _f32(m).data_ptr(), _f32(v).data_ptr(),
                                             _f32(ema).data_ptr(), param.numel(), _p(sqn), float(prescale), float(clip), float(lr),
                                             float(beta1), float(beta2), float(eps), int(step), float(one_minus_decay), _stream()),
        "bl_adam_clip_step_ema")


def adam_clip_step_dp_ema(param, grad, m, v, ema, sqn, batch_total, *, one_minus_decay, clip=0.5, lr=1e-4, beta1=0.9, beta2=0.999,
                          eps=1e-8, step=1):
    """adam_clip_step_dp with the parameter average; a zero batch_total leaves `ema` untouched too."""
    _check(
        load_library().bl_adam_clip_step_dp_ema(_f32(param).data_ptr(), _f32(grad).data_ptr(), _f32(m).data_ptr(), _f32(v).data_ptr(),
                                                _f32(ema).data_ptr(), param.numel(), _p(sqn), _f32(batch_total).data_ptr(), float(clip),
                                                float(lr), float(beta1), float(beta2), float(eps), int(step), float(one_minus_decay),
                                                _stream()),
        "bl_adam_clip_step_dp_ema")


def swap_buffers(a: torch.Tensor, b: torch.Tensor):
    """Exchange the contents of two fp32 buffers of equal size on the device (one pass, no temporary)."""
    if a.numel() != b.numel():
        raise ValueError(f"swap_buffers: {a.numel()} vs {b.numel()} elements")
    _check(load_library().bl_swap_f32(_f32(a).data_ptr(), _f32(b).data_ptr(), a.numel(), _stream()), "bl_swap_f32")
