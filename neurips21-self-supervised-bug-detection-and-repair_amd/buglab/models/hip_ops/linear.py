"""Row-wise building blocks with autograd: gathered rows, the (gathered, concatenated) Linear, row dot products, dropout."""
from __future__ import annotations

from typing import Sequence

import torch

from . import _switches
from ._cabi import (ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH, _ACTS, _check, Dropout, _f32, _i32, load_library, NO_DROPOUT, _p,
                    RowSource, _stream)
from ._autograd import _grad_target, _in_seq_gemm_mode, _seq_gemm_mode_code, _take_saved
from .gemm import act_bwd, gemm_rows, gemm_rows_x6, gemm_wgrad, gemm_wgrad_x6, pack_bf16x3, scatter_add_rows
from .weights import _packed_layer_weights

__all__ = ["_GatherRows", "gather_rows", "act_bwd_packed", "_GatherLinear", "gather_linear", "_RowDot", "rowdot",
           "dropout_rows", "_DropoutFn"]


class _GatherRows(torch.autograd.Function):
    """x[idx] as a compact copy; backward = one zero-filled [N, H] buffer + one scatter-add."""

    @staticmethod
    def forward(ctx, x, idx):
        _f32(x, "x")
        R, H = idx.shape[0], x.shape[1]
        out = torch.empty((R, H), dtype=torch.float32, device=x.device)
        _check(load_library().bl_gather_rows(x.data_ptr(), x.stride(0), _i32(idx).data_ptr(), R, H, out.data_ptr(), out.stride(0), _stream()),
               "bl_gather_rows")
        ctx.saved = (idx, x.shape)
        return out

    @staticmethod
    def backward(ctx, g_out):
        idx, shape = _take_saved(ctx)
        g_x = torch.zeros(shape, dtype=torch.float32, device=g_out.device)
        scatter_add_rows(g_out.contiguous(), 0, shape[1], idx, g_x)
        return g_x, None


def gather_rows(x, idx):
    return _GatherRows.apply(x, idx)


def act_bwd_packed(g_y, y, act, drop: "Dropout", g_bias=None):
    """-> bf16x3-packed g_z int16 [R, 3 N] of y = drop(act(z + bias)) (bl_act_bwd_packed); g_bias accumulates column sums."""
    R, N = y.shape
    out = torch.empty((R, 3 * N), dtype=torch.int16, device=y.device)
    _check(load_library().bl_act_bwd_packed(_f32(g_y).data_ptr(), _f32(y).data_ptr(), R, N, y.stride(0), int(act), drop.c(), None, _p(g_bias),
                                            out.data_ptr(), _stream()), "bl_act_bwd_packed")
    return out


class _GatherLinear(torch.autograd.Function):
    """act(concat_j(X_j[idx_j]) @ W + b) without materialising the gather/concat."""

    @staticmethod
    def forward(ctx, W, bias, act, nsrc, *flat):
        drop = NO_DROPOUT
        if len(flat) == 2 * nsrc + 1:  # optional trailing Dropout: y = drop(act(x W + b))
            drop, flat = flat[-1], flat[:-1]
        xs, idxs = flat[:nsrc], flat[nsrc:]
        sources = list(zip(xs, idxs))
        R = idxs[0].shape[0] if idxs[0] is not None else xs[0].shape[0]
        K, N = W.shape
        x6 = (_switches.LINEAR_X6 and _switches.GEMM_MODE == "bf16x6" and nsrc == 1 and idxs[0] is None and R >= _switches.LINEAR_X6_MIN_ROWS and K % 32 == 0
              and N % 32 == 0 and act in (ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH) and xs[0].is_contiguous())
        if x6:
            need_bwd = any(ctx.needs_input_grad)
            xp = pack_bf16x3(xs[0])
            wkn, wnk = _packed_layer_weights(_f32(W, "W"), need_bwd)
            out = gemm_rows_x6([(xp, None, K)], wkn, R, N, bias=bias, act=act, drop=drop, kind="linear_x6")
            # (the OUTPUT goes through save_for_backward: kept as a plain ctx attribute it forms the cycle output -> grad_fn -> ctx ->
            # output, which Python's collector cannot see through the C++ node -- every step's activations stayed allocated,
            # ~1 GiB per seq-great step until the device was full)
            ctx.save_for_backward(out)
            ctx.saved = (W, bias, act, sources, drop, xp if need_bwd else None, wnk)
            ctx.seq_mode = _seq_gemm_mode_code()
            return out
        out = gemm_rows(sources, _f32(W, "W"), R, W.shape[1], bias=bias, act=act, drop=drop)
        ctx.save_for_backward(out)
        ctx.saved = (W, bias, act, sources, drop, None, None)
        return out

    @staticmethod
    def backward(ctx, g_out):
        W, bias_p, act, sources, drop, xp, wnk = _take_saved(ctx)
        (out,) = ctx.saved_tensors
        has_bias = bias_p is not None
        R, N = out.shape
        K = W.shape[0]
        dev = W.device
        # weight / bias gradients are accumulated by the kernels: straight into .grad where the optimiser opted in (FlatAdam's flat
        # buffer: no zero fill, no autograd accumulation kernel -- 20 Linears per step in seq-great), into fresh zeros otherwise
        g_W, r_W = _grad_target(W)
        g_bias, r_bias = _grad_target(bias_p) if has_bias else (None, None)
        if xp is not None:  # bf16x6 path
            gzp = act_bwd_packed(g_out.contiguous(), out, act, drop, g_bias)
            with _in_seq_gemm_mode(ctx.seq_mode):
                gemm_wgrad_x6([(xp, None, K)], gzp, R, N, g_W)
                g_x = gemm_rows_x6([(gzp, None, N)], wnk, R, K, kind="linear_dgrad_x6") if ctx.needs_input_grad[4] else None
            return (r_W, r_bias, None, None, g_x, None) + ((None,) if drop is not NO_DROPOUT else ())
        g_z = act_bwd(g_out.contiguous(), out, act, drop, g_bias)
        gemm_wgrad(sources, g_z, R, N, g_W)
        g_a = gemm_rows([(g_z, None)], W, R, K, b_is_nk=True, ldb=N)
        g_xs, off = [], 0
        for j, (x, idx) in enumerate(sources):
            w = x.shape[1]
            if not ctx.needs_input_grad[4 + j]:
                g_xs.append(None)
            elif idx is None:
                g_xs.append(g_a[:, off : off + w].contiguous())
            else:
                g_x = torch.zeros_like(x)
                scatter_add_rows(g_a, off, w, idx, g_x)
                g_xs.append(g_x)
            off += w
        return (r_W, r_bias, None, None) + tuple(g_xs) + (None,) * (len(sources) + (1 if drop is not NO_DROPOUT else 0))


def gather_linear(sources: Sequence[RowSource], W, bias, act: str = "none", drop: Dropout = NO_DROPOUT):
    """drop(act(concat_j(x_j[idx_j]) @ W + bias)).  W / bias gradients: added straight into `W.grad` / `bias.grad` (backward
    returns None for them) when the parameter opted in -- see _opted_in_for_direct_grad for the contract and its consequences
    for torch.autograd.grad and parameter hooks -- through autograd otherwise."""
    xs = [x for x, _ in sources]
    idxs = [i for _, i in sources]
    extra = (drop,) if drop is not NO_DROPOUT else ()
    return _GatherLinear.apply(W, bias, _ACTS[act], len(sources), *xs, *idxs, *extra)


class _RowDot(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        R, H = x.shape
        y = torch.empty((R,), dtype=torch.float32, device=x.device)
        _check(load_library().bl_rowdot_fwd(_f32(x).data_ptr(), x.stride(0), _f32(w).data_ptr(), _p(b), R, H, y.data_ptr(), _stream()),
               "bl_rowdot_fwd")
        ctx.saved = (x, w, b is not None)
        return y

    @staticmethod
    def backward(ctx, g_y):
        x, w, has_b = _take_saved(ctx)
        R, H = x.shape
        g_x = torch.empty_like(x)
        g_w = torch.zeros_like(w)
        g_b = torch.zeros((1,), dtype=torch.float32, device=x.device) if has_b else None
        _check(
            load_library().bl_rowdot_bwd(_f32(g_y.contiguous()).data_ptr(), x.data_ptr(), x.stride(0), w.data_ptr(), R, H,
                                         g_x.data_ptr(), g_x.stride(0), g_w.data_ptr(), _p(g_b), _stream()),
            "bl_rowdot_bwd")
        return g_x, g_w, g_b


def rowdot(x, w, b=None):
    return _RowDot.apply(x, w, b)


def dropout_rows(x, drop: Dropout):
    """Elementwise counter-hash dropout with autograd (embedding dropout of the sequence models)."""
    if drop.p <= 0:
        return x
    return _DropoutFn.apply(x, drop)


class _DropoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, drop):
        y = x.contiguous().clone()
        _check(load_library().bl_dropout_inplace(_f32(y).data_ptr(), y.numel(), drop.c(), _stream()), "bl_dropout_inplace")
        ctx.drop = drop
        return y

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous().clone()
        _check(load_library().bl_dropout_inplace(g.data_ptr(), g.numel(), ctx.drop.c(), _stream()), "bl_dropout_inplace")
        return g, None
