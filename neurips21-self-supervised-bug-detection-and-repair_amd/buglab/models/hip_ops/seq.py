"""Sequence models: residual LayerNorm, relational attention, the GRU scan and the one-call GREAT encoder layer."""
from __future__ import annotations

import ctypes
import os
from typing import NamedTuple, Optional

import torch

from . import _switches, _streams
from ._cabi import bl_great_layer_grads_t, bl_great_layer_t, bl_head_view_t, _check, Dropout, _f32, _i32, load_library, NO_DROPOUT, _p, _stream
from ._streams import _timed
from ._autograd import _grad_target, _in_seq_gemm_mode, _seq_gemm_mode_code, _take_saved
from .gemm import gemm_rows, gemm_wgrad, layernorm_bwd
from .weights import _packed_layer_weights

__all__ = ["_AddLayerNorm", "add_layernorm", "RelEdges", "_group_ptr_cache", "_uniform_group_ptr", "ATTN_STORED_MAX_L", "attention_path",
           "_RelAttention", "rel_attention", "_GruScan", "gru_scan", "great_layer_ok", "_great_desc", "_GreatLayer", "great_layer"]


# ------------------------------------------------------------------------------------------------
# `seq-great` relational transformer block (csrc/bl_seq_ops.hip + the MFMA GEMMs)
class _AddLayerNorm(torch.autograd.Function):
    """y = LayerNorm(x + r) (r optional); backward hands the same gradient to x and r."""

    @staticmethod
    def forward(ctx, x, r, gamma, beta, eps):
        _f32(x, "x")
        n, D = x.shape
        dev = x.device
        z = torch.empty_like(x) if r is not None else x
        y = torch.empty_like(x)
        mean = torch.empty((n,), dtype=torch.float32, device=dev)
        rstd = torch.empty((n,), dtype=torch.float32, device=dev)
        lib = load_library()
        ptrs = (x.data_ptr(), _p(r), _f32(gamma).data_ptr(), _f32(beta).data_ptr(), float(eps), n, D, z.data_ptr() if r is not None else None,
                y.data_ptr(), mean.data_ptr(), rstd.data_ptr())
        if _seq_gemm_mode_code() == 1 and D % 4 == 0 and all(t is None or t.data_ptr() % 16 == 0 for t in (x, r, gamma, beta, y, z)):
            # bf16x1: the next Linear rounds this output to its bf16 high plane, where an ulp decides between two neighbours 2^-8
            # apart.  The one-call GREAT layer normalises with the four-channels-per-lane kernel (other order of the row sums, an
            # ulp apart); the same kernel here keeps the op-by-op path equal to it to fp32 rounding in this mode as well.
            _check(lib.bl_add_layernorm_fwd_packed(*ptrs, None, _stream()), "bl_add_layernorm_fwd_packed")
        else:
            _check(lib.bl_add_layernorm_fwd(*ptrs, _stream()), "bl_add_layernorm_fwd")
        ctx.saved = (z, mean, rstd, gamma, beta, r is not None)
        return y

    @staticmethod
    def backward(ctx, g_y):
        z, mean, rstd, gamma, beta, has_r = _take_saved(ctx)
        (gg, rg), (gb, rb) = _grad_target(gamma), _grad_target(beta)
        g_z = layernorm_bwd(g_y.contiguous(), z, mean, rstd, gamma, gg, gb)
        return g_z, (g_z if has_r else None), rg, rb, None


def add_layernorm(x, r, gamma, beta, eps: float = 1e-5):
    return _AddLayerNorm.apply(x.contiguous(), r.contiguous() if r is not None else None, gamma, beta, eps)


class RelEdges(NamedTuple):
    """Edges of a padded [B, L] minibatch as a CSR over query rows b * L + i (buglab.data.seqcollate.edge_csr)."""

    row_ptr: torch.Tensor   # int32 [B * L + 1]
    key: torch.Tensor       # int32 [n]  key position of the entry
    code: torch.Tensor      # int32 [n]  2 * edge_type + direction (0: the query is the edge's source, 1: its target)
    num_entries: int


_group_ptr_cache = {}


def _uniform_group_ptr(G: int, L: int, device):
    key = (G, L, str(device))
    t = _group_ptr_cache.get(key)
    if t is None:
        if len(_group_ptr_cache) > 64:
            _group_ptr_cache.clear()
        t = (torch.arange(G + 1, dtype=torch.int64) * L).to(torch.int32).to(device)
        _group_ptr_cache[key] = t
    return t


# The attention without an [L, L] array (csrc/bl_attn_stream.hip): "auto" = only where neither stored-P path takes the shape
# (L > ATTN_STORED_MAX_L), "1" = wherever bl_rel_attn_stream_ok holds and the mode allows, "0" = never.  An A/B switch like those
# of _switches.py, assigned on the package (`hip_ops.STREAMING_ATTENTION = "1"`) and forwarded to this module, its one owner; it
# is read here at call time and is deliberately not in `__all__` (a star-imported copy would go stale).
STREAMING_ATTENTION = os.environ.get("BL_STREAMING_ATTENTION", "auto")
ATTN_STORED_MAX_L = 1024  # bl_masked_softmax_* / bl_softmax_bwd and K^T in LDS (bl_rel_attn_probs_ok) stop here


def _streaming_switch() -> str:
    v = STREAMING_ATTENTION
    v = {True: "1", False: "0"}.get(v, v) if isinstance(v, bool) else str(v).strip().lower()
    if v not in ("auto", "1", "0"):
        raise ValueError(f"STREAMING_ATTENTION / BL_STREAMING_ATTENTION must be 'auto', '1' or '0' (got {STREAMING_ATTENTION!r})")
    return v


def attention_path(L: int, dk: int, T: int, scalar_bias: bool = False, value_biases: bool = False) -> str:
    """Which kernels _RelAttention runs for the shape: "fused" (scores -> probabilities in one kernel, P stored), "rowwise" (GEMM +
    edge terms + masked softmax, P stored) or "stream" (online softmax, nothing of size L x L).  A pure function of the shape, the
    mode and the switches; raises ValueError, before any launch, when no path takes the shape."""
    L, dk, T = int(L), int(dk), int(T)
    lib = load_library()
    switch = _streaming_switch()
    why_not = None  # why the streaming kernels cannot take it
    if scalar_bias:
        why_not = "the scalar key-bias mode has no streaming form"
    elif value_biases:
        why_not = "edge value biases (seq-rat) have no streaming form"
    elif not lib.bl_rel_attn_stream_ok(L, dk, T):
        why_not = f"bl_rel_attn_stream_ok(L={L}, dk={dk}, T={T}) is 0 (needs L % 4 == 0, dk == 32, 2 T dk <= 1024)"
    stored_ok = L <= ATTN_STORED_MAX_L
    if switch == "1" and why_not is None:
        return "stream"
    if stored_ok:
        return "fused" if (_switches.FUSED_ATTENTION and not scalar_bias and lib.bl_rel_attn_probs_ok(L, dk, T)) else "rowwise"
    if switch == "0":
        why_not = "streaming attention is switched off (STREAMING_ATTENTION = 0)"
    if why_not is None:
        return "stream"
    raise ValueError(f"rel_attention: sequence length L={L} exceeds the limit of {ATTN_STORED_MAX_L} keys of the stored-probability "
                     f"kernels, and the streaming attention cannot take the shape: {why_not}")


def _qkv_head_views(t, L, H, dk):
    """q / k / v (or their gradients) as head views of a [B L, H 3 dk] matrix, per head [q | k | v]: no permuted copies."""
    W = 3 * H * dk
    return [bl_head_view_t(t.data_ptr() + 4 * which * dk, L * W, 3 * dk, W) for which in range(3)]


def _row_head_view(t, L, H, dk):
    """[B L, H dk] as a [B, H, L, dk] head view."""
    return bl_head_view_t(t.data_ptr(), L * H * dk, dk, H * dk)


def _edge_ptrs(edges):
    if edges.num_entries > 0:
        return _i32(edges.row_ptr).data_ptr(), _i32(edges.key).data_ptr(), _i32(edges.code).data_ptr()
    return None, None, None


def _stream_attention_fwd(ctx, qkv, lens, edges, bias_f, bias_r, B, L, H, dk, T, drop):
    lib = load_library()
    G, D = B * H, H * dk
    scale = float(dk) ** -0.5
    out = torch.empty((B * L, D), dtype=torch.float32, device=qkv.device)
    lse = torch.empty((G * L,), dtype=torch.float32, device=qkv.device)
    q, k, v = _qkv_head_views(qkv, L, H, dk)
    o = _row_head_view(out, L, H, dk)
    with _timed("attn_stream_fwd", 4.0 * G * L * L * dk, nbytes=4.0 * G * L * (4 * dk + 1)):
        _check(lib.bl_rel_attn_stream_fwd(ctypes.byref(q), scale, ctypes.byref(k), ctypes.byref(v), *_edge_ptrs(edges), B, L, H, dk, T,
                                          _f32(bias_f).data_ptr(), _f32(bias_r).data_ptr(), _i32(lens).data_ptr(), drop.c(), ctypes.byref(o),
                                          lse.data_ptr(), _stream()), "bl_rel_attn_stream_fwd")
    # (the backward recomputes the probabilities from qkv and lse and sums delta from them: the context itself is not kept)
    ctx.saved = (qkv, lse, lens, edges, bias_f, bias_r, B, L, H, dk, T, drop, scale)
    return out


def _stream_attention_bwd(ctx, g_out):
    qkv, lse, lens, edges, bias_f, bias_r, B, L, H, dk, T, drop, scale = _take_saved(ctx)
    lib = load_library()
    G, D = B * H, H * dk
    g_out = _f32(g_out.contiguous())
    g_qkv = torch.empty((B * L, 3 * D), dtype=torch.float32, device=g_out.device)
    delta = torch.empty((G * L,), dtype=torch.float32, device=g_out.device)
    (g_bf, r_bf), (g_br, r_br) = _grad_target(bias_f), _grad_target(bias_r)
    q, k, v = _qkv_head_views(qkv, L, H, dk)
    gq, gk, gv = _qkv_head_views(g_qkv, L, H, dk)
    go = _row_head_view(g_out, L, H, dk)
    with _timed("attn_stream_bwd", 18.0 * G * L * L * dk, nbytes=4.0 * G * L * (10 * dk + 4)):
        _check(lib.bl_rel_attn_stream_bwd(ctypes.byref(go), lse.data_ptr(), ctypes.byref(q), scale, ctypes.byref(k), ctypes.byref(v),
                                          *_edge_ptrs(edges), B, L, H, dk, T, bias_f.data_ptr(), bias_r.data_ptr(), _i32(lens).data_ptr(),
                                          drop.c(), delta.data_ptr(), ctypes.byref(gq), ctypes.byref(gk), ctypes.byref(gv),
                                          g_bf.data_ptr(), g_br.data_ptr(), _stream()), "bl_rel_attn_stream_bwd")
    return g_qkv, None, None, r_bf, r_br, None, None, None, None, None, None, None, None, None


class _RelAttention(torch.autograd.Function):
    """Relational multi-head self-attention between the QKV projection and the output projection
    (reference multihead_attention.py:46-80, relational_multihead_attention.py:72-178).  Q.K^T, P.V and their four
    gradient products are MFMA GEMMs grouped by (sample, head); edge terms, masked softmax and value biases are the
    row-wise kernels of csrc/bl_seq_ops.hip."""

    @staticmethod
    def forward(ctx, qkv, lens, edges: RelEdges, bias_f, bias_r, vb_f, vb_r, B, L, H, dk, T, scalar_bias, drop: Dropout):
        lib = load_library()
        _f32(qkv, "qkv")
        ctx.path = attention_path(L, dk, T, scalar_bias, vb_f is not None)
        if ctx.path == "stream":
            return _stream_attention_fwd(ctx, qkv, lens, edges, bias_f, bias_r, B, L, H, dk, T, drop)
        G, D = B * H, H * dk
        st = _stream()
        scale = float(dk) ** -0.5
        t3 = qkv.view(B, L, H, 3, dk).permute(3, 0, 2, 1, 4).contiguous()  # [3, B, H, L, dk]
        qs, kt, vt = t3[0], t3[1], t3[2]
        qs.mul_(scale)  # multihead_attention.py:54: queries pre-scaled
        gptr = _uniform_group_ptr(G, L, qkv.device)
        mode = 1 if scalar_bias else 0
        has_e = edges.num_entries > 0
        if _switches.FUSED_ATTENTION and mode == 0 and lib.bl_rel_attn_probs_ok(L, dk, T):
            # scores, edge terms, masked softmax and nn.Dropout in one kernel: the scores never reach memory
            P = torch.empty((G * L, L), dtype=torch.float32, device=qkv.device)
            Pd = torch.empty_like(P) if drop.p > 0 else P
            with _timed("attn_probs_fwd", 0.0, nbytes=4.0 * G * L * (L * (2 if drop.p > 0 else 1) + 2 * dk)):  # writes P (+ Pd), reads q, k
                _check(lib.bl_rel_attn_probs_fwd(qs.data_ptr(), kt.data_ptr(), edges.row_ptr.data_ptr() if has_e else None,
                                                 edges.key.data_ptr() if has_e else None, edges.code.data_ptr() if has_e else None, B, L, H, dk, T,
                                                 _f32(bias_f).data_ptr(), _f32(bias_r).data_ptr(), _i32(lens).data_ptr(), drop.c(), P.data_ptr(),
                                                 Pd.data_ptr(), st), "bl_rel_attn_probs_fwd")
        else:
            S = gemm_rows([(qs.view(G * L, dk), None)], kt, G * L, L, b_is_nk=True, b_group_stride=L * dk, ldb=dk, group_ptr=gptr, G=G)
            if has_e:
                _check(lib.bl_rel_attn_bias_fwd(edges.row_ptr.data_ptr(), edges.key.data_ptr(), edges.code.data_ptr(), B, L, H, dk, mode,
                                                (kt if scalar_bias else qs).data_ptr(), _f32(bias_f).data_ptr(), _f32(bias_r).data_ptr(),
                                                S.data_ptr(), st), "bl_rel_attn_bias_fwd")
            P = S
            # softmax and nn.Dropout on the probabilities (multihead_attention.py:65-72) in one pass over the scores
            Pd = torch.empty_like(P) if drop.p > 0 else P
            _check(lib.bl_masked_softmax_dropout_fwd(S.data_ptr(), G * L, L, H * L, _i32(lens).data_ptr(), drop.c(), Pd.data_ptr(), st),
                   "bl_masked_softmax_dropout_fwd")
        mm32 = bool(_switches.FUSED_ATTENTION and lib.bl_attn_mm32_ok(L, dk))  # the skinny products on their own kernels (head dimension 32)
        if mm32:
            ctx_t = torch.empty((G * L, dk), dtype=torch.float32, device=qkv.device)
            with _timed("attn_rows_times", 2.0 * G * L * L * dk, nbytes=4.0 * G * L * (L + 2 * dk)):
                _check(lib.bl_attn_rows_times(Pd.data_ptr(), vt.data_ptr(), G, L, dk, None, 1.0, ctx_t.data_ptr(), st), "bl_attn_rows_times")
        else:
            ctx_t = gemm_rows([(Pd, None)], vt, G * L, dk, b_group_stride=L * dk, ldb=dk, group_ptr=gptr, G=G)
        if vb_f is not None and edges.num_entries > 0:
            _check(lib.bl_rel_value_bias_fwd(edges.row_ptr.data_ptr(), edges.key.data_ptr(), edges.code.data_ptr(), B, L, H, dk,
                                             Pd.data_ptr(), _f32(vb_f).data_ptr(), _f32(vb_r).data_ptr(), ctx_t.data_ptr(), st),
                   "bl_rel_value_bias_fwd")
        out = ctx_t.view(B, H, L, dk).permute(0, 2, 1, 3).contiguous().view(B * L, D)
        ctx.fused = bool(_switches.FUSED_ATTENTION and mode == 0 and vb_f is None and lib.bl_rel_attn_probs_ok(L, dk, T))
        ctx.mm32 = mm32
        ctx.saved = (qs, kt, vt, P, Pd, lens, edges, bias_f, bias_r, vb_f, vb_r, B, L, H, dk, T, mode, drop, gptr, scale)
        return out

    @staticmethod
    def backward(ctx, g_out):
        if ctx.path == "stream":
            return _stream_attention_bwd(ctx, g_out)
        qs, kt, vt, P, Pd, lens, edges, bias_f, bias_r, vb_f, vb_r, B, L, H, dk, T, mode, drop, gptr, scale = _take_saved(ctx)
        lib = load_library()
        G, D = B * H, H * dk
        dev = g_out.device
        st = _stream()
        g_ct = g_out.view(B, L, H, dk).permute(0, 2, 1, 3).contiguous().view(G * L, dk)
        mm32 = ctx.mm32
        g3 = (torch.empty if mm32 else torch.zeros)((3, B, H, L, dk), dtype=torch.float32, device=dev)
        g_qs, g_k, g_v = g3[0], g3[1], g3[2]

        def tn(a, bm, out):  # out[g] = a[g]^T . bm[g]
            if mm32:
                with _timed("attn_transposed_times", 2.0 * G * L * L * dk, nbytes=4.0 * G * L * (L + 2 * dk)):
                    _check(lib.bl_attn_transposed_times(a.data_ptr(), bm.data_ptr(), G, L, dk, out.data_ptr(), st), "bl_attn_transposed_times")
            else:
                gemm_wgrad([(a, None)], bm.view(G * L, dk), G * L, dk, out.view(G, L, dk), gw_group_stride=L * dk, group_ptr=gptr, G=G)

        tn(Pd, g_ct, g_v)
        has_e = edges.num_entries > 0
        ep = (edges.row_ptr.data_ptr(), edges.key.data_ptr(), edges.code.data_ptr()) if has_e else None
        if ctx.fused:
            # dO.V^T, dropout mask, softmax backward and the edge terms' gradients in one kernel; dS is written once
            (g_bf, r_bf), (g_br, r_br) = _grad_target(bias_f), _grad_target(bias_r)
            dS = torch.empty((G * L, L), dtype=torch.float32, device=dev)
            gq_edge = torch.empty((G * L, dk), dtype=torch.float32, device=dev) if has_e else None  # (the kernel writes every row)
            with _timed("attn_probs_bwd", 0.0, nbytes=4.0 * G * L * (2 * L + 3 * dk)):  # reads P, dO, v, q; writes dS
                _check(lib.bl_rel_attn_probs_bwd(g_ct.data_ptr(), vt.data_ptr(), P.data_ptr(), qs.data_ptr(), *(ep or (None, None, None)), B, L, H, dk, T,
                                                 bias_f.data_ptr(), bias_r.data_ptr(), drop.c(), dS.data_ptr(), _p(gq_edge), g_bf.data_ptr(),
                                                 g_br.data_ptr(), st), "bl_rel_attn_probs_bwd")
            if mm32:  # dQ = (dS.K + edge part) * scale in one kernel
                with _timed("attn_rows_times", 2.0 * G * L * L * dk, nbytes=4.0 * G * L * (L + 2 * dk)):
                    _check(lib.bl_attn_rows_times(dS.data_ptr(), kt.data_ptr(), G, L, dk, _p(gq_edge), scale, g_qs.data_ptr(), st), "bl_attn_rows_times")
            else:
                gemm_rows([(dS, None)], kt, G * L, dk, b_group_stride=L * dk, ldb=dk, group_ptr=gptr, G=G, out=g_qs.view(G * L, dk))
                if has_e:
                    g_qs.view(G * L, dk).add_(gq_edge)
                g_qs.mul_(scale)
            tn(dS, qs, g_k)
            g_qkv = g3.permute(1, 3, 2, 0, 4).contiguous().view(B * L, 3 * D)
            return g_qkv, None, None, r_bf, r_br, None, None, None, None, None, None, None, None, None
        dP = gemm_rows([(g_ct, None)], vt, G * L, L, b_is_nk=True, b_group_stride=L * dk, ldb=dk, group_ptr=gptr, G=G)
        r_vbf = r_vbr = None
        if vb_f is not None:
            (g_vbf, r_vbf), (g_vbr, r_vbr) = _grad_target(vb_f), _grad_target(vb_r)
            if has_e:
                _check(lib.bl_rel_value_bias_bwd(*ep, B, L, H, dk, T, Pd.data_ptr(), g_ct.data_ptr(), vb_f.data_ptr(), vb_r.data_ptr(),
                                                 dP.data_ptr(), g_vbf.data_ptr(), g_vbr.data_ptr(), st), "bl_rel_value_bias_bwd")
        _check(lib.bl_softmax_dropout_bwd(P.data_ptr(), dP.data_ptr(), G * L, L, drop.c(), st), "bl_softmax_dropout_bwd")  # (mask, then softmax')
        dS = dP
        if mm32:
            _check(lib.bl_attn_rows_times(dS.data_ptr(), kt.data_ptr(), G, L, dk, None, 1.0, g_qs.data_ptr(), st), "bl_attn_rows_times")
        else:
            gemm_rows([(dS, None)], kt, G * L, dk, b_group_stride=L * dk, ldb=dk, group_ptr=gptr, G=G, out=g_qs.view(G * L, dk))
        tn(dS, qs, g_k)
        (g_bf, r_bf), (g_br, r_br) = _grad_target(bias_f), _grad_target(bias_r)
        if has_e:
            _check(lib.bl_rel_attn_bias_bwd(*ep, B, L, H, dk, mode, T, (kt if mode == 1 else qs).data_ptr(), bias_f.data_ptr(),
                                            bias_r.data_ptr(), dS.data_ptr(), g_qs.data_ptr(), g_k.data_ptr(), g_bf.data_ptr(),
                                            g_br.data_ptr(), st), "bl_rel_attn_bias_bwd")
        g_qs.mul_(scale)
        g_qkv = g3.permute(1, 3, 2, 0, 4).contiguous().view(B * L, 3 * D)
        return g_qkv, None, None, r_bf, r_br, r_vbf, r_vbr, None, None, None, None, None, None, None


def rel_attention(qkv, lens, edges: RelEdges, bias_f, bias_r, vb_f, vb_r, B, L, H, dk, T, scalar_bias=False, drop: Dropout = NO_DROPOUT):
    """qkv [B*L, H*3*dk] (per head [q | k | v]) -> attention context [B*L, H*dk]."""
    return _RelAttention.apply(qkv.contiguous(), lens, edges, bias_f, bias_r, vb_f, vb_r, int(B), int(L), int(H), int(dk), int(T),
                               bool(scalar_bias), drop)


# ---- `seq-gru`: the time recurrence of one bidirectional GRU layer (csrc/bl_gru_scan.hip) -------------------------------------
class _GruScan(torch.autograd.Function):
    """gi [B L, 6 Hh] (x W_ih + b_ih of both directions, columns [direction][r | z | n]) -> h_t of both directions [B L, 2 Hh] with
    torch.nn.GRU's PackedSequence semantics (reference seqmodel.py:385-392).  Backward: one reverse scan (bl_gru_scan_bwd) gives the
    gradient of gi and of the recurrent pre-activations; the recurrent weight gradient h_prev^T d_gh is a weight-gradient GEMM."""

    @staticmethod
    def forward(ctx, gi, W_hh, b_hh, lens, B, L):
        lib = load_library()
        _f32(gi, "gi")
        Hh = W_hh.shape[1]
        R = B * L
        assert gi.shape == (R, 6 * Hh) and W_hh.shape == (2, Hh, 3 * Hh) and b_hh.shape == (2, 3 * Hh)
        need_bwd = any(ctx.needs_input_grad)
        out = torch.empty((R, 2 * Hh), dtype=torch.float32, device=gi.device)
        saved = torch.empty((lib.bl_gru_scan_saved_elems(B, L, Hh),), dtype=torch.float32, device=gi.device) if need_bwd else None
        _check(lib.bl_gru_scan_fwd(gi.data_ptr(), gi.stride(0), _f32(W_hh.contiguous()).data_ptr(), _f32(b_hh.contiguous()).data_ptr(),
                                   _i32(lens).data_ptr(), B, L, Hh, out.data_ptr(), out.stride(0), _p(saved), _stream()), "bl_gru_scan_fwd")
        ctx.saved = (W_hh, lens, B, L, Hh, saved)
        return out

    @staticmethod
    def backward(ctx, g_out):
        W_hh, lens, B, L, Hh, saved = _take_saved(ctx)
        lib = load_library()
        R = B * L
        dev = g_out.device
        g_out = g_out.contiguous()
        g_gi = torch.empty((R, 6 * Hh), dtype=torch.float32, device=dev)
        g_gh = torch.empty((2, R, 3 * Hh), dtype=torch.float32, device=dev)
        _check(lib.bl_gru_scan_bwd(g_out.data_ptr(), g_out.stride(0), _f32(W_hh.contiguous()).data_ptr(), saved.data_ptr(), _i32(lens).data_ptr(),
                                   B, L, Hh, g_gi.data_ptr(), g_gi.stride(0), g_gh.data_ptr(), _stream()), "bl_gru_scan_bwd")
        g_W = torch.zeros_like(W_hh)
        h_prev = saved[2 * R * 4 * Hh:].view(2, R, Hh)
        for d in range(2):
            gemm_wgrad([(h_prev[d], None)], g_gh[d], R, 3 * Hh, g_W[d])  # h_prev^T . d_gh
        return g_gi, g_W, g_gh.sum(1), None, None, None


def gru_scan(gi, W_hh, b_hh, lens, B: int, L: int):
    return _GruScan.apply(gi.contiguous(), W_hh, b_hh, lens, int(B), int(L))


# ---- one relational transformer encoder layer per C call (csrc/bl_great_layer.hip) ----------------------------------------
def great_layer_ok(B: int, L: int, H: int, dk: int, T: int, FF: int) -> bool:
    """Whether bl_great_layer_fwd / _bwd take the shape (the caller also checks the layer's configuration: postnorm, rezero
    off, vector query bias, no value biases)."""
    return bool(_switches.FUSED_GREAT_LAYER and _switches.LINEAR_X6 and _switches.GEMM_MODE == "bf16x6"
                and load_library().bl_great_layer_ok(int(B), int(L), int(H), int(dk), int(T), int(FF)))


def _great_desc(B, L, H, dk, T, FF, lens, edges: "RelEdges", bias_f, bias_r, norm_g, norm_b, lin1_b, lin2_b, packs, drops) -> bl_great_layer_t:
    d = bl_great_layer_t()
    d.B, d.L, d.H, d.dk, d.T, d.FF = int(B), int(L), int(H), int(dk), int(T), int(FF)
    if edges.num_entries > 0:
        d.row_ptr, d.ekey, d.ecode = _i32(edges.row_ptr).data_ptr(), _i32(edges.key).data_ptr(), _i32(edges.code).data_ptr()
    d.lens = _i32(lens).data_ptr()
    d.bias_f, d.bias_r = _f32(bias_f).data_ptr(), _f32(bias_r).data_ptr()
    d.norm_g, d.norm_b, d.lin1_b, d.lin2_b = _f32(norm_g).data_ptr(), _f32(norm_b).data_ptr(), _f32(lin1_b).data_ptr(), _f32(lin2_b).data_ptr()
    (qkv, qkv_b), (out, out_b), (l1, l1_b), (l2, l2_b) = packs
    d.qkv_w, d.out_w, d.lin1_w, d.lin2_w = qkv.data_ptr(), out.data_ptr(), l1.data_ptr(), l2.data_ptr()
    d.qkv_w_bwd, d.out_w_bwd, d.lin1_w_bwd, d.lin2_w_bwd = _p(qkv_b), _p(out_b), _p(l1_b), _p(l2_b)
    d.ln_eps = 1e-5
    d.drop_attn, d.drop_att_out, d.drop_ff_hidden, d.drop_ff_out = (x.c() for x in drops)
    return d


class _GreatLayer(torch.autograd.Function):
    """RelationalTransformerEncoderLayer.forward ("postnorm", rezero off, vector query bias) = one C call forward, one backward.
    `chain` carries the packed form of the activations from layer to layer: chain["packed"] is bl_pack_bf16x3 of THIS layer's
    input if chain["of"] is that tensor's address (written by the previous layer's call), and is replaced by the packed output."""

    @staticmethod
    def forward(ctx, x, qkv_W, out_W, bias_f, bias_r, lin1_W, lin1_b, lin2_W, lin2_b, norm_g, norm_b, lens, edges, dims, drops, chain):
        lib = load_library()
        _f32(x, "x")
        B, L, H, dk, T, FF = dims
        R, D = x.shape
        dev = x.device
        need_bwd = any(ctx.needs_input_grad)
        packs = [_packed_layer_weights(_f32(W, "W"), need_bwd) for W in (qkv_W, out_W, lin1_W, lin2_W)]
        d = _great_desc(B, L, H, dk, T, FF, lens, edges, bias_f, bias_r, norm_g, norm_b, lin1_b, lin2_b, packs, drops)
        xp = chain.get("packed") if (chain is not None and chain.get("of") == (x.data_ptr(), x._version)) else None
        saved = (torch.empty((lib.bl_great_layer_saved_bytes(B, L, H, dk, FF, 1 if xp is None else 0),),
                             dtype=torch.uint8, device=dev) if need_bwd else None)
        ws = torch.empty((lib.bl_great_layer_workspace_bytes(B, L, H, dk, FF, 0 if need_bwd else 3),), dtype=torch.uint8, device=dev)
        out = torch.empty_like(x)
        outp = torch.empty((R, 3 * D), dtype=torch.int16, device=dev) if chain is not None else None
        _check(lib.bl_great_layer_fwd(ctypes.byref(d), x.data_ptr(), _p(xp), out.data_ptr(), _p(outp), _p(saved), ws.data_ptr(), _stream()),
               "bl_great_layer_fwd")
        if chain is not None:
            chain["packed"], chain["of"] = outp, (out.data_ptr(), out._version)
        ctx.saved = (qkv_W, out_W, bias_f, bias_r, lin1_W, lin1_b, lin2_W, lin2_b, norm_g, norm_b, lens, edges, dims, drops, xp, saved, packs)
        ctx.seq_mode = _seq_gemm_mode_code()
        return out

    @staticmethod
    def backward(ctx, g_out):
        (qkv_W, out_W, bias_f, bias_r, lin1_W, lin1_b, lin2_W, lin2_b, norm_g, norm_b, lens, edges, dims, drops, xp, saved,
         packs) = _take_saved(ctx)
        lib = load_library()
        B, L, H, dk, T, FF = dims
        dev = g_out.device
        packs = [p if p[1] is not None else _packed_layer_weights(W, True) for p, W in zip(packs, (qkv_W, out_W, lin1_W, lin2_W))]
        d = _great_desc(B, L, H, dk, T, FF, lens, edges, bias_f, bias_r, norm_g, norm_b, lin1_b, lin2_b, packs, drops)
        params = (qkv_W, out_W, lin1_W, lin1_b, lin2_W, lin2_b, norm_g, norm_b, bias_f, bias_r)
        targets = [_grad_target(p) for p in params]
        g = bl_great_layer_grads_t()
        (g.qkv_w, g.out_w, g.lin1_w, g.lin1_b, g.lin2_w, g.lin2_b, g.norm_g, g.norm_b, g.bias_f, g.bias_r) = (t[0].data_ptr() for t in targets)
        ws = torch.empty((lib.bl_great_layer_workspace_bytes(B, L, H, dk, FF, 1),), dtype=torch.uint8, device=dev)
        g_x = torch.empty((B * L, H * dk), dtype=torch.float32, device=dev)
        side = _streams.side_stream_for_current_device()
        with _in_seq_gemm_mode(ctx.seq_mode):
            _check(lib.bl_great_layer_bwd(ctypes.byref(d), _p(xp), _f32(g_out.contiguous()).data_ptr(), saved.data_ptr(), ws.data_ptr(),
                                          g_x.data_ptr(), ctypes.byref(g), _stream(), side.cuda_stream if side is not None else None),
                   "bl_great_layer_bwd")
        r = {id(p): t[1] for p, t in zip(params, targets)}
        return (g_x, r[id(qkv_W)], r[id(out_W)], r[id(bias_f)], r[id(bias_r)], r[id(lin1_W)], r[id(lin1_b)], r[id(lin2_W)], r[id(lin2_b)],
                r[id(norm_g)], r[id(norm_b)], None, None, None, None, None)


def great_layer(x, qkv_W, out_W, bias_f, bias_r, lin1_W, lin1_b, lin2_W, lin2_b, norm_g, norm_b, lens, edges: RelEdges, B, L, H, dk, T,
                drops=(NO_DROPOUT,) * 4, chain: Optional[dict] = None):
    """out = norm1(x1 + drop(linear2(drop(relu(linear1(x1)))))), x1 = norm1(x + drop(out_proj(rel_attention(qkv_proj(x))))) --
    reference relational_transformer.py:104-124 (postnorm; both sublayers normalised by norm1).  drops = (attention
    probabilities, attention branch, inside the feed-forward block, feed-forward branch)."""
    FF = lin1_W.shape[1]
    return _GreatLayer.apply(x.contiguous(), qkv_W, out_W, bias_f, bias_r, lin1_W, lin1_b, lin2_W, lin2_b, norm_g, norm_b, lens, edges,
                             (int(B), int(L), int(H), int(dk), int(T), int(FF)), tuple(drops), chain)
