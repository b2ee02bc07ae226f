"""Raw (non-autograd) entry points of buglab.models.hip_ops: the row GEMMs (exact fp32, bf16x6, f16x3), their operand packers
and weight-gradient forms, the routed forms of the max-aggregated messages and the row-wise kernels next to them."""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from . import _switches
from ._cabi import ACT_NONE, _check, Dropout, _f32, _i32, load_library, NO_DROPOUT, _p, _req, _rows, _rows_packed, _stream
from ._streams import _timed

__all__ = ["gemm_rows", "pack_bf16x3", "pack_weights_x6", "rows_x6w_ok", "pack_weights_x6w", "gemm_rows_x6", "H3_ROW_SCALE",
           "H3_W_SCALE", "pack_f16x2", "h3_saturation_events", "amax", "pack_weights_h3", "gemm_rows_h3", "gemm_wgrad_h3",
           "gemm_wgrad_routed_x6", "gemm_wgrad_x6", "x6_ok", "gemm_rows_routed", "gemm_wgrad_routed", "gemm_wgrad",
           "segment_max", "segment_max_bwd", "layernorm_bwd", "act_bwd", "scatter_add_rows", "routed_dgrad_vec",
           "routed_dgrad_nodes"]


# ------------------------------------------------------------------------------------------------
# raw (non-autograd) entry points
def gemm_rows(sources, b, M, N, *, b_is_nk=False, b_group_stride=0, ldb=None, bias=None, group_ptr=None, group_w=None,
              G=1, act=ACT_NONE, drop: Dropout = NO_DROPOUT, out=None):
    rows, K = _rows(sources)
    _f32(b, "b")
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=b.device)
    if M == 0:
        return out
    kind = ("gemm_rows_nk" if b_is_nk else "gemm_rows") + ("_grouped" if group_ptr is not None else "")
    with _timed(kind, 2.0 * M * N * K):
        _check(
            load_library().bl_gemm_rows(
                ctypes.byref(rows), b.data_ptr(), int(b_group_stride), int(ldb if ldb is not None else b.shape[-1]), int(b_is_nk),
                _p(bias), _p(group_ptr), _p(group_w), int(G), int(M), int(N), int(K), int(act), drop.c(), out.data_ptr(),
                out.stride(0), _stream()),
            "bl_gemm_rows")
    return out


# ------------------------------------------------------------------------------------------------
# fp32-accurate GEMM on the bf16 matrix cores (csrc/bl_gemm_x6.hip)
def pack_bf16x3(x: torch.Tensor) -> torch.Tensor:
    """fp32 [R, D] -> packed int16 [R, 3 * D]: per row the three bf16 planes [hi x D | mid x D | lo x D]."""
    _f32(x, "x")
    R, D = x.shape
    out = torch.empty((R, 3 * D), dtype=torch.int16, device=x.device)
    _check(load_library().bl_pack_bf16x3(x.data_ptr(), x.stride(0), R, D, out.data_ptr(), _stream()), "bl_pack_bf16x3")
    return out


def pack_weights_x6(w: torch.Tensor, w_is_kn: bool) -> torch.Tensor:
    """fp32 weights -> the tiled packed B operand of gemm_rows_x6 (int16 [G, tiles * stages * 12288]).
    w is [G, K, N] when w_is_kn (C = A @ w[g]) or [G, N, K] (C = A @ w[g]^T)."""
    _f32(w, "w")
    G, K, N = (w.shape[0], w.shape[1], w.shape[2]) if w_is_kn else (w.shape[0], w.shape[2], w.shape[1])
    out = torch.empty((G, ((N + 127) // 128) * (K // 32) * 12288), dtype=torch.int16, device=w.device)
    _check(load_library().bl_pack_weights_x6(w.data_ptr(), G, K, N, 1 if w_is_kn else 0, out.data_ptr(), _stream()), "bl_pack_weights_x6")
    return out


def rows_x6w_ok(N: int, K: int) -> bool:
    """Shapes the wide row GEMM takes (bl_gemm_rows_x6w_ok: N a multiple of 256, K of 64)."""
    return bool(load_library().bl_gemm_rows_x6w_ok(int(N), int(K)))


def pack_weights_x6w(w: torch.Tensor, w_is_kn: bool) -> torch.Tensor:
    """fp32 weights -> the weight image of gemm_rows_x6(..., wide=True) (bl_pack_weights_x6w; same shapes as pack_weights_x6)."""
    _f32(w, "w")
    G, K, N = (w.shape[0], w.shape[1], w.shape[2]) if w_is_kn else (w.shape[0], w.shape[2], w.shape[1])
    lib = load_library()
    out = torch.empty((G, int(lib.bl_packed_weight_elems_x6w(1, K, N))), dtype=torch.int16, device=w.device)
    _check(lib.bl_pack_weights_x6w(w.data_ptr(), G, K, N, 1 if w_is_kn else 0, out.data_ptr(), _stream()), "bl_pack_weights_x6w")
    return out


def gemm_rows_x6(sources, bp, M, N, *, group_ptr=None, group_w=None, G=1, win_bits=None, kind="gemm_rows_x6", bias=None, act=None,
                 drop: "Dropout" = None, wide: bool = False):
    """sources: [(packed int16 [*, 3*width], row index or None, width)]; bp: pack_weights_x6 output [G, *];
    win_bits: segment_max's per-row routing bitmask -> the routed (winner-masked) left operand;
    bias / act / drop: the epilogue drop(act(. + bias)) of bl_gemm_rows_x6_epi."""
    r, K = _rows_packed(sources)
    out = torch.empty((M, N), dtype=torch.float32, device=bp.device)
    if M == 0:
        return out
    if bias is not None or act is not None or drop is not None:
        with _timed(kind + "_epi", 2.0 * M * N * K):
            _check(
                load_library().bl_gemm_rows_x6_epi(ctypes.byref(r), _req(bp, torch.int16, "bp").data_ptr(), int(bp.stride(0)), _p(group_ptr),
                                                   _p(group_w), int(G), int(M), int(N), int(K), _p(bias), int(act or ACT_NONE),
                                                   (drop or NO_DROPOUT).c(), out.data_ptr(), out.stride(0), _stream()),
                "bl_gemm_rows_x6_epi")
        return out
    if wide:  # bp = pack_weights_x6w(...): the 128 x 256-tile kernel (bit-identical results)
        with _timed(kind + ("_grouped" if group_ptr is not None else ""), 2.0 * M * N * K):
            _check(
                load_library().bl_gemm_rows_x6w(ctypes.byref(r), _p(win_bits), win_bits.stride(0) if win_bits is not None else 0,
                                                _req(bp, torch.int16, "bp").data_ptr(), int(bp.stride(0)), _p(group_ptr), _p(group_w),
                                                int(G), int(M), int(N), int(K), out.data_ptr(), out.stride(0), _stream()),
                "bl_gemm_rows_x6w")
        return out
    with _timed(kind + ("_grouped" if group_ptr is not None else ""), 2.0 * M * N * K):
        _check(
            load_library().bl_gemm_rows_x6(ctypes.byref(r), _p(win_bits), win_bits.stride(0) if win_bits is not None else 0,
                                           _req(bp, torch.int16, "bp").data_ptr(), int(bp.stride(0)), _p(group_ptr), _p(group_w),
                                           int(G), int(M), int(N), int(K), out.data_ptr(), out.stride(0), _stream()),
            "bl_gemm_rows_x6")
    return out


# ------------------------------------------------------------------------------------------------
# f16x3: fp32-accurate GEMMs on the fp16 matrix cores (csrc/bl_gemm_h3.hip) -- two fp16 planes per operand, three MFMA terms,
# power-of-two tensor scales.  H3_ROW_SCALE: layer inputs (|h| <= 1.25 after tanh x dropout; embedding rows), H3_W_SCALE: weights.
H3_ROW_SCALE = 256.0
H3_W_SCALE = 64.0


def pack_f16x2(x: torch.Tensor, scale: float = H3_ROW_SCALE, amax: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[R, D] fp32 -> [R, 2 D] int16 (hi plane | lo plane of x * scale; amax: device float with max |x| -> the scale is derived on
    the device, the consumer GEMM takes the same tensor as `a_amax` / `g_amax`)."""
    _f32(x, "x")
    R, D = x.shape
    out = torch.empty((R, 2 * D), dtype=torch.int16, device=x.device)
    _check(load_library().bl_pack_f16x2(x.data_ptr(), x.stride(0), int(R), int(D), int(D), 0, float(scale), _p(amax), out.data_ptr(), _stream()),
           "bl_pack_f16x2")
    return out


def h3_saturation_events(reset: bool = False) -> int:
    """f16x2 packing threads that had to saturate a finite value since the last reset on the current device (synchronises): 0 in a
    healthy run -- a layer input beyond +-255.9 or a weight beyond +-1023 would count (bl_h3_saturation_events)."""
    return int(load_library().bl_h3_saturation_events(1 if reset else 0))


def amax(x: torch.Tensor) -> torch.Tensor:
    """device float [1] = max |x| (bl_amax)"""
    _f32(x, "x")
    out = torch.zeros((1,), dtype=torch.float32, device=x.device)
    _check(load_library().bl_amax(x.data_ptr(), int(x.numel()), out.data_ptr(), _stream()), "bl_amax")
    return out


def pack_weights_h3(w: torch.Tensor, w_is_kn: bool, scale: float = H3_W_SCALE) -> torch.Tensor:
    """w [G, K, N] (w_is_kn) or [G, N, K] -> tiled f16x2 image [G, *] int16 (bl_pack_weights_h3)"""
    _f32(w, "w")
    G, K, N = (w.shape[0], w.shape[1], w.shape[2]) if w_is_kn else (w.shape[0], w.shape[2], w.shape[1])
    lib = load_library()
    out = torch.empty((G, int(lib.bl_packed_weight_elems_h3(1, K, N))), dtype=torch.int16, device=w.device)
    _check(lib.bl_pack_weights_h3(w.data_ptr(), G, K, N, 1 if w_is_kn else 0, float(scale), out.data_ptr(), _stream()), "bl_pack_weights_h3")
    return out


def gemm_rows_h3(sources, bp, M, N, *, out_scale, group_ptr=None, group_w=None, G=1, win_bits=None, a_amax=None, kind="gemm_rows_h3"):
    """sources: [(pack_f16x2 rows, row index or None, width)]; bp: pack_weights_h3 image; out_scale = 1 / (row scale x weight scale)"""
    r, K = _rows_packed(sources)
    out = torch.empty((M, N), dtype=torch.float32, device=bp.device)
    if M == 0:
        return out
    with _timed(kind + ("_grouped" if group_ptr is not None else ""), 2.0 * M * N * K):
        _check(load_library().bl_gemm_rows_h3(ctypes.byref(r), _p(win_bits), int(win_bits.stride(0)) if win_bits is not None else 0,
                                              _req(bp, torch.int16, "bp").data_ptr(), int(bp.stride(0)), _p(group_ptr), _p(group_w), int(G),
                                              int(M), int(N), int(K), float(out_scale), _p(a_amax), out.data_ptr(), out.stride(0), _stream()),
               "bl_gemm_rows_h3")
    return out


def gemm_wgrad_h3(sources, g_packed, M, N, gw, *, out_scale, g_idx=None, win_bits=None, g_amax=None, gw_group_stride=0, group_ptr=None,
                  group_w=None, G=1):
    """gw[g] += out_scale * rows(sources)^T . G rows (g_idx gather, win_bits routing): bl_gemm_wgrad_h3"""
    r, K = _rows_packed(sources)
    if M == 0:
        return gw
    with _timed("gemm_wgrad_h3", 2.0 * M * N * K):
        _check(load_library().bl_gemm_wgrad_h3(ctypes.byref(r), _req(g_packed, torch.int16, "g_packed").data_ptr(), _p(g_idx), _p(win_bits),
                                               int(win_bits.stride(0)) if win_bits is not None else 0, _p(group_ptr), _p(group_w), int(G), int(M),
                                               int(N), int(K), float(out_scale), _p(g_amax), gw.data_ptr(), int(gw_group_stride), int(gw.stride(-2)),
                                               _stream()), "bl_gemm_wgrad_h3")
    return gw


def gemm_wgrad_routed_x6(sources, g_node_packed, node_of_row, win_bits, M, N, gw, *, gw_group_stride=0, group_ptr=None, group_w=None, G=1):
    """bf16x6 weight gradient of the routed (max-aggregated) messages; accumulates into gw."""
    rows, K = _rows_packed(sources)
    if M == 0:
        return gw
    with _timed("gemm_wgrad_routed_x6", 2.0 * M * N * K):
        _check(
            load_library().bl_gemm_wgrad_routed_x6(ctypes.byref(rows), _req(g_node_packed, torch.int16, "g_node_packed").data_ptr(),
                                                   _i32(node_of_row).data_ptr(), _i32(win_bits).data_ptr(), win_bits.stride(0),
                                                   _p(group_ptr), _p(group_w), int(G), int(M), int(N), int(K),
                                                   _f32(gw).data_ptr(), int(gw_group_stride), int(gw.shape[-1]), _stream()),
            "bl_gemm_wgrad_routed_x6")
    return gw


def gemm_wgrad_x6(sources, g_packed, M, N, gw, *, g_idx=None, gw_group_stride=0, group_ptr=None, group_w=None, G=1):
    """gw[g] += rows(sources)^T . g_packed[(g_idx[r] or r)] from bf16x3-packed operands (no routing): the weight gradient of a
    plain Linear.  sources as in gemm_rows_x6; g_packed int16 [*, 3 N]."""
    r, K = _rows_packed(sources)
    if M == 0:
        return gw
    with _timed("gemm_wgrad_x6", 2.0 * M * N * K):
        _check(
            load_library().bl_gemm_wgrad_x6(ctypes.byref(r), _req(g_packed, torch.int16, "g_packed").data_ptr(), _p(g_idx), _p(group_ptr),
                                            _p(group_w), int(G), int(M), int(N), int(K), _f32(gw, "gw").data_ptr(), int(gw_group_stride),
                                            int(gw.shape[-1]), _stream()),
            "bl_gemm_wgrad_x6")
    return gw


def x6_ok(*dims) -> bool:
    return _switches.GEMM_MODE == "bf16x6" and all(d % 32 == 0 for d in dims)


def gemm_rows_routed(g_node, node_of_row, winner, b, M, N, *, b_group_stride=0, ldb=None, group_ptr=None, group_w=None, G=1):
    """C[r, :] = (g_node[node_of_row[r]] masked to the entries row r won) . B_g^T  (include/buglab_hip.h)."""
    rows, K = _rows([(g_node, node_of_row)])
    out = torch.empty((M, N), dtype=torch.float32, device=b.device)
    if M == 0:
        return out
    with _timed("gemm_rows_nk_routed", 2.0 * M * N * K):
        _check(
            load_library().bl_gemm_rows_routed(ctypes.byref(rows), _i32(winner).data_ptr(), winner.stride(0), _f32(b).data_ptr(),
                                               int(b_group_stride), int(ldb if ldb is not None else b.shape[-1]), _p(group_ptr),
                                               _p(group_w), int(G), int(M), int(N), int(K), out.data_ptr(), out.stride(0), _stream()),
            "bl_gemm_rows_routed")
    return out


def gemm_wgrad_routed(sources, g_node, node_of_row, winner, M, N, gw, *, gw_group_stride=0, group_ptr=None, group_w=None, G=1):
    rows, K = _rows(sources)
    if M == 0:
        return gw
    with _timed("gemm_wgrad_routed", 2.0 * M * N * K):
        _check(
            load_library().bl_gemm_wgrad_routed(ctypes.byref(rows), _f32(g_node).data_ptr(), g_node.stride(0),
                                                _i32(node_of_row).data_ptr(), _i32(winner).data_ptr(), winner.stride(0),
                                                _p(group_ptr), _p(group_w), int(G), int(M), int(N), int(K), _f32(gw).data_ptr(),
                                                int(gw_group_stride), int(gw.shape[-1]), _stream()),
            "bl_gemm_wgrad_routed")
    return gw


def gemm_wgrad(sources, g_c, M, N, gw, *, gw_group_stride=0, group_ptr=None, group_w=None, G=1):
    rows, K = _rows(sources)
    _f32(g_c, "g_c")
    _f32(gw, "gw")
    if M == 0:
        return gw
    with _timed("gemm_wgrad" + ("_grouped" if group_ptr is not None else ""), 2.0 * M * N * K):
        _check(
            load_library().bl_gemm_wgrad(ctypes.byref(rows), g_c.data_ptr(), g_c.stride(0), _p(group_ptr), _p(group_w), int(G),
                                         int(M), int(N), int(K), gw.data_ptr(), int(gw_group_stride), int(gw.shape[-1]), _stream()),
            "bl_gemm_wgrad")
    return gw


def segment_max(x, seg_ptr, seg_items, nseg, act=ACT_NONE, ln=None, eps=1e-5, want_dact=False, want_bits=False, seg_order=None):
    """-> (out [nseg, D], arg int32 [nseg, D], ln_out | None, mean | None, rstd | None[, dact][, winbits])

    winbits: int32 [items, ceil(D/32)], bit d of row i set iff item i won channel d of its segment
    (every item must belong to exactly one segment)."""
    _f32(x, "x")
    D = x.shape[1]
    dev = x.device
    out = torch.empty((nseg, D), dtype=torch.float32, device=dev)
    arg = torch.empty((nseg, D), dtype=torch.int32, device=dev)
    ln_out = mean = rstd = None
    if ln is not None:
        ln_out = torch.empty((nseg, D), dtype=torch.float32, device=dev)
        mean = torch.empty((nseg,), dtype=torch.float32, device=dev)
        rstd = torch.empty((nseg,), dtype=torch.float32, device=dev)
    dact = torch.empty((nseg, D), dtype=torch.float32, device=dev) if want_dact else None
    bits = torch.empty((x.shape[0], (D + 31) // 32), dtype=torch.int32, device=dev) if want_bits else None
    _check(
        load_library().bl_segment_max_fwd(x.data_ptr(), x.stride(0), _i32(seg_ptr).data_ptr(), _p(seg_items), int(nseg), int(D),
                                          int(act), out.data_ptr(), arg.data_ptr(), _p(ln[0]) if ln else None,
                                          _p(ln[1]) if ln else None, float(eps), _p(ln_out), _p(mean), _p(rstd), _p(dact), _p(bits), _p(seg_order), _stream()),
        "bl_segment_max_fwd")
    res = (out, arg, ln_out, mean, rstd)
    if want_dact:
        res += (dact,)
    if want_bits:
        res += (bits,)
    return res


def segment_max_bwd(g_out, arg, x, seg_of, act=ACT_NONE, out=None):
    nitems, D = x.shape
    if out is None:
        out = torch.empty_like(x)
    _check(
        load_library().bl_segment_max_bwd(_f32(g_out).data_ptr(), _i32(arg).data_ptr(), x.data_ptr(), x.stride(0),
                                          _i32(seg_of).data_ptr(), int(nitems), int(D), int(act), out.data_ptr(), _stream()),
        "bl_segment_max_bwd")
    return out


def layernorm_bwd(g_y, x, mean, rstd, gamma, g_gamma, g_beta, post_scale=None, want="f32"):
    """want: "f32" -> g_x; "packed" -> bf16x3-packed g_x only (int16 [n, 3 D]); "both" -> (g_x, packed)."""
    n, D = x.shape
    g_x = torch.empty_like(x) if want != "packed" else None
    g_xp = torch.empty((n, 3 * D), dtype=torch.int16, device=x.device) if want != "f32" else None
    _check(
        load_library().bl_layernorm_bwd(_f32(g_y).data_ptr(), _f32(x).data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                        _f32(gamma).data_ptr(), int(n), int(D), _p(g_x), g_gamma.data_ptr(),
                                        g_beta.data_ptr(), _p(post_scale), _p(g_xp), _stream()),
        "bl_layernorm_bwd")
    return g_x if want == "f32" else (g_xp if want == "packed" else (g_x, g_xp))


def act_bwd(g_y, y, act, drop: Dropout = NO_DROPOUT, g_bias=None):
    n, N = y.shape
    g_z = torch.empty_like(y)
    _check(
        load_library().bl_act_bwd(_f32(g_y).data_ptr(), _f32(y).data_ptr(), int(n), int(N), y.stride(0), int(act), drop.c(),
                                  g_z.data_ptr(), _p(g_bias), _stream()),
        "bl_act_bwd")
    return g_z


def scatter_add_rows(src, col_off, width, idx, out):
    R = src.shape[0]
    _check(
        load_library().bl_scatter_add_rows(_f32(src).data_ptr(), src.stride(0), int(col_off), int(width), _i32(idx).data_ptr(),
                                           int(R), _f32(out).data_ptr(), out.stride(0), _stream()),
        "bl_scatter_add_rows")
    return out


def routed_dgrad_vec(gq, msg_tgt, win_bits, type_ptr, T, wt, E, K2):
    """g_a [E, K2] = routed message gradient x W^T from its non-zeros only (vector units; csrc/bl_routed_dgrad.hip).
    gq [N, Dm] fp32, wt [T, Dm, K2] = W transposed, win_bits [E, Dm/32] from segment_max."""
    Dm = gq.shape[1]
    out = torch.empty((E, K2), dtype=torch.float32, device=gq.device)
    with _timed("msg_dgrad_vec", 2.0 * gq.shape[0] * Dm * K2):
        _check(load_library().bl_routed_dgrad_vec(_f32(gq).data_ptr(), gq.stride(0), _i32(msg_tgt).data_ptr(), win_bits.data_ptr(),
                                                 win_bits.stride(0), _i32(type_ptr).data_ptr(), int(T), _f32(wt).data_ptr(), int(E), Dm,
                                                 int(K2), out.data_ptr(), out.stride(0), _stream()), "bl_routed_dgrad_vec")
    return out


def routed_dgrad_nodes(gq, msg_src, msg_tgt, win_bits, type_ptr, T, wt, E, Din, out_lo, out_hi=None, src_rows=None):
    """Adds the routed input gradient straight into the node gradient out_lo [N, split] (+ out_hi [N, Din - split]):
    routed_dgrad_vec + mp_scatter_grad without the per-message rows (fp32 atomics; the outputs must be zeroed).
    src_rows [E, Din]: the source half is written there per message instead (sum it with mp_scatter_grad, accumulate=1)."""
    Dm = gq.shape[1]
    split = out_lo.shape[1]
    with _timed("msg_dgrad_nodes", 2.0 * gq.shape[0] * Dm * 2 * Din):
        _check(load_library().bl_routed_dgrad_nodes_rows(_f32(gq).data_ptr(), gq.stride(0), _i32(msg_src).data_ptr(), _i32(msg_tgt).data_ptr(),
                                                        win_bits.data_ptr(), win_bits.stride(0), _i32(type_ptr).data_ptr(), int(T),
                                                        _f32(wt).data_ptr(), int(E), Dm, int(Din), int(split), out_lo.data_ptr(), out_lo.stride(0),
                                                        _p(out_hi), out_hi.stride(0) if out_hi is not None else 0, _p(src_rows),
                                                        src_rows.stride(0) if src_rows is not None else 0, _stream()),
               "bl_routed_dgrad_nodes_rows")
    return out_lo, out_hi
