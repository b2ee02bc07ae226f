"""Message-passing layers of the graph models as autograd Functions (kernel by kernel and one C call per layer and direction),
the subtoken embedding, and the "backward launched" notifications of the data-parallel gradient buckets."""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional

import torch

from . import _switches, _streams
from ._cabi import (ACT_GELU_AGG, ACT_NONE, ACT_TANH, _ACTS, bl_mp_layer_t, _check, Dropout, _f32, _i32, load_library,
                    NO_DROPOUT, _p, _stream)
from ._streams import _direct_grad_target, _direct_small, _on_side_stream, _timed
from ._autograd import _take_saved
from .gemm import (act_bwd, gemm_rows, gemm_rows_routed, gemm_rows_x6, gemm_wgrad, gemm_wgrad_routed, gemm_wgrad_routed_x6,
                   layernorm_bwd, pack_bf16x3, pack_weights_x6, scatter_add_rows, segment_max, x6_ok)
from .weights import _as_groups, _packed_layer_weights, _packed_message_weights, _transposed_layer_weights

__all__ = ["GraphIndex", "MessageRuns", "LiveRows", "live_rows_of", "live_forward_ok", "LIVE_FWD_INNER", "LIVE_FWD_LAST", "POOLINGS", "AGGREGATIONS", "_EmbedSubtokenMax", "embed_subtoken_max", "_MpLayer", "node_update_bwd",
           "_use_vector_dgrad", "_layer_desc", "_MpLayerFused", "_pending_uses", "set_grad_ready_callback", "_note_use",
           "_notify_backward_launched", "fused_layer_ok", "_GatedMpLayer", "gated_mp_layer", "_MpLayerFeat",
           "mp_layer_with_edge_features", "mp_layer"]


class MessageRuns(NamedTuple):
    """Device-side run arrays of one minibatch (buglab.data.collate.message_run_arrays): the backward row space of E + R rows in
    which the target halves of the routed gradients are computed once per run (bl_mp_layer_t.num_runs)."""

    run_ptr: torch.Tensor
    bwd_group_ptr: torch.Tensor
    bwd_group_w: torch.Tensor
    bwd_rows_tgt: torch.Tensor
    bwd_rows_src: torch.Tensor
    tgt_run_ptr: torch.Tensor
    tgt_run_rows: torch.Tensor

    @classmethod
    def of(cls, *arrays) -> Optional["MessageRuns"]:
        """The tuple, or None when the minibatch carries none of the arrays (hand-built minibatches: per-message backward)."""
        return cls(*arrays) if all(a is not None for a in arrays) else None

    @property
    def num_runs(self) -> int:
        return int(self.run_ptr.shape[0]) - 1


class LiveRows(NamedTuple):
    """Device-side live arrays of ONE layer of one minibatch (buglab.data.collate.live_set_arrays): the rows of the layer's output
    whose gradient can be non-zero, and the reduced backward problem over them (bl_mp_layer_t.live_nodes ...).  Handing them to a
    layer is the caller's statement that the gradient of the layer's output IS zero everywhere else."""

    nodes: torch.Tensor
    recv: torch.Tensor
    msgs: torch.Tensor
    run_ptr: torch.Tensor
    group_ptr: torch.Tensor
    rows_tgt: torch.Tensor
    rows_src: torch.Tensor
    src_ptr: torch.Tensor
    src_msgs: torch.Tensor
    run_csr_ptr: torch.Tensor
    run_csr_rows: torch.Tensor


def live_rows_of(live_arrays: torch.Tensor, live_layout, T: int):
    """Per live layer (the last layer first) the LiveRows views into the minibatch's one `live_arrays` tensor."""
    out = []
    for row in (live_layout.tolist() if hasattr(live_layout, "tolist") else live_layout):
        nn, nr, ex, rx = row[:4]
        sizes = (nn, nr, ex, rx + 1, 2 * T + 1, ex + rx, ex + rx, nr + 1, ex, nr + 1, rx)
        out.append(LiveRows(*[live_arrays[o : o + n] for o, n in zip(row[4:], sizes)]))
    return out


class GraphIndex(NamedTuple):
    """Device-side index arrays of one minibatch (buglab.data.collate.to_device)."""

    msg_src: torch.Tensor
    msg_tgt: torch.Tensor
    type_ptr: torch.Tensor
    tgt_ptr: torch.Tensor
    tgt_msgs: torch.Tensor
    src_ptr: torch.Tensor
    src_msgs: torch.Tensor
    num_nodes: int
    num_messages: int
    num_types: int
    node_order: Optional[torch.Tensor] = None  # processing order of the per-node kernels: high-degree nodes first
    num_hubs: int = -1  # leading entries of node_order that are hubs (-1: unknown, the kernels look at the first 4096)
    runs: Optional[MessageRuns] = None  # None: backward works message by message
    live: Optional[LiveRows] = None  # the live rows of the layer this index is handed to (None: backward over all rows)
    # forward over the live rows too (bl_mp_layer_t.live_fwd): 0, LIVE_FWD_INNER or LIVE_FWD_LAST.  Set by GraphNeuralNetwork.forward for
    # the longest run of layers from the top for which live_forward_ok() said yes; a layer handed it runs live or raises.
    live_fwd: int = 0


LIVE_FWD_INNER, LIVE_FWD_LAST = 1, 2  # BL_LIVE_FWD_INNER / _LAST (LAST: the output is zero-filled first, it is handed out)
POOLINGS = ("max", "sum", "mean")  # BL_POOL_MAX / _SUM / _MEAN


AGGREGATIONS = ("max", "sum", "mean")  # BL_AGG_MAX / _SUM / _MEAN (ptgnn's message_aggregation_function values)


class _EmbedSubtokenMax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, table, ids, lens, drop: Dropout, tok_csr, before_pool: bool, comb: int):
        _f32(table, "embedding table")
        N, S = ids.shape
        V, H = table.shape
        out = torch.empty((N, H), dtype=torch.float32, device=table.device)
        argsub = torch.empty((N, H), dtype=torch.int8, device=table.device) if comb == 0 else None
        _check(
            load_library().bl_embed_subtoken_pool_fwd(table.data_ptr(), V, H, _i32(ids).data_ptr(), _i32(lens).data_ptr(), N, S, comb,
                                                      drop.c(), int(bool(before_pool)), out.data_ptr(), out.stride(0), _p(argsub), _stream()),
            "bl_embed_subtoken_pool_fwd")
        ctx.saved = (table, ids, lens, argsub, drop, V, H, tok_csr, int(bool(before_pool)), comb)
        return out

    @staticmethod
    def backward(ctx, g_out):
        table, ids, lens, argsub, drop, V, H, tok_csr, before_pool, comb = _take_saved(ctx)
        g_out = g_out.contiguous()
        N, S = ids.shape
        direct = _direct_small(table)
        g_table = direct if direct is not None else torch.zeros((V, H), dtype=torch.float32, device=g_out.device)
        if tok_csr is not None:
            occ, chunk_ptr, chunk_tok = tok_csr
            _check(
                load_library().bl_embed_subtoken_pool_bwd_sorted(g_out.data_ptr(), g_out.stride(0), _i32(occ).data_ptr(),
                                                                 _i32(chunk_ptr).data_ptr(), _i32(chunk_tok).data_ptr(),
                                                                 int(chunk_tok.shape[0]), _i32(lens).data_ptr(), _p(argsub), S, H, comb, drop.c(),
                                                                 before_pool, g_table.data_ptr(), _stream()),
                "bl_embed_subtoken_pool_bwd_sorted")
        else:
            _check(
                load_library().bl_embed_subtoken_pool_bwd(g_out.data_ptr(), g_out.stride(0), ids.data_ptr(), _i32(lens).data_ptr(), _p(argsub),
                                                          N, S, H, V, comb, drop.c(), before_pool, g_table.data_ptr(), _stream()),
                "bl_embed_subtoken_pool_bwd")
        return (None if direct is not None else g_table), None, None, None, None, None, None


def embed_subtoken_max(table, ids, lens, drop: Dropout = NO_DROPOUT, tok_csr=None, dropout_before_pooling: bool = False,
                       combination: str = "max"):
    """tok_csr = (occ, chunk_ptr, chunk_tok) from the collator (token-sorted subtoken occurrences): backward
    then sums per token in registers instead of issuing one atomic per (node, channel).
    dropout_before_pooling: dropout on the embedded subtokens (then max) instead of on the pooled rows.
    combination: "max" (the registry's default, modelregistry.py:65-66), "sum" or "mean" over the subtokens."""
    return _EmbedSubtokenMax.apply(table, ids, lens, drop, tok_csr, bool(dropout_before_pooling), POOLINGS.index(combination))


class _MpLayer(torch.autograd.Function):
    """One MlpMessagePassingLayer: message GEMM -> segmented max(+GELU) + LayerNorm -> dense+tanh+dropout.

    Saved for backward: only per-NODE arrays -- argmax [N, Dm] int32, the message activation's
    derivative at the winner `dact` [N, Dm], the aggregate, LayerNorm statistics/output and the layer
    output.  The [E, Dm] messages are dropped right after the segmented max: backward re-creates the
    (80 % zero) message gradient on the fly inside the two GEMMs' operand loads
    (bl_gemm_rows_routed / bl_gemm_wgrad_routed) from the node gradient and the winner table."""

    @staticmethod
    def forward(ctx, h, W, ln_g, ln_b, Wd, bd, g: GraphIndex, msg_act: int, drop: Dropout):
        _f32(h, "node states")
        N, Din = h.shape
        T, K2, Dm = W.shape
        Dout = Wd.shape[1]
        E = g.num_messages
        assert K2 == 2 * Din and T == g.num_types and N == g.num_nodes
        if x6_ok(Din, Dm):
            hp = pack_bf16x3(h)                   # [N, 3*Din]
            wtp = pack_weights_x6(_f32(W, "W"), True)
            pre = gemm_rows_x6([(hp, g.msg_src, Din), (hp, g.msg_tgt, Din)], wtp, E, Dm, group_ptr=g.type_ptr, G=T)
            del wtp
            if not _switches.WGRAD_X6:
                hp = None
        else:
            hp = None
            pre = gemm_rows([(h, g.msg_src), (h, g.msg_tgt)], _f32(W, "W"), E, Dm, b_group_stride=K2 * Dm, ldb=Dm,
                            group_ptr=g.type_ptr, G=T)
        use_bits = x6_ok(Din, Dm)
        res = segment_max(pre, g.tgt_ptr, g.tgt_msgs, N, act=msg_act, ln=(_f32(ln_g), _f32(ln_b)), want_dact=True, want_bits=use_bits,
                          seg_order=g.node_order)
        agg, arg, ln_out, mean, rstd, dact = res[:6]
        bits = res[6] if use_bits else None
        if _switches.WINNER_SINK is not None:
            _switches.WINNER_SINK.append(arg.clone())
        if use_bits and _switches.WGRAD_X6:
            arg = None  # the bf16x6 backward routes with the per-message bitmask only
        del pre, res
        if msg_act == ACT_NONE:
            dact = None  # derivative is identically 1
        out = gemm_rows([(ln_out, None)], _f32(Wd, "Wd"), N, Dout, bias=_f32(bd), act=ACT_TANH, drop=drop)
        # (the OUTPUT goes through save_for_backward: output -> grad_fn -> ctx -> output held as a plain attribute is a cycle
        # across the C++ boundary that nothing collects when no backward pass runs -- see _GatherLinear)
        ctx.save_for_backward(out)
        ctx.saved = (h, hp, W, ln_g, ln_b, Wd, bd, dact, arg, bits, agg, mean, rstd, ln_out, g, msg_act, drop)
        return out

    @staticmethod
    def backward(ctx, g_out):
        h, hp, W, ln_g, ln_b, Wd, bd, dact, arg, bits, agg, mean, rstd, ln_out, g, msg_act, drop = _take_saved(ctx)
        (out,) = ctx.saved_tensors
        N, Din = h.shape
        T, K2, Dm = W.shape
        Dout = Wd.shape[1]
        E = g.num_messages
        dev = h.device
        g_out = g_out.contiguous()
        # dense + tanh + dropout
        bd_direct, lng_direct, lnb_direct = _direct_small(bd), _direct_small(ln_g), _direct_small(ln_b)
        g_bd = bd_direct if bd_direct is not None else torch.zeros((Dout,), dtype=torch.float32, device=dev)
        g_z = act_bwd(g_out, out, ACT_TANH, drop, g_bd)
        Wd_direct, W_direct = _direct_grad_target(Wd), _direct_grad_target(W)
        g_Wd = Wd_direct if Wd_direct is not None else torch.zeros_like(Wd)
        g_W = W_direct if W_direct is not None else torch.zeros_like(W)
        side1 = _on_side_stream(dev)
        with side1:
            gemm_wgrad([(ln_out, None)], g_z, N, Dout, g_Wd)
        g_ln = gemm_rows([(g_z, None)], Wd, N, Dm, b_is_nk=True, ldb=Dout)
        # LayerNorm
        g_lng = lng_direct if lng_direct is not None else torch.zeros((Dm,), dtype=torch.float32, device=dev)
        g_lnb = lnb_direct if lnb_direct is not None else torch.zeros((Dm,), dtype=torch.float32, device=dev)
        # LayerNorm (+ the message activation's derivative at each winner): d loss / d (winning pre-activation) per node;
        # the bf16x6 GEMMs take it packed, straight from the LayerNorm kernel
        use_x6 = x6_ok(Din, Dm) and bits is not None
        if use_x6 and hp is not None:
            gq, gqp = None, layernorm_bwd(g_ln, agg, mean, rstd, ln_g, g_lng, g_lnb, post_scale=dact, want="packed")
        elif use_x6:
            gq, gqp = layernorm_bwd(g_ln, agg, mean, rstd, ln_g, g_lng, g_lnb, post_scale=dact, want="both")
        else:
            gq, gqp = layernorm_bwd(g_ln, agg, mean, rstd, ln_g, g_lng, g_lnb, post_scale=dact), None
        if bd_direct is not None:
            g_bd = None
        if lng_direct is not None:
            g_lng = None
        if lnb_direct is not None:
            g_lnb = None
        # per-edge-type weights; message m's gradient row = gq[tgt(m)] masked to the channels m won
        pair = _timed("mp_bwd_gemm_pair(wgrad||dgrad+node-sums)", 2.0 * (2.0 * E * K2 * Dm), span=True)
        pair.__enter__()
        side2 = _on_side_stream(dev)
        with side2:
            if hp is not None:
                gemm_wgrad_routed_x6([(hp, g.msg_src, Din), (hp, g.msg_tgt, Din)], gqp, g.msg_tgt, bits, E, Dm, g_W,
                                     gw_group_stride=K2 * Dm, group_ptr=g.type_ptr, G=T)
            else:
                gemm_wgrad_routed([(h, g.msg_src), (h, g.msg_tgt)], gq, g.msg_tgt, arg, E, Dm, g_W, gw_group_stride=K2 * Dm,
                                  group_ptr=g.type_ptr, G=T)
        # node states: per-message input gradients, then segmented sums over the src / tgt CSRs
        if gqp is not None:
            # d a = G . W_t^T: B_g = W_t itself read as [n = 2*Din, k = Dm]
            g_a = gemm_rows_x6([(gqp, g.msg_tgt, Dm)], pack_weights_x6(W, False), E, K2, group_ptr=g.type_ptr, G=T,
                               win_bits=bits, kind="gemm_rows_nk_routed_x6")
        else:
            g_a = gemm_rows_routed(gq, g.msg_tgt, arg, W, E, K2, b_group_stride=K2 * Dm, ldb=Dm, group_ptr=g.type_ptr, G=T)
        g_h = torch.empty((N, Din), dtype=torch.float32, device=dev)
        _check(
            load_library().bl_mp_scatter_grad(g_a.data_ptr(), g_a.stride(0), g.src_ptr.data_ptr(), g.src_msgs.data_ptr(),
                                              g.tgt_ptr.data_ptr(), g.tgt_msgs.data_ptr(), N, Din, 0, g_h.data_ptr(),
                                              g_h.stride(0), _p(g.node_order), _stream()),
            "bl_mp_scatter_grad")
        if W_direct is not None and Wd_direct is not None:
            # gradients land in param.grad behind the main chain; joined by join_side_stream()
            _streams.mark_free_running()
            side2.detach(h, gq, arg, bits, hp, gqp)
            side1.detach(ln_out, g_z)
            pair.__exit__(None, None, None)
            return g_h, None, g_lng, g_lnb, None, g_bd, None, None, None
        side2.join()
        side1.join()
        pair.__exit__(None, None, None)
        if W_direct is not None:
            g_W = None
        if Wd_direct is not None:
            g_Wd = None
        return g_h, g_W, g_lng, g_lnb, g_Wd, g_bd, None, None, None


def node_update_bwd(g_out, h_out, drop: "Dropout", wd_packed_bwd, agg, mean, rstd, ln_g, dact, g_bias, g_ln_g, g_ln_b, want_f32=True):
    """bl_node_update_bwd (csrc/bl_node_bwd.hip) -> (packed g_z [N, 3 Dout] int16, gq fp32 [N, Dm] or None, packed gq [N, 3 Dm])."""
    N, Dout = g_out.shape
    Dm = agg.shape[1]
    dev = g_out.device
    gz = torch.empty((N, 3 * Dout), dtype=torch.int16, device=dev)
    gq = torch.empty((N, Dm), dtype=torch.float32, device=dev) if want_f32 else None
    gqp = torch.empty((N, 3 * Dm), dtype=torch.int16, device=dev)
    _check(load_library().bl_node_update_bwd(_f32(g_out).data_ptr(), _f32(h_out).data_ptr(), N, Dout, drop.c(), wd_packed_bwd.data_ptr(),
                                             _f32(agg).data_ptr(), mean.data_ptr(), rstd.data_ptr(), ln_g.data_ptr(), _p(dact), Dm,
                                             gz.data_ptr(), _p(g_bias), _p(gq), gqp.data_ptr(), g_ln_g.data_ptr(), g_ln_b.data_ptr(),
                                             _stream()), "bl_node_update_bwd")
    return gz, gq, gqp


def _use_vector_dgrad(lib, E: int, Dm: int, K2: int) -> bool:
    want = _switches.DGRAD_VEC if _switches.DGRAD_VEC is not None else not lib.bl_get_msg_gemm_mode()
    return bool(want) and E > 0 and bool(lib.bl_routed_dgrad_vec_ok(Dm, K2))


def _layer_desc(g: "GraphIndex", W, ln_g, ln_b, Wd, bd, Din, msg_act, drop: Dropout, agg: int = 0, live_fwd: int = 0) -> bl_mp_layer_t:
    L = bl_mp_layer_t()
    L.aggregation = int(agg)
    L.N, L.E, L.T, L.Din, L.Dm, L.Dout = g.num_nodes, g.num_messages, W.shape[0], Din, W.shape[2], Wd.shape[1]
    L.msg_src, L.msg_tgt, L.type_ptr = g.msg_src.data_ptr(), g.msg_tgt.data_ptr(), g.type_ptr.data_ptr()
    L.tgt_ptr, L.tgt_msgs, L.src_ptr, L.src_msgs = g.tgt_ptr.data_ptr(), g.tgt_msgs.data_ptr(), g.src_ptr.data_ptr(), g.src_msgs.data_ptr()
    L.node_order = _p(g.node_order)
    L.num_hub_slots = int(g.num_hubs)
    L.W, L.ln_g, L.ln_b, L.Wd, L.bd = W.data_ptr(), ln_g.data_ptr(), ln_b.data_ptr(), Wd.data_ptr(), bd.data_ptr()
    L.msg_act, L.ln_eps, L.drop = int(msg_act), 1e-5, drop.c()
    if g.runs is not None and g.runs.num_runs > 0:  # (forward and backward must agree: the routing bitmask in `saved` has E + R rows)
        L.num_runs = g.runs.num_runs
        for name in MessageRuns._fields:
            setattr(L, name, getattr(g.runs, name).data_ptr())
    # (forward reads them only with live_fwd set; whether backward takes them is bl_mp_layer_bwd's decision -- bl_mp_layer_live_ok's)
    if g.live is not None and g.live.nodes.shape[0] > 0:
        lv = g.live
        L.live_num_nodes, L.live_num_recv = int(lv.nodes.shape[0]), int(lv.recv.shape[0])
        L.live_num_msgs, L.live_num_runs = int(lv.msgs.shape[0]), int(lv.run_ptr.shape[0]) - 1
        for name in LiveRows._fields:
            setattr(L, "live_" + name, getattr(lv, name).data_ptr())
    L.live_fwd = int(live_fwd)
    return L


def live_forward_ok(din: int, lo_width: Optional[int], W, ln_g, ln_b, Wd, bd, g: "GraphIndex", msg_act: str, drop: Dropout,
                    aggregation: str = "max") -> bool:
    """Whether mp_layer(...) on these arguments (g.live set; lo_width: the stash's width of a ConcatResidual pair, else None) may run
    its FORWARD over the live rows: the layer takes the one-call form, a backward pass will follow, no winner table is wanted, and
    the library's predicate (bl_mp_layer_live_ok, the same one bl_mp_layer_bwd evaluates) says yes.  No GPU work."""
    if g.live is None or g.live.nodes.shape[0] == 0 or not torch.is_grad_enabled():
        return False
    if not (fused_layer_ok(din, W.shape[2]) and (lo_width is None or lo_width % 32 == 0)):
        return False
    if not all(p.requires_grad for p in (W, ln_g, ln_b, Wd, bd)):  # (_direct_grad_target and the packed W^T image presuppose it)
        return False
    lib = load_library()
    agg = AGGREGATIONS.index(aggregation)
    Dm, Dout = W.shape[2], Wd.shape[1]
    if not (_switches.DENSE_X6 and Dm % 32 == 0 and Dout % 32 == 0):
        return False
    use_vec = agg == 0 and _use_vector_dgrad(lib, g.num_messages, Dm, 2 * din)
    L = _layer_desc(g, W, ln_g, ln_b, Wd, bd, din, _ACTS[msg_act], drop, agg)
    L.Wd_packed = _packed_layer_weights(Wd, True)[0].data_ptr()  # (cached: the same image forward is about to use)
    return bool(lib.bl_mp_layer_live_ok(ctypes.byref(L), 0 if use_vec else 1, 1, 1 if _switches.WINNER_SINK is not None else 0))


class _MpLayerFused(torch.autograd.Function):
    """One MlpMessagePassingLayer = one C call forward, one backward.  The layer input is `h_lo` alone or the
    virtual concatenation [h_lo ; h_hi] of a ConcatResidual layer (never materialised).  What forward keeps for
    backward is one opaque byte blob (packed input, routing bitmask, LayerNorm state; layout in csrc/bl_mp_layer.hip)."""

    @staticmethod
    def forward(ctx, h_lo, h_hi, W, ln_g, ln_b, Wd, bd, g: GraphIndex, msg_act: int, drop: Dropout, agg: int = 0):
        _f32(h_lo, "node states")
        lib = load_library()
        N = h_lo.shape[0]
        Din = h_lo.shape[1] + (h_hi.shape[1] if h_hi is not None else 0)
        T, K2, Dm = W.shape
        Dout = Wd.shape[1]
        E = g.num_messages
        assert K2 == 2 * Din and T == g.num_types and N == g.num_nodes
        for t, nm in ((W, "W"), (ln_g, "ln_g"), (ln_b, "ln_b"), (Wd, "Wd"), (bd, "bd")):
            _f32(t, nm)
        # (grad mode is always off inside Function.forward: whether a backward pass will follow is in needs_input_grad)
        need_bwd = any(ctx.needs_input_grad[:7])
        # which form of W the input gradient will read: its fp32 transpose (vector-unit path) or the packed C = G . W^T form
        use_vec = agg == 0 and _use_vector_dgrad(lib, E, Dm, K2)  # (sum / mean: no routing bits -> matrix-core input gradient)
        wkn, wnk = _packed_message_weights(W, Din, need_bwd and not use_vec)
        wt = _transposed_layer_weights(W) if (need_bwd and use_vec) else None
        dev = h_lo.device
        # (g.live_fwd: decided for the whole run of layers before the first of them ran; the call runs live or fails -- a silent full
        # forward here would read rows the layer below never computed)
        L = _layer_desc(g, W, ln_g, ln_b, Wd, bd, Din, msg_act, drop, agg, live_fwd=g.live_fwd)
        dense_x6 = _switches.DENSE_X6 and Dm % 32 == 0 and Dout % 32 == 0
        wd_kn = wd_nk = None
        if dense_x6:
            wd_kn, wd_nk = _packed_layer_weights(Wd, need_bwd)
            L.Wd_packed = wd_kn.data_ptr()
        # no backward pass will follow (predict / evaluate under no_grad): nothing is saved, the call skips every store that
        # only a backward pass reads (routing bitmask, activation derivative, aggregate, LayerNorm statistics)
        infer = not need_bwd and _switches.INFERENCE_MODE
        # ("mean" without an activation keeps the derivative array all the same: it carries the 1 / in-degree)
        saved_act = ACT_GELU_AGG if (agg == 2 and msg_act == ACT_NONE) else msg_act
        saved = None if infer else torch.empty((lib.bl_mp_layer_saved_bytes(N, E + L.num_runs, Din, Dm, saved_act),), dtype=torch.uint8, device=dev)
        ws = torch.empty((lib.bl_mp_layer_workspace_bytes(N, E, Din, Dm, Dout, 3 if infer else 0),), dtype=torch.uint8, device=dev)
        out = torch.empty((N, Dout), dtype=torch.float32, device=dev)
        winner = torch.empty((N, Dm), dtype=torch.int32, device=dev) if (_switches.WINNER_SINK is not None and agg == 0) else None
        _check(lib.bl_mp_layer_fwd(ctypes.byref(L), h_lo.data_ptr(), h_lo.stride(0), h_lo.shape[1], _p(h_hi),
                                   h_hi.stride(0) if h_hi is not None else 0, wkn.data_ptr(), out.data_ptr(), _p(winner),
                                   _p(saved), ws.data_ptr() if (E > 0 or infer) else None, _stream()), "bl_mp_layer_fwd")
        if winner is not None:
            _switches.WINNER_SINK.append(winner)
        if need_bwd:
            _note_use((W, ln_g, ln_b, Wd, bd))
        ctx.save_for_backward(out)  # (an output: never as a plain ctx attribute, see _MpLayer)
        ctx.saved = (h_lo.shape[1], h_hi.shape[1] if h_hi is not None else 0, W, ln_g, ln_b, Wd, bd, g, msg_act, drop, saved, wnk,
                     dense_x6, wd_kn, wd_nk, wt, agg)
        return out

    @staticmethod
    def backward(ctx, g_out):
        w_lo, w_hi, W, ln_g, ln_b, Wd, bd, g, msg_act, drop, saved, wnk, dense_x6, wd_kn, wd_nk, wt, agg = _take_saved(ctx)
        (out,) = ctx.saved_tensors
        lib = load_library()
        N, E = g.num_nodes, g.num_messages
        T, K2, Dm = W.shape
        Din, Dout = w_lo + w_hi, Wd.shape[1]
        dev = out.device
        g_out = g_out.contiguous()
        use_vec = agg == 0 and _use_vector_dgrad(lib, E, Dm, 2 * Din)
        if use_vec and wt is None:
            wt = _transposed_layer_weights(W)
        if wnk is None and not use_vec:  # forward ran without grad mode knowing a backward would follow
            wnk = _packed_message_weights(W, Din, True)[1]
        direct = [_direct_small(bd), _direct_small(ln_g), _direct_small(ln_b), _direct_grad_target(Wd), _direct_grad_target(W)]
        tgt = [d if d is not None else torch.zeros_like(p) for d, p in zip(direct, (bd, ln_g, ln_b, Wd, W))]
        g_bd, g_lng, g_lnb, g_Wd, g_W = tgt
        L = _layer_desc(g, W, ln_g, ln_b, Wd, bd, Din, msg_act, drop, agg, live_fwd=g.live_fwd)  # (forward's decision binds backward)
        if dense_x6:  # (forward kept the LayerNorm output in packed form: backward must take the same path)
            if wd_nk is None:
                wd_nk = pack_weights_x6(_as_groups(Wd.detach()), False)
            L.Wd_packed, L.Wd_packed_bwd = wd_kn.data_ptr(), wd_nk.data_ptr()
        ws_mode = 1
        if use_vec:
            L.Wt = wt.data_ptr()
            if not lib.bl_get_deterministic():
                ws_mode = 2  # node sums fused into the input-gradient kernel: no [E, 2 Din] scratch
        ws = torch.empty((lib.bl_mp_layer_workspace_bytes(N, E, Din, Dm, Dout, ws_mode),), dtype=torch.uint8, device=dev)
        g_lo = torch.empty((N, w_lo), dtype=torch.float32, device=dev)
        g_hi = torch.empty((N, w_hi), dtype=torch.float32, device=dev) if w_hi else None
        side = _streams.side_stream_for_current_device()
        free_running = side is not None and direct[3] is not None and direct[4] is not None
        _check(lib.bl_mp_layer_bwd(ctypes.byref(L), out.data_ptr(), g_out.data_ptr(), _p(wnk), saved.data_ptr(), ws.data_ptr(),
                                   g_lo.data_ptr(), g_lo.stride(0), w_lo, _p(g_hi), g_hi.stride(0) if g_hi is not None else 0,
                                   g_W.data_ptr(), g_lng.data_ptr(), g_lnb.data_ptr(), g_Wd.data_ptr(), g_bd.data_ptr(), _stream(),
                                   side.cuda_stream if side is not None else None, 0 if free_running else 1), "bl_mp_layer_bwd")
        if free_running:
            # the two weight-gradient GEMMs keep running behind the main chain (joined by join_side_stream()):
            # what they read must not be recycled by the allocator before they are done -- held until the join
            _streams.mark_free_running(saved, ws)
        ret = [None if d is not None else t for d, t in zip(direct, tgt)]
        if all(d is not None for d in direct):  # (gradients returned through autograd are not in place yet)
            _notify_backward_launched((W, ln_g, ln_b, Wd, bd))
        return g_lo, g_hi, ret[4], ret[1], ret[2], ret[3], ret[0], None, None, None, None


# ---- "the backward of this layer has been launched" notifications (data-parallel gradient buckets, runtime/optim.py) ----
_pending_uses = {}  # id(param) -> forward uses whose backward has not been launched yet (weight sharing)


def set_grad_ready_callback(fn) -> None:
    """fn(list of parameters) is called from a message-passing layer's backward once every kernel that adds into those
    parameters' gradients has been LAUNCHED (on the training stream or the side stream); None switches it off."""
    _switches.GRAD_READY_CALLBACK = fn
    _pending_uses.clear()


def _note_use(params) -> None:
    if _switches.GRAD_READY_CALLBACK is not None:
        for p in params:
            _pending_uses[id(p)] = _pending_uses.get(id(p), 0) + 1


def _notify_backward_launched(params) -> None:
    if _switches.GRAD_READY_CALLBACK is None:
        return
    done = []
    for p in params:
        n = _pending_uses.get(id(p), 1) - 1
        if n <= 0:
            _pending_uses.pop(id(p), None)
            done.append(p)
        else:
            _pending_uses[id(p)] = n
    if done:
        _switches.GRAD_READY_CALLBACK(done)


def fused_layer_ok(Din: int, Dm: int) -> bool:
    return _switches.FUSED_LAYER and _switches.WGRAD_X6 and x6_ok(Din, Dm) and Dm <= 512


class _GatedMpLayer(torch.autograd.Function):
    """One GatedMessagePassingLayer (GGNN): m_e = h[src] @ W[type] -> segmented max -> GRU cell(+dropout).
    Backward keeps per-node arrays only (winner table + GRU gate pre-activations)."""

    @staticmethod
    def forward(ctx, h, W, Wi, bi, Wh, bh, g: GraphIndex, drop: Dropout):
        _f32(h, "node states")
        N, D = h.shape
        T, Din, Dm = W.shape
        E = g.num_messages
        assert Din == D and Wi.shape == (Dm, 3 * D) and Wh.shape == (D, 3 * D)
        msgs = gemm_rows([(h, g.msg_src)], _f32(W, "W"), E, Dm, b_group_stride=D * Dm, ldb=Dm, group_ptr=g.type_ptr, G=T)
        agg, arg, _, _, _ = segment_max(msgs, g.tgt_ptr, g.tgt_msgs, N, seg_order=g.node_order)
        del msgs
        gi = gemm_rows([(agg, None)], _f32(Wi), N, 3 * D, bias=_f32(bi))
        gh = gemm_rows([(h, None)], _f32(Wh), N, 3 * D, bias=_f32(bh))
        out = torch.empty((N, D), dtype=torch.float32, device=h.device)
        _check(load_library().bl_gru_cell_fwd(gi.data_ptr(), gh.data_ptr(), h.data_ptr(), h.stride(0), N, D, drop.c(), out.data_ptr(), _stream()),
               "bl_gru_cell_fwd")
        ctx.saved = (h, W, Wi, Wh, agg, arg, gi, gh, g, drop)
        return out

    @staticmethod
    def backward(ctx, g_out):
        h, W, Wi, Wh, agg, arg, gi, gh, g, drop = _take_saved(ctx)
        N, D = h.shape
        T, _, Dm = W.shape
        E = g.num_messages
        dev = h.device
        g_out = g_out.contiguous()
        g_gi = torch.empty_like(gi)
        g_gh = torch.empty_like(gh)
        g_h = torch.empty_like(h)
        _check(load_library().bl_gru_cell_bwd(g_out.data_ptr(), gi.data_ptr(), gh.data_ptr(), h.data_ptr(), h.stride(0), N, D, drop.c(),
                                              g_gi.data_ptr(), g_gh.data_ptr(), g_h.data_ptr(), _stream()), "bl_gru_cell_bwd")
        g_bi, g_bh = g_gi.sum(0), g_gh.sum(0)
        g_Wi, g_Wh, g_W = torch.zeros_like(Wi), torch.zeros_like(Wh), torch.zeros_like(W)
        side = _on_side_stream(dev)
        with side:
            gemm_wgrad([(agg, None)], g_gi, N, 3 * D, g_Wi)
            gemm_wgrad([(h, None)], g_gh, N, 3 * D, g_Wh)
        g_h += gemm_rows([(g_gh, None)], Wh, N, D, b_is_nk=True, ldb=3 * D)
        gq = gemm_rows([(g_gi, None)], Wi, N, Dm, b_is_nk=True, ldb=3 * D)  # d loss / d aggregate
        with side:
            gemm_wgrad_routed([(h, g.msg_src)], gq, g.msg_tgt, arg, E, Dm, g_W, gw_group_stride=D * Dm, group_ptr=g.type_ptr, G=T)
        g_a = gemm_rows_routed(gq, g.msg_tgt, arg, W, E, D, b_group_stride=D * Dm, ldb=Dm, group_ptr=g.type_ptr, G=T)
        _check(
            load_library().bl_mp_scatter_grad(g_a.data_ptr(), g_a.stride(0), g.src_ptr.data_ptr(), g.src_msgs.data_ptr(), None, None,
                                              N, D, 1, g_h.data_ptr(), g_h.stride(0), _p(g.node_order), _stream()),
            "bl_mp_scatter_grad")
        side.join()
        side.join()
        return g_h, g_W, g_Wi, g_bi, g_Wh, g_bh, None, None


def gated_mp_layer(h, W, Wi, bi, Wh, bh, graph: GraphIndex, drop: Dropout = NO_DROPOUT):
    return _GatedMpLayer.apply(h.contiguous(), W, Wi, bi, Wh, bh, graph, drop)


class _MpLayerFeat(torch.autograd.Function):
    """MlpMessagePassingLayer with edge features (`features_dimension` F > 0, reference gnnlayerdefs.py:13,22): the message
    input is [h_src ; h_tgt ; f_e] with f_e = edge_table[msg_feat[e]] read as a THIRD gathered source of the message GEMM --
    the [E, F] feature matrix is never materialised.  The three message GEMMs (forward, routed weight gradient, routed
    input gradient) run on the bf16x6 kernels with three packed sources when Din, Dm and F are multiples of 32 (the table
    is packed once per call like the node states); otherwise on the exact-fp32 kernels.  Kernel by kernel (non-default
    configuration), dense node update on the exact-fp32 GEMMs."""

    @staticmethod
    def forward(ctx, h, W, ln_g, ln_b, Wd, bd, table, msg_feat, g: GraphIndex, msg_act: int, drop: Dropout):
        _f32(h, "node states")
        N, Din = h.shape
        T, K3, Dm = W.shape
        F = table.shape[1]
        Dout = Wd.shape[1]
        E = g.num_messages
        assert K3 == 2 * Din + F and T == g.num_types and N == g.num_nodes and msg_feat.shape[0] == E
        use_x6 = x6_ok(Din, Dm, F) and _switches.WGRAD_X6
        hp = tp = bits = None
        if use_x6:
            hp, tp = pack_bf16x3(h), pack_bf16x3(_f32(table, "edge table"))
            pre = gemm_rows_x6([(hp, g.msg_src, Din), (hp, g.msg_tgt, Din), (tp, msg_feat, F)], _packed_layer_weights(W, False)[0], E, Dm,
                               group_ptr=g.type_ptr, G=T)
        else:
            src3 = [(h, g.msg_src), (h, g.msg_tgt), (_f32(table, "edge table"), msg_feat)]
            pre = gemm_rows(src3, _f32(W, "W"), E, Dm, b_group_stride=K3 * Dm, ldb=Dm, group_ptr=g.type_ptr, G=T)
        res = segment_max(pre, g.tgt_ptr, g.tgt_msgs, N, act=msg_act, ln=(_f32(ln_g), _f32(ln_b)), want_dact=True, want_bits=use_x6,
                          seg_order=g.node_order)
        agg, arg, ln_out, mean, rstd, dact = res[:6]
        if use_x6:
            bits = res[6]
        if _switches.WINNER_SINK is not None:
            _switches.WINNER_SINK.append(arg.clone())
        if use_x6:
            arg = None  # the bf16x6 backward routes with the per-message bitmask only
        del pre, res
        if msg_act == ACT_NONE:
            dact = None
        out = gemm_rows([(ln_out, None)], _f32(Wd, "Wd"), N, Dout, bias=_f32(bd), act=ACT_TANH, drop=drop)
        ctx.save_for_backward(out)  # (an output: never as a plain ctx attribute, see _MpLayer)
        ctx.saved = (h, hp, tp, bits, W, ln_g, Wd, table, msg_feat, dact, arg, agg, mean, rstd, ln_out, g, drop)
        return out

    @staticmethod
    def backward(ctx, g_out):
        h, hp, tp, bits, W, ln_g, Wd, table, msg_feat, dact, arg, agg, mean, rstd, ln_out, g, drop = _take_saved(ctx)
        (out,) = ctx.saved_tensors
        N, Din = h.shape
        T, K3, Dm = W.shape
        F, Dout, E, dev = table.shape[1], Wd.shape[1], g.num_messages, h.device
        z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
        g_bd, g_Wd, g_W, g_lng, g_lnb, g_table = z(Dout), torch.zeros_like(Wd), torch.zeros_like(W), z(Dm), z(Dm), torch.zeros_like(table)
        g_z = act_bwd(g_out.contiguous(), out, ACT_TANH, drop, g_bd)
        gemm_wgrad([(ln_out, None)], g_z, N, Dout, g_Wd)
        g_ln = gemm_rows([(g_z, None)], Wd, N, Dm, b_is_nk=True, ldb=Dout)
        if hp is not None:
            # d loss / d (winning pre-activation) per node, packed for the bf16x6 GEMMs; message e's gradient row is
            # gq[tgt(e)] masked to the channels e won (the routing bitmask)
            gqp = layernorm_bwd(g_ln, agg, mean, rstd, ln_g, g_lng, g_lnb, post_scale=dact, want="packed")
            gemm_wgrad_routed_x6([(hp, g.msg_src, Din), (hp, g.msg_tgt, Din), (tp, msg_feat, F)], gqp, g.msg_tgt, bits, E, Dm, g_W,
                                 gw_group_stride=K3 * Dm, group_ptr=g.type_ptr, G=T)
            g_a = gemm_rows_x6([(gqp, g.msg_tgt, Dm)], _packed_layer_weights(W, True)[1], E, K3, group_ptr=g.type_ptr, G=T, win_bits=bits,
                               kind="gemm_rows_nk_routed_x6")  # [E, 2 Din + F]
        else:
            gq = layernorm_bwd(g_ln, agg, mean, rstd, ln_g, g_lng, g_lnb, post_scale=dact)
            src3 = [(h, g.msg_src), (h, g.msg_tgt), (table, msg_feat)]
            gemm_wgrad_routed(src3, gq, g.msg_tgt, arg, E, Dm, g_W, gw_group_stride=K3 * Dm, group_ptr=g.type_ptr, G=T)
            g_a = gemm_rows_routed(gq, g.msg_tgt, arg, W, E, K3, b_group_stride=K3 * Dm, ldb=Dm, group_ptr=g.type_ptr, G=T)  # [E, 2 Din + F]
        g_h = torch.empty((N, Din), dtype=torch.float32, device=dev)
        _check(load_library().bl_mp_scatter_grad(g_a.data_ptr(), g_a.stride(0), g.src_ptr.data_ptr(), g.src_msgs.data_ptr(), g.tgt_ptr.data_ptr(),
                                                 g.tgt_msgs.data_ptr(), N, Din, 0, g_h.data_ptr(), g_h.stride(0), _p(g.node_order), _stream()),
               "bl_mp_scatter_grad")
        if E > 0:
            scatter_add_rows(g_a, 2 * Din, F, msg_feat, g_table)  # the feature columns go back to the table rows they came from
        return g_h, g_W, g_lng, g_lnb, g_Wd, g_bd, g_table, None, None, None, None


def mp_layer_with_edge_features(h, W, ln_g, ln_b, Wd, bd, table, msg_feat, graph: GraphIndex, msg_act: str = "gelu_aggregated",
                                drop: Dropout = NO_DROPOUT):
    """mp_layer with [h_src ; h_tgt ; table[msg_feat]] as the message input (W: [T, 2 Din + F, Dm])."""
    if isinstance(h, (tuple, list)):
        h = torch.cat(list(h), dim=-1)
    return _MpLayerFeat.apply(h.contiguous(), W, ln_g, ln_b, Wd, bd, table, msg_feat, graph, _ACTS[msg_act], drop)


def mp_layer(h, W, ln_g, ln_b, Wd, bd, graph: GraphIndex, msg_act: str = "gelu_aggregated", drop: Dropout = NO_DROPOUT,
             aggregation: str = "max"):
    """h: the node states [N, Din], or a pair (stash, current) standing for their concatenation (ConcatResidual).
    aggregation: "max" (the reference's recipe, gnnlayerdefs.py:11,21) or ptgnn's "sum" / "mean" (one-call layer form only)."""
    pair = isinstance(h, (tuple, list))
    Din = sum(t.shape[1] for t in h) if pair else h.shape[1]
    agg = AGGREGATIONS.index(aggregation)
    if fused_layer_ok(Din, W.shape[2]) and (not pair or h[0].shape[1] % 32 == 0):
        lo, hi = (h[0].contiguous(), h[1].contiguous()) if pair else (h.contiguous(), None)
        return _MpLayerFused.apply(lo, hi, W, ln_g, ln_b, Wd, bd, graph, _ACTS[msg_act], drop, agg)
    if graph.live_fwd:
        raise RuntimeError("mp_layer: the graph index asks for the live forward, which only the one-call layer form has")
    if agg != 0:
        raise NotImplementedError("sum / mean message aggregation runs in the one-call layer form only (state and message widths multiples of "
                                  "32, message width <= 512, FUSED_LAYER on)")
    if pair:
        h = torch.cat(list(h), dim=-1)
    return _MpLayer.apply(h.contiguous(), W, ln_g, ln_b, Wd, bd, graph, _ACTS[msg_act], drop)
