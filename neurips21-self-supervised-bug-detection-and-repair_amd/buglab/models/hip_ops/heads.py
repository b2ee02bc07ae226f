"""Scoring heads and losses: segmented softmax / max pooling, the fused scorers, the bug-loss assembly, GREAT's var-misuse head."""
from __future__ import annotations

import ctypes
from ctypes import c_int32, c_void_p
from typing import NamedTuple, Sequence

import torch

from ._cabi import (bl_bug_loss_t, bl_varmisuse_head_t, _check, _f32, _i32, load_library, _p, _req, _rows, RowSource, _stream,
                    VARMISUSE_STATS)
from ._autograd import _grad_target, _take_saved
from .gemm import segment_max, segment_max_bwd

__all__ = ["_SegmentLogSoftmax", "segment_log_softmax", "_SegmentMaxPool", "segment_max_pool", "_MlpScore", "mlp_score",
           "_LocalizationScores", "localization_scores", "BUG_LOSS_STATS", "BugLossIndex", "_bug_loss_desc", "_BugLoss",
           "bug_loss", "_byte_mask", "_varmisuse_desc", "_varmisuse_workspace", "_VarMisuseHead", "varmisuse_head",
           "VARMISUSE_RECORD_D", "VARMISUSE_RECORD_I", "varmisuse_predict", "DISTILL_OUT", "DISTILL_STATS", "distill_fwd", "distill_bwd",
           "_DistillLoss", "distill_loss"]


class _SegmentLogSoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, seg_ptr, seg_items, nseg, eps):
        y = torch.empty_like(x)
        _check(
            load_library().bl_segment_log_softmax_fwd(_f32(x).data_ptr(), _i32(seg_ptr).data_ptr(), _p(seg_items), int(nseg),
                                                      float(eps), y.data_ptr(), _stream()),
            "bl_segment_log_softmax_fwd")
        ctx.save_for_backward(y)  # (an output: see _GatherLinear)
        ctx.saved = (seg_ptr, seg_items, nseg)
        return y

    @staticmethod
    def backward(ctx, g_y):
        seg_ptr, seg_items, nseg = _take_saved(ctx)
        (y,) = ctx.saved_tensors
        g_x = torch.zeros_like(y)
        _check(
            load_library().bl_segment_log_softmax_bwd(_f32(g_y.contiguous()).data_ptr(), y.data_ptr(), seg_ptr.data_ptr(),
                                                      _p(seg_items), int(nseg), g_x.data_ptr(), _stream()),
            "bl_segment_log_softmax_bwd")
        return g_x, None, None, None, None


def segment_log_softmax(x, seg_ptr, seg_items, nseg: int, eps: float = 1e-12):
    """scatter_log_softmax (reference buglab/models/utils.py:15-28) over a CSR of the segment ids."""
    if x.numel() == 0:
        return x
    return _SegmentLogSoftmax.apply(x.contiguous(), seg_ptr, seg_items, nseg, eps)


class _SegmentMaxPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, seg_ptr, seg_of, nseg):
        out, arg, _, _, _ = segment_max(x, seg_ptr, None, nseg)
        ctx.saved = (arg, x.shape, seg_of)
        ctx.mark_non_differentiable(arg)
        return out, arg

    @staticmethod
    def backward(ctx, g_out, _g_arg):
        arg, shape, seg_of = _take_saved(ctx)
        x_like = torch.empty(shape, dtype=torch.float32, device=g_out.device)
        g_x = segment_max_bwd(g_out.contiguous(), arg, x_like, seg_of, out=x_like)
        return g_x, None, None, None


def segment_max_pool(x, seg_ptr, seg_of, nseg: int):
    """scatter_max over CONTIGUOUS segments (rows of segment s are seg_ptr[s]..seg_ptr[s+1]).
    Returns (values [nseg, D], argmax row int32 [nseg, D]; -1 for an empty segment)."""
    return _SegmentMaxPool.apply(x.contiguous(), seg_ptr, seg_of, nseg)


# ------------------------------------------------------------------------------------------------
# whole scoring heads per C call (csrc/bl_heads_fused.hip)
class _MlpScore(torch.autograd.Function):
    """score[r] = w2 . relu(concat_j(x_j[idx_j[r]]) @ W1 + b1) + b2: forward and backward are one C call each."""

    @staticmethod
    def forward(ctx, W1, b1, w2, b2, nsrc, *flat):
        xs, idxs = flat[:nsrc], flat[nsrc:]
        rows, K = _rows(list(zip(xs, idxs)))
        R = idxs[0].shape[0] if idxs[0] is not None else xs[0].shape[0]
        H = W1.shape[1]
        dev = W1.device
        hidden = torch.empty((R, H), dtype=torch.float32, device=dev)
        score = torch.empty((R,), dtype=torch.float32, device=dev)
        _check(load_library().bl_gather_concat_mlp_score_fwd(ctypes.byref(rows), _f32(W1, "W1").data_ptr(), _f32(b1).data_ptr(),
                                                             _f32(w2).data_ptr(), _p(b2), R, H, hidden.data_ptr(), score.data_ptr(),
                                                             _stream()), "bl_gather_concat_mlp_score_fwd")
        ctx.saved = (W1, b1, w2, b2, xs, idxs, hidden, K)
        return score

    @staticmethod
    def backward(ctx, g_score):
        W1, b1, w2, b2, xs, idxs, hidden, K = _take_saved(ctx)
        lib = load_library()
        R, H = hidden.shape
        dev = W1.device
        rows, _ = _rows(list(zip(xs, idxs)))
        (gW1, rW1), (gb1, rb1), (gw2, rw2) = _grad_target(W1), _grad_target(b1), _grad_target(w2)
        gb2, rb2 = _grad_target(b2) if b2 is not None else (None, None)
        # one gradient matrix per DISTINCT source tensor (the scorers read the same node-state matrix two or three times)
        bufs, ret = {}, []
        gx = (c_void_p * 3)()
        ld = (c_int32 * 3)()
        for j, x in enumerate(xs):
            if not ctx.needs_input_grad[5 + j]:
                ret.append(None)
                continue
            key = x.data_ptr()
            if key not in bufs:
                bufs[key] = torch.zeros_like(x)
                ret.append(bufs[key])
            else:
                ret.append(None)
            gx[j], ld[j] = bufs[key].data_ptr(), bufs[key].stride(0)
        ws = torch.empty((lib.bl_gather_concat_mlp_score_workspace_bytes(R, H, K),), dtype=torch.uint8, device=dev)
        _check(lib.bl_gather_concat_mlp_score_bwd(ctypes.byref(rows), W1.data_ptr(), w2.data_ptr(), hidden.data_ptr(),
                                                  _f32(g_score.contiguous()).data_ptr(), R, H, ws.data_ptr(), gW1.data_ptr(), gb1.data_ptr(),
                                                  gw2.data_ptr(), _p(gb2), gx, ld, _stream()), "bl_gather_concat_mlp_score_bwd")
        return (rW1, rb1, rw2, rb2, None) + tuple(ret) + (None,) * len(xs)


def mlp_score(sources: Sequence[RowSource], W1, b1, w2, b2):
    xs = [x for x, _ in sources]
    idxs = [i for _, i in sources]
    return _MlpScore.apply(W1, b1, w2, b2, len(sources), *xs, *idxs)


class _LocalizationScores(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, cand, cand_graph, cand_ptr, B, Ws, bs, W1, b1, w):
        lib = load_library()
        _f32(x, "node states")
        C, H = cand.shape[0], x.shape[1]
        dev = x.device
        saved = torch.empty((lib.bl_localization_scores_saved_bytes(C, B, H),), dtype=torch.uint8, device=dev)
        ws = torch.empty((lib.bl_localization_scores_workspace_bytes(C, B, H, 0),), dtype=torch.uint8, device=dev)
        score = torch.empty((C,), dtype=torch.float32, device=dev)
        _check(lib.bl_localization_scores_fwd(x.data_ptr(), x.stride(0), _i32(cand).data_ptr(), _i32(cand_graph).data_ptr(),
                                              _i32(cand_ptr).data_ptr(), C, B, H, _f32(Ws).data_ptr(), _f32(bs).data_ptr(),
                                              _f32(W1).data_ptr(), _f32(b1).data_ptr(), _f32(w).data_ptr(), saved.data_ptr(),
                                              ws.data_ptr(), score.data_ptr(), _stream()), "bl_localization_scores_fwd")
        ctx.saved = (x, cand, cand_graph, cand_ptr, B, Ws, bs, W1, b1, w, saved)
        return score

    @staticmethod
    def backward(ctx, g_score):
        x, cand, cand_graph, cand_ptr, B, Ws, bs, W1, b1, w, saved = _take_saved(ctx)
        lib = load_library()
        C, H = cand.shape[0], x.shape[1]
        dev = x.device
        g_x = torch.zeros_like(x)
        (gWs, rWs), (gbs, rbs), (gW1, rW1), (gb1, rb1), (gw, rw) = (_grad_target(t) for t in (Ws, bs, W1, b1, w))
        ws = torch.empty((lib.bl_localization_scores_workspace_bytes(C, B, H, 1),), dtype=torch.uint8, device=dev)
        _check(lib.bl_localization_scores_bwd(x.data_ptr(), x.stride(0), cand.data_ptr(), cand_graph.data_ptr(), cand_ptr.data_ptr(), C, B, H,
                                              Ws.data_ptr(), W1.data_ptr(), w.data_ptr(), saved.data_ptr(), ws.data_ptr(),
                                              _f32(g_score.contiguous()).data_ptr(), g_x.data_ptr(), g_x.stride(0), gWs.data_ptr(),
                                              gbs.data_ptr(), gW1.data_ptr(), gb1.data_ptr(), gw.data_ptr(), _stream()),
               "bl_localization_scores_bwd")
        return g_x, None, None, None, None, rWs, rbs, rW1, rb1, rw


def localization_scores(x, cand, cand_graph, cand_ptr, num_graphs: int, Ws, bs, W1, b1, w):
    """Candidate scores of the localization head before the NO_BUG logit (reference localizationmodule.py:54-60)."""
    if cand.shape[0] == 0:
        return torch.zeros((0,), dtype=torch.float32, device=x.device)
    return _LocalizationScores.apply(x.contiguous(), cand, cand_graph, cand_ptr, int(num_graphs), Ws, bs, W1, b1, w)


# ------------------------------------------------------------------------------------------------
# loss assembly (csrc/bl_loss.hip): everything between the scorers' logits and the scalar loss in one kernel per direction
BUG_LOSS_STATS = 16


class BugLossIndex(NamedTuple):
    """Index tensors of one minibatch the loss assembly reads (all int32 on the device, has_bug bool)."""

    loc_group_ptr: torch.Tensor
    loc_group_items: torch.Tensor
    candidate_ptr: torch.Tensor
    has_bug: torch.Tensor
    correct_candidate_idxs: torch.Tensor
    repair_group_ptr: torch.Tensor
    repair_group_items: torch.Tensor
    logit_groups: tuple   # (text, var, swap): location group of every logit
    targets: tuple        # (text, var, swap): indices of the correct rewrites inside their slice
    num_groups: int


def _bug_loss_desc(loc_scores, logits, sizes, ix: BugLossIndex, w_buggy: float, abstain: float) -> bl_bug_loss_t:
    d = bl_bug_loss_t()
    d.B, d.C = int(ix.has_bug.shape[0]), int(loc_scores.shape[0])
    d.Rt, d.Rv, d.Rs = (int(n) for n in sizes)
    d.G = int(ix.num_groups)
    d.loc_scores, d.repair_logits = _p(loc_scores), _p(logits)
    d.loc_group_ptr, d.loc_group_items = _i32(ix.loc_group_ptr).data_ptr(), _i32(ix.loc_group_items).data_ptr()
    d.candidate_ptr = _i32(ix.candidate_ptr).data_ptr()
    d.has_bug = _req(ix.has_bug, torch.bool, "has_bug").data_ptr()
    d.correct_candidate_idxs = _i32(ix.correct_candidate_idxs).data_ptr()
    d.repair_group_ptr, d.repair_group_items = _p(ix.repair_group_ptr), _p(ix.repair_group_items)
    for k in range(3):
        d.logit_group[k] = _i32(ix.logit_groups[k]).data_ptr() if ix.logit_groups[k].numel() else None
        d.target[k] = _i32(ix.targets[k]).data_ptr() if ix.targets[k].numel() else None
        d.ntarget[k] = int(ix.targets[k].shape[0])
    d.w_buggy, d.abstain_weight = float(w_buggy), float(abstain)
    return d


class _BugLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, loc_scores, logits, sizes, ix: BugLossIndex, w_buggy: float, abstain: float):
        _f32(loc_scores, "loc_scores")
        _f32(logits, "repair logits")
        dev = loc_scores.device
        d = _bug_loss_desc(loc_scores, logits, sizes, ix, w_buggy, abstain)
        loc_lp = torch.empty((d.C + d.B,), dtype=torch.float32, device=dev)
        rep_lp = torch.empty((max(1, logits.shape[0]),), dtype=torch.float32, device=dev)
        gmax = torch.empty((max(1, d.G),), dtype=torch.float32, device=dev)
        out = torch.empty((1 + BUG_LOSS_STATS,), dtype=torch.float32, device=dev)  # [loss | stats]
        _check(load_library().bl_bug_loss_fwd(ctypes.byref(d), loc_lp.data_ptr(), rep_lp.data_ptr(), gmax.data_ptr(), out.data_ptr(),
                                              out[1:].data_ptr(), _stream()), "bl_bug_loss_fwd")
        ctx.saved = (loc_scores, logits, sizes, ix, w_buggy, abstain, loc_lp, rep_lp)
        loss, stats = out[0], out[1:]
        ctx.mark_non_differentiable(stats)
        return loss, stats

    @staticmethod
    def backward(ctx, g_loss, _g_stats):
        loc_scores, logits, sizes, ix, w_buggy, abstain, loc_lp, rep_lp = _take_saved(ctx)
        dev = loc_scores.device
        d = _bug_loss_desc(loc_scores, logits, sizes, ix, w_buggy, abstain)
        scratch = torch.empty((d.C + d.B + logits.shape[0] + 1,), dtype=torch.float32, device=dev)
        g_scores = torch.empty_like(loc_scores)
        g_logits = torch.empty_like(logits)
        g = g_loss.contiguous().reshape(1)
        _check(load_library().bl_bug_loss_bwd(ctypes.byref(d), loc_lp.data_ptr(), rep_lp.data_ptr(), _f32(g).data_ptr(), scratch.data_ptr(),
                                              _p(g_scores), _p(g_logits), _stream()), "bl_bug_loss_bwd")
        return g_scores, g_logits, None, None, None, None


def bug_loss(loc_scores, logits, sizes, ix: BugLossIndex, w_buggy: float = 1.0, abstain_weight: float = 0.0):
    """-> (loss scalar, stats [16]); see include/buglab_hip.h::bl_bug_loss_t.  logits = cat(text, var, swap) with `sizes` rows each."""
    return _BugLoss.apply(loc_scores.contiguous(), logits.contiguous(), tuple(int(n) for n in sizes), ix, float(w_buggy), float(abstain_weight))


# ------------------------------------------------------------------------------------------------
# knowledge distillation (csrc/bl_distill.hip; include/buglab_hip.h::bl_distill_fwd): the soft-target term beside the bug loss
DISTILL_OUT = 8      # bl_distill_fwd's out: [location KL, repair KL | the DISTILL_STATS counters]
DISTILL_STATS = ("distilled_location_segments", "distilled_repair_groups", "location_agreement", "skipped_segments")


def distill_fwd(loc_scores, logits, teacher_loc, teacher_repair, candidate_ptr, repair_group_ptr, repair_group_items,
                temperature: float, delta=None, out=None):
    """bl_distill_fwd -> (delta [C + R], out [8]); `delta` / `out`: write into these buffers instead of fresh ones."""
    C, R = int(loc_scores.shape[0]), int(logits.shape[0])
    B, G = int(candidate_ptr.shape[0]) - 1, int(repair_group_ptr.shape[0]) - 1
    if B < 0 or G < 0:
        raise ValueError("distill_fwd: candidate_ptr and repair_group_ptr need at least one entry")
    if teacher_loc.shape[0] != C + B or teacher_repair.shape[0] != R or repair_group_items.shape[0] != R:
        raise ValueError(f"distill_fwd: teacher_loc has {teacher_loc.shape[0]} entries for {C} candidates + {B} graphs, teacher_repair "
                         f"{teacher_repair.shape[0]} and repair_group_items {repair_group_items.shape[0]} for {R} logits")
    dev = teacher_loc.device
    lib = load_library()
    if delta is None:
        delta = torch.empty((C + R,), dtype=torch.float32, device=dev)
    if out is None:
        out = torch.empty((DISTILL_OUT,), dtype=torch.float32, device=dev)
    if delta.shape[0] != C + R or out.shape[0] != DISTILL_OUT:
        raise ValueError(f"distill_fwd: delta needs {C + R} entries and out {DISTILL_OUT}")
    ws = torch.empty((int(lib.bl_distill_workspace_bytes(B, G)) // 8,), dtype=torch.float64, device=dev)
    _check(lib.bl_distill_fwd(_p(_f32(loc_scores, "loc_scores")), _p(_f32(logits, "repair logits")), _f32(teacher_loc, "teacher_loc").data_ptr(),
                              _p(_f32(teacher_repair, "teacher_repair")), _i32(candidate_ptr, "candidate_ptr").data_ptr(),
                              _i32(repair_group_ptr, "repair_group_ptr").data_ptr(), _p(_i32(repair_group_items, "repair_group_items")),
                              B, G, C, R, float(temperature), ws.data_ptr(), _p(_f32(delta, "delta")), _f32(out, "out").data_ptr(),
                              _stream()), "bl_distill_fwd")
    return delta, out


def distill_bwd(delta, num_candidates: int, g_kl, temperature: float, g_loc_scores=None, g_logits=None):
    """bl_distill_bwd: g_kl = the device gradients of (location KL, repair KL) -> (g_loc_scores [C], g_logits [R])."""
    C = int(num_candidates)
    R = int(delta.shape[0]) - C
    dev = delta.device
    if g_loc_scores is None:
        g_loc_scores = torch.empty((C,), dtype=torch.float32, device=dev)
    if g_logits is None:
        g_logits = torch.empty((R,), dtype=torch.float32, device=dev)
    if R < 0 or g_loc_scores.shape[0] != C or g_logits.shape[0] != R or g_kl.numel() != 2:
        raise ValueError(f"distill_bwd: {delta.shape[0]} deltas do not split into {C} candidates and {g_logits.shape[0]} logits")
    g = _f32(g_kl.contiguous().reshape(2), "g_kl")
    _check(load_library().bl_distill_bwd(_p(_f32(delta, "delta")), C, R, g.data_ptr(), g[1:].data_ptr(), float(temperature),
                                         _p(_f32(g_loc_scores, "g_loc_scores")), _p(_f32(g_logits, "g_logits")), _stream()), "bl_distill_bwd")
    return g_loc_scores, g_logits


class _DistillLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, loc_scores, logits, teacher_loc, teacher_repair, ix: BugLossIndex, temperature: float):
        delta, out = distill_fwd(loc_scores, logits, teacher_loc, teacher_repair, ix.candidate_ptr, ix.repair_group_ptr,
                                 ix.repair_group_items, temperature)
        ctx.saved = (delta, int(loc_scores.shape[0]), temperature)
        kl, stats = out[:2], out[2:]
        ctx.mark_non_differentiable(stats)
        return kl, stats

    @staticmethod
    def backward(ctx, g_kl, _g_stats):
        delta, C, temperature = _take_saved(ctx)
        g_scores, g_logits = distill_bwd(delta, C, g_kl, temperature)
        return g_scores, g_logits, None, None, None, None


def distill_loss(loc_scores, logits, teacher_loc, teacher_repair, ix: BugLossIndex, temperature: float = 1.0):
    """-> (kl [2] = location KL sum, repair KL sum of KL(teacher || student) at `temperature`, differentiable in loc_scores and
    logits; stats [6]: DISTILL_STATS, then two zeros).  See include/buglab_hip.h::bl_distill_fwd."""
    return _DistillLoss.apply(loc_scores.contiguous(), logits.contiguous(), teacher_loc.contiguous(), teacher_repair.contiguous(), ix,
                              float(temperature))


# ------------------------------------------------------------------------------------------------
# GREAT var-misuse head (csrc/bl_varmisuse_head.hip; include/buglab_hip.h::bl_varmisuse_head_t)
def _byte_mask(t: torch.Tensor, name: str) -> torch.Tensor:
    return _req(t.view(torch.uint8) if t.dtype == torch.bool else t, torch.uint8, name)


def _varmisuse_desc(x, ln_g, ln_b, W, bias, lens_att, error_location, cand, tgt, eps: float) -> bl_varmisuse_head_t:
    d = bl_varmisuse_head_t()
    B = int(lens_att.shape[0])
    n, D = x.shape
    if B < 1 or n % B != 0:
        raise ValueError(f"varmisuse_head: x has {n} rows, not a multiple of B = {B}")
    if tuple(W.shape) != (D, 2) or tuple(bias.shape) != (2,) or tuple(ln_g.shape) != (D,) or tuple(ln_b.shape) != (D,):
        raise ValueError(f"varmisuse_head: expected W [{D}, 2], bias [2], ln_g / ln_b [{D}]")
    if cand.numel() != n or tgt.numel() != n or error_location.numel() != B:
        raise ValueError("varmisuse_head: candidate / target masks must have B * L entries and error_location B")
    d.B, d.L, d.D, d.ln_eps = B, n // B, int(D), float(eps)
    d.x, d.ln_g, d.ln_b = _f32(x, "x").data_ptr(), _f32(ln_g, "ln_g").data_ptr(), _f32(ln_b, "ln_b").data_ptr()
    d.W, d.bias = _f32(W, "W").data_ptr(), _f32(bias, "bias").data_ptr()
    d.lens_att, d.error_location = _i32(lens_att, "lens_att").data_ptr(), _i32(error_location, "error_location").data_ptr()
    d.candidate_mask = _byte_mask(cand, "candidate_mask").data_ptr()
    d.target_mask = _byte_mask(tgt, "target_mask").data_ptr()
    return d


def _varmisuse_workspace(d: bl_varmisuse_head_t, dev) -> torch.Tensor:
    nbytes = int(load_library().bl_varmisuse_head_workspace_bytes(d.B, d.L, d.D))
    if nbytes < 0:
        raise ValueError(f"varmisuse_head: unsupported shape B={d.B} L={d.L} D={d.D} (D: a multiple of 4, at most 1024)")
    return torch.empty(((nbytes + 15) // 16 * 4,), dtype=torch.float32, device=dev)


class _VarMisuseHead(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, ln_g, ln_b, W, bias, lens_att, error_location, cand, tgt, stats, eps):
        d = _varmisuse_desc(x, ln_g, ln_b, W, bias, lens_att, error_location, cand, tgt, eps)
        dev = x.device
        n = x.shape[0]
        logits = torch.empty((n, 2), dtype=torch.float32, device=dev)
        mean = torch.empty((n,), dtype=torch.float32, device=dev)
        rstd = torch.empty((n,), dtype=torch.float32, device=dev)
        lse = torch.empty((d.B, 3), dtype=torch.float32, device=dev)
        out = torch.empty((2,), dtype=torch.float32, device=dev)  # [loss | number of buggy samples]
        ws = _varmisuse_workspace(d, dev)
        _req(stats, torch.float64, "stats")
        if stats.numel() != VARMISUSE_STATS:
            raise ValueError(f"varmisuse_head: stats must have {VARMISUSE_STATS} entries")
        _check(load_library().bl_varmisuse_head_fwd(ctypes.byref(d), logits.data_ptr(), mean.data_ptr(), rstd.data_ptr(), lse.data_ptr(),
                                                    ws.data_ptr(), out.data_ptr(), stats.data_ptr(), _stream()), "bl_varmisuse_head_fwd")
        ctx.saved = (x, ln_g, ln_b, W, bias, lens_att, error_location, cand, tgt, eps, logits, mean, rstd, lse, out)
        loss, num_buggy = out[0], out[1]
        ctx.mark_non_differentiable(logits, num_buggy)
        return loss, logits, num_buggy

    @staticmethod
    def backward(ctx, g_loss, _g_logits, _g_num_buggy):
        x, ln_g, ln_b, W, bias, lens_att, error_location, cand, tgt, eps, logits, mean, rstd, lse, out = _take_saved(ctx)
        d = _varmisuse_desc(x, ln_g, ln_b, W, bias, lens_att, error_location, cand, tgt, eps)
        dev = x.device
        ws = _varmisuse_workspace(d, dev)
        g_x = torch.empty_like(x)
        g_W, g_bias = torch.empty_like(W), torch.empty_like(bias)
        g_ln_g, g_ln_b = torch.empty_like(ln_g), torch.empty_like(ln_b)
        g = _f32(g_loss.contiguous().reshape(1), "g_loss")
        _check(load_library().bl_varmisuse_head_bwd(ctypes.byref(d), logits.data_ptr(), mean.data_ptr(), rstd.data_ptr(), lse.data_ptr(),
                                                    out.data_ptr(), g.data_ptr(), ws.data_ptr(), g_x.data_ptr(), g_W.data_ptr(),
                                                    g_bias.data_ptr(), g_ln_g.data_ptr(), g_ln_b.data_ptr(), _stream()),
               "bl_varmisuse_head_bwd")
        return g_x, g_ln_g, g_ln_b, g_W, g_bias, None, None, None, None, None, None


def varmisuse_head(x, ln_g, ln_b, W, bias, lens_att, error_location, candidate_mask, target_mask, stats, eps: float = 1e-5):
    """GREAT's output head (reference greatreimplementation.py:143-174, :202-214) on x [B * L, D]: LayerNorm(ln_g, ln_b), Linear
    (W [D, 2], bias [2]), the masked localization / pointer logits and loss = localization cross-entropy + mean repair loss over
    the buggy samples.  lens_att int32 [B]: unmasked positions per sample; error_location int32 [B]; masks bool / uint8 [B * L].
    `stats` (float64 [VARMISUSE_STATS], on the device) is added to (see include/buglab_hip.h).
    -> (loss scalar, logits [B * L, 2], number of buggy samples as a device scalar); nothing is read back to the host."""
    return _VarMisuseHead.apply(x.contiguous(), ln_g, ln_b, W.contiguous(), bias, lens_att.contiguous(), error_location.contiguous(),
                                candidate_mask.reshape(-1).contiguous(), target_mask.reshape(-1).contiguous(), stats, float(eps))


VARMISUSE_RECORD_D, VARMISUSE_RECORD_I = 7, 4  # rows of a sample's fp64 / int32 prediction record (include/buglab_hip.h)


def varmisuse_predict(x, ln_g, ln_b, W, bias, lens_att, error_locations, candidate_mask, target_mask, out_d, out_i, offset: int,
                      eps: float = 1e-5):
    """The head forward-only (csrc/bl_varmisuse_predict.hip): the masked logits of `varmisuse_head` for the same tensors, bit for
    bit, and every sample judged on the device.  Sample b's record is written at sample offset + b of the run-long buffers
    out_d (float64 [VARMISUSE_RECORD_D, N]: localization lse | pointer lse | log-probabilities of the predicted location, of
    position 0, of the error location, of the predicted repair | repair log-probability over the targets) and out_i (int32
    [VARMISUSE_RECORD_I, N]: predicted location | predicted repair, -1 without a candidate | location correct | repair is a
    target); see include/buglab_hip.h.  error_locations / target_mask: zeros for unlabelled data.  No autograd, no sync.
    -> logits [B * L, 2]."""
    x, W = x.detach(), W.detach()
    if not x.is_contiguous() or not W.is_contiguous():
        raise ValueError("varmisuse_predict: x and W must be contiguous")
    d = _varmisuse_desc(x, ln_g.detach(), ln_b.detach(), W, bias.detach(), lens_att, error_locations, candidate_mask.reshape(-1),
                        target_mask.reshape(-1), eps)
    if d.D % 4 != 0 or d.D > 1024:
        raise ValueError(f"varmisuse_predict: unsupported shape B={d.B} L={d.L} D={d.D} (D: a multiple of 4, at most 1024)")
    _req(out_d, torch.float64, "out_d"), _i32(out_i, "out_i")
    N = out_d.shape[-1]
    if tuple(out_d.shape) != (VARMISUSE_RECORD_D, N) or tuple(out_i.shape) != (VARMISUSE_RECORD_I, N) or out_d.device != x.device \
            or out_i.device != x.device:
        raise ValueError(f"varmisuse_predict: out_d {tuple(out_d.shape)} must be [{VARMISUSE_RECORD_D}, N] and out_i "
                         f"{tuple(out_i.shape)} [{VARMISUSE_RECORD_I}, N], both on {x.device}")
    offset = int(offset)
    if not 0 <= offset <= N - d.B:
        raise ValueError(f"varmisuse_predict: samples {offset} .. {offset + d.B} do not fit the record buffers of {N} samples")
    logits = torch.empty((x.shape[0], 2), dtype=torch.float32, device=x.device)
    _check(load_library().bl_varmisuse_predict(ctypes.byref(d), logits.data_ptr(), out_d.data_ptr(), out_i.data_ptr(), offset, N,
                                               _stream()), "bl_varmisuse_predict")
    return logits
