"""Forward-only device services: ensemble combine, self-supervision scoring / sampling, bug reports, evaluation, confidence
calibration, near-duplicate detection, drift detection, warning grouping, warning triage, review queues, warning tracking."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from ._cabi import HipOpsUnavailable, _check, _f32, _i32, load_library, _p, _req, _stream

__all__ = ["ENSEMBLE_KINDS", "ENSEMBLE_MAX_MEMBERS", "ensemble_combine", "ens_loc_stats", "ens_rw_stats", "ensemble_combine_weighted",
           "SELECTOR_MAX_K", "_f64", "score_targets",
           "selector_sample", "REPORT_MAX_SAMPLES", "REPORT_INDEX_FIELDS", "report_summarize", "report_order", "EVAL_INDEX_FIELDS", "eval_judge",
           "SUGGEST_MAX_K", "SUGGEST_INDEX_FIELDS", "rank_suggestions", "FDR_MAX_REFERENCE", "fdr_counts", "fdr_bh", "fdr_bh_workspace_bytes", "EXPLAIN_MAX_K", "attribute_node_scores", "attribute_topk",
           "SIM_MAX_D", "SIM_MAX_CANDIDATES", "SIM_MAX_SLICES", "SIM_SITE_MODES", "similar_embed_sites", "similar_quantize", "similar_search", "similar_search_slices", "similar_rescore",
           "GROUP_MAX_N", "GROUP_MAX_SLICES", "group_thresholds", "group_link_slices", "group_row_l1", "group_link", "group_labels",
           "TRIAGE_MAX_D", "TRIAGE_MAX_SLICES", "triage_slices", "triage_workspace_bytes", "triage_newton_stats", "triage_score",
           "REVIEW_MAX_ROWS", "REVIEW_MAX_BUDGET", "REVIEW_MAX_SLICES", "REVIEW_MAX_BLOCKS", "REVIEW_ROWS_PER_BLOCK", "review_blocks",
           "review_workspace_bytes", "review_cover_slices", "review_norms", "review_cover", "review_greedy",
           "TRACK_MAX_SLICES", "TRACK_MAX_ROUNDS", "track_slices", "track_best", "track_match",
           "DRIFT_MAX_D", "DRIFT_MAX_PERMUTATIONS", "drift_ok", "drift_mask_ld", "drift_bandwidth", "drift_subsets", "drift_permutation_sums",
           "BOOTSTRAP_MAX_MODELS", "BOOTSTRAP_MAX_SCOUTS", "bootstrap_counts", "CURVE_MAX_BINS", "CURVE_COUNTERS", "bootstrap_curve_counts", "conf_loc_stats", "conf_group_stats", "conf_apply", "DEDUP_MAX_PERM",
           "DEDUP_EMPTY_SLOT", "_i64", "dedup_sha1_u32", "dedup_minhash", "dedup_lsh_insert_query"]


# ------------------------------------------------------------------------------------------------
# ensemble combine (csrc/bl_ensemble.hip; include/buglab_hip.h::bl_ensemble_combine)
ENSEMBLE_KINDS = {"avg": 0, "consensus": 1}  # BL_ENSEMBLE_AVG, BL_ENSEMBLE_CONSENSUS
ENSEMBLE_MAX_MEMBERS = 16  # BL_ENSEMBLE_MAX_MEMBERS


def ensemble_combine(src, loc_idx, loc_off, rw_idx, rw_off, kind: str) -> torch.Tensor:
    """M members' concatenated flat fp32 outputs `src` -> the ensemble's values in the canonical layout, float64
    [total_loc + total_rw] (locations first): ONE buffer, so the caller needs one device->host copy.  loc_idx [M, total_loc] /
    rw_idx [M, total_rw] int32 (-1: member absent from that sample), loc_off / rw_off int32 [B + 1].  No sync."""
    if kind not in ENSEMBLE_KINDS:
        raise ValueError(f"ensemble_combine: kind must be one of {sorted(ENSEMBLE_KINDS)} (got {kind!r})")
    _f32(src, "src")
    _i32(loc_idx, "loc_idx"), _i32(rw_idx, "rw_idx"), _i32(loc_off, "loc_off"), _i32(rw_off, "rw_off")
    M, total_loc = loc_idx.shape
    total_rw = rw_idx.shape[1]
    assert rw_idx.shape[0] == M and loc_off.shape == rw_off.shape
    out = torch.empty(total_loc + total_rw, dtype=torch.float64, device=src.device)
    _check(load_library().bl_ensemble_combine(src.data_ptr(), src.numel(), loc_idx.data_ptr(), loc_off.data_ptr(), total_loc,
                                              rw_idx.data_ptr(), rw_off.data_ptr(), total_rw, M, loc_off.shape[0] - 1,
                                              ENSEMBLE_KINDS[kind], out.data_ptr(), out.data_ptr() + 8 * total_loc, _stream()),
           "bl_ensemble_combine")
    return out


# ------------------------------------------------------------------------------------------------
# fitted ensembles (csrc/bl_ensemble_fit.hip; include/buglab_hip.h::bl_ens_loc_stats, bl_ens_rw_stats,
# bl_ensemble_combine_weighted).  The parameters travel as M host doubles each: the launcher reads them before the launch.
def _member_params(values, M: int, name: str):
    import ctypes

    values = [float(v) for v in values]
    if len(values) != M:
        raise ValueError(f"{name}: {len(values)} values for {M} ensemble members")
    return (ctypes.c_double * M)(*values)


def ens_loc_stats(vals, present, seg_off, tgt, theta, beta) -> torch.Tensor:
    """The weighted ensemble's location loss over a pool of S segments and its gradient, float64 [1 + 2M] = F | dF/dtheta [M] |
    dF/dbeta [M].  vals float32 [M, total]: every member's log-probabilities in the canonical layout, segment s =
    vals[m, seg_off[s] : seg_off[s + 1]], NO_BUG last; present int32 [M, S]; seg_off int32 [S + 1]; tgt int32 [S]: the target's
    place within its segment; theta, beta: M floats each.  Exactly buglab/models/ensemble/_weights.py::loc_stats.  No sync."""
    _f32(vals, "vals"), _i32(present, "present"), _i32(seg_off, "seg_off"), _i32(tgt, "tgt")
    S = tgt.shape[0]
    if vals.dim() != 2 or present.dim() != 2 or tgt.dim() != 1 or tuple(present.shape) != (vals.shape[0], S) or seg_off.dim() != 1 \
            or seg_off.shape[0] != S + 1:
        raise ValueError(f"ens_loc_stats: vals {tuple(vals.shape)} must be [M, total], present {tuple(present.shape)} [M, S], tgt "
                         f"{tuple(tgt.shape)} [S] and seg_off {tuple(seg_off.shape)} [S + 1]")
    M, total = vals.shape
    cols = 1 + 2 * M
    work = (torch.empty if S else torch.zeros)(cols * (S + 1), dtype=torch.float64, device=vals.device)  # [the result | partials]
    _check(load_library().bl_ens_loc_stats(vals.data_ptr(), total, present.data_ptr(), seg_off.data_ptr(), tgt.data_ptr(), M, S,
                                           _member_params(theta, M, "theta"), _member_params(beta, M, "beta"),
                                           work.data_ptr() + 8 * cols, work.data_ptr(), _stream()), "bl_ens_loc_stats")
    return work[:cols]


def ens_rw_stats(vals, present, phi) -> torch.Tensor:
    """The weighted ensemble's rewrite loss over S buggy samples and its gradient, float64 [1 + M] = F | dF/dphi [M].  vals float32
    [M, S]: every member's log-probability of the sample's true rewrite; present int32 [M, S]; phi: M floats.  Exactly
    buglab/models/ensemble/_weights.py::rw_stats.  No sync."""
    _f32(vals, "vals"), _i32(present, "present")
    if vals.dim() != 2 or vals.shape != present.shape:
        raise ValueError(f"ens_rw_stats: vals {tuple(vals.shape)} and present {tuple(present.shape)} must both be [M, S]")
    M, S = vals.shape
    cols = 1 + M
    work = (torch.empty if S else torch.zeros)(cols * (S + 1), dtype=torch.float64, device=vals.device)
    _check(load_library().bl_ens_rw_stats(vals.data_ptr(), present.data_ptr(), M, S, _member_params(phi, M, "phi"),
                                          work.data_ptr() + 8 * cols, work.data_ptr(), _stream()), "bl_ens_rw_stats")
    return work[:cols]


def ensemble_combine_weighted(src, loc_idx, loc_off, rw_idx, rw_off, theta, beta, phi) -> torch.Tensor:
    """`ensemble_combine` for the `weighted` kind: the same arguments without the kind, and the members' location weights theta,
    inverse temperatures beta and rewrite weights phi (M floats each) -> float64 [total_loc + total_rw].  Exactly
    buglab/models/ensemble/_weights.py::combine_weighted.  No sync."""
    _f32(src, "src")
    _i32(loc_idx, "loc_idx"), _i32(rw_idx, "rw_idx"), _i32(loc_off, "loc_off"), _i32(rw_off, "rw_off")
    if loc_idx.dim() != 2 or rw_idx.dim() != 2 or rw_idx.shape[0] != loc_idx.shape[0] or loc_off.dim() != 1 or loc_off.shape[0] < 1 \
            or loc_off.shape != rw_off.shape:
        raise ValueError(f"ensemble_combine_weighted: loc_idx {tuple(loc_idx.shape)} must be [M, total_loc], rw_idx {tuple(rw_idx.shape)} "
                         f"[M, total_rw], loc_off {tuple(loc_off.shape)} and rw_off {tuple(rw_off.shape)} both [B + 1]")
    M, total_loc = loc_idx.shape
    total_rw = rw_idx.shape[1]
    out = torch.empty(total_loc + total_rw, dtype=torch.float64, device=src.device)
    _check(load_library().bl_ensemble_combine_weighted(
        src.data_ptr(), src.numel(), loc_idx.data_ptr(), loc_off.data_ptr(), total_loc, rw_idx.data_ptr(), rw_off.data_ptr(), total_rw,
        M, loc_off.shape[0] - 1, _member_params(theta, M, "theta"), _member_params(beta, M, "beta"), _member_params(phi, M, "phi"),
        out.data_ptr(), out.data_ptr() + 8 * total_loc, _stream()), "bl_ensemble_combine_weighted")
    return out


# ------------------------------------------------------------------------------------------------
# self-supervision services (csrc/bl_selfsup.hip; include/buglab_hip.h::bl_score_targets, bl_selector_sample)
SELECTOR_MAX_K = 32  # BL_SELECTOR_MAX_K


def _f64(t, name="tensor"):
    return _req(t, torch.float64, name)


def score_targets(src, tgt_loc, tgt_rw) -> torch.Tensor:
    """The log-probability a model's flat fp32 output `src` gives to each sample's true fix, float64 [B]:
    src[tgt_loc[b]] + (src[tgt_rw[b]] if tgt_rw[b] >= 0).  tgt_loc / tgt_rw int32 [B].  No sync."""
    _f32(src, "src"), _i32(tgt_loc, "tgt_loc"), _i32(tgt_rw, "tgt_rw")
    if tgt_loc.dim() != 1 or tgt_loc.shape != tgt_rw.shape:
        raise ValueError(f"score_targets: tgt_loc {tuple(tgt_loc.shape)} and tgt_rw {tuple(tgt_rw.shape)} must both be [B]")
    out = torch.empty(tgt_loc.shape[0], dtype=torch.float64, device=src.device)
    _check(load_library().bl_score_targets(src.data_ptr(), src.numel(), tgt_loc.data_ptr(), tgt_rw.data_ptr(), tgt_loc.shape[0],
                                           out.data_ptr(), _stream()), "bl_score_targets")
    return out


def selector_sample(src, rw_idx, rw_loc_idx, rw_off, nobug_idx, u_eps, u, *, temperature: float, epsilon: float, k: int
                    ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Bug selection on a model's flat fp32 output `src` -> (logprob, p, entropy, selected).  Sample b owns the entries
    rw_off[b] + b .. rw_off[b + 1] + b (its rewrites by original index, then NO_BUG) of logprob / p / u (float64
    [total_rw + B]); entropy float64 [B]; selected int32 [B, k]: entry indices within the sample (n_b = NO_BUG) in descending
    Gumbel-key order, -1 padded.  rw_idx / rw_loc_idx int32 [total_rw], rw_off int32 [B + 1], nobug_idx int32 [B], u_eps
    float64 [B], u float64 [total_rw + B] in (0, 1).  No sync."""
    _f32(src, "src")
    _i32(rw_idx, "rw_idx"), _i32(rw_loc_idx, "rw_loc_idx"), _i32(rw_off, "rw_off"), _i32(nobug_idx, "nobug_idx")
    _f64(u_eps, "u_eps"), _f64(u, "u")
    B, total_rw = nobug_idx.shape[0], rw_idx.shape[0]
    if rw_loc_idx.shape != rw_idx.shape or rw_off.shape[0] != B + 1 or u_eps.shape[0] != B or u.shape[0] != total_rw + B:
        raise ValueError(f"selector_sample: inconsistent shapes (B {B}, total_rw {total_rw}, rw_loc_idx {tuple(rw_loc_idx.shape)}, "
                         f"rw_off {tuple(rw_off.shape)}, u_eps {tuple(u_eps.shape)}, u {tuple(u.shape)})")
    values = torch.empty(2 * (total_rw + B) + B, dtype=torch.float64, device=src.device)  # one buffer: [logprob | p | entropy]
    selected = torch.empty((B, int(k)), dtype=torch.int32, device=src.device)
    n = total_rw + B
    _check(load_library().bl_selector_sample(src.data_ptr(), src.numel(), rw_idx.data_ptr(), rw_loc_idx.data_ptr(), rw_off.data_ptr(),
                                             total_rw, nobug_idx.data_ptr(), B, u_eps.data_ptr(), u.data_ptr(), float(temperature),
                                             float(epsilon), int(k), values.data_ptr(), values.data_ptr() + 8 * n,
                                             values.data_ptr() + 16 * n, selected.data_ptr(), _stream()), "bl_selector_sample")
    return values[:n], values[n:2 * n], values[2 * n:], selected


# ------------------------------------------------------------------------------------------------
# bug reports (csrc/bl_report.hip; include/buglab_hip.h::bl_report_summarize, bl_report_order)
REPORT_MAX_SAMPLES = 1 << 20  # BL_REPORT_MAX_SAMPLES
REPORT_INDEX_FIELDS = ("loc_idx", "loc_off", "rw_idx", "rw_off", "rw_eq_target", "grp_rw", "grp_rw_off", "grp_loc", "grp_shown",
                       "grp_off", "tgt_grp", "ground_loc", "nobug_idx")


def report_summarize(src, ix) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """The verdicts of one predict minibatch from a model's flat fp32 output `src` -> (best_rw int32 [total_grp],
    best_range_logprob float64 [total_grp], sample_i int32 [3, B] = pred_loc | pred_is_nobug | is_wrong, sample_d float64
    [2, B] = prediction_logprob | no_bug_logprob).  `ix`: a mapping with the int32 tensors of REPORT_INDEX_FIELDS
    (buglab/models/_report.py::report_indices).  No sync."""
    _f32(src, "src")
    t = {name: _i32(ix[name], name) for name in REPORT_INDEX_FIELDS}
    B, total_loc, total_rw, total_grp = t["nobug_idx"].shape[0], t["loc_idx"].shape[0], t["rw_idx"].shape[0], t["grp_loc"].shape[0]
    sizes = {"loc_off": B + 1, "rw_off": B + 1, "grp_off": B + 1, "tgt_grp": B, "ground_loc": B, "rw_eq_target": total_rw,
             "grp_rw": total_rw, "grp_rw_off": total_grp + 1, "grp_shown": total_grp}
    bad = {name: tuple(t[name].shape) for name, n in sizes.items() if t[name].dim() != 1 or t[name].shape[0] != n}
    if bad:
        raise ValueError(f"report_summarize: inconsistent shapes (B {B}, total_loc {total_loc}, total_rw {total_rw}, "
                         f"total_grp {total_grp}): {bad}")
    best_rw = torch.empty(total_grp, dtype=torch.int32, device=src.device)
    best_range = torch.empty(total_grp, dtype=torch.float64, device=src.device)
    sample_i = torch.empty((3, B), dtype=torch.int32, device=src.device)
    sample_d = torch.empty((2, B), dtype=torch.float64, device=src.device)
    p = lambda name: t[name].data_ptr()
    _check(load_library().bl_report_summarize(
        src.data_ptr(), src.numel(), p("loc_idx"), p("loc_off"), total_loc, p("rw_idx"), p("rw_off"), total_rw, p("rw_eq_target"),
        p("grp_rw"), p("grp_rw_off"), p("grp_loc"), p("grp_shown"), p("grp_off"), total_grp, p("tgt_grp"), p("ground_loc"),
        p("nobug_idx"), B, best_rw.data_ptr(), best_range.data_ptr(), sample_i.data_ptr(), sample_d.data_ptr(), _stream()),
        "bl_report_summarize")
    return best_rw, best_range, sample_i, sample_d


def report_order(keys, keep, *, by_confidence: bool, k: int = 0) -> torch.Tensor:
    """The indices of the samples with keep != 0, int32, in report order: as Python's stable sorted(key=-keys[i]) when
    `by_confidence`, else input order; the first k when k > 0.  keys float64 [n], keep int32 [n].  Syncs (reads the count)."""
    _f64(keys, "keys"), _i32(keep, "keep")
    if keys.dim() != 1 or keys.shape != keep.shape:
        raise ValueError(f"report_order: keys {tuple(keys.shape)} and keep {tuple(keep.shape)} must both be [n]")
    n = keys.shape[0]
    out = torch.full((n,), -1, dtype=torch.int32, device=keys.device)
    count = torch.zeros(1, dtype=torch.int32, device=keys.device)
    _check(load_library().bl_report_order(keys.data_ptr(), keep.data_ptr(), n, int(k), int(bool(by_confidence)), out.data_ptr(),
                                          count.data_ptr(), _stream()), "bl_report_order")
    return out[:int(count.item())]


# ------------------------------------------------------------------------------------------------
# evaluation (csrc/bl_evaluate.hip; include/buglab_hip.h::bl_eval_judge)
EVAL_INDEX_FIELDS = ("loc_idx", "loc_off", "key_node", "rw_idx", "rw_off", "rw_node", "tgt_rw")


def eval_judge(src, ix, out_conf, out_verdict, offset: int, *, assume_buggy: bool = False) -> None:
    """The verdicts of one predict minibatch of B samples from a model's flat fp32 output `src`, written to samples offset ..
    offset + B - 1 of the run-long buffers out_conf (float64 [N]) and out_verdict (int32 [4, N] = warned | location_correct |
    repair_given_location (-1 without a bug) | repaired).  `ix`: a mapping with the int32 tensors of EVAL_INDEX_FIELDS
    (buglab/models/_evaluate.py::eval_indices).  No sync."""
    _f32(src, "src"), _f64(out_conf, "out_conf"), _i32(out_verdict, "out_verdict")
    t = {name: _i32(ix[name], name) for name in EVAL_INDEX_FIELDS}
    B, total_loc, total_rw = t["tgt_rw"].shape[0], t["loc_idx"].shape[0], t["rw_idx"].shape[0]
    sizes = {"loc_idx": total_loc, "loc_off": B + 1, "key_node": total_loc, "rw_idx": total_rw, "rw_off": B + 1, "rw_node": total_rw,
             "tgt_rw": B}
    bad = {name: tuple(t[name].shape) for name, n in sizes.items() if t[name].dim() != 1 or t[name].shape[0] != n}
    if bad:
        raise ValueError(f"eval_judge: inconsistent shapes (B {B}, total_loc {total_loc}, total_rw {total_rw}): {bad}")
    N = out_conf.shape[0]
    if out_conf.dim() != 1 or tuple(out_verdict.shape) != (4, N) or out_conf.device != src.device or out_verdict.device != src.device:
        raise ValueError(f"eval_judge: out_conf {tuple(out_conf.shape)} must be [N] and out_verdict {tuple(out_verdict.shape)} [4, N], "
                         f"both on {src.device}")
    offset = int(offset)
    if not 0 <= offset <= N - B:
        raise ValueError(f"eval_judge: samples {offset} .. {offset + B} do not fit the outcome buffers of {N} samples")
    p = lambda name: t[name].data_ptr()
    _check(load_library().bl_eval_judge(src.data_ptr(), src.numel(), p("loc_idx"), p("loc_off"), p("key_node"), total_loc, p("rw_idx"),
                                        p("rw_off"), p("rw_node"), total_rw, p("tgt_rw"), B, int(bool(assume_buggy)),
                                        out_conf.data_ptr(), out_verdict.data_ptr(), offset, N, _stream()), "bl_eval_judge")


# ------------------------------------------------------------------------------------------------
# ranked suggestions (csrc/bl_suggest.hip; include/buglab_hip.h::bl_rank_suggestions)
SUGGEST_MAX_K = 32  # BL_SUGGEST_MAX_K
SUGGEST_INDEX_FIELDS = ("rw_idx", "rw_loc_idx", "rw_off", "nobug_idx", "tgt_rw", "loc_idx", "loc_off", "key_node", "rw_node")


def rank_suggestions(src, ix, out_rank, out_entry, out_logprob, offset: int, *, k: int, skip_nobug: bool = False) -> None:
    """The k most probable fixes of every sample of one predict minibatch of B samples from a model's flat fp32 output `src`, and
    the ranks of the true fix and the true location, written to samples offset .. offset + B - 1 of the run-long buffers out_rank
    (int32 [2, N] = joint rank | location rank, -1: none), out_entry (int32 [N, k]: entries in rank order, the sample's rewrite
    count = NO_BUG, -1 padded) and out_logprob (float64 [N, k], -inf padded).  `ix`: a mapping with the int32 tensors of
    SUGGEST_INDEX_FIELDS (buglab/models/_suggest.py::suggest_indices).  Exactly buglab/models/_suggest.py::rank_host.  No sync."""
    _f32(src, "src"), _i32(out_rank, "out_rank"), _i32(out_entry, "out_entry"), _f64(out_logprob, "out_logprob")
    t = {name: _i32(ix[name], name) for name in SUGGEST_INDEX_FIELDS}
    k = int(k)
    B, total_loc, total_rw = t["tgt_rw"].shape[0], t["loc_idx"].shape[0], t["rw_idx"].shape[0]
    sizes = {"rw_idx": total_rw, "rw_loc_idx": total_rw, "rw_off": B + 1, "nobug_idx": B, "tgt_rw": B, "loc_idx": total_loc,
             "loc_off": B + 1, "key_node": total_loc, "rw_node": total_rw}
    bad = {name: tuple(t[name].shape) for name, n in sizes.items() if t[name].dim() != 1 or t[name].shape[0] != n}
    if bad:
        raise ValueError(f"rank_suggestions: inconsistent shapes (B {B}, total_loc {total_loc}, total_rw {total_rw}): {bad}")
    if not 1 <= k <= SUGGEST_MAX_K:
        raise ValueError(f"rank_suggestions: k must be in [1, {SUGGEST_MAX_K}] (got {k})")
    N = out_rank.shape[1] if out_rank.dim() == 2 else -1
    if tuple(out_rank.shape) != (2, N) or tuple(out_entry.shape) != (N, k) or tuple(out_logprob.shape) != (N, k) \
            or any(o.device != src.device for o in (out_rank, out_entry, out_logprob)):
        raise ValueError(f"rank_suggestions: out_rank {tuple(out_rank.shape)} must be [2, N], out_entry {tuple(out_entry.shape)} and "
                         f"out_logprob {tuple(out_logprob.shape)} [N, {k}], all on {src.device}")
    offset = int(offset)
    if not 0 <= offset <= N - B:
        raise ValueError(f"rank_suggestions: samples {offset} .. {offset + B} do not fit the result buffers of {N} samples")
    p = lambda name: t[name].data_ptr()
    _check(load_library().bl_rank_suggestions(src.data_ptr(), src.numel(), p("rw_idx"), p("rw_loc_idx"), p("rw_off"), total_rw,
                                              p("nobug_idx"), p("tgt_rw"), p("loc_idx"), p("loc_off"), p("key_node"), total_loc,
                                              p("rw_node"), B, k, int(bool(skip_nobug)), out_entry.data_ptr(), out_logprob.data_ptr(),
                                              out_rank.data_ptr(), offset, N, _stream()), "bl_rank_suggestions")


# ------------------------------------------------------------------------------------------------
# false-discovery-controlled warnings (csrc/bl_fdr.hip; include/buglab_hip.h::bl_fdr_counts, bl_fdr_bh)
FDR_MAX_REFERENCE = 1 << 20  # BL_FDR_MAX_REFERENCE


def fdr_counts(src, nobug_idx, ref, out_score, out_count, offset: int) -> None:
    """The scores src[nobug_idx[b]] of one predict minibatch of B samples and their counts against the sorted reference `ref`
    (c = #{j : ref[j] <= s}, len(ref) for a NaN score), written to samples offset .. offset + B - 1 of the run-long buffers
    out_score (float32 [N]) and out_count (int32 [N]).  src float32 [n_src], nobug_idx int32 [B] (outside src: NaN), ref float32
    [n_ref] ascending without NaN.  Exactly buglab/models/_fdr.py::counts_host.  No sync."""
    _f32(src, "src"), _i32(nobug_idx, "nobug_idx"), _f32(ref, "ref"), _f32(out_score, "out_score"), _i32(out_count, "out_count")
    if src.dim() != 1 or nobug_idx.dim() != 1 or ref.dim() != 1:
        raise ValueError(f"fdr_counts: src {tuple(src.shape)}, nobug_idx {tuple(nobug_idx.shape)} and ref {tuple(ref.shape)} must be "
                         "one-dimensional")
    if not 1 <= ref.shape[0] <= FDR_MAX_REFERENCE:
        raise ValueError(f"fdr_counts: the reference must hold between 1 and {FDR_MAX_REFERENCE} scores (got {ref.shape[0]})")
    B, N = nobug_idx.shape[0], out_score.shape[0]
    if out_score.dim() != 1 or tuple(out_count.shape) != (N,) or any(t.device != src.device for t in (nobug_idx, ref, out_score, out_count)):
        raise ValueError(f"fdr_counts: out_score {tuple(out_score.shape)} and out_count {tuple(out_count.shape)} must both be [N], and "
                         f"every tensor on {src.device}")
    offset = int(offset)
    if not 0 <= offset <= N - B:
        raise ValueError(f"fdr_counts: samples {offset} .. {offset + B} do not fit the result buffers of {N} samples")
    _check(load_library().bl_fdr_counts(src.data_ptr(), src.numel(), nobug_idx.data_ptr(), B, ref.data_ptr(), ref.shape[0],
                                        out_score.data_ptr(), out_count.data_ptr(), offset, N, _stream()), "bl_fdr_counts")


def fdr_bh(count, n_ref: int, q: float, workspace: Optional[torch.Tensor] = None
           ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Benjamini-Hochberg at level q over the counts of N scanned samples against a reference of n_ref scores -> (cutoff int32
    [2] = c* | R[c*] or 0, flag int32 [N], q_value float64 [N], R int32 [n_ref + 1]: a view of the workspace).  count int32 [N],
    values clamped into [0, n_ref].  `workspace`: a uint8 tensor of at least `fdr_bh_workspace_bytes(n_ref)` bytes to reuse (its
    contents do not matter); allocated when None.  Exactly buglab/models/_fdr.py::bh_host.  No sync."""
    _i32(count, "count")
    n_ref, q = int(n_ref), float(q)
    if count.dim() != 1 or count.shape[0] < 1:
        raise ValueError(f"fdr_bh: count {tuple(count.shape)} must be [N] with N >= 1")
    if not 1 <= n_ref <= FDR_MAX_REFERENCE:
        raise ValueError(f"fdr_bh: n_ref must be in [1, {FDR_MAX_REFERENCE}] (got {n_ref})")
    if not 0.0 < q <= 1.0:
        raise ValueError(f"fdr_bh: the level q must be in (0, 1] (got {q})")
    need = fdr_bh_workspace_bytes(n_ref)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=count.device)
    elif _req(workspace, torch.uint8, "workspace").dim() != 1 or workspace.shape[0] < need or workspace.device != count.device:
        raise ValueError(f"fdr_bh: workspace {tuple(workspace.shape)} must be uint8 [>= {need}] on {count.device}")
    N = count.shape[0]
    cutoff = torch.empty(2, dtype=torch.int32, device=count.device)
    flag = torch.empty(N, dtype=torch.int32, device=count.device)
    q_value = torch.empty(N, dtype=torch.float64, device=count.device)
    _check(load_library().bl_fdr_bh(count.data_ptr(), N, n_ref, q, workspace.data_ptr(), cutoff.data_ptr(), flag.data_ptr(),
                                    q_value.data_ptr(), _stream()), "bl_fdr_bh")
    return cutoff, flag, q_value, workspace[:4 * (n_ref + 1)].view(torch.int32)


def fdr_bh_workspace_bytes(n_ref: int) -> int:
    """Bytes of workspace `fdr_bh` needs for a reference of n_ref scores (host arithmetic; no GPU)."""
    return int(load_library().bl_fdr_bh_workspace_bytes(int(n_ref)))


# ------------------------------------------------------------------------------------------------
# explanations (csrc/bl_explain.hip; include/buglab_hip.h::bl_attr_node_scores, bl_attr_topk)
EXPLAIN_MAX_K = 32  # BL_EXPLAIN_MAX_K


def _rows_f32(t, name: str, what: str):
    """an fp32 [N, D] operand whose rows are contiguous and at least D apart (a view with a larger row stride, or an unaligned
    base, is taken as it is)"""
    if not t.is_cuda:
        raise ValueError(f"{what}: {name} is on {t.device}; the kernel only runs on a ROCm GPU")
    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] < 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]) \
            or (t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError(f"{what}: {name} must be float32 [N, D >= 1] with contiguous rows (got {t.dtype} {tuple(t.shape)}, "
                         f"strides {tuple(t.stride())})")
    return t


def attribute_node_scores(x, g, score, *, weight: float = 1.0, accumulate: bool = False) -> None:
    """score[n] = weight * sum_d x[n, d] * g[n, d] in fp64, or that added to score[n] with `accumulate` (the steps of an
    integrated-gradients path).  x, g float32 [N, D] (row strides above D and unaligned bases are fine), score float64 [N].
    Exactly buglab/models/_explain.py::node_scores_host.  No sync."""
    what = "attribute_node_scores"
    _rows_f32(x, "x", what), _rows_f32(g, "g", what)
    if x.shape != g.shape or score.dtype != torch.float64 or tuple(score.shape) != (x.shape[0],) or not score.is_contiguous() \
            or score.device != x.device or g.device != x.device:
        raise ValueError(f"{what}: inconsistent shapes (x {tuple(x.shape)}, g {tuple(g.shape)}, score {score.dtype} {tuple(score.shape)} "
                         f"must be float64 [N], all on {x.device})")
    N, D = x.shape
    ld = lambda t: t.stride(0) if N > 1 else max(t.stride(0), D)
    _check(load_library().bl_attr_node_scores(x.data_ptr(), ld(x), g.data_ptr(), ld(g), N, D, float(weight), int(bool(accumulate)),
                                              score.data_ptr(), _stream()), "bl_attr_node_scores")


def attribute_topk(score, node_off, out_node, out_score, out_sums, offset: int, *, k: int, by_abs: bool = True) -> None:
    """Per graph of one minibatch of B graphs: its k first nodes by |score| (by score when not `by_abs`), the lower index first
    among equals, NaNs never listed, and the sums of score and |score| over its nodes, written to graphs offset .. offset + B - 1
    of the run-long buffers out_node (int32 [C, k]: indices within the graph, -1 padded), out_score (float64 [C, k], 0.0 padded)
    and out_sums (float64 [2, C]).  score float64 [N]; node_off int32 [B + 1].  Exactly buglab/models/_explain.py::topk_host.
    No sync."""
    _f64(score, "score"), _i32(node_off, "node_off"), _i32(out_node, "out_node"), _f64(out_score, "out_score"), _f64(out_sums, "out_sums")
    k = int(k)
    if score.dim() != 1 or node_off.dim() != 1 or node_off.shape[0] < 1:
        raise ValueError(f"attribute_topk: inconsistent shapes (score {tuple(score.shape)} must be [N], node_off {tuple(node_off.shape)} "
                         "[B + 1])")
    if not 1 <= k <= EXPLAIN_MAX_K:
        raise ValueError(f"attribute_topk: k must be in [1, {EXPLAIN_MAX_K}] (got {k})")
    B, N = node_off.shape[0] - 1, score.shape[0]
    C = out_sums.shape[1] if out_sums.dim() == 2 else -1
    if tuple(out_sums.shape) != (2, C) or tuple(out_node.shape) != (C, k) or tuple(out_score.shape) != (C, k) \
            or any(t.device != score.device for t in (node_off, out_node, out_score, out_sums)):
        raise ValueError(f"attribute_topk: inconsistent shapes (out_sums {tuple(out_sums.shape)} must be [2, C], out_node "
                         f"{tuple(out_node.shape)} and out_score {tuple(out_score.shape)} [C, {k}], all on {score.device})")
    offset = int(offset)
    if not 0 <= offset <= C - B:
        raise ValueError(f"attribute_topk: graphs {offset} .. {offset + B} do not fit the result buffers of {C} graphs")
    _check(load_library().bl_attr_topk(score.data_ptr(), node_off.data_ptr(), B, N, k, int(bool(by_abs)), out_node.data_ptr(),
                                       out_score.data_ptr(), out_sums.data_ptr(), offset, C, _stream()), "bl_attr_topk")


# ------------------------------------------------------------------------------------------------
# similar-bug search (csrc/bl_similar.hip; include/buglab_hip.h::bl_sim_embed_sites, bl_sim_quantize, bl_sim_search_i8,
# bl_sim_rescore).  Shapes and ranges are checked first (plain ValueErrors, also without a GPU), devices after.
SIM_MAX_D = 512           # BL_SIM_MAX_D
SIM_MAX_CANDIDATES = 16   # BL_SIM_MAX_CANDIDATES
SIM_MAX_SLICES = 64       # BL_SIM_MAX_SLICES
SIM_SITE_MODES = {"predicted": 0, "truth": 1}  # BL_SIM_SITE_PREDICTED, BL_SIM_SITE_TRUTH


def _sim_dim(D: int, what: str) -> int:
    if not 1 <= int(D) <= SIM_MAX_D:
        raise ValueError(f"{what}: the embedding size D must be in [1, {SIM_MAX_D}] (got {D})")
    return int(D)


def _ld(t, D: int) -> int:
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), D)


def similar_embed_sites(flat, loc_idx, loc_off, cand_rows, h, out_rows, out_place, out_logprob, offset: int, *, mode: str = "predicted",
                        truth=None, skip_nobug: bool = False) -> None:
    """The site of each of the B samples of one predict minibatch and the row of `h` behind it, written to samples offset ..
    offset + B - 1 of the run-long buffers out_rows (float32 [N, D]; zeros without a site), out_place (int32 [N]: the site's place
    among the sample's location entries, -1 without) and out_logprob (float32 [N]).  flat float32 [n_flat]; loc_idx / loc_off
    int32: the PredictionLayout's; cand_rows int32 [n_cand]: the forward's own refs["candidate_nodes"]; h float32 [n_rows, D]
    (any row stride); mode "predicted" (the first maximum; `skip_nobug` leaves NO_BUG out; a winning NO_BUG is no site) or
    "truth" (`truth` int32 [B]: the place, -1 for none).  Exactly buglab/models/_similar.py::embed_sites_host.  No sync."""
    what = "similar_embed_sites"
    if mode not in SIM_SITE_MODES:
        raise ValueError(f"{what}: mode must be one of {sorted(SIM_SITE_MODES)} (got {mode!r})")
    if h.dim() != 2 or loc_off.dim() != 1 or loc_off.shape[0] < 1 or out_rows.dim() != 2:
        raise ValueError(f"{what}: h {tuple(h.shape)} must be [n_rows, D], loc_off {tuple(loc_off.shape)} [B + 1], out_rows "
                         f"{tuple(out_rows.shape)} [N, D]")
    D, B, N = _sim_dim(h.shape[1], what), loc_off.shape[0] - 1, out_rows.shape[0]
    if (mode == "truth") != (truth is not None):
        raise ValueError(f"{what}: `truth` goes with mode 'truth' and with no other")
    if out_rows.shape[1] != D or tuple(out_place.shape) != (N,) or tuple(out_logprob.shape) != (N,) \
            or (truth is not None and tuple(truth.shape) != (B,)):
        raise ValueError(f"{what}: inconsistent shapes (out_rows {tuple(out_rows.shape)} must be [N, {D}], out_place "
                         f"{tuple(out_place.shape)} and out_logprob {tuple(out_logprob.shape)} [N], truth [{B}])")
    offset = int(offset)
    if not 0 <= offset <= N - B:
        raise ValueError(f"{what}: samples {offset} .. {offset + B} do not fit the result buffers of {N} samples")
    _f32(flat, "flat"), _i32(loc_idx, "loc_idx"), _i32(loc_off, "loc_off"), _i32(cand_rows, "cand_rows"), _rows_f32(h, "h", what)
    _f32(out_rows, "out_rows"), _i32(out_place, "out_place"), _f32(out_logprob, "out_logprob")
    if truth is not None:
        _i32(truth, "truth")
    _check(load_library().bl_sim_embed_sites(flat.data_ptr(), flat.numel(), loc_idx.data_ptr(), loc_off.data_ptr(), loc_idx.numel(), B,
                                             cand_rows.data_ptr(), cand_rows.numel(), h.data_ptr(), _ld(h, D), h.shape[0], D, _p(truth),
                                             int(bool(skip_nobug)), SIM_SITE_MODES[mode], out_rows.data_ptr(), out_place.data_ptr(),
                                             out_logprob.data_ptr(), offset, N, _stream()), "bl_sim_embed_sites")


def similar_quantize(x, mean, out_c=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """x float32 [N, D] (any row stride and alignment), mean float32 [D] -> (c float32 [N, D] = x - mean, q int8 [N, Dp], sumsq
    float64 [N], r float64 [N]); Dp = D rounded up to a multiple of 64.  `out_c`: where to write c (x itself centres in place; a
    new contiguous tensor when None).  An invalid row (not finite, or all zero after centring) has q = 0, sumsq = 0, r = 0.
    Exactly buglab/models/_similar.py::quantize_host.  No sync."""
    what = "similar_quantize"
    if x.dim() != 2 or mean.dim() != 1 or mean.shape[0] != x.shape[1]:
        raise ValueError(f"{what}: x {tuple(x.shape)} must be [N, D] and mean {tuple(mean.shape)} [D]")
    N, D = x.shape[0], _sim_dim(x.shape[1], what)
    if out_c is not None and tuple(out_c.shape) != (N, D):
        raise ValueError(f"{what}: out_c {tuple(out_c.shape)} must be [{N}, {D}]")
    _rows_f32(x, "x", what), _f32(mean, "mean")
    c = torch.empty((N, D), dtype=torch.float32, device=x.device) if out_c is None else _rows_f32(out_c, "out_c", what)
    Dp = (D + 63) // 64 * 64
    q = torch.empty((N, Dp), dtype=torch.int8, device=x.device)
    stats = torch.empty((2, N), dtype=torch.float64, device=x.device)
    _check(load_library().bl_sim_quantize(x.data_ptr(), _ld(x, D), mean.data_ptr(), N, D, c.data_ptr(), _ld(c, D), q.data_ptr(),
                                          stats[0].data_ptr(), stats[1].data_ptr(), _stream()), "bl_sim_quantize")
    return c, q, stats[0], stats[1]


def similar_search_slices(Q: int, N: int) -> int:
    """The number of index slices `similar_search` takes by default.  A search workgroup (16 queries x one slice) holds 48 KB of
    LDS and 230 VGPRs, so two are resident per compute unit, 512 on the chip: the grid ceil(Q / 16) x S stays within that one
    round (measured: at Q = 1000 the search takes 0.71 ms with S = 8, 504 workgroups, and 1.26 ms with S = 9, 567: DESIGN.md).
    Each slice ends in a ranking whose cost does not depend on its length, about that of searching 10^4 rows, so no slice is
    shorter than 1024 rows.  The result of a search does not depend on S."""
    tiles_q = max((int(Q) + 15) // 16, 1)
    return max(1, min(SIM_MAX_SLICES, 512 // tiles_q, int(N) // 1024))


def similar_search(qx, rx, qy, ry, candidates: int = SIM_MAX_CANDIDATES, slices: Optional[int] = None
                   ) -> Tuple[torch.Tensor, torch.Tensor]:
    """The exact top `candidates` of every query under the coarse key -> (index int32 [Q, C], -1 padded; key float64 [Q, C], 0.0
    padded), in order: greater key first, the lower index among equals.  qx int8 [Q, Dp] / rx float64 [Q]: the queries; qy int8
    [N, Dp] / ry float64 [N]: the index (`similar_quantize`'s q and r).  `slices`: into how many parts the index is cut (for
    tests and tuning; `similar_search_slices` when None) -- the result does not depend on it.  Exactly
    buglab/models/_similar.py::search_host.  No sync."""
    what = "similar_search"
    C = int(candidates)
    if not 1 <= C <= SIM_MAX_CANDIDATES:
        raise ValueError(f"{what}: candidates must be in [1, {SIM_MAX_CANDIDATES}] (got {candidates})")
    if qx.dim() != 2 or qy.dim() != 2 or qx.shape[1] != qy.shape[1] or qx.shape[1] % 64 or not 64 <= qx.shape[1] <= SIM_MAX_D:
        raise ValueError(f"{what}: qx {tuple(qx.shape)} and qy {tuple(qy.shape)} must be [Q, Dp] and [N, Dp], Dp a multiple of 64 up to "
                         f"{SIM_MAX_D}")
    Q, N, Dp = qx.shape[0], qy.shape[0], qx.shape[1]
    if tuple(rx.shape) != (Q,) or tuple(ry.shape) != (N,):
        raise ValueError(f"{what}: rx {tuple(rx.shape)} must be [{Q}] and ry {tuple(ry.shape)} [{N}]")
    S = similar_search_slices(Q, N) if slices is None else int(slices)
    if not 1 <= S <= SIM_MAX_SLICES:
        raise ValueError(f"{what}: slices must be in [1, {SIM_MAX_SLICES}] (got {slices})")
    _req(qx, torch.int8, "qx"), _req(qy, torch.int8, "qy"), _f64(rx, "rx"), _f64(ry, "ry")
    lib = load_library()
    need = int(lib.bl_sim_search_workspace_bytes(Q, S))
    workspace = torch.empty(max(need // 8, 1), dtype=torch.float64, device=qx.device)
    out_idx = torch.empty((Q, C), dtype=torch.int32, device=qx.device)
    out_key = torch.empty((Q, C), dtype=torch.float64, device=qx.device)
    _check(lib.bl_sim_search_i8(qx.data_ptr(), rx.data_ptr(), Q, qy.data_ptr(), ry.data_ptr(), N, Dp, C, S, workspace.data_ptr(), need,
                                out_idx.data_ptr(), out_key.data_ptr(), _stream()), "bl_sim_search_i8")
    return out_idx, out_key


def similar_rescore(cx, cy, sumsq_y, cand, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The candidates of every query re-scored in fp64 -> (index int32 [Q, k], -1 padded; dot float64 [Q, k], 0.0 padded): the k
    first by key2 = dot |dot| / sumsq_y, the lower index among equals.  cx float32 [Q, D], cy float32 [N, D] (any row stride and
    alignment), sumsq_y float64 [N], cand int32 [Q, C] (-1: none).  Exactly buglab/models/_similar.py::rescore_host.  No sync."""
    what = "similar_rescore"
    if cx.dim() != 2 or cy.dim() != 2 or cx.shape[1] != cy.shape[1] or cand.dim() != 2 or cand.shape[0] != cx.shape[0]:
        raise ValueError(f"{what}: cx {tuple(cx.shape)} must be [Q, D], cy {tuple(cy.shape)} [N, D] and cand {tuple(cand.shape)} [Q, C]")
    Q, N, D, C, k = cx.shape[0], cy.shape[0], _sim_dim(cx.shape[1], what), cand.shape[1], int(k)
    if not 1 <= C <= SIM_MAX_CANDIDATES:
        raise ValueError(f"{what}: the number of candidates must be in [1, {SIM_MAX_CANDIDATES}] (got {C})")
    if not 1 <= k <= C:
        raise ValueError(f"{what}: k must be in [1, C = {C}] (got {k})")
    if tuple(sumsq_y.shape) != (N,):
        raise ValueError(f"{what}: sumsq_y {tuple(sumsq_y.shape)} must be [{N}]")
    _rows_f32(cx, "cx", what), _f64(sumsq_y, "sumsq_y"), _i32(cand, "cand")
    if N:
        _rows_f32(cy, "cy", what)
    out_idx = torch.empty((Q, k), dtype=torch.int32, device=cx.device)
    out_dot = torch.empty((Q, k), dtype=torch.float64, device=cx.device)
    _check(load_library().bl_sim_rescore(cx.data_ptr(), _ld(cx, D), Q, cy.data_ptr(), _ld(cy, D), sumsq_y.data_ptr(), N, D, cand.data_ptr(),
                                         C, k, out_idx.data_ptr(), out_dot.data_ptr(), _stream()), "bl_sim_rescore")
    return out_idx, out_dot


# ------------------------------------------------------------------------------------------------
# warning grouping (csrc/bl_group.hip; include/buglab_hip.h::bl_group_row_l1, bl_group_link, bl_group_labels).  Shapes and
# ranges are checked first (plain ValueErrors, also without a GPU), devices after.
GROUP_MAX_N = 1 << 19    # BL_GROUP_MAX_N
GROUP_MAX_SLICES = 64    # BL_GROUP_MAX_SLICES


def group_thresholds(similarity: float) -> Tuple[float, float]:
    """(s2, K) of a similarity S in (0, 1]: s2 = S S and K = ((16 16129^2) s2) (1 - 2^-40), in double, as include/buglab_hip.h
    states them (buglab/models/_group.py::thresholds is the twin's copy).  ValueError for any other S, NaN included."""
    S = float(similarity)
    if not 0.0 < S <= 1.0:
        raise ValueError(f"group: the similarity must be in (0, 1] (got {similarity})")
    s2 = S * S
    return s2, ((16.0 * 16129.0 * 16129.0) * s2) * (1.0 - 2.0 ** -40)


def group_link_slices(N: int) -> int:
    """Into how many parts `group_link` cuts every tile row's range by default.  Two needs, the greater wins: about 8192
    workgroups, so that the tile rows that hold a large group -- whose pairs are all re-scored -- are spread over the chip; and
    slices of about 1500 tiles at most, because workgroups are handed out slice by slice, so those running at one time walk the
    same part of the int8 image and find it in L2 (measured at 524 288 rows: 371 ms with 1 slice, 248 ms with 16).
    The result does not depend on it."""
    tiles = max((int(N) + 15) // 16, 1)
    return max(1, min(GROUP_MAX_SLICES, max(-(-8192 // tiles), tiles // 1536)))


def group_row_l1(q) -> torch.Tensor:
    """q int8 [N, Dp] (`similar_quantize`'s image) -> l1 int32 [N], l1_i = sum_d |q_id|, exact.  Exactly
    buglab/models/_group.py::row_l1_host.  No sync."""
    what = "group_row_l1"
    if q.dim() != 2 or q.shape[1] % 64 or not 64 <= q.shape[1] <= SIM_MAX_D:
        raise ValueError(f"{what}: q {tuple(q.shape)} must be [N, Dp], Dp a multiple of 64 up to {SIM_MAX_D}")
    _req(q, torch.int8, "q")
    l1 = torch.empty(q.shape[0], dtype=torch.int32, device=q.device)
    _check(load_library().bl_group_row_l1(q.data_ptr(), q.shape[0], q.shape[1], l1.data_ptr(), _stream()), "bl_group_row_l1")
    return l1


def group_link(c, q, sumsq, r, l1, similarity: float, slices: Optional[int] = None
               ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The single-linkage join of N rows with themselves at the cosine `similarity` -> (parent int32 [N], degree int32 [N],
    counters int64 [2] = number of candidates, number of edges).  c float32 [N, D] (any row stride and alignment), q int8 [N, Dp],
    sumsq / r float64 [N]: `similar_quantize`'s outputs; l1 int32 [N]: `group_row_l1`'s.  parent is a forest with parent[x] <= x
    whose trees are the groups (`group_labels` gives every row's root, the smallest row of its group); the forest itself depends on
    the order of the hooks, the groups, the degrees and the counters do not.  `slices`: into how many parts every tile row's range
    is cut (for tests and tuning; `group_link_slices` when None) -- the result does not depend on it.  Labels, degrees and
    counters are exactly buglab/models/_group.py::link_host's.  No sync."""
    what = "group_link"
    s2, K = group_thresholds(similarity)
    if c.dim() != 2 or q.dim() != 2 or q.shape[0] != c.shape[0]:
        raise ValueError(f"{what}: c {tuple(c.shape)} must be [N, D] and q {tuple(q.shape)} [N, Dp]")
    N, D = c.shape[0], _sim_dim(c.shape[1], what)
    Dp = (D + 63) // 64 * 64
    if q.shape[1] != Dp:
        raise ValueError(f"{what}: q {tuple(q.shape)} must be [{N}, {Dp}]: D = {D} rounded up to a multiple of 64")
    if N > GROUP_MAX_N:
        raise ValueError(f"{what}: N = {N} is above {GROUP_MAX_N} rows (the work is N^2 / 2)")
    if tuple(sumsq.shape) != (N,) or tuple(r.shape) != (N,) or tuple(l1.shape) != (N,):
        raise ValueError(f"{what}: sumsq {tuple(sumsq.shape)}, r {tuple(r.shape)} and l1 {tuple(l1.shape)} must be [{N}]")
    S = group_link_slices(N) if slices is None else int(slices)
    if not 1 <= S <= GROUP_MAX_SLICES:
        raise ValueError(f"{what}: slices must be in [1, {GROUP_MAX_SLICES}] (got {slices})")
    _req(q, torch.int8, "q"), _f64(sumsq, "sumsq"), _f64(r, "r"), _i32(l1, "l1")
    if N:
        _rows_f32(c, "c", what)
    parent = torch.arange(N, dtype=torch.int32, device=q.device)
    degree = torch.zeros(N, dtype=torch.int32, device=q.device)
    counters = torch.zeros(2, dtype=torch.int64, device=q.device)
    _check(load_library().bl_group_link(q.data_ptr(), r.data_ptr(), l1.data_ptr(), c.data_ptr(), _ld(c, D), sumsq.data_ptr(), N, D, Dp, s2, K,
                                        S, parent.data_ptr(), degree.data_ptr(), counters.data_ptr(), _stream()), "bl_group_link")
    return parent, degree, counters


def group_labels(parent) -> torch.Tensor:
    """parent int32 [N] (`group_link`'s) -> label int32 [N]: every row's root, the smallest row of its group.  Exactly
    buglab/models/_group.py::labels_host.  No sync."""
    if parent.dim() != 1 or parent.shape[0] > GROUP_MAX_N:
        raise ValueError(f"group_labels: parent {tuple(parent.shape)} must be [N], N up to {GROUP_MAX_N}")
    _i32(parent, "parent")
    label = torch.empty_like(parent)
    _check(load_library().bl_group_labels(parent.data_ptr(), parent.shape[0], label.data_ptr(), _stream()), "bl_group_labels")
    return label


# ------------------------------------------------------------------------------------------------
# drift detection (csrc/bl_drift.hip; include/buglab_hip.h::bl_drift_bandwidth, bl_drift_subsets, bl_drift_permutation_sums).
# Shapes and ranges are checked first (plain ValueErrors, also without a GPU), devices after.
DRIFT_MAX_D = 512                # BL_DRIFT_MAX_D
DRIFT_MAX_PERMUTATIONS = 65533   # BL_DRIFT_MAX_PERMUTATIONS


def drift_ok(D: int, R: int) -> bool:
    """Whether the drift kernels take embeddings of size D and R permutations (bl_drift_ok, restated: no library needed)."""
    return 1 <= int(D) <= DRIFT_MAX_D and 1 <= int(R) <= DRIFT_MAX_PERMUTATIONS


def drift_mask_ld(N: int) -> int:
    """The row stride of the subset mask: N rounded up to a multiple of 32 (bl_drift_mask_ld)."""
    return (int(N) + 31) // 32 * 32


def _drift_sizes(what: str, N: int, n: int, D: int, R: int) -> None:
    if not (2 <= int(n) <= int(N) - 2):
        raise ValueError(f"{what}: both samples need at least 2 rows (got n {n} of N {N})")
    if not drift_ok(D, R):
        raise ValueError(f"{what}: need 1 <= D <= {DRIFT_MAX_D} and 1 <= R <= {DRIFT_MAX_PERMUTATIONS} (got D {D}, R {R})")


def _drift_out(out, shape, dtype, device, name: str, what: str):
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if tuple(out.shape) != tuple(shape) or out.device != device:
        raise ValueError(f"{what}: {name} {tuple(out.shape)} on {out.device} must be {tuple(shape)} on {device}")
    return _req(out, dtype, name)


def drift_bandwidth(z, scale: float = 1.0, out_rownorm=None, out_bandwidth=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """z float32 [N, D] (any row stride and alignment) -> (bandwidth float64 [1], rownorm float32 [N]): s = scale * 2 (mean |z_i|^2
    - |mean z_i|^2) from fp64 column sums, 0 when there is no spread, and every row's |z_i|^2 summed in fp64 and rounded once.
    `out_*`: the caller's tensors to fill.  Twin: buglab/models/_drift.py::bandwidth_host.  No sync."""
    what = "drift_bandwidth"
    if z.dim() != 2 or z.shape[0] < 4 or not 1 <= z.shape[1] <= DRIFT_MAX_D:
        raise ValueError(f"{what}: z {tuple(z.shape)} must be [N >= 4, 1 <= D <= {DRIFT_MAX_D}]")
    scale = float(scale)
    if not 0.0 < scale < float("inf"):
        raise ValueError(f"{what}: the scale must be positive and finite (got {scale})")
    _rows_f32(z, "z", what)
    N, D = z.shape
    rown = _drift_out(out_rownorm, (N,), torch.float32, z.device, "out_rownorm", what)
    bw = _drift_out(out_bandwidth, (1,), torch.float64, z.device, "out_bandwidth", what)
    lib = load_library()
    need = int(lib.bl_drift_bandwidth_workspace_bytes(N, D))
    workspace = torch.empty(max(need // 8, 1), dtype=torch.float64, device=z.device)
    _check(lib.bl_drift_bandwidth(z.data_ptr(), _ld(z, D), N, D, scale, workspace.data_ptr(), need, rown.data_ptr(), bw.data_ptr(),
                                  _stream()), "bl_drift_bandwidth")
    return bw, rown


def drift_subsets(N: int, n: int, R: int, seed: int, device=None, out=None) -> torch.Tensor:
    """The subset mask uint8 [R + 2, drift_mask_ld(N)]: row 0 the observed split (i < n), rows 1 .. R seeded n-subsets of the N
    rows, row R + 1 all ones; bytes beyond N are 0.  `out`: the caller's tensor to fill (then `device` is its own).  Rows 0 .. R
    equal buglab/models/_drift.py::subsets_host bit for bit.  No sync."""
    what = "drift_subsets"
    N, n, R = int(N), int(n), int(R)
    _drift_sizes(what, N, n, 1, R)
    if N > 0x7FFFFFFF:
        raise ValueError(f"{what}: N = {N} is beyond int32")
    ldm = drift_mask_ld(N)
    if out is None and device is None:
        raise ValueError(f"{what}: give a device or an out tensor")
    device = torch.device(device) if out is None else out.device
    if device.type != "cuda":
        raise ValueError(f"{what}: the mask is on {device}; the kernel only runs on a ROCm GPU")
    mask = _drift_out(out, (R + 2, ldm), torch.uint8, device, "out", what)
    _check(load_library().bl_drift_subsets(N, n, R, int(seed) & 0xFFFFFFFFFFFFFFFF, mask.data_ptr(), ldm, _stream()), "bl_drift_subsets")
    return mask


def drift_permutation_sums(z, rownorm, mask, n: int, bandwidth, shift: float = 0.0, *, col_tiles: Optional[int] = None, out_sums=None,
                           out_u0=None, out_rho=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The fused permutation sums -> (sums float64 [2 (R + 1) + 1] = A_0 .. A_R | B_0 .. B_R | S, u0 float64 [N] = U[:, 0], rho
    float64 [N] = K 1) of the RBF kernel matrix K of the pooled rows z float32 [N, D] (any row stride and alignment; the first n
    are the reference), which is never formed.  rownorm float32 [N] and bandwidth float64 [1]: `drift_bandwidth`'s; mask uint8
    [R + 2, drift_mask_ld(N)]: `drift_subsets`'.  shift in [0, 1]: the constant the kernel subtracts from K while it sums (added
    back in fp64: the outputs are of K).  `col_tiles` (4, 8 or 16): how many 16-row groups of the mask a workgroup takes, for tests
    and tuning -- the result does not depend on it.  `out_*`: the caller's tensors to fill.  Reference:
    buglab/models/_drift.py::permutation_sums_host (fp64).  No sync."""
    what = "drift_permutation_sums"
    if z.dim() != 2 or mask.dim() != 2 or rownorm.dim() != 1 or bandwidth.numel() != 1:
        raise ValueError(f"{what}: z {tuple(z.shape)} must be [N, D], mask {tuple(mask.shape)} [R + 2, ld], rownorm "
                         f"{tuple(rownorm.shape)} [N] and bandwidth {tuple(bandwidth.shape)} [1]")
    N, D, R = z.shape[0], z.shape[1], mask.shape[0] - 2
    _drift_sizes(what, N, n, D, R)
    if tuple(mask.shape) != (R + 2, drift_mask_ld(N)) or rownorm.shape[0] != N:
        raise ValueError(f"{what}: mask {tuple(mask.shape)} must be [{R + 2}, {drift_mask_ld(N)}] and rownorm {tuple(rownorm.shape)} [{N}]")
    ct = 0 if col_tiles is None else int(col_tiles)
    if ct not in (0, 4, 8, 16):
        raise ValueError(f"{what}: col_tiles must be 4, 8 or 16 (got {col_tiles})")
    shift = float(shift)
    if not 0.0 <= shift <= 1.0:
        raise ValueError(f"{what}: the shift must be in [0, 1] (got {shift})")
    _rows_f32(z, "z", what), _f32(rownorm, "rownorm"), _req(mask, torch.uint8, "mask"), _f64(bandwidth, "bandwidth")
    sums = _drift_out(out_sums, (2 * (R + 1) + 1,), torch.float64, z.device, "out_sums", what)
    u0 = _drift_out(out_u0, (N,), torch.float64, z.device, "out_u0", what)
    rho = _drift_out(out_rho, (N,), torch.float64, z.device, "out_rho", what)
    lib = load_library()
    need = int(lib.bl_drift_sums_workspace_bytes(N, R))
    workspace = torch.empty(max(need // 8, 1), dtype=torch.float64, device=z.device)
    _check(lib.bl_drift_permutation_sums(z.data_ptr(), _ld(z, D), N, int(n), D, rownorm.data_ptr(), mask.data_ptr(), mask.shape[1], R,
                                         bandwidth.data_ptr(), shift, ct, workspace.data_ptr(), need, sums.data_ptr(), u0.data_ptr(),
                                         rho.data_ptr(), _stream()), "bl_drift_permutation_sums")
    return sums, u0, rho


# ------------------------------------------------------------------------------------------------
# warning triage (csrc/bl_triage.hip; include/buglab_hip.h::bl_triage_newton_stats, bl_triage_score).  Shapes and ranges are
# checked first (plain ValueErrors, also without a GPU), devices after.
TRIAGE_MAX_D = 512       # BL_TRIAGE_MAX_D
TRIAGE_MAX_SLICES = 64   # BL_TRIAGE_MAX_SLICES


def triage_slices(N: int) -> Tuple[int, int]:
    """(number of row slices, rows per slice) of `triage_newton_stats` over N rows, as include/buglab_hip.h states them
    (restated: no library needed).  A function of N alone; the last slice is the ragged one."""
    N = int(N)
    S = max(1, min(TRIAGE_MAX_SLICES, -(-N // 128)))
    return S, (-(-N // S) + 3) // 4 * 4


def triage_workspace_bytes(N: int, D: int) -> int:
    """The bytes of workspace `triage_newton_stats` needs for N rows of size D (bl_triage_workspace_bytes)."""
    if int(N) < 0 or not 1 <= int(D) <= TRIAGE_MAX_D:
        raise ValueError(f"triage_workspace_bytes: need N >= 0 and 1 <= D <= {TRIAGE_MAX_D} (got N {N}, D {D})")
    return int(load_library().bl_triage_workspace_bytes(int(N), int(D)))


def _triage_rows(what: str, x, logprob, shift, scale, w) -> Tuple[int, int]:
    if x.dim() != 2 or not 1 <= x.shape[1] <= TRIAGE_MAX_D:
        raise ValueError(f"{what}: x {tuple(x.shape)} must be [N, 1 <= D <= {TRIAGE_MAX_D}]")
    N, D = x.shape
    if tuple(logprob.shape) != (N,) or tuple(shift.shape) != (D + 1,) or tuple(scale.shape) != (D + 1,) or tuple(w.shape) != (D + 2,):
        raise ValueError(f"{what}: logprob {tuple(logprob.shape)} must be [{N}], shift {tuple(shift.shape)} and scale "
                         f"{tuple(scale.shape)} [{D + 1}] and w {tuple(w.shape)} [{D + 2}]")
    return N, D


def _triage_on_device(what: str, x, logprob, shift, scale, w) -> None:
    if x.shape[0]:
        _rows_f32(x, "x", what)
    _f32(logprob, "logprob"), _f64(shift, "shift"), _f64(scale, "scale"), _f64(w, "w")


def triage_newton_stats(x, logprob, shift, scale, w, y, c, l2: float, *, workspace=None, out=None) -> torch.Tensor:
    """The Newton statistics of the ridge-regularised logistic loss at w over N labelled rows -> ONE float64 buffer [P P + P + 4],
    P = D + 2: H [P, P] | g [P] | L, sum of c over the rows used, rows used, rows skipped -- one device->host copy for the
    caller.  x float32 [N, D] (any row stride and alignment), logprob float32 [N], shift / scale float64 [D + 1], w float64 [P],
    y uint8 [N], c float64 [N] >= 0 or None for all ones, l2 > 0.  `workspace`: a float64 tensor of at least
    triage_workspace_bytes(N, D) bytes to reuse across calls; `out`: the caller's buffer to fill.  H == H^T bit for bit and every
    number has the same bits on every run.  Twin: buglab/models/_triage.py::newton_stats_host (margins bit for bit).  No sync."""
    what = "triage_newton_stats"
    N, D = _triage_rows(what, x, logprob, shift, scale, w)
    P = D + 2
    l2 = float(l2)
    if not 0.0 < l2 < float("inf"):
        raise ValueError(f"{what}: l2 must be positive and finite (got {l2})")
    if tuple(y.shape) != (N,) or (c is not None and tuple(c.shape) != (N,)):
        raise ValueError(f"{what}: y {tuple(y.shape)} and c must be [{N}]")
    _triage_on_device(what, x, logprob, shift, scale, w)
    _req(y, torch.uint8, "y")
    if c is not None:
        _f64(c, "c")
    if out is None:
        out = torch.empty(P * P + P + 4, dtype=torch.float64, device=x.device)
    elif tuple(out.shape) != (P * P + P + 4,):
        raise ValueError(f"{what}: out {tuple(out.shape)} must be [{P * P + P + 4}]")
    _f64(out, "out")
    if N == 0:
        return out.zero_()
    lib = load_library()
    need = int(lib.bl_triage_workspace_bytes(N, D))
    if workspace is None:
        workspace = torch.empty(need // 8, dtype=torch.float64, device=x.device)
    _f64(workspace, "workspace")
    base = out.data_ptr()
    _check(lib.bl_triage_newton_stats(x.data_ptr(), _ld(x, D), logprob.data_ptr(), shift.data_ptr(), scale.data_ptr(), w.data_ptr(),
                                      y.data_ptr(), _p(c), N, D, l2, workspace.data_ptr(), workspace.numel() * 8, base, base + 8 * P * P,
                                      base + 8 * (P * P + P), _stream()), "bl_triage_newton_stats")
    return out


def triage_score(x, logprob, shift, scale, w, out=None) -> torch.Tensor:
    """The margins and probabilities of N rows under w -> float64 [2, N]: row 0 the margin z, row 1 p = sigmoid(z); NaN in both
    for a row with a non-finite entry.  Operands as `triage_newton_stats`.  The margins are exactly
    buglab/models/_triage.py::score_host's.  No sync."""
    what = "triage_score"
    N, D = _triage_rows(what, x, logprob, shift, scale, w)
    _triage_on_device(what, x, logprob, shift, scale, w)
    if out is None:
        out = torch.empty((2, N), dtype=torch.float64, device=x.device)
    elif tuple(out.shape) != (2, N):
        raise ValueError(f"{what}: out {tuple(out.shape)} must be [2, {N}]")
    _f64(out, "out")
    if N:
        _check(load_library().bl_triage_score(x.data_ptr(), _ld(x, D), logprob.data_ptr(), shift.data_ptr(), scale.data_ptr(), w.data_ptr(),
                                              N, D, out.data_ptr(), out.data_ptr() + 8 * N, _stream()), "bl_triage_score")
    return out


# ------------------------------------------------------------------------------------------------
# review queues (csrc/bl_review.hip; include/buglab_hip.h::bl_review_norms, bl_review_cover_i8, bl_review_greedy).  Shapes and
# ranges are checked first (plain ValueErrors, also without a GPU), devices after.
REVIEW_MAX_ROWS = 1 << 20      # BL_REVIEW_MAX_ROWS
REVIEW_MAX_BUDGET = 16384      # BL_REVIEW_MAX_BUDGET
REVIEW_MAX_SLICES = 64         # BL_REVIEW_MAX_SLICES
REVIEW_MAX_BLOCKS = 1024       # BL_REVIEW_MAX_BLOCKS
REVIEW_ROWS_PER_BLOCK = 64     # BL_REVIEW_ROWS_PER_BLOCK


def review_blocks(M: int) -> int:
    """The number of workgroups of a `review_greedy` step over M rows by default, as include/buglab_hip.h states it (restated: no
    library needed): one per 64 rows -- a pass of the step kernel, four lanes per row -- up to 1024, beyond which every workgroup
    takes more passes over a contiguous part of the rows.  A function of M alone; the results do not depend on it."""
    return max(1, min(REVIEW_MAX_BLOCKS, -(-int(M) // REVIEW_ROWS_PER_BLOCK)))


def review_workspace_bytes(M: int) -> int:
    """The bytes of workspace `review_greedy` needs for M rows (bl_review_workspace_bytes): a control word and two sets of
    per-workgroup partials."""
    if not 0 <= int(M) <= REVIEW_MAX_ROWS:
        raise ValueError(f"review_workspace_bytes: M must be in [0, {REVIEW_MAX_ROWS}] (got {M})")
    return int(load_library().bl_review_workspace_bytes(int(M)))


def review_cover_slices(M: int, L: int) -> int:
    """Into how many parts `review_cover` cuts the centres by default: enough workgroups (ceil(M / 16) x S) to fill the chip when
    the rows are few, and no slice shorter than 1024 centres, because every slice ends in a combine whose cost does not depend
    on its length.  The result does not depend on it."""
    tiles = max((int(M) + 15) // 16, 1)
    return max(1, min(REVIEW_MAX_SLICES, 2048 // tiles, int(L) // 1024))


def _review_image(t, name: str, what: str) -> Tuple[int, int]:
    """(rows, row stride) of an int8 image [rows, Dp]: Dp a multiple of 64 up to 512, unit column stride, a row stride that is a
    multiple of 16"""
    if t.dim() != 2 or t.shape[1] % 64 or not 64 <= t.shape[1] <= SIM_MAX_D:
        raise ValueError(f"{what}: {name} {tuple(t.shape)} must be [rows, Dp], Dp a multiple of 64 up to {SIM_MAX_D}")
    if t.shape[0] > REVIEW_MAX_ROWS:
        raise ValueError(f"{what}: {name} has {t.shape[0]} rows, above {REVIEW_MAX_ROWS}")
    ld = _ld(t, t.shape[1])
    if t.dtype != torch.int8 or t.stride(1) != 1 or ld % 16 or ld < t.shape[1]:
        raise ValueError(f"{what}: {name} must be int8 with unit column stride and a row stride that is a multiple of 16 (got {t.dtype}, "
                         f"strides {tuple(t.stride())})")
    if not t.is_cuda:
        raise HipOpsUnavailable(f"{what}: {name} is on {t.device}; the BugLab hot path only runs on a ROCm GPU (no CPU fallback)")
    return t.shape[0], ld


def review_norms(q) -> torch.Tensor:
    """q int8 [M, Dp] (`similar_quantize`'s image; any row stride that is a multiple of 16) -> n int32 [M], n_i = sum_d q_id^2,
    exact; 0 marks an invalid row.  Exactly buglab/models/_review.py::norms_host.  No sync."""
    M, ld = _review_image(q, "q", "review_norms")
    n = torch.empty(M, dtype=torch.int32, device=q.device)
    _check(load_library().bl_review_norms(q.data_ptr(), ld, M, q.shape[1], n.data_ptr(), _stream()), "bl_review_norms")
    return n


def _review_state(what: str, M: int, n, best, near, device):
    if tuple(n.shape) != (M,):
        raise ValueError(f"{what}: n {tuple(n.shape)} must be [{M}]")
    if (best is None) != (near is None):
        raise ValueError(f"{what}: best and near come together")
    if best is None:
        best = torch.full((M,), -2.0, dtype=torch.float64, device=device)
        near = torch.full((M,), -1, dtype=torch.int32, device=device)
    elif tuple(best.shape) != (M,) or tuple(near.shape) != (M,):
        raise ValueError(f"{what}: best {tuple(best.shape)} and near {tuple(near.shape)} must be [{M}]")
    _i32(n, "n"), _f64(best, "best"), _i32(near, "near")
    return best, near


def review_cover(q, n, centres_q, centres_n, best=None, near=None, *, first_id: int = 0, slices: Optional[int] = None
                 ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Applies L centres to M rows -> (best float64 [M], near int32 [M]): per valid row the greatest affinity to a centre and that
    centre's index, the lower index among equals; -2.0 / -1 where nothing covers.  q int8 [M, Dp] / n int32 [M]: the rows
    (`similar_quantize`'s image, `review_norms`' norms); centres_q int8 [L, Dp] / centres_n int32 [L]: the centres, centre j
    carrying the index first_id + j.  `best` / `near`: a state to UPDATE in place (and return) instead of a fresh one -- two
    calls over two parts of the centres equal one call over all.  `slices`: into how many parts the centres are cut (for tests
    and tuning; `review_cover_slices` when None) -- the result does not depend on it.  Exactly
    buglab/models/_review.py::cover_host.  No sync."""
    what = "review_cover"
    if q.dim() != 2 or centres_q.dim() != 2 or q.shape[1] != centres_q.shape[1]:
        raise ValueError(f"{what}: q {tuple(q.shape)} and centres_q {tuple(centres_q.shape)} must be [M, Dp] and [L, Dp]")
    S = review_cover_slices(q.shape[0], centres_q.shape[0]) if slices is None else int(slices)
    if not 1 <= S <= REVIEW_MAX_SLICES:
        raise ValueError(f"{what}: slices must be in [1, {REVIEW_MAX_SLICES}] (got {slices})")
    first_id = int(first_id)
    if first_id < 0 or first_id + centres_q.shape[0] > 0x7FFFFFFF:
        raise ValueError(f"{what}: the centre indices {first_id} .. {first_id + centres_q.shape[0]} leave int32")
    if tuple(centres_n.shape) != (centres_q.shape[0],):
        raise ValueError(f"{what}: centres_n {tuple(centres_n.shape)} must be [{centres_q.shape[0]}]")
    M, ldq = _review_image(q, "q", what)
    L, ldc = _review_image(centres_q, "centres_q", what)
    best, near = _review_state(what, M, n, best, near, q.device)
    _i32(centres_n, "centres_n")
    lib = load_library()
    need = int(lib.bl_review_cover_workspace_bytes(M, S))
    workspace = torch.empty(max((need + 7) // 8, 1), dtype=torch.float64, device=q.device)
    _check(lib.bl_review_cover_i8(q.data_ptr(), ldq, n.data_ptr(), M, centres_q.data_ptr(), ldc, centres_n.data_ptr(), L, first_id,
                                  q.shape[1], S, workspace.data_ptr(), workspace.numel() * 8, best.data_ptr(), near.data_ptr(), _stream()),
           "bl_review_cover_i8")
    return best, near


def review_greedy(q, n, best, near, budget: int, *, eligible=None, stop: float = 1.0, blocks: Optional[int] = None, workspace=None
                  ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """`budget` k-center greedy picks from the cover state -> (picks int32 [B], -1 once the queue has ended; pick_affinity float64
    [B] and pick_near int32 [B]: the pick's `best` and `near` when it was taken, its nearest earlier item; 0.0 and -1 for no
    pick).  UPDATES best float64 [M] / near int32 [M] in place (-2.0 / -1:
    no centre yet): every pick is applied as a centre to every valid row.  q int8 [M, Dp] / n int32 [M] as in `review_cover`;
    eligible uint8 [M] or None for all; stop = S S for a greatest similarity S in (0, 1]: rows with best >= stop are never
    picked.  One call enqueues budget + 1 launches and nothing else: no host synchronisation, no communication between
    workgroups inside a launch.  `blocks`: the number of workgroups (for tests and tuning; `review_blocks(M)` when None) -- the
    results do not depend on it.  `workspace`: a float64 tensor of at least review_workspace_bytes(M) bytes to reuse.  Exactly
    buglab/models/_review.py::greedy_host.  No sync."""
    what = "review_greedy"
    B, stop = int(budget), float(stop)
    if not 0 <= B <= REVIEW_MAX_BUDGET:
        raise ValueError(f"{what}: the budget must be in [0, {REVIEW_MAX_BUDGET}] (got {budget})")
    if not 0.0 < stop <= 1.0:
        raise ValueError(f"{what}: stop must be in (0, 1]: the square of a similarity in (0, 1] (got {stop})")
    G = 0 if blocks is None else int(blocks)
    if blocks is not None and not 1 <= G <= REVIEW_MAX_BLOCKS:
        raise ValueError(f"{what}: blocks must be in [1, {REVIEW_MAX_BLOCKS}] (got {blocks})")
    if best is None or near is None:
        raise ValueError(f"{what}: best and near are the state to update")
    if q.dim() != 2:
        raise ValueError(f"{what}: q {tuple(q.shape)} must be [M, Dp]")
    if eligible is not None and tuple(eligible.shape) != (q.shape[0],):
        raise ValueError(f"{what}: eligible {tuple(eligible.shape)} must be [{q.shape[0]}]")
    M, ldq = _review_image(q, "q", what)
    _review_state(what, M, n, best, near, q.device)
    if eligible is not None:
        _req(eligible, torch.uint8, "eligible")
    picks = torch.empty(B, dtype=torch.int32, device=q.device)
    pick_aff = torch.empty(B, dtype=torch.float64, device=q.device)
    pick_near = torch.empty(B, dtype=torch.int32, device=q.device)
    if B == 0:
        return picks, pick_aff, pick_near
    lib = load_library()
    need = int(lib.bl_review_workspace_bytes(M))
    if workspace is None:
        workspace = torch.empty(need // 8, dtype=torch.float64, device=q.device)
    _f64(workspace, "workspace")
    _check(lib.bl_review_greedy(q.data_ptr(), ldq, n.data_ptr(), _p(eligible), M, q.shape[1], B, stop, G, workspace.data_ptr(),
                                workspace.numel() * 8, best.data_ptr(), near.data_ptr(), picks.data_ptr(), pick_aff.data_ptr(),
                                pick_near.data_ptr(), _stream()), "bl_review_greedy")
    return picks, pick_aff, pick_near


# ------------------------------------------------------------------------------------------------
# warning tracking (csrc/bl_track.hip; include/buglab_hip.h::bl_track_best_i8, bl_track_match).  Shapes and ranges are checked
# first (plain ValueErrors, also without a GPU), devices after.
TRACK_MAX_SLICES = 64      # BL_TRACK_MAX_SLICES
TRACK_MAX_ROUNDS = 4096    # BL_TRACK_MAX_ROUNDS


def track_slices(X: int, Y: int) -> int:
    """Into how many parts `track_best` / `track_match` cut the other side by default: `review_cover_slices`' rule.  The result
    does not depend on it."""
    tiles = max((int(X) + 15) // 16, 1)
    return max(1, min(TRACK_MAX_SLICES, 2048 // tiles, int(Y) // 1024))


def _track_sides(what: str, q_old, n_old, q_new, n_new, key_old, key_new, floor, slices):
    """the checks `track_best` and `track_match` share -> (L, ld_old, N, ld_new, floor, S)"""
    if q_old.dim() != 2 or q_new.dim() != 2 or q_old.shape[1] != q_new.shape[1]:
        raise ValueError(f"{what}: the images {tuple(q_old.shape)} and {tuple(q_new.shape)} must be [L, Dp] and [N, Dp]")
    floor = float(floor)
    if not 0.0 < floor <= 1.0:
        raise ValueError(f"{what}: floor must be in (0, 1]: the square of a similarity in (0, 1] (got {floor})")
    S = track_slices(min(q_old.shape[0], q_new.shape[0]), max(q_old.shape[0], q_new.shape[0])) if slices is None else int(slices)
    if not 1 <= S <= TRACK_MAX_SLICES:
        raise ValueError(f"{what}: slices must be in [1, {TRACK_MAX_SLICES}] (got {slices})")
    if (key_old is None) != (key_new is None):
        raise ValueError(f"{what}: the keys of both sides come together")
    for n, q, name in ((n_old, q_old, "n_old"), (n_new, q_new, "n_new"), (key_old, q_old, "key_old"), (key_new, q_new, "key_new")):
        if n is not None and tuple(n.shape) != (q.shape[0],):
            raise ValueError(f"{what}: {name} {tuple(n.shape)} must be [{q.shape[0]}]")
    L, ld_old = _review_image(q_old, "q_old", what)
    N, ld_new = _review_image(q_new, "q_new", what)
    for t, name in ((n_old, "n_old"), (n_new, "n_new"), (key_old, "key_old"), (key_new, "key_new")):
        if t is not None:
            _i32(t, name)
    return L, ld_old, N, ld_new, floor, S


def track_best(q_old, n_old, q_new, n_new, floor: float, *, key_old=None, key_new=None, open_old=None, open_new=None,
               slices: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The directional best -> (best float64 [L], arg int32 [L]): for each OPEN row of the first side the best admissible OPEN row
    of the second as (affinity, index), the lower index among equals; (-2.0, -1) for none and for a row that is not open.  A pair
    is admissible when both norms are > 0, its affinity (review's) is >= floor and, with keys (int32 per row, both sides or
    neither), the keys are equal.  q_* int8 [rows, Dp] / n_* int32 [rows] (`similar_quantize`'s images, `review_norms`' norms);
    open_* uint8 [rows] or None for all.  The other direction is the same call with the sides exchanged.  `slices`: into how many
    parts the second side is cut (for tests and tuning) -- the result does not depend on it.  Exactly
    buglab/models/_track.py::best_host.  No sync."""
    what = "track_best"
    for mask, q, name in ((open_old, q_old, "open_old"), (open_new, q_new, "open_new")):
        if mask is not None and (q.dim() != 2 or tuple(mask.shape) != (q.shape[0],)):
            raise ValueError(f"{what}: {name} {tuple(mask.shape)} must be [{q.shape[0] if q.dim() == 2 else '?'}]")
    L, ld_old, N, ld_new, floor, S = _track_sides(what, q_old, n_old, q_new, n_new, key_old, key_new, floor, slices)
    for mask, name in ((open_old, "open_old"), (open_new, "open_new")):
        if mask is not None:
            _req(mask, torch.uint8, name)
    best = torch.empty(L, dtype=torch.float64, device=q_old.device)
    arg = torch.empty(L, dtype=torch.int32, device=q_old.device)
    lib = load_library()
    need = int(lib.bl_track_best_workspace_bytes(L, N, S))
    workspace = torch.empty(max((need + 7) // 8, 1), dtype=torch.float64, device=q_old.device)
    _check(lib.bl_track_best_i8(q_old.data_ptr(), ld_old, n_old.data_ptr(), _p(key_old), _p(open_old), L, q_new.data_ptr(), ld_new,
                                n_new.data_ptr(), _p(key_new), _p(open_new), N, q_old.shape[1], floor, S, workspace.data_ptr(),
                                workspace.numel() * 8, best.data_ptr(), arg.data_ptr(), _stream()), "bl_track_best_i8")
    return best, arg


def track_match(q_old, n_old, q_new, n_new, floor: float, match_old, match_new, match_aff, *, max_rounds: int = 16, key_old=None,
                key_new=None, slices: Optional[int] = None, workspace=None, status=None) -> torch.Tensor:
    """Up to `max_rounds` rounds of mutual best from the state it UPDATES in place: match_old int32 [L] / match_new int32 [N] (the
    partner, -1: unmatched; a fresh state is all -1) and match_aff float64 [N] -> status int32 [4] ON THE DEVICE: rounds of this
    call that matched something | pairs matched by this call | whether the matching has ended | open new rows left.  One call
    enqueues every launch of its rounds and nothing else: no host synchronisation, no communication between workgroups inside a
    launch; a call from the state an earlier call left continues the matching.  The caller copies `status` back and calls again
    while the matching has not ended.  `workspace`: a float64 tensor to reuse.  Exactly buglab/models/_track.py::rounds_host.
    No sync."""
    what = "track_match"
    R = int(max_rounds)
    if not 1 <= R <= TRACK_MAX_ROUNDS:
        raise ValueError(f"{what}: max_rounds must be in [1, {TRACK_MAX_ROUNDS}] (got {max_rounds})")
    L, ld_old, N, ld_new, floor, S = _track_sides(what, q_old, n_old, q_new, n_new, key_old, key_new, floor, slices)
    if match_old is None or match_new is None or match_aff is None:
        raise ValueError(f"{what}: match_old, match_new and match_aff are the state to update")
    if tuple(match_old.shape) != (L,) or tuple(match_new.shape) != (N,) or tuple(match_aff.shape) != (N,):
        raise ValueError(f"{what}: the state {tuple(match_old.shape)}, {tuple(match_new.shape)}, {tuple(match_aff.shape)} must be "
                         f"[{L}], [{N}], [{N}]")
    _i32(match_old, "match_old"), _i32(match_new, "match_new"), _f64(match_aff, "match_aff")
    if status is None:
        status = torch.empty(4, dtype=torch.int32, device=q_old.device)
    _i32(status, "status")
    lib = load_library()
    need = int(lib.bl_track_match_workspace_bytes(L, N, S))
    if workspace is None:
        workspace = torch.empty((need + 7) // 8, dtype=torch.float64, device=q_old.device)
    _f64(workspace, "workspace")
    _check(lib.bl_track_match(q_old.data_ptr(), ld_old, n_old.data_ptr(), _p(key_old), L, q_new.data_ptr(), ld_new, n_new.data_ptr(),
                              _p(key_new), N, q_old.shape[1], floor, R, S, workspace.data_ptr(), workspace.numel() * 8,
                              match_old.data_ptr(), match_new.data_ptr(), match_aff.data_ptr(), status.data_ptr(), _stream()),
           "bl_track_match")
    return status


# ------------------------------------------------------------------------------------------------
# paired bootstrap of the evaluation counts (csrc/bl_bootstrap.hip; include/buglab_hip.h::bl_bootstrap_counts)
BOOTSTRAP_MAX_MODELS = 6   # BL_BOOTSTRAP_MAX_MODELS
BOOTSTRAP_MAX_SCOUTS = 64  # BL_BOOTSTRAP_MAX_SCOUTS


def bootstrap_counts(packed, M: int, K: int, seed: int, r0: int, R: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The counts of bootstrap replicates r0 .. r0 + R - 1 over the packed outcome words of n samples, int32 [R, K + M (4 + 2K)]
    (the columns: include/buglab_hip.h; the words: buglab/models/_compare.py::pack_outcomes).  packed int32 [n]: the uint32
    words as the int32 with the same bits.  `out`: at least R rows of a larger buffer to fill (the first R are written and
    returned).  Exactly buglab/models/_compare.py::bootstrap_counts_host.  No sync."""
    _i32(packed, "packed")
    M, K, R = int(M), int(K), int(R)
    if packed.dim() != 1 or packed.shape[0] < 1:
        raise ValueError(f"bootstrap_counts: packed {tuple(packed.shape)} must be [n] with n >= 1")
    if not 1 <= M <= BOOTSTRAP_MAX_MODELS or not 1 <= K <= BOOTSTRAP_MAX_SCOUTS or R < 0 or int(r0) < 0:
        raise ValueError(f"bootstrap_counts: need 1 <= M <= {BOOTSTRAP_MAX_MODELS}, 1 <= K <= {BOOTSTRAP_MAX_SCOUTS}, R >= 0 and "
                         f"r0 >= 0 (got M {M}, K {K}, R {R}, r0 {r0})")
    C = K + M * (4 + 2 * K)
    if out is None:
        out = torch.empty((R, C), dtype=torch.int32, device=packed.device)
    elif _i32(out, "out").dim() != 2 or out.shape[0] < R or out.shape[1] != C or out.device != packed.device:
        raise ValueError(f"bootstrap_counts: out {tuple(out.shape)} must be [>= {R}, {C}] on {packed.device}")
    if R:
        _check(load_library().bl_bootstrap_counts(packed.data_ptr(), packed.shape[0], M, K, int(seed) & 0xFFFFFFFFFFFFFFFF, int(r0), R,
                                                  out.data_ptr(), _stream()), "bl_bootstrap_counts")
    return out[:R]


CURVE_MAX_BINS = 1024  # BL_CURVE_MAX_BINS
CURVE_COUNTERS = 5     # det_true | det_false | full_true | full_false | false_alarm


def bootstrap_curve_counts(packed, bins, M: int, G: int, seed: int, r0: int, R: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The threshold-curve counts of bootstrap replicates r0 .. r0 + R - 1, int32 [R, 1 + M * 5 * G]: column 0 the replicate's
    num_buggy, then [M][5][G] the cumulative counts over bins 0 .. g of the five counters of `_curves_of_ranked` (the columns:
    include/buglab_hip.h).  packed int32 [n] as for `bootstrap_counts`; bins int16 [M, n], each value in [0, G] (G: the sample
    passes no threshold of that model).  The draws are those of `bootstrap_counts`.  `out`: at least R rows of a larger buffer
    to fill (the first R are written and returned).  Exactly buglab/models/_operatingpoint.py::curve_counts_host.  No sync."""
    _i32(packed, "packed"), _req(bins, torch.int16, "bins")
    M, G, R = int(M), int(G), int(R)
    if packed.dim() != 1 or packed.shape[0] < 1:
        raise ValueError(f"bootstrap_curve_counts: packed {tuple(packed.shape)} must be [n] with n >= 1")
    if not 1 <= M <= BOOTSTRAP_MAX_MODELS or not 1 <= G <= CURVE_MAX_BINS or R < 0 or int(r0) < 0:
        raise ValueError(f"bootstrap_curve_counts: need 1 <= M <= {BOOTSTRAP_MAX_MODELS}, 1 <= G <= {CURVE_MAX_BINS}, R >= 0 and "
                         f"r0 >= 0 (got M {M}, G {G}, R {R}, r0 {r0})")
    if tuple(bins.shape) != (M, packed.shape[0]) or bins.device != packed.device:
        raise ValueError(f"bootstrap_curve_counts: bins {tuple(bins.shape)} must be [{M}, {packed.shape[0]}] on {packed.device}")
    C = 1 + M * CURVE_COUNTERS * G
    if out is None:
        out = torch.empty((R, C), dtype=torch.int32, device=packed.device)
    elif _i32(out, "out").dim() != 2 or out.shape[0] < R or out.shape[1] != C or out.device != packed.device:
        raise ValueError(f"bootstrap_curve_counts: out {tuple(out.shape)} must be [>= {R}, {C}] on {packed.device}")
    if R:
        _check(load_library().bl_bootstrap_curve_counts(packed.data_ptr(), bins.data_ptr(), packed.shape[0], M, G,
                                                        int(seed) & 0xFFFFFFFFFFFFFFFF, int(r0), R, out.data_ptr(), _stream()),
               "bl_bootstrap_curve_counts")
    return out[:R]


# ------------------------------------------------------------------------------------------------
# confidence calibration (csrc/bl_confidence.hip; include/buglab_hip.h::bl_conf_loc_stats, bl_conf_group_stats, bl_conf_apply)
def _conf_stats(what: str, cols: int, vals, seg_off, tgt, scalars) -> torch.Tensor:
    _f32(vals, "vals"), _i32(seg_off, "seg_off"), _i32(tgt, "tgt")
    nseg = tgt.shape[0]
    if vals.dim() != 1 or tgt.dim() != 1 or seg_off.dim() != 1 or seg_off.shape[0] != nseg + 1:
        raise ValueError(f"{what}: vals {tuple(vals.shape)} must be [n], tgt {tuple(tgt.shape)} [nseg] and seg_off "
                         f"{tuple(seg_off.shape)} [nseg + 1]")
    work = torch.empty(cols * (nseg + 1), dtype=torch.float64, device=vals.device)  # [the result | cols x nseg partials]
    _check(getattr(load_library(), "bl_" + what)(vals.data_ptr(), vals.numel(), seg_off.data_ptr(), tgt.data_ptr(), nseg, *scalars,
                                                 work.data_ptr() + 8 * cols, work.data_ptr(), _stream()), "bl_" + what)
    return work[:cols]


def conf_loc_stats(vals, seg_off, tgt, beta: float, bias: float) -> torch.Tensor:
    """The calibration loss of a pool of location segments at (beta, bias) and its derivatives, float64 [6] = F | dF/dbeta |
    dF/dbias | d2F/dbeta2 | d2F/dbeta dbias | d2F/dbias2.  vals float32 [n]: the segments' log-probabilities back to back,
    NO_BUG last in each; seg_off int32 [nseg + 1]; tgt int32 [nseg]: the target's place within its segment.  No sync."""
    return _conf_stats("conf_loc_stats", 6, vals, seg_off, tgt, (float(beta), float(bias)))


def conf_group_stats(vals, seg_off, tgt, beta: float) -> torch.Tensor:
    """The same for repair groups under one scale: float64 [3] = F_r | F_r' | F_r''.  No sync."""
    return _conf_stats("conf_group_stats", 3, vals, seg_off, tgt, (float(beta),))


def conf_apply(flat, candidate_ptr, num_samples: int, repair_group_ptr, repair_group_items, *, beta: float, no_bug_bias: float,
               repair_beta: float) -> None:
    """Calibrates a predict minibatch's flat fp32 output [loc | text | var | swap] IN PLACE: each sample's location entries
    (candidates candidate_ptr[b] : candidate_ptr[b + 1], NO_BUG at C + b) become log_softmax(beta * l + no_bug_bias * [NO_BUG]),
    each repair group (the CSR repair_group_ptr / repair_group_items over the entries behind the C + B location entries)
    log_softmax(repair_beta * r).  The location part is left alone when (beta, no_bug_bias) == (1, 0), the repair part when
    repair_beta == 1.  candidate_ptr int32 [B + 1] (C is read from the flat layout: the repair items fill the rest).  No sync."""
    _f32(flat, "flat"), _i32(candidate_ptr, "candidate_ptr"), _i32(repair_group_ptr, "repair_group_ptr")
    _i32(repair_group_items, "repair_group_items")
    B, n_items = int(num_samples), repair_group_items.shape[0]
    if flat.dim() != 1 or candidate_ptr.dim() != 1 or candidate_ptr.shape[0] != B + 1 or repair_group_ptr.dim() != 1 \
            or repair_group_ptr.shape[0] < 1 or repair_group_items.dim() != 1 or flat.shape[0] < B + n_items:
        raise ValueError(f"conf_apply: inconsistent shapes (B {B}, flat {tuple(flat.shape)}, candidate_ptr {tuple(candidate_ptr.shape)}, "
                         f"repair_group_ptr {tuple(repair_group_ptr.shape)}, repair_group_items {tuple(repair_group_items.shape)})")
    C = flat.shape[0] - n_items - B
    do_loc = not (float(beta) == 1.0 and float(no_bug_bias) == 0.0)
    G = repair_group_ptr.shape[0] - 1 if float(repair_beta) != 1.0 else 0
    _check(load_library().bl_conf_apply(flat.data_ptr(), flat.numel(), candidate_ptr.data_ptr(), B if do_loc else 0, C,
                                        repair_group_ptr.data_ptr(), _p(repair_group_items), G, n_items, C + B, float(beta),
                                        float(no_bug_bias), float(repair_beta), _stream()), "bl_conf_apply")


# ------------------------------------------------------------------------------------------------
# near-duplicate detection (csrc/bl_dedup.hip; include/buglab_hip.h::bl_dedup_sha1_u32, bl_dedup_minhash,
# bl_dedup_lsh_insert_query).  torch has no arithmetic on unsigned 32 / 64-bit tensors, so the unsigned buffers travel as
# int32 / int64 tensors holding the same bits.
DEDUP_MAX_PERM = 256  # BL_DEDUP_MAX_PERM
DEDUP_EMPTY_SLOT = -1  # 0xFFFFFFFF


def _i64(t, name="offsets"):
    return _req(t, torch.int64, name)


def dedup_sha1_u32(token_bytes, tok_off) -> torch.Tensor:
    """One hash value per token: the first four bytes of SHA-1(token) as a little-endian uint32 (returned as the int32 with the
    same bits).  token_bytes uint8 [nbytes]: the tokens' UTF-8 bytes back to back; tok_off int64 [ntokens + 1].  No sync."""
    _req(token_bytes, torch.uint8, "token_bytes"), _i64(tok_off, "tok_off")
    if token_bytes.dim() != 1 or tok_off.dim() != 1 or tok_off.shape[0] < 1:
        raise ValueError(f"dedup_sha1_u32: token_bytes {tuple(token_bytes.shape)} must be [nbytes] and tok_off {tuple(tok_off.shape)} [ntokens + 1]")
    n = tok_off.shape[0] - 1
    out = torch.empty(n, dtype=torch.int32, device=token_bytes.device)
    _check(load_library().bl_dedup_sha1_u32(token_bytes.data_ptr(), token_bytes.numel(), tok_off.data_ptr(), n, out.data_ptr(), _stream()),
           "bl_dedup_sha1_u32")
    return out


def dedup_minhash(hashes, doc_off, perm_a, perm_b, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """MinHash signatures int32 [ndocs, num_perm] (uint32 bits) of documents given as token hashes int32 [nhashes] with doc_off
    int64 [ndocs + 1]; perm_a / perm_b int64 [num_perm] (uint64 bits).  `out`: rows of a larger signature matrix to fill.  No sync."""
    _i32(hashes, "hashes"), _i64(doc_off, "doc_off"), _i64(perm_a, "perm_a"), _i64(perm_b, "perm_b")
    if hashes.dim() != 1 or doc_off.dim() != 1 or doc_off.shape[0] < 1 or perm_a.dim() != 1 or perm_a.shape != perm_b.shape:
        raise ValueError(f"dedup_minhash: inconsistent shapes (hashes {tuple(hashes.shape)}, doc_off {tuple(doc_off.shape)}, "
                         f"perm_a {tuple(perm_a.shape)}, perm_b {tuple(perm_b.shape)})")
    ndocs, num_perm = doc_off.shape[0] - 1, perm_a.shape[0]
    if out is None:
        out = torch.empty((ndocs, num_perm), dtype=torch.int32, device=hashes.device)
    elif tuple(_i32(out, "out").shape) != (ndocs, num_perm):
        raise ValueError(f"dedup_minhash: out {tuple(out.shape)} must be [{ndocs}, {num_perm}]")
    _check(load_library().bl_dedup_minhash(hashes.data_ptr(), hashes.numel(), doc_off.data_ptr(), ndocs, perm_a.data_ptr(),
                                           perm_b.data_ptr(), num_perm, out.data_ptr(), _stream()), "bl_dedup_minhash")
    return out


def dedup_lsh_insert_query(sigs, bands: int, rows: int, table, status, *, insert_from: int, query_from: int, total: int
                           ) -> Optional[torch.Tensor]:
    """Files documents insert_from .. total - 1 of sigs (int32 [>= total, num_perm]) in the band index `table` (int32
    [bands, slots], DEDUP_EMPTY_SLOT where empty) and answers for documents query_from .. total - 1: int32 [total - query_from],
    1 = an earlier document shares a whole band (None when query_from == total).  `status` int32 [1], zeroed once by the
    caller: non-zero after a call that broke the load bound (see include/buglab_hip.h).  No sync."""
    _i32(sigs, "sigs"), _i32(table, "table"), _i32(status, "status")
    if sigs.dim() != 2 or table.dim() != 2 or table.shape[0] != bands or sigs.shape[0] < total:
        raise ValueError(f"dedup_lsh_insert_query: sigs {tuple(sigs.shape)} must hold {total} rows and table {tuple(table.shape)} "
                         f"{bands} bands")
    flags = torch.empty(total - query_from, dtype=torch.int32, device=sigs.device) if 0 <= query_from < total else None
    _check(load_library().bl_dedup_lsh_insert_query(sigs.data_ptr(), sigs.shape[1], int(bands), int(rows), table.data_ptr(),
                                                    table.shape[1], int(insert_from), int(query_from), int(total), _p(flags),
                                                    status.data_ptr(), _stream()), "bl_dedup_lsh_insert_query")
    return flags
