"""The index arrays and the NumPy twin of the ranking kernel (csrc/bl_suggest.hip) behind buglab/models/suggest.py and
`evaluate.py --top-k`, and the top-k metrics both evaluation paths print.

An ENTRY of a sample is one of its candidate rewrites (entry i = rewrite i, original index) or NO_BUG (entry n, n = the number
of rewrites).  Its value is the joint log-probability `location_logprobs[reference_nodes[i]] + rewrite_logprobs[i]`, one fp64
addition of two fp32 numbers, and `location_logprobs[NO_BUG]` for NO_BUG: the g_i of bl_selector_sample.  Entries are ranked by
value, the lower index first among equals; an entry whose value is NaN or not above -inf is not rankable (it precedes nothing
and is never listed).  `suggest_indices` states this as int32 arrays (in the collate worker, next to `prediction_layout`);
`hip_ops.rank_suggestions` runs it on the device; `rank_host` runs the same arrays on the host, and `suggestions_of_prediction`
the same rule on one `predict` triple (the host path, and so ensembles).  Nothing here takes an exp: compares, one addition and
integer counts, which is what makes the device equal to the twin bit for bit.

Joint rank 0 is NOT the evaluation report's `repaired`: that takes the best rewrite at the first-maximum location, this ranks
the sums."""
from __future__ import annotations

import math
from typing import Any, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from buglab.models._report import NO_BUG_NODE, location_entries

MAX_K = 32  # BL_SUGGEST_MAX_K


class SuggestIndices(NamedTuple):
    """int32 arrays of one minibatch of B samples for bl_rank_suggestions (include/buglab_hip.h has the contract).  All but
    rw_loc_idx and nobug_idx are the arrays of `EvalIndices`, so one upload serves bl_eval_judge too."""

    rw_idx: np.ndarray      # [total_rw]  flat index of every rewrite, by original rewrite index
    rw_loc_idx: np.ndarray  # [total_rw]  flat index of the location entry of the rewrite's reference node, -1: the node has no key
    rw_off: np.ndarray      # [B + 1]
    nobug_idx: np.ndarray   # [B] flat index of NO_BUG's location entry
    tgt_rw: np.ndarray      # [B] target_fix_action_idx, -1 without a bug
    loc_idx: np.ndarray     # [total_loc] flat index of every location entry, in location-key order (NO_BUG last)
    loc_off: np.ndarray     # [B + 1]
    key_node: np.ndarray    # [total_loc] dense id of the entry's node, -1 for NO_BUG
    rw_node: np.ndarray     # [total_rw]  dense id of the rewrite's reference node


def indices_from_keys(loc_idx: np.ndarray, loc_off: np.ndarray, rw_idx: np.ndarray, rw_off: np.ndarray, datapoints: Sequence[Any],
                      all_keys: Sequence[Sequence[int]]) -> SuggestIndices:
    """The arrays from each sample's location keys in order (NO_BUG last) and the flat indices of its location entries in that
    order.  Nodes are named by their dense id, the index in np.unique(reference_nodes), as in `eval_indices`.  A reference node
    without a key gets rw_loc_idx -1 (`selfsup_indices` asserts there is none: not used here)."""
    B = len(datapoints)
    assert len(all_keys) == B and loc_off.shape[0] == B + 1 and rw_off.shape[0] == B + 1
    key_node = np.empty(loc_idx.shape[0], np.int32)
    rw_node = np.empty(rw_idx.shape[0], np.int32)
    rw_loc = np.empty(rw_idx.shape[0], np.int32)
    nobug = np.empty(B, np.int32)
    tgt_rw = np.full(B, -1, np.int32)
    for b, (point, keys) in enumerate(zip(datapoints, all_keys)):
        nodes, place = np.unique(np.asarray(point["graph"]["reference_nodes"], dtype=np.int64), return_inverse=True)
        lo, hi, r0, r1 = int(loc_off[b]), int(loc_off[b + 1]), int(rw_off[b]), int(rw_off[b + 1])
        assert hi - lo == len(keys) and keys[-1] == NO_BUG_NODE and place.shape[0] == r1 - r0
        dense = np.searchsorted(nodes, np.asarray(keys[:-1], dtype=np.int64))  # every key is a reference node
        key_node[lo:hi - 1] = dense
        key_node[hi - 1] = -1
        entry_of = np.full(nodes.shape[0], -1, np.int64)  # dense id -> flat index of its location entry
        entry_of[dense[::-1]] = loc_idx[lo:hi - 1][::-1]  # (the first key of a node, should a node ever have two)
        rw_node[r0:r1] = place
        rw_loc[r0:r1] = entry_of[place]
        nobug[b] = loc_idx[hi - 1]
        target = point["target_fix_action_idx"]
        if target is not None:
            tgt_rw[b] = int(target)
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    return SuggestIndices(i32(rw_idx), rw_loc, i32(rw_off), nobug, tgt_rw, i32(loc_idx), i32(loc_off), key_node, rw_node)


def suggest_indices(layout, datapoints: Sequence[Any], node_mappings: Optional[Sequence[Dict[int, int]]] = None) -> SuggestIndices:
    """`layout`: the minibatch's `PredictionLayout`; `node_mappings`: the sequence models' node -> token maps
    (`mb["node_mappings"]`), None for graph models."""
    loc_idx, all_keys = location_entries(layout, datapoints, node_mappings)
    return indices_from_keys(loc_idx, layout.loc_off, layout.rw_idx, layout.rw_off, datapoints, all_keys)


# ------------------------------------------------------------------------------------------------
# the one rule, on a vector of fp64 values
def _rankable(values: np.ndarray) -> np.ndarray:
    with np.errstate(invalid="ignore"):
        return values > -np.inf  # False for NaN and -inf


def _first_k(values: np.ndarray, k: int) -> Tuple[np.ndarray, np.ndarray]:
    """-> (entries int32 [k], values float64 [k]): the first min(k, #rankable) entries of the total order, padded -1 / -inf"""
    at = np.flatnonzero(_rankable(values))
    at = at[np.argsort(-values[at], kind="stable")][:k]  # stable: the lower index first among equals
    entries, logprobs = np.full(k, -1, np.int32), np.full(k, -np.inf, np.float64)
    entries[:at.shape[0]], logprobs[:at.shape[0]] = at, values[at]
    return entries, logprobs


def _rank_of(values: np.ndarray, truth: int) -> int:
    """the number of rankable entries that precede entry `truth`; -1 if there is no such entry or it is not rankable"""
    if not 0 <= truth < values.shape[0] or not _rankable(values[truth:truth + 1])[0]:
        return -1
    ok = _rankable(values)
    v, t = values[ok], values[truth]
    return int(np.count_nonzero((v > t) | ((v == t) & (np.flatnonzero(ok) < truth))))


def rank_host(src: np.ndarray, ix: SuggestIndices, k: int, skip_nobug: bool = False) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """bl_rank_suggestions in NumPy, in fp64: -> (rank int32 [2, B] = joint rank | location rank, entry int32 [B, k], logprob
    float64 [B, k]); equal to the device bit for bit, padding included."""
    if not 1 <= int(k) <= MAX_K:
        raise ValueError(f"rank_host: k must be in [1, {MAX_K}] (got {k})")
    k = int(k)
    src = np.asarray(src, dtype=np.float64)

    def read(idx):  # an index outside src reads as NaN, as on the device
        idx = np.asarray(idx, dtype=np.int64)
        out = np.full(idx.shape, np.nan)
        ok = (idx >= 0) & (idx < src.shape[0])
        out[ok] = src[idx[ok]]
        return out

    B = ix.tgt_rw.shape[0]
    rank, entry, logprob = np.empty((2, B), np.int32), np.empty((B, k), np.int32), np.empty((B, k), np.float64)
    for b in range(B):
        lo, hi, r0, r1 = int(ix.loc_off[b]), int(ix.loc_off[b + 1]), int(ix.rw_off[b]), int(ix.rw_off[b + 1])
        n = r1 - r0
        values = read(ix.rw_idx[r0:r1]) + read(ix.rw_loc_idx[r0:r1])
        if not skip_nobug:
            values = np.concatenate([values, read(ix.nobug_idx[b:b + 1])])
        entry[b], logprob[b] = _first_k(values, k)
        target = int(ix.tgt_rw[b])
        has_bug = target >= 0
        rank[0, b] = _rank_of(values, (target if target < n else -1) if has_bug else (-1 if skip_nobug else n))
        loc = read(ix.loc_idx[lo:max(hi - 1, lo) if skip_nobug else hi])
        if not has_bug:
            truth = -1 if skip_nobug or hi == lo else hi - lo - 1
        elif target < n and int(ix.rw_node[r0 + target]) >= 0:
            hits = np.flatnonzero(ix.key_node[lo:lo + loc.shape[0]] == ix.rw_node[r0 + target])
            truth = int(hits[0]) if hits.size else -1
        else:
            truth = -1
        rank[1, b] = _rank_of(loc, truth)
    return rank, entry, logprob


class Ranked(NamedTuple):
    """One sample's ranking: `entries` in order (a rewrite's original index; the number of rewrites = NO_BUG) with their joint
    log-probabilities, and the two ranks (-1: none)."""

    entries: List[int]
    logprobs: List[float]
    truth_rank: int
    truth_location_rank: int


def suggestions_of_prediction(datapoint, location_logprobs: Dict[int, float], rewrite_logprobs: Sequence[float], k: int,
                              assume_buggy: bool = False) -> Ranked:
    """The same rule on one `(datapoint, location_logprobs, rewrite_logprobs)` triple of `model.predict`.  The triple holds fp32
    values as Python floats, so the fp64 sum is the number the device forms.  A reference node without a location key makes its
    rewrites NaN (not rankable); with `assume_buggy` NO_BUG does not take part."""
    if not 1 <= int(k) <= MAX_K:
        raise ValueError(f"suggestions_of_prediction: k must be in [1, {MAX_K}] (got {k})")
    refs = datapoint["graph"]["reference_nodes"]
    assert len(refs) == len(rewrite_logprobs)
    nan = math.nan
    values = [float(rw) + float(location_logprobs.get(int(node), nan)) for node, rw in zip(refs, rewrite_logprobs)]
    if not assume_buggy:
        values.append(float(location_logprobs.get(NO_BUG_NODE, nan)))
    values = np.asarray(values, dtype=np.float64)
    keys = [int(key) for key in location_logprobs if not (assume_buggy and key == NO_BUG_NODE)]
    loc = np.asarray([float(location_logprobs[key]) for key in keys], dtype=np.float64)
    target = datapoint["target_fix_action_idx"]
    if target is None:
        truth = -1 if assume_buggy else len(refs)
        truth_loc = keys.index(NO_BUG_NODE) if NO_BUG_NODE in keys else -1
    else:
        truth = int(target) if 0 <= int(target) < len(refs) else -1
        node = int(refs[target]) if truth >= 0 else None
        truth_loc = keys.index(node) if node in keys and node != NO_BUG_NODE else -1
    entries, logprobs = _first_k(values, int(k))
    listed = int(np.count_nonzero(entries >= 0))
    return Ranked(entries[:listed].tolist(), logprobs[:listed].tolist(), _rank_of(values, truth), _rank_of(loc, truth_loc))


# ------------------------------------------------------------------------------------------------
# the top-k metrics of evaluate.py --top-k: ONE set of formulas, on columns, for both evaluation paths
def top_k_summary(joint_rank, location_rank, has_bug, scout, scout_names: Sequence[str], k: int) -> Dict[str, Any]:
    """`joint_rank` / `location_rank`: int32 [n], the rank of the truth among the sample's entries / location entries (-1:
    none); `has_bug` bool [n]; `scout` ids into `scout_names` (id 0 = "NoBug").  For j = 1..k the number of samples whose truth
    is within the top j (0 <= rank < j) over all, buggy and non-buggy samples; the mean reciprocal rank 1 / (rank + 1), a rank
    of -1 contributing 0; per scout the buggy samples within the top k; the histograms of the two columns."""
    k = int(k)
    assert k >= 1
    has_bug = np.asarray(has_bug, dtype=bool)
    scout = np.asarray(scout, dtype=np.int64)
    groups = {"all": np.ones(has_bug.shape[0], dtype=bool), "buggy": has_bug, "correct": ~has_bug}
    out: Dict[str, Any] = {"k": k, "num_samples": {name: int(np.count_nonzero(rows)) for name, rows in groups.items()}}
    for what, column in (("joint", joint_rank), ("location", location_rank)):
        column = np.asarray(column, dtype=np.int64)
        assert column.shape == has_bug.shape == scout.shape
        listed = column >= 0
        reciprocal = np.where(listed, 1.0 / (np.where(listed, column, 0) + 1.0), 0.0)
        ranks, counts = np.unique(column, return_counts=True)
        out[what] = {
            "within": {name: [int(np.count_nonzero(listed & (column < j) & rows)) for j in range(1, k + 1)] for name, rows in groups.items()},
            "mrr": {name: float(reciprocal[rows].sum() / np.count_nonzero(rows)) if rows.any() else float("nan") for name, rows in groups.items()},
            "histogram": [[int(r), int(c)] for r, c in zip(ranks, counts)],
        }
    totals = np.bincount(scout[has_bug], minlength=len(scout_names))
    per_scout = {}
    for name, i in sorted((n, i) for i, n in enumerate(scout_names)):
        if i and totals[i]:
            rows = has_bug & (scout == i)
            within = lambda column: int(np.count_nonzero(rows & (np.asarray(column) >= 0) & (np.asarray(column) < k)))
            per_scout[name] = {"joint": within(joint_rank), "location": within(location_rank), "total": int(totals[i])}
    out["per_scout"] = per_scout
    return out


def format_top_k(s: Dict[str, Any]) -> str:
    """The block `evaluate.py --top-k` prints after the report."""
    k, n = s["k"], s["num_samples"]
    share = lambda c, total: f"{c / total:.2%} ({c}/{total})" if total else "NaN (0/0)"
    mrr = lambda x: "NaN" if x != x else f"{x:.4f}"
    bar, lines = "=" * 34, []
    add = lines.append
    add(bar)
    add(f"Ranked Suggestions (top {k}): the rank of the true fix among a sample's rewrites and NO_BUG by joint probability.")
    add("Top-1 here is not the Accuracy above: that takes the best rewrite at the most probable location.")
    for title, what in (("Fix (Localization & Repair)", "joint"), ("Location", "location")):
        add(bar)
        for j in range(1, k + 1):
            w = s[what]["within"]
            add(f"{title} within top {j}: {share(w['all'][j - 1], n['all'])}  buggy {share(w['buggy'][j - 1], n['buggy'])}  "
                f"non-buggy {share(w['correct'][j - 1], n['correct'])}")
        m = s[what]["mrr"]
        add(f"{title} mean reciprocal rank: {mrr(m['all'])}  buggy {mrr(m['buggy'])}  non-buggy {mrr(m['correct'])}")
    add(bar)
    add(f"Buggy samples within top {k}, by scout (fix | location)")
    for scout, c in s["per_scout"].items():
        add(f"\t{scout}: {c['joint'] / c['total']:.1%} ({c['joint']}/{c['total']}) | {c['location'] / c['total']:.1%} ({c['location']}/{c['total']})")
    return "\n".join(lines) + "\n"
