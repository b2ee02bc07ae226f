"""The index arrays and the NumPy twins of the two report kernels (csrc/bl_report.hip) behind buglab/models/visualize.py.

What decides whether and where a sample appears in a bug report -- its predicted location, the best rewrite of every code
range, its confidence and the "mistake" flag (reference buglab/models/visualize.py:75-144) -- is a segmented reduction over
the model's flat output.  `report_indices` states that reduction as int32 arrays (in the collate worker, next to
`prediction_layout`); `hip_ops.report_summarize` / `report_order` run it on the device; `summarize_host` / `order_host` run
the same arrays on the host, for `predictions_to_html`'s callers that already hold `predict` triples and for a CPU device.

A LOCATION ENTRY of a sample is named by its position in the key order of the dict `predict` yields (graph models:
np.unique(reference_nodes) ascending, then NO_BUG; sequence models: the order `_iter_per_sample_results` builds, NO_BUG last).
Positions, not flat indices: two nodes of a sequence model that map to one token share a flat index and stay two keys."""
from __future__ import annotations

from typing import Any, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from buglab.utils.text import Range, as_range, shown_ranges

NO_BUG_NODE = -1


class SampleGroups(NamedTuple):
    """One sample's range groups: rewrites whose `candidate_rewrite_ranges` entries are equal share a group, groups numbered
    by first occurrence."""

    ranges: List[Range]       # [G] the group's range
    rw_grp: np.ndarray        # [n_rw] group of each rewrite
    rw_eq_target: np.ndarray  # [n_rw] 1: the rewrite's value == the target rewrite's value (all 0 without a target)
    grp_loc: np.ndarray       # [G] location entry of the node of the group's LAST rewrite (-1: the node has none)
    grp_shown: np.ndarray     # [G] 1: the range survives text_to_range_segments (of two colliding ranges only the later does)
    tgt_grp: int              # group of the target rewrite, -1 for NO_BUG
    ground_loc: int           # location entry of reference_nodes[target]; NO_BUG's without a target; -2: the node has none


def location_keys(datapoint, node_mapping: Optional[Dict[int, int]] = None) -> List[int]:
    """The keys of the location dict `predict` yields for this datapoint, in its order (NO_BUG = -1 last)."""
    nodes = np.unique(np.asarray(datapoint["graph"]["reference_nodes"], dtype=np.int64)).tolist()
    if node_mapping is None:
        return nodes + [NO_BUG_NODE]
    # sequence models (basemodel.py::_iter_per_sample_results): token by token in order of first use, and per token the nodes
    # that map to it in the order of the node -> token map
    in_refs = set(nodes)
    by_token: Dict[int, List[int]] = {}
    for old, new in node_mapping.items():
        if old in in_refs:
            by_token.setdefault(new, []).append(old)
    keys: List[int] = []
    for token in dict.fromkeys(node_mapping[k] for k in nodes):
        keys.extend(by_token[token])
    return keys + [NO_BUG_NODE]


def sample_groups(datapoint, keys: Sequence[int]) -> SampleGroups:
    """`keys`: the sample's location keys in order (`location_keys`, or the keys of a `predict` dict)."""
    graph = datapoint["graph"]
    refs = graph["reference_nodes"]
    rewrites = datapoint["candidate_rewrites"]
    place = {int(k): i for i, k in enumerate(keys)}
    group_of: Dict[Range, int] = {}
    rw_grp = np.empty(len(refs), np.int32)
    node_of: List[int] = []
    for i, (node, rng) in enumerate(zip(refs, datapoint["candidate_rewrite_ranges"])):
        g = group_of.setdefault(as_range(rng), len(group_of))
        if g == len(node_of):
            node_of.append(int(node))
        else:
            node_of[g] = int(node)  # the last rewrite with this range names the group's node
        rw_grp[i] = g
    ranges = list(group_of)
    shown = set(shown_ranges(as_range(graph["code_range"]), ranges).values())
    grp_shown = np.array([r in shown for r in ranges], dtype=np.int32)
    grp_loc = np.array([place.get(n, -1) for n in node_of], dtype=np.int32)
    target = datapoint["target_fix_action_idx"]
    if target is None:
        return SampleGroups(ranges, rw_grp, np.zeros(len(refs), np.int32), grp_loc, grp_shown, -1, place.get(NO_BUG_NODE, -2))
    value = rewrites[target]
    rw_eq = np.array([r == value for r in rewrites], dtype=np.int32)
    return SampleGroups(ranges, rw_grp, rw_eq, grp_loc, grp_shown, int(rw_grp[target]), place.get(int(refs[target]), -2))


class ReportIndices(NamedTuple):
    """int32 arrays of one minibatch of B samples for bl_report_summarize (include/buglab_hip.h has the contract).  `rw_grp` is
    the per-rewrite form of the grouping; `grp_rw` / `grp_rw_off` is the same grouping as a CSR (a stable sort of the rewrites
    by group), which is what the kernel walks so that a group's rewrites are contiguous."""

    loc_idx: np.ndarray       # [total_loc] flat index of every location entry, in location-key order
    loc_off: np.ndarray       # [B + 1]
    rw_idx: np.ndarray        # [total_rw]  flat index of every rewrite, by original rewrite index
    rw_off: np.ndarray        # [B + 1]
    rw_grp: np.ndarray        # [total_rw]  sample-local group
    rw_eq_target: np.ndarray  # [total_rw]
    grp_rw: np.ndarray        # [total_rw]  positions in rw_idx, group by group
    grp_rw_off: np.ndarray    # [total_grp + 1]
    grp_loc: np.ndarray       # [total_grp]
    grp_shown: np.ndarray     # [total_grp]
    grp_off: np.ndarray       # [B + 1]
    tgt_grp: np.ndarray       # [B]
    ground_loc: np.ndarray    # [B]
    nobug_idx: np.ndarray     # [B] flat index of NO_BUG's entry


def assemble(loc_idx: np.ndarray, loc_off: np.ndarray, rw_idx: np.ndarray, rw_off: np.ndarray, groups: Sequence[SampleGroups]
             ) -> ReportIndices:
    B = len(groups)
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    cat = lambda arrays: np.concatenate(arrays) if arrays else np.zeros(0, np.int32)
    grp_off = np.zeros(B + 1, np.int64)
    np.cumsum([len(s.ranges) for s in groups], out=grp_off[1:])
    rw_grp = cat([s.rw_grp for s in groups])
    assert rw_grp.shape[0] == rw_idx.shape[0]
    # minibatch-wide group of every rewrite -> the CSR
    wide = rw_grp.astype(np.int64) + np.repeat(grp_off[:-1], np.diff(rw_off))
    grp_rw = np.argsort(wide, kind="stable")
    grp_rw_off = np.zeros(int(grp_off[-1]) + 1, np.int64)
    np.cumsum(np.bincount(wide, minlength=int(grp_off[-1])), out=grp_rw_off[1:])
    nobug = loc_idx[np.asarray(loc_off[1:], dtype=np.int64) - 1] if B else np.zeros(0, np.int32)
    return ReportIndices(i32(loc_idx), i32(loc_off), i32(rw_idx), i32(rw_off), i32(rw_grp), i32(cat([s.rw_eq_target for s in groups])),
                         i32(grp_rw), i32(grp_rw_off), i32(cat([s.grp_loc for s in groups])), i32(cat([s.grp_shown for s in groups])),
                         i32(grp_off), i32([s.tgt_grp for s in groups]), i32([s.ground_loc for s in groups]), i32(nobug))


def location_entries(layout, datapoints: Sequence[Any], node_mappings: Optional[Sequence[Dict[int, int]]] = None
                     ) -> Tuple[np.ndarray, List[List[int]]]:
    """-> (`layout.loc_idx` with every sample's entries in the key order of the dict `predict` yields, each sample's location
    keys in that order).  The layout's own order is canonical (np.unique(reference_nodes), NO_BUG): graph models keep it, the
    sequence models' keys go token by token (`location_keys`).  Shared by the report and the evaluation index arrays."""
    assert len(datapoints) == layout.num_samples
    loc_idx = layout.loc_idx.copy()
    all_keys = []
    for b, point in enumerate(datapoints):
        keys = location_keys(point, None if node_mappings is None else node_mappings[b])
        lo, hi = int(layout.loc_off[b]), int(layout.loc_off[b + 1])
        assert hi - lo == len(keys) and int(layout.rw_off[b + 1]) - int(layout.rw_off[b]) == len(point["candidate_rewrites"])
        if node_mappings is not None:
            canonical = {n: i for i, n in enumerate(sorted(keys[:-1]))}
            loc_idx[lo:hi - 1] = layout.loc_idx[lo:hi - 1][[canonical[k] for k in keys[:-1]]]
        all_keys.append(keys)
    return loc_idx, all_keys


def report_indices(layout, datapoints: Sequence[Any], node_mappings: Optional[Sequence[Dict[int, int]]] = None
                   ) -> Tuple[ReportIndices, List[SampleGroups], List[List[int]]]:
    """-> (the minibatch's arrays, each sample's groups, each sample's location keys).  `layout`: the minibatch's
    `PredictionLayout` (canonical location order: np.unique(reference_nodes), NO_BUG); `node_mappings`: the sequence
    models' node -> token maps (`mb["node_mappings"]`), None for graph models."""
    loc_idx, all_keys = location_entries(layout, datapoints, node_mappings)
    groups = [sample_groups(point, keys) for point, keys in zip(datapoints, all_keys)]
    return assemble(loc_idx, layout.loc_off, layout.rw_idx, layout.rw_off, groups), groups, all_keys


# ------------------------------------------------------------------------------------------------
def _first_max(values: np.ndarray) -> int:
    """Python's max(): the first value stays unless a later one is greater -- a NaN in front wins, a NaN elsewhere never."""
    if values[0] != values[0]:
        return 0
    return int(np.argmax(np.where(np.isnan(values), -np.inf, values)))


def summarize_host(src: np.ndarray, ix: ReportIndices) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """bl_report_summarize in NumPy: -> (best_rw int32 [total_grp], best_range_logprob float64 [total_grp], sample_i int32
    [3, B] = pred_loc | pred_is_nobug | is_wrong, sample_d float64 [2, B] = prediction_logprob | no_bug_logprob)."""
    src = np.asarray(src, dtype=np.float64)
    B = ix.nobug_idx.shape[0]
    best_rw = np.empty(ix.grp_loc.shape[0], np.int32)
    best_range = np.empty(ix.grp_loc.shape[0], np.float64)
    sample_i, sample_d = np.empty((3, B), np.int32), np.empty((2, B), np.float64)
    for b in range(B):
        loc = src[ix.loc_idx[ix.loc_off[b]:ix.loc_off[b + 1]]]
        pred = _first_max(loc) if loc.size else 0
        r0, g0, g1 = int(ix.rw_off[b]), int(ix.grp_off[b]), int(ix.grp_off[b + 1])
        tg = int(ix.tgt_grp[b])
        logprob, wrong = -np.inf, int(ix.ground_loc[b] != pred)
        for g in range(g0, g1):
            members = ix.grp_rw[ix.grp_rw_off[g]:ix.grp_rw_off[g + 1]]
            values = src[ix.rw_idx[members]]
            j = _first_max(values)
            gl = int(ix.grp_loc[g])
            best_rw[g] = members[j] - r0
            best_range[g] = (loc[gl] if 0 <= gl < loc.size else np.nan) + values[j]
            if ix.grp_shown[g]:
                if best_range[g] > logprob:
                    logprob = best_range[g]
                if g - g0 == tg:
                    wrong = int(gl != pred or ix.rw_eq_target[members[j]] == 0)
        sample_i[:, b] = pred, int(pred == loc.size - 1), wrong
        sample_d[:, b] = logprob, src[ix.nobug_idx[b]]
    return best_rw, best_range, sample_i, sample_d


def order_host(keys, keep, by_confidence: bool, k: int = 0) -> np.ndarray:
    """bl_report_order in NumPy: the indices with keep != 0 as Python's stable sorted(key=-key) orders them (greater key first,
    input order on ties, -inf last, NaN after that) when `by_confidence`, else in input order; the first k when k > 0."""
    keys = np.asarray(keys, dtype=np.float64)
    kept = np.flatnonzero(np.asarray(keep) != 0)
    if by_confidence and kept.size:
        sel = keys[kept]
        nan = np.isnan(sel)
        kept = kept[np.lexsort((np.where(nan, 0.0, -sel), nan))]  # lexsort is stable; last key first: NaNs to the back
    if k > 0:
        kept = kept[:k]
    return kept.astype(np.int32)
