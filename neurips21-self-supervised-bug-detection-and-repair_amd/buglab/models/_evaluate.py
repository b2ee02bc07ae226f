"""The index arrays and the NumPy twin of the evaluation kernel (csrc/bl_evaluate.hip) behind buglab/models/evaluate.py.

What a sample contributes to the evaluation report -- its predicted location, the best rewrite at the predicted and at the true
node, and the verdicts `judge_sample` derives from them (reference buglab/models/evaluate.py:60-140) -- is a segmented reduction
over the model's flat output.  `eval_indices` states it as int32 arrays (in the collate worker, next to `prediction_layout`);
`hip_ops.eval_judge` runs it on the device; `judge_host` runs the same arrays on the host.

Nodes are compared by IDENTITY, as the host compares node ids: every node of a sample is named by its dense id, its index in
np.unique(reference_nodes).  Two nodes of a sequence model that map to one token share a flat index and stay two keys."""
from __future__ import annotations

from typing import Any, Dict, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from buglab.models._report import NO_BUG_NODE, _first_max, location_entries


class EvalIndices(NamedTuple):
    """int32 arrays of one minibatch of B samples for bl_eval_judge (include/buglab_hip.h has the contract)."""

    loc_idx: np.ndarray   # [total_loc] flat index of every location entry, in location-key order (NO_BUG last)
    loc_off: np.ndarray   # [B + 1]
    key_node: np.ndarray  # [total_loc] dense id of the entry's node, -1 for NO_BUG
    rw_idx: np.ndarray    # [total_rw]  flat index of every rewrite, by original rewrite index
    rw_off: np.ndarray    # [B + 1]
    rw_node: np.ndarray   # [total_rw]  dense id of the rewrite's reference node
    tgt_rw: np.ndarray    # [B] target_fix_action_idx, -1 without a bug


def eval_indices(layout, datapoints: Sequence[Any], node_mappings: Optional[Sequence[Dict[int, int]]] = None) -> EvalIndices:
    """`layout`: the minibatch's `PredictionLayout`; `node_mappings`: the sequence models' node -> token maps
    (`mb["node_mappings"]`), None for graph models."""
    loc_idx, all_keys = location_entries(layout, datapoints, node_mappings)
    key_node = np.empty(loc_idx.shape[0], np.int32)
    rw_node = np.empty(layout.rw_idx.shape[0], np.int32)
    tgt_rw = np.full(layout.num_samples, -1, np.int32)
    for b, (point, keys) in enumerate(zip(datapoints, all_keys)):
        nodes, place = np.unique(np.asarray(point["graph"]["reference_nodes"], dtype=np.int64), return_inverse=True)
        lo, hi = int(layout.loc_off[b]), int(layout.loc_off[b + 1])
        assert keys[-1] == NO_BUG_NODE
        key_node[lo:hi - 1] = np.searchsorted(nodes, np.asarray(keys[:-1], dtype=np.int64))  # every key is a reference node
        key_node[hi - 1] = -1
        rw_node[int(layout.rw_off[b]):int(layout.rw_off[b + 1])] = place
        target = point["target_fix_action_idx"]
        if target is not None:
            tgt_rw[b] = int(target)
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    return EvalIndices(i32(loc_idx), i32(layout.loc_off), key_node, i32(layout.rw_idx), i32(layout.rw_off), rw_node, tgt_rw)


def check_assume_buggy(ix: EvalIndices) -> None:
    """What `judge_sample(..., assume_buggy=True)` refuses, before anything is launched: a sample without a bug (its
    assertion), and a sample that has nothing but NO_BUG to choose from (max() of nothing)."""
    assert (ix.tgt_rw >= 0).all(), "assume_buggy: every sample must have a bug (target_fix_action_idx is None)"
    if (np.diff(ix.loc_off) < 2).any():
        raise ValueError("assume_buggy: a sample has no candidate location besides NO_BUG")


def _best_rewrite_at(node: int, nodes: np.ndarray, values: np.ndarray) -> int:
    """The host's loop from -inf that takes a candidate only if it is strictly greater: the lowest index among the maxima at
    `node`; a NaN never wins; -1 ("none") where nothing is above -inf."""
    at = np.flatnonzero((nodes == node) & (values > -np.inf)) if node >= 0 else np.zeros(0, np.int64)
    return int(at[np.argmax(values[at])]) if at.size else -1


def judge_host(src: np.ndarray, ix: EvalIndices, assume_buggy: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """bl_eval_judge in NumPy, in fp64: -> (confidence float64 [B], verdict int32 [4, B] = warned | location_correct |
    repair_given_location (-1 without a bug) | repaired)."""
    if assume_buggy:
        check_assume_buggy(ix)
    src = np.asarray(src, dtype=np.float64)

    def read(idx):  # an index outside src reads as NaN, as on the device
        out = np.full(idx.shape, np.nan)
        ok = (idx >= 0) & (idx < src.shape[0])
        out[ok] = src[idx[ok]]
        return out

    B = ix.tgt_rw.shape[0]
    confidence, verdict = np.empty(B, np.float64), np.empty((4, B), np.int32)
    for b in range(B):
        lo, hi, r0, r1 = int(ix.loc_off[b]), int(ix.loc_off[b + 1]), int(ix.rw_off[b]), int(ix.rw_off[b + 1])
        loc = read(ix.loc_idx[lo:hi - 1 if assume_buggy else hi].astype(np.int64))
        rw, rw_node = read(ix.rw_idx[r0:r1].astype(np.int64)), ix.rw_node[r0:r1]
        target = int(ix.tgt_rw[b])
        has_bug = 0 <= target < r1 - r0
        if loc.size:
            pred = _first_max(loc)
            conf, pred_node = loc[pred], int(ix.key_node[lo + pred])
            if assume_buggy:  # minus the log-sum-exp of what is left, shifted by its greatest value (0 where that is infinite)
                finite = loc[~np.isnan(loc)]
                shift = finite.max() if finite.size and np.isfinite(finite.max()) else 0.0
                with np.errstate(divide="ignore", invalid="ignore"):
                    conf = conf - (shift + np.log(np.sum(np.exp(loc - shift))))
        else:
            conf, pred_node = np.nan, -1
        true_node = int(rw_node[target]) if has_bug else -1
        with np.errstate(invalid="ignore"):
            pred_rw = _best_rewrite_at(pred_node, rw_node, rw)
            true_rw = _best_rewrite_at(true_node, rw_node, rw)
        location_correct = pred_node == true_node
        confidence[b] = conf
        verdict[:, b] = (pred_node >= 0, location_correct, int(true_rw == target) if has_bug else -1,
                         location_correct and pred_rw == (target if has_bug else -1))
    return confidence, verdict
