"""Rewrite bookkeeping shared by the BugLab models -- counterpart of reference
buglab/models/basemodel.py (`AbstractBugLabModel`): the rewrite-operator vocabulary (:13-69),
grouping of a sample's candidate rewrites by scout and location into flat index arrays (:80-238)
and un-batching of predicted log-probabilities into per-sample results (:240-346).  Host-side
Python; outputs are consumed by buglab.data.collate."""
from __future__ import annotations

from collections import defaultdict
from contextlib import contextmanager
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from buglab.runtime.vocabulary import Vocabulary

_ARITH = ["+", "-", "*", "/", "**", "//", "%", "@", "<<", ">>", "|", "&", "^"]
OPERATOR_REWRITES = frozenset(
    _ARITH + [op + "=" for op in _ARITH] + ["=", "<", "<=", ">", ">=", "==", "!=", " in ", " not in ", " is ", " is not ",
                                             "0", "1", "2", "-1", "-2", "and", "or", "not ", "", "True", "False"]
)  # reference basemodel.py:13-64 (48 entries; language specific)


class _FlatSelection:
    """Flattened candidates of one scout family (the reference's `to_flat_node_selection`, :157-182)."""

    __slots__ = ("location_node_ids", "payload", "location_groups", "correct_idx", "original_rewrite_idxs")

    def __init__(self):
        self.location_node_ids: List[int] = []
        self.payload: List = []
        self.location_groups: List[int] = []
        self.correct_idx: Optional[int] = None
        self.original_rewrite_idxs: List[int] = []


class AbstractBugLabModel:
    OPERATOR_REWRITES = OPERATOR_REWRITES

    def _init(self):
        self._target_rewrite_ops = Vocabulary.create_vocabulary(
            sorted(self.OPERATOR_REWRITES), max_size=len(self.OPERATOR_REWRITES), count_threshold=0, add_unk=False)
        self._tensorize_only_at_target_location_rewrites = True

    @contextmanager
    def _tensorize_all_location_rewrites(self):
        try:
            self._tensorize_only_at_target_location_rewrites = False
            yield
        finally:
            self._tensorize_only_at_target_location_rewrites = True

    # -------------------------------------------------------------------------------------------
    @property
    def confidence_calibration(self):
        """The `ConfidenceCalibration` fitted by buglab/models/calibrate.py (beyond the reference), or None: `predict` and the
        services' `flat_prediction_output` then report calibrated log-probabilities.  Pickled with the model; a checkpoint
        written before the field existed has none."""
        return getattr(self, "_confidence_calibration", None)

    @confidence_calibration.setter
    def confidence_calibration(self, value) -> None:
        self._confidence_calibration = value

    @property
    def warning_operating_point(self):
        """The `OperatingPoint` fitted by buglab/models/operatingpoint.py (beyond the reference), or None: the confidence at
        which a warning is shown, read by `visualize --at-operating-point` and `evaluate --at-operating-point`.  Pickled with
        the model; a checkpoint written before the field existed has none."""
        return getattr(self, "_warning_operating_point", None)

    @warning_operating_point.setter
    def warning_operating_point(self, value) -> None:
        self._warning_operating_point = value

    @property
    def null_reference(self):
        """The `NullReference` fitted by `python -m buglab.models.fdr fit` (beyond the reference), or None: the sorted NO_BUG
        scores of clean samples that `fdr scan` ranks a scanned sample in.  Pickled with the model; a checkpoint written
        before the field existed has none, and nothing but buglab/models/fdr.py reads it."""
        return getattr(self, "_null_reference", None)

    @null_reference.setter
    def null_reference(self, value) -> None:
        self._null_reference = value

    def _compute_rewrite_data(self, datapoint, candidate_node_idxs: Sequence[int]):
        """Same 16-tuple as reference basemodel.py:80-238.

        During training only rewrites AT THE TARGET LOCATION are kept (:119-121); with
        `_tensorize_all_location_rewrites()` (predict) every location is kept."""
        graph = datapoint["graph"]
        target_idx = datapoint["target_fix_action_idx"]
        target_node = graph["reference_nodes"][target_idx] if target_idx is not None else None

        call_args: Dict[int, List[int]] = defaultdict(list)  # Call node -> its `args` children, in order (:88-98)
        nodes = graph["nodes"]
        from buglab.data.native import NativeGraph

        if isinstance(graph, NativeGraph):
            # native reader: the labelled Child edges are a few entries of an int32 array -- no Python loop over all edges
            for src, tgt in graph.edges.labelled("Child", "args"):
                if nodes[src] == "Call":
                    call_args[src].append(tgt)
        else:
            for edge in graph["edges"].get("Child", ()):
                if len(edge) == 3 and edge[2] == "args" and nodes[edge[0]] == "Call":
                    call_args[edge[0]].append(edge[1])

        # per family: location node -> (payloads, original rewrite ids); insertion-ordered like the reference's dicts
        fam_payload = {k: defaultdict(list) for k in ("text", "var", "swap")}
        fam_orig = {k: defaultdict(list) for k in ("text", "var", "swap")}
        fam_correct: Dict[str, Optional[Tuple[int, int]]] = {"text": None, "var": None, "swap": None}

        for i, (node_idx, (_rw_type, rw_data), (scout, rw_meta)) in enumerate(
                zip(graph["reference_nodes"], datapoint["candidate_rewrites"], datapoint["candidate_rewrite_metadata"])):
            if self._tensorize_only_at_target_location_rewrites and node_idx != target_node:
                continue
            if scout == "VariableMisuseRewriteScout":
                fam, payload = "var", rw_meta
            elif scout == "ArgSwapRewriteScout":
                args = call_args[node_idx]
                fam, payload = "swap", (args[rw_data[0]], args[rw_data[1]])
            else:
                fam, payload = "text", self._target_rewrite_ops.get_id_or_unk(rw_data)
            if target_idx == i:
                fam_correct[fam] = (node_idx, len(fam_payload[fam][node_idx]))
            fam_payload[fam][node_idx].append(payload)
            fam_orig[fam][node_idx].append(i)

        group_of = {int(n): g for g, n in enumerate(candidate_node_idxs)}  # :155

        def flatten(fam: str) -> _FlatSelection:
            out = _FlatSelection()
            correct = fam_correct[fam]
            for loc_node, payloads in fam_payload[fam].items():
                if correct is not None and correct[0] == loc_node:
                    out.correct_idx = len(out.payload) + correct[1]
                out.location_node_ids.extend([loc_node] * len(payloads))
                out.payload.extend(payloads)
                out.location_groups.extend([group_of[int(loc_node)]] * len(payloads))
                out.original_rewrite_idxs.extend(fam_orig[fam][loc_node])
            return out

        text, var, swap = flatten("text"), flatten("var"), flatten("swap")
        return (
            text.location_node_ids, text.payload, text.location_groups, text.correct_idx, text.original_rewrite_idxs,
            var.location_node_ids, var.location_groups, var.payload, var.correct_idx, var.original_rewrite_idxs,
            swap.location_node_ids, swap.payload, swap.correct_idx, swap.location_groups, swap.original_rewrite_idxs,
            group_of,
        )

    # -------------------------------------------------------------------------------------------
    def _finalize_prediction_minibatch(self, accumulated_minibatch_data, device):
        """`finalize_minibatch` for predict: collate, compute the un-batching gather indices on the host (in the collate worker
        of `minibatch_iterator`, off the device's critical path), then the one host->device copy."""
        from buglab.data.collate import to_device

        mb = self.collate_minibatch(accumulated_minibatch_data)
        layout = prediction_layout(mb)
        out = to_device(mb, device)
        out["prediction_layout"] = layout
        if self.confidence_calibration is not None:
            out["confidence_calibration"] = self.confidence_calibration
        return out

    def _iter_per_sample_results(self, mb_data, candidate_location_sample_idx, candidate_location_log_probs,
                                 arg_swap_logprobs, num_samples, original_datapoints, text_repair_logprobs,
                                 varmisuse_logprobs, node_mappings: List[Dict[int, int]] = None):
        """Un-batch a predicted minibatch into (datapoint, {node_idx: logprob, -1: NO_BUG}, [rewrite logprob])
        triples -- reference basemodel.py:240-346.  The four outputs are concatenated and copied to the host once, then
        gathered through `prediction_layout` (precomputed by `_finalize_prediction_minibatch` when present)."""
        to_np = lambda t: t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
        layout = mb_data.get("prediction_layout")
        if layout is None:
            keys = None
            if node_mappings is not None:
                keys = [[node_mappings[b][k] for k in np.unique(original_datapoints[b]["graph"]["reference_nodes"])]
                        for b in range(num_samples)]
            layout = prediction_layout(mb_data, to_np(candidate_location_sample_idx), keys)
        parts = (candidate_location_log_probs, text_repair_logprobs, varmisuse_logprobs, arg_swap_logprobs)
        if all(hasattr(t, "detach") for t in parts):
            import torch

            flat = torch.cat([t.detach().reshape(-1).float() for t in parts])
            if mb_data.get("confidence_calibration") is not None:
                from buglab.models._calibrate import apply_to_flat

                apply_to_flat(mb_data["confidence_calibration"], flat, mb_data)
            flat = flat.cpu().numpy()
        else:
            flat = np.concatenate([to_np(t).reshape(-1).astype(np.float32) for t in parts])
            assert mb_data.get("confidence_calibration") is None, "calibrated models predict from tensors"
        assert flat.shape[0] == layout.flat_size
        loc_all, rw_all = flat[layout.loc_idx].tolist(), flat[layout.rw_idx].tolist()
        assert layout.num_samples == num_samples
        for b in range(num_samples):
            point = original_datapoints[b]
            ref_nodes = point["graph"]["reference_nodes"]
            cand_nodes = np.unique(ref_nodes).tolist()
            lo, hi = int(layout.loc_off[b]), int(layout.loc_off[b + 1])
            dist = loc_all[lo:hi]
            assert len(dist) == len(cand_nodes) + 1
            rewrite_probs = rw_all[int(layout.rw_off[b]):int(layout.rw_off[b + 1])]
            assert len(rewrite_probs) == len(point["candidate_rewrites"])
            if node_mappings is None:
                location_logprobs = dict(zip(cand_nodes, dist))
            else:  # :320-335 (sequence models map graph nodes to tokens): the reference's key order, token by token
                value = dict(zip(cand_nodes, dist))
                in_refs = set(cand_nodes)
                reverse = defaultdict(list)
                for old, new in node_mappings[b].items():
                    if old in in_refs:
                        reverse[new].append(old)
                location_logprobs = {}
                for n in dict.fromkeys(node_mappings[b][k] for k in cand_nodes):
                    for node in reverse[n]:
                        location_logprobs[node] = value[node]
            location_logprobs[-1] = dist[-1]
            yield point, location_logprobs, rewrite_probs


class PredictionLayout(NamedTuple):
    """Where each per-sample prediction value sits in a model's flat output `[loc | text | var | swap]` (the concatenation of
    `compute_localization_logprobs`'s log-probabilities and `_compute_repair_logprobs`' text / var-misuse / arg-swap
    log-probabilities).  Canonical order per sample b:
      locations  loc_idx[loc_off[b] : loc_off[b + 1]]  -- np.unique(reference_nodes) ascending, then NO_BUG;
      rewrites   rw_idx[rw_off[b] : rw_off[b + 1]]     -- by original candidate-rewrite index.
    All int32; every index < flat_size."""

    loc_idx: np.ndarray
    loc_off: np.ndarray
    rw_idx: np.ndarray
    rw_off: np.ndarray
    flat_size: int
    num_samples: int


def prediction_layout(mb, candidate_location_sample_idx=None, location_keys: Optional[Sequence[Sequence]] = None
                      ) -> PredictionLayout:
    """Gather indices of `_iter_per_sample_results` (reference basemodel.py:240-346) from a collated minibatch (NumPy, or
    tensors on the CPU), so that un-batching is one gather.  Rules reproduced exactly:
      * the location entries of sample b are those with sample id b, in flat order: the candidates, NO_BUG last;
      * a family's logprobs of sample b are its entries ordered by location group (stable), and the k-th of them belongs to
        the k-th original rewrite index of that family (text, then var-misuse, then arg-swap);
      * location keys (sequence models: the token a candidate node maps to; `node_mappings` branch, :320-335): candidates that
        share a key all take the value of the LAST flat entry with that key (the reference builds {token: logprob} first).
    `candidate_location_sample_idx`: default cat(candidate -> sample ids, arange(B)), what the localization head returns.
    `location_keys`: per sample, one key per unique reference node; default: none for graph minibatches, the candidates' token
    positions for sequence minibatches (`collate_sequences`, which carry `node_mappings`)."""
    as_np = lambda a: a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    gd = mb["graph_data"]
    B = int(gd["num_graphs"])
    cand = as_np(gd["reference_node_ids"]["candidate_nodes"]).astype(np.int64)
    if candidate_location_sample_idx is None:
        candidate_location_sample_idx = np.concatenate(
            [as_np(gd["reference_node_graph_idx"]["candidate_nodes"]).astype(np.int64), np.arange(B, dtype=np.int64)])
    ids = np.asarray(candidate_location_sample_idx, dtype=np.int64).reshape(-1)
    n_loc = np.bincount(ids, minlength=B)[:B]
    loc_off = np.zeros(B + 1, dtype=np.int64)
    np.cumsum(n_loc, out=loc_off[1:])
    loc_order = np.argsort(ids, kind="stable")  # sample b's entries, in flat order: loc_order[loc_off[b]:loc_off[b + 1]]
    if location_keys is None and mb.get("node_mappings") is not None:
        cand_ptr = as_np(gd["candidate_ptr"]).astype(np.int64)
        location_keys = [cand[cand_ptr[b]:cand_ptr[b + 1]] for b in range(B)]
    loc_idx = loc_order.copy()
    if location_keys is not None:
        for b in range(B):
            keys = [int(k) for k in location_keys[b]]
            assert len(keys) + 1 == n_loc[b]
            last = {k: j for j, k in enumerate(keys)}
            loc_idx[loc_off[b]:loc_off[b] + len(keys)] = loc_order[loc_off[b] + np.asarray([last[k] for k in keys], dtype=np.int64)]

    fams = (("rewrite_to_location_group", "text_rewrite_original_idxs"),
            ("candidate_symbol_to_location_group", "candidate_rewrite_original_idxs"),
            ("swapped_pair_to_call_location_group", "pair_rewrite_original_idx"))
    sizes = [int(as_np(mb[g]).shape[0]) for g, _ in fams]
    n_rw = np.array([sum(len(mb[o][b]) for _, o in fams) for b in range(B)], dtype=np.int64)
    rw_off = np.zeros(B + 1, dtype=np.int64)
    np.cumsum(n_rw, out=rw_off[1:])
    rw_idx = np.full(int(rw_off[-1]), -1, dtype=np.int64)
    base = ids.shape[0]
    for (g, o), size in zip(fams, sizes):
        order = np.argsort(as_np(mb[g]).astype(np.int64), kind="stable") + base
        pos = 0
        for b in range(B):
            orig = np.asarray(mb[o][b], dtype=np.int64)
            if orig.size:
                assert orig.min() >= 0 and orig.max() < n_rw[b] and (rw_idx[rw_off[b] + orig] == -1).all()
                rw_idx[rw_off[b] + orig] = order[pos:pos + orig.size]
            pos += orig.size
        assert pos == size
        base += size
    assert (rw_idx >= 0).all()
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    return PredictionLayout(i32(loc_idx), i32(loc_off), i32(rw_idx), i32(rw_off), int(base), B)
