"""Ensembles of trained BugLab detectors -- counterpart of reference buglab/models/ensemble/wrapper.py.

`EnsembleWrapper(models, kind)` is the host-side model and `EnsembleModuleWrapper(nns)` the device module; a pickled pair
restores through `restore_model` and predicts like a single model: `predict(data, nn, device, parallelize)` yields
`(datapoint, {node: logprob, -1: NO_BUG}, [rewrite logprob])` triples.

The reference calls every member's `predict` on one-sample lists and combines Python dicts with np.logaddexp
(:33-89).  Here a minibatch is built once for all members, each member runs its own HIP forward on it, and the members'
outputs are combined on the device by one kernel (hip_ops.ensemble_combine, csrc/bl_ensemble.hip) in fp64, then copied to
the host once.  Where the members' values sit is decided by `prediction_layout`, the rule every single model un-batches with.

Semantics kept (:33-89): `avg` folds the present members in member order, r = a_0 + w, r = logaddexp(r, a_m + w),
w = -log(M'); `consensus` is `avg` when every present member's arg-max location is the same node, else every location -inf,
NO_BUG 0 and the first present member's rewrites.  A member whose `tensorize` rejects a sample drops out of that sample (a
warning is logged); a sample no member accepts is skipped.

Where this can differ from the reference: the arg-max of a member under `consensus` is the FIRST maximum in the canonical
order (nodes ascending, NO_BUG last), which is the reference's dict order for graph members.  A sequence member's own dict is
ordered token by token (basemodel.py:320-335), so when EXACT ties between different nodes decide a sequence member's arg-max,
the reference may pick another of the tied nodes than this port.  The returned location dicts are in the canonical order.

Beyond the reference: a third kind, `weighted`, carries fitted per-member weights and location temperatures
(`EnsembleWeights`, buglab/models/ensemble/_weights.py has the arithmetic, fit.py the fit) and is combined by
hip_ops.ensemble_combine_weighted (csrc/bl_ensemble_fit.hip).  With the identity weights it is `avg`.
"""
from __future__ import annotations

import logging
from collections import deque
from concurrent.futures import ThreadPoolExecutor
from contextlib import ExitStack
from typing import Any, Dict, Iterator, List, Literal, NamedTuple, Optional, Tuple

import numpy as np
import torch
from torch import nn

from buglab.data.collate import to_device
from buglab.models import hip_ops
from buglab.models.basemodel import PredictionLayout, prediction_layout
from buglab.models.ensemble._weights import EnsembleWeights
from buglab.runtime.module import ModuleWithMetrics
from buglab.runtime.neuralmodel import COLLATE_WORKERS, ordered_map

LOGGER = logging.getLogger(__name__)
MAX_MINIBATCH_SIZE = 50  # samples per minibatch, as the members' own predict


def _member_view(datapoint):
    g = datapoint["graph"]
    if not isinstance(g, dict):  # the native reader's graphs are read-only arrays
        return datapoint
    return dict(datapoint, graph=dict(g, nodes=list(g["nodes"]), edges=dict(g["edges"])))


class EnsembleModuleWrapper(ModuleWithMetrics):
    """The members' modules in an nn.ModuleList, so that `.to(device)` / `.eval()` reach every member (the reference keeps a
    plain list)."""

    def __init__(self, nns):
        super().__init__()
        self._members = nn.ModuleList(nns)

    @property
    def nns(self) -> Iterator[ModuleWithMetrics]:
        yield from self._members


class _EnsembleMinibatch(NamedTuple):
    members: List[Optional[Dict[str, Any]]]  # per member: its minibatch on the device, None when it has no sample here
    index: Optional[torch.Tensor]            # int32 device blob: [loc_idx (M x total_loc) | rw_idx (M x total_rw) | loc_off | rw_off]
    sizes: Tuple[int, int, int, int]         # (M, total_loc, total_rw, B)
    flat_sizes: List[int]                    # per present member: length of its flat output [loc | text | var | swap]
    loc_off: np.ndarray
    rw_off: np.ndarray
    originals: List[Any]


class EnsembleWrapper:
    def __init__(self, models: List[Any], kind: Literal["avg", "consensus", "weighted"], weights: Optional[EnsembleWeights] = None):
        models = list(models)
        if not models:
            raise ValueError("An ensemble needs at least one member.")
        if not all(hasattr(m, "predict") for m in models):
            raise ValueError("One of the models doesn't have a predict function.")  # reference :26 (an assert there)
        from buglab.models.greatreimplementation import GreatVarMisuse

        if any(isinstance(m, GreatVarMisuse) for m in models):  # its predict yields a VarMisusePrediction per record
            raise ValueError("The GREAT var-misuse model's predict does not yield the location / rewrite log-probabilities an "
                             "ensemble combines.")
        if kind not in ("avg", "consensus", "weighted"):
            raise ValueError(f"Unrecognized ensemble kind `{kind}`: expected `avg`, `consensus` or `weighted`.")
        if weights is not None and kind != "weighted":
            raise ValueError(f"Ensemble weights belong to the `weighted` kind, not to `{kind}`.")
        if len(models) > hip_ops.ENSEMBLE_MAX_MEMBERS:
            raise ValueError(f"At most {hip_ops.ENSEMBLE_MAX_MEMBERS} ensemble members are supported (got {len(models)}).")
        self._models = models
        self._kind = kind
        self._weights: Optional[EnsembleWeights] = None
        if kind == "weighted":
            self.ensemble_weights = weights if weights is not None else EnsembleWeights.identity(len(models))

    @property
    def kind(self) -> str:
        return self._kind

    @property
    def ensemble_weights(self) -> Optional[EnsembleWeights]:
        """The fitted weights of a `weighted` ensemble; None for the other kinds (and for a file written before there were any)."""
        return getattr(self, "_weights", None)

    @ensemble_weights.setter
    def ensemble_weights(self, weights: EnsembleWeights) -> None:
        if self._kind != "weighted":
            raise ValueError(f"Ensemble weights belong to the `weighted` kind, not to `{self._kind}`.")
        M = len(self._models)
        if not all(len(p) == M for p in (weights.theta, weights.beta, weights.phi)):
            raise ValueError(f"Ensemble weights for {len(weights.theta)} members do not fit an ensemble of {M}.")
        self._weights = weights

    @property
    def models(self) -> List[Any]:
        return list(self._models)

    # ---- host side: tensorise, group, collate -------------------------------------------------------------------------
    def _tensorize_all(self, datapoint):
        """Every member's `tensorize` of the sample, each on its own shallow view: a graph member adds subtoken nodes and
        `HasSubtoken` edges to the graph in place (representations/data.py::add_open_vocab_nodes_and_edges), which would change
        what the next member sees -- a sequence member's token projection then fails.  Each member sees what its own
        `predict` would see."""
        return [m.tensorize(_member_view(datapoint)) for m in self._models], datapoint

    def _gather(self, tensorized) -> Iterator[Tuple[List[Dict[str, Any]], List[List[int]], List[Any]]]:
        """Groups samples until a member's `extend_minibatch_with` says stop or MAX_MINIBATCH_SIZE samples are in.
        -> (per-member accumulated minibatches, per sample the members' local sample index or -1, original datapoints)."""
        M = len(self._models)

        def fresh():
            return [m.initialize_minibatch() for m in self._models], [0] * M, [], []

        accs, counts, slots, originals = fresh()
        for ts, datapoint in tensorized:
            present = [t is not None for t in ts]
            if not all(present):
                LOGGER.warning("One of the ensemble members did not return a prediction: %s", [int(p) for p in present])
                if not any(present):
                    continue
            keep, slot = True, []
            for m, t in enumerate(ts):
                if t is None:
                    slot.append(-1)
                    continue
                slot.append(counts[m])
                counts[m] += 1
                keep = self._models[m].extend_minibatch_with(t, accs[m]) and keep
            slots.append(slot)
            originals.append(datapoint)
            if not keep or len(originals) >= MAX_MINIBATCH_SIZE:
                yield accs, slots, originals
                accs, counts, slots, originals = fresh()
        if originals:
            yield accs, slots, originals

    def _finalize(self, batch, device) -> _EnsembleMinibatch:
        """Collation, the members' un-batching layouts and the ensemble's gather indices (host, NumPy; runs in a collate
        worker), then one host->device copy per member minibatch and one for the indices."""
        accs, slots, originals = batch
        M, B = len(self._models), len(originals)
        member_mbs: List[Optional[Dict[str, Any]]] = [None] * M
        layouts: List[Optional[PredictionLayout]] = [None] * M
        for m, model in enumerate(self._models):
            if any(s[m] >= 0 for s in slots):
                mb = model.collate_minibatch(accs[m])
                layouts[m] = prediction_layout(mb)
                member_mbs[m] = to_device(mb, device)
        # canonical per-sample sizes, from any member that predicts the sample (all members agree: same datapoint)
        n_loc, n_rw = np.zeros(B, np.int64), np.zeros(B, np.int64)
        for b, slot in enumerate(slots):
            m = next(i for i, k in enumerate(slot) if k >= 0)
            lay, k = layouts[m], slot[m]
            n_loc[b], n_rw[b] = lay.loc_off[k + 1] - lay.loc_off[k], lay.rw_off[k + 1] - lay.rw_off[k]
        loc_off, rw_off = np.zeros(B + 1, np.int64), np.zeros(B + 1, np.int64)
        np.cumsum(n_loc, out=loc_off[1:])
        np.cumsum(n_rw, out=rw_off[1:])
        total_loc, total_rw = int(loc_off[-1]), int(rw_off[-1])
        loc_idx = np.full((M, total_loc), -1, np.int64)
        rw_idx = np.full((M, total_rw), -1, np.int64)
        base, flat_sizes = 0, []
        for m in range(M):
            lay = layouts[m]
            if lay is None:
                continue
            for b, slot in enumerate(slots):
                k = slot[m]
                if k < 0:
                    continue
                src_loc = lay.loc_idx[lay.loc_off[k]:lay.loc_off[k + 1]]
                src_rw = lay.rw_idx[lay.rw_off[k]:lay.rw_off[k + 1]]
                assert src_loc.shape[0] == n_loc[b] and src_rw.shape[0] == n_rw[b], "ensemble members disagree on a sample's layout"
                loc_idx[m, loc_off[b]:loc_off[b + 1]] = base + src_loc
                rw_idx[m, rw_off[b]:rw_off[b + 1]] = base + src_rw
            base += lay.flat_size
            flat_sizes.append(lay.flat_size)
        blob = np.concatenate([loc_idx.reshape(-1), rw_idx.reshape(-1), loc_off, rw_off]).astype(np.int32)
        dev = torch.device(device)
        staging = torch.empty(blob.shape[0], dtype=torch.int32, pin_memory=dev.type == "cuda")
        np.copyto(staging.numpy(), blob)
        index = staging.to(dev, non_blocking=True)
        return _EnsembleMinibatch(member_mbs, index, (M, total_loc, total_rw, B), flat_sizes, loc_off, rw_off, originals)

    def _minibatches(self, tensorized, device, parallelize: bool) -> Iterator[_EnsembleMinibatch]:
        if not parallelize:
            for batch in self._gather(tensorized):
                yield self._finalize(batch, device)
            return
        with ThreadPoolExecutor(max_workers=COLLATE_WORKERS) as pool:
            pending: "deque" = deque()
            for batch in self._gather(tensorized):
                pending.append(pool.submit(self._finalize, batch, device))
                if len(pending) > COLLATE_WORKERS:
                    yield pending.popleft().result()
            while pending:
                yield pending.popleft().result()

    # ---- device side --------------------------------------------------------------------------------------------------
    @staticmethod
    def _member_flat_output(trained_nn, mb_data) -> torch.Tensor:
        """The member's own predict forward (gnn.py / seqmodel.py `predict`) -> its flat output [loc | text | var | swap]."""
        ids, loc_lp, enc_out, _ = trained_nn.compute_localization_logprobs(mb_data["graph_data"])
        swap_lp, text_lp, var_lp, _ = trained_nn._compute_repair_logprobs(
            enc_out, mb_data["target_rewrites"], mb_data["rewrite_to_location_group"],
            mb_data["candidate_symbol_to_location_group"], mb_data["swapped_pair_to_call_location_group"],
            mb_data["repair_group_ptr"], mb_data["repair_group_items"])
        return torch.cat([t.reshape(-1) for t in (loc_lp, text_lp, var_lp, swap_lp)])

    def _predict_minibatch(self, emb: _EnsembleMinibatch, nns) -> Iterator[Tuple[Any, Dict[int, float], List[float]]]:
        flats = [self._member_flat_output(nn_, mb) for nn_, mb in zip(nns, emb.members) if mb is not None]
        assert [int(f.shape[0]) for f in flats] == emb.flat_sizes
        src = torch.cat(flats) if len(flats) > 1 else flats[0]
        M, total_loc, total_rw, B = emb.sizes
        a, c = M * total_loc, M * total_loc + M * total_rw
        ix = emb.index
        gather = (src.contiguous(), ix[:a].view(M, total_loc), ix[c:c + B + 1], ix[a:c].view(M, total_rw), ix[c + B + 1:])
        if self._kind == "weighted":
            w = self.ensemble_weights
            out = hip_ops.ensemble_combine_weighted(*gather, w.theta, w.beta, w.phi)
        else:
            out = hip_ops.ensemble_combine(*gather, self._kind)
        values = out.cpu().numpy()  # the one device->host copy of the minibatch
        loc_all, rw_all = values[:total_loc].tolist(), values[total_loc:].tolist()
        for b, point in enumerate(emb.originals):
            dist = loc_all[emb.loc_off[b]:emb.loc_off[b + 1]]
            nodes = np.unique(point["graph"]["reference_nodes"]).tolist()
            assert len(nodes) + 1 == len(dist)
            location_logprobs = dict(zip(nodes, dist))
            location_logprobs[-1] = dist[-1]
            yield point, location_logprobs, rw_all[emb.rw_off[b]:emb.rw_off[b + 1]]

    def predict(self, data, trained_nn: EnsembleModuleWrapper, device, parallelize: bool
                ) -> Iterator[Tuple[Any, Dict[int, float], List[float]]]:
        """reference :33-82: the same triples, one minibatch of up to MAX_MINIBATCH_SIZE samples at a time for all members."""
        nns = list(trained_nn.nns)
        if len(nns) != len(self._models):
            raise ValueError(f"{len(self._models)} ensemble members but {len(nns)} modules")
        for n in nns:
            n.eval()
        if not getattr(self, "_calibration_notice_given", False) and any(
                getattr(m, "confidence_calibration", None) is not None for m in self._models):
            self._calibration_notice_given = True  # once per wrapper
            if self._kind == "weighted":
                LOGGER.info("Ensemble members carry a confidence calibration; the ensemble combines their uncalibrated values, and its "
                            "fitted per-member temperatures take the calibration's place.")
            else:
                LOGGER.info("Ensemble members carry a confidence calibration; the ensemble combines their uncalibrated values.")
        with torch.no_grad(), ExitStack() as stack:
            for m in self._models:
                stack.enter_context(m._tensorize_all_location_rewrites())
            tensorized = ordered_map(self._tensorize_all, data, parallelize)
            for emb in self._minibatches(tensorized, device, parallelize):
                yield from self._predict_minibatch(emb, nns)
