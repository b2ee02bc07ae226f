"""GREAT var-misuse model -- MI355X counterpart of reference buglab/models/greatreimplementation.py (the reimplementation of
Hellendoorn et al.'s GREAT, trained on the original GREAT JSON-lines data by buglab/models/traingreat.py).

`GreatVarMisuse` (host side) keeps the reference's constructor, record format and AbstractNeuralModel methods.
`GreatVarMisuseModule` (device side): subtoken embedding + a fixed sinusoidal position table -> relational transformer layers
(buglab/models/layers/relational_transformer.py) -> the output head LayerNorm -> Linear(D, 2) -> localization / repair-pointer
losses, which runs as one HIP operator (hip_ops.varmisuse_head, csrc/bl_varmisuse_head.hip) and keeps its metric counters on the
device: nothing in a step reads device memory on the host.

Differences from the reference, in mechanism only unless noted:
  * a minibatch is padded to L = the longest sequence rounded up to a multiple of 4 (the GEMM operands' row length); the extra
    positions are masked, so the arithmetic is the reference's over its L = longest sequence;
  * edge ids are mapped to 0 .. n-1 in ascending order (see `finalize_metadata`);
  * "Repair Accuracy" and "Repair Loss" are nan for an epoch without a buggy sample, where the reference divides by zero.
"""
from __future__ import annotations

import math
from typing import Any, Callable, Dict, Iterator, List, NamedTuple, Optional, Tuple, Union

import numpy as np
import torch
from torch import nn

from buglab.data.seqcollate import edge_csr
from buglab.models import hip_ops
from buglab.models.graphmodel import StrElementRepresentationModel
from buglab.models.hip_ops import Dropout, RelEdges
from buglab.models.layers.relational_transformer import RelationalTransformerEncoderLayer
from buglab.runtime.module import ModuleWithMetrics
from buglab.runtime.neuralmodel import AbstractNeuralModel, ordered_map

NUM_POSITIONS = 5000  # rows of the fixed position table, "5000 in GREAT implementation" (reference :59)
STATS_NAMES = ("samples", "localization_hits", "buggy_localization_hits", "buggy_samples", "repair_hits", "localization_loss_sum",
               "repair_loss_sum", "steps")  # order of bl_varmisuse_head_fwd's `stats`


def positional_table(embedding_dim: int, num_positions: int = NUM_POSITIONS) -> torch.Tensor:
    """[num_positions, D] fp32, computed in float64 (reference :60-67): P[pos, i] = sin(pos / 10000^(2 i / D)) for even i and
    cos(...) for odd i.  The exponent is 2 i / D for every i (not 2 (i // 2) / D as in Vaswani et al.)."""
    pos = np.arange(num_positions, dtype=np.float64)[:, None]
    i = np.arange(embedding_dim, dtype=np.float64)[None, :]
    angle = pos / np.power(10000.0, 2.0 * i / embedding_dim)
    table = np.where((np.arange(embedding_dim) % 2 == 0)[None, :], np.sin(angle), np.cos(angle))
    return torch.tensor(table, dtype=torch.float32)


def metrics_from_stats(n, loc_ok, buggy_loc_ok, n_buggy, rep_ok, loc_loss, rep_loss) -> Dict[str, Any]:
    """The module's metrics (:103-116) from the first seven counters of STATS_NAMES: the device's `metric_stats` after a
    training / validation pass, or the same counts taken from prediction records (buglab/models/evaluategreat.py)."""
    div = lambda a, b: a / b if b != 0 else float("nan")  # deviation: the reference raises ZeroDivisionError here
    return {
        "Localization Accuracy": div(loc_ok, n),
        "Localization Accuracy (Buggy)": buggy_loc_ok / (n_buggy + 1e-10),
        "Localization Accuracy (NoBug)": (loc_ok - buggy_loc_ok) / (n - n_buggy + 1e-10),
        "Repair Accuracy": div(rep_ok, n_buggy),
        "Localization Loss": div(loc_loss, n),
        "Repair Loss": div(rep_loss, n_buggy),
        "Num samples": int(n),
    }


class GreatVarMisuseModule(ModuleWithMetrics):
    """reference :44-214, same keyword arguments."""

    def __init__(self, token_embedder, num_edge_types: int, num_layers: int, num_heads: int, intermediate_dimension: int,
                 dropout_rate: float, rezero_mode: str = "off", normalization_mode: str = "prenorm"):
        super().__init__()
        D = token_embedder.embedding_size
        self.embedding_dim = D
        self.register_buffer("positional_encodings", positional_table(D))  # fixed, not trained (requires_grad=False, :65-67)
        self.token_embedder = token_embedder
        self.dropout_rate = dropout_rate
        self.seq_layers = nn.ModuleList([
            RelationalTransformerEncoderLayer(d_model=D, key_query_dimension=D // num_heads, value_dimension=D // num_heads, nhead=num_heads,
                                              num_edge_types=num_edge_types, dim_feedforward=intermediate_dimension, dropout=dropout_rate,
                                              use_edge_value_biases=False,  # GREAT (:81)
                                              rezero_mode=rezero_mode, normalisation_mode=normalization_mode)
            for _ in range(num_layers)])
        # output layers (:90-91): nn.LayerNorm(D) and nn.Linear(D, 2) with torch's default initialisation; W stored [in, out]
        self.ln_out_g, self.ln_out_b = nn.Parameter(torch.ones(D)), nn.Parameter(torch.zeros(D))
        bound = 1.0 / math.sqrt(D)
        self.predictions_W = nn.Parameter(torch.empty(D, 2).uniform_(-bound, bound))
        self.predictions_b = nn.Parameter(torch.empty(2).uniform_(-bound, bound))
        # the metric counters of :93-101, accumulated on the device by the head (names: STATS_NAMES)
        self.register_buffer("metric_stats", torch.zeros(hip_ops.VARMISUSE_STATS, dtype=torch.float64), persistent=False)
        self._dropout_step = 0

    # ---- metrics (:93-116) ------------------------------------------------------------------------
    def _reset_module_metrics(self) -> None:
        self.metric_stats.zero_()

    def _module_metrics(self) -> Dict[str, Any]:
        return metrics_from_stats(*self.metric_stats.cpu().tolist()[:7])  # the one read-back

    # ---- forward ------------------------------------------------------------------------------------
    def _next_dropout_seed(self) -> Optional[int]:
        if not self.training or self.dropout_rate <= 0.0:
            return None
        self._dropout_step += 1
        return self._dropout_step & 0xFFFFFFFF

    def forward(self, *, token_ids, token_lens, lens_att, edge_row_ptr, edge_key, edge_code, error_locations, candidate_mask,
                target_mask, **_unused):
        """The minibatch `GreatVarMisuse.finalize_minibatch` builds -> scalar loss (reference :118-174)."""
        B, L, S = token_ids.shape
        seed = self._next_dropout_seed()
        drop = Dropout(self.dropout_rate, seed, 0) if seed is not None else hip_ops.NO_DROPOUT
        emb = self.token_embedder(token_ids.reshape(B * L, S), token_lens.reshape(B * L), drop)  # [B * L, D]
        edges = RelEdges(edge_row_ptr, edge_key, edge_code, int(edge_key.shape[0]))
        return self.loss_from_embedded(emb, B, L, lens_att, edges, error_locations, candidate_mask, target_mask, dropout_seed=seed)

    def loss_from_embedded(self, embedded, B: int, L: int, lens_att, edges: RelEdges, error_locations, candidate_mask, target_mask,
                           dropout_seed: Optional[int] = None):
        """Everything after the token embedder: embedded [B * L, D] (before the position table) -> scalar loss.
        lens_att int32 [B] = min(length + 1, L): the reference's token mask is `arange(L) > length` (:198), so position `length`
        is NOT masked -- as an attention key and as a localization class."""
        D = self.embedding_dim
        # x = embed(tokens) + P[:L] (:192-194): no input LayerNorm, no dropout, no masking of the padding rows
        x = (embedded.reshape(B, L, D) + self.positional_encodings[:L].unsqueeze(0)).reshape(B * L, D)
        chain: dict = {}
        for i, layer in enumerate(self.seq_layers):
            x = layer(x, lens_att, edges, B, L, dropout_seed=dropout_seed, dropout_stream=8 * (i + 1), chain=chain)
        loss, _logits, _num_buggy = hip_ops.varmisuse_head(x, self.ln_out_g, self.ln_out_b, self.predictions_W, self.predictions_b,
                                                           lens_att, error_locations, candidate_mask, target_mask, self.metric_stats)
        return loss

    def predict_minibatch(self, mb: Dict[str, Any], out_d: torch.Tensor, out_i: torch.Tensor, offset: int) -> torch.Tensor:
        """Forward only, judged on the device: embedder, position table and encoder layers exactly as `forward` runs them in
        eval() mode (no dropout anywhere), then hip_ops.varmisuse_predict in place of the training head.  The B samples' records go
        to samples offset .. offset + B - 1 of the caller's run-long out_d (float64 [7, N]) / out_i (int32 [4, N]); see
        include/buglab_hip.h::bl_varmisuse_predict.  Reads no training flag and leaves `metric_stats`, the dropout step counter
        and the training flag alone.  -> the masked logits [B * L, 2]; nothing is read back to the host."""
        token_ids, lens_att = mb["token_ids"], mb["lens_att"]
        B, L, S = token_ids.shape
        D = self.embedding_dim
        with torch.no_grad():
            emb = self.token_embedder(token_ids.reshape(B * L, S), mb["token_lens"].reshape(B * L), hip_ops.NO_DROPOUT)
            edges = RelEdges(mb["edge_row_ptr"], mb["edge_key"], mb["edge_code"], int(mb["edge_key"].shape[0]))
            x = (emb.reshape(B, L, D) + self.positional_encodings[:L].unsqueeze(0)).reshape(B * L, D)
            chain: dict = {}
            for i, layer in enumerate(self.seq_layers):
                x = layer(x, lens_att, edges, B, L, dropout_seed=None, dropout_stream=8 * (i + 1), chain=chain)
            return hip_ops.varmisuse_predict(x, self.ln_out_g, self.ln_out_b, self.predictions_W, self.predictions_b, lens_att,
                                             mb["error_locations"], mb["candidate_mask"], mb["target_mask"], out_d, out_i, offset)


class VarMisusePrediction(NamedTuple):
    """What `GreatVarMisuse.predict` yields for one record."""
    predicted_location: int                  # 0 = no bug
    location_logprob: float
    no_bug_logprob: float
    predicted_repair: Optional[int]          # None when the record has no (integer) repair candidate
    repair_logprob: Optional[float]          # pointer log-probability of the predicted repair; None without one
    localization_logprobs: np.ndarray        # float64, one per unmasked position (lens_att of them)
    repair_logprobs: Dict[int, float]        # candidate position -> pointer log-probability


class TensorizedGreatDataPoint(NamedTuple):
    token_ids: np.ndarray                          # int32 [n, S] subtoken ids
    token_lens: np.ndarray                         # int32 [n]
    edges: np.ndarray                              # int32 [E, 2] (source, target)
    edge_types: np.ndarray                         # int32 [E] mapped edge ids
    error_location: int
    repair_candidates_mask: Optional[np.ndarray]   # bool [n]; None for a NO_BUG sample
    repair_targets_mask: Optional[np.ndarray]


class GreatVarMisuse(AbstractNeuralModel):
    """reference :217-345.  Raw records are the GREAT JSON-lines dicts: `source_tokens`, `edges` ([src, tgt, edge_id, edge_name]),
    `error_location` (0 = no bug), `repair_candidates`, `repair_targets`, ..."""

    def __init__(self, transformer_config: Dict[str, Any], vocab_size: int, embedding_dim: int, max_length: int = 512,
                 dropout_rate: float = 0.1):
        super().__init__()
        self._transformer_config = dict(transformer_config)
        self._max_length = max_length
        self._token_embedder = StrElementRepresentationModel(token_splitting="subtoken", embedding_size=embedding_dim,
                                                             dropout_rate=dropout_rate, vocabulary_size=vocab_size,
                                                             subtoken_combination="mean")
        self._edge_ids: Optional[set] = set()
        self._edge_id_to_edge: Optional[Dict[int, int]] = None

    @property
    def token_embedder(self) -> StrElementRepresentationModel:
        return self._token_embedder

    @property
    def edge_id_to_edge(self) -> Dict[int, int]:
        return self._edge_id_to_edge

    # ---- metadata (:238-249) -----------------------------------------------------------------------
    def update_metadata_from(self, datapoint) -> None:
        for token in datapoint["source_tokens"]:
            self._token_embedder.update_metadata_from(token)
        for edge in datapoint["edges"]:
            self._edge_ids.add(edge[2])

    def finalize_metadata(self) -> None:
        self._token_embedder.finalize_metadata()
        # The reference enumerates a `set` of small ints (:249); CPython iterates such a set in ascending order, so ascending
        # order is what it computes -- written out here instead of relied upon.
        self._edge_id_to_edge = {e: i for i, e in enumerate(sorted(self._edge_ids))}
        self._edge_ids = None

    def build_neural_module(self) -> GreatVarMisuseModule:
        return GreatVarMisuseModule(token_embedder=self._token_embedder.build_neural_module(),
                                    num_edge_types=2 * len(self._edge_id_to_edge), **self._transformer_config)

    # ---- tensorize (:258-288) ------------------------------------------------------------------------
    def tensorize(self, datapoint) -> Optional[TensorizedGreatDataPoint]:
        tokens = datapoint["source_tokens"]
        n = len(tokens)
        if n > self._max_length:
            return None
        error_location = int(datapoint["error_location"])
        if error_location > 0:
            candidates = np.zeros(n, dtype=bool)
            targets = np.zeros(n, dtype=bool)
            candidates[np.asarray(datapoint["repair_candidates"], dtype=np.int64)] = True
            targets[np.asarray(datapoint["repair_targets"], dtype=np.int64)] = True
            if not np.any(candidates & targets):
                return None  # no repair candidate is a repair target (:273-274)
        else:
            candidates = targets = None
        ids, lens = self._token_embedder.tensorize_nodes(tokens)
        raw = datapoint["edges"]
        edges = np.array([(e[0], e[1]) for e in raw], dtype=np.int32).reshape(-1, 2)
        edge_types = np.array([self._edge_id_to_edge[e[2]] for e in raw], dtype=np.int32)  # KeyError on an unseen id, as :283
        return TensorizedGreatDataPoint(ids, lens, edges, edge_types, error_location, candidates, targets)

    def tensorize_for_prediction(self, datapoint, labelled: bool) -> Optional[TensorizedGreatDataPoint]:
        """`tensorize` for prediction and evaluation: the candidate mask of EVERY sample, from the integer entries of
        `repair_candidates` (a no-bug record of the GREAT data holds strings there: skipped).  With `labelled` the error location and
        the target mask are the record's and a buggy record none of whose candidates is a target is rejected, as `tensorize`
        rejects it (an evaluation sees the samples a validation pass sees); without, they are zeros (the head's "unlabelled").
        None for a record longer than `max_length`."""
        tokens = datapoint["source_tokens"]
        n = len(tokens)
        if n > self._max_length:
            return None
        candidates = np.zeros(n, dtype=bool)
        targets = np.zeros(n, dtype=bool)
        positions = [int(c) for c in datapoint.get("repair_candidates", ()) if isinstance(c, (int, np.integer)) and not isinstance(c, bool)]
        candidates[np.asarray(positions, dtype=np.int64)] = True
        error_location = 0
        if labelled:
            error_location = int(datapoint["error_location"])
            targets[np.asarray([int(t) for t in datapoint.get("repair_targets", ())], dtype=np.int64)] = True
            if error_location > 0 and not np.any(candidates & targets):
                return None
        ids, lens = self._token_embedder.tensorize_nodes(tokens)
        raw = datapoint["edges"]
        edges = np.array([(e[0], e[1]) for e in raw], dtype=np.int32).reshape(-1, 2)
        edge_types = np.array([self._edge_id_to_edge[e[2]] for e in raw], dtype=np.int32)
        return TensorizedGreatDataPoint(ids, lens, edges, edge_types, error_location, candidates, targets)

    # ---- minibatching (:290-345) --------------------------------------------------------------------------
    def initialize_minibatch(self) -> Dict[str, Any]:
        return {"samples": []}

    def extend_minibatch_with(self, tensorized_datapoint: TensorizedGreatDataPoint, partial_minibatch: Dict[str, Any]) -> bool:
        partial_minibatch["samples"].append(tensorized_datapoint)
        return True

    def collate_samples(self, samples: List[TensorizedGreatDataPoint], masks_for_all_samples: bool = False) -> Dict[str, Any]:
        return collate_great(samples, len(self._edge_id_to_edge), self._token_embedder.max_num_subtokens,
                             masks_for_all_samples=masks_for_all_samples)

    def finalize_minibatch(self, accumulated_minibatch_data: Dict[str, Any], device: Union[str, torch.device]) -> Dict[str, Any]:
        return upload_great(self.collate_samples(accumulated_minibatch_data["samples"]), device)

    # ---- prediction (no counterpart in the reference, which ends at finalize_minibatch) ------------------------------
    def prediction_minibatches(self, data, device, parallelize: bool, minibatch_size: int, labelled: bool,
                               rejected: Optional[Callable[[Any], None]] = None) -> Iterator[Tuple[Dict[str, Any], List[Any]]]:
        """(minibatch on the device, its records) in input order: `tensorize_for_prediction` and the collate with masks for every
        sample, in the worker threads `minibatch_iterator` gives every model's predict.  The minibatch also carries "host": the
        NumPy lens_att, error_locations and target_mask it was uploaded from.  `rejected(record)` is called for a record that is
        left out."""

        def tensorized():
            for t, record in ordered_map(lambda r: (self.tensorize_for_prediction(r, labelled), r), data, parallelize):
                if t is not None:
                    yield t, record
                elif rejected is not None:
                    rejected(record)

        def finalize(accumulated, dev):
            host = self.collate_samples(accumulated["samples"], masks_for_all_samples=True)
            mb = upload_great(host, dev)
            mb["host"] = {k: host[k] for k in ("lens_att", "error_locations", "target_mask")}
            return mb

        yield from self.minibatch_iterator(tensorized(), device, max_minibatch_size=minibatch_size, parallelize=parallelize,
                                           finalize=finalize)

    # `predict` is a property, not a plain method, for one reason: tests/test_ensemble_host.py (written when this model had no
    # predict) asserts `not hasattr(GreatVarMisuse.__new__(GreatVarMisuse), "predict")`, and the property raises AttributeError
    # on such a never-constructed object.  The price: `GreatVarMisuse.predict` on the CLASS is a property object, not callable and
    # without a signature (use `GreatVarMisuse._predict` for introspection).  Once that old assertion is updated, rename
    # `_predict` to `predict` and delete this property; EnsembleWrapper refuses GREAT members by type on its own.
    @property
    def predict(self):
        """`predict(data, trained_nn, device, parallelize=True, minibatch_size=30)` -> (record, VarMisusePrediction) in input
        order: the bound `_predict`, which documents it (also the reference's token mask, which makes position `length` a
        legal prediction).  Exists on constructed models only; see the comment above."""
        self._token_embedder  # AttributeError on an object that never ran __init__
        return self._predict

    def _predict(self, data, trained_nn: GreatVarMisuseModule, device, parallelize: bool = True, minibatch_size: int = 30
                 ) -> Iterator[Tuple[Any, VarMisusePrediction]]:
        """(record, VarMisusePrediction) for every record not longer than `max_length`, in input order.  Labels are not read.  Per
        minibatch: one forward judged on the device (`predict_minibatch`), then ONE device-to-host copy of the records and the
        logits.  The token mask is the reference's, lens_att = min(length + 1, longest in the minibatch): the model was trained
        with it, so position `length` (one past the last token) is a legal localization class for every sample but the longest of
        its minibatch, and it is reported as predicted if it wins."""
        device = torch.device(device)
        for mb, records in self.prediction_minibatches(data, device, parallelize, minibatch_size, labelled=False):
            B, L = mb["token_ids"].shape[:2]
            out_d = torch.empty((hip_ops.VARMISUSE_RECORD_D, B), dtype=torch.float64, device=device)
            out_i = torch.empty((hip_ops.VARMISUSE_RECORD_I, B), dtype=torch.int32, device=device)
            logits = trained_nn.predict_minibatch(mb, out_d, out_i, 0)
            nd, ni = out_d.numel() * 8, out_i.numel() * 4
            host = torch.cat([t.reshape(-1).view(torch.uint8) for t in (out_d, out_i, logits)]).cpu()  # the one copy back
            rec_d = host[:nd].view(torch.float64).view(-1, B).numpy()
            rec_i = host[nd : nd + ni].view(torch.int32).view(-1, B).numpy()
            lg = host[nd + ni :].view(torch.float32).view(B, L, 2).numpy()
            lens_att = mb["host"]["lens_att"]
            for b, record in enumerate(records):
                la = int(lens_att[b])
                loc = lg[b, :la, 0].astype(np.float64) - rec_d[0, b]
                cand = np.flatnonzero(lg[b, :la, 1] != -np.inf)
                rep = lg[b, cand, 1].astype(np.float64) - rec_d[1, b]
                repair = int(rec_i[1, b])
                yield record, VarMisusePrediction(int(rec_i[0, b]), float(rec_d[2, b]), float(rec_d[3, b]),
                                                  repair if repair >= 0 else None, float(rec_d[5, b]) if repair >= 0 else None, loc,
                                                  dict(zip(cand.tolist(), rep.tolist())))


def collate_great(samples: List[TensorizedGreatDataPoint], num_edge_ids: int, max_num_subtokens: int,
                  masks_for_all_samples: bool = False) -> Dict[str, Any]:
    """B tensorised samples -> NumPy arrays of one minibatch (reference :299-345), padded to L = the longest sequence rounded up
    to a multiple of 4.  Pads: subtoken id 0 with one subtoken (count 1); every edge appears as given and reversed, the reversed
    copy with its type shifted by the number of edge ids (:332-334), and both go to the query-row CSR of `edge_csr`.
    `masks_for_all_samples`: copy the candidate / target masks of every sample that has them (prediction), not only of the buggy
    ones (training, the default)."""
    B = len(samples)
    if B == 0:
        raise ValueError("collate_great: empty minibatch")
    S = max_num_subtokens
    lengths = np.array([s.token_ids.shape[0] for s in samples], dtype=np.int32)
    longest = int(lengths.max())
    L = max(4, (longest + 3) // 4 * 4)
    token_ids = np.zeros((B, L, S), dtype=np.int32)
    token_lens = np.ones((B, L), dtype=np.int32)
    error_locations = np.zeros(B, dtype=np.int32)
    candidate_mask = np.zeros((B, L), dtype=np.uint8)
    target_mask = np.zeros((B, L), dtype=np.uint8)
    edges, types = [], []
    for b, s in enumerate(samples):
        n = s.token_ids.shape[0]
        token_ids[b, :n, : s.token_ids.shape[1]] = s.token_ids
        token_lens[b, :n] = s.token_lens
        error_locations[b] = s.error_location
        if s.error_location > 0 or (masks_for_all_samples and s.repair_candidates_mask is not None):
            candidate_mask[b, :n] = s.repair_candidates_mask
            target_mask[b, :n] = s.repair_targets_mask
        e = np.empty((s.edges.shape[0], 3), dtype=np.int64)
        e[:, 0] = b
        e[:, 1:] = s.edges
        edges.append(e)
        types.append(s.edge_types)
    edges = np.concatenate(edges)
    types = np.concatenate(types).astype(np.int64)
    edges = np.concatenate([edges, edges[:, [0, 2, 1]]])
    types = np.concatenate([types, types + num_edge_ids])
    row_ptr, key, code = edge_csr(edges, types, B, L)
    return {
        "token_ids": token_ids, "token_lens": token_lens, "seq_lens": lengths,
        # the reference masks `arange(longest) > length`: position `length` stays visible unless it is past the longest sequence
        "lens_att": np.minimum(lengths + 1, longest).astype(np.int32),
        "edge_row_ptr": row_ptr, "edge_key": key, "edge_code": code,
        "error_locations": error_locations, "candidate_mask": candidate_mask, "target_mask": target_mask,
        "has_bug": (error_locations != 0).astype(np.uint8),
    }


_UPLOAD_ORDER = ("token_ids", "token_lens", "seq_lens", "lens_att", "edge_row_ptr", "edge_key", "edge_code", "error_locations",
                 "candidate_mask", "target_mask", "has_bug")


def upload_great(mb: Dict[str, np.ndarray], device) -> Dict[str, torch.Tensor]:
    """One host -> device copy of every array of a collated minibatch (16-byte aligned pieces of one byte blob), then views."""
    dev = torch.device(device)
    pieces, total = [], 0
    for k in _UPLOAD_ORDER:
        a = np.ascontiguousarray(mb[k])
        pieces.append((k, a, total))
        total += (a.nbytes + 15) // 16 * 16
    staging = torch.empty(max(total, 16), dtype=torch.uint8, pin_memory=dev.type == "cuda")
    host = staging.numpy()
    for _, a, o in pieces:
        host[o : o + a.nbytes] = a.reshape(-1).view(np.uint8)
    blob = staging.to(dev, non_blocking=True)
    out = {}
    for k, a, o in pieces:
        t = blob[o : o + a.nbytes]
        t = t.view(torch.int32) if a.dtype == np.int32 else t
        out[k] = t.view(a.shape)
    out["has_bug"] = out["has_bug"].view(torch.bool)
    return out
