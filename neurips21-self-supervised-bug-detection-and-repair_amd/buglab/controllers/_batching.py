"""What the two services share: the minibatches of a model's own `predict` with the services' gather indices added in the
collate worker, the model's flat output, and input-order bookkeeping."""
from __future__ import annotations

import threading
from collections import deque
from typing import Any, Callable, Dict, Iterable, Iterator, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from buglab.models.basemodel import PredictionLayout
from buglab.runtime.neuralmodel import ordered_map

MAX_MINIBATCH_SIZE = 50  # samples per minibatch, as the models' own predict


class SelfSupIndices(NamedTuple):
    """Indices into a model's flat output [loc | text | var | swap], int32, from `prediction_layout` and the datapoints:
      rw_loc_idx [total_rw]  per rewrite (layout order: sample by sample, by original rewrite index), the location entry of its
                             reference node -- what `location_logprobs[reference_nodes[i]]` reads;
      nobug_idx  [B]         the sample's NO_BUG location entry (`location_logprobs[-1]`);
      tgt_loc    [B]         the ground node's location entry, NO_BUG's when `target_fix_action_idx` is None;
      tgt_rw     [B]         the target rewrite's entry, -1 when `target_fix_action_idx` is None.
    Sequence models need nothing extra: `prediction_layout` has already resolved their location keys."""

    rw_loc_idx: np.ndarray
    nobug_idx: np.ndarray
    tgt_loc: np.ndarray
    tgt_rw: np.ndarray


def selfsup_indices(layout: PredictionLayout, datapoints: Sequence[Any]) -> SelfSupIndices:
    B = layout.num_samples
    assert len(datapoints) == B
    rw_loc = np.empty(int(layout.rw_off[-1]), np.int32)
    nobug, tgt_loc, tgt_rw = np.empty(B, np.int32), np.empty(B, np.int32), np.full(B, -1, np.int32)
    for b, point in enumerate(datapoints):
        loc = layout.loc_idx[layout.loc_off[b]:layout.loc_off[b + 1]]
        r0, r1 = int(layout.rw_off[b]), int(layout.rw_off[b + 1])
        # a reference node's place in np.unique(reference_nodes): the canonical order of the location entries
        nodes, place = np.unique(np.asarray(point["graph"]["reference_nodes"], dtype=np.int64), return_inverse=True)
        assert loc.shape[0] == nodes.shape[0] + 1 and place.shape[0] == r1 - r0
        rw_loc[r0:r1] = loc[place]
        nobug[b] = loc[-1]
        target = point["target_fix_action_idx"]
        if target is None:
            tgt_loc[b] = loc[-1]
        else:
            tgt_loc[b] = loc[place[target]]
            tgt_rw[b] = layout.rw_idx[r0 + int(target)]
    return SelfSupIndices(rw_loc, nobug, tgt_loc, tgt_rw)


def to_device_i32(arrays: Sequence[np.ndarray], device) -> List[torch.Tensor]:
    """Several int32 arrays -> device tensors through ONE pinned staging buffer and one (non-blocking) copy."""
    sizes = [int(a.shape[0]) for a in arrays]
    dev = torch.device(device)
    staging = torch.empty(sum(sizes), dtype=torch.int32, pin_memory=dev.type == "cuda")
    if sum(sizes):
        np.concatenate([np.asarray(a, np.int32) for a in arrays], out=staging.numpy())
    blob = staging.to(dev, non_blocking=True)
    out, pos = [], 0
    for n in sizes:
        out.append(blob[pos:pos + n])
        pos += n
    return out


def require_single_model(model, what: str) -> None:
    from buglab.models.ensemble.wrapper import EnsembleWrapper

    if isinstance(model, EnsembleWrapper):
        raise TypeError(f"{what} runs on a single detector / selector model; ensembles (EnsembleWrapper) are not supported here.")
    for attr in ("tensorize", "minibatch_iterator", "_finalize_prediction_minibatch", "_tensorize_all_location_rewrites"):
        if not hasattr(model, attr):
            raise TypeError(f"{what}: {type(model).__name__} has no `{attr}`; expected one of the registry's BugLab models.")


def prediction_minibatches(model, tagged: Iterable[Tuple[Any, Any]], device, parallelize: bool,
                           extend: Callable[[PredictionLayout, List[Any], Any], Dict[str, Any]],
                           rejected: Callable[[Any], None], extend_sees_minibatch: bool = False
                           ) -> Iterator[Tuple[Dict[str, Any], List[Any]]]:
    """The minibatches `model.predict` would form from the datapoints of `tagged` = (datapoint, tag) pairs (same
    `minibatch_iterator`, same `_finalize_prediction_minibatch`, 50 samples at most), as (minibatch on the device, [tag]).
    `extend(layout, datapoints, device)` runs in the collate worker, after the layout; its result is the minibatch's
    "selfsup" entry (with `extend_sees_minibatch` it is called as `extend(layout, datapoints, device, minibatch)`: the
    sequence models' minibatch carries their node -> token maps).  `rejected(tag)` is called (from the tensorising side, in input order) for a datapoint `tensorize`
    rejects.  The tags of a minibatch are in the order of its samples (`minibatch_iterator` appends a sample and its tag
    together), which is also the order `extend` sees the datapoints in: `evaluate_on_device(..., positions_out=)` relies on it.
    Call under `torch.no_grad()` and `model._tensorize_all_location_rewrites()`."""
    side: Dict[int, Any] = {}  # id(tensorised sample) -> (the sample: keeps the id unique, its datapoint)

    def tensorized():
        for t, (point, tag) in ordered_map(lambda x: (model.tensorize(x[0]), x), tagged, parallelize):
            if t is None:
                rejected(tag)
                continue
            side[id(t)] = (t, point)
            yield t, tag

    def finalize(accumulated, dev):
        points = [side.pop(id(s))[1] for s in accumulated["samples"]]
        out = model._finalize_prediction_minibatch(accumulated, dev)
        out["selfsup"] = (extend(out["prediction_layout"], points, dev, out) if extend_sees_minibatch
                          else extend(out["prediction_layout"], points, dev))
        return out

    yield from model.minibatch_iterator(tensorized(), device, max_minibatch_size=MAX_MINIBATCH_SIZE, parallelize=parallelize,
                                        finalize=finalize)


def flat_prediction_output_and_encoding(trained_nn, mb_data) -> Tuple[torch.Tensor, Any]:
    """The forward of the model's own `predict` (gnn.py / seqmodel.py) -> (its flat fp32 output [loc | text | var | swap], left
    on the device and calibrated there (hip_ops.conf_apply) when the model carries a `confidence_calibration`; the encoder
    output both heads read, for a service that needs the head input as well: `trained_nn._head_inputs`)."""
    _, loc_lp, enc_out, _ = trained_nn.compute_localization_logprobs(mb_data["graph_data"])
    swap_lp, text_lp, var_lp, _ = trained_nn._compute_repair_logprobs(
        enc_out, mb_data["target_rewrites"], mb_data["rewrite_to_location_group"], mb_data["candidate_symbol_to_location_group"],
        mb_data["swapped_pair_to_call_location_group"], mb_data["repair_group_ptr"], mb_data["repair_group_items"])
    flat = torch.cat([t.detach().reshape(-1).float() for t in (loc_lp, text_lp, var_lp, swap_lp)])
    assert flat.shape[0] == mb_data["prediction_layout"].flat_size
    if mb_data.get("confidence_calibration") is not None:  # the model's own, put there by `_finalize_prediction_minibatch`
        from buglab.models._calibrate import apply_to_flat

        apply_to_flat(mb_data["confidence_calibration"], flat, mb_data)
    return flat, enc_out


def flat_prediction_output(trained_nn, mb_data) -> torch.Tensor:
    """The flat output of `flat_prediction_output_and_encoding` alone."""
    return flat_prediction_output_and_encoding(trained_nn, mb_data)[0]


SAMPLES = -1  # the sample axis in the shape of a `RunColumns` column


class RunColumns:
    """The run-long results of a scan tool: named columns, all views of ONE device allocation, so that a run ends with one
    copy back.  `spec` = ordered (name, "float64" | "float32" | "int32", shape) with exactly one SAMPLES axis in each shape:
    (SAMPLES,), (SAMPLES, k), (2, SAMPLES).  Every column starts 8-byte aligned and is contiguous at full capacity, whatever the
    capacity and the other sizes are.  `reserve(B)` makes room for the next minibatch and gives the sample offset its kernel
    writes at; read the views (`cols[name]`) after it, because it may have moved them."""

    def __init__(self, device, capacity: int, spec: Sequence[Tuple[str, str, Tuple[int, ...]]]):
        self.device, self.capacity, self.n = torch.device(device), max(int(capacity), 1), 0
        self._spec = [(name, getattr(torch, dtype), tuple(shape)) for name, dtype, shape in spec]
        assert all(shape.count(SAMPLES) == 1 and dtype in (torch.float64, torch.float32, torch.int32) for _, dtype, shape in self._spec)
        self._blob, self._cols = self._views(self.capacity)

    def _views(self, capacity: int, blob: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
        """(the allocation, name -> view of it) at `capacity`; without `blob` a new one is allocated"""
        shapes = [tuple(capacity if s == SAMPLES else s for s in shape) for _, _, shape in self._spec]
        cells = [int(np.prod(shape)) for shape in shapes]
        doubles = [c if dtype == torch.float64 else (c + 1) // 2 for c, (_, dtype, _) in zip(cells, self._spec)]  # odd 4-byte cells: padded
        if blob is None:
            blob = torch.empty(sum(doubles), dtype=torch.float64, device=self.device)
        out, pos = {}, 0
        for (name, dtype, _), shape, c, d in zip(self._spec, shapes, cells, doubles):
            out[name] = blob[pos:pos + d].view(dtype)[:c].view(shape)
            pos += d
        return blob, out

    def __getitem__(self, name: str) -> torch.Tensor:
        return self._cols[name]

    def _trimmed(self, cols: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        return {name: cols[name].narrow(shape.index(SAMPLES), 0, self.n) for name, _, shape in self._spec}

    def reserve(self, B: int) -> int:
        """Room for B more samples -> their offset (the count before).  A stream of unknown length: double, on the device --
        one new allocation, every column's samples so far copied along its own sample axis, no synchronisation."""
        n = self.n
        if n + B > self.capacity:
            old = self._trimmed(self._cols)
            self.capacity = max(2 * self.capacity, n + B)
            self._blob, self._cols = self._views(self.capacity)
            for name, t in self._trimmed(self._cols).items():
                t.copy_(old[name])
        self.n = n + B
        return n

    def device_columns(self) -> Dict[str, torch.Tensor]:
        """The columns trimmed to the samples reserved so far, still on the device."""
        return self._trimmed(self._cols)

    def to_host(self) -> Dict[str, np.ndarray]:
        """The trimmed columns as arrays: the one copy (and the one synchronisation) of the run."""
        return {name: t.numpy() for name, t in self._trimmed(self._views(self.capacity, self._blob.cpu())[1]).items()}


def run_capacity(capacity: Optional[int], data, of_a_stream: int) -> int:
    """The samples a tool's `RunColumns` start with: what the caller asked for, else `len(data)`, else the tool's constant."""
    return capacity if capacity is not None else len(data) if hasattr(data, "__len__") else of_a_stream


def predictions_in_order(model, nn, tagged: Iterable[Tuple[Any, Any]], device, parallelize: bool, rejected: Callable[[Any], None],
                         what: str) -> Iterator[Tuple[Any, Any, Any, Any]]:
    """`model.predict` over the datapoints of `tagged` = (datapoint, tag) pairs -> (tag, datapoint, location_logprobs,
    rewrite_logprobs) in input order.  `predict` keeps the input order and yields the datapoint objects it was given, so what it
    passed over -- its `tensorize` rejected them -- is what was sent before the one that comes out: `rejected(tag)` is called
    for those, in input order, and for the tail.  `what` names the caller and its predict in the error."""
    pending: "deque" = deque()  # (datapoint, tag) of what went in and has not come out

    def tracked():
        for point, tag in tagged:
            pending.append((point, tag))
            yield point

    for point, location_logprobs, rewrite_logprobs in model.predict(tracked(), nn, device, parallelize):
        while True:
            if not pending:
                raise RuntimeError(f"{what} yielded a datapoint it was not given")
            sent, tag = pending.popleft()
            if sent is point:
                break
            rejected(tag)
        yield tag, point, location_logprobs, rewrite_logprobs
    while pending:
        rejected(pending.popleft()[1])


class InOrder:
    """Results leave in the order their slots were opened, whatever order they are completed in.  Slots are opened by the
    tensorising side (a worker thread when parallelised) and completed / drained by the consumer."""

    def __init__(self):
        self._slots: "deque" = deque()
        self.lock = threading.Lock()

    def open(self, slot) -> None:  # slot: any object with a boolean `done`
        self._slots.append(slot)

    def drain(self) -> Iterator[Any]:
        while self._slots and self._slots[0].done:
            yield self._slots.popleft()

    def __len__(self) -> int:
        return len(self._slots)


def save_msgpack_l_gz_reproducibly(data: Iterable[Any], filename) -> None:
    """`utils.msgpackutils.save_msgpack_l_gz` without the time stamp and file name in the gzip header: the same data gives the
    same bytes."""
    import gzip

    import msgpack

    with open(filename, "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as out_file:
        packer = msgpack.Packer(use_bin_type=True)
        for element in data:
            out_file.write(packer.pack(element))
