#!/usr/bin/env python
"""
Usage:
    python -m buglab.controllers.detectorscoring MODEL_FILENAME RECORDS_PATH OUT_FILENAME [--sequential]

Detector scoring of rewritten code -- the compute of reference buglab/controllers/detectordatascoringworker.py without its
ZeroMQ plumbing and replay buffer.  A record is `{"original": datapoint, "rewrites": {str(idx) | "NO_BUG": (datapoint |
None, prob)}}`: the original and what it became under each selected rewrite (each rewritten datapoint's own
`target_fix_action_idx` points at the rewrite that undoes it; None for NO_BUG).  The log-probability the detector gives to the
TRUE FIX of each one -- `location_logprobs[-1]` without a bug, else `location_logprobs[ground node] +
rewrite_logprobs[target_fix_action_idx]` (:118-130) -- is written into `original["candidate_rewrite_logprobs"]`
(`len(reference_nodes) + 1` values, NO_BUG last, -inf where nothing was scored).  The scored originals, written to
OUT_FILENAME, are selector training data for `buglab/models/train.py` as they are.

The reference calls `model.predict` on the ~5 graphs of one record, copies every prediction value to the host and picks two
of them per graph in Python.  Here the graphs of MANY records form one stream through the minibatches of the model's own
`predict` (full minibatches, not 5 graphs); where the two values sit is computed on the host in the collate worker, and
after the forward one kernel (hip_ops.score_targets, csrc/bl_selfsup.hip) adds them in fp64: B doubles are copied back per
minibatch.  A record is yielded as soon as its last graph is scored, in input order.

Where this differs from the reference ("Self-supervision services"): a None graph, or one the model's `tensorize`
rejects, leaves ITS slot at -inf; in the reference's loop such a graph shifts the scores of the graphs after it to the wrong
rewrite indices (:101-111, 118-130 index `rewrite_idxs` by position among the predictions).
"""
from __future__ import annotations

import argparse
import logging
import math
import sys
from pathlib import Path
from typing import Any, Iterable, Iterator

if __package__ in (None, ""):
    sys.path.insert(0, str(Path(__file__).resolve().parents[2]))

LOGGER = logging.getLogger(__name__)


class _Record:
    __slots__ = ("original", "scores", "pending")

    def __init__(self, original, pending: int):
        self.original = original
        self.scores = [-math.inf] * (len(original["graph"]["reference_nodes"]) + 1)  # +1 for the NO_BUG case (:113-114)
        self.pending = pending  # graphs on their way through the model

    @property
    def done(self) -> bool:
        return self.pending == 0


def rewrite_indices(record) -> list:
    """The record's rewrite keys as indices into `candidate_rewrite_logprobs` ("NO_BUG" -> -1, the last slot); duplicates and
    indices outside the original's candidate rewrites are rejected (the reference asserts the former, :110)."""
    num = len(record["original"]["graph"]["reference_nodes"])
    idxs = [-1 if key == "NO_BUG" else int(key) for key in record["rewrites"]]
    if len(idxs) != len(set(idxs)):
        raise ValueError(f"score_rewrites: duplicate rewrite indices in a record: {sorted(idxs)}")
    if any(i < -1 or i >= num for i in idxs):
        raise ValueError(f"score_rewrites: rewrite index outside the original's {num} candidate rewrites: {sorted(idxs)}")
    return idxs


def score_rewrites(model, nn, records: Iterable[Any], device, *, parallelize: bool = False) -> Iterator[Any]:
    """-> each record's original datapoint with `candidate_rewrite_logprobs` filled, in input order."""
    import torch

    from buglab.controllers import _batching as Bt
    from buglab.models import hip_ops

    Bt.require_single_model(model, "score_rewrites")
    device = torch.device(device)
    order = Bt.InOrder()

    def tagged():
        for record in records:
            graphs = []
            for idx, (key, (graph, _prob)) in zip(rewrite_indices(record), record["rewrites"].items()):
                if graph is None:
                    LOGGER.error(f"None element for graph. Rewrite_idx: {key}")
                    continue
                graphs.append((graph, idx))
            state = _Record(record["original"], len(graphs))
            order.open(state)
            for graph, idx in graphs:
                yield graph, (state, idx)

    def rejected(tag):  # the model cannot tensorise this graph: its slot stays -inf
        with order.lock:
            tag[0].pending -= 1

    def extend(layout, points, dev):
        ix = Bt.selfsup_indices(layout, points)
        return dict(zip(("tgt_loc", "tgt_rw"), Bt.to_device_i32([ix.tgt_loc, ix.tgt_rw], dev)))

    def emit():
        for state in order.drain():
            state.original["candidate_rewrite_logprobs"] = state.scores
            yield state.original

    nn.eval()
    with torch.no_grad(), model._tensorize_all_location_rewrites():
        for mb, tags in Bt.prediction_minibatches(model, tagged(), device, parallelize, extend, rejected):
            flat = Bt.flat_prediction_output(nn, mb)
            scores = hip_ops.score_targets(flat, mb["selfsup"]["tgt_loc"], mb["selfsup"]["tgt_rw"]).cpu().tolist()  # B doubles
            with order.lock:
                for (state, idx), value in zip(tags, scores):
                    state.scores[idx] = value  # -1 (NO_BUG) is the last slot
                    state.pending -= 1
            yield from emit()
    yield from emit()
    assert len(order) == 0


def parse_args(argv=None) -> argparse.Namespace:
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("MODEL_FILENAME", help="A trained detector checkpoint (`*.pkl.gz`).")
    p.add_argument("RECORDS_PATH", help="A `*.msgpack.l.gz` file of records, or a folder of them.")
    p.add_argument("OUT_FILENAME", help="The `*.msgpack.l.gz` file to write the scored originals to.")
    p.add_argument("--sequential", action="store_true", help="Should any computations happen sequentially?")
    return p.parse_args(argv)


def load_records(path) -> Iterator[Any]:
    """Records are nested datapoints: always through the msgpack reader (the native shard reader reads plain datapoints)."""
    from buglab.utils.msgpackutils import load_msgpack_l_gz

    path = Path(path)
    files = sorted(path.glob("*.msgpack.l.gz")) if path.is_dir() else [path]
    for f in files:
        yield from load_msgpack_l_gz(f, native=False)


def run(args: argparse.Namespace) -> int:
    from buglab.controllers._batching import save_msgpack_l_gz_reproducibly
    from buglab.models._cli import open_model, require_gpu

    require_gpu(None, "detectorscoring")
    model, nn, device, _ = open_model(args.MODEL_FILENAME)
    count = 0

    def scored():
        nonlocal count
        for original in score_rewrites(model, nn, load_records(args.RECORDS_PATH), device, parallelize=not args.sequential):
            count += 1
            yield original

    save_msgpack_l_gz_reproducibly(scored(), args.OUT_FILENAME)
    print(f"Scored {count} records.")
    return count


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    run(parse_args())
