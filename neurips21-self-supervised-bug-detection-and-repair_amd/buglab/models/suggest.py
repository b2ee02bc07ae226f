#!/usr/bin/env python
"""
Usage:
    suggest.py [options] MODEL_FILENAME DATA_PATH OUT_PATH

Options:
    --top-k=<K>                Suggestions listed per sample, 1 <= K <= 32. [default: 5]
    --limit-num-elements=<num> Limit the number of elements to rank.
    --sequential               Do not parallelize data loading. Makes debugging easier.
    --host                     Rank the `predict` triples on the host (always, for an ensemble).
    --assume-buggy             NO_BUG is never suggested.
    --min-probability=<P>      List only suggestions of at least this probability (the ranks are unchanged).
    -h --help                  Show this screen.

BEYOND THE REFERENCE, which reduces every sample to one answer.  For each sample: the K most probable fixes in order -- each a
candidate rewrite or NO_BUG, ranked by JOINT probability, location times rewrite -- with their probabilities, and, where the
sample carries a label, the rank the model gave the true fix and the true location.  OUT_PATH receives JSON lines (gzip when
the name ends in .gz), one record per sample `tensorize` accepts, in input order; the rejected ones are counted on stderr.

Two paths give the same records.  The default one (single registry models) leaves the model's flat output on the device and
ranks each predict minibatch there in one launch (hip_ops.rank_suggestions, csrc/bl_suggest.hip, through the index arrays of
buglab/models/_suggest.py); the results stay on the device for the whole run and are copied back once.  `--host`, and any
ensemble, walk the triples of `model.predict` (`suggestions_of_prediction`).  Calibrated values are ranked where the checkpoint
carries a calibration.  The probabilities (exp of the log-probabilities) and their sum `mass` are formed on the host.

A suggestion's `rank` 0 is not what evaluate.py calls a repaired sample: that takes the best rewrite at the most probable
location, this ranks the products.
"""
import argparse
import math
import sys
from pathlib import Path
from typing import Any, Callable, Dict, Iterable, Iterator, List, NamedTuple, Optional

if __package__ in (None, ""):
    sys.path.insert(0, str(Path(__file__).resolve().parents[2]))

import torch

from buglab.models import _suggest as S
from buglab.models._cli import open_model, require_gpu, write_records  # noqa: F401  (write_records: imported from here too)
from buglab.models._suggest import Ranked


class Suggestions(NamedTuple):
    """One sample's answer: its position in the input, the datapoint, and its ranking."""

    position: int
    datapoint: Any
    ranked: Ranked

    def record(self, min_probability: Optional[float] = None) -> Dict[str, Any]:
        return suggestion_record(self.position, self.datapoint, self.ranked, min_probability)


def suggestion_record(position: int, datapoint, ranked: Ranked, min_probability: Optional[float] = None) -> Dict[str, Any]:
    """The JSON record of one sample.  Identification as visualize.py reads it (graph.path without its site-packages prefix,
    package_name).  `mass`: the sum of the listed probabilities, added in rank order."""
    graph = datapoint["graph"]
    path = graph.get("path", "")
    if "/site-packages/" in path:
        path = path[path.find("/site-packages/") + len("/site-packages/"):]
    refs = graph["reference_nodes"]
    listed, mass = [], 0.0
    for rank, (entry, logprob) in enumerate(zip(ranked.entries, ranked.logprobs)):
        probability = math.exp(logprob) if logprob < math.inf else math.inf
        if min_probability is not None and not probability >= min_probability:
            break  # in rank order: nothing later is more probable
        mass += probability
        item: Dict[str, Any] = {"rank": rank, "logprob": logprob, "probability": probability}
        if entry == len(refs):
            item.update(kind="no_bug", rewrite_index=None, reference_node=None)
        else:
            item.update(kind="rewrite", rewrite_index=entry, reference_node=int(refs[entry]),
                        candidate_rewrite_range=datapoint["candidate_rewrite_ranges"][entry],
                        candidate_rewrite=datapoint["candidate_rewrites"][entry],
                        candidate_rewrite_metadata=datapoint["candidate_rewrite_metadata"][entry])
        listed.append(item)
    out: Dict[str, Any] = {"position": position, "filename": path, "package": datapoint.get("package_name"), "suggestions": listed,
                           "mass": mass}
    if "target_fix_action_idx" in datapoint:
        out.update(target_fix_action_idx=datapoint["target_fix_action_idx"], truth_rank=ranked.truth_rank,
                   truth_location_rank=ranked.truth_location_rank)
    return out


def _suggest_host(model, nn, data, device, k, assume_buggy, parallelize, rejected) -> Iterator[Suggestions]:
    from buglab.controllers._batching import predictions_in_order

    tagged = ((point, position) for position, point in enumerate(data))
    for position, point, location_logprobs, rewrite_logprobs in predictions_in_order(model, nn, tagged, device, parallelize, rejected,
                                                                                     "suggest: predict"):
        yield Suggestions(position, point, S.suggestions_of_prediction(point, location_logprobs, rewrite_logprobs, k, assume_buggy))


def _suggest_on_device(model, nn, data, device, k, assume_buggy, parallelize, rejected, capacity) -> Iterator[Suggestions]:
    from buglab.controllers import _batching as Bt
    from buglab.models import hip_ops

    Bt.require_single_model(model, "suggest")
    device = torch.device(device)

    def extend(layout, points, dev, mb):
        ix = S.suggest_indices(layout, points, mb.get("node_mappings"))
        fields = hip_ops.SUGGEST_INDEX_FIELDS
        return {"ix": dict(zip(fields, Bt.to_device_i32([getattr(ix, f) for f in fields], dev))), "points": points}

    cols = Bt.RunColumns(device, Bt.run_capacity(capacity, data, 1 << 14),
                         [("logprob", "float64", (Bt.SAMPLES, k)), ("entry", "int32", (Bt.SAMPLES, k)), ("rank", "int32", (2, Bt.SAMPLES))])
    points: List[Any] = []
    positions: List[int] = []
    nn.eval()
    with torch.no_grad(), model._tensorize_all_location_rewrites():
        for mb, tags in Bt.prediction_minibatches(model, ((d, i) for i, d in enumerate(data)), device, parallelize, extend, rejected,
                                                  extend_sees_minibatch=True):
            flat = Bt.flat_prediction_output(nn, mb)
            B = len(mb["selfsup"]["points"])
            assert len(tags) == B
            n = cols.reserve(B)
            hip_ops.rank_suggestions(flat, mb["selfsup"]["ix"], cols["rank"], cols["entry"], cols["logprob"], n, k=k,
                                     skip_nobug=assume_buggy)
            points.extend(mb["selfsup"]["points"]), positions.extend(tags)
    host = cols.to_host()  # the one copy (and the one synchronisation) of the run
    logprob, entry, rank = host["logprob"], host["entry"], host["rank"]
    for b in range(cols.n):
        listed = int((entry[b] >= 0).sum())
        yield Suggestions(positions[b], points[b], Ranked(entry[b, :listed].tolist(), logprob[b, :listed].tolist(), int(rank[0, b]),
                                                          int(rank[1, b])))


def suggest(model, nn, data: Iterable[Any], device, k: int = 5, *, host: bool = False, assume_buggy: bool = False,
            parallelize: bool = True, rejected: Optional[Callable[[int], None]] = None, capacity: Optional[int] = None
            ) -> Iterator[Suggestions]:
    """The ranked suggestions of every datapoint of `data` that `tensorize` accepts, in input order; `rejected(position)` is
    called for the others.  On the device unless `host` is set or `model` is an ensemble (`EnsembleWrapper`), which
    `require_single_model` refuses there.  The device path yields after the run's one copy back; `capacity`: the samples its
    buffers (`RunColumns`) start with, by default `len(data)`, or 1 << 14 for a stream."""
    from buglab.models.ensemble.wrapper import EnsembleWrapper

    if not 1 <= int(k) <= S.MAX_K:
        raise ValueError(f"suggest: k must be in [1, {S.MAX_K}] (got {k})")
    rejected = rejected or (lambda position: None)
    if host or isinstance(model, EnsembleWrapper):
        return _suggest_host(model, nn, data, device, int(k), bool(assume_buggy), parallelize, rejected)
    return _suggest_on_device(model, nn, data, device, int(k), bool(assume_buggy), parallelize, rejected, capacity)


def run(arguments) -> int:
    from buglab.runtime.richpath import RichPath
    from buglab.utils.msgpackutils import load_all_msgpack_l_gz

    lim = None if arguments["--limit-num-elements"] is None else int(arguments["--limit-num-elements"])
    data = load_all_msgpack_l_gz(RichPath.create(arguments["DATA_PATH"]), shuffle=False, limit_num_yielded_elements=lim)  # a stream
    require_gpu(None, "suggest.py")
    model, nn, device, _ = open_model(arguments["MODEL_FILENAME"])
    min_probability = None if arguments.get("--min-probability") is None else float(arguments["--min-probability"])
    refused: List[int] = []
    found = suggest(model, nn, data, device, int(arguments["--top-k"]), host=bool(arguments.get("--host")),
                    assume_buggy=bool(arguments.get("--assume-buggy")), parallelize=not arguments.get("--sequential"),
                    rejected=refused.append)
    count = write_records((s.record(min_probability) for s in found), arguments["OUT_PATH"])
    print(f"suggest.py: {count} samples ranked, {len(refused)} rejected by tensorize", file=sys.stderr)
    return count


if __name__ == "__main__":
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("MODEL_FILENAME")
    p.add_argument("DATA_PATH")
    p.add_argument("OUT_PATH")
    p.add_argument("--top-k", default=5, type=int)
    p.add_argument("--limit-num-elements", default=None)
    p.add_argument("--sequential", action="store_true")
    p.add_argument("--host", action="store_true")
    p.add_argument("--assume-buggy", action="store_true")
    p.add_argument("--min-probability", default=None, type=float)
    ns = p.parse_args()
    run({"MODEL_FILENAME": ns.MODEL_FILENAME, "DATA_PATH": ns.DATA_PATH, "OUT_PATH": ns.OUT_PATH, "--top-k": ns.top_k,
         "--limit-num-elements": ns.limit_num_elements, "--sequential": ns.sequential, "--host": ns.host,
         "--assume-buggy": ns.assume_buggy, "--min-probability": ns.min_probability})
