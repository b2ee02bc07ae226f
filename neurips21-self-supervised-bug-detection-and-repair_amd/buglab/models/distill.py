#!/usr/bin/env python
"""
Usage:
    python -m buglab.models.distill TEACHER_MODEL DATA_PATH OUT_DIR [--limit-num-elements N] [--sequential] [--report-json FILE]

Knowledge distillation, step one: annotate training records with a teacher's distributions -- BEYOND THE REFERENCE, which has
no counterpart.  An `avg` / `consensus` ensemble (buglab.models.ensemble) is the most accurate detector this project builds,
but costs one forward per member and is refused by `visualize`, `bugselector`, `detectorscoring` and `evaluate --on-device`.
Distillation puts its quality into ONE model: the teacher runs once over the training data (here), then a single graph
student trains on the teacher's location and rewrite distributions mixed with the hard labels
(`train.py --distill-weight W --distill-temperature T`, GnnBugLabModule.set_distillation, csrc/bl_distill.hip).

TEACHER_MODEL is any checkpoint `restore_model` loads whose `predict` yields `(datapoint, location_logprobs,
rewrite_logprobs)` triples: the six registry models and `EnsembleWrapper` files.  A teacher that carries a
`ConfidenceCalibration` (buglab.models.calibrate) annotates with calibrated values -- that is what its `predict` reports.

Every record of DATA_PATH (`*.msgpack.l.gz`, a file or a folder) is read with the Python msgpack reader, so that it
round-trips verbatim, and written to OUT_DIR under its shard's name with three more top-level keys:
    teacher_location_nodes      np.unique(graph["reference_nodes"]) ascending, then -1 (NO_BUG)
    teacher_location_logprobs   the same length: what `predict` gave (float32 values, -inf allowed)
    teacher_rewrite_logprobs    one value per `candidate_rewrites` entry, by original index
Records the teacher's `tensorize` rejects are dropped and counted.

One inherited rule to know: `predict` (reference basemodel.py:240-346, `PredictionLayout` here) hands the values of a scout
family (text / var-misuse / arg-swap) out in location order -- the k-th rewrite of the family in first-seen-location order
takes the k-th value of the family's entries sorted by node.  `teacher_rewrite_logprobs[i]` is therefore rewrite i's own value
only where a family's rewrites are listed in ascending node order; elsewhere it is another rewrite's, the values at a node do
not sum to 1, and the training kernel renormalises what it is given.  Such records are counted in the report
(`records_with_unnormalised_rewrite_groups`) and a warning is logged once.
"""
from __future__ import annotations

import argparse
import logging
import sys
from pathlib import Path
from typing import Any, Dict, Iterable, Iterator, Optional

if __package__ in (None, ""):
    sys.path.insert(0, str(Path(__file__).resolve().parents[2]))

import numpy as np

from buglab.models import _distill as K

LOGGER = logging.getLogger(__name__)
TEACHER_KEYS = ("teacher_location_nodes", "teacher_location_logprobs", "teacher_rewrite_logprobs")


def _teacher_view(datapoint):
    """What the teacher's `predict` gets to see: a graph model adds subtoken nodes and `HasSubtoken` edges to a dict graph in
    place (representations/data.py::add_open_vocab_nodes_and_edges); the record that is written must not carry them."""
    g = datapoint["graph"]
    if not isinstance(g, dict):  # the native reader's graphs are read-only arrays
        return datapoint
    return dict(datapoint, graph=dict(g, nodes=list(g["nodes"]), edges={k: list(v) for k, v in g["edges"].items()}))


def _rewrite_groups_normalised(record, tolerance: float = 1e-3) -> bool:
    """Are the annotated rewrite values at every reference node a distribution (|logsumexp| <= tolerance)?  They are whenever
    rewrite i carries its own value; see the warning in `annotate_with_teacher` for when it does not."""
    refs = np.asarray(record["graph"]["reference_nodes"], dtype=np.int64)
    values = np.asarray(record["teacher_rewrite_logprobs"], dtype=np.float64)
    for node in np.unique(refs):
        v = values[refs == node]
        v = v[v > -np.inf]
        if v.size and abs(float(np.log(np.exp(v - v.max()).sum()) + v.max())) > tolerance:
            return False
    return True


def require_teacher(model) -> None:
    from buglab.models.greatreimplementation import GreatVarMisuse

    if isinstance(model, GreatVarMisuse):
        raise ValueError("distill: the GREAT var-misuse model's predict yields a VarMisusePrediction per record, not the location / "
                         "rewrite log-probabilities a student is trained on; use one of the six registry models or an ensemble")
    if not hasattr(model, "predict"):
        raise ValueError(f"distill: {type(model).__name__} has no predict")


def annotate_with_teacher(model, nn, data: Iterable[Any], device, parallelize: bool = False,
                          report: Optional[Dict[str, Any]] = None) -> Iterator[Any]:
    """Yields every record of `data` the teacher predicts, in input order, with the three TEACHER_KEYS added (the record itself
    otherwise untouched).  `report`, when given, is filled as the stream is consumed: records in / out / dropped and the sum
    of the teacher's location entropies."""
    require_teacher(model)
    report = report if report is not None else {}
    report.update({"records_in": 0, "records_out": 0, "records_dropped": 0, "location_entropy_sum": 0.0,
                   "records_with_unnormalised_rewrite_groups": 0})
    if getattr(model, "confidence_calibration", None) is not None:
        LOGGER.info("The teacher carries a confidence calibration %s: records are annotated with CALIBRATED log-probabilities "
                    "(what its predict reports).", model.confidence_calibration)
    from buglab.controllers._batching import predictions_in_order

    def views():  # (view handed to predict, record)
        for record in data:
            if record is not None:
                report["records_in"] += 1
                yield _teacher_view(record), record

    def dropped(_record):  # what predict passed over: its tensorize rejected the record
        report["records_dropped"] += 1

    for record, _, location_logprobs, rewrite_logprobs in predictions_in_order(model, nn, views(), device, parallelize, dropped,
                                                                               "distill: the teacher's predict"):
        nodes = np.unique(record["graph"]["reference_nodes"]).tolist()
        if sorted(k for k in location_logprobs if k != -1) != nodes or -1 not in location_logprobs:
            raise RuntimeError("distill: the teacher's location distribution is not over the record's candidate nodes + NO_BUG")
        if len(rewrite_logprobs) != len(record["candidate_rewrites"]):
            raise RuntimeError("distill: the teacher's rewrite distribution does not have one value per candidate rewrite")
        # float32 values, the student's precision: an ensemble's predict combines its members in fp64
        f32 = lambda v: float(np.float32(v))
        loc = [f32(location_logprobs[n]) for n in nodes] + [f32(location_logprobs[-1])]
        record["teacher_location_nodes"] = [int(n) for n in nodes] + [-1]
        record["teacher_location_logprobs"] = loc
        record["teacher_rewrite_logprobs"] = [f32(v) for v in rewrite_logprobs]
        if not _rewrite_groups_normalised(record):
            report["records_with_unnormalised_rewrite_groups"] += 1
            if report["records_with_unnormalised_rewrite_groups"] == 1:
                LOGGER.warning(
                    "distill: the teacher's rewrite values at a location of %s do not sum to 1.  `predict` hands a scout family's "
                    "values out in location order (PredictionLayout): where a family's rewrites are not listed in ascending node "
                    "order, rewrite i carries another rewrite's value and the student is taught the renormalised mix.  Counted in "
                    "the report; logged once.", record["graph"].get("path"))
        report["records_out"] += 1
        report["location_entropy_sum"] += K.entropy(loc)
        yield record


def annotate_shards(model, nn, data_path, out_dir, device, *, parallelize: bool = False, limit_num_elements: Optional[int] = None
                    ) -> Dict[str, Any]:
    """Every `*.msgpack.l.gz` shard of `data_path` -> the same shard name under `out_dir`, annotated.  -> the report."""
    from buglab.utils.msgpackutils import load_msgpack_l_gz, save_msgpack_l_gz

    local = Path(str(getattr(data_path, "path", data_path)))
    files = [local] if local.is_file() else sorted(local.glob("*.msgpack.l.gz"))
    if not files:
        raise ValueError(f"distill: no *.msgpack.l.gz shard under {data_path}")
    out_dir = Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    total = {"records_in": 0, "records_out": 0, "records_dropped": 0, "location_entropy_sum": 0.0,
             "records_with_unnormalised_rewrite_groups": 0, "shards": []}
    for shard in files:
        remaining = None if limit_num_elements is None else limit_num_elements - total["records_in"]
        if remaining is not None and remaining <= 0:
            break

        def records():
            # the Python reader: plain dicts and lists, which round-trip verbatim (buglab/data/deduplication/__main__.py)
            for i, record in enumerate(load_msgpack_l_gz(shard, native=False)):
                if remaining is not None and i >= remaining:
                    return
                yield record

        rep: Dict[str, Any] = {}
        target = out_dir / shard.name
        if target.resolve() == shard.resolve():
            raise ValueError(f"distill: OUT_DIR would overwrite the input shard {shard}")
        save_msgpack_l_gz(annotate_with_teacher(model, nn, records(), device, parallelize, rep), target)
        for k in ("records_in", "records_out", "records_dropped", "location_entropy_sum", "records_with_unnormalised_rewrite_groups"):
            total[k] += rep[k]
        total["shards"].append({"name": shard.name, "records_in": rep["records_in"], "records_out": rep["records_out"]})
    total["mean_location_entropy"] = total["location_entropy_sum"] / total["records_out"] if total["records_out"] else float("nan")
    return total


def format_report(report: Dict[str, Any]) -> str:
    return (f"Annotated {report['records_out']} of {report['records_in']} records in {len(report['shards'])} shard(s) "
            f"({report['records_dropped']} dropped: the teacher could not tensorise them).\n"
            f"  mean teacher entropy of the location distribution: {report['mean_location_entropy']:.6f} nats\n"
            + (f"  {report['records_with_unnormalised_rewrite_groups']} record(s) whose rewrite values at a location do not sum to 1 "
               "(predict's family order; see the module docstring)\n" if report["records_with_unnormalised_rewrite_groups"] else ""))


def parse_args(argv=None) -> argparse.Namespace:
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("TEACHER_MODEL", help="A trained detector or ensemble checkpoint (`*.pkl.gz`).")
    p.add_argument("DATA_PATH", help="Training `*.msgpack.l.gz` data: a file or a folder.")
    p.add_argument("OUT_DIR", help="Where to write the annotated shards, under the input shard names.")
    p.add_argument("--limit-num-elements", type=int, default=None, help="Annotate at most this many records.")
    p.add_argument("--sequential", action="store_true", help="Do not parallelize data loading.")
    p.add_argument("--report-json", default=None, help="Also write the report as data.")
    return p.parse_args(argv)


def main(argv=None) -> Dict[str, Any]:
    from buglab.models._cli import open_model, require_gpu, write_report_json

    args = parse_args(argv)
    require_gpu(None, "distill")
    model, nn, device, _ = open_model(args.TEACHER_MODEL)
    require_teacher(model)
    report = annotate_shards(model, nn, args.DATA_PATH, args.OUT_DIR, device, parallelize=not args.sequential,
                             limit_num_elements=args.limit_num_elements)
    sys.stdout.write(format_report(report))
    write_report_json(args.report_json, report)
    return report


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    main()
