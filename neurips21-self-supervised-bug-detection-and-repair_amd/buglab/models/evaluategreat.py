#!/usr/bin/env python
"""
Usage:
    evaluategreat.py [options] MODEL_FILENAME TEST_DATA_PATH

Options:
    --minibatch-size=<size>    The minibatch size. [default: 30]
    --limit-num-elements=<num> Limit the number of records to evaluate on.
    --sequential               Do not parallelize data loading. Makes debugging easier.
    --report-json=<path>       Also write both blocks of the report as data.
    --predictions-out=<path>   Write one JSON line per evaluated sample.
    --host-judge               Copy every minibatch's logits back and judge them on the host (the comparison path).
    -h --help                  Show this screen.

Evaluates a checkpoint of the GREAT var-misuse model (buglab/models/traingreat.py) on a directory of GREAT `*.jsonl.gz` files.
The reference has no counterpart: its greatreimplementation.py ends at `finalize_minibatch`.

Every minibatch is one forward judged on the device (`GreatVarMisuseModule.predict_minibatch`, csrc/bl_varmisuse_predict.hip): the
samples' records -- predicted location and repair, their log-probabilities, the two verdicts -- are written into one buffer that
stays on the device for the whole run and is copied back once.  `--host-judge` copies each minibatch's logits back instead and
judges them with the NumPy twin (buglab/models/_great_predict.py); the report is the same.

The report has two blocks: the model's own metrics (the seven entries `GreatVarMisuseModule.report_metrics` gives after a
validation pass, under the same names, plus three that need a prediction) and the text buglab/models/evaluate.py prints, from
the same `ColumnarEvaluationReport`.
"""
import argparse
import json
import sys
from pathlib import Path
from typing import Any, Dict, Iterable, List, NamedTuple, Optional

if __package__ in (None, ""):
    sys.path.insert(0, str(Path(__file__).resolve().parents[2]))

import numpy as np
import torch

from buglab.models._great_predict import RECORD_D, RECORD_I, judge_great_host
from buglab.models.evaluate import ColumnarEvaluationReport
from buglab.models.greatreimplementation import metrics_from_stats

COUNT_NAMES = ("samples", "localization_hits", "buggy_localization_hits", "buggy_samples", "repair_hits", "localization_loss_sum",
               "repair_loss_sum")  # the first seven of greatreimplementation.STATS_NAMES


class GreatEvaluation(NamedTuple):
    out_d: np.ndarray            # float64 [7, n]: the records' fp64 rows (include/buglab_hip.h::bl_varmisuse_predict)
    out_i: np.ndarray            # int32 [4, n]
    error_location: np.ndarray   # int64 [n]
    kinds: List[str]             # per sample: `bug_kind_name` of a buggy record, "NoBug" otherwise
    skipped: int                 # records left out (too long, or buggy without a candidate that is a target)

    @property
    def has_bug(self) -> np.ndarray:
        return self.error_location != 0

    def counts(self) -> Dict[str, float]:
        """What `metric_stats` holds after a validation pass over the same samples (names: COUNT_NAMES).  A sample whose
        error location is outside its unmasked positions has log-probability -inf there (row 4), so it makes the localization
        loss sum +inf, as it makes the training loss; `unreachable_error_locations` counts such samples."""
        buggy = self.has_bug
        loc_ok, rep_ok = self.out_i[2] != 0, self.out_i[3] != 0
        values = (buggy.shape[0], loc_ok.sum(), (loc_ok & buggy).sum(), buggy.sum(), (rep_ok & buggy).sum(),
                  -self.out_d[4].sum(), -self.out_d[6][buggy].sum())
        return {k: float(v) for k, v in zip(COUNT_NAMES, values)}

    def unreachable_error_locations(self) -> int:
        """Samples whose error location lies outside [0, lens_att): no prediction can be right and their loss is infinite."""
        return int(np.isneginf(self.out_d[4]).sum())

    def metrics(self) -> Dict[str, Any]:
        """Block 1."""
        buggy = self.has_bug
        n, n_buggy = int(buggy.shape[0]), int(buggy.sum())
        warned = self.out_i[0] != 0
        both = (self.out_i[2] != 0) & (self.out_i[3] != 0) & buggy
        div = lambda a, b: a / b if b != 0 else float("nan")
        out = metrics_from_stats(*self.counts().values())
        out["Classification Accuracy"] = div(int((warned == buggy).sum()), n)
        out["Localization+Repair Accuracy (Buggy)"] = div(int(both.sum()), n_buggy)
        out["False Alarm Rate"] = div(int((warned & ~buggy).sum()), n - n_buggy)
        return out

    def report(self) -> ColumnarEvaluationReport:
        """Block 2: confidence = log-probability of the predicted location; warned = a location was predicted; a no-bug sample
        is "repaired" when position 0 is predicted."""
        buggy = self.has_bug
        names = ["NoBug"] + sorted(set(self.kinds) - {"NoBug"})
        ids = {name: i for i, name in enumerate(names)}
        loc_ok, rep_ok = self.out_i[2] != 0, self.out_i[3] != 0
        return ColumnarEvaluationReport(self.out_d[2], buggy, self.out_i[0] != 0, loc_ok, np.where(buggy, self.out_i[3], -1),
                                        loc_ok & (~buggy | rep_ok), [ids[k] for k in self.kinds], names)

    def format(self) -> str:
        lines = ["=" * 34, "GREAT var-misuse model"]
        for name, value in self.metrics().items():
            lines.append(f"{name}: {value}" if isinstance(value, int) else f"{name}: {value:.4f}")
        lines.append(f"Skipped records: {self.skipped}")
        if self.unreachable_error_locations():
            lines.append(f"Samples with the error location outside the unmasked positions (their localization loss is inf): "
                         f"{self.unreachable_error_locations()}")
        return "\n".join(lines) + "\n" + self.report().format()

    def to_json(self) -> str:
        r = self.report()
        return json.dumps({"metrics": self.metrics(), "counts": self.counts(), "skipped": self.skipped,
                           "unreachable_error_locations": self.unreachable_error_locations(), "summary": r.summary(),
                           "per_scout": r.per_scout(), "curves": {k: v.tolist() for k, v in r.curves().items()}},
                          indent=1, sort_keys=True) + "\n"

    def prediction_lines(self) -> Iterable[str]:
        buggy = self.has_bug
        for k in range(buggy.shape[0]):
            repair = int(self.out_i[1, k])
            yield json.dumps({
                "index": k, "has_bug": bool(buggy[k]), "error_location": int(self.error_location[k]), "kind": self.kinds[k],
                "predicted_location": int(self.out_i[0, k]), "location_logprob": float(self.out_d[2, k]),
                "no_bug_logprob": float(self.out_d[3, k]), "error_location_logprob": float(self.out_d[4, k]),
                "predicted_repair": repair if repair >= 0 else None, "repair_logprob": float(self.out_d[5, k]) if repair >= 0 else None,
                "location_correct": bool(self.out_i[2, k]), "repair_is_target": bool(self.out_i[3, k])})


def evaluate_great(model, nn, data: Iterable[Any], device, *, minibatch_size: int = 30, parallelize: bool = True,
                   on_device: bool = True, capacity: Optional[int] = None) -> GreatEvaluation:
    """Labelled records -> GreatEvaluation.  The samples are those a validation pass sees (`tensorize_for_prediction(...,
    labelled=True)` rejects what `tensorize` rejects), in input order, `minibatch_size` at a time.  `on_device`: the records of
    all minibatches stay in one device buffer (`RunColumns`: 72 bytes per sample, `capacity` samples to start with, by default
    `len(data)` or 1 << 14 for a stream) that is copied back once, the run's only synchronisation.  Otherwise every
    minibatch's logits are copied back and judged by `judge_great_host`.  Leaves `nn`'s training flag, metric counters and dropout step counter alone."""
    from buglab.models import hip_ops

    device = torch.device(device)
    assert (RECORD_D, RECORD_I) == (hip_ops.VARMISUSE_RECORD_D, hip_ops.VARMISUSE_RECORD_I)
    error_location: List[int] = []
    kinds: List[str] = []
    skipped = [0]

    def rejected(_record):
        skipped[0] += 1

    if on_device:  # [out_d | out_i] in one allocation: one copy back
        from buglab.controllers import _batching as Bt

        cols = Bt.RunColumns(device, Bt.run_capacity(capacity, data, 1 << 14),
                             [("out_d", "float64", (RECORD_D, Bt.SAMPLES)), ("out_i", "int32", (RECORD_I, Bt.SAMPLES))])
    host_d, host_i = [], []
    for mb, records in model.prediction_minibatches(data, device, parallelize, minibatch_size, labelled=True, rejected=rejected):
        B = len(records)
        for r in records:
            err = int(r["error_location"])
            error_location.append(err)
            kinds.append(str(r.get("bug_kind_name") or "VARIABLE_MISUSE") if err != 0 else "NoBug")
        if on_device:
            n = cols.reserve(B)
            nn.predict_minibatch(mb, cols["out_d"], cols["out_i"], n)
        else:
            scratch_d = torch.empty((RECORD_D, B), dtype=torch.float64, device=device)
            scratch_i = torch.empty((RECORD_I, B), dtype=torch.int32, device=device)
            logits = nn.predict_minibatch(mb, scratch_d, scratch_i, 0).cpu().numpy()
            h = mb["host"]
            d, i = judge_great_host(logits, mb["token_ids"].shape[1], h["lens_att"], h["error_locations"], h["target_mask"])
            host_d.append(d), host_i.append(i)
    if on_device:
        rec_d, rec_i = cols.to_host().values()  # the one copy (and the one synchronisation) of the run
    else:
        rec_d = np.concatenate(host_d, axis=1) if host_d else np.empty((RECORD_D, 0))
        rec_i = np.concatenate(host_i, axis=1) if host_i else np.empty((RECORD_I, 0), dtype=np.int32)
    return GreatEvaluation(rec_d, rec_i, np.asarray(error_location, dtype=np.int64), kinds, skipped[0])


def run(arguments):
    from buglab.models.traingreat import load_all_json_l_gz
    from buglab.models._cli import open_model, require_gpu

    require_gpu(None, "evaluategreat.py", "the GREAT model")
    lim = None if arguments.get("--limit-num-elements") is None else int(arguments["--limit-num-elements"])
    data = load_all_json_l_gz(arguments["TEST_DATA_PATH"], limit_num_yielded_elements=lim)
    model, nn, device, _ = open_model(arguments["MODEL_FILENAME"])
    result = evaluate_great(model, nn, data, device, minibatch_size=int(arguments.get("--minibatch-size") or 30),
                            parallelize=not arguments.get("--sequential"), on_device=not arguments.get("--host-judge"))
    sys.stdout.write(result.format())
    if arguments.get("--report-json") is not None:
        with open(arguments["--report-json"], "w", encoding="utf-8") as f:
            f.write(result.to_json())
    if arguments.get("--predictions-out") is not None:
        with open(arguments["--predictions-out"], "w", encoding="utf-8") as f:
            for line in result.prediction_lines():
                f.write(line + "\n")
    return result


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("MODEL_FILENAME")
    p.add_argument("TEST_DATA_PATH")
    p.add_argument("--minibatch-size", default="30")
    p.add_argument("--limit-num-elements", default=None)
    p.add_argument("--sequential", action="store_true")
    p.add_argument("--report-json", default=None)
    p.add_argument("--predictions-out", default=None)
    p.add_argument("--host-judge", action="store_true")
    ns = p.parse_args(argv)
    d = {"MODEL_FILENAME": ns.MODEL_FILENAME, "TEST_DATA_PATH": ns.TEST_DATA_PATH}
    for k, v in vars(ns).items():
        if not k.isupper():
            d["--" + k.replace("_", "-")] = v
    return d


if __name__ == "__main__":
    run(parse_args())
