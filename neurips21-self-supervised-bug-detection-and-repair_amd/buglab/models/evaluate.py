#!/usr/bin/env python
"""
Usage:
    evaluate.py [options] MODEL_FILENAME TEST_DATA_PATH

Options:
    --assume-buggy             Never predict NO_BUG
    --eval-only-no-bug         Evaluate only NO_BUG samples.
    --limit-num-elements=<num> Limit the number of elements to evaluate on.
    --sequential               Do not parallelize data loading. Makes debugging easier.
    --on-device                Judge every predict minibatch on the device (single models only; same report).
    --report-json=<path>       Also write the report as data: summary, per-scout tables and curves.
    --top-k=<K>                After the report, a block on ranked suggestions (buglab/models/suggest.py): the share of samples
                               whose true fix, and whose true location, is within the model's top 1..K, and the mean reciprocal
                               ranks.  The fix is ranked among the sample's rewrites and NO_BUG by JOINT probability (location
                               times rewrite), so its top-1 is not the "Accuracy" above, which takes the best rewrite at the
                               most probable location.  1 <= K <= 32.
    --at-operating-point       After the report, what the checkpoint's warning operating point gives on this data
                               (buglab/models/operatingpoint.py): warnings raised, precisions and recalls at that threshold.
    --minibatch-size=<size>    Accepted for command-line compatibility (the reference parses and ignores it too).
    --restore-path=<path>      Accepted for command-line compatibility (unused by the reference's run()).
    --quiet                    Accepted for command-line compatibility.
    --debug                    Accepted for command-line compatibility.
    -h --help                  Show this screen.

Counterpart of reference buglab/models/evaluate.py (same positional arguments and the options that
do not need Azure).  The metrics and the printed report follow reference evaluate.py:60-255 line for line in content:
joint / detection / localization / repair-given-location accuracies, the per-scout breakdowns, and the six
threshold curves (false-discovery rate, detection precision / recall, NO_BUG precision, detect-and-repair precision /
recall) sampled at 100 thresholds.  tests/test_evaluate_golden.py compares the report with the one the reference's
own loop prints for the same predictions.

Two paths give the same report.  The default one walks the `(datapoint, location_logprobs, rewrite_logprobs)` triples of
`model.predict` on the host, one sample at a time (`judge_sample`).  `--on-device` (`evaluate_on_device`) leaves the model's flat
output on the device, judges each predict minibatch there in one launch (hip_ops.eval_judge, csrc/bl_evaluate.hip, through the
index arrays of buglab/models/_evaluate.py), keeps the outcome columns on the device for the whole run and copies them back once;
the counts and curves are then the same NumPy code on columns (`ColumnarEvaluationReport`).

`--top-k K` adds, on both paths, the ranks of the true fix and of the true location (buglab/models/_suggest.py: the host path
ranks each triple with `suggestions_of_prediction`, the device path launches hip_ops.rank_suggestions next to the judge) and
prints `top_k_summary` of the two rank columns after the report.  Without the flag nothing of this is allocated or launched.
"""
import argparse
import json
import math
import sys
from collections import defaultdict
from pathlib import Path
from typing import Any, Dict, Iterable, List, NamedTuple, Optional, Sequence

if __package__ in (None, ""):
    sys.path.insert(0, str(Path(__file__).resolve().parents[2]))

import numpy as np
import torch

from buglab.models._cli import open_model, require_gpu
from buglab.runtime.richpath import RichPath
from buglab.utils.msgpackutils import load_all_msgpack_l_gz

NO_BUG_NODE = -1  # key of the "no bug" option in a sample's location log-probabilities
CURVE_POINTS = 100


class SampleOutcome(NamedTuple):
    """What the report needs from one evaluated sample.  Field order = the sort order of the threshold curves
    (most confident prediction first; ties fall through to the flags, like the reference's tuple sort)."""
    confidence: float                    # log-probability of the predicted location (or of "no bug")
    has_bug: bool
    warned: bool                         # the prediction is a location, not "no bug"
    location_correct: bool               # for a correct sample: "no bug" was predicted
    repair_given_location: Optional[bool]  # best rewrite AT THE TRUE location is the target; None without a bug
    repaired: bool                       # location and rewrite both right
    scout: str                           # rewrite scout of the target, "NoBug" for a correct sample


def _best_rewrite_at(node: int, reference_nodes, rewrite_logprobs) -> Optional[int]:
    best, best_lp = None, -math.inf
    for i, (at, lp) in enumerate(zip(reference_nodes, rewrite_logprobs)):
        if at == node and lp > best_lp:
            best, best_lp = i, lp
    return best


def judge_sample(datapoint, location_logprobs: Dict[int, float], rewrite_logprobs, assume_buggy: bool = False) -> SampleOutcome:
    """One `(datapoint, location_logprobs, rewrite_logprobs)` triple of `model.predict` -> SampleOutcome
    (reference evaluate.py:60-140)."""
    if assume_buggy:  # the "no bug" option is taken away and the rest renormalised (:61-64)
        location_logprobs = {k: v for k, v in location_logprobs.items() if k != NO_BUG_NODE}
        norm = float(torch.logsumexp(torch.tensor(list(location_logprobs.values())), dim=-1))
        location_logprobs = {k: v - norm for k, v in location_logprobs.items()}
    target = datapoint["target_fix_action_idx"]
    has_bug = target is not None
    assert has_bug or not assume_buggy
    reference_nodes = datapoint["graph"]["reference_nodes"]
    predicted_node = max(location_logprobs, key=lambda k: location_logprobs[k])
    predicted_rewrite = _best_rewrite_at(predicted_node, reference_nodes, rewrite_logprobs)
    if has_bug:
        true_node = reference_nodes[target]
        scout = datapoint["candidate_rewrite_metadata"][target][0]
        repair_given_location = _best_rewrite_at(true_node, reference_nodes, rewrite_logprobs) == target
    else:
        true_node, scout, repair_given_location = NO_BUG_NODE, "NoBug", None
    location_correct = predicted_node == true_node
    return SampleOutcome(location_logprobs[predicted_node], has_bug, predicted_node != NO_BUG_NODE, location_correct,
                         repair_given_location, location_correct and predicted_rewrite == target, scout)


def _curves_of_ranked(has_bug: np.ndarray, warned: np.ndarray, loc_ok: np.ndarray, repair_ok: np.ndarray, confidence: np.ndarray
                      ) -> Dict[str, np.ndarray]:
    """The threshold curves from boolean columns and confidences that are already in ranking order."""
    num_buggy = int(has_bug.sum())
    det_true = np.cumsum(has_bug & loc_ok)
    det_false = np.cumsum(warned & ~loc_ok)
    full_true = np.cumsum(has_bug & loc_ok & repair_ok)
    full_false = np.cumsum(warned & (~loc_ok | ~repair_ok))
    false_alarms = np.cumsum(warned & ~has_bug)
    with np.errstate(divide="ignore", invalid="ignore"):
        running = {
            "fdr": det_false / (det_true + det_false),
            "detection_precision": det_true / (det_true + det_false),
            "detection_recall": det_true / num_buggy,
            "no_bug_precision": 1 - false_alarms / (num_buggy + 1e-10),
            "precision": full_true / (full_true + full_false),
            "recall": full_true / num_buggy,
        }
    x = np.linspace(0, 1, num=CURVE_POINTS)
    prob = np.exp(confidence)
    out = {"x": x}
    for name, values in running.items():  # np.interp wants increasing abscissae: walk the ranking backwards
        out[name] = np.interp(x, prob[::-1], values[::-1], right=0)
    return out


class EvaluationReport:
    """Aggregates SampleOutcomes; `summary()` = the scalar metrics, `curves()` = the threshold curves, `format()` =
    the text the reference prints."""

    top_k: Optional[Dict[str, Any]] = None  # `_suggest.top_k_summary` of the run, when it was asked for (--top-k)

    def __init__(self, outcomes: Iterable[SampleOutcome], eval_only_no_bug: bool = False):
        self.outcomes: List[SampleOutcome] = [o for o in outcomes if not (eval_only_no_bug and o.has_bug)]

    def format_top_k(self) -> str:
        """The ranked-suggestions block printed after `format()`; empty when the run did not rank."""
        from buglab.models._suggest import format_top_k

        return "" if self.top_k is None else format_top_k(self.top_k)

    # ---- counts ---------------------------------------------------------------------------------
    def _count(self, pred) -> int:
        return sum(1 for o in self.outcomes if pred(o))

    def summary(self) -> Dict[str, float]:
        n = len(self.outcomes)
        buggy = self._count(lambda o: o.has_bug)
        correct_code = n - buggy
        warned_buggy = self._count(lambda o: o.has_bug and o.warned)
        silent_correct = self._count(lambda o: not o.has_bug and not o.warned)
        div = lambda a, b: a / b if b else float("nan")
        return {
            "num_samples": n,
            "num_buggy_samples": buggy,
            "num_repaired_correct": self._count(lambda o: o.repaired),
            "num_location_correct": self._count(lambda o: o.location_correct),
            "num_repaired_given_location_correct": self._count(lambda o: o.repair_given_location is True),
            "num_detection_correct": warned_buggy + silent_correct,
            "accuracy": div(self._count(lambda o: o.repaired), n),
            "bug_detection_accuracy": div(warned_buggy + silent_correct, n),
            "bug_detection_false_negatives": 1 - div(warned_buggy, buggy),
            "bug_detection_false_positives": 1 - div(silent_correct, correct_code),
            "localization_accuracy": div(self._count(lambda o: o.location_correct), n),
            "repair_accuracy_given_location": div(self._count(lambda o: o.repair_given_location is True), buggy),
            # kept from the first version of this module
            "repair_accuracy": div(self._count(lambda o: o.repaired and o.has_bug), buggy),
            "bug_detection_recall": div(warned_buggy, buggy),
            "no_bug_precision": div(silent_correct, correct_code),
        }

    def per_scout(self) -> Dict[str, Dict[str, List[int]]]:
        """{"localization" | "repair": {scout: [correct, total]}}; repair counts buggy samples only (:104-108,114-118)."""
        loc, rep = defaultdict(lambda: [0, 0]), defaultdict(lambda: [0, 0])
        for o in self.outcomes:
            loc[o.scout][0] += int(o.location_correct)
            loc[o.scout][1] += 1
            if o.has_bug:
                rep[o.scout][0] += int(bool(o.repair_given_location))
                rep[o.scout][1] += 1
        return {"localization": dict(sorted(loc.items())), "repair": dict(sorted(rep.items()))}

    # ---- threshold curves -------------------------------------------------------------------------
    def curves(self) -> Dict[str, np.ndarray]:
        """Samples ordered by decreasing confidence; every curve is a running ratio over that order, resampled at
        CURVE_POINTS probability thresholds in [0, 1] (:186-255).  Kept as the reference has it: a warning counts as
        false for the detect-and-repair curves when the rewrite at the TRUE location is wrong, and a warning on
        correct code counts as a wrong location; NO_BUG precision is 1 - false alarms / (number of buggy samples)."""
        ranked = sorted(self.outcomes, key=lambda o: tuple(o[:5]), reverse=True)
        col = lambda f: np.array([f(o) for o in ranked], dtype=bool)
        return _curves_of_ranked(col(lambda o: o.has_bug), col(lambda o: o.warned), col(lambda o: o.location_correct),
                                 col(lambda o: bool(o.repair_given_location)), np.array([o.confidence for o in ranked]))

    # ---- text -------------------------------------------------------------------------------------
    def format(self) -> str:
        s, scouts = self.summary(), self.per_scout()
        n, buggy = s["num_samples"], s["num_buggy_samples"]
        bar, lines = "=" * 34, []
        add = lines.append
        add(bar)
        add(f"Accuracy (Localization & Repair) {s['accuracy']:.2%} ({s['num_repaired_correct']}/{n})")
        add(f"Bug Detection Accuracy (no Localization or Repair) {s['bug_detection_accuracy']:.2%} ({s['num_detection_correct']}/{n})")
        fn = f"{s['bug_detection_false_negatives']:.2%}" if buggy > 0 else "NaN (0/0)"
        fp = f"{s['bug_detection_false_positives']:.2%}" if n - buggy > 0 else "NaN (0/0)"
        add(f"Bug Detection (no Localization or Repair) False Negatives: {fn}")
        add(f"Bug Detection (no Localization or Repair) False Positives: {fp}")
        add(bar)
        add(f"Localization Accuracy {s['localization_accuracy']:.2%} ({s['num_location_correct']}/{n})")
        for scout, (ok, total) in scouts["localization"].items():
            add(f"\t{scout}: {ok / total:.1%}  ({ok}/{total})")
        add("=" * 41)
        if buggy == 0:
            add("--eval-only-no-bug is True. Repair Accuracy Given Location cannot be computed.")
        else:
            add(f"Repair Accuracy Given Location {s['repair_accuracy_given_location']:.2%}  ({s['num_repaired_given_location_correct']}/{buggy})")
        for scout, (ok, total) in scouts["repair"].items():
            add(f"\t{scout}: {ok / total:.1%}  ({ok}/{total})")
        c = self.curves()
        add("x = np." + repr(c["x"]))
        for title, name in (("False Detection Rate", "fdr"), ("Detection Precision", "detection_precision"),
                            ("Detection Recall", "detection_recall"), ("Detection NO_BUG Precision", "no_bug_precision"),
                            ("Precision (Detect and Repair)", "precision"), ("Recall (Detect and Repair)", "recall")):
            add(f"### {title} ###")
            add(f"{name} = np." + repr(c[name]))
        return "\n".join(lines) + "\n"


def evaluate_predictions(predictions, assume_buggy: bool = False, eval_only_no_bug: bool = False, top_k: Optional[int] = None
                         ) -> EvaluationReport:
    """`predictions` = what `model.predict` yields.  With `eval_only_no_bug` the buggy samples are skipped before
    anything is computed for them (:69-70).  With `top_k` every judged sample is also ranked (`suggestions_of_prediction`) and
    the report carries `top_k_summary` of the ranks."""
    from buglab.models import _suggest as S

    if top_k is not None:
        top_k = _checked_top_k(top_k)
    outcomes, ranks = [], []
    for datapoint, location_logprobs, rewrite_logprobs in predictions:
        if eval_only_no_bug and datapoint["target_fix_action_idx"] is not None:
            continue
        outcomes.append(judge_sample(datapoint, location_logprobs, rewrite_logprobs, assume_buggy))
        if top_k is not None:  # the ranks do not depend on how many entries are listed
            ranked = S.suggestions_of_prediction(datapoint, location_logprobs, rewrite_logprobs, 1, assume_buggy)
            ranks.append((ranked.truth_rank, ranked.truth_location_rank))
    report = EvaluationReport(outcomes)
    if top_k is not None:
        names = ["NoBug"] + sorted({o.scout for o in outcomes} - {"NoBug"})
        ids = {name: i for i, name in enumerate(names)}
        columns = np.asarray(ranks, dtype=np.int32).reshape(-1, 2)
        report.top_k = S.top_k_summary(columns[:, 0], columns[:, 1], [o.has_bug for o in outcomes], [ids[o.scout] for o in outcomes],
                                       names, top_k)
    return report


def _checked_top_k(top_k) -> int:
    from buglab.models._suggest import MAX_K

    if not 1 <= int(top_k) <= MAX_K:
        raise ValueError(f"--top-k must be in [1, {MAX_K}] (got {top_k})")
    return int(top_k)


class ColumnarEvaluationReport(EvaluationReport):
    """The same report from outcome COLUMNS (one NumPy array per SampleOutcome field) instead of a list of tuples: what
    `evaluate_on_device` copies back.  `repair_given_location`: 1 / 0, -1 = the host's None (no bug); `scout`: ids into
    `scout_names`, where id 0 is "NoBug".  Counts and curves are vectorised; `format()` is inherited, so the text is the host
    path's text."""

    def __init__(self, confidence, has_bug, warned, location_correct, repair_given_location, repaired, scout,
                 scout_names: Sequence[str] = ("NoBug",), eval_only_no_bug: bool = False):
        has_bug = np.asarray(has_bug, dtype=bool)
        keep = ~has_bug if eval_only_no_bug else np.ones(has_bug.shape[0], dtype=bool)
        self.confidence = np.asarray(confidence, dtype=np.float64)[keep]
        self.has_bug = has_bug[keep]
        self.warned = np.asarray(warned, dtype=bool)[keep]
        self.location_correct = np.asarray(location_correct, dtype=bool)[keep]
        self.repair_given_location = np.asarray(repair_given_location, dtype=np.int8)[keep]
        self.repaired = np.asarray(repaired, dtype=bool)[keep]
        self.scout = np.asarray(scout, dtype=np.int64)[keep]
        self.scout_names = list(scout_names)
        assert self.scout_names and self.scout_names[0] == "NoBug"
        assert all(c.shape == self.confidence.shape for c in (self.has_bug, self.warned, self.location_correct,
                                                                self.repair_given_location, self.repaired, self.scout))

    @classmethod
    def from_outcomes(cls, outcomes: Iterable[SampleOutcome], eval_only_no_bug: bool = False) -> "ColumnarEvaluationReport":
        outcomes = list(outcomes)
        names = ["NoBug"] + sorted({o.scout for o in outcomes} - {"NoBug"})
        ids = {n: i for i, n in enumerate(names)}
        return cls([o.confidence for o in outcomes], [o.has_bug for o in outcomes], [o.warned for o in outcomes],
                   [o.location_correct for o in outcomes], [-1 if o.repair_given_location is None else int(o.repair_given_location)
                                                            for o in outcomes],
                   [o.repaired for o in outcomes], [ids[o.scout] for o in outcomes], names, eval_only_no_bug)

    @property
    def outcomes(self) -> List[SampleOutcome]:
        rgl = [None if r < 0 else bool(r) for r in self.repair_given_location.tolist()]
        return [SampleOutcome(*t) for t in zip(self.confidence.tolist(), self.has_bug.tolist(), self.warned.tolist(),
                                               self.location_correct.tolist(), rgl, self.repaired.tolist(),
                                               (self.scout_names[i] for i in self.scout.tolist()))]

    def summary(self) -> Dict[str, float]:
        count = lambda mask: int(np.count_nonzero(mask))
        n = int(self.confidence.shape[0])
        buggy = count(self.has_bug)
        correct_code = n - buggy
        warned_buggy = count(self.has_bug & self.warned)
        silent_correct = count(~self.has_bug & ~self.warned)
        repaired, located, repair_ok = count(self.repaired), count(self.location_correct), count(self.repair_given_location == 1)
        div = lambda a, b: a / b if b else float("nan")
        return {
            "num_samples": n,
            "num_buggy_samples": buggy,
            "num_repaired_correct": repaired,
            "num_location_correct": located,
            "num_repaired_given_location_correct": repair_ok,
            "num_detection_correct": warned_buggy + silent_correct,
            "accuracy": div(repaired, n),
            "bug_detection_accuracy": div(warned_buggy + silent_correct, n),
            "bug_detection_false_negatives": 1 - div(warned_buggy, buggy),
            "bug_detection_false_positives": 1 - div(silent_correct, correct_code),
            "localization_accuracy": div(located, n),
            "repair_accuracy_given_location": div(repair_ok, buggy),
            "repair_accuracy": div(count(self.repaired & self.has_bug), buggy),
            "bug_detection_recall": div(warned_buggy, buggy),
            "no_bug_precision": div(silent_correct, correct_code),
        }

    def per_scout(self) -> Dict[str, Dict[str, List[int]]]:
        k = len(self.scout_names)

        def table(rows, ok):
            total = np.bincount(self.scout[rows], minlength=k)
            good = np.bincount(self.scout[rows & ok], minlength=k)
            return {name: [int(good[i]), int(total[i])] for name, i in sorted((n, i) for i, n in enumerate(self.scout_names)) if total[i]}

        everything = np.ones(self.scout.shape[0], dtype=bool)
        return {"localization": table(everything, self.location_correct), "repair": table(self.has_bug, self.repair_given_location == 1)}

    def curves(self) -> Dict[str, np.ndarray]:
        # the descending stable sort of (confidence, has_bug, warned, location_correct, repair_given_location) the host path does
        # on tuples; np.lexsort takes its LAST key first.  None only ever meets None there (has_bug is compared before it).
        neg = lambda c: -c.astype(np.int8)
        order = np.lexsort((neg(self.repair_given_location), neg(self.location_correct), neg(self.warned), neg(self.has_bug),
                            -self.confidence))
        return _curves_of_ranked(self.has_bug[order], self.warned[order], self.location_correct[order],
                                 self.repair_given_location[order] == 1, self.confidence[order])


def evaluate_on_device(model, nn, data: Iterable[Any], device, *, assume_buggy: bool = False, eval_only_no_bug: bool = False,
                       parallelize: bool = True, positions_out: Optional[list] = None, top_k: Optional[int] = None,
                       capacity: Optional[int] = None) -> ColumnarEvaluationReport:
    """`evaluate_predictions(model.predict(data, nn, device, parallelize), ...)` without the per-sample host work: the
    minibatches `predict` forms (same `tensorize`, same 50 samples), the same forward, and one hip_ops.eval_judge launch per
    minibatch that writes the verdicts into outcome buffers kept on the device until the end (24 bytes per sample, one copy
    back).  `has_bug` and the scout names never go to the device.  With `eval_only_no_bug` every sample still runs, as in
    `predict`, so that a sequence model's minibatches -- and with them its fp32 values -- are those of the host path; the buggy
    samples are left out of the report.  Single models only: an ensemble keeps the host path.  `positions_out`, when given,
    receives the position in `data` of every judged sample, in the order of the outcome columns before `eval_only_no_bug`
    (a datapoint `tensorize` rejects has none): what buglab/models/compare.py pairs two models' samples by.  With `top_k` one
    hip_ops.rank_suggestions launch follows each judge launch, on index arrays that extend the judge's by two, and writes the
    ranks of the true fix and the true location into columns of the same allocation (the ranks do not depend on how many entries
    are listed, so one is); the report carries `top_k_summary`.  `capacity`: the samples the buffers (`RunColumns`) start with,
    by default `len(data)`, or 1 << 14 for a stream."""
    from buglab.controllers import _batching as Bt
    from buglab.models import _evaluate as E
    from buglab.models import _suggest as S
    from buglab.models import hip_ops

    Bt.require_single_model(model, "evaluate_on_device")
    if top_k is not None:
        top_k = _checked_top_k(top_k)
    index_fields = hip_ops.EVAL_INDEX_FIELDS if top_k is None else hip_ops.SUGGEST_INDEX_FIELDS  # (the second holds the first)
    device = torch.device(device)
    names, ids = ["NoBug"], {"NoBug": 0}
    has_bug: List[bool] = []
    scout: List[int] = []

    def extend(layout, points, dev, mb):
        ix = (E.eval_indices if top_k is None else S.suggest_indices)(layout, points, mb.get("node_mappings"))
        if assume_buggy:
            E.check_assume_buggy(ix)
        targets = [p["target_fix_action_idx"] for p in points]
        scouts = ["NoBug" if t is None else p["candidate_rewrite_metadata"][t][0] for p, t in zip(points, targets)]
        return {"ix": dict(zip(index_fields, Bt.to_device_i32([getattr(ix, f) for f in index_fields], dev))), "scouts": scouts}

    spec = [("confidence", "float64", (Bt.SAMPLES,)), ("verdict", "int32", (4, Bt.SAMPLES))]
    if top_k is not None:  # the two rank rows, one listed entry and its log-probability
        spec += [("rank", "int32", (2, Bt.SAMPLES)), ("entry", "int32", (Bt.SAMPLES, 1)), ("logprob", "float64", (Bt.SAMPLES, 1))]
    cols = Bt.RunColumns(device, Bt.run_capacity(capacity, data, 1 << 14), spec)
    nn.eval()
    with torch.no_grad(), model._tensorize_all_location_rewrites():
        for mb, tags in Bt.prediction_minibatches(model, ((d, i) for i, d in enumerate(data)), device, parallelize, extend,
                                                  lambda tag: None, extend_sees_minibatch=True):
            flat = Bt.flat_prediction_output(nn, mb)
            B = len(mb["selfsup"]["scouts"])
            if positions_out is not None:
                assert len(tags) == B
                positions_out.extend(tags)
            n = cols.reserve(B)
            hip_ops.eval_judge(flat, mb["selfsup"]["ix"], cols["confidence"], cols["verdict"], n, assume_buggy=assume_buggy)
            if top_k is not None:
                hip_ops.rank_suggestions(flat, mb["selfsup"]["ix"], cols["rank"], cols["entry"], cols["logprob"], n, k=1,
                                         skip_nobug=assume_buggy)
            for name in mb["selfsup"]["scouts"]:
                has_bug.append(name != "NoBug")
                scout.append(ids.setdefault(name, len(ids)))
                if scout[-1] == len(names):
                    names.append(name)
    host = cols.to_host()  # the one copy (and the one synchronisation) of the run
    verdict = host["verdict"]
    report = ColumnarEvaluationReport(host["confidence"], has_bug, verdict[0] != 0, verdict[1] != 0, verdict[2], verdict[3] != 0, scout,
                                      names, eval_only_no_bug)
    if top_k is not None:
        keep = ~np.asarray(has_bug, dtype=bool) if eval_only_no_bug else np.ones(cols.n, dtype=bool)
        report.top_k = S.top_k_summary(host["rank"][0][keep], host["rank"][1][keep], report.has_bug, report.scout, names, top_k)
    return report


def at_operating_point(report: EvaluationReport, point) -> Dict[str, Any]:
    """What the report's samples give when a warning is shown only at or above `point.threshold_logprob` (an `OperatingPoint` of
    buglab/models/operatingpoint.py): the five counts of the threshold curves there (`curve_counts_point` with that one
    threshold), the warnings raised, and the precisions and recalls by the formulas of `_curves_of_ranked`."""
    from buglab.models import _operatingpoint as P

    columns = report if isinstance(report, ColumnarEvaluationReport) else ColumnarEvaluationReport.from_outcomes(report.outcomes)
    out: Dict[str, Any] = {"threshold_logprob": float(point.threshold_logprob), "num_samples": int(columns.confidence.shape[0])}
    if columns.confidence.shape[0] == 0:
        counts = np.zeros((1, P.num_columns(1, 1)), np.int32)
    else:
        packed, _, _ = P.pack_outcomes([columns])
        counts = P.curve_counts_point(packed, P.bin_of(columns.confidence, [point.threshold_logprob])[None, :], 1, 1)
    out["num_buggy_samples"] = int(counts[0, 0])
    out.update({name: int(counts[0, 1 + c]) for c, name in enumerate(P.COUNTERS)})
    out["num_warnings"] = out["det_true"] + out["det_false"]
    curves = P.curves_from_counts(counts, 1, 1)
    out.update({name: float(curves[name][0, 0, 0]) for name in ("detection_precision", "precision", "detection_recall", "recall")})
    return out


def format_at_operating_point(at: Dict[str, Any]) -> str:
    pct = lambda x: "NaN" if x != x else f"{x:.2%}"
    return "\n".join([
        "=" * 34,
        f"At the warning operating point (probability >= {math.exp(at['threshold_logprob']):.6f}): {at['num_warnings']} warnings "
        f"on {at['num_samples']} samples",
        f"Detection Precision {pct(at['detection_precision'])} ({at['det_true']}/{at['det_true'] + at['det_false']})",
        f"Precision (Detect and Repair) {pct(at['precision'])} ({at['full_true']}/{at['full_true'] + at['full_false']})",
        f"Detection Recall {pct(at['detection_recall'])} ({at['det_true']}/{at['num_buggy_samples']})",
        f"Recall (Detect and Repair) {pct(at['recall'])} ({at['full_true']}/{at['num_buggy_samples']})",
    ]) + "\n"


def report_to_json(report: EvaluationReport, at: Optional[Dict[str, Any]] = None) -> str:
    """summary, per-scout tables and curves as data (NaN where the text says NaN); with `at` (`at_operating_point`), that too."""
    blob = {"summary": report.summary(), "per_scout": report.per_scout(), "curves": {k: v.tolist() for k, v in report.curves().items()}}
    if at is not None:
        blob["at_operating_point"] = at
    if report.top_k is not None:
        blob["top_k"] = report.top_k
    return json.dumps(blob, indent=1, sort_keys=True) + "\n"


def run(arguments):
    data_path = RichPath.create(arguments["TEST_DATA_PATH"])
    lim = None if arguments["--limit-num-elements"] is None else int(arguments["--limit-num-elements"])
    data = load_all_msgpack_l_gz(data_path, shuffle=True, limit_num_yielded_elements=lim)
    require_gpu(None, "evaluate.py")
    model, nn, device, _ = open_model(arguments["MODEL_FILENAME"])
    top_k = None if arguments.get("--top-k") is None else _checked_top_k(arguments["--top-k"])
    if arguments.get("--on-device"):
        report = evaluate_on_device(model, nn, data, device, assume_buggy=arguments["--assume-buggy"],
                                    eval_only_no_bug=arguments["--eval-only-no-bug"], parallelize=not arguments["--sequential"],
                                    top_k=top_k)
    else:
        predictions = model.predict(data, nn, device, parallelize=not arguments["--sequential"])
        report = evaluate_predictions(predictions, arguments["--assume-buggy"], arguments["--eval-only-no-bug"], top_k)
    sys.stdout.write(report.format())
    sys.stdout.write(report.format_top_k())
    at = None
    if arguments.get("--at-operating-point"):
        if getattr(model, "warning_operating_point", None) is None:
            raise ValueError("--at-operating-point: the checkpoint carries no warning operating point; fit one with "
                             "python -m buglab.models.operatingpoint")
        at = at_operating_point(report, model.warning_operating_point)
        sys.stdout.write(format_at_operating_point(at))
    if arguments.get("--report-json") is not None:
        with open(arguments["--report-json"], "w", encoding="utf-8") as f:
            f.write(report_to_json(report, at))
    return report.summary()


if __name__ == "__main__":
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("MODEL_FILENAME")
    p.add_argument("TEST_DATA_PATH")
    p.add_argument("--assume-buggy", action="store_true")
    p.add_argument("--eval-only-no-bug", action="store_true")
    p.add_argument("--limit-num-elements", default=None)
    p.add_argument("--sequential", action="store_true")
    p.add_argument("--on-device", action="store_true")
    p.add_argument("--report-json", default=None)
    p.add_argument("--at-operating-point", action="store_true")
    p.add_argument("--top-k", default=None, type=int)
    p.add_argument("--minibatch-size", default=300)
    p.add_argument("--restore-path", default=None)
    p.add_argument("--quiet", action="store_true")
    p.add_argument("--debug", action="store_true")
    ns = p.parse_args()
    run({"MODEL_FILENAME": ns.MODEL_FILENAME, "TEST_DATA_PATH": ns.TEST_DATA_PATH, "--assume-buggy": ns.assume_buggy,
         "--eval-only-no-bug": ns.eval_only_no_bug, "--limit-num-elements": ns.limit_num_elements, "--sequential": ns.sequential,
         "--on-device": ns.on_device, "--report-json": ns.report_json, "--at-operating-point": ns.at_operating_point,
         "--top-k": ns.top_k})
