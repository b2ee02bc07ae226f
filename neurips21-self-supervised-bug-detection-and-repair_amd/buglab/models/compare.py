#!/usr/bin/env python
"""
Usage:
    python -m buglab.models.compare DATA MODEL [MODEL ...] [--num-replicates 10000] [--seed 0] [--confidence 0.95]
                                    [--limit-num-elements N] [--sequential] [--assume-buggy] [--eval-only-no-bug]
                                    [--host-bootstrap] [--report-json FILE] [--curves [--max-bins G]]

Paired bootstrap comparison of trained models -- BEYOND THE REFERENCE, which has no counterpart: its evaluate.py prints point
estimates such as "Accuracy (Localization & Repair) 71.30% (1426/2000)" and nothing that says whether a second model's 72.1% is
better or noise.  This evaluates every MODEL (the first is the baseline) on the same samples in the same order, keeps what
each sample contributed (the verdicts of evaluate.py's `judge_sample`), and resamples the samples with replacement: every
metric of the evaluation report gets a percentile interval, every metric's difference against the baseline an interval and a
two-sided p-value over the SAME draws, and `repaired` an exact McNemar test.

Evaluation: the data is read once, in file order (no shuffle); a single model is judged on the device (`evaluate_on_device`,
csrc/bl_evaluate.hip), an ensemble file through `predict` on the host path, which the on-device path refuses.  `predict`
leaves out a sample a model's `tensorize` rejects (a sequence model and a sample beyond its `max_seq_size`): each datapoint's
position travels with it, the paired set is the intersection of the positions every model kept, and the report says how many
samples each model dropped.  `--eval-only-no-bug` is applied after pairing.

Resampling: the verdicts of all models are packed into one uint32 per sample (buglab/models/_compare.py::pack_outcomes) that
goes to the device once; hip_ops.bootstrap_counts (csrc/bl_bootstrap.hip) counts at most 4096 replicates per call, and the
counts come back once per call.  `--host-bootstrap` has the NumPy twin produce the same counts, bit for bit; everything after
the counts is the same code.  The draws are splitmix64 of a counter (the contract is in include/buglab_hip.h): a result depends
on the seed alone, not on the device, the grid or the call size.  The multiply-shift that maps a 32-bit hash to a sample
position has a relative bias below n / 2^32.
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path
from typing import Any, Dict, List, Optional, Sequence, Tuple

if __package__ in (None, ""):
    sys.path.insert(0, str(Path(__file__).resolve().parents[2]))

import numpy as np

from buglab.models import _compare as C
from buglab.models._compare import ComparisonReport

REPLICATES_PER_CALL = 4096  # bounds the device's output buffer: 4096 x C int32


def bootstrap_counts_device(packed: np.ndarray, M: int, K: int, seed: int, num_replicates: int, device) -> np.ndarray:
    """The counts of replicates 0 .. num_replicates - 1 from the device, int32 [R, C]: the words go up once, the counts come
    back once per call of at most REPLICATES_PER_CALL replicates."""
    import torch

    from buglab.models import hip_ops

    words = torch.from_numpy(np.ascontiguousarray(packed, dtype=np.uint32).view(np.int32)).to(device)
    counts = np.empty((num_replicates, C.num_columns(M, K)), np.int32)
    buffer = torch.empty((min(num_replicates, REPLICATES_PER_CALL), C.num_columns(M, K)), dtype=torch.int32, device=words.device)
    for r0 in range(0, num_replicates, REPLICATES_PER_CALL):
        R = min(REPLICATES_PER_CALL, num_replicates - r0)
        counts[r0:r0 + R] = hip_ops.bootstrap_counts(words, M, K, seed, r0, R, out=buffer).cpu().numpy()
    return counts


def compare_reports(reports: Sequence[Any], *, num_replicates: int = 10000, seed: int = 0, confidence: float = 0.95,
                    host_bootstrap: bool = False, device=None, names: Optional[Sequence[str]] = None,
                    models: Optional[List[Dict[str, Any]]] = None, curves: bool = False, max_bins: int = 256) -> ComparisonReport:
    """`reports`: M `ColumnarEvaluationReport`s over the same samples in the same order, the baseline first.  The counts come
    from `device` (hip_ops.bootstrap_counts) or, with `host_bootstrap`, from the NumPy twin.  `curves`: the report also
    carries, per model, the bands of its six threshold curves at up to `max_bins` thresholds of its own
    (buglab/models/operatingpoint.py::report_curve_bands), over the same seed and replicate numbers."""
    if num_replicates < 1:
        raise ValueError(f"num_replicates must be at least 1 (got {num_replicates})")
    packed, K, scout_names = C.pack_outcomes(reports)
    if packed.shape[0] == 0:
        raise ValueError("compare: the paired set is empty: there is no sample every model kept")
    M = len(reports)
    names = list(names) if names is not None else [f"model_{m}" for m in range(M)]
    if len(names) != M:
        raise ValueError(f"compare: {len(names)} names for {M} models")
    if host_bootstrap:
        counts = C.bootstrap_counts_host(packed, M, K, seed, 0, int(num_replicates))
    else:
        counts = bootstrap_counts_device(packed, M, K, seed, int(num_replicates), "cuda" if device is None else device)
    report = C.summarize(packed, M, K, counts, names=names, scout_names=scout_names, seed=seed, confidence=confidence, models=models)
    if curves:
        from buglab.models.operatingpoint import report_curve_bands

        report.curve_bands = report_curve_bands(reports, num_replicates=int(num_replicates), seed=seed, confidence=confidence,
                                                max_bins=max_bins, device=device, host_bootstrap=host_bootstrap)
    return report


def _rows_of(report, rows: np.ndarray):
    from buglab.models.evaluate import ColumnarEvaluationReport

    return ColumnarEvaluationReport(report.confidence[rows], report.has_bug[rows], report.warned[rows], report.location_correct[rows],
                                    report.repair_given_location[rows], report.repaired[rows], report.scout[rows], report.scout_names)


def evaluate_with_positions(model, nn, data: List[Any], device, *, assume_buggy: bool = False, parallelize: bool = True
                            ) -> Tuple[Any, List[int]]:
    """-> (the model's `ColumnarEvaluationReport` over the samples it kept, their positions in `data`, in column order).  A
    single model is judged on the device; an `EnsembleWrapper` goes through `predict` on the host path and its datapoints are
    matched back by identity."""
    from buglab.models.ensemble.wrapper import EnsembleWrapper
    from buglab.models.evaluate import ColumnarEvaluationReport, evaluate_on_device, evaluate_predictions

    positions: List[int] = []
    if not isinstance(model, EnsembleWrapper):
        report = evaluate_on_device(model, nn, data, device, assume_buggy=assume_buggy, parallelize=parallelize, positions_out=positions)
        return report, positions
    position_of = {id(d): i for i, d in enumerate(data)}

    def tap(predictions):
        for datapoint, location_logprobs, rewrite_logprobs in predictions:
            positions.append(position_of[id(datapoint)])
            yield datapoint, location_logprobs, rewrite_logprobs

    host = evaluate_predictions(tap(model.predict(iter(data), nn, device, parallelize)), assume_buggy)
    return ColumnarEvaluationReport.from_outcomes(host.outcomes), positions


def paired_reports(evaluated: Sequence[Tuple[Any, List[int]]], num_samples: int, eval_only_no_bug: bool = False
                   ) -> Tuple[List[Any], np.ndarray, List[int]]:
    """Every model's report restricted to the positions all of them kept, in position order -> (reports, the positions, the
    number of samples each model dropped).  `eval_only_no_bug` leaves out the buggy samples AFTER pairing."""
    common = None
    for _, positions in evaluated:
        if len(set(positions)) != len(positions):
            raise ValueError("compare: a model yielded a sample twice")
        common = set(positions) if common is None else common & set(positions)
    kept = np.array(sorted(common), dtype=np.int64)
    dropped = [num_samples - len(positions) for _, positions in evaluated]
    out = []
    for report, positions in evaluated:
        row_of = np.full(num_samples, -1, np.int64)
        row_of[np.asarray(positions, dtype=np.int64)] = np.arange(len(positions))
        out.append(_rows_of(report, row_of[kept]))
    if eval_only_no_bug and kept.size:
        clean = ~out[0].has_bug
        kept, out = kept[clean], [_rows_of(r, np.flatnonzero(clean)) for r in out]
    if kept.size == 0:
        raise ValueError("compare: the paired set is empty: there is no sample every model kept")
    return out, kept, dropped


def compare_models(models: Sequence[Tuple[Any, Any]], data, device, *, num_replicates: int = 10000, seed: int = 0,
                   confidence: float = 0.95, assume_buggy: bool = False, eval_only_no_bug: bool = False, parallelize: bool = True,
                   host_bootstrap: bool = False, names: Optional[Sequence[str]] = None, curves: bool = False, max_bins: int = 256
                   ) -> ComparisonReport:
    """`models`: (model, nn) pairs, the baseline first; `data`: the datapoints, read once into a list that every model sees in
    that order."""
    if not 1 <= len(models) <= C.MAX_MODELS:
        raise ValueError(f"compare: {len(models)} models; a comparison takes 1 to {C.MAX_MODELS} (BL_BOOTSTRAP_MAX_MODELS)")
    data = data if isinstance(data, list) else list(data)
    names = list(names) if names is not None else [f"model_{m}" for m in range(len(models))]
    evaluated = [evaluate_with_positions(model, nn, data, device, assume_buggy=assume_buggy, parallelize=parallelize)
                 for model, nn in models]
    reports, _, dropped = paired_reports(evaluated, len(data), eval_only_no_bug)
    info = [{"name": name, "num_samples": len(data), "num_dropped": d} for name, d in zip(names, dropped)]
    return compare_reports(reports, num_replicates=num_replicates, seed=seed, confidence=confidence, host_bootstrap=host_bootstrap,
                           device=device, names=names, models=info, curves=curves, max_bins=max_bins)


def parse_args(argv=None) -> argparse.Namespace:
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("DATA", help="`*.msgpack.l.gz` test data: a file or a folder.")
    p.add_argument("MODEL", nargs="+", help="Trained checkpoints or ensemble files (`*.pkl.gz`); the first is the baseline.")
    p.add_argument("--num-replicates", type=int, default=10000, help="Bootstrap replicates.")
    p.add_argument("--seed", type=int, default=0, help="Seed of the draws.")
    p.add_argument("--confidence", type=float, default=0.95, help="Coverage of the percentile intervals.")
    p.add_argument("--limit-num-elements", type=int, default=None, help="Compare on at most this many samples.")
    p.add_argument("--sequential", action="store_true", help="Do not parallelize data loading.")
    p.add_argument("--assume-buggy", action="store_true", help="Never predict NO_BUG.")
    p.add_argument("--eval-only-no-bug", action="store_true", help="Compare on the NO_BUG samples only (applied after pairing).")
    p.add_argument("--host-bootstrap", action="store_true", help="Resample with the NumPy twin instead of the device kernel.")
    p.add_argument("--report-json", default=None, help="Also write the report as data.")
    p.add_argument("--curves", action="store_true",
                   help="--report-json also gets, per model, the bands of its six threshold curves (the printed text gains nothing).")
    p.add_argument("--max-bins", type=int, default=256, help="Thresholds per model of --curves, at most 1024.")
    return p.parse_args(argv)


def run(args: argparse.Namespace) -> ComparisonReport:
    import torch

    from buglab.models._cli import open_model, read_data, require_gpu

    require_gpu(None, "compare")
    if len(args.MODEL) > C.MAX_MODELS:
        raise ValueError(f"compare: {len(args.MODEL)} models; a comparison takes 1 to {C.MAX_MODELS} (BL_BOOTSTRAP_MAX_MODELS)")
    device = torch.device("cuda")
    data = read_data(args.DATA, args.limit_num_elements)
    models = [open_model(name)[:2] for name in args.MODEL]
    report = compare_models(models, data, device, num_replicates=args.num_replicates, seed=args.seed, confidence=args.confidence,
                            assume_buggy=args.assume_buggy, eval_only_no_bug=args.eval_only_no_bug, parallelize=not args.sequential,
                            host_bootstrap=args.host_bootstrap, names=[str(name) for name in args.MODEL], curves=args.curves,
                            max_bins=args.max_bins)
    sys.stdout.write(report.format())
    if args.report_json is not None:
        with open(args.report_json, "w", encoding="utf-8") as f:
            f.write(report.to_json())
    return report


if __name__ == "__main__":
    run(parse_args())
