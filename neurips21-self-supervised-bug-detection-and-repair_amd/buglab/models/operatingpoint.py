#!/usr/bin/env python
"""
Usage:
    python -m buglab.models.operatingpoint MODEL VALID_DATA OUT_MODEL --target-precision P [--curve precision|detection_precision]
                                           [--confidence 0.95] [--num-replicates 2000] [--seed 0] [--max-bins 256]
                                           [--min-warnings 20] [--limit-num-elements N] [--sequential] [--host-bootstrap]
                                           [--report-json FILE]

Warning operating points -- BEYOND THE REFERENCE, whose evaluate.py prints the six threshold curves as point estimates and
leaves the reader to pick a threshold by eye.  This answers what a deployment asks first: at which confidence is a warning
shown, and how sure is the precision there?  It evaluates MODEL on held-out data (`evaluate_on_device`, so a checkpoint's
confidence calibration is in effect), fixes at most --max-bins candidate thresholds (the distinct confidences of the warned
samples, evenly spaced by rank), bootstraps the threshold curves over the samples, and chooses the LOWEST threshold whose
precision has a one-sided lower confidence bound of at least --target-precision and that raises at least --min-warnings
warnings: the highest recall at which the precision claim still holds.  OUT_MODEL is MODEL with `warning_operating_point` set;
`visualize --at-operating-point` and `evaluate --at-operating-point` read it.  When no threshold qualifies, the best lower
bound reached and its threshold are printed, nothing is written and the exit status is 2.

Resampling: every sample carries the index of the first threshold it passes (buglab/models/_operatingpoint.py), so a replicate
is a histogram and a prefix sum, not a ranking: hip_ops.bootstrap_curve_counts (csrc/bl_bootstrap.hip), one workgroup per
replicate, over the draws of buglab/models/compare.py's bootstrap (the contract is in include/buglab_hip.h).
`--host-bootstrap` has the NumPy twin produce the same counts, bit for bit; everything after the counts is the same code.
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path
from typing import Any, Dict, Iterable, List, Optional, Sequence

if __package__ in (None, ""):
    sys.path.insert(0, str(Path(__file__).resolve().parents[2]))

import numpy as np

from buglab.models import _compare as C
from buglab.models import _operatingpoint as P
from buglab.models._operatingpoint import OperatingPoint

REPLICATES_PER_CALL = 4096     # as compare.py
OUTPUT_BUFFER_INTS = 1 << 24   # and at most 64 MB of counts per call: a row has 1 + 5 M G columns
TABLE_ROWS = 10
EXIT_NOTHING_QUALIFIES = 2


def replicates_per_call(M: int, G: int) -> int:
    return max(1, min(REPLICATES_PER_CALL, OUTPUT_BUFFER_INTS // P.num_columns(M, G)))


def curve_counts_device(packed: np.ndarray, bins: np.ndarray, M: int, G: int, seed: int, num_replicates: int, device) -> np.ndarray:
    """The curve counts of replicates 0 .. num_replicates - 1 from the device, int32 [R, 1 + 5 M G]: the words and bins go up
    once, the counts come back once per call."""
    import torch

    from buglab.models import hip_ops

    words = torch.from_numpy(np.ascontiguousarray(packed, dtype=np.uint32).view(np.int32)).to(device)
    d_bins = torch.from_numpy(np.ascontiguousarray(bins, dtype=np.int16)).to(device)
    cols, per_call = P.num_columns(M, G), replicates_per_call(M, G)
    counts = np.empty((num_replicates, cols), np.int32)
    buffer = torch.empty((min(num_replicates, per_call), cols), dtype=torch.int32, device=words.device)
    for r0 in range(0, num_replicates, per_call):
        R = min(per_call, num_replicates - r0)
        counts[r0:r0 + R] = hip_ops.bootstrap_curve_counts(words, d_bins, M, G, seed, r0, R, out=buffer).cpu().numpy()
    return counts


def curve_counts(packed: np.ndarray, bins: np.ndarray, M: int, G: int, seed: int, num_replicates: int, device=None,
                 host_bootstrap: bool = False) -> np.ndarray:
    """From `device` (hip_ops.bootstrap_curve_counts) or, with `host_bootstrap` or a device that is not a GPU, from the twin."""
    if not host_bootstrap and device is not None:
        import torch

        host_bootstrap = torch.device(device).type != "cuda"
    if host_bootstrap:
        return P.curve_counts_host(packed, bins, M, G, seed, 0, int(num_replicates))
    return curve_counts_device(packed, bins, M, G, seed, int(num_replicates), "cuda" if device is None else device)


def report_curve_bands(reports: Sequence[Any], *, num_replicates: int, seed: int, confidence: float = 0.95, max_bins: int = 256,
                       device=None, host_bootstrap: bool = False) -> List[Dict[str, Any]]:
    """Per model of a comparison (M `ColumnarEvaluationReport`s over the same samples) the bands of its six curves on its OWN
    grid, over the draws of the comparison's scalar metrics (same seed, same replicate numbers), as data."""
    packed, _, _ = C.pack_outcomes(reports)
    M = len(reports)
    grids = [P.curve_grid(r.confidence, r.warned, max_bins) for r in reports]
    G = max(1, max(g.shape[0] for g in grids))  # one launch for all models: a shorter grid leaves its upper bins empty
    bins = [P.bin_of(r.confidence, g) for r, g in zip(reports, grids)]
    bins = np.stack([np.where(b >= g.shape[0], G, b) for b, g in zip(bins, grids)]).astype(np.int16)
    replicates = curve_counts(packed, bins, M, G, seed, num_replicates, device, host_bootstrap)
    bands = P.curve_bands(P.curve_counts_point(packed, bins, M, G), replicates, M, G, confidence)
    return [P.bands_to_dict({name: ivs[:g.shape[0]] for name, ivs in bands[m].items()}, g) for m, g in enumerate(grids)]


def fit_from_report(report, *, target_precision: float, curve: str = "precision", confidence: float = 0.95,
                    num_replicates: int = 2000, seed: int = 0, max_bins: int = 256, min_warnings: int = 20, device=None,
                    host_bootstrap: bool = False, calibrated: bool = False, details: Optional[Dict[str, Any]] = None
                    ) -> Optional[OperatingPoint]:
    """The operating point of ONE model from its evaluation columns (a `ColumnarEvaluationReport`), or None when no threshold
    qualifies.  `details`, when given, is filled with the point (or None), the curve bands on the grid and the best lower bound
    reached."""
    if num_replicates < 1:
        raise ValueError(f"num_replicates must be at least 1 (got {num_replicates})")
    if curve not in P.RECALL_OF:
        raise ValueError(f"curve must be one of {sorted(P.RECALL_OF)} (got {curve!r})")
    n = int(report.confidence.shape[0])
    thresholds = P.curve_grid(report.confidence, report.warned, max_bins)
    G = int(thresholds.shape[0])
    point = None
    out: Dict[str, Any] = {"num_samples": n, "num_replicates": int(num_replicates), "seed": int(seed), "curve": curve,
                           "target": float(target_precision), "confidence": float(confidence), "grid_size": G,
                           "calibrated": bool(calibrated), "best_lower_bound": None, "curve_bands": None}
    if G:
        packed, _, _ = C.pack_outcomes([report])
        bins = P.bin_of(report.confidence, thresholds)[None, :]
        replicates = curve_counts(packed, bins, 1, G, seed, num_replicates, device, host_bootstrap)
        point_counts = P.curve_counts_point(packed, bins, 1, G)
        point = P.choose_operating_point(point_counts, replicates, thresholds, curve=curve, target=target_precision,
                                         confidence=confidence, min_warnings=min_warnings, num_samples=n, seed=seed,
                                         calibrated=calibrated)
        bound = P.lower_bounds(replicates, G, curve, confidence)
        best = int(np.argmax(bound))  # the first maximum: the highest threshold among equals
        out["best_lower_bound"] = {"lower_bound": float(bound[best]), "threshold_logprob": float(thresholds[best])}
        out["curve_bands"] = P.bands_to_dict(P.curve_bands(point_counts, replicates, 1, G, confidence)[0], thresholds)
    out["operating_point"] = None if point is None else point.to_dict()
    if details is not None:
        details.update(out)
    return point


def fit_operating_point(model, nn, data: Iterable[Any], device, *, target_precision: float, curve: str = "precision",
                        confidence: float = 0.95, num_replicates: int = 2000, seed: int = 0, max_bins: int = 256,
                        min_warnings: int = 20, parallelize: bool = True, host_bootstrap: bool = False,
                        details: Optional[Dict[str, Any]] = None) -> Optional[OperatingPoint]:
    """Evaluates (model, nn) on `data` on the device -- with the model's confidence calibration, if it carries one -- fits the
    operating point and stores it on `model` (`model.warning_operating_point`).  None, and the model unchanged, when no
    threshold qualifies."""
    from buglab.models.evaluate import evaluate_on_device

    report = evaluate_on_device(model, nn, data, device, parallelize=parallelize)
    if report.confidence.shape[0] == 0:
        raise ValueError("fit_operating_point: no sample of the data could be tensorised")
    point = fit_from_report(report, target_precision=target_precision, curve=curve, confidence=confidence,
                            num_replicates=num_replicates, seed=seed, max_bins=max_bins, min_warnings=min_warnings, device=device,
                            host_bootstrap=host_bootstrap, calibrated=getattr(model, "confidence_calibration", None) is not None,
                            details=details)
    if point is not None:
        model.warning_operating_point = point
    return point


def format_details(details: Dict[str, Any]) -> str:
    pct = lambda x: "NaN" if x != x else f"{100 * x:.2f}%"
    span = lambda iv: f"{pct(iv['point'])} [{pct(iv['low'])}, {pct(iv['high'])}]"
    lines = [f"Bootstrap of the threshold curves over {details['num_samples']} samples, {details['num_replicates']} replicates, seed "
             f"{details['seed']}, {details['grid_size']} candidate thresholds"
             f"{' (calibrated confidences)' if details['calibrated'] else ''}."]
    point = details["operating_point"]
    what = f"{details['curve']} >= {pct(details['target'])} with {100 * details['confidence']:g}% confidence"
    if point is not None:
        lines.append(f"Operating point for {what}: warn at probability >= {np.exp(point['threshold_logprob']):.6f} "
                     f"(log-probability {point['threshold_logprob']:.6f}), {point['num_warnings']} warnings.")
        lines.append(f"  {details['curve']}: {span(point['precision'])}")
        lines.append(f"  {P.RECALL_OF[details['curve']]}: {span(point['recall'])}")
    elif details["best_lower_bound"] is None:
        lines.append(f"No threshold qualifies for {what}: the model warned on no sample.")
    else:
        best = details["best_lower_bound"]
        lines.append(f"No threshold qualifies for {what}: the best lower bound reached is {pct(best['lower_bound'])}, at probability "
                     f">= {np.exp(best['threshold_logprob']):.6f} (log-probability {best['threshold_logprob']:.6f}).")
    bands = details["curve_bands"]
    if bands is not None:
        G = len(bands["thresholds_logprob"])
        rows = sorted({(i * (G - 1)) // max(1, min(TABLE_ROWS, G) - 1) for i in range(min(TABLE_ROWS, G))})
        names = (details["curve"], P.RECALL_OF[details["curve"]])
        lines.append(f"  probability >=   {names[0]} [low, high]   {names[1]} [low, high]")
        for g in rows:
            cell = lambda name: span({k: bands["curves"][name][k][g] for k in ("point", "low", "high")})
            lines.append(f"  {np.exp(bands['thresholds_logprob'][g]):.6f}   {cell(names[0])}   {cell(names[1])}")
    return "\n".join(lines) + "\n"


def parse_args(argv=None) -> argparse.Namespace:
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("MODEL", help="A trained detector checkpoint (`*.pkl.gz`).")
    p.add_argument("VALID_DATA", help="Held-out `*.msgpack.l.gz` data: a file or a folder.")
    p.add_argument("OUT_MODEL", help="Where to write the checkpoint that carries the operating point.")
    p.add_argument("--target-precision", type=float, required=True, help="The precision the warnings must reach, in (0, 1].")
    p.add_argument("--curve", choices=sorted(P.RECALL_OF), default="precision",
                   help="precision: detect and repair; detection_precision: the location alone.")
    p.add_argument("--confidence", type=float, default=0.95, help="Confidence of the one-sided lower bound and of the intervals.")
    p.add_argument("--num-replicates", type=int, default=2000, help="Bootstrap replicates.")
    p.add_argument("--seed", type=int, default=0, help="Seed of the draws.")
    p.add_argument("--max-bins", type=int, default=256, help=f"Candidate thresholds, at most {P.MAX_BINS}.")
    p.add_argument("--min-warnings", type=int, default=20, help="Warnings a threshold must raise on the data to qualify.")
    p.add_argument("--limit-num-elements", type=int, default=None, help="Fit on at most this many samples.")
    p.add_argument("--sequential", action="store_true", help="Do not parallelize data loading.")
    p.add_argument("--host-bootstrap", action="store_true", help="Resample with the NumPy twin instead of the device kernel.")
    p.add_argument("--report-json", default=None, help="Also write the report as data.")
    return p.parse_args(argv)


def run(args: argparse.Namespace) -> Optional[OperatingPoint]:
    from buglab.models._cli import open_model, read_data, require_gpu, write_report_json

    require_gpu(None, "operatingpoint")
    model, nn, device, _ = open_model(args.MODEL)
    data = read_data(args.VALID_DATA, args.limit_num_elements)
    details: Dict[str, Any] = {}
    point = fit_operating_point(model, nn, data, device, target_precision=args.target_precision, curve=args.curve,
                                confidence=args.confidence, num_replicates=args.num_replicates, seed=args.seed, max_bins=args.max_bins,
                                min_warnings=args.min_warnings, parallelize=not args.sequential, host_bootstrap=args.host_bootstrap,
                                details=details)
    sys.stdout.write(format_details(details))
    if point is None:  # nothing is written: neither the checkpoint nor the report
        return None
    write_report_json(args.report_json, details)
    model.save(Path(args.OUT_MODEL), nn)
    return point


if __name__ == "__main__":
    sys.exit(0 if run(parse_args()) is not None else EXIT_NOTHING_QUALIFIES)
