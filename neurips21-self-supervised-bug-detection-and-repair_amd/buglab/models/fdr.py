#!/usr/bin/env python
"""
Usage:
    python -m buglab.models.fdr fit MODEL CLEAN_DATA OUT_MODEL [--max-reference 1048576] [--limit-num-elements N] [--sequential]
    python -m buglab.models.fdr scan MODEL DATA OUT --fdr Q [--dependence independent|arbitrary] [--top-k 3] [--html FILE]
                                     [--host] [--limit-num-elements N] [--sequential] [--report-json FILE]

False-discovery-controlled warnings -- BEYOND THE REFERENCE, which has no counterpart.  `scan` flags samples so that the expected
share of false alarms among the flagged ones is at most Q, whatever share of the scanned code is buggy.  `operatingpoint.py`
does not promise that: it bounds the precision of a threshold on the validation mix, and precision moves with the bug rate.

`fit` runs MODEL over CLEAN_DATA, keeps the NO_BUG log-probability (the SCORE; calibrated where the checkpoint carries a
calibration) of the first --max-reference samples without a bug, sorted, and writes OUT_MODEL = MODEL with `null_reference`
set.  Samples with a bug are skipped and counted, NaN scores dropped and counted.

`scan` gives every sample of DATA a conformal p-value, (1 + #{reference scores <= its score}) / (n + 1), and runs the
Benjamini-Hochberg step-up at level Q over the scan (`--dependence arbitrary`: Benjamini-Yekutieli, Q divided by sum 1 / i).  OUT
receives one JSON line per sample `tensorize` accepts, in input order: position, score, count, p_value, q_value, flagged; a
flagged sample's record also carries its --top-k fixes from `suggest(..., assume_buggy=True)`.  --html writes a page of the
flagged samples (`visualize.scan`).  DATA is read twice: once for the scan, once for the flagged samples.  Where the samples
carry labels the realised false discovery proportion and the share of buggy samples flagged are printed.

The guarantee needs the reference to be exchangeable with the clean part of the scan -- the same kind of code, and not the
training data; a validation set used for early stopping is a mild violation -- and BH needs p-values that are independent or
positively dependent, which conformal p-values sharing one reference are.  Nothing can be flagged unless the reference is large
enough: n + 1 >= N / (Q R) for R discoveries.  The tool prints the smallest attainable p-value next to what the scan needs.

Two paths give the same records.  The default leaves the model's flat output on the device: one hip_ops.fdr_counts launch per
predict minibatch into run-long buffers, one hip_ops.fdr_bh over the run (csrc/bl_fdr.hip), one copy back.  `--host` walks the
triples of `model.predict` through the NumPy twin (buglab/models/_fdr.py).  Exit status 2 when MODEL carries no reference.
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path
from typing import Any, Callable, Dict, Iterable, List, NamedTuple, Optional, Tuple

if __package__ in (None, ""):
    sys.path.insert(0, str(Path(__file__).resolve().parents[2]))

import numpy as np

from buglab.models import _fdr as F
from buglab.models._cli import open_model, read_data, require_gpu, write_records, write_report_json
from buglab.models._fdr import NullReference

EXIT_NO_REFERENCE = 2


def _label(point) -> Optional[bool]:
    """True: the sample carries a bug; False: it is labelled clean; None: it carries no label."""
    if "target_fix_action_idx" not in point:
        return None
    return point["target_fix_action_idx"] is not None


class _Scores(NamedTuple):
    positions: List[int]           # input positions of the samples `tensorize` accepted, in input order
    labels: List[Optional[bool]]
    score: Any                     # float32 [n]: a device tensor on the device path, an array on the host path
    count: Any                     # int32 [n] against the reference the run was given


def _scores_host(model, nn, tagged: Iterable[Tuple[Any, int]], device, parallelize: bool, ref: np.ndarray,
                 rejected: Callable[[int], None]) -> _Scores:
    from buglab.controllers._batching import predictions_in_order

    positions, labels, values = [], [], []
    for position, point, location_logprobs, _ in predictions_in_order(model, nn, tagged, device, parallelize, rejected, "fdr: predict"):
        positions.append(position), labels.append(_label(point)), values.append(location_logprobs[-1])
    src = np.asarray(values, np.float32)  # the fp32 values `predict` copied back, as they were
    score, count = F.counts_host(src, np.arange(src.shape[0]), ref)
    return _Scores(positions, labels, score, count)


def _scores_on_device(model, nn, tagged: Iterable[Tuple[Any, int]], device, parallelize: bool, ref: np.ndarray,
                      rejected: Callable[[int], None], capacity: int) -> _Scores:
    import torch

    from buglab.controllers import _batching as Bt
    from buglab.models import hip_ops

    device = torch.device(device)
    d_ref = torch.from_numpy(np.ascontiguousarray(ref, np.float32)).to(device)

    def extend(layout, points, dev):
        nobug = np.asarray(layout.loc_idx, np.int64)[np.asarray(layout.loc_off, np.int64)[1:] - 1]  # NO_BUG: a sample's last entry
        return {"nobug_idx": Bt.to_device_i32([nobug], dev)[0], "labels": [_label(p) for p in points]}

    cols = Bt.RunColumns(device, capacity, [("score", "float32", (Bt.SAMPLES,)), ("count", "int32", (Bt.SAMPLES,))])
    positions: List[int] = []
    labels: List[Optional[bool]] = []
    nn.eval()
    with torch.no_grad(), model._tensorize_all_location_rewrites():
        for mb, tags in Bt.prediction_minibatches(model, tagged, device, parallelize, extend, rejected):
            flat = Bt.flat_prediction_output(nn, mb)
            B = len(tags)
            assert mb["selfsup"]["nobug_idx"].shape[0] == B
            n = cols.reserve(B)
            hip_ops.fdr_counts(flat, mb["selfsup"]["nobug_idx"], d_ref, cols["score"], cols["count"], n)
            positions.extend(tags), labels.extend(mb["selfsup"]["labels"])
    found = cols.device_columns()
    return _Scores(positions, labels, found["score"], found["count"])


def fit_null_reference(model, nn, data: Iterable[Any], device, *, max_reference: int = F.MAX_REFERENCE, parallelize: bool = True,
                       host: bool = False) -> NullReference:
    """Scores the samples of `data` WITHOUT a bug (`target_fix_action_idx is None`; the others are skipped and counted) with
    the model's own predict minibatches, keeps the first `max_reference` of them in input order (NaN scores dropped and
    counted), and stores the sorted scores on `model` (`model.null_reference`).  The scores stay on the device for the run and
    are copied back once; `host` walks `model.predict` instead."""
    from buglab.controllers import _batching as Bt

    Bt.require_single_model(model, "fdr fit")
    if not 1 <= int(max_reference) <= F.MAX_REFERENCE:
        raise ValueError(f"max_reference must be in [1, {F.MAX_REFERENCE}] (got {max_reference})")
    skipped = [0]

    def clean():
        for position, point in enumerate(data):
            if point.get("target_fix_action_idx") is not None:
                skipped[0] += 1
                continue
            yield point, position

    anything = np.zeros(1, np.float32)  # the counts of a fit are not used: any reference serves
    run = _scores_host if host else _scores_on_device
    extra = () if host else (Bt.run_capacity(None, data, 1 << 14),)
    found = run(model, nn, clean(), device, parallelize, anything, lambda position: None, *extra)
    scores = found.score if host else found.score.cpu().numpy()  # the one copy (and the one synchronisation) of the run
    reference = F.make_null_reference(scores, max_reference, skipped[0], getattr(model, "confidence_calibration", None))
    model.null_reference = reference
    return reference


class FdrScan(NamedTuple):
    """What `scan_with_fdr` returns: the per-sample columns (every sample `tensorize` accepted, in input order) and the run's
    numbers."""

    positions: List[int]
    labels: List[Optional[bool]]
    score: np.ndarray      # float32 [n]
    count: np.ndarray      # int32 [n]
    p_value: np.ndarray    # float64 [n]
    q_value: np.ndarray    # float64 [n]
    flagged: np.ndarray    # bool [n]
    cutoff: int            # c*: a sample is flagged iff count <= cutoff; -1: nothing is flagged
    num_flagged: int
    q: float
    q_effective: float
    summary: Dict[str, Any]
    suggestions: Dict[int, Dict[str, Any]]  # position -> the `suggest` record of a flagged sample
    html: Optional[str]

    def records(self) -> List[Dict[str, Any]]:
        n_ref = self.summary["num_reference"]
        out = []
        for b, position in enumerate(self.positions):
            record = F.scan_record(position, self.score[b], self.count[b], n_ref, self.q_value[b], self.flagged[b])
            if position in self.suggestions:
                record["suggestions"] = self.suggestions[position]["suggestions"]
            out.append(record)
        return out


def scan_with_fdr(model, nn, data: Iterable[Any], device, q: float = 0.1, *, dependence: str = "independent", top_k: int = 3,
                  html: bool = False, host: bool = False, parallelize: bool = True) -> FdrScan:
    """Conformal p-values of every sample of `data` against `model.null_reference` and the BH step-up at level `q` over them.
    `data` is iterated twice (the scan, then the flagged samples once more through `suggest(..., top_k, assume_buggy=True)`
    and, with `html`, `visualize`), so it must be re-iterable.  LookupError without a reference, ValueError when the
    checkpoint's calibration is not the one the reference was fitted under, TypeError for an ensemble."""
    from buglab.controllers import _batching as Bt

    Bt.require_single_model(model, "fdr scan")
    reference = F.check_reference(getattr(model, "null_reference", None), getattr(model, "confidence_calibration", None), "fdr scan")
    if dependence not in F.DEPENDENCE:
        raise ValueError(f"dependence must be one of {F.DEPENDENCE} (got {dependence!r})")
    if not 0.0 < float(q) <= 1.0:
        raise ValueError(f"the false discovery rate must be in (0, 1] (got {q})")
    n_ref = reference.num_kept
    refused: List[int] = []
    tagged = ((point, position) for position, point in enumerate(data))
    if host:
        found = _scores_host(model, nn, tagged, device, parallelize, reference.scores, refused.append)
    else:
        found = _scores_on_device(model, nn, tagged, device, parallelize, reference.scores, refused.append,
                                  Bt.run_capacity(None, data, 1 << 14))
    N = len(found.positions)
    q_effective = F.effective_level(q, N, dependence) if N else float(q)
    if N == 0:
        score, count = np.zeros(0, np.float32), np.zeros(0, np.int32)
        cutoff, flag, q_value = np.array([-1, 0], np.int32), np.zeros(0, np.int32), np.zeros(0, np.float64)
    elif host:
        score, count = found.score, found.count
        cutoff, flag, q_value, _ = F.bh_host(count, n_ref, q_effective)
    else:
        import torch

        from buglab.models import hip_ops

        d_cutoff, d_flag, d_q, _ = hip_ops.fdr_bh(found.count.contiguous(), n_ref, q_effective)
        # the one copy back (and the one synchronisation) of the run: [q-values | scores | counts | flags | cutoff]
        blob = torch.cat([d_q.view(torch.int32), found.score.contiguous().view(torch.int32), found.count, d_flag, d_cutoff]).cpu()
        q_value = blob[:2 * N].view(torch.float64).numpy()
        score = blob[2 * N:3 * N].view(torch.float32).numpy()
        count, flag, cutoff = blob[3 * N:4 * N].numpy(), blob[4 * N:5 * N].numpy(), blob[5 * N:].numpy()
    flagged = flag != 0
    summary = F.summary(count, flagged, cutoff, n_ref, q, q_effective, dependence, found.labels, len(refused))

    # the flagged samples, and only they, once more
    wanted = {found.positions[b] for b in np.flatnonzero(flagged)}
    suggestions: Dict[int, Dict[str, Any]] = {}
    page = None
    if wanted or html:
        from buglab.models.suggest import suggest

        kept = [(position, point) for position, point in enumerate(data) if position in wanted]
        subset = [point for _, point in kept]
        if subset:
            for s in suggest(model, nn, subset, device, int(top_k), host=host, assume_buggy=True, parallelize=parallelize):
                suggestions[kept[s.position][0]] = s.record()
        if html:
            from buglab.models import visualize as V

            if not subset:
                snippets: List[Dict[str, Any]] = []
            elif host:
                snippets = V.predictions_to_report(model.predict(iter(subset), nn, device, parallelize)).snippets
            else:
                snippets = V.scan(model, nn, subset, device, parallelize=parallelize).snippets
            page = V.report_to_html(snippets)
    return FdrScan(found.positions, found.labels, score, count, F.p_values(count, n_ref), q_value, flagged, int(cutoff[0]),
                   int(flagged.sum()), float(q), float(q_effective), summary, suggestions, page)


# ---- command line ------------------------------------------------------------------------------------------------------------
def parse_args(argv=None) -> argparse.Namespace:
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = p.add_subparsers(dest="command", required=True)
    fit = sub.add_parser("fit", help="Fit the reference of clean scores and write a checkpoint that carries it.")
    fit.add_argument("MODEL", help="A trained detector checkpoint (`*.pkl.gz`).")
    fit.add_argument("CLEAN_DATA", help="`*.msgpack.l.gz` data known to be clean and not used for training: a file or a folder.")
    fit.add_argument("OUT_MODEL", help="Where to write the checkpoint that carries the reference.")
    fit.add_argument("--max-reference", type=int, default=F.MAX_REFERENCE, help=f"Keep at most this many scores (<= {F.MAX_REFERENCE}).")
    scan = sub.add_parser("scan", help="Flag the samples of DATA at a false discovery rate.")
    scan.add_argument("MODEL", help="A checkpoint written by `fit`.")
    scan.add_argument("DATA", help="`*.msgpack.l.gz` data to scan: a file or a folder.")
    scan.add_argument("OUT", help="JSON lines, one record per sample (gzip when the name ends in .gz).")
    scan.add_argument("--fdr", type=float, required=True, help="The false discovery rate Q, in (0, 1].")
    scan.add_argument("--dependence", choices=F.DEPENDENCE, default="independent",
                      help="independent: Benjamini-Hochberg (also right under positive dependence); arbitrary: Benjamini-Yekutieli.")
    scan.add_argument("--top-k", type=int, default=3, help="Fixes listed per flagged sample.")
    scan.add_argument("--html", default=None, help="Also write a page of the flagged samples.")
    scan.add_argument("--host", action="store_true", help="Walk `model.predict` through the NumPy twin instead of the device kernels.")
    scan.add_argument("--report-json", default=None, help="Also write the run's numbers as data.")
    for s in (fit, scan):
        s.add_argument("--limit-num-elements", type=int, default=None, help="Read at most this many samples.")
        s.add_argument("--sequential", action="store_true", help="Do not parallelize data loading.")
    return p.parse_args(argv)


def run(args: argparse.Namespace) -> int:
    model, nn, device, have_gpu = open_model(args.MODEL)
    if args.command == "scan":  # before anything is read or run: a checkpoint without a reference is the caller's mistake
        try:
            F.check_reference(getattr(model, "null_reference", None), getattr(model, "confidence_calibration", None), "fdr scan")
        except LookupError as e:
            print(str(e), file=sys.stderr)
            return EXIT_NO_REFERENCE
    require_gpu(have_gpu, "fdr")
    data = read_data(args.CLEAN_DATA if args.command == "fit" else args.DATA, args.limit_num_elements)
    if args.command == "fit":
        reference = fit_null_reference(model, nn, data, device, max_reference=args.max_reference, parallelize=not args.sequential)
        print(f"fdr fit: kept {reference.num_kept} clean scores ({reference.num_dropped_nan} NaN dropped, {reference.num_skipped_buggy} "
              f"buggy samples skipped); the smallest attainable p-value is {1.0 / (reference.num_kept + 1):.3g}.")
        model.save(Path(args.OUT_MODEL), nn)
        return 0
    found = scan_with_fdr(model, nn, data, device, args.fdr, dependence=args.dependence, top_k=args.top_k, html=args.html is not None,
                          host=args.host, parallelize=not args.sequential)
    write_records(found.records(), args.OUT)
    sys.stdout.write(F.format_summary(found.summary))
    if args.html is not None:
        with open(args.html, "w", encoding="utf-8") as f:
            f.write(found.html)
    write_report_json(args.report_json, found.summary)
    return 0


if __name__ == "__main__":
    sys.exit(run(parse_args()))
