#!/usr/bin/env python
"""
Usage:
    python -m buglab.models.triage fit MODEL OUT_TRIAGE --accepted DATA [DATA ...] --dismissed DATA [DATA ...]
                                   [--site predicted|truth] [--assume-buggy] [--folds 5] [--seed 0] [--l2 V | --l2-grid V,V,...]
                                   [--balance] [--min-per-class 10] [--max-iterations 50] [--limit-num-elements N] [--sequential]
                                   [--host] [--report-json FILE]
    python -m buglab.models.triage rank MODEL TRIAGE DATA OUT [--site predicted|truth] [--assume-buggy] [--min-confidence P]
                                   [--min-triage-probability Q] [--top-k K] [--limit-num-elements N] [--sequential] [--host]
                                   [--report-json FILE]

Warning triage -- BEYOND THE REFERENCE, which has no counterpart.  Every other tool of the scan side ends at the reviewer's desk;
this one learns from what the reviewer then does.  The user keeps the warnings somebody accepted and the warnings somebody
dismissed as ordinary shards; `fit` embeds both (a warning is a SITE as `similar` defines it, its features the embedding behind it
and its location log-probability) and fits a ridge-regularised logistic model on them: no retraining of the detector, seconds of
work.  `rank` reorders the next scan with it: warnings like the accepted ones first, warnings like the dismissed ones last.

`fit` chooses the ridge by stratified K-fold cross-validation over `--l2-grid` (default 10^-2 .. 10^3 in steps of half a decade;
the lowest out-of-fold log-loss, ties to the larger value; `--l2 V` fixes it instead).  `--balance` weights a row by N / (2 N_class).
The report gives the out-of-fold log-loss, AUC and the precision among the top 10 % and 25 %, and the same numbers for the
baseline "order by the detector's own log-probability", so it says whether triage beats the detector's confidence.  Exit status
2: a class with fewer than `--min-per-class` usable rows.  A fit that did not converge is a warning and the report says so.

`rank` writes JSON lines, most acceptable first: triage probability descending, then log-probability descending, then position;
each line has position, node, label, filename, package, logprob and `triage_probability` (null, and last, for a site whose
embedding is not finite).  `--min-confidence P` drops sites whose exp(log-probability) is below P, `--min-triage-probability Q`
those whose triage probability is below Q, `--top-k K` keeps the first K.  Exit status 2: the triage file was fitted on embeddings
of another size than the model's; other weights are a warning.

The fit is Newton's method on P = D + 2 parameters.  Every iteration needs the weighted Gram matrix of all labelled rows, and
that runs on the device: fp64 MFMA, fixed summation order, the same bits on every run (csrc/bl_triage.hip; the arithmetic:
include/buglab_hip.h).  The rows go to the device once and stay there for every fold and every l2; an iteration copies back
P^2 + P + 4 doubles.  `--host` runs the NumPy twin (buglab/models/_triage.py) through the same driver.
"""
from __future__ import annotations

import argparse
import logging
import sys
from pathlib import Path
from typing import Any, Dict, Iterable, List, NamedTuple, Optional, Sequence, Tuple

if __package__ in (None, ""):
    sys.path.insert(0, str(Path(__file__).resolve().parents[2]))

import numpy as np

from buglab.models import _similar as S
from buglab.models import _triage as R
from buglab.models._cli import collect_sites as _collect_sites, embed_sites as _embed_sites, embedding_dim as _embedding_dim
from buglab.models._cli import open_model as _open_model, read_data as _read_data, require_gpu, write_records, write_report_json
from buglab.models._triage import TriageModel

LOGGER = logging.getLogger(__name__)
EXIT_DIMENSION_MISMATCH = 2
EXIT_TOO_FEW_VERDICTS = 2


class TooFewVerdicts(ValueError):
    """A class has fewer usable rows than the fit was told to need."""


class TriageFit(NamedTuple):
    model: TriageModel
    report: Dict[str, Any]


def _as_array(x, dtype=np.float32) -> np.ndarray:
    return np.ascontiguousarray(x if isinstance(x, np.ndarray) else x.detach().cpu().numpy(), dtype)


class DeviceProblem:
    """The labelled rows on the device, for `_triage.cross_validate`: uploaded once; `stats` is one call of
    `hip_ops.triage_newton_stats` and one copy back of P^2 + P + 4 doubles, `score` one of `hip_ops.triage_score`."""

    def __init__(self, x: np.ndarray, logprob: np.ndarray, y: np.ndarray, shift: np.ndarray, scale: np.ndarray, device):
        import torch

        from buglab.models import hip_ops

        self._torch, self._ops = torch, hip_ops
        self.N, D = x.shape
        self.P = D + 2
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        self.x, self.logprob, self.y = up(x), up(logprob), up(np.asarray(y).astype(np.uint8))
        self.shift, self.scale = up(np.asarray(shift, np.float64)), up(np.asarray(scale, np.float64))
        self.workspace = torch.empty(max(hip_ops.triage_workspace_bytes(self.N, D) // 8, 1), dtype=torch.float64, device=device)
        self.out = torch.empty(self.P * self.P + self.P + 4, dtype=torch.float64, device=device)
        self._weights: Tuple[Any, Any] = (None, None)  # the last c and its copy on the device: a fit passes the same one every time

    def _c(self, c):
        if c is None:
            return None
        if self._weights[0] is not c:
            self._weights = (c, self._torch.from_numpy(np.ascontiguousarray(c, np.float64)).to(self.x.device))
        return self._weights[1]

    def stats(self, w, c, l2: float) -> R.Stats:
        P = self.P
        d_w = self._torch.from_numpy(np.ascontiguousarray(w, np.float64)).to(self.x.device)
        blob = self._ops.triage_newton_stats(self.x, self.logprob, self.shift, self.scale, d_w, self.y, self._c(c), l2,
                                             workspace=self.workspace, out=self.out).cpu().numpy()
        return R.Stats(blob[:P * P].reshape(P, P), blob[P * P:P * P + P], float(blob[-4]), float(blob[-3]), int(blob[-2]), int(blob[-1]))

    def score(self, w) -> Tuple[np.ndarray, np.ndarray]:
        d_w = self._torch.from_numpy(np.ascontiguousarray(w, np.float64)).to(self.x.device)
        both = self._ops.triage_score(self.x, self.logprob, self.shift, self.scale, d_w).cpu().numpy()
        return both[0], both[1]


def fit_triage_embeddings(rows, logprobs, labels, *, folds: int = 5, seed: int = 0, l2: Optional[float] = None,
                          l2_grid: Optional[Sequence[float]] = None, balance: bool = False, min_per_class: int = 10,
                          max_iterations: int = 50, device=None, host: bool = False, site: str = "predicted", model_class: str = "",
                          fingerprint: str = "") -> TriageFit:
    """The re-ranker of embeddings that already exist: rows [N, D] fp32 (an array or a tensor), logprobs [N], labels [N] (1 =
    accepted).  -> TriageFit(model, report).  `l2` fixes the ridge, otherwise it is chosen over `l2_grid` (None: the default
    grid) by stratified `folds`-fold cross-validation seeded with `seed`.  `host`: the NumPy twin through the same driver.
    TooFewVerdicts when a class has fewer than `min_per_class` rows whose entries are all finite; ValueError for sizes the
    kernels do not take or an l2 that is not positive."""
    x, lp = _as_array(rows), _as_array(logprobs)
    y = np.asarray(labels).astype(bool)
    if x.ndim != 2 or not 1 <= x.shape[1] <= R.MAX_D or lp.shape != (x.shape[0],) or y.shape != (x.shape[0],):
        raise ValueError(f"triage: rows {x.shape} must be [N, 1 <= D <= {R.MAX_D}], logprobs {lp.shape} and labels {y.shape} [N]")
    if l2 is not None and l2_grid is not None:
        raise ValueError("triage: give l2 or l2_grid, not both")
    grid = [float(l2)] if l2 is not None else [float(v) for v in (R.DEFAULT_L2_GRID if l2_grid is None else l2_grid)]
    if not grid or any(not (v > 0.0 and np.isfinite(v)) for v in grid):
        raise ValueError(f"triage: every l2 must be positive and finite (got {grid})")
    if int(folds) < 2 or int(max_iterations) < 1:
        raise ValueError(f"triage: need folds >= 2 and max_iterations >= 1 (got {folds}, {max_iterations})")
    N, D = x.shape
    usable = R.finite_rows(x, lp)
    n1, n0 = int((usable & y).sum()), int((usable & ~y).sum())
    need = max(int(min_per_class), int(folds) if len(grid) > 1 else 1)
    if min(n1, n0) < need:
        raise TooFewVerdicts(f"triage: {n1} accepted and {n0} dismissed usable rows; the fit needs at least {need} of each")
    shift, scale = R.standardise(x, lp)
    c = R.balance_weights(y, usable) if balance else None
    if host:
        problem: Any = R.HostProblem(x, lp, y, shift, scale)
    else:
        if device is None:
            device = rows.device if not isinstance(rows, np.ndarray) and rows.is_cuda else "cuda"
        problem = DeviceProblem(x, lp, y, shift, scale, device)
    cv = R.cross_validate(problem, y, c, usable, folds=folds, seed=seed, l2_grid=grid, max_iterations=max_iterations)
    if not cv.converged:
        LOGGER.warning("triage: the fit at l2 = %g did not converge in %d iterations (|g|_inf = %.3g)", cv.l2, cv.fit.iterations,
                       cv.fit.gradient_norm)
    table = np.asarray(cv.table, np.float64).reshape(-1, 2)
    model = TriageModel(cv.w, shift, scale, cv.l2, D, str(site), str(model_class), str(fingerprint), n1, n0, table[:, 0].copy(),
                        table[:, 1].copy(), bool(cv.converged))
    report: Dict[str, Any] = {
        "num_rows": N, "num_skipped": int(N - usable.sum()), "num_accepted": n1, "num_dismissed": n0, "dim": D, "l2": cv.l2,
        "balanced": bool(balance), "folds": int(folds) if len(grid) > 1 else 0, "seed": int(seed), "converged": bool(cv.converged),
        "all_folds_converged": bool(cv.all_converged), "newton_iterations": int(cv.newton_iterations),
        "final_iterations": int(cv.fit.iterations), "final_loss": float(cv.fit.losses[-1]), "gradient_norm": float(cv.fit.gradient_norm),
        "cv": [{"l2": a, "log_loss": b} for a, b in cv.table], "path": "host" if host else "device"}
    if len(grid) > 1:
        in_fold = ~np.isnan(cv.oof_margin)
        base_c = np.ones(N) if c is None else c
        report["triage"] = dict(R.ranking_metrics(cv.oof_margin[in_fold], y[in_fold]),
                                log_loss=R.log_loss(cv.oof_margin[in_fold], y[in_fold], base_c[in_fold]))
        report["baseline_logprob"] = R.ranking_metrics(lp[in_fold].astype(np.float64), y[in_fold])
        report["beats_baseline"] = bool(report["triage"]["auc"] > report["baseline_logprob"]["auc"])
    return TriageFit(model, report)


def fit_triage(model, nn, accepted: Iterable[Any], dismissed: Iterable[Any], device, *, site: str = "predicted", assume_buggy: bool = False,
               folds: int = 5, seed: int = 0, l2: Optional[float] = None, l2_grid: Optional[Sequence[float]] = None, balance: bool = False,
               min_per_class: int = 10, max_iterations: int = 50, host: bool = False, parallelize: bool = True,
               report: Optional[Dict[str, Any]] = None) -> TriageModel:
    """Fit the re-ranker on the sites of the `accepted` and the `dismissed` samples (module docstring).  `report`: a dict that
    receives the run's numbers.  TypeError for an ensemble or the GREAT var-misuse model, TooFewVerdicts when a class is too
    small."""
    from buglab.controllers import _batching as Bt

    Bt.require_single_model(model, "triage")
    options = dict(assume_buggy=assume_buggy, host=host, parallelize=parallelize)
    yes = _embed_sites(model, nn, accepted, device, site, **options)
    no = _embed_sites(model, nn, dismissed, device, site, **options)
    n_yes, n_no = yes.rows.shape[0], no.rows.shape[0]
    if min(n_yes, n_no) == 0:  # (an empty set's rows have no width to concatenate with)
        raise TooFewVerdicts(f"triage: {n_yes} accepted and {n_no} dismissed sites; the fit needs both")
    rows = np.concatenate([yes.rows, no.rows])
    logprobs = np.concatenate([yes.logprobs, no.logprobs])
    labels = np.concatenate([np.ones(n_yes, bool), np.zeros(n_no, bool)])
    fit = fit_triage_embeddings(rows, logprobs, labels, folds=folds, seed=seed, l2=l2, l2_grid=l2_grid, balance=balance,
                                min_per_class=min_per_class, max_iterations=max_iterations, device=device, host=host, site=site,
                                model_class=type(model).__name__, fingerprint=S.model_fingerprint(nn))
    if report is not None:
        report.update(fit.report)
        for name, sites in (("accepted", yes), ("dismissed", no)):
            report[name] = {"num_samples": sites.num_samples, "num_rejected": sites.num_rejected, "num_without_site": sites.num_without_site}
    return fit.model


# ---- ranking -----------------------------------------------------------------------------------------------------------------
class TriagedWarning(NamedTuple):
    position: int
    node: int
    label: str
    filename: str
    package: str
    logprob: float
    triage_probability: Optional[float]   # None: the site's embedding is not finite
    margin: Optional[float]

    def record(self) -> Dict[str, Any]:
        return {"position": self.position, "node": self.node, "label": self.label, "filename": self.filename, "package": self.package,
                "logprob": self.logprob, "triage_probability": self.triage_probability}


class Ranking(NamedTuple):
    warnings: List[TriagedWarning]
    summary: Dict[str, Any]


def score_embeddings(triage: TriageModel, rows, logprobs, device=None, host: bool = False):
    """(margin, probability) of rows [N, D] under a fitted re-ranker: float64 arrays on the host path, ONE float64 [2, N] device
    tensor on the device path (row 0 the margins), not copied back.  DimensionMismatch for rows of another size."""
    if int(rows.shape[1]) != triage.dim:
        raise S.DimensionMismatch(f"the triage file was fitted on embeddings of size {triage.dim}; these are of size {int(rows.shape[1])}")
    if host:
        return R.score_host(_as_array(rows), _as_array(logprobs), triage.shift, triage.scale, triage.w)
    import torch

    from buglab.models import hip_ops

    if isinstance(rows, np.ndarray):
        rows, logprobs = torch.from_numpy(_as_array(rows)).to(device or "cuda"), torch.from_numpy(_as_array(logprobs)).to(device or "cuda")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(rows.device)
    return hip_ops.triage_score(rows, logprobs, up(triage.shift), up(triage.scale), up(triage.w))


def rank_sites(triage: TriageModel, found, *, min_confidence: Optional[float] = None, min_triage_probability: Optional[float] = None,
               top_k: Optional[int] = None, host: bool = False) -> Ranking:
    """The ranking of sites that were collected already (`similar._collect_sites`): what `rank_warnings` does after the model
    ran.  On the device path the scores are one launch over the run-long embedding buffer and one copy back of
    [margins | probabilities | places | log-probabilities]; the embeddings stay where they are."""
    n = len(found.positions)
    if n == 0:
        place, logprob, z, p = np.zeros(0, np.int32), np.zeros(0, np.float32), np.zeros(0), np.zeros(0)
    elif host:
        place, logprob = np.asarray(found.place), np.asarray(found.logprob, np.float32)
        z, p = score_embeddings(triage, found.rows, logprob, host=True)
    else:
        import torch

        both = score_embeddings(triage, found.rows, found.logprob)
        blob = torch.cat([both.reshape(-1).view(torch.int32), found.place, found.logprob.view(torch.int32)]).cpu()
        f64 = blob[:4 * n].view(torch.float64).numpy()
        z, p = f64[:n], f64[n:]
        place, logprob = blob[4 * n:5 * n].numpy(), blob[5 * n:].view(torch.float32).numpy()
    sites = np.flatnonzero(place >= 0)
    keep = sites
    dropped_confidence = dropped_probability = 0
    if min_confidence is not None:
        with np.errstate(over="ignore"):
            ok = np.exp(logprob[keep].astype(np.float64)) >= float(min_confidence)
        dropped_confidence, keep = int((~ok).sum()), keep[ok]
    if min_triage_probability is not None:
        ok = np.isnan(p[keep]) | (p[keep] >= float(min_triage_probability))  # a site without a probability is never dropped for it
        dropped_probability, keep = int((~ok).sum()), keep[ok]
    positions = np.asarray([found.positions[b] for b in keep], np.int64)
    order = keep[R.rank_order(p[keep], logprob[keep], positions)]
    if top_k is not None:
        order = order[:max(int(top_k), 0)]
    out: List[TriagedWarning] = []
    for b in order:
        node, label, path, package = S.site_metadata(found.points[b], place[b])
        missing = bool(np.isnan(p[b]))
        out.append(TriagedWarning(int(found.positions[b]), node, label, path, package, float(logprob[b]), None if missing else float(p[b]),
                                  None if missing else float(z[b])))
    have = p[keep][~np.isnan(p[keep])]
    summary = {"num_samples": found.num_samples, "num_rejected": found.num_rejected, "num_without_site": n - sites.shape[0],
               "num_warnings": int(sites.shape[0]), "num_below_min_confidence": dropped_confidence,
               "num_below_min_triage_probability": dropped_probability, "num_ranked": int(keep.shape[0]), "num_listed": len(out),
               "num_invalid_embeddings": int(np.isnan(p[keep]).sum()), "probability_histogram": R.probability_histogram(have),
               "share_above_half": float((have > 0.5).mean()) if have.shape[0] else 0.0, "l2": triage.l2, "dim": triage.dim,
               "triage_converged": bool(triage.converged)}
    return Ranking(out, summary)


def rank_scan(model, nn, triage: TriageModel, data: Iterable[Any], device, *, site: str = "predicted", assume_buggy: bool = False,
              min_confidence: Optional[float] = None, min_triage_probability: Optional[float] = None, top_k: Optional[int] = None,
              host: bool = False, parallelize: bool = True) -> Ranking:
    """`rank_warnings` with the run's numbers."""
    from buglab.controllers import _batching as Bt

    Bt.require_single_model(model, "triage")
    warning = triage.check_model(type(model).__name__, _embedding_dim(nn), S.model_fingerprint(nn))  # DimensionMismatch before any work
    if warning:
        LOGGER.warning("%s", warning)
    found = _collect_sites(model, nn, data, device, site, assume_buggy, host, parallelize)
    return rank_sites(triage, found, min_confidence=min_confidence, min_triage_probability=min_triage_probability, top_k=top_k, host=host)


def rank_warnings(model, nn, triage: TriageModel, data: Iterable[Any], device, **options) -> List[TriagedWarning]:
    """The warnings of `data`, most acceptable first (module docstring).  Options: site, assume_buggy, min_confidence,
    min_triage_probability, top_k, host, parallelize.  TypeError for an ensemble or the GREAT var-misuse model,
    `_similar.DimensionMismatch` when the re-ranker was fitted on embeddings of another size; other weights are logged as a
    warning."""
    return rank_scan(model, nn, triage, data, device, **options).warnings


# ---- command line ------------------------------------------------------------------------------------------------------------
def _grid(text: str) -> List[float]:
    try:
        return [float(v) for v in text.split(",") if v.strip()]
    except ValueError:
        raise argparse.ArgumentTypeError(f"not a comma-separated list of numbers: {text!r}")


def parse_args(argv=None) -> argparse.Namespace:
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = p.add_subparsers(dest="command", required=True)
    fit = sub.add_parser("fit", help="Fit the re-ranker on accepted and dismissed warnings.")
    fit.add_argument("MODEL", help="A trained detector checkpoint (`*.pkl.gz`).")
    fit.add_argument("OUT_TRIAGE", help="The triage file to write (.npz).")
    fit.add_argument("--accepted", nargs="+", required=True, help="`*.msgpack.l.gz` data of the warnings a reviewer accepted.")
    fit.add_argument("--dismissed", nargs="+", required=True, help="`*.msgpack.l.gz` data of the warnings a reviewer dismissed.")
    fit.add_argument("--folds", type=int, default=5, help="Folds of the cross-validation that chooses the ridge.")
    fit.add_argument("--seed", type=int, default=0, help="Seed of the folds.")
    ridge = fit.add_mutually_exclusive_group()
    ridge.add_argument("--l2", type=float, default=None, help="The ridge, instead of choosing it.")
    ridge.add_argument("--l2-grid", type=_grid, default=None, help="The values to choose the ridge from, comma-separated.")
    fit.add_argument("--balance", action="store_true", help="Weight a row by N / (2 N_class).")
    fit.add_argument("--min-per-class", type=int, default=10, help="Usable rows each class needs (exit status 2 below it).")
    fit.add_argument("--max-iterations", type=int, default=50, help="Newton iterations per fit.")
    rank = sub.add_parser("rank", help="Order the warnings of DATA, most acceptable first.")
    rank.add_argument("MODEL", help="The checkpoint the triage file was fitted with.")
    rank.add_argument("TRIAGE", help="A file written by `fit`.")
    rank.add_argument("DATA", help="`*.msgpack.l.gz` data to scan: a file or a folder.")
    rank.add_argument("OUT", help="JSON lines, one warning per line (gzip when the name ends in .gz).")
    rank.add_argument("--min-confidence", type=float, default=None, help="Drop sites whose probability is below this.")
    rank.add_argument("--min-triage-probability", type=float, default=None, help="Drop sites whose triage probability is below this.")
    rank.add_argument("--top-k", type=int, default=None, help="List only the first K.")
    for s in (fit, rank):
        s.add_argument("--site", choices=S.SITE_MODES, default="predicted", help="Which location of a sample is its warning.")
        s.add_argument("--assume-buggy", action="store_true", help="Leave NO_BUG out when the site is predicted.")
        s.add_argument("--limit-num-elements", type=int, default=None, help="Read at most this many samples of each data path.")
        s.add_argument("--sequential", action="store_true", help="Do not parallelize data loading.")
        s.add_argument("--host", action="store_true", help="Fit / score in the NumPy twin instead of the device kernels.")
        s.add_argument("--report-json", default=None, help="Also write the run's numbers as data.")
    args = p.parse_args(argv)
    if args.command == "fit" and (args.folds < 2 or args.max_iterations < 1 or args.min_per_class < 1 or (args.l2 is not None and not args.l2 > 0.0)
                                  or (args.l2_grid is not None and (not args.l2_grid or min(args.l2_grid) <= 0.0))):
        p.error("need --folds >= 2, --max-iterations >= 1, --min-per-class >= 1 and every l2 > 0")
    return args


def run(args: argparse.Namespace) -> int:
    model, nn, device, have_gpu = _open_model(args.MODEL)
    if args.command == "rank":  # before anything is read or run: a re-ranker of another model's embeddings is the caller's mistake
        triage = TriageModel.load(args.TRIAGE)
        try:
            triage.check_model(type(model).__name__, _embedding_dim(nn), triage.fingerprint)
        except S.DimensionMismatch as e:
            print(str(e), file=sys.stderr)
            return EXIT_DIMENSION_MISMATCH
    require_gpu(have_gpu, "triage")
    if args.command == "fit":
        accepted = [p for path in args.accepted for p in _read_data(path, args.limit_num_elements)]
        dismissed = [p for path in args.dismissed for p in _read_data(path, args.limit_num_elements)]
        report: Dict[str, Any] = {}
        try:
            fitted = fit_triage(model, nn, accepted, dismissed, device, site=args.site, assume_buggy=args.assume_buggy, folds=args.folds,
                                seed=args.seed, l2=args.l2, l2_grid=args.l2_grid, balance=args.balance, min_per_class=args.min_per_class,
                                max_iterations=args.max_iterations, host=args.host, parallelize=not args.sequential, report=report)
        except TooFewVerdicts as e:
            print(str(e), file=sys.stderr)
            return EXIT_TOO_FEW_VERDICTS
        fitted.save(args.OUT_TRIAGE)
        line = f"triage fit: {fitted.num_accepted} accepted and {fitted.num_dismissed} dismissed sites of size {fitted.dim}, l2 = {fitted.l2:g}"
        if "triage" in report:
            t, b = report["triage"], report["baseline_logprob"]
            line += (f"; out of fold: log-loss {t['log_loss']:.4f}, AUC {t['auc']:.4f} (the detector's log-probability alone: "
                     f"{b['auc']:.4f}), precision in the top 10 % {t['precision_at_10']:.3f} ({b['precision_at_10']:.3f})")
        print(line + ("." if fitted.converged else "; THE FIT DID NOT CONVERGE."))
        write_report_json(args.report_json, report)
        return 0
    data = _read_data(args.DATA, args.limit_num_elements)
    ranked = rank_scan(model, nn, triage, data, device, site=args.site, assume_buggy=args.assume_buggy, min_confidence=args.min_confidence,
                       min_triage_probability=args.min_triage_probability, top_k=args.top_k, host=args.host,
                       parallelize=not args.sequential)
    write_records([w.record() for w in ranked.warnings], args.OUT)
    s = ranked.summary
    print(f"triage rank: {s['num_listed']} of {s['num_warnings']} warnings of {s['num_samples']} samples listed "
          f"({s['num_invalid_embeddings']} without a probability); {100.0 * s['share_above_half']:.1f}% above 1/2.")
    write_report_json(args.report_json, s)
    return 0


if __name__ == "__main__":
    sys.exit(run(parse_args()))
