#!/usr/bin/env python
"""
Usage:
    python -m buglab.models.review MODEL DATA OUT --budget B [--reviewed INDEX] [--triage TRIAGE [--uncertainty-band LO HI]]
                                   [--max-similarity S] [--min-confidence P] [--site predicted|truth] [--assume-buggy] [--no-center]
                                   [--limit-num-elements N] [--sequential] [--host] [--report-json FILE]

Review queues -- BEYOND THE REFERENCE, which has no counterpart.  `calibrate`, `operatingpoint` and `fdr` decide what becomes a
warning, `similar` and `drift` say what it resembles, `group` folds duplicates and `triage` learns from a reviewer's verdicts;
this says WHICH warnings the reviewer should look at.  "Most confident first" labels the same pattern again and again, and those
are the labels `triage fit` learns least from.  Given a budget of B reviews and what was reviewed already, the queue is the B
warnings that cover the scan best: each pick is the warning least like everything reviewed or queued so far -- k-center greedy,
or farthest-point selection (Gonzalez 1985; the core-set selection of Sener & Savarese 2018).  It closes the loop
scan -> review queue -> verdicts -> `triage fit` -> scan.

A warning is a SITE as `similar` defines it (`--site`, `--assume-buggy`: buglab/models/similar.py), its embedding the row of the
head input behind it.  `--reviewed INDEX` is a file written by `similar index` over everything already accepted or dismissed:
its entries are the first centres and the candidates are centred with the index's mean, as `similar query` does; an index of
embeddings of another size ends the run with status 2, other weights are a warning.  Without an index the candidates are centred
with their own column mean (`--no-center`: as they are), as `group` does, and the most probable eligible warning is the first
pick and the first centre (the cold start).  `--triage TRIAGE` (a file written by `triage fit`; another embedding size: status
2) restricts the picks to the warnings the re-ranker is unsure about: those whose triage probability lies in
`--uncertainty-band`, 0.2 to 0.8 by default.  `--min-confidence P` drops the sites whose exp(log-probability) is below P before
anything else.  `--max-similarity S` ends the queue when every warning left has a cosine of at least S to something reviewed or
queued.

OUT is JSON lines, one queued warning per line in pick order: rank, position, node, label, filename, package, logprob, the
triage probability if any, `nearest` -- the nearest earlier item, a reviewed index entry with its metadata or an earlier rank,
with the cosine re-scored in fp64 from the fp32 rows -- and `stands_for`, the number of eligible warnings that have this pick as
their nearest item.  The report has the counts, the picks made, why the queue ended -- budget; max-similarity, with S < 1;
nothing-left, which at the default S = 1 includes "only exact copies of reviewed or queued warnings are left", counted as
num_left_as_copies -- the coverage curve (the cosine of the worst-covered eligible warning after 1, 2, 4, ... picks) and the
same worst-covered cosine for "review the B most confident instead".

The selection runs on the int8 images of `similar`, where dot products are exact integers: the first centres are applied by an
M x L int8 GEMM that is never stored (v_mfma_i32_16x16x64_i8), the B dependent picks by one call that enqueues B + 1 launches
with no host synchronisation and no communication between workgroups inside a launch (csrc/bl_review.hip; the arithmetic:
include/buglab_hip.h).  `--host` runs the NumPy twin (buglab/models/_review.py); both paths write the same bytes.
"""
from __future__ import annotations

import argparse
import logging
import sys
from pathlib import Path
from typing import Any, Iterable, List, Optional, Sequence

if __package__ in (None, ""):
    sys.path.insert(0, str(Path(__file__).resolve().parents[2]))

import numpy as np

from buglab.models import _review as R
from buglab.models import _similar as S
from buglab.models._cli import embed_sites as _embed_sites, embedding_dim as _embedding_dim, open_model as _open_model
from buglab.models._cli import read_data as _read_data, require_gpu, write_records, write_report_json
from buglab.models._review import QueuedWarning, ReviewQueue, Selection
from buglab.models._similar import SiteEmbeddings, SiteIndex

LOGGER = logging.getLogger(__name__)
EXIT_DIMENSION_MISMATCH = 2
DEFAULT_BAND = (0.2, 0.8)


def _as_array(x) -> np.ndarray:
    return np.ascontiguousarray(x if isinstance(x, np.ndarray) else x.detach().cpu().numpy(), np.float32)


class _HostOps:
    """the NumPy twin behind the one driver below; a state is (best, near)"""

    def images(self, x, mean, y):
        cx, qx, sx, _ = S.quantize_host(x, mean)
        cy, qy, sy, _ = S.quantize_host(y, np.zeros(x.shape[1], np.float32))
        self.c, self.q, self.sumsq = np.concatenate([cy, cx]), np.concatenate([qy, qx]), np.concatenate([sy, sx])
        self.n = R.norms_host(self.q)
        return self.n

    def cover(self, centres: np.ndarray, state, first_id: int):
        best, near = state if state is not None else (None, None)
        return R.cover_host(self.q, self.n, self.q[centres], self.n[centres], best, near, first_id)

    def greedy(self, state, budget: int, open_: np.ndarray, stop: float, blocks):
        picks, aff, pnear, best, near = R.greedy_host(self.q, self.n, state[0], state[1], budget, open_.astype(np.uint8), stop)
        return (picks, aff, pnear), (best, near)

    def rescore(self, picks: np.ndarray, pnear: np.ndarray):
        return S.rescore_host(self.c[picks], self.c, self.sumsq, pnear[:, None], 1)[1][:, 0]

    def fetch(self, state, other_best, dot):
        return state, other_best, dot, self.sumsq


class _DeviceOps:
    """the kernels behind the same driver; three copies back: the norms, the pick lists, and `fetch`'s final state"""

    def __init__(self, device):
        import torch

        from buglab.models import hip_ops

        self.torch, self.ops, self.device = torch, hip_ops, device

    def _up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.device)

    def images(self, x, mean, y):
        torch, ops = self.torch, self.ops
        d_x = self._up(x)
        cx, qx, sx, _ = ops.similar_quantize(d_x, self._up(mean), out_c=d_x)
        if y.shape[0]:
            d_y = self._up(y)
            cy, qy, sy, _ = ops.similar_quantize(d_y, torch.zeros(x.shape[1], dtype=torch.float32, device=self.device), out_c=d_y)
            self.c, self.q, self.sumsq = torch.cat([cy, cx]), torch.cat([qy, qx]), torch.cat([sy, sx])
        else:
            self.c, self.q, self.sumsq = cx, qx, sx
        self.n = ops.review_norms(self.q)
        return self.n.cpu().numpy()  # the first copy back: which rows are valid decides who is eligible

    def cover(self, centres: np.ndarray, state, first_id: int):
        best, near = (state[0].clone(), state[1].clone()) if state is not None else (None, None)
        at = self._up(np.asarray(centres, np.int64))
        return self.ops.review_cover(self.q, self.n, self.q[at], self.n[at], best, near, first_id=first_id)

    def greedy(self, state, budget: int, open_: np.ndarray, stop: float, blocks):
        best, near = state[0].clone(), state[1].clone()
        lists = self.ops.review_greedy(self.q, self.n, best, near, budget, eligible=self._up(open_.astype(np.uint8)), stop=stop, blocks=blocks)
        return lists, (best, near)

    def rescore(self, picks: np.ndarray, pnear: np.ndarray):
        at = self._up(np.asarray(picks, np.int64))
        return self.ops.similar_rescore(self.c[at], self.c, self.sumsq, self._up(pnear.astype(np.int32)[:, None]), 1)[1][:, 0]

    def fetch(self, state, other_best, dot):
        torch = self.torch
        host = lambda t: t.cpu().numpy()
        # the last copy back: [best | other best | sumsq | dot] as one float64 blob, [near] as int32
        M, P = state[0].shape[0], dot.shape[0]
        blob = host(torch.cat([state[0], other_best, self.sumsq, dot]))
        return (blob[:M], host(state[1])), blob[M:2 * M], blob[3 * M:3 * M + P], blob[2 * M:3 * M]


def queue_embeddings(rows, budget: int, logprobs=None, reviewed_rows=None, eligible=None, *, mean=None, center: bool = True,
                     max_similarity: float = 1.0, device=None, host: bool = False, blocks: Optional[int] = None) -> Selection:
    """The review queue of embeddings that already exist: rows [N, D], fp32, an array or a tensor, the candidates;
    `reviewed_rows` [L, D]: what was reviewed already, CENTRED (a `SiteIndex`'s embeddings); `logprobs` [N] decides the cold
    start and the order the queue is compared with; `eligible` [N], bool: who may be picked (None: everyone).  `mean`: what to
    subtract from the candidates (a `SiteIndex`'s mean); when None their own column mean (`center`) or nothing.  `host`: the
    NumPy twin, equal bit for bit.  Row indices of the result are in the one row space: reviewed rows 0 .. L - 1, candidates
    after them.  ValueError for a similarity outside (0, 1] or sizes the kernels do not take.  Three copies back: the norms
    (which rows are valid decides who is eligible), the pick lists (they decide what is re-scored), the final state."""
    stop = R.stop_of(max_similarity)
    B = int(budget)
    if not 0 <= B <= R.MAX_BUDGET:
        raise ValueError(f"review: the budget must be in [0, {R.MAX_BUDGET}] (got {budget})")
    x = _as_array(rows)
    if x.ndim != 2 or not 1 <= x.shape[1] <= S.MAX_D:
        raise ValueError(f"review: rows {x.shape} must be [N, 1 <= D <= {S.MAX_D}]")
    N, D = x.shape
    y = np.zeros((0, D), np.float32) if reviewed_rows is None else _as_array(reviewed_rows)
    if N == 0:  # no candidate has a size to disagree with
        y = np.zeros((y.shape[0], D), np.float32)
    if y.ndim != 2 or y.shape[1] != D:
        raise S.DimensionMismatch(f"the reviewed rows hold embeddings of size {y.shape[-1]}; the candidates' are of size {D}")
    L, M = y.shape[0], y.shape[0] + N
    if M > R.MAX_ROWS:
        raise ValueError(f"review: {L} reviewed rows and {N} candidates are above {R.MAX_ROWS} rows")
    if mean is None:
        mean = S.column_mean(x) if center else np.zeros(D, np.float32)
    mean = np.ascontiguousarray(mean, np.float32)
    lp = np.zeros(M, np.float64)
    if logprobs is not None:
        lp[L:] = np.asarray(logprobs, np.float64).reshape(-1)
    allowed = np.ones(N, bool) if eligible is None else np.asarray(eligible).reshape(-1) != 0
    if allowed.shape != (N,):
        raise ValueError(f"review: eligible {allowed.shape} must be [{N}]")
    empty_i, empty_f = np.zeros(0, np.int32), np.zeros(0, np.float64)
    if N == 0:
        return Selection(empty_i, empty_f, empty_i, empty_f, np.full(M, R.NO_CENTRE), np.full(M, -1, np.int32), np.zeros(M, bool),
                         np.zeros(M, bool), L, B, stop, R.end_reason(0, B, 0), float("nan"), mean)
    if host:
        ops = _HostOps()
    else:
        if device is None:
            device = rows.device if not isinstance(rows, np.ndarray) and rows.is_cuda else "cuda"
        ops = _DeviceOps(device)
    valid = ops.images(x, mean, y) > 0
    open_ = np.zeros(M, bool)
    open_[L:] = valid[L:] & allowed
    reviewed = ops.cover(np.arange(L), None, 0)  # L == 0: the fresh state
    state, first = reviewed, None
    if L == 0 and B > 0 and open_.any():  # the cold start: the most probable eligible warning is the first pick and centre
        first = int(R.most_confident(lp, open_, 1)[0])
        state = ops.cover(np.asarray([first]), reviewed, first)
    lists, state = ops.greedy(state, B - (first is not None), open_, stop, blocks)
    confident = R.most_confident(lp, open_, B)
    other = ops.cover(confident, reviewed, 0) if confident.shape[0] else reviewed
    if host:
        picks, aff, pnear = lists
    else:
        blob = ops.torch.cat([lists[0], lists[2], lists[1].view(ops.torch.int32)]).cpu().numpy()  # the picks decide what is re-scored
        Bg = lists[0].shape[0]
        picks, pnear, aff = blob[:Bg], blob[Bg:2 * Bg], blob[2 * Bg:].view(np.float64)
    made = picks >= 0
    picks, aff, pnear = picks[made], aff[made], pnear[made]
    if first is not None:
        picks, aff, pnear = np.r_[np.int32(first), picks], np.r_[R.NO_CENTRE, aff], np.r_[np.int32(-1), pnear]
    picks, pnear = picks.astype(np.int32), pnear.astype(np.int32)
    P = picks.shape[0]
    dot = ops.rescore(picks, pnear) if P else (empty_f if host else ops.torch.zeros(0, dtype=ops.torch.float64, device=ops.device))
    (best, near), other_best, dot, sumsq = ops.fetch(state, other[0], dot)
    sim = S.similarity(dot, sumsq[picks], np.where(pnear >= 0, sumsq[np.maximum(pnear, 0)], 0.0)) if P else empty_f
    return Selection(picks, np.asarray(aff, np.float64), pnear, np.asarray(sim, np.float64), np.asarray(best, np.float64),
                     np.asarray(near, np.int32), valid, open_, L, B, stop, R.end_reason(P, B, int(open_.sum()), stop),
                     R.worst_covered(other_best, open_), mean)


def review_sites(sites: SiteEmbeddings, budget: int, *, reviewed: Optional[SiteIndex] = None, triage=None,
                 band: Sequence[float] = DEFAULT_BAND, max_similarity: float = 1.0, min_confidence: Optional[float] = None,
                 center: bool = True, device=None, host: bool = False) -> ReviewQueue:
    """The review queue of sites that were embedded already (`similar.embed_sites`): what `review_queue` does after the model
    ran.  `_similar.DimensionMismatch` when `reviewed` or `triage` hold embeddings of another size than the sites'."""
    lo, hi = float(band[0]), float(band[1])
    if not 0.0 <= lo <= hi <= 1.0:
        raise ValueError(f"review: the uncertainty band must satisfy 0 <= LO <= HI <= 1 (got {lo}, {hi})")
    D = int(sites.rows.shape[1])
    if reviewed is not None and reviewed.dim != D and sites.rows.shape[0]:
        raise S.DimensionMismatch(f"the index holds embeddings of size {reviewed.dim}; the sites' are of size {D}")
    n_sites = int(sites.rows.shape[0])
    keep = np.arange(n_sites)
    if min_confidence is not None:
        with np.errstate(over="ignore"):
            keep = np.flatnonzero(np.exp(sites.logprobs.astype(np.float64)) >= float(min_confidence))
    rows, logprobs = np.ascontiguousarray(sites.rows[keep]), np.ascontiguousarray(sites.logprobs[keep])
    prob = eligible = None
    if triage is not None and keep.shape[0]:
        from buglab.models import triage as T

        scored = T.score_embeddings(triage, rows, logprobs, device, host)
        prob = np.asarray(scored[1] if host else scored[1].cpu().numpy(), np.float64)
        with np.errstate(invalid="ignore"):
            eligible = (prob >= lo) & (prob <= hi)  # a warning without a probability is not one the re-ranker is unsure about
    sel = queue_embeddings(rows, budget, logprobs, None if reviewed is None else reviewed.embeddings, eligible,
                           mean=None if reviewed is None else reviewed.mean, center=center, max_similarity=max_similarity, device=device,
                           host=host)
    L = sel.num_reviewed
    rank_of = {int(s): k for k, s in enumerate(sel.picks)}
    stands_for = sel.stands_for
    out: List[QueuedWarning] = []
    for k, s in enumerate(sel.picks.tolist()):
        b = int(keep[s - L])
        near = int(sel.pick_near[k])
        if near < 0:
            nearest = None
        elif near < L:
            nearest = {"reviewed": reviewed.entry(near), "similarity": float(sel.pick_similarity[k])}
        else:
            nearest = {"rank": rank_of[near], "similarity": float(sel.pick_similarity[k])}
        p = None if prob is None or np.isnan(prob[s - L]) else float(prob[s - L])
        out.append(QueuedWarning(k, int(sites.positions[b]), int(sites.nodes[b]), sites.labels[b], sites.paths[b], sites.packages[b],
                                 float(sites.logprobs[b]), p, nearest, int(stands_for[k])))
    summary = R.report(sel, sites.num_samples, sites.num_rejected, sites.num_without_site, n_sites - keep.shape[0],
                       None if eligible is None else int((~eligible).sum()))
    summary["picked_positions"] = [w.position for w in out]
    if triage is not None:
        summary["uncertainty_band"] = [lo, hi]
    return ReviewQueue(out, summary)


def review_queue(model, nn, data: Iterable[Any], device, budget: int, reviewed: Optional[SiteIndex] = None, triage=None, *,
                 band: Sequence[float] = DEFAULT_BAND, max_similarity: float = 1.0, min_confidence: Optional[float] = None,
                 site: str = "predicted", assume_buggy: bool = False, center: bool = True, host: bool = False,
                 parallelize: bool = True) -> ReviewQueue:
    """The `budget` warnings of `data` a reviewer should look at next, in pick order (module docstring).  `reviewed`: a
    `SiteIndex` of everything accepted or dismissed so far; `triage`: a `_triage.TriageModel`, with `band` the probabilities
    that count as unsure.  The sites are `similar.embed_sites`'.  TypeError for an ensemble or the GREAT var-misuse model;
    ValueError for a similarity outside (0, 1], a band outside [0, 1] or a budget the kernels do not take;
    `_similar.DimensionMismatch` when the index or the triage file hold embeddings of another size, and a logged warning for
    other weights."""
    from buglab.controllers import _batching as Bt

    Bt.require_single_model(model, "review")
    R.stop_of(max_similarity)  # before the model runs
    if not 0 <= int(budget) <= R.MAX_BUDGET:
        raise ValueError(f"review: the budget must be in [0, {R.MAX_BUDGET}] (got {budget})")
    for held in (reviewed, triage):
        if held is not None:
            warning = held.check_model(type(model).__name__, _embedding_dim(nn), S.model_fingerprint(nn))
            if warning:
                LOGGER.warning("%s", warning)
    sites = _embed_sites(model, nn, data, device, site, assume_buggy=assume_buggy, host=host, parallelize=parallelize)
    return review_sites(sites, budget, reviewed=reviewed, triage=triage, band=band, max_similarity=max_similarity,
                        min_confidence=min_confidence, center=center, device=device, host=host)


# ---- command line ------------------------------------------------------------------------------------------------------------
def parse_args(argv=None) -> argparse.Namespace:
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("MODEL", help="A trained detector checkpoint (`*.pkl.gz`).")
    p.add_argument("DATA", help="`*.msgpack.l.gz` data: a file or a folder.")
    p.add_argument("OUT", help="JSON lines, one queued warning per line in pick order (gzip when the name ends in .gz).")
    p.add_argument("--budget", type=int, required=True, help="How many warnings the reviewer will look at.")
    p.add_argument("--reviewed", default=None, help="An index written by `similar index` of everything already accepted or dismissed.")
    p.add_argument("--triage", default=None, help="A file written by `triage fit`: only warnings it is unsure about are queued.")
    p.add_argument("--uncertainty-band", type=float, nargs=2, default=None, metavar=("LO", "HI"),
                   help="The triage probabilities that count as unsure (with --triage; 0.2 0.8 by default).")
    p.add_argument("--max-similarity", type=float, default=1.0, help="End the queue when every warning left is at least this similar to "
                   "something reviewed or queued, in (0, 1].")
    p.add_argument("--min-confidence", type=float, default=None, help="Drop sites whose probability is below this before anything else.")
    p.add_argument("--site", choices=S.SITE_MODES, default="predicted", help="Which location of a sample is its warning.")
    p.add_argument("--assume-buggy", action="store_true", help="Leave NO_BUG out when the site is predicted.")
    p.add_argument("--no-center", action="store_true", help="Do not subtract the mean embedding (without --reviewed).")
    p.add_argument("--limit-num-elements", type=int, default=None, help="Read at most this many samples.")
    p.add_argument("--sequential", action="store_true", help="Do not parallelize data loading.")
    p.add_argument("--host", action="store_true", help="Pick sites and select in the NumPy twin instead of the device kernels.")
    p.add_argument("--report-json", default=None, help="Also write the run's numbers as data.")
    args = p.parse_args(argv)
    if args.uncertainty_band is not None and args.triage is None:
        p.error("--uncertainty-band goes with --triage")
    if args.budget < 0 or args.budget > R.MAX_BUDGET:
        p.error(f"--budget must be in [0, {R.MAX_BUDGET}]")
    return args


def run(args: argparse.Namespace) -> int:
    from buglab.models._triage import TriageModel
    R.stop_of(args.max_similarity)
    model, nn, device, have_gpu = _open_model(args.MODEL)
    reviewed = triage = None
    try:  # before anything is read or run: files of another model's embeddings are the caller's mistake.  Only the SIZE is
        # checked here (each file's own fingerprint is handed back to it, so this call cannot warn): other weights are a
        # warning, which `review_queue` logs with the model's real fingerprint
        if args.reviewed is not None:
            reviewed = SiteIndex.load(args.reviewed)
            reviewed.check_model(type(model).__name__, _embedding_dim(nn), reviewed.fingerprint)
        if args.triage is not None:
            triage = TriageModel.load(args.triage)
            triage.check_model(type(model).__name__, _embedding_dim(nn), triage.fingerprint)
    except S.DimensionMismatch as e:
        print(str(e), file=sys.stderr)
        return EXIT_DIMENSION_MISMATCH
    require_gpu(have_gpu, "review")
    data = _read_data(args.DATA, args.limit_num_elements)
    queue = review_queue(model, nn, data, device, args.budget, reviewed, triage, band=args.uncertainty_band or DEFAULT_BAND,
                         max_similarity=args.max_similarity, min_confidence=args.min_confidence, site=args.site,
                         assume_buggy=args.assume_buggy, center=not args.no_center, host=args.host, parallelize=not args.sequential)
    write_records([w.record() for w in queue.warnings], args.OUT)
    s = queue.summary
    worst, other = s["worst_similarity"], s["most_confident_worst_similarity"]
    text = lambda v: "n/a" if v is None else f"{v:.3f}"
    print(f"review: {s['num_picked']} of {s['num_eligible']} eligible warnings ({s['num_warnings']} of {s['num_samples']} samples, "
          f"{s['num_reviewed']} reviewed before) queued for a budget of {s['budget']}; ended by {s['end']}.  The worst-covered warning "
          f"has cosine {text(worst)} to something reviewed or queued; {text(other)} had the {s['budget']} most confident been "
          f"reviewed instead" + ("" if s["beats_most_confident"] is None else
                                 (": the queue covers better." if s["beats_most_confident"] else ": the queue does not cover better.")))
    write_report_json(args.report_json, s)
    return 0


if __name__ == "__main__":
    sys.exit(run(parse_args()))
