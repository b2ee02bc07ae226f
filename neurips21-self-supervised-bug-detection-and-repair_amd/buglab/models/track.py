#!/usr/bin/env python
"""
Usage:
    python -m buglab.models.track MODEL OLD_INDEX DATA OUT [--min-similarity 0.9] [--within none|file|package]
                                  [--site predicted|truth] [--assume-buggy] [--min-confidence P] [--hide-tag TAG ...]
                                  [--write-index NEW_INDEX [--tag TEXT]] [--max-rounds R] [--limit-num-elements N] [--sequential]
                                  [--host] [--report-json FILE]

Warning tracking -- BEYOND THE REFERENCE, which has no counterpart.  Every other scan tool answers a question about ONE scan;
this one connects a scan to the scan before it: which warnings are NEW, which were there last time -- and what the reviewer said
about those -- and which are GONE.  It is the "baseline" or "only new findings" of every static analyser that people keep
running: verdicts carry from revision to revision, a CI job has something to gate on, and a reviewer does not meet the warning
they dismissed last week again.

OLD_INDEX is a `similar index --site predicted` file of the earlier scan; its tags may carry verdicts such as `accepted` and
`dismissed`.  The warnings of DATA are SITES as `similar` defines them (`--site`, `--assume-buggy`), their embeddings centred
with the index's mean, as `similar query` does.  The answer is a ONE-TO-ONE matching between the old entries and the new
warnings: a pair is admissible when the cosine of their int8 images is at least `--min-similarity` and, with `--within file`
or `--within package`, both lie in the same file or package; among the admissible pairs the most similar pair of two still
unmatched warnings is matched, again and again, until none is left (ties: the lower old entry, then the lower new warning).

WHAT A MATCH IS.  A match says "an old warning with an embedding this close was still free" -- not "this is the same line of
code".  `similar query` is one-directional top-k: twenty copies of one pattern in the new scan all find the same old entry, and
one fixed instance among twenty never shows as gone; here every old entry is used once.  The price: a FRESH warning of a pattern
whose old instance was fixed is matched to that old instance and reported as persisting (in an experiment with 2000 old rows in
50 clusters, 10 % dropped and 200 fresh rows, 130 to 141 of the 200 fresh rows were, without keys).  `--within file` is what
narrows it.

OUT is JSON lines: one line per warning of DATA in input order, each with `status` ("new" or "persisting"), position, node,
label, filename, package and logprob, a persisting one also with `previous` -- the index entry with its tag, and the cosine
re-scored in fp64 from the fp32 rows; then one line per unmatched old entry with `status: "gone"`.  `--hide-tag TAG` leaves out
(and counts) the persisting warnings whose previous entry carries one of the tags.  `--write-index NEW_INDEX` writes the new scan
as an index with its own mean: a persisting entry inherits the previous entry's tag, a new one gets `--tag`, so the next run
compares against this file.  The report has the counts of new, persisting, gone and hidden, the same per tag, the rounds, the
floor and `within`, the samples that gave no warning and the lowest listed cosine.

Exit status 0: no new warning.  1: NEW WARNINGS -- a finding, not an error, so a script can gate a merge on it.  2: the index
holds embeddings of another size.  Other weights than the index's are a warning and `"other_weights": true` in the report.
Ensembles and the GREAT var-misuse model are refused, as `similar` refuses them.

The matching runs on the int8 images of `similar`, where dot products are exact integers, in ROUNDS of mutual best: every open
row of either side finds its best admissible open row of the other by an int8 MFMA GEMM that is never stored
(v_mfma_i32_16x16x64_i8), every pair that chose each other is matched, the open rows are compacted, and a round that matches
nothing ends it -- one call enqueues many rounds with no host synchronisation (csrc/bl_track.hip; the arithmetic:
include/buglab_hip.h).  `--host` runs the NumPy twin (buglab/models/_track.py), which orders the pairs instead; both paths write
the same bytes.
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
from buglab.models import _track as T
from buglab.models._cli import embed_sites as _embed_sites, embedding_dim as _embedding_dim, open_model as _open_model
from buglab.models._cli import read_data as _read_data, require_gpu, write_records, write_report_json
from buglab.models._similar import SiteEmbeddings, SiteIndex
from buglab.models._track import Matching, TrackedScan, TrackedWarning

LOGGER = logging.getLogger(__name__)
EXIT_NEW_WARNINGS = 1
EXIT_DIMENSION_MISMATCH = 2
DEFAULT_MAX_ROUNDS = 16  # per call; the driver calls again while the matching has not ended


def _as_array(x) -> np.ndarray:
    return np.ascontiguousarray(x if isinstance(x, np.ndarray) else x.detach().cpu().numpy(), np.float32)


def _match_on_host(y, x, mean, floor, key_old, key_new):
    c_new, q_new, s_new, _ = S.quantize_host(x, mean)
    c_old, q_old, s_old, _ = S.quantize_host(y, np.zeros(y.shape[1], np.float32))
    n_old, n_new = R.norms_host(q_old), R.norms_host(q_new)
    m_old, m_new, m_aff, rounds = T.match_host(q_old, n_old, q_new, n_new, floor, key_old, key_new)
    dot = S.rescore_host(c_new, c_old, s_old, m_new[:, None], 1)[1][:, 0]
    return m_old, m_new, m_aff, rounds, dot, s_old, s_new, n_old, n_new


def _match_on_device(y, x, mean, floor, key_old, key_new, device, max_rounds, slices):
    import torch

    from buglab.models import hip_ops as ops

    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    d_x, d_y = up(x), up(y)
    c_new, q_new, s_new, _ = ops.similar_quantize(d_x, up(mean), out_c=d_x)
    c_old, q_old, s_old, _ = ops.similar_quantize(d_y, torch.zeros(y.shape[1], dtype=torch.float32, device=device), out_c=d_y)
    n_old, n_new = ops.review_norms(q_old), ops.review_norms(q_new)
    L, N = y.shape[0], x.shape[0]
    m_old = torch.full((L,), -1, dtype=torch.int32, device=device)
    m_new = torch.full((N,), -1, dtype=torch.int32, device=device)
    m_aff = torch.zeros(N, dtype=torch.float64, device=device)
    d_ko, d_kn = (None, None) if key_old is None else (up(key_old), up(key_new))
    S_ = ops.track_slices(min(L, N), max(L, N)) if slices is None else int(slices)
    need = int(ops.load_library().bl_track_match_workspace_bytes(L, N, S_))
    workspace = torch.empty((need + 7) // 8, dtype=torch.float64, device=device)
    rounds = 0
    while True:  # one copy back of four words per call: whether to call again
        status = ops.track_match(q_old, n_old, q_new, n_new, floor, m_old, m_new, m_aff, max_rounds=max_rounds, key_old=d_ko, key_new=d_kn,
                                 slices=S_, workspace=workspace).cpu().numpy()
        rounds += int(status[0])
        if status[2]:
            break
    dot = ops.similar_rescore(c_new, c_old, s_old, m_new[:, None].contiguous(), 1)[1][:, 0]
    # the last copy back: [match_aff | dot | sumsq_new | sumsq_old] as one float64 blob, [match_old | match_new | norms] as int32
    f64 = torch.cat([m_aff, dot, s_new, s_old]).cpu().numpy()
    i32 = torch.cat([m_old, m_new, n_old, n_new]).cpu().numpy()
    return (i32[:L], i32[L:L + N], f64[:N], rounds, f64[N:2 * N], f64[3 * N:], f64[2 * N:3 * N], i32[L + N:2 * L + N], i32[2 * L + N:])


def match_embeddings(old_rows, new_rows, *, mean=None, min_similarity: float = 0.9, old_keys=None, new_keys=None, device=None,
                     host: bool = False, max_rounds: Optional[int] = None, slices: Optional[int] = None) -> Matching:
    """The one-to-one matching (module docstring) of embeddings that already exist: old_rows [L, D], fp32, CENTRED (a
    `SiteIndex`'s embeddings); new_rows [N, D], from which `mean` (the index's; None: nothing) is subtracted.  `old_keys` /
    `new_keys`: int32 per row, both or neither -- only rows of equal keys match.  `host`: the NumPy twin, equal bit for bit.
    `max_rounds`: rounds per device call (the driver copies four status words back per call and calls again while the matching
    has not ended); `slices`: a launch detail of the device path -- the result depends on neither.  ValueError for a similarity
    outside (0, 1] or sizes the kernels do not take, `_similar.DimensionMismatch` for rows of two sizes."""
    floor = T.floor_of(min_similarity)
    rounds_per_call = DEFAULT_MAX_ROUNDS if max_rounds is None else int(max_rounds)
    if not 1 <= rounds_per_call <= T.MAX_ROUNDS:
        raise ValueError(f"track: --max-rounds must be in [1, {T.MAX_ROUNDS}] (got {max_rounds})")
    x, y = _as_array(new_rows), _as_array(old_rows)
    if x.ndim != 2 or y.ndim != 2 or not 1 <= x.shape[1] <= S.MAX_D:
        raise ValueError(f"track: rows {y.shape} and {x.shape} must be [L, D] and [N, 1 <= D <= {S.MAX_D}]")
    if y.shape[1] != x.shape[1]:
        if x.shape[0] and y.shape[0]:
            raise S.DimensionMismatch(f"the old rows hold embeddings of size {y.shape[1]}; the new ones are of size {x.shape[1]}")
        y = np.zeros((y.shape[0], x.shape[1]), np.float32) if not y.shape[0] else y
        x = np.zeros((0, y.shape[1]), np.float32) if not x.shape[0] else x
    L, N = y.shape[0], x.shape[0]
    if L > T.MAX_ROWS or N > T.MAX_ROWS:
        raise ValueError(f"track: {L} old and {N} new rows are above {T.MAX_ROWS} rows a side")
    if (old_keys is None) != (new_keys is None):
        raise ValueError("track: the keys of both sides come together")
    if old_keys is not None:
        old_keys, new_keys = np.ascontiguousarray(old_keys, np.int32).reshape(-1), np.ascontiguousarray(new_keys, np.int32).reshape(-1)
        if old_keys.shape != (L,) or new_keys.shape != (N,):
            raise ValueError(f"track: keys {old_keys.shape} / {new_keys.shape} must be [{L}] / [{N}]")
    mean = np.zeros(x.shape[1], np.float32) if mean is None else np.ascontiguousarray(mean, np.float32).reshape(-1)
    if mean.shape != (x.shape[1],):
        raise S.DimensionMismatch(f"the mean is of size {mean.shape[0]}; the rows are of size {x.shape[1]}")
    if L == 0 or N == 0:  # nothing can match; a side without rows has nothing to quantise
        valid = lambda rows, m: S.quantize_host(rows, m)[2] > 0.0
        return Matching(np.full(L, -1, np.int32), np.full(N, -1, np.int32), np.zeros(N), np.zeros(N), 0, floor,
                        valid(y, np.zeros(y.shape[1], np.float32)), valid(x, mean))
    if host:
        out = _match_on_host(y, x, mean, floor, old_keys, new_keys)
    else:
        if device is None:
            device = new_rows.device if not isinstance(new_rows, np.ndarray) and new_rows.is_cuda else "cuda"
        out = _match_on_device(y, x, mean, floor, old_keys, new_keys, device, rounds_per_call, slices)
    m_old, m_new, m_aff, rounds, dot, s_old, s_new, n_old, n_new = out
    m_old, m_new = np.asarray(m_old, np.int32), np.asarray(m_new, np.int32)
    sim = S.similarity(dot, s_new, np.where(m_new >= 0, s_old[np.maximum(m_new, 0)], 0.0))
    return Matching(m_old, m_new, np.asarray(m_aff, np.float64), np.asarray(sim, np.float64), int(rounds), floor,
                    np.asarray(n_old) > 0, np.asarray(n_new) > 0)


def track_sites(sites: SiteEmbeddings, index: SiteIndex, *, min_similarity: float = 0.9, within: str = "none",
                min_confidence: Optional[float] = None, hide_tags: Sequence[str] = (), tag: Optional[str] = None, device=None,
                host: bool = False, max_rounds: Optional[int] = None, model_class: Optional[str] = None,
                fingerprint: Optional[str] = None, other_weights: bool = False) -> TrackedScan:
    """Tracks sites that were embedded already (`similar.embed_sites`) against `index`: what `track_warnings` does after the model
    ran.  `model_class` / `fingerprint`: what the new index records (the old index's when None).  `_similar.DimensionMismatch`
    when the index holds embeddings of another size than the sites'."""
    D = int(sites.rows.shape[1])
    if index.dim != D and sites.rows.shape[0]:
        raise S.DimensionMismatch(f"the index holds embeddings of size {index.dim}; the sites' are of size {D}")
    n_sites = int(sites.rows.shape[0])
    if n_sites == 0:  # no site has a size to disagree with: the new index keeps the old one's
        D = index.dim
    keep = np.arange(n_sites)
    if min_confidence is not None:
        with np.errstate(over="ignore"):
            keep = np.flatnonzero(np.exp(sites.logprobs.astype(np.float64)) >= float(min_confidence))
    pick = lambda values: [values[b] for b in keep]
    kept = SiteEmbeddings(np.ascontiguousarray(sites.rows[keep]).reshape(len(keep), D), np.asarray(sites.positions)[keep],
                          np.asarray(sites.nodes)[keep], np.asarray(sites.logprobs)[keep], pick(sites.labels), pick(sites.paths),
                          pick(sites.packages), pick(sites.scouts), sites.num_samples, sites.num_rejected, sites.num_without_site)
    key_old, key_new = T.within_keys(within, index.paths.tolist(), index.packages.tolist(), kept.paths, kept.packages)
    matching = match_embeddings(index.embeddings, kept.rows, mean=index.mean, min_similarity=min_similarity, old_keys=key_old,
                                new_keys=key_new, device=device, host=host, max_rounds=max_rounds)
    hide = {str(t) for t in hide_tags}
    listed: List[TrackedWarning] = []
    hidden: List[TrackedWarning] = []
    tags: List[str] = []
    for s in range(len(keep)):
        i = int(matching.match_new[s])
        previous = None if i < 0 else {**index.entry(i), "similarity": float(matching.similarity[s])}
        w = TrackedWarning(T.STATUS_NEW if i < 0 else T.STATUS_PERSISTING, int(kept.positions[s]), int(kept.nodes[s]), kept.labels[s],
                           kept.paths[s], kept.packages[s], float(kept.logprobs[s]), previous, (tag or "") if i < 0 else str(index.tags[i]))
        tags.append(w.tag)
        (hidden if i >= 0 and w.tag in hide else listed).append(w)
    for i in np.flatnonzero(matching.match_old < 0).tolist():
        e = index.entry(i)
        listed.append(TrackedWarning(T.STATUS_GONE, e["position"], e["node"], e["label"], e["filename"], e["package"], None, e, e["tag"]))
    new_index = S.make_index(kept, None, True, model_class or index.model_class, fingerprint or index.fingerprint)
    new_index = new_index._replace(tags=S._text(tags))
    summary = T.report(listed, hidden, matching, within, sites.num_samples, sites.num_rejected, sites.num_without_site,
                       n_sites - len(keep), other_weights)
    return TrackedScan(listed, summary, new_index, hidden)


def track_warnings(model, nn, index: SiteIndex, data: Iterable[Any], device, min_similarity: float = 0.9, within: str = "none", *,
                   site: str = "predicted", assume_buggy: bool = False, min_confidence: Optional[float] = None,
                   hide_tags: Sequence[str] = (), tag: Optional[str] = None, max_rounds: Optional[int] = None, host: bool = False,
                   parallelize: bool = True) -> TrackedScan:
    """The warnings of `data` against the earlier scan in `index` (module docstring): new, persisting (with the previous entry and
    its tag) and gone, and the new scan as an index whose tags are inherited.  The sites are `similar.embed_sites`'.  TypeError
    for an ensemble or the GREAT var-misuse model; ValueError for a similarity outside (0, 1] or an unknown `within`;
    `_similar.DimensionMismatch` when the index holds embeddings of another size, and a logged warning for other weights."""
    from buglab.controllers import _batching as Bt

    Bt.require_single_model(model, "track")
    T.floor_of(min_similarity)  # before the model runs
    if within not in T.WITHIN:
        raise ValueError(f"track: --within must be one of {T.WITHIN} (got {within!r})")
    fingerprint = S.model_fingerprint(nn)
    warning = index.check_model(type(model).__name__, _embedding_dim(nn), fingerprint)
    if warning:
        LOGGER.warning("%s", warning)
    sites = _embed_sites(model, nn, data, device, site, assume_buggy=assume_buggy, host=host, parallelize=parallelize)
    return track_sites(sites, index, min_similarity=min_similarity, within=within, min_confidence=min_confidence, hide_tags=hide_tags,
                       tag=tag, device=device, host=host, max_rounds=max_rounds, model_class=type(model).__name__,
                       fingerprint=fingerprint, other_weights=warning is not None)


# ---- command line ------------------------------------------------------------------------------------------------------------
def parse_args(argv=None) -> argparse.Namespace:
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("MODEL", help="A trained detector checkpoint (`*.pkl.gz`).")
    p.add_argument("OLD_INDEX", help="An index written by `similar index --site predicted` (or by --write-index) of the earlier scan.")
    p.add_argument("DATA", help="`*.msgpack.l.gz` data: a file or a folder.")
    p.add_argument("OUT", help="JSON lines: the warnings of DATA in input order, then the gone ones (gzip when the name ends in .gz).")
    p.add_argument("--min-similarity", type=float, default=0.9, help="The least cosine (of the int8 images) of a match, in (0, 1].")
    p.add_argument("--within", choices=T.WITHIN, default="none", help="Only match warnings of the same file or package.")
    p.add_argument("--site", choices=S.SITE_MODES, default="predicted", help="Which location of a sample is its warning.")
    p.add_argument("--assume-buggy", action="store_true", help="Leave NO_BUG out when the site is predicted.")
    p.add_argument("--min-confidence", type=float, default=None, help="Drop sites whose probability is below this before anything else.")
    p.add_argument("--hide-tag", action="append", default=[], metavar="TAG",
                   help="Leave out (and count) persisting warnings whose previous entry carries this tag; may be repeated.")
    p.add_argument("--write-index", default=None, metavar="NEW_INDEX", help="Write the new scan as an index; tags are inherited.")
    p.add_argument("--tag", default=None, help="The tag of a new warning in NEW_INDEX (with --write-index).")
    p.add_argument("--max-rounds", type=int, default=None, help=f"Rounds per device call ({DEFAULT_MAX_ROUNDS} by default).")
    p.add_argument("--limit-num-elements", type=int, default=None, help="Read at most this many samples.")
    p.add_argument("--sequential", action="store_true", help="Do not parallelize data loading.")
    p.add_argument("--host", action="store_true", help="Pick sites and match in the NumPy twin instead of the device kernels.")
    p.add_argument("--report-json", default=None, help="Also write the run's numbers as data.")
    args = p.parse_args(argv)
    if args.tag is not None and args.write_index is None:
        p.error("--tag goes with --write-index")
    if args.max_rounds is not None and not 1 <= args.max_rounds <= T.MAX_ROUNDS:
        p.error(f"--max-rounds must be in [1, {T.MAX_ROUNDS}]")
    return args


def run(args: argparse.Namespace) -> int:
    T.floor_of(args.min_similarity)
    model, nn, device, have_gpu = _open_model(args.MODEL)
    try:  # before anything is read or run: an index of another model's embeddings is the caller's mistake.  Only the SIZE is checked
        # here (the index's own fingerprint is handed back to it, so this call cannot warn): `track_warnings` warns of other weights
        index = SiteIndex.load(args.OLD_INDEX)
        index.check_model(type(model).__name__, _embedding_dim(nn), index.fingerprint)
    except S.DimensionMismatch as e:
        print(str(e), file=sys.stderr)
        return EXIT_DIMENSION_MISMATCH
    require_gpu(have_gpu, "track")
    data = _read_data(args.DATA, args.limit_num_elements)
    scan = track_warnings(model, nn, index, data, device, args.min_similarity, args.within, site=args.site, assume_buggy=args.assume_buggy,
                          min_confidence=args.min_confidence, hide_tags=args.hide_tag, tag=args.tag, max_rounds=args.max_rounds,
                          host=args.host, parallelize=not args.sequential)
    write_records([w.record() for w in scan.warnings], args.OUT)
    if args.write_index is not None:
        scan.index.save(args.write_index)
    s = scan.summary
    low = s["lowest_listed_similarity"]
    print(f"track: {s['num_new']} new, {s['num_persisting']} persisting ({s['num_hidden']} more hidden) and {s['num_gone']} gone: "
          f"{s['num_warnings']} warnings of {s['num_samples']} samples against {s['num_old']} earlier ones, matched in {s['rounds']} rounds at "
          f"cosine >= {s['min_similarity']:g} within {s['within']}; the lowest listed cosine is {'n/a' if low is None else f'{low:.3f}'}.")
    write_report_json(args.report_json, s)
    return EXIT_NEW_WARNINGS if s["num_new"] else 0


if __name__ == "__main__":
    sys.exit(run(parse_args()))
