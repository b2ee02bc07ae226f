#!/usr/bin/env python
"""
Usage:
    python -m buglab.models.group MODEL DATA OUT [--similarity 0.9] [--site predicted|truth] [--assume-buggy] [--min-confidence P]
                                  [--no-center] [--index INDEX [--candidates 16]] [--min-group-size 1] [--limit-num-elements N]
                                  [--sequential] [--host] [--report-json FILE]

Warning grouping -- BEYOND THE REFERENCE, which has no counterpart.  A scan of a real code base does not yield a thousand
different warnings but the same few mistakes many times: a copied helper, a vendored file, an idiom the detector dislikes
wherever it occurs.  This groups the warnings of DATA so that a reviewer looks at a pattern once and accepts or dismisses it
as a whole.

A warning is a SITE as `similar` defines it (`--site`, `--assume-buggy`: buglab/models/similar.py), its embedding the row of the
head input behind it.  `--min-confidence P` drops the sites whose exp(log-probability) is below P before grouping.  The groups
are the connected components of "cosine of the centred embeddings >= --similarity" (the embeddings minus their own column mean;
`--no-center`: as they are): SINGLE LINKAGE, so a group is a chain of near-copies and two of its members may be far apart.
That is why every member is listed with its cosine to the group's representative -- a member far from it is how the reader
sees a chain.  The representative is the member with the most links, then the most probable, then the first.

OUT is JSON lines, one group per line, the largest first: an id, the size, the representative's position, node, label,
filename, package and logprob, and the members in input order, each with its position, node, label, filename and `similarity`.
`--min-group-size` leaves smaller groups out of OUT (the report counts them all).  With `--index` the representative of every
listed group is looked up in an index written by `similar index` and its nearest entry added as "resembles"; an index of
embeddings of another size ends the run with status 2, other weights are a warning.

The join is exact: an N x N / 2 integer GEMM on the int8 images (v_mfma_i32_16x16x64_i8) whose epilogue filters, re-scores the
few pairs that pass in fp64 and links them in a lock-free union-find, nothing of size N x N stored (csrc/bl_group.hip; the
arithmetic: include/buglab_hip.h).  `--host` runs the NumPy twin (buglab/models/_group.py); both paths write the same bytes.
"""
from __future__ import annotations

import argparse
import logging
import sys
from pathlib import Path
from typing import Any, Dict, Iterable, List, Optional

if __package__ in (None, ""):
    sys.path.insert(0, str(Path(__file__).resolve().parents[2]))

import numpy as np

from buglab.models import _group as G
from buglab.models import _similar as S
from buglab.models._cli import open_model, read_data, require_gpu, write_records, write_report_json
from buglab.models._group import Grouping, WarningGroup, WarningGroups
from buglab.models._similar import SiteEmbeddings, SiteIndex

LOGGER = logging.getLogger(__name__)
EXIT_DIMENSION_MISMATCH = 2


def _as_array(x) -> np.ndarray:
    return np.ascontiguousarray(x if isinstance(x, np.ndarray) else x.detach().cpu().numpy(), np.float32)


def group_embeddings(rows, similarity: float = 0.9, logprobs=None, *, center: bool = True, device=None, host: bool = False,
                     slices: Optional[int] = None) -> Grouping:
    """The grouping of embeddings that already exist: rows [N, D], fp32, an array or a tensor; `logprobs` [N] breaks ties between
    representatives.  `center` subtracts the rows' own column mean (formed on the host in fp64).  `host`: the NumPy twin, equal
    bit for bit.  ValueError for a similarity outside (0, 1] or sizes the kernels do not take.  Two copies back: the labels, then
    the members' dots with their representatives."""
    G.thresholds(similarity)
    x = _as_array(rows)
    if x.ndim != 2 or not 1 <= x.shape[1] <= S.MAX_D or x.shape[0] > G.MAX_N:
        raise ValueError(f"group: rows {x.shape} must be [N <= {G.MAX_N}, 1 <= D <= {S.MAX_D}]")
    N, D = x.shape
    mean = S.column_mean(x) if center else np.zeros(D, np.float32)
    if N == 0:
        return Grouping(np.zeros(0, np.int32), np.zeros(0, np.int32), 0, 0, [], np.zeros(0, np.float64), np.zeros(0, bool), mean)
    if host:
        label, degree, nc, ne, c, sumsq = G.group_rows_host(x, mean, similarity)
        groups = G.groups_from_labels(label, degree, logprobs)
        rep = _representative_of(groups, N)
        _, dot = S.rescore_host(c, c, sumsq, rep[:, None], 1)
        dot = dot[:, 0]
    else:
        import torch

        from buglab.models import hip_ops

        if device is None:
            device = rows.device if not isinstance(rows, np.ndarray) and rows.is_cuda else "cuda"
        d_x = torch.from_numpy(x).to(device)
        c, q, d_sumsq, r = hip_ops.similar_quantize(d_x, torch.from_numpy(mean).to(device), out_c=d_x)
        parent, d_degree, counters = hip_ops.group_link(c, q, d_sumsq, r, hip_ops.group_row_l1(q), similarity, slices)
        d_label = hip_ops.group_labels(parent)
        # the one copy back of the join: [sumsq | counters | label | degree]
        blob = torch.cat([d_sumsq.view(torch.int32), counters.view(torch.int32), d_label, d_degree]).cpu().numpy()
        sumsq, (nc, ne) = blob[:2 * N].view(np.float64), blob[2 * N:2 * N + 4].view(np.int64).tolist()
        label, degree = blob[2 * N + 4:3 * N + 4], blob[3 * N + 4:]
        groups = G.groups_from_labels(label, degree, logprobs)
        rep = _representative_of(groups, N)
        _, d_dot = hip_ops.similar_rescore(c, c, d_sumsq, torch.from_numpy(rep[:, None]).to(device), 1)
        dot = d_dot[:, 0].cpu().numpy()
    sim = S.similarity(dot, sumsq, sumsq[rep])
    return Grouping(label, degree, int(nc), int(ne), groups, sim, sumsq > 0.0, mean)


def _representative_of(groups: List[G.Members], N: int) -> np.ndarray:
    rep = np.zeros(N, np.int32)
    for g in groups:
        rep[g.members] = g.representative
    return rep


def _resembles(sites: SiteEmbeddings, reps: np.ndarray, index: SiteIndex, candidates: int, device, host: bool) -> List[Optional[Dict[str, Any]]]:
    """the index entry nearest to each of the representatives' embeddings (None: none), with `similar`'s own search"""
    if reps.shape[0] == 0 or index.size == 0:
        return [None] * reps.shape[0]
    x = np.ascontiguousarray(sites.rows[reps])
    if host:
        idx, dot, sx, sy = S.find_neighbours_host(x, index.mean, index.embeddings, 1, candidates)
    else:
        import torch

        from buglab.models import hip_ops

        d_x = torch.from_numpy(x).to(device)
        d_index = torch.from_numpy(np.ascontiguousarray(index.embeddings)).to(device)
        d_mean = torch.from_numpy(np.ascontiguousarray(index.mean)).to(device)
        cx, qx, d_sx, rx = hip_ops.similar_quantize(d_x, d_mean, out_c=d_x)
        cy, qy, d_sy, ry = hip_ops.similar_quantize(d_index, torch.zeros_like(d_mean), out_c=d_index)
        cand, _ = hip_ops.similar_search(qx, rx, qy, ry, candidates)
        d_idx, d_dot = hip_ops.similar_rescore(cx, cy, d_sy, cand, 1)
        idx, dot, sx, sy = d_idx.cpu().numpy(), d_dot.cpu().numpy(), d_sx.cpu().numpy(), d_sy.cpu().numpy()
    sim = S.similarity(dot[:, 0], sx, np.where(idx[:, 0] >= 0, sy[np.maximum(idx[:, 0], 0)], 0.0))
    return [dict(index.entry(i), similarity=float(s)) if i >= 0 else None for i, s in zip(idx[:, 0], sim)]


def group_sites(sites: SiteEmbeddings, similarity: float = 0.9, *, min_confidence: Optional[float] = None, center: bool = True,
                index: Optional[SiteIndex] = None, candidates: int = S.MAX_CANDIDATES, min_group_size: int = 1, device=None,
                host: bool = False) -> WarningGroups:
    """The groups of sites that were embedded already (`similar.embed_sites`): what `group_warnings` does after the model ran."""
    if int(min_group_size) < 1:
        raise ValueError(f"group: --min-group-size must be at least 1 (got {min_group_size})")
    if not 1 <= int(candidates) <= S.MAX_CANDIDATES:
        raise ValueError(f"group: candidates must be in [1, {S.MAX_CANDIDATES}] (got {candidates})")
    n_sites = int(sites.rows.shape[0])
    keep = np.arange(n_sites)
    if min_confidence is not None:
        with np.errstate(over="ignore"):
            keep = np.flatnonzero(np.exp(sites.logprobs.astype(np.float64)) >= float(min_confidence))
    rows, logprobs = np.ascontiguousarray(sites.rows[keep]), sites.logprobs[keep]
    grouping = group_embeddings(rows, similarity, logprobs, center=center, device=device, host=host)
    listed = [g for g in grouping.groups if g.size >= int(min_group_size)]
    reps = keep[np.asarray([g.representative for g in listed], np.int64)]
    resembles = _resembles(sites, reps, index, int(candidates), device, host) if index is not None else [None] * len(listed)

    def site(b: int) -> Dict[str, Any]:
        return {"position": int(sites.positions[b]), "node": int(sites.nodes[b]), "label": sites.labels[b], "filename": sites.paths[b]}

    out: List[WarningGroup] = []
    for number, (g, rep, near) in enumerate(zip(listed, reps, resembles)):
        members = [dict(site(keep[m]), similarity=float(grouping.similarity[m])) for m in g.members]
        head = dict(site(rep), package=sites.packages[rep], logprob=float(sites.logprobs[rep]))
        out.append(WarningGroup(number, g.size, head, members, [sites.scouts[keep[m]] for m in g.members],
                                near if index is not None else None))
    summary = G.report([g.size for g in grouping.groups], [[sites.scouts[keep[m]] for m in g.members] for g in grouping.groups],
                       similarity, sites.num_samples, sites.num_rejected, sites.num_without_site, n_sites - keep.shape[0],
                       int((~grouping.valid).sum()), grouping.num_candidates, grouping.num_edges)
    summary["num_groups_listed"] = len(out)
    return WarningGroups(out, summary)


def group_warnings(model, nn, data: Iterable[Any], device, similarity: float = 0.9, *, site: str = "predicted",
                   assume_buggy: bool = False, min_confidence: Optional[float] = None, center: bool = True,
                   index: Optional[SiteIndex] = None, candidates: int = S.MAX_CANDIDATES, min_group_size: int = 1, host: bool = False,
                   parallelize: bool = True) -> WarningGroups:
    """The warnings of `data` in groups (module docstring).  The sites are `similar.embed_sites`': one launch per predict
    minibatch into run-long buffers, one copy back.  TypeError for an ensemble or the GREAT var-misuse model; ValueError for a
    similarity outside (0, 1]; with `index`, `_similar.DimensionMismatch` when it holds embeddings of another size, and a logged
    warning for other weights."""
    from buglab.controllers import _batching as Bt
    from buglab.models import similar

    Bt.require_single_model(model, "group")
    G.thresholds(similarity)  # before the model runs
    if index is not None:
        warning = index.check_model(type(model).__name__, similar.embedding_dim(nn), S.model_fingerprint(nn))
        if warning:
            LOGGER.warning("%s", warning)
    sites = similar.embed_sites(model, nn, data, device, site, assume_buggy=assume_buggy, host=host, parallelize=parallelize)
    return group_sites(sites, similarity, min_confidence=min_confidence, center=center, index=index, candidates=candidates,
                       min_group_size=min_group_size, device=device, host=host)


# ---- command line ------------------------------------------------------------------------------------------------------------
def parse_args(argv=None) -> argparse.Namespace:
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("MODEL", help="A trained detector checkpoint (`*.pkl.gz`).")
    p.add_argument("DATA", help="`*.msgpack.l.gz` data: a file or a folder.")
    p.add_argument("OUT", help="JSON lines, one group per line (gzip when the name ends in .gz).")
    p.add_argument("--similarity", type=float, default=0.9, help="The cosine at or above which two warnings are linked, in (0, 1].")
    p.add_argument("--site", choices=S.SITE_MODES, default="predicted", help="Which location of a sample is its warning.")
    p.add_argument("--assume-buggy", action="store_true", help="Leave NO_BUG out when the site is predicted.")
    p.add_argument("--min-confidence", type=float, default=None, help="Drop sites whose probability is below this before grouping.")
    p.add_argument("--no-center", action="store_true", help="Do not subtract the mean embedding.")
    p.add_argument("--index", default=None, help="An index written by `similar index`: each group's representative is looked up in it.")
    p.add_argument("--candidates", type=int, default=S.MAX_CANDIDATES, help="Index entries the int8 stage hands to the re-score (with --index).")
    p.add_argument("--min-group-size", type=int, default=1, help="Leave smaller groups out of OUT.")
    p.add_argument("--limit-num-elements", type=int, default=None, help="Read at most this many samples.")
    p.add_argument("--sequential", action="store_true", help="Do not parallelize data loading.")
    p.add_argument("--host", action="store_true", help="Pick sites and group in the NumPy twin instead of the device kernels.")
    p.add_argument("--report-json", default=None, help="Also write the run's numbers as data.")
    return p.parse_args(argv)


def run(args: argparse.Namespace) -> int:
    from buglab.models import similar

    G.thresholds(args.similarity)
    model, nn, device, have_gpu = open_model(args.MODEL)
    index = None
    if args.index is not None:  # before anything is read or run: an index of another model's embeddings is the caller's mistake
        index = SiteIndex.load(args.index)
        try:
            index.check_model(type(model).__name__, similar.embedding_dim(nn), index.fingerprint)
        except S.DimensionMismatch as e:
            print(str(e), file=sys.stderr)
            return EXIT_DIMENSION_MISMATCH
    require_gpu(have_gpu, "group")
    data = read_data(args.DATA, args.limit_num_elements)
    found = group_warnings(model, nn, data, device, args.similarity, site=args.site, assume_buggy=args.assume_buggy,
                           min_confidence=args.min_confidence, center=not args.no_center, index=index, candidates=args.candidates,
                           min_group_size=args.min_group_size, host=args.host, parallelize=not args.sequential)
    write_records([g.record() for g in found.groups], args.OUT)
    s = found.summary
    print(f"group: {s['num_warnings']} warnings of {s['num_samples']} samples in {s['num_groups']} groups at similarity "
          f"{s['similarity']} ({s['num_singletons']} singletons, the largest of {s['largest_group']}; {s['num_edges']} links among "
          f"{s['num_candidates']} candidate pairs); {100.0 * s['spared']:.1f}% of the warnings spared.")
    write_report_json(args.report_json, s)
    return 0


if __name__ == "__main__":
    sys.exit(run(parse_args()))
