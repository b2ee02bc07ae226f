#!/usr/bin/env python
"""
Usage:
    python -m buglab.models.similar index MODEL DATA OUT_INDEX [--site truth|predicted] [--assume-buggy] [--tag TEXT] [--no-center]
                                          [--limit-num-elements N] [--sequential] [--host]
    python -m buglab.models.similar query MODEL INDEX DATA OUT [--top-k 5] [--candidates 16] [--site predicted|truth] [--assume-buggy]
                                          [--min-similarity S] [--limit-num-elements N] [--sequential] [--host] [--report-json FILE]

Similar-bug search -- BEYOND THE REFERENCE, which has no counterpart.  "Have we seen this before?": which known bugs a warning
resembles, and which warnings like it somebody already dismissed.

A SITE is one candidate location of one sample, and its embedding the row of the head input behind that candidate -- what the
localisation head scores.  `--site truth` takes the true bug's location (samples without a bug or a label have no site),
`--site predicted` the most probable location (the first maximum in canonical order; a sample whose most probable entry is NO_BUG
raises no warning and has no site; `--assume-buggy` leaves NO_BUG out).  Samples without a site are counted; they produce no
index entry and no query record.

`index` writes one .npz file: the centred fp32 embeddings, the mean that was subtracted (`--no-center`: zeros), and per entry
the input position, the site's node and its label, the file, the package, the scout of the true rewrite (empty for predicted
sites) and the --tag ("known-bug", "false-alarm", ...); and the model's class, the embedding size and a SHA-1 of its weights.
`query` exits with status 2 when the model's embeddings are of another size than the index's, and warns when the weights differ.

`query` writes one JSON line per sample with a site: position, node, label, the site's log-probability, and up to --top-k
neighbours in order -- index entry, cosine similarity and the entry's metadata; --min-similarity drops neighbours below it after
the search.  The search has two stages (the arithmetic: include/buglab_hip.h): the exact top --candidates of every query on the
int8 images of the embeddings (v_mfma_i32_16x16x64_i8), then an fp64 re-score that makes the listed cosines exact and exactly
ordered.  What the int8 stage can lose is a true neighbour outside the first --candidates: measured
recall@5 against fp64 brute force is 1.0 with 16 candidates and 0.98 with 5 (synthetic rows and an untrained model's
embeddings; a trained model's have not been measured).

Two paths give the same records bit for bit.  The default leaves the model's flat output and the head input on the device: one
hip_ops.similar_embed_sites launch per predict minibatch into run-long buffers, then one quantise launch, one search, one
re-score (csrc/bl_similar.hip) and one copy back.  `--host` copies each minibatch's flat output and candidate rows back and does
the rest in the NumPy twin (buglab/models/_similar.py).
"""
from __future__ import annotations

import argparse
import logging
import sys
from pathlib import Path
from typing import Any, Dict, Iterable, Iterator, List, NamedTuple, Optional, Tuple

if __package__ in (None, ""):
    sys.path.insert(0, str(Path(__file__).resolve().parents[2]))

import numpy as np

from buglab.models import _similar as S
from buglab.models._cli import open_model, read_data, require_gpu, write_records, write_report_json
from buglab.models._similar import Neighbours, SiteEmbeddings, SiteIndex

LOGGER = logging.getLogger(__name__)
EXIT_DIMENSION_MISMATCH = 2


class _Sites(NamedTuple):
    """Every sample `tensorize` accepted, in input order; place -1: no site."""

    positions: List[int]
    points: List[Any]
    rows: Any        # float32 [n, D]: a device tensor on the device path, an array on the host path (None: nothing was accepted)
    place: Any       # int32 [n]
    logprob: Any     # float32 [n]
    num_samples: int
    num_rejected: int


def _flat_and_head(nn, mb):
    """The minibatch's flat output, the head input, and the candidates' rows in it (the forward's own, not recomputed)."""
    import torch

    from buglab.controllers import _batching as Bt

    flat, enc_out = Bt.flat_prediction_output_and_encoding(nn, mb)
    h, refs = nn._head_inputs(enc_out)
    return flat, h.detach().float(), refs["candidate_nodes"].to(torch.int32)


def embedding_dim(nn) -> int:
    """The size of a site embedding: the width of the head input, which is what the localisation head's score vector spans."""
    return int(nn._localization_module.w.shape[0])


def _collect_sites(model, nn, data: Iterable[Any], device, site: str, assume_buggy: bool, host: bool, parallelize: bool,
                   capacity: Optional[int] = None) -> _Sites:
    import torch

    from buglab.controllers import _batching as Bt
    from buglab.models import hip_ops

    if site not in S.SITE_MODES:
        raise ValueError(f"site must be one of {S.SITE_MODES} (got {site!r})")
    device = torch.device(device)
    refused: List[int] = []
    seen = [0]

    def tagged():
        for position, point in enumerate(data):
            seen[0] += 1
            yield point, position

    def extend(layout, points, dev):
        arrays = [layout.loc_idx, layout.loc_off, np.asarray([S.truth_place(p) for p in points], np.int32)]
        loc_idx, loc_off, truth = arrays if host else Bt.to_device_i32(arrays, dev)
        return {"loc_idx": loc_idx, "loc_off": loc_off, "truth": truth, "points": points}

    cols = None if host else Bt.RunColumns(device, Bt.run_capacity(capacity, data, 1 << 12),
                                           [("rows", "float32", (Bt.SAMPLES, embedding_dim(nn))), ("place", "int32", (Bt.SAMPLES,)),
                                            ("logprob", "float32", (Bt.SAMPLES,))])
    rows = place = logprob = None
    host_parts: List[Tuple[np.ndarray, np.ndarray, np.ndarray]] = []
    positions: List[int] = []
    points: List[Any] = []
    nn.eval()
    with torch.no_grad(), model._tensorize_all_location_rewrites():
        for mb, tags in Bt.prediction_minibatches(model, tagged(), device, parallelize, extend, refused.append):
            flat, h, cand = _flat_and_head(nn, mb)
            ix = mb["selfsup"]
            B = len(tags)
            truth = ix["truth"] if site == "truth" else None
            if host:  # the minibatch's flat output and candidate rows come back; the twin does the rest
                h_cand = h[cand.long()].cpu().numpy()
                host_parts.append(S.embed_sites_host(flat.cpu().numpy(), ix["loc_idx"], ix["loc_off"], np.arange(h_cand.shape[0]), h_cand,
                                                     site, truth, assume_buggy))
            else:
                n = cols.reserve(B)
                hip_ops.similar_embed_sites(flat, ix["loc_idx"], ix["loc_off"], cand, h, cols["rows"], cols["place"], cols["logprob"], n,
                                            mode=site, truth=truth, skip_nobug=assume_buggy)
            positions.extend(tags), points.extend(ix["points"])
    if host and host_parts:
        rows, place, logprob = (np.concatenate([p[i] for p in host_parts]) for i in range(3))
    elif positions:  # (nothing accepted: no rows, as on the host path)
        rows, place, logprob = cols.device_columns().values()
    return _Sites(positions, points, rows, place, logprob, seen[0], len(refused))


def _with_metadata(found: _Sites, rows: np.ndarray, place: np.ndarray, logprob: np.ndarray, site: str) -> SiteEmbeddings:
    """the samples with a site, and what the records say about them"""
    keep = np.flatnonzero(place >= 0)
    meta = [S.site_metadata(found.points[b], place[b]) for b in keep]
    scouts = [S.true_scout(found.points[b]) if site == "truth" else "" for b in keep]
    return SiteEmbeddings(np.ascontiguousarray(rows[keep]), np.asarray([found.positions[b] for b in keep], np.int64),
                          np.asarray([m[0] for m in meta], np.int32), np.ascontiguousarray(logprob[keep]), [m[1] for m in meta],
                          [m[2] for m in meta], [m[3] for m in meta], scouts, found.num_samples, found.num_rejected,
                          len(found.positions) - keep.shape[0])


def _copy_back(found: _Sites, D_if_empty: int = 1) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """the one copy back (and the one synchronisation) of an embedding run: [rows | places | log-probabilities]"""
    import torch

    if found.rows is None:
        return np.zeros((0, D_if_empty), np.float32), np.zeros(0, np.int32), np.zeros(0, np.float32)
    if isinstance(found.rows, np.ndarray):
        return found.rows, found.place, found.logprob
    n, D = found.rows.shape
    blob = torch.cat([found.rows.reshape(-1).view(torch.int32), found.place, found.logprob.view(torch.int32)]).cpu()
    return (blob[:n * D].view(torch.float32).numpy().reshape(n, D), blob[n * D:n * D + n].numpy(),
            blob[n * D + n:].view(torch.float32).numpy())


def embed_sites(model, nn, data: Iterable[Any], device, site: str = "predicted", *, assume_buggy: bool = False, host: bool = False,
                parallelize: bool = True) -> SiteEmbeddings:
    """The site embeddings of `data` (module docstring), one entry per sample with a site, in input order.  The rows stay on the
    device for the run and are copied back once; `host` copies every minibatch back and picks the sites in the twin."""
    from buglab.controllers import _batching as Bt

    Bt.require_single_model(model, "similar")
    found = _collect_sites(model, nn, data, device, site, assume_buggy, host, parallelize)
    return _with_metadata(found, *_copy_back(found), site)


def build_site_index(model, nn, data: Iterable[Any], device, site: str = "truth", tag: Optional[str] = None, center: bool = True, *,
                     assume_buggy: bool = False, host: bool = False, parallelize: bool = True) -> SiteIndex:
    """An index of the sites of `data`: their embeddings minus their mean (`center`; the mean is computed on the host in fp64
    from the rows, which are copied back once) and the metadata of every entry.  TypeError for an ensemble or the GREAT
    var-misuse model."""
    sites = embed_sites(model, nn, data, device, site, assume_buggy=assume_buggy, host=host, parallelize=parallelize)
    return S.make_index(sites, tag, center, type(model).__name__, S.model_fingerprint(nn))


class Search(NamedTuple):
    found: List[Neighbours]
    summary: Dict[str, Any]


def search_similar(model, nn, index: SiteIndex, data: Iterable[Any], device, k: int = 5, candidates: int = S.MAX_CANDIDATES, *,
                   site: str = "predicted", assume_buggy: bool = False, min_similarity: Optional[float] = None, host: bool = False,
                   parallelize: bool = True, capacity: Optional[int] = None) -> Search:
    """`find_similar` as a list, with the run's numbers (`_similar.report`)."""
    import torch

    from buglab.controllers import _batching as Bt

    Bt.require_single_model(model, "similar")
    k, C = int(k), int(candidates)
    if not 1 <= C <= S.MAX_CANDIDATES or not 1 <= k <= C:
        raise ValueError(f"similar: need 1 <= k <= candidates <= {S.MAX_CANDIDATES} (got k {k}, candidates {candidates})")
    warning = index.check_model(type(model).__name__, embedding_dim(nn), S.model_fingerprint(nn))  # DimensionMismatch before any work
    if warning:
        LOGGER.warning("%s", warning)
    found = _collect_sites(model, nn, data, device, site, assume_buggy, host, parallelize, capacity)
    n = len(found.positions)
    assert n == 0 or int(found.rows.shape[1]) == index.dim
    if n == 0:
        place, logprob = np.zeros(0, np.int32), np.zeros(0, np.float32)
        idx, sim, valid = np.zeros((0, k), np.int32), np.zeros((0, k), np.float64), np.zeros(0, bool)
    elif host:
        place, logprob = found.place, found.logprob
        idx, dot, sx, sy = S.find_neighbours_host(found.rows, index.mean, index.embeddings, k, C)
        sim, valid = S.similarity(dot, sx[:, None], np.where(idx >= 0, sy[np.maximum(idx, 0)] if index.size else 0.0, 0.0)), sx > 0.0
    else:
        from buglab.models import hip_ops

        dev = found.rows.device
        N = index.size
        d_index = torch.from_numpy(np.ascontiguousarray(index.embeddings)).to(dev)
        d_mean = torch.from_numpy(np.ascontiguousarray(index.mean)).to(dev)
        # one launch quantises the queries (centred in place) and one the index (the int8 image is not stored: rebuilt here)
        cx, qx, sx, rx = hip_ops.similar_quantize(found.rows, d_mean, out_c=found.rows)
        cy, qy, sy, ry = hip_ops.similar_quantize(d_index, torch.zeros_like(d_mean), out_c=d_index)
        cand, _ = hip_ops.similar_search(qx, rx, qy, ry, C)
        d_idx, d_dot = hip_ops.similar_rescore(cx, cy, sy, cand, k)
        d_sy = sy[d_idx.clamp(min=0).long()] if N else torch.zeros_like(d_dot)
        # the one copy back (and the one synchronisation) of the run: [dots | sumsq_y of the neighbours | sumsq_x | idx | place | logprob]
        blob = torch.cat([d_dot.reshape(-1).view(torch.int32), d_sy.reshape(-1).view(torch.int32), sx.view(torch.int32), d_idx.reshape(-1),
                          found.place, found.logprob.view(torch.int32)]).cpu()
        f64 = blob[:2 * (2 * n * k + n)].view(torch.float64).numpy()
        dot, sy_of, sx_h = f64[:n * k].reshape(n, k), f64[n * k:2 * n * k].reshape(n, k), f64[2 * n * k:]
        rest = blob[2 * (2 * n * k + n):]
        idx, place, logprob = rest[:n * k].numpy().reshape(n, k), rest[n * k:n * k + n].numpy(), rest[n * k + n:].view(torch.float32).numpy()
        sim, valid = S.similarity(dot, sx_h[:, None], np.where(idx >= 0, sy_of, 0.0)), sx_h > 0.0
    out: List[Neighbours] = []
    for b in np.flatnonzero(place >= 0):
        point = found.points[b]
        node, label, _, _ = S.site_metadata(point, place[b])
        out.append(Neighbours(int(found.positions[b]), node, label, float(logprob[b]), S.true_scout(point), bool(valid[b]),
                              S.neighbour_list(index, idx[b], sim[b], min_similarity)))
    return Search(out, S.report(out, found.num_samples, found.num_rejected, n - len(out)))


def find_similar(model, nn, index: SiteIndex, data: Iterable[Any], device, k: int = 5, candidates: int = S.MAX_CANDIDATES,
                 **options) -> Iterator[Neighbours]:
    """For every sample of `data` with a site, in input order: its `k` nearest index entries by the cosine of the centred
    embeddings, searched among the first `candidates` of the int8 stage (module docstring).  Options: site, assume_buggy,
    min_similarity, host, parallelize.  TypeError for an ensemble or the GREAT var-misuse model, `_similar.DimensionMismatch`
    when the index holds embeddings of another size; other weights than the index's are logged as a warning."""
    from buglab.controllers import _batching as Bt

    Bt.require_single_model(model, "similar")  # now, not at the first next()
    return iter(search_similar(model, nn, index, data, device, k, candidates, **options).found)


# ---- command line ------------------------------------------------------------------------------------------------------------
def parse_args(argv=None) -> argparse.Namespace:
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = p.add_subparsers(dest="command", required=True)
    index = sub.add_parser("index", help="Embed the sites of DATA and write an index of them.")
    index.add_argument("MODEL", help="A trained detector checkpoint (`*.pkl.gz`).")
    index.add_argument("DATA", help="`*.msgpack.l.gz` data: a file or a folder.")
    index.add_argument("OUT_INDEX", help="The index file to write (.npz).")
    index.add_argument("--site", choices=S.SITE_MODES, default="truth", help="Which location of a sample is indexed.")
    index.add_argument("--tag", default=None, help="A label every entry carries, such as known-bug or false-alarm.")
    index.add_argument("--no-center", action="store_true", help="Do not subtract the mean embedding.")
    query = sub.add_parser("query", help="List the index entries nearest to the sites of DATA.")
    query.add_argument("MODEL", help="The checkpoint the index was built with.")
    query.add_argument("INDEX", help="An index written by `index`.")
    query.add_argument("DATA", help="`*.msgpack.l.gz` data to look up: a file or a folder.")
    query.add_argument("OUT", help="JSON lines, one record per sample with a site (gzip when the name ends in .gz).")
    query.add_argument("--site", choices=S.SITE_MODES, default="predicted", help="Which location of a sample is looked up.")
    query.add_argument("--top-k", type=int, default=5, help="Neighbours listed per sample (<= --candidates).")
    query.add_argument("--candidates", type=int, default=S.MAX_CANDIDATES,
                       help=f"Index entries the int8 stage hands to the fp64 re-score, 1 .. {S.MAX_CANDIDATES}.  A true neighbour the int8 "
                            "keys rank below this many others is lost: measured recall@5 is 1.0 at 16, 0.9998 to 1.0 at 8 and 0.98 at 5 "
                            "(DESIGN.md; synthetic rows and an untrained model's embeddings).")
    query.add_argument("--min-similarity", type=float, default=None, help="Drop neighbours below this cosine after the search.")
    query.add_argument("--report-json", default=None, help="Also write the run's numbers as data.")
    for s in (index, query):
        s.add_argument("--assume-buggy", action="store_true", help="Leave NO_BUG out when the site is predicted.")
        s.add_argument("--host", action="store_true", help="Pick sites and search in the NumPy twin instead of the device kernels.")
        s.add_argument("--limit-num-elements", type=int, default=None, help="Read at most this many samples.")
        s.add_argument("--sequential", action="store_true", help="Do not parallelize data loading.")
    return p.parse_args(argv)


def run(args: argparse.Namespace) -> int:
    model, nn, device, have_gpu = open_model(args.MODEL)
    if args.command == "query":  # before anything is read or run: an index of another model's embeddings is the caller's mistake
        index = SiteIndex.load(args.INDEX)
        try:
            index.check_model(type(model).__name__, embedding_dim(nn), index.fingerprint)
        except S.DimensionMismatch as e:
            print(str(e), file=sys.stderr)
            return EXIT_DIMENSION_MISMATCH
    require_gpu(have_gpu, "similar")
    data = read_data(args.DATA, args.limit_num_elements)
    options = dict(assume_buggy=args.assume_buggy, host=args.host, parallelize=not args.sequential)
    if args.command == "index":
        index = build_site_index(model, nn, data, device, args.site, args.tag, not args.no_center, **options)
        index.save(args.OUT_INDEX)
        print(f"similar index: {index.size} entries of size {index.dim} from {len(data)} samples ({args.site} sites).")
        return 0
    found = search_similar(model, nn, index, data, device, args.top_k, args.candidates, site=args.site,
                           min_similarity=args.min_similarity, **options)
    write_records([f.record() for f in found.found], args.OUT)
    s = found.summary
    print(f"similar query: {s['num_with_site']} of {s['num_samples']} samples have a site ({s['num_rejected']} rejected, "
          f"{s['num_invalid_embeddings']} invalid embeddings); {s['num_with_neighbours']} have neighbours.")
    write_report_json(args.report_json, s)
    return 0


if __name__ == "__main__":
    sys.exit(run(parse_args()))
