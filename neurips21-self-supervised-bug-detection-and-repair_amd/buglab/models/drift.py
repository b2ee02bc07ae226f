#!/usr/bin/env python
"""
Usage:
    python -m buglab.models.drift MODEL INDEX DATA OUT [--num-permutations 1000] [--seed 0] [--alpha 0.05] [--bandwidth-scale 1.0]
                                  [--top-k 20] [--site predicted|truth] [--assume-buggy] [--max-reference N]
                                  [--limit-num-elements N] [--sequential] [--host] [--report-json FILE]

Drift detection -- BEYOND THE REFERENCE, which has no counterpart.  A fitted temperature, ensemble weight, warning threshold,
FDR reference or site index is valid only while the code being scanned looks like the code it was fitted on; this is the test of
that assumption.  It compares the site embeddings (buglab/models/similar.py: the row of the head input behind a sample's site)
of a reference, a SiteIndex written by `similar index`, with those of DATA: a two-sample permutation test of the kernel maximum
mean discrepancy with an RBF kernel whose bandwidth is --bandwidth-scale times the mean squared distance of the pooled rows
(the statistic, the subsets and the arithmetic: include/buglab_hip.h).

OUT gets one JSON line per listed outlier, the --top-k scanned samples with the most negative witness value -- those least like
the reference: position, witness, node, label, file, package, scout.  --report-json gets the run's numbers: n, m, D, the
bandwidth, MMD2, the p-value, the verdict at --alpha, the null distribution's mean and 95 % quantile, and the counts of rejected
and site-less samples.  The p-value is (1 + #{permutations with MMD2 >= the observed}) / (permutations + 1), so 1 / (R + 1) is
the smallest it can be.

Exit status: 0 no drift at --alpha; 1 DRIFT (p-value <= alpha) -- a finding, not an error, so that a script can gate a scan on
it; 2 the index holds embeddings of another size than the model's (checked before any data is read).  Other weights than the
index's fingerprint are a warning.  The models are `similar`'s, with its refusals (no ensemble, no GREAT var-misuse model).

--max-reference N takes a seeded subset of a larger index.  Two paths: the default keeps the embeddings on the device -- one
bandwidth launch, one subsets launch, the fused permutation sums (csrc/bl_drift.hip: the N x N kernel matrix is never formed)
and one copy back; `--host` runs the NumPy twin (buglab/models/_drift.py, fp64) on the same embeddings.
"""
from __future__ import annotations

import argparse
import logging
import math
import sys
from pathlib import Path
from typing import Any, Iterable, Optional

if __package__ in (None, ""):
    sys.path.insert(0, str(Path(__file__).resolve().parents[2]))

import numpy as np

from buglab.models import _drift as Dr
from buglab.models import _similar as S
from buglab.models._cli import embedding_dim as _embedding_dim, open_model as _open_model, read_data as _read_data
from buglab.models._cli import require_gpu, write_records, write_report_json
from buglab.models._drift import DriftReport
from buglab.models._similar import SiteIndex

LOGGER = logging.getLogger(__name__)
EXIT_NO_DRIFT, EXIT_DRIFT, EXIT_DIMENSION_MISMATCH = 0, 1, 2


def kernel_shift(bandwidth_scale: float) -> float:
    """The constant the device subtracts from K while it sums: the kernel value at the mean squared distance."""
    return math.exp(-1.0 / float(bandwidth_scale))


def drift_between(x_ref, x_new, device=None, num_permutations: int = 1000, seed: int = 0, *, alpha: float = 0.05,
                  bandwidth_scale: float = 1.0, top_k: int = 20, host: bool = False, col_tiles: Optional[int] = None) -> DriftReport:
    """The test on embeddings that already exist: x_ref [n, D] and x_new [m, D], fp32, centred alike, arrays or tensors (tensors
    on the device stay there).  `host`: the NumPy twin.  ValueError for fewer than 2 rows on a side or sizes the kernels do not
    take.  One copy back (and one synchronisation) at the end."""
    Dr.check_samples(tuple(x_ref.shape), tuple(x_new.shape), num_permutations)
    if host:
        as_array = lambda x: x if isinstance(x, np.ndarray) else x.detach().cpu().numpy()
        return Dr.drift_host(as_array(x_ref), as_array(x_new), num_permutations, seed, alpha, bandwidth_scale, top_k)
    import torch

    from buglab.models import hip_ops

    to_device = lambda x: (torch.from_numpy(np.ascontiguousarray(x, np.float32)) if isinstance(x, np.ndarray) else x.detach().float()).to(device)
    if device is None:
        device = x_ref.device if not isinstance(x_ref, np.ndarray) else "cuda"
    n, m, D, R = int(x_ref.shape[0]), int(x_new.shape[0]), int(x_ref.shape[1]), int(num_permutations)
    z = torch.cat([to_device(x_ref), to_device(x_new)])
    bandwidth, rownorm = hip_ops.drift_bandwidth(z, bandwidth_scale)
    mask = hip_ops.drift_subsets(n + m, n, R, seed, z.device)
    sums, u0, rho = hip_ops.drift_permutation_sums(z, rownorm, mask, n, bandwidth, kernel_shift(bandwidth_scale), col_tiles=col_tiles)
    blob = torch.cat([bandwidth, sums, u0, rho]).cpu().numpy()  # the one copy back
    s, sums, u0, rho = float(blob[0]), blob[1:2 * R + 4], blob[2 * R + 4:2 * R + 4 + n + m], blob[2 * R + 4 + n + m:]
    return Dr.make_report(n, m, D, s, sums[:R + 1], sums[R + 1:2 * R + 2], sums[2 * R + 2], u0, rho, alpha, seed, top_k)


def reference_rows(index: SiteIndex, max_reference: Optional[int], seed: int) -> np.ndarray:
    """The index rows the test takes: all, or a seeded `max_reference`-subset in index order."""
    if max_reference is None or int(max_reference) >= index.size:
        return np.arange(index.size)
    if int(max_reference) < 2:
        raise ValueError(f"drift: --max-reference must be at least 2 (got {max_reference})")
    return np.sort(np.random.default_rng(int(seed)).choice(index.size, int(max_reference), replace=False))


def detect_drift(model, nn, index: SiteIndex, data: Iterable[Any], device, num_permutations: int = 1000, seed: int = 0, *,
                 alpha: float = 0.05, bandwidth_scale: float = 1.0, top_k: int = 20, site: str = "predicted", assume_buggy: bool = False,
                 max_reference: Optional[int] = None, host: bool = False, parallelize: bool = True) -> DriftReport:
    """Whether the sites of `data` look like the index's: the report of the permutation test (module docstring).  The embeddings
    are `similar.embed_sites`' and stay on the device; `host` runs the twin on the same embeddings.  TypeError for an ensemble or
    the GREAT var-misuse model, `_similar.DimensionMismatch` when the index holds embeddings of another size; other weights than
    the index's are logged as a warning.  ValueError when either side has fewer than 2 sites."""
    from buglab.controllers import _batching as Bt
    from buglab.models import similar

    Bt.require_single_model(model, "drift")
    warning = index.check_model(type(model).__name__, similar.embedding_dim(nn), S.model_fingerprint(nn))  # DimensionMismatch first
    if warning:
        LOGGER.warning("%s", warning)
    ref = np.ascontiguousarray(index.embeddings[reference_rows(index, max_reference, seed)])
    found = similar._collect_sites(model, nn, data, device, site, assume_buggy, host, parallelize)
    if found.rows is None:
        raise ValueError("drift: no sample of the data was accepted")
    if host:
        place = np.asarray(found.place)
        x_new = S.centre(found.rows[place >= 0], index.mean)
    else:
        import torch

        mean = torch.from_numpy(np.ascontiguousarray(index.mean)).to(found.rows.device)
        place = found.place.cpu().numpy()  # which samples have a site: the embeddings themselves stay on the device
        keep = torch.from_numpy(np.flatnonzero(place >= 0)).to(found.rows.device)
        x_new = (found.rows.index_select(0, keep).double() - mean.double()[None, :]).float()  # `_similar.centre`, on the device
    with_site = np.flatnonzero(place >= 0)
    report = drift_between(ref, x_new, None if host else found.rows.device, num_permutations, seed, alpha=alpha,
                           bandwidth_scale=bandwidth_scale, top_k=top_k, host=host)
    listed = []
    for o in report.outliers:
        b = int(with_site[o["position"]])
        point = found.points[b]
        node, label, path, package = S.site_metadata(point, place[b])
        listed.append({"position": int(found.positions[b]), "witness": o["witness"], "node": node, "label": label, "filename": path,
                       "package": package, "scout": S.true_scout(point)})
    return report._replace(outliers=listed, num_samples=found.num_samples, num_rejected=found.num_rejected,
                           num_without_site=len(found.positions) - with_site.shape[0])


# ---- command line ------------------------------------------------------------------------------------------------------------
def parse_args(argv=None) -> argparse.Namespace:
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("MODEL", help="The checkpoint the index was built with (`*.pkl.gz`).")
    p.add_argument("INDEX", help="The reference: an index written by `python -m buglab.models.similar index`.")
    p.add_argument("DATA", help="`*.msgpack.l.gz` data about to be scanned: a file or a folder.")
    p.add_argument("OUT", help="JSON lines, one per listed outlier (gzip when the name ends in .gz).")
    p.add_argument("--num-permutations", type=int, default=1000, help="Permutations R; the smallest p-value is 1 / (R + 1).")
    p.add_argument("--seed", type=int, default=0, help="Seed of the permutations (and of --max-reference).")
    p.add_argument("--alpha", type=float, default=0.05, help="Level of the test: drift when the p-value is at most this.")
    p.add_argument("--bandwidth-scale", type=float, default=1.0, help="The RBF bandwidth as a multiple of the mean squared distance.")
    p.add_argument("--top-k", type=int, default=20, help="Scanned samples listed, the least like the reference first.")
    p.add_argument("--site", choices=S.SITE_MODES, default="predicted", help="Which location of a sample is compared.")
    p.add_argument("--assume-buggy", action="store_true", help="Leave NO_BUG out when the site is predicted.")
    p.add_argument("--max-reference", type=int, default=None, help="Take a seeded subset of this many index entries.")
    p.add_argument("--limit-num-elements", type=int, default=None, help="Read at most this many samples.")
    p.add_argument("--sequential", action="store_true", help="Do not parallelize data loading.")
    p.add_argument("--host", action="store_true", help="Run the test in the NumPy twin instead of the device kernels.")
    p.add_argument("--report-json", default=None, help="Also write the run's numbers as data.")
    args = p.parse_args(argv)
    if args.num_permutations < 1 or not 0.0 < args.alpha < 1.0 or not args.bandwidth_scale > 0.0 or args.top_k < 0:
        p.error("need --num-permutations >= 1, 0 < --alpha < 1, --bandwidth-scale > 0 and --top-k >= 0")
    return args


def run(args: argparse.Namespace) -> int:
    model, nn, device, have_gpu = _open_model(args.MODEL)
    index = SiteIndex.load(args.INDEX)
    try:  # before anything is read or run: an index of another model's embeddings is the caller's mistake
        index.check_model(type(model).__name__, _embedding_dim(nn), index.fingerprint)
    except S.DimensionMismatch as e:
        print(str(e), file=sys.stderr)
        return EXIT_DIMENSION_MISMATCH
    require_gpu(have_gpu, "drift")
    data = _read_data(args.DATA, args.limit_num_elements)
    report = detect_drift(model, nn, index, data, device, args.num_permutations, args.seed, alpha=args.alpha,
                          bandwidth_scale=args.bandwidth_scale, top_k=args.top_k, site=args.site, assume_buggy=args.assume_buggy,
                          max_reference=args.max_reference, host=args.host, parallelize=not args.sequential)
    write_records(report.outliers, args.OUT)
    spread = "" if report.bandwidth > 0.0 else " (no spread: every embedding is the same point)"
    print(f"drift: {'DRIFT' if report.drift else 'no drift'} at alpha {report.alpha:g}: p-value {report.p_value:.4g}, MMD2 "
          f"{report.statistic:.6g} (null mean {report.null_mean:.6g}, 95 % {report.null_q95:.6g}){spread}; {report.n} reference and "
          f"{report.m} scanned sites of size {report.dim}, {report.num_rejected} samples rejected, {report.num_without_site} without a site.")
    write_report_json(args.report_json, report.record())
    return EXIT_DRIFT if report.drift else EXIT_NO_DRIFT


if __name__ == "__main__":
    sys.exit(run(parse_args()))
