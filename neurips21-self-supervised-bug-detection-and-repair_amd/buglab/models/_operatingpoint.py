"""Warning operating points: the candidate thresholds, the NumPy twin of bl_bootstrap_curve_counts (csrc/bl_bootstrap.hip) and
the statistics behind buglab/models/operatingpoint.py.  NumPy only: nothing here needs a GPU or the HIP library.

`evaluate.py` prints the six threshold curves (false-discovery rate, detection precision / recall, NO_BUG precision,
detect-and-repair precision / recall) as point estimates.  A deployment asks at which confidence a warning is shown and how
sure the precision there is; that needs the curves inside every bootstrap replicate.  They need no ranking per replicate: the
candidate thresholds are fixed once (`curve_grid`: confidences of warned samples, descending), every sample gets the index of
the first threshold it passes (`bin_of`), and a replicate is a histogram over those indices followed by a prefix sum.  The
draws are `_compare.draw_indices`, the words `_compare.pack_outcomes`: the curve replicates are the replicates `compare.py`
draws.

The columns of a counts row, C = 1 + M * 5 * G:  num_buggy | per model m, per counter c, per threshold g: the count over the
draws that pass threshold g (bin <= g) of, in the order of `_curves_of_ranked` in buglab/models/evaluate.py,
    det_true = has_bug & loc_ok | det_false = warned & ~loc_ok | full_true = has_bug & loc_ok & rep_ok |
    full_false = warned & (~loc_ok | ~rep_ok) | false_alarm = warned & ~has_bug
with has_bug = (word & 0xFF) != 0 and warned, loc_ok, rep_ok = bits 0, 1, 2 of model m's four bits at 8 + 4m.  A bin outside
[0, G) passes no threshold."""
from __future__ import annotations

from typing import Any, Dict, List, NamedTuple, Optional, Sequence

import numpy as np

from buglab.models._compare import _HOST_CHUNK_DRAWS, MAX_MODELS, Interval, _interval, draw_indices
from buglab.models._compare import pack_outcomes  # noqa: F401  the words this module counts; callers take it from here

MAX_BINS = 1024  # BL_CURVE_MAX_BINS
COUNTERS = ("det_true", "det_false", "full_true", "full_false", "false_alarm")
CURVES = ("fdr", "detection_precision", "detection_recall", "no_bug_precision", "precision", "recall")
RECALL_OF = {"precision": "recall", "detection_precision": "detection_recall"}  # the curves a point can be chosen on
_TRUE_FALSE_OF = {"precision": (2, 3), "detection_precision": (0, 1)}             # their true / false counters


def num_columns(M: int, G: int) -> int:
    return 1 + M * len(COUNTERS) * G


def curve_grid(confidence: np.ndarray, warned: np.ndarray, max_bins: int) -> np.ndarray:
    """The candidate thresholds, float64 [G], G <= max_bins, descending: the distinct confidences (log-probabilities) of the
    warned samples; when there are more than `max_bins`, that many of them evenly spaced by rank, the first and the last
    included (max_bins == 1: the last, which every warned sample passes).  Empty without a warned sample."""
    max_bins = int(max_bins)
    if not 1 <= max_bins <= MAX_BINS:
        raise ValueError(f"curve_grid: max_bins must be in [1, {MAX_BINS}] (BL_CURVE_MAX_BINS), got {max_bins}")
    confidence = np.asarray(confidence, dtype=np.float64)
    shown = confidence[np.asarray(warned, dtype=bool) & ~np.isnan(confidence)]
    distinct = np.unique(shown)[::-1]
    if distinct.shape[0] <= max_bins:
        return distinct.copy()
    if max_bins == 1:
        return distinct[-1:].copy()
    ranks = (np.arange(max_bins, dtype=np.int64) * (distinct.shape[0] - 1)) // (max_bins - 1)
    return distinct[ranks]


def bin_of(confidence: np.ndarray, thresholds: np.ndarray) -> np.ndarray:
    """int16 [n]: the number of thresholds strictly greater than the sample's confidence, so that bin <= g means
    confidence >= thresholds[g]; G for a sample below every threshold (and for a NaN confidence)."""
    thresholds = np.asarray(thresholds, dtype=np.float64)
    G = thresholds.shape[0]
    if thresholds.ndim != 1 or G > MAX_BINS or (G > 1 and not (np.diff(thresholds) < 0).all()):
        raise ValueError(f"bin_of: thresholds must be at most {MAX_BINS} strictly descending values")
    confidence = np.asarray(confidence, dtype=np.float64)
    bins = G - np.searchsorted(thresholds[::-1], confidence, side="right")
    return np.where(np.isnan(confidence), G, bins).astype(np.int16)


def _check(packed: np.ndarray, bins: np.ndarray, M: int, G: int, what: str) -> None:
    if not 1 <= M <= MAX_MODELS:
        raise ValueError(f"{what}: M must be in [1, {MAX_MODELS}] (BL_BOOTSTRAP_MAX_MODELS), got {M}")
    if not 1 <= G <= MAX_BINS:
        raise ValueError(f"{what}: G must be in [1, {MAX_BINS}] (BL_CURVE_MAX_BINS), got {G}")
    if packed.ndim != 1 or packed.shape[0] < 1 or bins.shape != (M, packed.shape[0]):
        raise ValueError(f"{what}: need packed [n >= 1] and bins [{M}, n] (got {packed.shape}, {bins.shape})")


def count_curve_words(words: np.ndarray, bins: np.ndarray, M: int, G: int) -> np.ndarray:
    """The counts of rows of packed words and their bins, int32 [rows, C]: row i counts words[i, :] with bins[:, i, :]
    (bins [M, rows, n]).  The columns of bl_bootstrap_curve_counts."""
    words = np.asarray(words, dtype=np.uint32)
    rows = words.shape[0]
    out = np.zeros((rows, num_columns(M, G)), np.int32)
    has_bug = (words & np.uint32(0xFF)) != 0
    out[:, 0] = has_bug.sum(axis=1)
    first = np.arange(rows, dtype=np.int64)[:, None] * G
    for m in range(M):
        f = words >> np.uint32(8 + 4 * m)
        warned, loc, rep = ((f >> np.uint32(b)) & np.uint32(1) != 0 for b in range(3))
        b = bins[m].astype(np.int64)
        passes = (b >= 0) & (b < G)
        slot = first + b
        masks = (has_bug & loc, warned & ~loc, has_bug & loc & rep, warned & (~loc | ~rep), warned & ~has_bug)
        for c, mask in enumerate(masks):
            per_bin = np.bincount(slot[mask & passes], minlength=rows * G).reshape(rows, G)
            at = 1 + (m * len(COUNTERS) + c) * G
            out[:, at:at + G] = np.cumsum(per_bin, axis=1)
    return out


def curve_counts_host(packed: np.ndarray, bins: np.ndarray, M: int, G: int, seed: int, r0: int, R: int) -> np.ndarray:
    """bl_bootstrap_curve_counts in NumPy: the counts of replicates r0 .. r0 + R - 1, int32 [R, C].  Chunked over replicates."""
    packed = np.ascontiguousarray(packed, dtype=np.uint32)
    bins = np.asarray(bins)
    M, G, R, r0 = int(M), int(G), int(R), int(r0)
    _check(packed, bins, M, G, "curve_counts_host")
    if R < 0 or r0 < 0:
        raise ValueError(f"curve_counts_host: need R >= 0 and r0 >= 0 (got R {R}, r0 {r0})")
    n = packed.shape[0]
    out = np.empty((R, num_columns(M, G)), np.int32)
    step = max(1, _HOST_CHUNK_DRAWS // n)
    for lo in range(0, R, step):
        hi = min(R, lo + step)
        at = draw_indices(seed, np.arange(r0 + lo, r0 + hi, dtype=np.uint64), n)
        out[lo:hi] = count_curve_words(packed[at], bins[:, at], M, G)
    return out


def curve_counts_point(packed: np.ndarray, bins: np.ndarray, M: int, G: int) -> np.ndarray:
    """The same counts for the data as they are, without draws: int32 [1, C]."""
    packed = np.ascontiguousarray(packed, dtype=np.uint32)
    bins = np.asarray(bins)
    _check(packed, bins, int(M), int(G), "curve_counts_point")
    return count_curve_words(packed[None, :], bins[:, None, :], int(M), int(G))


def split_counts(counts: np.ndarray, M: int, G: int):
    """counts [R, C] -> (num_buggy int64 [R], the counters int64 [R, M, 5, G])."""
    counts = np.asarray(counts)
    if counts.ndim != 2 or counts.shape[1] != num_columns(M, G):
        raise ValueError(f"counts {counts.shape} must be [R, {num_columns(M, G)}]")
    counts = counts.astype(np.int64)
    return counts[:, 0], counts[:, 1:].reshape(counts.shape[0], M, len(COUNTERS), G)


def curves_from_counts(counts: np.ndarray, M: int, G: int) -> Dict[str, np.ndarray]:
    """counts [R, C] (the device's or the twin's) -> {curve: float64 [R, M, G]} by the formulas of `_curves_of_ranked`, each
    replicate with its own num_buggy; NaN where a denominator is 0 (NO_BUG precision has the reference's + 1e-10 and is never
    undefined)."""
    num_buggy, t = split_counts(counts, M, G)
    det_true, det_false, full_true, full_false, false_alarm = (t[:, :, c, :] for c in range(len(COUNTERS)))
    buggy = np.broadcast_to(num_buggy[:, None, None], det_true.shape)

    def div(a, b):
        out = np.full(a.shape, np.nan)
        np.divide(a, b, out=out, where=b != 0)
        return out

    return {
        "fdr": div(det_false, det_true + det_false),
        "detection_precision": div(det_true, det_true + det_false),
        "detection_recall": div(det_true, buggy),
        "no_bug_precision": 1 - false_alarm / (buggy + 1e-10),
        "precision": div(full_true, full_true + full_false),
        "recall": div(full_true, buggy),
    }


def curve_bands(point_counts: np.ndarray, replicate_counts: np.ndarray, M: int, G: int, confidence: float = 0.95
                ) -> List[Dict[str, List[Interval]]]:
    """bands[m][curve][g]: the `Interval` of model m's curve at threshold g -- the point estimate from `point_counts` [1, C],
    se and the percentile interval over the defined replicates (`_compare._interval`) and the number of replicates in which
    the value was undefined."""
    if not 0 < confidence < 1:
        raise ValueError(f"confidence must be in (0, 1) (got {confidence})")
    point, values = curves_from_counts(point_counts, M, G), curves_from_counts(replicate_counts, M, G)
    return [{name: [_interval(point[name][0, m, g], values[name][:, m, g], confidence) for g in range(G)] for name in CURVES}
            for m in range(M)]


def bands_to_dict(bands: Dict[str, List[Interval]], thresholds: np.ndarray) -> Dict[str, Any]:
    """One model's bands as data: the thresholds (log-probabilities) and per curve the columns of its Intervals."""
    return {"thresholds_logprob": [float(t) for t in thresholds],
            "curves": {name: {field: [getattr(iv, field) for iv in ivs] for field in Interval._fields} for name, ivs in bands.items()}}


class OperatingPoint(NamedTuple):
    """The warning threshold `fit_operating_point` chose and a model object carries (`model.warning_operating_point`); pickled
    with the checkpoint.  Plain Python values only."""

    threshold_logprob: float  # warn when the prediction is a location and its log-probability is >= this
    curve: str                # "precision" (detect and repair) or "detection_precision"
    target: float
    confidence: float
    precision: Interval       # of `curve` at the threshold: point estimate and two-sided percentile interval
    recall: Interval          # of the matching recall curve
    num_warnings: int         # point-estimate warnings at the threshold (the curve's true + false counts)
    num_samples: int
    num_replicates: int
    seed: int
    grid_size: int
    calibrated: bool          # the model carried a `confidence_calibration` when the point was fitted

    def to_dict(self) -> Dict[str, Any]:
        return {**self._asdict(), "precision": self.precision._asdict(), "recall": self.recall._asdict()}


def _plain(iv: Interval) -> Interval:
    return Interval(float(iv.point), float(iv.se), float(iv.low), float(iv.high), int(iv.num_undefined))


def lower_bounds(replicate_counts: np.ndarray, G: int, curve: str, confidence: float) -> np.ndarray:
    """float64 [G]: the one-sided lower bound of `curve` at every threshold -- the (1 - confidence) quantile of the replicate
    values, an undefined replicate (no warning at that threshold) counted as 0."""
    values = np.nan_to_num(curves_from_counts(replicate_counts, 1, G)[curve][:, 0, :], nan=0.0)
    return np.quantile(values, 1 - confidence, axis=0)


def choose_operating_point(point_counts: np.ndarray, replicate_counts: np.ndarray, thresholds: Sequence[float], *,
                           curve: str = "precision", target: float, confidence: float = 0.95, min_warnings: int = 20,
                           num_samples: int = 0, seed: int = 0, calibrated: bool = False) -> Optional[OperatingPoint]:
    """The lowest threshold (the largest g, hence the highest recall) at which the one-sided lower bound of `curve` is at least
    `target` and the data as they are raise at least `min_warnings` warnings; None when no threshold qualifies.  Counts of ONE
    model: point_counts [1, 1 + 5G], replicate_counts [R, 1 + 5G], G = len(thresholds)."""
    if curve not in RECALL_OF:
        raise ValueError(f"curve must be one of {sorted(RECALL_OF)} (got {curve!r})")
    if not 0 < confidence < 1:
        raise ValueError(f"confidence must be in (0, 1) (got {confidence})")
    thresholds = np.asarray(thresholds, dtype=np.float64)
    G = int(thresholds.shape[0])
    replicate_counts = np.asarray(replicate_counts)
    if G == 0 or replicate_counts.shape[0] == 0:
        return None
    _, point_table = split_counts(point_counts, 1, G)
    true_c, false_c = _TRUE_FALSE_OF[curve]
    warnings = point_table[0, 0, true_c, :] + point_table[0, 0, false_c, :]
    bound = lower_bounds(replicate_counts, G, curve, confidence)
    qualifies = np.flatnonzero((bound >= target) & (warnings >= int(min_warnings)))
    if qualifies.size == 0:
        return None
    g = int(qualifies[-1])
    point, values = curves_from_counts(point_counts, 1, G), curves_from_counts(replicate_counts, 1, G)
    iv = lambda name: _plain(_interval(point[name][0, 0, g], values[name][:, 0, g], confidence))
    return OperatingPoint(float(thresholds[g]), curve, float(target), float(confidence), iv(curve), iv(RECALL_OF[curve]),
                          int(warnings[g]), int(num_samples), int(replicate_counts.shape[0]), int(seed), G, bool(calibrated))
