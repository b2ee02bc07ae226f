"""False-discovery-controlled warnings: the NumPy twin of csrc/bl_fdr.hip, the reference a checkpoint carries, and the records.

BEYOND THE REFERENCE.  The definitions (include/buglab_hip.h has them in full):
  score    s = src[nobug_idx[b]], the fp32 NO_BUG location log-probability; an index outside src reads as NaN
  count    c = #{ j : ref[j] <= s } over the sorted reference ref[0 .. n); n for a NaN s
  p-value  p = (c + 1) / (n + 1)
  BH       R[c] = #{samples with count <= c};  c* = max{ c : R[c] > 0 and (double)((c + 1) N) <= q * (double)((n + 1) R[c]) }, -1
           if none; flagged iff c <= c*
  q-value  qv(c) = min over c' >= c with R[c'] > 0 of min(1, (double)((c' + 1) N) / (double)((n + 1) R[c']))
`counts_host` and `bh_host` equal the kernels bit for bit on every output: fp32 compares, integer counts, one fp64 product or
quotient per bin and fp64 minima."""
from __future__ import annotations

import math
from typing import Any, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

MAX_REFERENCE = 1 << 20  # BL_FDR_MAX_REFERENCE
DEPENDENCE = ("independent", "arbitrary")


# ---- the twin ----------------------------------------------------------------------------------------------------------------
def counts_host(src: np.ndarray, nobug_idx: np.ndarray, ref: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """bl_fdr_counts: (score float32 [B], count int32 [B]).  src float32 [n_src], nobug_idx int [B], ref float32 [n] ascending
    without NaN."""
    src, ref = np.ascontiguousarray(src, np.float32), np.ascontiguousarray(ref, np.float32)
    idx = np.asarray(nobug_idx, np.int64)
    n = int(ref.shape[0])
    if not 1 <= n <= MAX_REFERENCE:
        raise ValueError(f"counts_host: the reference must hold between 1 and {MAX_REFERENCE} scores (got {n})")
    inside = (idx >= 0) & (idx < src.shape[0])
    score = np.full(idx.shape[0], np.nan, np.float32)
    score[inside] = src[idx[inside]]  # a NaN of src keeps its bits
    count = np.searchsorted(ref, score, side="right").astype(np.int32)  # ties: every equal entry is counted
    count[score != score] = n
    return score, count


def bh_host(count: np.ndarray, n_ref: int, q: float) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """bl_fdr_bh: (cutoff int32 [2] = c* | R[c*] or 0, flag int32 [N], q_value float64 [N], R int32 [n_ref + 1])."""
    n_ref, q = int(n_ref), float(q)
    count = np.asarray(count, np.int32)
    N = int(count.shape[0])
    if N < 1 or not 1 <= n_ref <= MAX_REFERENCE:
        raise ValueError(f"bh_host: need N >= 1 and 1 <= n_ref <= {MAX_REFERENCE} (got N {N}, n_ref {n_ref})")
    if not 0.0 < q <= 1.0:
        raise ValueError(f"bh_host: the level q must be in (0, 1] (got {q})")
    c = np.clip(count, 0, n_ref).astype(np.int64)
    R = np.cumsum(np.bincount(c, minlength=n_ref + 1).astype(np.int64))
    lhs = ((np.arange(n_ref + 1, dtype=np.int64) + 1) * N).astype(np.float64)  # exact: below 2^53
    pool = ((n_ref + 1) * R).astype(np.float64)
    qualifies = np.flatnonzero((R > 0) & (lhs <= q * pool))
    cut = int(qualifies[-1]) if qualifies.shape[0] else -1
    with np.errstate(divide="ignore", invalid="ignore"):
        term = np.where(R > 0, np.minimum(1.0, lhs / pool), np.inf)
    qv = np.minimum.accumulate(term[::-1])[::-1]
    cutoff = np.array([cut, R[cut] if cut >= 0 else 0], np.int32)
    return cutoff, (c <= cut).astype(np.int32), np.ascontiguousarray(qv[c]), R.astype(np.int32)


def p_values(count: np.ndarray, n_ref: int) -> np.ndarray:
    return (np.clip(np.asarray(count, np.int64), 0, int(n_ref)) + 1) / float(int(n_ref) + 1)


def harmonic(N: int) -> float:
    """sum_{i = 1 .. N} 1 / i: the Benjamini-Yekutieli divisor."""
    return math.fsum(1.0 / i for i in range(1, int(N) + 1))


def effective_level(q: float, N: int, dependence: str = "independent") -> float:
    """The level the step-up runs at: q, or q / harmonic(N) under arbitrary dependence (Benjamini-Yekutieli)."""
    if dependence not in DEPENDENCE:
        raise ValueError(f"dependence must be one of {DEPENDENCE} (got {dependence!r})")
    if not 0.0 < float(q) <= 1.0:
        raise ValueError(f"the false discovery rate must be in (0, 1] (got {q})")
    return float(q) if dependence == "independent" else float(q) / harmonic(N)


# ---- the reference -----------------------------------------------------------------------------------------------------------
def calibration_fingerprint(calibration) -> Optional[Tuple[float, float, float]]:
    """What identifies the calibration a score was formed under: its three parameters, or None without one."""
    if calibration is None:
        return None
    return float(calibration.beta), float(calibration.no_bug_bias), float(calibration.repair_beta)


class NullReference(NamedTuple):
    """What `fit_null_reference` keeps and a model object carries (`model.null_reference`); pickled with the checkpoint."""

    scores: np.ndarray                 # float32 [num_kept], ascending, no NaN
    num_kept: int
    num_dropped_nan: int               # accepted clean samples whose score was NaN
    num_skipped_buggy: int             # samples of CLEAN_DATA that carry a bug
    calibration: Optional[Tuple[float, float, float]]  # `calibration_fingerprint` of the model at fit time

    def to_dict(self) -> Dict[str, Any]:
        return {"num_kept": self.num_kept, "num_dropped_nan": self.num_dropped_nan, "num_skipped_buggy": self.num_skipped_buggy,
                "calibration": None if self.calibration is None else list(self.calibration),
                "smallest_p_value": 1.0 / (self.num_kept + 1),
                "score_min": float(self.scores[0]), "score_max": float(self.scores[-1])}


def make_null_reference(scores: np.ndarray, max_reference: int, num_skipped_buggy: int, calibration) -> NullReference:
    """From the clean samples' scores in input order: the first `max_reference` of them, NaNs dropped and counted, sorted."""
    max_reference = int(max_reference)
    if not 1 <= max_reference <= MAX_REFERENCE:
        raise ValueError(f"max_reference must be in [1, {MAX_REFERENCE}] (got {max_reference})")
    taken = np.asarray(scores, np.float32)[:max_reference]
    kept = np.sort(taken[taken == taken])
    if kept.shape[0] < 1:
        raise ValueError("the clean data yields no score: a reference needs at least one sample without a bug")
    return NullReference(np.ascontiguousarray(kept), int(kept.shape[0]), int(taken.shape[0] - kept.shape[0]), int(num_skipped_buggy),
                         calibration_fingerprint(calibration))


def check_reference(reference: Optional[NullReference], calibration, what: str) -> NullReference:
    if reference is None:
        raise LookupError(f"{what}: the checkpoint carries no null reference; run `python -m buglab.models.fdr fit` first")
    if reference.calibration != calibration_fingerprint(calibration):
        raise ValueError(f"{what}: the reference was fitted under calibration {reference.calibration} and the checkpoint now carries "
                         f"{calibration_fingerprint(calibration)}: the scores are not comparable; fit the reference again")
    return reference


# ---- records and report ------------------------------------------------------------------------------------------------------
def scan_record(position: int, score: float, count: int, n_ref: int, q_value: float, flagged: bool) -> Dict[str, Any]:
    score = float(score)
    return {"position": int(position), "score": None if score != score else score, "count": int(count),
            "p_value": (int(count) + 1) / float(int(n_ref) + 1), "q_value": float(q_value), "flagged": bool(flagged)}


def realised(flagged: np.ndarray, labels: Sequence[Optional[bool]]) -> Optional[Dict[str, Any]]:
    """The realised false discovery proportion and the share of buggy samples flagged, over the labelled samples; None when no
    sample carries a label."""
    known = np.array([l is not None for l in labels], bool)
    if not known.any():
        return None
    buggy = np.array([bool(l) for l in labels], bool)
    flagged = np.asarray(flagged, bool) & known
    num_flagged, false_alarms = int(flagged.sum()), int((flagged & ~buggy).sum())
    num_buggy, found = int((buggy & known).sum()), int((flagged & buggy).sum())
    return {"num_labelled": int(known.sum()), "num_buggy": num_buggy, "num_flagged": num_flagged, "false_alarms": false_alarms,
            "false_discovery_proportion": false_alarms / max(num_flagged, 1), "buggy_flagged": found,
            "power": found / num_buggy if num_buggy else None}


def summary(count: np.ndarray, flagged: np.ndarray, cutoff: np.ndarray, n_ref: int, q: float, q_effective: float, dependence: str,
            labels: Sequence[Optional[bool]], num_rejected: int = 0) -> Dict[str, Any]:
    N = int(np.asarray(count).shape[0])
    lowest = int(np.min(count)) if N else None
    return {"num_scanned": N, "num_rejected": int(num_rejected), "num_reference": int(n_ref), "fdr": float(q), "dependence": dependence,
            "q_effective": float(q_effective), "cutoff_count": int(cutoff[0]), "cutoff_rank": int(cutoff[1]),
            "cutoff_p_value": (int(cutoff[0]) + 1) / float(n_ref + 1) if cutoff[0] >= 0 else None,
            "num_flagged": int(np.asarray(flagged, bool).sum()), "smallest_attainable_p_value": 1.0 / (n_ref + 1),
            "p_value_needed_for_one_discovery": q_effective / N if N else None,
            "smallest_p_value_in_scan": None if lowest is None else (lowest + 1) / float(n_ref + 1),
            "labelled": realised(flagged, labels)}


def format_summary(s: Dict[str, Any]) -> str:
    lines = [f"Scanned {s['num_scanned']} samples ({s['num_rejected']} rejected by tensorize) against a reference of "
             f"{s['num_reference']} clean samples.",
             f"False discovery rate {s['fdr']:g} ({s['dependence']} dependence: the step-up runs at {s['q_effective']:.6g})."]
    if s["num_scanned"]:
        lines.append(f"Resolution: the smallest attainable p-value is {s['smallest_attainable_p_value']:.3g}; a lone discovery needs "
                     f"p <= {s['p_value_needed_for_one_discovery']:.3g}, R joint discoveries R times that; the smallest p-value of "
                     f"this scan is {s['smallest_p_value_in_scan']:.3g}.")
    if s["cutoff_count"] >= 0:
        lines.append(f"Flagged {s['num_flagged']} samples: p-value <= {s['cutoff_p_value']:.6g} (count <= {s['cutoff_count']}).")
    else:
        lines.append("Flagged 0 samples: no p-value passes the step-up.")
    lab = s["labelled"]
    if lab is not None:
        power = "n/a" if lab["power"] is None else f"{100 * lab['power']:.2f}% ({lab['buggy_flagged']}/{lab['num_buggy']})"
        lines.append(f"Labelled samples: realised false discovery proportion {100 * lab['false_discovery_proportion']:.2f}% "
                     f"({lab['false_alarms']}/{lab['num_flagged']}), buggy samples flagged {power}.")
    return "\n".join(lines) + "\n"
