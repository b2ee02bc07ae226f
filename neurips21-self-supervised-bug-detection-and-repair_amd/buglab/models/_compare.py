"""The packed outcome words, the NumPy twin of the bootstrap kernel (csrc/bl_bootstrap.hip) and the statistics behind
buglab/models/compare.py.  NumPy only: nothing here needs a GPU or the HIP library.

A paired bootstrap asks whether model b is better than model 0 on the SAME samples: replicate r draws n sample positions with
replacement, every model's counts are taken over those draws, every metric is a ratio of the counts, and the spread of
metric_b - metric_0 over the replicates is the answer.  What a sample contributes is one uint32 (`pack_outcomes`), so a
replicate is n random gathers and a handful of integer adds: `hip_ops.bootstrap_counts` on the device,
`bootstrap_counts_host` here.  Both produce the same [R, C] integer array, bit for bit; `metrics_from_counts` and everything
after it is shared.

The draw contract (include/buglab_hip.h has the same text).  Replicate r >= 0, draw j in [0, n), all arithmetic uint64, wrapping:
    mix(z):  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  return z ^ (z >> 31)
    base   = mix(seed * 0x9E3779B97F4A7C15 + 0x9E3779B97F4A7C15)
    h      = mix(r * n + j + base) >> 32
    index  = (h * n) >> 32
splitmix64 as a counter generator: a draw depends on (seed, r, j, n) alone.  The multiply-shift's relative bias is below n / 2^32.

The columns of a counts row, C = K + M (4 + 2K):  scout_total[K] | per model m: repaired, repaired_and_buggy, warned_and_buggy,
silent_and_not_buggy, loc_ok[K], rep_ok[K]."""
from __future__ import annotations

import math
from typing import Any, Dict, List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np

MAX_MODELS = 6   # BL_BOOTSTRAP_MAX_MODELS
MAX_SCOUTS = 64  # BL_BOOTSTRAP_MAX_SCOUTS
RATIO_METRICS = ("accuracy", "bug_detection_accuracy", "bug_detection_false_negatives", "bug_detection_false_positives",
                 "localization_accuracy", "repair_accuracy_given_location", "repair_accuracy", "bug_detection_recall",
                 "no_bug_precision")
_HOST_CHUNK_DRAWS = 1 << 21  # draws held at once by the twin: 16 MB of indices, a few tens of MB with the temporaries

_U = np.uint64
_GOLDEN = _U(0x9E3779B97F4A7C15)


def _mix(z: np.ndarray) -> np.ndarray:
    z = (z ^ (z >> _U(30))) * _U(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> _U(27))) * _U(0x94D049BB133111EB)
    return z ^ (z >> _U(31))


def num_columns(M: int, K: int) -> int:
    return K + M * (4 + 2 * K)


def draw_indices(seed: int, replicates: Union[int, Sequence[int], np.ndarray], n: int) -> np.ndarray:
    """The sample positions of the given replicates, int64 [R, n].  `replicates`: a count R (replicates 0 .. R - 1) or the
    replicate numbers themselves."""
    n = int(n)
    if not 1 <= n < 2 ** 31:
        raise ValueError(f"draw_indices: n must be in [1, 2^31) (got {n})")
    reps = np.arange(int(replicates), dtype=np.uint64) if np.ndim(replicates) == 0 else np.asarray(replicates).astype(np.uint64)
    with np.errstate(over="ignore"):
        base = _mix(np.asarray(_U(int(seed) & 0xFFFFFFFFFFFFFFFF) * _GOLDEN + _GOLDEN))
        counter = reps[:, None] * _U(n) + np.arange(n, dtype=np.uint64)[None, :] + base
        h = _mix(counter) >> _U(32)
        return ((h * _U(n)) >> _U(32)).astype(np.int64)


def pack_outcomes(reports: Sequence[Any]) -> Tuple[np.ndarray, int, List[str]]:
    """M `ColumnarEvaluationReport`s over the same samples, in the same order -> (packed uint32 [n], K, scout_names).  Bits
    0-7: the sample's scout id in the merged numbering (the first report's names in its order, "NoBug" = 0, then names only
    later reports know); model m's bits 8 + 4m .. 11 + 4m: warned | location_correct << 1 | (repair_given_location == 1) << 2 |
    repaired << 3."""
    M = len(reports)
    if not 1 <= M <= MAX_MODELS:
        raise ValueError(f"pack_outcomes: {M} models; a comparison takes 1 to {MAX_MODELS} (BL_BOOTSTRAP_MAX_MODELS)")
    names: List[str] = []
    for r in reports:
        if not r.scout_names or r.scout_names[0] != "NoBug":
            raise ValueError("pack_outcomes: a report's scout_names must start with 'NoBug'")
        names.extend(s for s in r.scout_names if s not in names)
    K = len(names)
    if K > MAX_SCOUTS:
        raise ValueError(f"pack_outcomes: {K} scouts; a comparison takes at most {MAX_SCOUTS} (BL_BOOTSTRAP_MAX_SCOUTS)")
    ids = {s: i for i, s in enumerate(names)}
    n = int(np.asarray(reports[0].has_bug).shape[0])
    has_bug = np.asarray(reports[0].has_bug, dtype=bool)
    scout = None
    packed = np.zeros(n, np.uint32)
    for m, r in enumerate(reports):
        if np.asarray(r.has_bug).shape[0] != n:
            raise ValueError(f"pack_outcomes: model {m} has {np.asarray(r.has_bug).shape[0]} samples, model 0 has {n}: the reports "
                             "are not over the same samples")
        mine = np.array([ids[s] for s in r.scout_names], dtype=np.int64)[np.asarray(r.scout, dtype=np.int64)]
        if scout is None:
            scout = mine
        if not np.array_equal(np.asarray(r.has_bug, dtype=bool), has_bug) or not np.array_equal(mine, scout):
            raise ValueError(f"pack_outcomes: has_bug / scout of model {m} differ from model 0's: the reports are not over the same "
                             "samples in the same order")
        flags = (np.asarray(r.warned, dtype=bool).astype(np.uint32)
                 | np.asarray(r.location_correct, dtype=bool).astype(np.uint32) << np.uint32(1)
                 | (np.asarray(r.repair_given_location) == 1).astype(np.uint32) << np.uint32(2)
                 | np.asarray(r.repaired, dtype=bool).astype(np.uint32) << np.uint32(3))
        packed |= flags << np.uint32(8 + 4 * m)
    if not np.array_equal(has_bug, scout != 0):
        raise ValueError("pack_outcomes: has_bug must be (scout != 'NoBug') for every sample")
    packed |= scout.astype(np.uint32)
    return packed, K, names


def _check_shape(M: int, K: int) -> None:
    if not 1 <= M <= MAX_MODELS:
        raise ValueError(f"M must be in [1, {MAX_MODELS}] (BL_BOOTSTRAP_MAX_MODELS), got {M}")
    if not 1 <= K <= MAX_SCOUTS:
        raise ValueError(f"K must be in [1, {MAX_SCOUTS}] (BL_BOOTSTRAP_MAX_SCOUTS), got {K}")


def count_words(words: np.ndarray, M: int, K: int) -> np.ndarray:
    """The counts of rows of packed words, int32 [rows, C]: row i counts words[i, :].  The columns of bl_bootstrap_counts."""
    _check_shape(M, K)
    words = np.asarray(words, dtype=np.uint32)
    rows = words.shape[0]
    out = np.zeros((rows, num_columns(M, K)), np.int32)
    scout = (words & np.uint32(0xFF)).astype(np.int64)
    buggy = scout != 0
    tabled = scout < K  # a scout id >= K counts as buggy and enters no [k] column
    slot = scout + np.arange(rows, dtype=np.int64)[:, None] * K

    def table(mask):
        return np.bincount(slot[mask], minlength=rows * K).reshape(rows, K)

    out[:, :K] = table(tabled)
    for m in range(M):
        f = words >> np.uint32(8 + 4 * m)
        warned, loc, rep_ok, repaired = ((f >> np.uint32(b)) & np.uint32(1) != 0 for b in range(4))
        at = K + m * (4 + 2 * K)
        out[:, at] = repaired.sum(axis=1)
        out[:, at + 1] = (repaired & buggy).sum(axis=1)
        out[:, at + 2] = (warned & buggy).sum(axis=1)
        out[:, at + 3] = (~warned & ~buggy).sum(axis=1)
        out[:, at + 4:at + 4 + K] = table(tabled & loc)
        out[:, at + 4 + K:at + 4 + 2 * K] = table(tabled & rep_ok & buggy)
    return out


def bootstrap_counts_host(packed: np.ndarray, M: int, K: int, seed: int, r0: int, R: int) -> np.ndarray:
    """bl_bootstrap_counts in NumPy: the counts of replicates r0 .. r0 + R - 1, int32 [R, C].  Chunked over replicates."""
    packed = np.ascontiguousarray(packed, dtype=np.uint32)
    n = packed.shape[0]
    _check_shape(M, K)
    if packed.ndim != 1 or n < 1 or R < 0 or r0 < 0:
        raise ValueError(f"bootstrap_counts_host: need packed [n >= 1], R >= 0, r0 >= 0 (got {packed.shape}, R {R}, r0 {r0})")
    out = np.empty((R, num_columns(M, K)), np.int32)
    step = max(1, _HOST_CHUNK_DRAWS // n)
    for lo in range(0, R, step):
        hi = min(R, lo + step)
        out[lo:hi] = count_words(packed[draw_indices(seed, np.arange(r0 + lo, r0 + hi, dtype=np.uint64), n)], M, K)
    return out


def metric_names(K: int) -> List[str]:
    """The keys of `metrics_from_counts`: the nine ratios of `summary()`, then per scout k the localization accuracy and (k >= 1:
    `per_scout()` counts buggy samples only) the repair accuracy given the location."""
    return (list(RATIO_METRICS) + [f"localization_accuracy[{k}]" for k in range(K)]
            + [f"repair_accuracy_given_location[{k}]" for k in range(1, K)])


def metrics_from_counts(counts: np.ndarray, n: int, M: int, K: int) -> Dict[str, np.ndarray]:
    """counts [R, C] (the device's or the twin's) -> {metric: float64 [R, M]}, by the formulas of
    `ColumnarEvaluationReport.summary()` / `per_scout()`; NaN where the denominator is 0."""
    counts = np.asarray(counts)
    if counts.ndim != 2 or counts.shape[1] != num_columns(M, K):
        raise ValueError(f"metrics_from_counts: counts {counts.shape} must be [R, {num_columns(M, K)}]")
    counts = counts.astype(np.int64)
    R = counts.shape[0]
    scout_total = counts[:, :K]                       # [R, K]
    per = counts[:, K:].reshape(R, M, 4 + 2 * K)      # [R, M, 4 + 2K]
    repaired, repaired_buggy, warned_buggy, silent_correct = (per[:, :, i] for i in range(4))
    loc_ok, rep_ok = per[:, :, 4:4 + K], per[:, :, 4 + K:]
    total = np.full((R, 1), int(n), np.int64)
    correct_code = scout_total[:, :1]
    buggy = total - correct_code

    def div(a, b):
        a, b = np.broadcast_arrays(a, b)
        out = np.full(a.shape, np.nan)
        np.divide(a, b, out=out, where=b != 0)
        return out

    m = {
        "accuracy": div(repaired, total),
        "bug_detection_accuracy": div(warned_buggy + silent_correct, total),
        "bug_detection_false_negatives": 1 - div(warned_buggy, buggy),
        "bug_detection_false_positives": 1 - div(silent_correct, correct_code),
        "localization_accuracy": div(loc_ok.sum(axis=2), total),
        "repair_accuracy_given_location": div(rep_ok.sum(axis=2), buggy),
        "repair_accuracy": div(repaired_buggy, buggy),
        "bug_detection_recall": div(warned_buggy, buggy),
        "no_bug_precision": div(silent_correct, correct_code),
    }
    for k in range(K):
        m[f"localization_accuracy[{k}]"] = div(loc_ok[:, :, k], scout_total[:, k:k + 1])
    for k in range(1, K):
        m[f"repair_accuracy_given_location[{k}]"] = div(rep_ok[:, :, k], scout_total[:, k:k + 1])
    return m


def mcnemar_exact(b: int, c: int) -> float:
    """The exact two-sided McNemar (binomial) test on b and c discordant samples: min(1, 2 sum_{i <= min(b, c)} C(b + c, i) /
    2^(b + c)), in integers; 1.0 without a discordant sample."""
    b, c = int(b), int(c)
    if b < 0 or c < 0:
        raise ValueError("mcnemar_exact: counts must not be negative")
    t = b + c
    if t == 0:
        return 1.0
    tail = sum(math.comb(t, i) for i in range(min(b, c) + 1))
    return min(1.0, (2 * tail) / (1 << t))  # int / int: correctly rounded, whatever the size


class Interval(NamedTuple):
    point: float
    se: float
    low: float
    high: float
    num_undefined: int


def _interval(point: float, values: np.ndarray, confidence: float) -> Interval:
    """se and the percentile interval over the defined replicates: the NaN ones are dropped first, so `np.std(ddof=1)` and
    `np.quantile` give what `np.nanstd(ddof=1)` and `np.nanquantile` give on all of them (without their all-NaN warnings)."""
    defined = values[~np.isnan(values)]
    undefined = int(values.shape[0] - defined.shape[0])
    if defined.shape[0] == 0:
        return Interval(float(point), float("nan"), float("nan"), float("nan"), undefined)
    se = float(np.std(defined, ddof=1)) if defined.shape[0] > 1 else float("nan")
    low, high = np.quantile(defined, [(1 - confidence) / 2, (1 + confidence) / 2])
    return Interval(float(point), se, float(low), float(high), undefined)


def _paired_p(delta: np.ndarray) -> float:
    """Two-sided: min(1, 2 min((1 + #{d <= 0}) / (R' + 1), (1 + #{d >= 0}) / (R' + 1))) over the R' defined replicates."""
    defined = delta[~np.isnan(delta)]
    r = defined.shape[0]
    if r == 0:
        return float("nan")
    return min(1.0, 2 * min((1 + int((defined <= 0).sum())) / (r + 1), (1 + int((defined >= 0).sum())) / (r + 1)))


class ComparisonReport:
    """What a comparison found.  `metrics[name][m]`: the `Interval` of model m; `deltas[name][b]` (b >= 1): the `Interval` of
    metric_b - metric_0 over the same draws and `p_values[name][b]`; `mcnemar[b]`: {"baseline_only", "model_only", "p"} on
    `repaired`.  `models`: per model its name, the samples it was given, dropped and kept."""

    def __init__(self, names, scout_names, num_paired, num_replicates, seed, confidence, metrics, deltas, p_values, mcnemar,
                 models=None):
        self.names, self.scout_names = list(names), list(scout_names)
        self.num_paired, self.num_replicates, self.seed, self.confidence = int(num_paired), int(num_replicates), int(seed), float(confidence)
        self.metrics, self.deltas, self.p_values, self.mcnemar = metrics, deltas, p_values, mcnemar
        self.models = models if models is not None else [{"name": n, "num_samples": self.num_paired, "num_dropped": 0} for n in self.names]
        self.curve_bands: Optional[List[Dict[str, Any]]] = None  # compare.py --curves: per model, the bands of its threshold curves

    def to_dict(self) -> Dict[str, Any]:
        bands = {} if self.curve_bands is None else {"curve_bands": self.curve_bands}
        return {
            **bands,
            "models": self.models, "scout_names": self.scout_names, "num_paired": self.num_paired,
            "num_replicates": self.num_replicates, "seed": self.seed, "confidence": self.confidence,
            "metrics": {k: [iv._asdict() for iv in v] for k, v in self.metrics.items()},
            "deltas": {k: {str(b): iv._asdict() for b, iv in v.items()} for k, v in self.deltas.items()},
            "p_values": {k: {str(b): p for b, p in v.items()} for k, v in self.p_values.items()},
            "mcnemar": {str(b): v for b, v in self.mcnemar.items()},
        }

    def to_json(self) -> str:
        import json

        return json.dumps(self.to_dict(), indent=1, sort_keys=True) + "\n"  # NaN where a value is undefined

    def format(self) -> str:
        pct = lambda x: "NaN" if x != x else f"{100 * x:.2f}%"
        span = lambda iv: f"{pct(iv.point)} [{pct(iv.low)}, {pct(iv.high)}]"
        lines = [f"Paired bootstrap over {self.num_paired} samples, {self.num_replicates} replicates, seed {self.seed}, "
                 f"{100 * self.confidence:g}% percentile intervals."]
        for i, m in enumerate(self.models):
            lines.append(f"  model {i}{' (baseline)' if i == 0 else ''}: {m['name']}: {m['num_samples']} samples given, "
                         f"{m['num_dropped']} dropped, {self.num_paired} paired")
        for name, ivs in self.metrics.items():
            lines.append(name)
            for i, iv in enumerate(ivs):
                text = f"  model {i}: {span(iv)} se {pct(iv.se)}"
                if iv.num_undefined:
                    text += f" ({iv.num_undefined} replicates undefined)"
                if i:
                    d, p = self.deltas[name][i], self.p_values[name][i]
                    text += f"   vs model 0: {'NaN' if d.point != d.point else f'{100 * d.point:+.2f}'} [{pct(d.low)}, {pct(d.high)}] p {p:.4g}"
                lines.append(text)
        for b, v in self.mcnemar.items():
            lines.append(f"McNemar (exact) on repaired, model {b} vs model 0: {v['baseline_only']} samples only the baseline repairs, "
                         f"{v['model_only']} only model {b}: p {v['p']:.4g}")
        return "\n".join(lines) + "\n"


def named_metrics(K: int, scout_names: Sequence[str]) -> Dict[str, str]:
    """metrics_from_counts key -> the key a report shows (scout ids replaced by names)."""
    out = {name: name for name in RATIO_METRICS}
    for k in range(K):
        out[f"localization_accuracy[{k}]"] = f"localization_accuracy[{scout_names[k]}]"
    for k in range(1, K):
        out[f"repair_accuracy_given_location[{k}]"] = f"repair_accuracy_given_location[{scout_names[k]}]"
    return out


def summarize(packed: np.ndarray, M: int, K: int, counts: np.ndarray, *, names: Sequence[str], scout_names: Sequence[str],
              seed: int, confidence: float, models: Optional[List[Dict[str, Any]]] = None) -> ComparisonReport:
    """Everything after the counts: the point estimates from the unresampled words, the intervals, the paired differences
    against model 0 and McNemar's test.  `counts` [R, C]: the device's or the twin's."""
    if not 0 < confidence < 1:
        raise ValueError(f"confidence must be in (0, 1) (got {confidence})")
    packed = np.asarray(packed, dtype=np.uint32)
    n = packed.shape[0]
    point = metrics_from_counts(count_words(packed[None, :], M, K), n, M, K)
    values = metrics_from_counts(counts, n, M, K)
    shown = named_metrics(K, scout_names)
    metrics, deltas, p_values = {}, {}, {}
    for key, name in shown.items():
        metrics[name] = [_interval(point[key][0, m], values[key][:, m], confidence) for m in range(M)]
        deltas[name], p_values[name] = {}, {}
        for b in range(1, M):
            d = values[key][:, b] - values[key][:, 0]
            deltas[name][b] = _interval(point[key][0, b] - point[key][0, 0], d, confidence)
            p_values[name][b] = _paired_p(d)
    repaired = lambda m: (packed >> np.uint32(11 + 4 * m)) & np.uint32(1) != 0
    mcnemar = {}
    for b in range(1, M):
        base_only, model_only = int((repaired(0) & ~repaired(b)).sum()), int((~repaired(0) & repaired(b)).sum())
        mcnemar[b] = {"baseline_only": base_only, "model_only": model_only, "p": mcnemar_exact(base_only, model_only)}
    return ComparisonReport(names, scout_names, n, counts.shape[0], seed, confidence, metrics, deltas, p_values, mcnemar, models)
