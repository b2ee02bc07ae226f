"""Confidence calibration: the value a model carries, the index arrays, and the NumPy fp64 twin of csrc/bl_confidence.hip.

Beyond the reference, which has no counterpart: post-hoc scaling on held-out data of the log-probabilities `predict` yields.
  localization  l' = log_softmax(beta * l + no_bug_bias * [entry is NO_BUG])   over a sample's flat location entries
  repair        r' = log_softmax(repair_beta * r)                              within each group the model normalises over
fitted by a damped Newton iteration on the convex losses  F(beta, b) = -sum_s l'_s[target]  and  F_r(beta_r) = -sum over the
buggy samples of the target rewrite's r'.

The twin is the statement of the arithmetic; the kernels follow it operation for operation (they are compiled without fused
multiply-adds), so the two differ only in exp / log1p and in the order of the sums:
  z = beta * l (+ bias on the last entry);  m = z's first maximum, at i_m;  w = exp(z - m);  Z' = sum of w without i_m;
  Z = 1 + Z';  l' = (z - m) - log1p(Z').
Entries that are not above -inf have probability 0: they enter no maximum and no sum, and apply leaves them as they are."""
from __future__ import annotations

from typing import Any, Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

BETA_BOX = (2.0 ** -6, 2.0 ** 6)   # beta, repair_beta
BIAS_BOX = (-32.0, 32.0)           # no_bug_bias
ARMIJO_C = 1e-4
ARMIJO_ROUNDING = 64 * 2.0 ** -52   # times |F|: what two evaluations of F may differ by in rounding alone (see newton_fit)
MAX_ITERATIONS = 50
GRADIENT_TOLERANCE = 1e-9          # times the number of samples in the fit
NOTE_BIAS_FIXED = "no_bug_bias fixed to 0: the data holds no bug-free sample or no buggy sample"
NOTE_REPAIR_FIXED = "repair_beta left at 1: the data holds no buggy sample"
LOC_COLUMNS = ("F", "dF/dbeta", "dF/dbias", "d2F/dbeta2", "d2F/dbeta dbias", "d2F/dbias2")


class ConfidenceCalibration(NamedTuple):
    """What `calibrate_model` fits and a model object carries (`model.confidence_calibration`); pickled with the checkpoint."""

    beta: float = 1.0
    no_bug_bias: float = 0.0
    repair_beta: float = 1.0
    converged: bool = True
    notes: Tuple[str, ...] = ()

    @property
    def is_identity(self) -> bool:
        return self.beta == 1.0 and self.no_bug_bias == 0.0 and self.repair_beta == 1.0


class Pool(NamedTuple):
    """Segments of fp32 log-probabilities back to back: segment s = vals[off[s] : off[s + 1]], the target at place tgt[s] of it.
    A location pool has NO_BUG at every segment's last place."""

    vals: np.ndarray  # float32 [n]
    off: np.ndarray   # int32 [nseg + 1]
    tgt: np.ndarray   # int32 [nseg]


# ---- the stats ------------------------------------------------------------------------------------------------------------
def _segment_terms(l32: np.ndarray, y: int, beta: float, bias: float, nobug: bool) -> Tuple[np.ndarray, np.ndarray]:
    """One segment's six terms and the sum of the absolute values of what each of them adds up (bl_confidence.hip's
    cf_segment_stats; the group form leaves the bias columns 0)."""
    n = l32.shape[0]
    if n == 0:
        return np.zeros(6), np.zeros(6)
    l = l32.astype(np.float64)
    keep = l > -np.inf  # False for NaN too
    if not keep.any() or not 0 <= y < n:
        return np.full(6, np.nan), np.full(6, np.nan)
    with np.errstate(invalid="ignore"):
        z = beta * l
        if nobug:
            z[n - 1] = z[n - 1] + bias
    idx = np.flatnonzero(keep)
    im = int(idx[np.argmax(z[idx])])  # the first maximum
    m = z[im]
    w = np.exp(z[idx] - m)
    lk = l[idx]
    zp = float(np.sum(w[idx != im]))
    s1 = float(np.sum(w * lk))
    a1 = float(np.sum(w * np.abs(lk)))
    Z = 1.0 + zp
    E = s1 / Z
    d = lk - E
    var = float(np.sum(w * (d * d)))
    ly = l[y]
    with np.errstate(invalid="ignore"):
        out = np.zeros(6)
        out[0] = np.log1p(zp) + (m - z[y])
        out[1] = E - ly
        out[3] = var / Z
        absolute = np.array([out[0], a1 / Z + abs(ly), 0.0, out[3], 0.0, 0.0])
        if nobug:
            ll = l[n - 1]
            p = float(np.exp(z[n - 1] - m) / Z) if keep[n - 1] else 0.0
            is_nobug = 1.0 if y == n - 1 else 0.0
            out[2] = p - is_nobug
            out[4] = p * (ll - E) if keep[n - 1] else 0.0
            out[5] = p * (1.0 - p)
            absolute[2] = p + is_nobug
            absolute[4] = p * (abs(ll) + a1 / Z) if keep[n - 1] else 0.0
            absolute[5] = p * (1.0 + p)
    return out, absolute


def _pool_stats(pool: Pool, beta: float, bias: float, nobug: bool) -> Tuple[np.ndarray, np.ndarray]:
    total, absolute = np.zeros(6), np.zeros(6)
    n_vals = pool.vals.shape[0]
    for s in range(pool.tgt.shape[0]):
        a, b = (min(max(int(pool.off[s + k]), 0), n_vals) for k in (0, 1))
        t, t_abs = _segment_terms(pool.vals[a:max(a, b)], int(pool.tgt[s]), beta, bias, nobug)
        total += t
        absolute += t_abs
    return total, absolute


def loc_stats(pool: Pool, beta: float, bias: float) -> Tuple[np.ndarray, np.ndarray]:
    """bl_conf_loc_stats in NumPy: -> (float64 [6] in the order of LOC_COLUMNS, float64 [6]: for each of them the sum of the
    absolute values of the terms it was added up from -- the scale its rounding error is measured in)."""
    return _pool_stats(pool, float(beta), float(bias), True)


def group_stats(pool: Pool, beta: float) -> Tuple[np.ndarray, np.ndarray]:
    """bl_conf_group_stats in NumPy: -> (float64 [3] = F_r | F_r' | F_r'', their absolute sums)."""
    total, absolute = _pool_stats(pool, float(beta), 0.0, False)
    return total[[0, 1, 3]], absolute[[0, 1, 3]]


# ---- the fit --------------------------------------------------------------------------------------------------------------
class FitResult(NamedTuple):
    x: Tuple[float, ...]   # (beta, bias) or (beta,)
    converged: bool
    iterations: int
    loss: float
    gradient: Tuple[float, ...]


def newton_fit(stats: Callable[[Tuple[float, ...]], Tuple[float, np.ndarray, np.ndarray]], n: int, start: Sequence[float],
               box: Sequence[Tuple[float, float]]) -> FitResult:
    """Damped Newton from `start`: stats(x) -> (F, gradient [k], Hessian [k, k]) in fp64, k = 1 or 2.  Armijo backtracking
    (c = 1e-4, the step halved each time) on the step actually taken; an iterate that leaves the box is clamped.  The test
    allows F the rounding error of its own sum, 64 ulp of |F|: next to the optimum a Newton step lowers F by less than F's last
    digits (observed on 2 000 samples: gradient 5e-6, predicted decrease 1e-14, F = 2 884 +- 5e-12), and without the allowance
    the backtracking takes whichever partial step the noise favours and never meets the gradient criterion.
    A parameter that sits on the box while the loss still falls towards the outside is held there and the Newton step is taken in
    the others alone (the full step's other components belong to a point the box forbids; kept, they crawled: 50 iterations
    without settling the bias on a pool whose beta wanted to be below 2^-6).  Stops when max|gradient| over the parameters that
    are not held <= 1e-9 n -- converged if none is held --, after 50 iterations, or when no step is left to take."""
    lo, hi = np.array([b[0] for b in box]), np.array([b[1] for b in box])
    x = np.clip(np.asarray(start, dtype=np.float64), lo, hi)
    F, g, H = stats(tuple(x))
    it = 0
    converged = False
    while True:
        if not (np.isfinite(F) and np.isfinite(g).all() and np.isfinite(H).all()):
            break
        held = ((x <= lo) & (g > 0.0)) | ((x >= hi) & (g < 0.0))
        free = np.flatnonzero(~held)
        if free.size == 0 or np.max(np.abs(g[free])) <= GRADIENT_TOLERANCE * n:
            converged = not held.any()
            break
        if it >= MAX_ITERATIONS:
            break
        it += 1
        step = np.zeros_like(x)
        solved = False
        if free.size == 1:
            i = int(free[0])
            if H[i, i] > 0.0:
                step[i] = -g[i] / H[i, i]
                solved = True
        else:
            det = H[0, 0] * H[1, 1] - H[0, 1] * H[0, 1]
            if H[0, 0] > 0.0 and det > 1e-14 * H[0, 0] * H[1, 1]:
                step = -np.array([H[1, 1] * g[0] - H[0, 1] * g[1], H[0, 0] * g[1] - H[0, 1] * g[0]]) / det
                solved = True
        if not solved or not np.isfinite(step).all():  # a flat direction: steepest descent, scaled by the curvature there is
            step = np.zeros_like(x)
            step[free] = -g[free] / max(float(np.max(np.abs(np.diag(H)))), 1e-12)
        t, moved = 1.0, False
        for _ in range(60):
            trial = np.clip(x + t * step, lo, hi)
            taken = trial - x
            if not taken.any():
                break
            Ft, gt, Ht = stats(tuple(trial))
            if np.isfinite(Ft) and Ft <= F + ARMIJO_C * float(g @ taken) + ARMIJO_ROUNDING * max(abs(F), abs(Ft)):
                x, F, g, H, moved = trial, Ft, gt, Ht, True
                break
            t *= 0.5
        if not moved:
            break
    return FitResult(tuple(float(v) for v in x), converged, it, float(F), tuple(float(v) for v in g))


def _loc_callable(fn, with_bias: bool):
    def stats(x):
        s = np.asarray(fn(x[0], x[1] if with_bias else 0.0), dtype=np.float64)
        if with_bias:
            return s[0], s[1:3].copy(), np.array([[s[3], s[4]], [s[4], s[5]]])
        return s[0], s[1:2].copy(), s[3:4].reshape(1, 1).copy()
    return stats


def fit_calibration(loc_fn: Callable[[float, float], Sequence[float]], n_samples: int, n_bug_free: int,
                    group_fn: Optional[Callable[[float], Sequence[float]]], n_buggy: int, *, fit_bias: bool = True,
                    fit_repair: bool = True) -> Tuple[ConfidenceCalibration, Dict[str, Any]]:
    """The whole fit, whoever computes the stats: loc_fn(beta, bias) -> the six sums, group_fn(beta_r) -> the three (the twin's
    `loc_stats(...)[0]`, or `hip_ops.conf_loc_stats(...)` copied to the host).  -> (calibration, details for a report)."""
    notes: List[str] = []
    with_bias = fit_bias
    if fit_bias and (n_bug_free == 0 or n_samples - n_bug_free == 0):
        with_bias = False
        notes.append(NOTE_BIAS_FIXED)
    if n_samples > 0:
        box = [BETA_BOX, BIAS_BOX] if with_bias else [BETA_BOX]
        loc = newton_fit(_loc_callable(loc_fn, with_bias), n_samples, [1.0, 0.0][:len(box)], box)
    else:
        loc = FitResult((1.0, 0.0), True, 0, 0.0, (0.0,))
    beta, bias = loc.x[0], (loc.x[1] if with_bias else 0.0)
    rep = FitResult((1.0,), True, 0, 0.0, (0.0,))
    if fit_repair and n_buggy == 0:
        notes.append(NOTE_REPAIR_FIXED)
    elif fit_repair and group_fn is not None:
        def stats(x):
            s = np.asarray(group_fn(x[0]), dtype=np.float64)
            return s[0], s[1:2].copy(), s[2:3].reshape(1, 1).copy()
        rep = newton_fit(stats, n_buggy, [1.0], [BETA_BOX])
    for name, value, (lo, hi) in (("beta", beta, BETA_BOX), ("no_bug_bias", bias, BIAS_BOX), ("repair_beta", rep.x[0], BETA_BOX)):
        if value in (lo, hi):
            notes.append(f"{name} clamped to the box [{lo:g}, {hi:g}]")
    cal = ConfidenceCalibration(beta, bias, rep.x[0], bool(loc.converged and rep.converged), tuple(notes))
    return cal, {"localization": loc._asdict(), "repair": rep._asdict()}


def fit_host(loc_pool: Pool, group_pool: Optional[Pool], *, fit_bias: bool = True, fit_repair: bool = True
             ) -> Tuple[ConfidenceCalibration, Dict[str, Any]]:
    """The fit with the twin's stats."""
    n = int(loc_pool.tgt.shape[0])
    last = np.diff(loc_pool.off.astype(np.int64)) - 1
    n_bug_free = int(np.sum(loc_pool.tgt == last))
    n_buggy = int(group_pool.tgt.shape[0]) if group_pool is not None else 0
    return fit_calibration(lambda b, c: loc_stats(loc_pool, b, c)[0], n, n_bug_free,
                           (lambda b: group_stats(group_pool, b)[0]) if group_pool is not None else None, n_buggy,
                           fit_bias=fit_bias, fit_repair=fit_repair)


# ---- apply ----------------------------------------------------------------------------------------------------------------
def _apply_segment(flat: np.ndarray, at: np.ndarray, beta: float, bias: float, nobug: bool) -> None:
    n = at.shape[0]
    if n == 0:
        return
    l = flat[at].astype(np.float64)
    keep = l > -np.inf
    if not keep.any():
        return
    with np.errstate(invalid="ignore"):
        z = beta * l
        if nobug:
            z[n - 1] = z[n - 1] + bias
    idx = np.flatnonzero(keep)
    im = int(idx[np.argmax(z[idx])])
    m = z[im]
    zp = float(np.sum(np.exp(z[idx[idx != im]] - m)))
    lz = np.log1p(zp)
    flat[at[idx]] = ((z[idx] - m) - lz).astype(np.float32)


def apply_host(flat: np.ndarray, candidate_ptr: np.ndarray, num_samples: int, repair_group_ptr: np.ndarray,
               repair_group_items: np.ndarray, cal: ConfidenceCalibration) -> None:
    """bl_conf_apply in NumPy, IN PLACE on a minibatch's flat fp32 output [loc | text | var | swap] (hip_ops.conf_apply has the
    contract): fp64 inside, rounded once to fp32."""
    assert flat.dtype == np.float32 and flat.ndim == 1
    B, n_items = int(num_samples), int(repair_group_items.shape[0])
    C = flat.shape[0] - n_items - B
    assert C >= 0 and candidate_ptr.shape[0] == B + 1
    if not (cal.beta == 1.0 and cal.no_bug_bias == 0.0):
        for b in range(B):
            c0, c1 = (min(max(int(candidate_ptr[b + k]), 0), C) for k in (0, 1))
            at = np.concatenate([np.arange(c0, max(c0, c1), dtype=np.int64), np.array([C + b], dtype=np.int64)])
            _apply_segment(flat, at, float(cal.beta), float(cal.no_bug_bias), True)
    if cal.repair_beta != 1.0:
        for g in range(repair_group_ptr.shape[0] - 1):
            g0, g1 = (min(max(int(repair_group_ptr[g + k]), 0), n_items) for k in (0, 1))
            items = repair_group_items[g0:max(g0, g1)].astype(np.int64)
            items = items[(items >= 0) & (items < n_items)]
            _apply_segment(flat, C + B + items, float(cal.repair_beta), 0.0, False)


def apply_pool_host(pool: Pool, beta: float, bias: float, nobug: bool) -> np.ndarray:
    """A pool's values after calibration (each segment as `apply_host` rewrites one), float32 [n]."""
    out = pool.vals.astype(np.float32).copy()
    for s in range(pool.tgt.shape[0]):
        _apply_segment(out, np.arange(int(pool.off[s]), int(pool.off[s + 1]), dtype=np.int64), float(beta), float(bias), nobug)
    return out


def apply_to_flat(cal: Optional[ConfidenceCalibration], flat, mb_data) -> None:
    """Calibrates the flat output `flat` (a torch tensor [loc | text | var | swap]) of the predict minibatch `mb_data` in place:
    hip_ops.conf_apply on the device, the twin on the CPU.  Nothing is launched without a calibration."""
    if cal is None or cal.is_identity:
        return
    B = int(mb_data["prediction_layout"].num_samples)
    cptr, gptr, gitems = mb_data["graph_data"]["candidate_ptr"], mb_data["repair_group_ptr"], mb_data["repair_group_items"]
    if flat.is_cuda:
        from buglab.models import hip_ops

        hip_ops.conf_apply(flat, cptr, B, gptr, gitems, beta=cal.beta, no_bug_bias=cal.no_bug_bias, repair_beta=cal.repair_beta)
    else:
        to_np = lambda t: t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
        apply_host(flat.numpy(), to_np(cptr), B, to_np(gptr), to_np(gitems), cal)


# ---- expected calibration error --------------------------------------------------------------------------------------------
def expected_calibration_error(confidence: np.ndarray, correct: np.ndarray, num_bins: int = 15) -> Tuple[float, List[Dict[str, float]]]:
    """ECE over equal-width bins of the probability `confidence` in [0, 1]: sum over bins of (share of the samples) *
    |accuracy - mean confidence|.  -> (ece, the non-empty bins)."""
    p = np.clip(np.asarray(confidence, dtype=np.float64), 0.0, 1.0)
    ok = np.asarray(correct, dtype=bool)
    assert p.shape == ok.shape and num_bins >= 1
    n = p.shape[0]
    if n == 0:
        return 0.0, []
    which = np.minimum((p * num_bins).astype(np.int64), num_bins - 1)
    ece, bins = 0.0, []
    for k in range(num_bins):
        sel = which == k
        count = int(sel.sum())
        if count == 0:
            continue
        acc, conf = float(ok[sel].mean()), float(p[sel].mean())
        ece += count / n * abs(acc - conf)
        bins.append({"lo": k / num_bins, "hi": (k + 1) / num_bins, "count": count, "accuracy": acc, "confidence": conf})
    return float(ece), bins


# ---- the index arrays of one predict minibatch ----------------------------------------------------------------------------
class CalibrationIndices(NamedTuple):
    """Where one predict minibatch's pool segments sit in its flat output (host, NumPy; built in the collate worker)."""

    loc_gather: np.ndarray  # int32 [C + B]  flat index of every location entry, sample by sample, NO_BUG last: each entry once
    loc_len: np.ndarray     # int32 [B]
    loc_tgt: np.ndarray     # int32 [B]      the target's place within its segment
    rw_gather: np.ndarray   # int32 [...]    flat index of the entries of every buggy sample's target group
    rw_len: np.ndarray      # int32 [number of buggy samples]
    rw_tgt: np.ndarray      # int32 [number of buggy samples]


def calibration_indices(layout, datapoints: Sequence[Any], tgt_loc: np.ndarray) -> CalibrationIndices:
    """`layout`: the minibatch's PredictionLayout; `tgt_loc`: SelfSupIndices.tgt_loc (the flat entry `predict` reports for the
    ground node).  The flat location part is [every sample's candidates, sample by sample | one NO_BUG entry per sample], so
    each flat entry is listed once -- `layout.loc_idx` would repeat the entry that several of a sequence model's candidates
    share.  A rewrite's group is what the model's log-softmax runs over: the rewrites of its sample at its reference node."""
    B = layout.num_samples
    n_loc = np.diff(layout.loc_off.astype(np.int64))
    C = int(n_loc.sum()) - B
    start = np.zeros(B + 1, np.int64)
    np.cumsum(n_loc - 1, out=start[1:])
    loc_gather = np.empty(C + B, np.int64)
    loc_tgt = np.empty(B, np.int64)
    rw_gather: List[np.ndarray] = []
    rw_len, rw_tgt = [], []
    for b, point in enumerate(datapoints):
        lo = int(layout.loc_off[b])
        loc_gather[lo:lo + n_loc[b] - 1] = np.arange(start[b], start[b + 1])
        loc_gather[lo + n_loc[b] - 1] = C + b
        t = int(tgt_loc[b])
        loc_tgt[b] = n_loc[b] - 1 if t >= C else t - start[b]
        assert 0 <= loc_tgt[b] < n_loc[b]
        target = point["target_fix_action_idx"]
        if target is not None:
            refs = np.asarray(point["graph"]["reference_nodes"], dtype=np.int64)
            members = np.flatnonzero(refs == refs[int(target)])
            rw_gather.append(layout.rw_idx[int(layout.rw_off[b]) + members].astype(np.int64))
            rw_len.append(members.shape[0])
            rw_tgt.append(int(np.searchsorted(members, int(target))))
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    return CalibrationIndices(i32(loc_gather), i32(n_loc), i32(loc_tgt),
                              i32(np.concatenate(rw_gather) if rw_gather else np.zeros(0, np.int64)), i32(rw_len), i32(rw_tgt))
