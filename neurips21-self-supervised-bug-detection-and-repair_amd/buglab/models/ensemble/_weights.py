"""Fitted ensembles: the value a `weighted` ensemble carries, the NumPy fp64 twin of csrc/bl_ensemble_fit.hip, and the fit.

Beyond the reference, whose ensembles (buglab/models/ensemble/wrapper.py:33-89) give every present member the weight 1 / M':
stacking on held-out data, without retraining anything.  Per sample, with P the present members and l_m member m's own fp32
log-probabilities (as `predict` yields them without calibration):
  locations  z_m = beta_m l_m;  s_m = z_m - LSE z_m;  a_m = theta_m - LSE_{k in P} theta_k;  out_i = LSE_{m in P} (a_m + s_m[i])
  rewrites   b_m = phi_m - LSE_{k in P} phi_k;         out_r = LSE_{m in P} (b_m + l_m[r])
theta_0 = phi_0 = 0 are fixed (only differences of weights matter).  A beta_m that is EXACTLY 1 leaves the member's values as
they are (s_m = l_m): a member's fp32 log-softmax sums to 1 only up to fp32 rounding, and the identity parameters
theta = phi = 0, beta = 1 are then `avg` up to the rounding of log(M') -- the rule `_calibrate.apply_host` has for its identity.
The losses  F_loc = -sum over samples of out[y_loc]  and  F_rw = -sum over buggy samples of out[y_rw]  have closed-form
gradients: with the responsibilities r_m = exp(a_m + s_m[y] + F_sample) and pi = softmax of theta over P,
  dF/dtheta_m = -(r_m - pi_m),    dF/dbeta_m = -r_m (l_m[y] - E_m[l]),  E_m[l] = sum_i exp(s_m[i]) l_m[i].

The twin is the statement of the arithmetic; the kernels follow it operation for operation (they are compiled without fused
multiply-adds), so the two differ only in exp / log1p and in the order of the sums.  Every LSE of the statistics subtracts its
FIRST maximum and takes log1p of the sum without it; entries that are not above -inf have probability 0: they enter no maximum
and no sum and are never multiplied."""
from __future__ import annotations

from typing import Any, Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from buglab.models._calibrate import ARMIJO_C, ARMIJO_ROUNDING, BETA_BOX, GRADIENT_TOLERANCE, MAX_ITERATIONS

WEIGHT_BOX = (-20.0, 20.0)  # theta, phi: a member whose weight wants to go to 0 stops at exp(-20) of the strongest one's
NOTE_NO_BUGGY = "phi left at 0: the data holds no buggy sample"


def note_member_absent(m: int, head: str) -> str:
    return f"member {m} is present in no {head} sample of the data: its parameters stay at the identity"


class EnsembleWeights(NamedTuple):
    """What `fit_ensemble_weights` fits and a `weighted` EnsembleWrapper carries (`ensemble_weights`); pickled with the file."""

    theta: Tuple[float, ...]                  # location weights (log scale), theta[0] = 0
    beta: Tuple[float, ...]                   # inverse temperatures of the members' location distributions
    phi: Tuple[float, ...]                    # rewrite weights (log scale), phi[0] = 0
    fitted_on: Tuple[int, int] = (0, 0)       # (samples, buggy samples) of the fit; (0, 0): not fitted
    nll_before: Tuple[float, float] = (float("nan"), float("nan"))  # (location NLL per sample, rewrite NLL per buggy sample) of `avg`
    nll_after: Tuple[float, float] = (float("nan"), float("nan"))   # the same with these parameters
    notes: Tuple[str, ...] = ()

    @classmethod
    def identity(cls, M: int) -> "EnsembleWeights":
        return cls((0.0,) * M, (1.0,) * M, (0.0,) * M)

    @property
    def is_identity(self) -> bool:
        return not any(self.theta) and not any(self.phi) and all(b == 1.0 for b in self.beta)

    def member_weights(self) -> Tuple[np.ndarray, np.ndarray]:
        """The softmax of theta and of phi over ALL members: the weights of a sample every member predicts."""
        return tuple(np.exp(_log_weights(np.asarray(p, np.float64), np.ones(len(p), bool))[0]) for p in (self.theta, self.phi))


class LocPool(NamedTuple):
    """Every member's location segments in the canonical layout (nodes ascending, NO_BUG last), back to back: member m's values of
    segment s = vals[m, off[s] : off[s + 1]], the target at place tgt[s]; present[m, s]: member m predicts sample s."""

    vals: np.ndarray     # float32 [M, total]
    present: np.ndarray  # int32 [M, S]
    off: np.ndarray      # int32 [S + 1]
    tgt: np.ndarray      # int32 [S]


class RwPool(NamedTuple):
    """Every member's log-probability of the true rewrite of each buggy sample."""

    vals: np.ndarray     # float32 [M, S]
    present: np.ndarray  # int32 [M, S]


# ---- the mixture ------------------------------------------------------------------------------------------------------------
def _first_max(values: np.ndarray, keep: np.ndarray) -> int:
    idx = np.flatnonzero(keep)
    return int(idx[np.argmax(values[idx])]) if idx.size else -1


def _log_weights(w: np.ndarray, present: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """a = w - LSE of w over the present members and pi = the softmax there (both 0 for an absent member): ef_log_weights."""
    a, pi = np.zeros(w.shape[0]), np.zeros(w.shape[0])
    km = _first_max(w, present)
    if km < 0:
        return a, pi
    e = np.where(present, np.exp(np.where(present, w, w[km]) - w[km]), 0.0)
    tz = float(np.sum(e[np.arange(w.shape[0]) != km]))
    a[present] = (w[present] - w[km]) - np.log1p(tz)
    pi[present] = e[present] / (1.0 + tz)
    return a, pi


def _mix(w: np.ndarray, v: np.ndarray, present: np.ndarray) -> Tuple[float, np.ndarray, np.ndarray, np.ndarray]:
    """One sample's mixture over the members (ef_mix): v = each member's log-probability of the target.
    -> (F = -LSE_{m in P} (a_m + v_m), the responsibilities r, dF/dw = -(r - pi), pi)."""
    M = w.shape[0]
    if not present.any():
        return 0.0, np.zeros(M), np.zeros(M), np.zeros(M)
    a, pi = _log_weights(w, present)
    with np.errstate(invalid="ignore"):
        c = a + v
    counted = present & (c > -np.inf)  # False for NaN too
    mm = _first_max(c, counted)
    if mm < 0:
        nan = np.full(M, np.nan)
        return float("nan"), nan, nan.copy(), pi
    others = counted & (np.arange(M) != mm)
    cz = float(np.sum(np.exp(c[others] - c[mm])))
    F = (-c[mm]) - np.log1p(cz)
    r = np.zeros(M)
    r[counted] = np.exp(c[counted] + F)
    g = np.where(present, -(r - pi), 0.0)
    return float(F), r, g, pi


def _member_segment(l32: np.ndarray, beta: float) -> Optional[Tuple[np.ndarray, float, float, np.ndarray, float]]:
    """One member's segment at its inverse temperature: (l in fp64, the first maximum m of beta l, log1p(Z'), w = exp(beta l - m)
    with 0 on the skipped entries, Z' = the sum of w without the maximum); None when nothing is above -inf."""
    l = l32.astype(np.float64)
    keep = l > -np.inf
    with np.errstate(invalid="ignore"):
        z = beta * l
    im = _first_max(z, keep)
    if im < 0:
        return None
    w = np.zeros(l.shape[0])
    w[keep] = np.exp(z[keep] - z[im])
    zp = float(np.sum(w[keep & (np.arange(l.shape[0]) != im)]))
    return l, float(z[im]), float(np.log1p(zp)), w, zp


def loc_stats(pool: LocPool, theta: Sequence[float], beta: Sequence[float]) -> Tuple[np.ndarray, np.ndarray]:
    """bl_ens_loc_stats in NumPy: -> (float64 [1 + 2M] = F | dF/dtheta | dF/dbeta, float64 [1 + 2M]: for each of them the sum of
    the absolute values of the terms it was added up from -- the scale its rounding error is measured in)."""
    theta, beta = np.asarray(theta, np.float64), np.asarray(beta, np.float64)
    M, total = pool.vals.shape
    S = pool.tgt.shape[0]
    out, absolute = np.zeros(1 + 2 * M), np.zeros(1 + 2 * M)
    for s in range(S):
        a, b = (min(max(int(pool.off[s + k]), 0), total) for k in (0, 1))
        n, y = max(a, b) - a, int(pool.tgt[s])
        here = (pool.present[:, s] != 0) & (n > 0)
        sy, ly, E, A = np.zeros(M), np.zeros(M), np.zeros(M), np.zeros(M)
        broken = False
        for m in np.flatnonzero(here):
            seg = _member_segment(pool.vals[m, a:a + n], float(beta[m]))
            if seg is None or not 0 <= y < n:
                broken = True
                break
            l, mx, lz, w, zp = seg
            keep = l > -np.inf
            ly[m] = l[y]
            E[m] = float(np.sum(w[keep] * l[keep])) / (1.0 + zp)
            A[m] = float(np.sum(w[keep] * np.abs(l[keep]))) / (1.0 + zp)
            with np.errstate(invalid="ignore"):
                sy[m] = ly[m] if beta[m] == 1.0 else (beta[m] * ly[m] - mx) - lz
        if broken:
            out += np.nan
            absolute += np.nan
            continue
        F, r, g, pi = _mix(theta, sy, here)
        with np.errstate(invalid="ignore"):
            gb = np.where(r > 0.0, -(r * (ly - E)), np.where(np.isnan(r), r, 0.0))
            gb_abs = np.where(r > 0.0, r * (np.abs(ly) + A), np.where(np.isnan(r), r, 0.0))
        out += np.concatenate([[F], g, gb])
        absolute += np.concatenate([[abs(F)], np.where(here, np.abs(r) + pi, 0.0), gb_abs])
    return out, absolute


def rw_stats(pool: RwPool, phi: Sequence[float]) -> Tuple[np.ndarray, np.ndarray]:
    """bl_ens_rw_stats in NumPy: -> (float64 [1 + M] = F | dF/dphi, their absolute sums)."""
    phi = np.asarray(phi, np.float64)
    M, S = pool.vals.shape
    out, absolute = np.zeros(1 + M), np.zeros(1 + M)
    for s in range(S):
        here = pool.present[:, s] != 0
        F, r, g, pi = _mix(phi, np.where(here, pool.vals[:, s].astype(np.float64), 0.0), here)
        out += np.concatenate([[F], g])
        absolute += np.concatenate([[abs(F)], np.where(here, np.abs(r) + pi, 0.0)])
    return out, absolute


# ---- combine ----------------------------------------------------------------------------------------------------------------
def _fold(terms: List[np.ndarray]) -> np.ndarray:
    with np.errstate(all="ignore"):
        r = terms[0]
        for t in terms[1:]:
            r = np.logaddexp(r, t)
    return r


def combine_sample(locs: Sequence[Optional[np.ndarray]], rws: Sequence[Optional[np.ndarray]], theta, beta, phi
                   ) -> Optional[Tuple[np.ndarray, np.ndarray]]:
    """One sample: per member its location values in the canonical order and its rewrite values (None: the member is absent)
    -> (locations, rewrites) in fp64, the present members folded in member order with np.logaddexp; None without a member."""
    theta, beta, phi = (np.asarray(p, np.float64) for p in (theta, beta, phi))
    present = np.array([l is not None for l in locs])
    if not present.any():
        return None
    a, _ = _log_weights(theta, present)
    b, _ = _log_weights(phi, present)
    loc_terms, rw_terms = [], []
    for m in np.flatnonzero(present):
        l = np.asarray(locs[m], np.float32)
        s = l.astype(np.float64)
        seg = None if beta[m] == 1.0 else _member_segment(l, float(beta[m]))
        if seg is not None:
            keep = s > -np.inf
            s[keep] = (beta[m] * s[keep] - seg[1]) - seg[2]
        loc_terms.append(a[m] + s)
        rw_terms.append(b[m] + np.asarray(rws[m], np.float32).astype(np.float64))
    return _fold(loc_terms), _fold(rw_terms)


def combine_weighted(src: np.ndarray, loc_idx: np.ndarray, loc_off: np.ndarray, rw_idx: np.ndarray, rw_off: np.ndarray, theta, beta,
                     phi) -> Tuple[np.ndarray, np.ndarray]:
    """bl_ensemble_combine_weighted in NumPy, over the same gather arguments -> (out_loc float64 [total_loc], out_rw float64
    [total_rw]); a sample no member predicts gets NaN."""
    M = loc_idx.shape[0]
    out_loc, out_rw = np.full(loc_idx.shape[1], np.nan), np.full(rw_idx.shape[1], np.nan)
    for b in range(loc_off.shape[0] - 1):
        ls, rs = slice(int(loc_off[b]), int(loc_off[b + 1])), slice(int(rw_off[b]), int(rw_off[b + 1]))
        here = [ls.stop > ls.start and loc_idx[m, ls.start] >= 0 for m in range(M)]
        c = combine_sample([src[loc_idx[m, ls]] if here[m] else None for m in range(M)],
                           [src[rw_idx[m, rs]] if here[m] else None for m in range(M)], theta, beta, phi)
        if c is not None:
            out_loc[ls], out_rw[rs] = c
    return out_loc, out_rw


# ---- the fit ----------------------------------------------------------------------------------------------------------------
class FitResult(NamedTuple):
    x: Tuple[float, ...]
    converged: bool            # the gradient criterion is met over the parameters that are not held on their box
    on_box: Tuple[int, ...]    # the parameters held on their box at the end
    iterations: int
    evaluations: int
    loss: float
    start_loss: float
    gradient: Tuple[float, ...]


def bfgs_fit(stats: Callable[[np.ndarray], Tuple[float, np.ndarray]], n: int, start: Sequence[float],
             box: Sequence[Tuple[float, float]]) -> FitResult:
    """Gradient-only quasi-Newton (BFGS on the inverse Hessian) with projection onto the box, from `start`: stats(x) -> (F,
    gradient [k]) in fp64.  A parameter whose box is a point is fixed.  A parameter that sits on its box while the loss still
    falls towards the outside is held there, and the step is taken in the others alone.  Armijo backtracking (c = 1e-4, the step
    halved each time) on the step actually taken after the projection, with `_calibrate.newton_fit`'s allowance of 64 ulp of |F|
    for the rounding of F's own sum -- and a step is accepted only if it does not raise F, so the loss at the end is never above
    the loss at the start.  When no step along the quasi-Newton direction is accepted, the curvature is forgotten and steepest
    descent is tried once.  Stops when max|gradient| over the parameters that are not held <= 1e-9 n (converged), after 50
    iterations, or when no step is left to take."""
    lo, hi = np.array([b[0] for b in box], np.float64), np.array([b[1] for b in box], np.float64)
    fixed = lo == hi
    x = np.clip(np.asarray(start, dtype=np.float64), lo, hi)
    F, g = stats(x)
    F0, evaluations = float(F), 1
    k = x.shape[0]
    H, fresh = np.eye(k), True
    it, converged = 0, False
    while True:
        if not (np.isfinite(F) and np.isfinite(g).all()):
            break
        held = fixed | ((x <= lo) & (g > 0.0)) | ((x >= hi) & (g < 0.0))
        free = np.flatnonzero(~held)
        if free.size == 0 or np.max(np.abs(g[free])) <= GRADIENT_TOLERANCE * n:
            converged = True
            break
        if it >= MAX_ITERATIONS:
            break
        it += 1
        moved = False
        for attempt in range(2):
            step = np.zeros(k)
            if fresh:  # no curvature yet: steepest descent, a first step of length at most 1
                step[free] = -g[free] / max(1.0, float(np.max(np.abs(g[free]))))
            else:
                step[free] = -(H[np.ix_(free, free)] @ g[free])
                if not np.isfinite(step).all() or float(g @ step) >= 0.0:
                    H, fresh = np.eye(k), True
                    continue
            t = 1.0
            for _ in range(60):
                trial = np.clip(x + t * step, lo, hi)
                taken = trial - x
                if not taken.any():
                    break
                Ft, gt = stats(trial)
                evaluations += 1
                if np.isfinite(Ft) and np.isfinite(gt).all() and Ft <= F and \
                        Ft <= F + ARMIJO_C * float(g @ taken) + ARMIJO_ROUNDING * max(abs(F), abs(Ft)):
                    moved = True
                    break
                t *= 0.5
            if moved or fresh:
                break
            H, fresh = np.eye(k), True
        if not moved:
            break
        s, yv = np.zeros(k), np.zeros(k)
        s[free], yv[free] = taken[free], (gt - g)[free]
        sy = float(s @ yv)
        if sy > 1e-12 * float(np.linalg.norm(s) * np.linalg.norm(yv)):
            if fresh:  # the usual first scaling of the inverse Hessian
                H, fresh = np.eye(k) * (sy / float(yv @ yv)), False
            rho = 1.0 / sy
            V = np.eye(k) - rho * np.outer(s, yv)
            H = V @ H @ V.T + rho * np.outer(s, s)
        x, F, g = trial, Ft, gt
    held = ~fixed & (((x <= lo) & (g > 0.0)) | ((x >= hi) & (g < 0.0)))
    return FitResult(tuple(float(v) for v in x), converged, tuple(int(i) for i in np.flatnonzero(held)), it, evaluations, float(F), F0,
                     tuple(float(v) for v in g))


def fit_weights(loc_fn: Callable[[np.ndarray, np.ndarray], Sequence[float]], n_samples: int, loc_present: np.ndarray,
                rw_fn: Optional[Callable[[np.ndarray], Sequence[float]]], n_buggy: int, rw_present: np.ndarray, *,
                fit_temperature: bool = True) -> Tuple[EnsembleWeights, Dict[str, Any]]:
    """The whole fit, whoever computes the statistics: loc_fn(theta, beta) -> F | dF/dtheta | dF/dbeta, rw_fn(phi) -> F | dF/dphi
    (the twin's `loc_stats(...)[0]`, or `hip_ops.ens_loc_stats(...)` copied to the host).  loc_present / rw_present: bool [M],
    whether the member is present in any sample / any buggy sample.  -> (weights, details for a report)."""
    M = int(loc_present.shape[0])
    notes: List[str] = []
    point = lambda v: (v, v)
    loc_box = [point(0.0) if (m == 0 or not loc_present[m]) else WEIGHT_BOX for m in range(M)] + \
              [BETA_BOX if (fit_temperature and loc_present[m]) else point(1.0) for m in range(M)]
    notes += [note_member_absent(m, "fitting") for m in range(M) if not loc_present[m]]

    def loc(x):
        s = np.asarray(loc_fn(x[:M], x[M:]), dtype=np.float64)
        return float(s[0]), s[1:].copy()

    if n_samples > 0:
        fl = bfgs_fit(loc, n_samples, [0.0] * M + [1.0] * M, loc_box)
    else:
        fl = FitResult((0.0,) * M + (1.0,) * M, True, (), 0, 0, 0.0, 0.0, (0.0,) * (2 * M))
    fr = FitResult((0.0,) * M, True, (), 0, 0, 0.0, 0.0, (0.0,) * M)
    if n_buggy == 0 or rw_fn is None:
        notes.append(NOTE_NO_BUGGY)
    else:
        notes += [note_member_absent(m, "buggy") for m in range(M) if loc_present[m] and not rw_present[m]]
        rw_box = [point(0.0) if (m == 0 or not rw_present[m]) else WEIGHT_BOX for m in range(M)]

        def rw(x):
            s = np.asarray(rw_fn(x), dtype=np.float64)
            return float(s[0]), s[1:].copy()

        fr = bfgs_fit(rw, n_buggy, [0.0] * M, rw_box)
    theta, beta, phi = fl.x[:M], fl.x[M:], fr.x
    for name, values, (lo, hi) in (("theta", theta, WEIGHT_BOX), ("beta", beta, BETA_BOX), ("phi", phi, WEIGHT_BOX)):
        notes += [f"{name}[{m}] clamped to the box [{lo:g}, {hi:g}]" for m, v in enumerate(values) if v in (lo, hi)]
    if not (fl.converged and fr.converged):
        notes.append(f"the fit stopped after {MAX_ITERATIONS} iterations or for want of a step, before its gradient criterion was met")
    per = lambda total, count: total / count if count else float("nan")
    weights = EnsembleWeights(tuple(theta), tuple(beta), tuple(phi), (int(n_samples), int(n_buggy)),
                              (per(fl.start_loss, n_samples), per(fr.start_loss, n_buggy)),
                              (per(fl.loss, n_samples), per(fr.loss, n_buggy)), tuple(notes))
    return weights, {"localization": fl._asdict(), "rewrite": fr._asdict()}


def fit_host(loc_pool: LocPool, rw_pool: RwPool, *, fit_temperature: bool = True) -> Tuple[EnsembleWeights, Dict[str, Any]]:
    """The fit with the twin's statistics."""
    return fit_weights(lambda t, b: loc_stats(loc_pool, t, b)[0], int(loc_pool.tgt.shape[0]), (loc_pool.present != 0).any(axis=1),
                       lambda p: rw_stats(rw_pool, p)[0], int(rw_pool.vals.shape[1]), (rw_pool.present != 0).any(axis=1),
                       fit_temperature=fit_temperature)
