"""Warning triage on the host: the NumPy twin of csrc/bl_triage.hip and everything of buglab/models/triage.py that is not a
kernel -- the features, the Newton driver, the folds, the choice of the ridge, the metrics, the file and the ordering.

The model (include/buglab_hip.h, "Warning triage"): for a site with embedding x [D] and location log-probability l,
    phi = ((x, l) - shift) * scale, with a 1 appended;  P = D + 2;  z = w . phi;  p = sigmoid(z)
    L(w) = sum_i c_i (softplus(z_i) - y_i z_i) + (l2 / 2) |w~|^2     (w~: everything but the intercept)
    g = Phi^T r + l2 w~,  r_i = c_i (p_i - y_i);     H = Phi^T diag(c_i p_i (1 - p_i)) Phi + l2 I~
  margins   `margins_host` restates the kernel's dot product -- lane-owned column quads in ascending order, then the xor
            butterfly -- so z is equal to the device's bit for bit
  sums      in fp64 through BLAS: the reference the device's fixed-order sums are held against, under the any-order summation
            bound (`newton_stats_host(..., with_abs=True)` returns the sums of the terms' magnitudes the bound needs)
  fit       `fit_logistic`: Newton with a Cholesky solve and step halving on L; ONE driver, the device path differs in `stats_fn`
  folds     stratified: within a class the rows are ordered by the splitmix64 key of (seed, row), `_compare`'s generator, and
            dealt round-robin
A row with a non-finite entry in x or l takes no part in any sum; it is counted."""
from __future__ import annotations

from typing import Any, Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from buglab.models._compare import _GOLDEN, _U, _mix
from buglab.models._similar import DimensionMismatch

__all__ = ["MAX_D", "MAX_SLICES", "DEFAULT_L2_GRID", "DimensionMismatch", "Stats", "Fit", "TriageModel", "standardise", "features_host",
           "margins_host", "logistic_host", "row_losses", "HostProblem", "newton_stats_host", "score_host", "fit_logistic", "stratified_folds",
           "choose_l2", "log_loss", "auc", "precision_at", "ranking_metrics", "cross_validate", "balance_weights", "rank_order",
           "probability_histogram", "slices"]

MAX_D = 512       # BL_TRIAGE_MAX_D
MAX_SLICES = 64   # BL_TRIAGE_MAX_SLICES
WAVE = 64
DEFAULT_L2_GRID = tuple(10.0 ** (k / 2.0) for k in range(-4, 7))  # 10^-2 .. 10^3 in steps of half a decade
FORMAT_VERSION = 1
SITE_MODES = ("predicted", "truth")


def slices(N: int) -> Tuple[int, int]:
    """(row slices, rows per slice) of bl_triage_newton_stats over N rows: a function of N alone."""
    S = max(1, min(MAX_SLICES, -(-int(N) // 128)))
    return S, (-(-int(N) // S) + 3) // 4 * 4


# ------------------------------------------------------------------------------------------------
# features
def finite_rows(x: np.ndarray, logprob: np.ndarray) -> np.ndarray:
    return np.isfinite(x).all(axis=1) & np.isfinite(logprob)


def standardise(x, logprob) -> Tuple[np.ndarray, np.ndarray]:
    """(shift, scale), float64 [D + 1]: the column means and inverse standard deviations of (x, logprob) over the finite rows,
    in fp64; a constant column (and every column when no row is finite) gets scale 0."""
    x, logprob = np.asarray(x, np.float32), np.asarray(logprob, np.float32)
    D = x.shape[1]
    ok = finite_rows(x, logprob)
    if not ok.any():
        return np.zeros(D + 1), np.zeros(D + 1)
    cols = np.concatenate([x[ok].astype(np.float64), logprob[ok].astype(np.float64)[:, None]], axis=1)
    shift = cols.mean(axis=0)
    std = np.sqrt(((cols - shift[None, :]) ** 2).mean(axis=0))
    with np.errstate(divide="ignore"):
        scale = np.where(std > 0.0, 1.0 / std, 0.0)
    return shift, np.where(np.isfinite(scale), scale, 0.0)


def features_host(x, logprob, shift, scale) -> Tuple[np.ndarray, np.ndarray]:
    """(Phi float64 [N, P], finite bool [N]): one rounded difference and one rounded product per entry, as the kernels form
    them; the rows that are not finite are zero."""
    x, logprob = np.asarray(x, np.float32), np.asarray(logprob, np.float32)
    N, D = x.shape
    ok = finite_rows(x, logprob)
    phi = np.zeros((N, D + 2))
    cols = np.concatenate([x[ok].astype(np.float64), logprob[ok].astype(np.float64)[:, None]], axis=1)
    phi[ok, :D + 1] = (cols - np.asarray(shift, np.float64)[None, :]) * np.asarray(scale, np.float64)[None, :]
    phi[ok, D + 1] = 1.0
    return phi, ok


def margins_host(phi: np.ndarray, w: np.ndarray) -> np.ndarray:
    """z = Phi w as ONE wave of the device forms it: column quad q belongs to lane q % 64, a lane adds the rounded products of
    its columns in ascending order to a sum that starts at +0.0, and the 64 sums go through the xor butterfly, strides 32 .. 1."""
    N, P = phi.shape
    rounds = -(-(-(-P // 4)) // WAVE)
    prod = np.zeros((N, rounds * WAVE * 4))
    prod[:, :P] = phi * np.asarray(w, np.float64)[None, :]  # padding adds +0.0, which changes no sum
    prod = prod.reshape(N, rounds, WAVE, 4)
    acc = np.zeros((N, WAVE))
    for k in range(rounds):
        for j in range(4):
            acc = acc + prod[:, k, :, j]
    lanes = np.arange(WAVE)
    o = WAVE // 2
    while o:
        acc = acc + acc[:, lanes ^ o]
        o //= 2
    return acc[:, 0].copy()


def logistic_host(z: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(p, 1 - p, log1p(exp(-|z|))) in the overflow-safe form of the kernels; softplus(u) = max(u, 0) + the third for u = +-z."""
    z = np.asarray(z, np.float64)
    e = np.exp(-np.abs(z))
    d = 1.0 + e
    big, small = 1.0 / d, e / d
    up = z >= 0.0
    return np.where(up, big, small), np.where(up, small, big), np.log1p(e)


def row_losses(z, y) -> np.ndarray:
    """softplus(z) - y z per row as the kernels form it: max(u, 0) + log1p(exp(-|z|)) with u = -z for y = 1 and z otherwise"""
    z = np.asarray(z, np.float64)
    u = np.where(np.asarray(y).astype(bool), -z, z)
    return np.where(u > 0.0, u, 0.0) + logistic_host(z)[2]


class Stats(NamedTuple):
    H: np.ndarray      # float64 [P, P]
    g: np.ndarray      # float64 [P]
    L: float
    csum: float        # sum of c over the rows used
    used: int
    skipped: int


class HostProblem:
    """The labelled rows of a fit, standardised once: `stats(w, c, l2)` and `score(w)` are the twin of the two kernels."""

    def __init__(self, x, logprob, y, shift, scale):
        self.phi, self.ok = features_host(x, logprob, shift, scale)
        self.y = np.asarray(y).astype(bool)
        self.N, self.P = self.phi.shape

    def terms(self, w, c):
        """per row: s, r, loss (zero for the rows that are not finite) and the margins"""
        w = np.asarray(w, np.float64)
        z = margins_host(self.phi, w)
        p, q, sp = logistic_host(z)
        c = np.ones(self.N) if c is None else np.asarray(c, np.float64)
        c = np.where(self.ok, c, 0.0)
        s = c * (p * q)
        r = np.where(self.y, -(c * q), c * p)
        loss = c * row_losses(z, self.y)
        return s, r, loss, c, z

    def stats(self, w, c, l2: float, with_abs: bool = False):
        w = np.asarray(w, np.float64)
        s, r, loss, c, _ = self.terms(w, c)
        ridge = np.full(self.P, float(l2))
        ridge[-1] = 0.0
        H = self.phi.T @ (s[:, None] * self.phi)
        H = 0.5 * (H + H.T) + np.diag(ridge)
        g = self.phi.T @ r + ridge * w
        L = float(loss.sum() + 0.5 * float(l2) * float((w[:-1] ** 2).sum()))
        used = int(self.ok.sum())
        st = Stats(H, g, L, float(c.sum()), used, self.N - used)
        if not with_abs:
            return st
        a = np.abs(self.phi)
        return st, (a.T @ (s[:, None] * a) + np.diag(ridge), a.T @ np.abs(r) + ridge * np.abs(w),
                    float(np.abs(loss).sum() + 0.5 * float(l2) * float((w[:-1] ** 2).sum())))

    def score(self, w) -> Tuple[np.ndarray, np.ndarray]:
        z = margins_host(self.phi, np.asarray(w, np.float64))
        p = logistic_host(z)[0]
        return np.where(self.ok, z, np.nan), np.where(self.ok, p, np.nan)


def newton_stats_host(x, logprob, shift, scale, w, y, c, l2: float, with_abs: bool = False):
    """The twin of bl_triage_newton_stats -> Stats; with `with_abs` also (sum |terms| of H, of g, of L), what the summation
    bound of the tests needs."""
    if not float(l2) > 0.0:
        raise ValueError(f"newton_stats_host: l2 must be positive (got {l2})")
    return HostProblem(x, logprob, y, shift, scale).stats(w, c, l2, with_abs)


def score_host(x, logprob, shift, scale, w) -> Tuple[np.ndarray, np.ndarray]:
    """The twin of bl_triage_score -> (margin, probability), float64 [N]; NaN for a row that is not finite."""
    x = np.asarray(x, np.float32)
    return HostProblem(x, logprob, np.zeros(x.shape[0], bool), shift, scale).score(w)


# ------------------------------------------------------------------------------------------------
# the fit
class Fit(NamedTuple):
    w: np.ndarray
    converged: bool
    iterations: int
    losses: List[float]       # L at the start and after every accepted step: never increasing
    gradient_norm: float      # |g|_inf at w
    stats: Stats


def fit_logistic(stats_fn: Callable[[np.ndarray, float], Stats], P: int, l2: float, *, max_iterations: int = 50,
                 w0: Optional[np.ndarray] = None) -> Fit:
    """Newton's method on L: the step solves H d = g by Cholesky, and is halved until L does not increase (below the resolution
    of L, until |g|_inf decreases: see the loop).  Stops when
    |g|_inf <= 1e-9 max(1, sum c) (converged) or after `max_iterations` steps, or when no step length lowers L (both: not
    converged).  `stats_fn(w, l2) -> Stats` is all that differs between the device path and the twin."""
    l2 = float(l2)
    if not l2 > 0.0:
        raise ValueError(f"fit_logistic: l2 must be positive (got {l2})")
    w = np.zeros(P) if w0 is None else np.array(w0, np.float64)
    st = stats_fn(w, l2)
    losses = [st.L]
    iterations = 0
    while True:
        gnorm = float(np.abs(st.g).max())
        if gnorm <= 1e-9 * max(1.0, st.csum):
            return Fit(w, True, iterations, losses, gnorm, st)
        if iterations >= int(max_iterations):
            return Fit(w, False, iterations, losses, gnorm, st)
        try:
            chol = np.linalg.cholesky(st.H)
        except np.linalg.LinAlgError:  # an intercept column with no curvature left (every s is 0): no Newton step exists
            return Fit(w, False, iterations, losses, gnorm, st)
        d = np.linalg.solve(chol.T, np.linalg.solve(chol, st.g))
        # Below the resolution of L the comparison of two losses says nothing: a step whose predicted decrease g.d / 2 is under
        # 1e-12 of L (some 4500 units in the last place of a sum of N rounded terms) is deep in the quadratic zone, and the full
        # step is taken if it lowers |g|_inf.  Everywhere else a step is accepted only if L does not increase.
        unresolved = 0.5 * float(st.g @ d) <= 1e-12 * max(1.0, abs(st.L))
        t, nxt = 1.0, None
        while t >= 2.0 ** -20:
            trial = stats_fn(w - t * d, l2)
            if np.isfinite(trial.L) and (trial.L <= st.L or (unresolved and t == 1.0 and float(np.abs(trial.g).max()) < gnorm)):
                nxt = trial
                break
            t *= 0.5
        if nxt is None:
            return Fit(w, False, iterations, losses, gnorm, st)
        w, st = w - t * d, nxt
        losses.append(st.L)
        iterations += 1


def stratified_folds(y, folds: int, seed: int, usable=None) -> np.ndarray:
    """fold of every row, int32 [N] (-1: not usable).  Within each class the usable rows are ordered by the key
    mix(base + row), base = mix(seed * 0x9E3779B97F4A7C15 + 0x9E3779B97F4A7C15) -- splitmix64 as `_compare` draws -- equal keys
    by row, and dealt round-robin: sizes within a class differ by at most 1, and the folds depend on (seed, y, usable) alone."""
    y = np.asarray(y).astype(bool)
    K = int(folds)
    if K < 2:
        raise ValueError(f"stratified_folds: need at least 2 folds (got {folds})")
    usable = np.ones(y.shape[0], bool) if usable is None else np.asarray(usable, bool)
    with np.errstate(over="ignore"):
        base = _mix(np.asarray(_U(int(seed) & 0xFFFFFFFFFFFFFFFF) * _GOLDEN + _GOLDEN))
        key = _mix(np.arange(y.shape[0], dtype=np.uint64) + base)
    fold = np.full(y.shape[0], -1, np.int32)
    for cls in (False, True):
        rows = np.flatnonzero(usable & (y == cls))
        rows = rows[np.lexsort((rows, key[rows]))]
        fold[rows] = np.arange(rows.shape[0]) % K
    return fold


def balance_weights(y, usable=None) -> np.ndarray:
    """c_i = N / (2 N_class) over the usable rows (1 for a class that is absent)."""
    y = np.asarray(y).astype(bool)
    usable = np.ones(y.shape[0], bool) if usable is None else np.asarray(usable, bool)
    n1, n0 = int((usable & y).sum()), int((usable & ~y).sum())
    N = n1 + n0
    return np.where(y, N / (2.0 * n1) if n1 else 1.0, N / (2.0 * n0) if n0 else 1.0)


def choose_l2(table: Sequence[Tuple[float, float]]) -> float:
    """The l2 of the lowest out-of-fold log-loss; ties go to the larger l2; a loss that is not finite never wins."""
    best = None
    for l2, loss in table:
        if not np.isfinite(loss):
            continue
        if best is None or loss < best[1] or (loss == best[1] and l2 > best[0]):
            best = (float(l2), float(loss))
    if best is None:
        raise ValueError("choose_l2: no finite loss in the table")
    return best[0]


# ------------------------------------------------------------------------------------------------
# metrics
def log_loss(z, y, c=None) -> float:
    """sum_i c_i (softplus(z_i) - y_i z_i) / sum_i c_i over the rows with a finite margin (NaN when there is none)"""
    z, y = np.asarray(z, np.float64), np.asarray(y).astype(bool)
    c = np.ones(z.shape[0]) if c is None else np.asarray(c, np.float64)
    ok = np.isfinite(z) & (c > 0.0)
    if not ok.any():
        return float("nan")
    return float((c[ok] * row_losses(z[ok], y[ok])).sum() / c[ok].sum())


def auc(score, y) -> float:
    """P(score of an accepted row > score of a dismissed one), ties counting 1/2, by average ranks; NaN without both classes.
    Rows whose score is NaN are left out."""
    score, y = np.asarray(score, np.float64), np.asarray(y).astype(bool)
    ok = ~np.isnan(score)
    score, y = score[ok], y[ok]
    n1, n0 = int(y.sum()), int((~y).sum())
    if n1 == 0 or n0 == 0:
        return float("nan")
    order = np.argsort(score, kind="stable")
    sorted_score = score[order]
    start = np.flatnonzero(np.concatenate([[True], sorted_score[1:] != sorted_score[:-1]]))
    end = np.concatenate([start[1:], [score.shape[0]]])
    rank_of_run = 0.5 * (start + 1 + end)  # the mean of the 1-based ranks start + 1 .. end
    ranks = np.empty(score.shape[0])
    ranks[order] = np.repeat(rank_of_run, end - start)
    return float((ranks[y].sum() - n1 * (n1 + 1) / 2.0) / (float(n1) * n0))


def precision_at(score, y, fraction: float) -> float:
    """The share of accepted rows among the ceil(fraction n) best scores (equal scores in input order)."""
    score, y = np.asarray(score, np.float64), np.asarray(y).astype(bool)
    ok = ~np.isnan(score)
    score, y = score[ok], y[ok]
    if score.shape[0] == 0:
        return float("nan")
    k = max(1, int(np.ceil(float(fraction) * score.shape[0])))
    return float(y[np.argsort(-score, kind="stable")[:k]].mean())


def ranking_metrics(score, y) -> Dict[str, float]:
    return {"auc": auc(score, y), "precision_at_10": precision_at(score, y, 0.10), "precision_at_25": precision_at(score, y, 0.25)}


# ------------------------------------------------------------------------------------------------
# cross-validation: the one driver of both paths
class CrossValidation(NamedTuple):
    w: np.ndarray
    l2: float
    converged: bool
    table: List[Tuple[float, float]]     # (l2, out-of-fold log-loss), in the grid's order
    oof_margin: np.ndarray               # float64 [N] at the chosen l2; NaN where a row was in no fold
    fit: Fit
    newton_iterations: int               # over every fit of the run
    all_converged: bool                  # every fold's fit at every l2


def cross_validate(problem, y, c, usable, *, folds: int = 5, seed: int = 0, l2_grid: Sequence[float] = DEFAULT_L2_GRID,
                   max_iterations: int = 50) -> CrossValidation:
    """Out-of-fold predictions for every l2 of the grid, the choice, and the fit on all rows at the chosen l2.  `problem` has
    `stats(w, c, l2) -> Stats`, `score(w) -> (z, p)` and `P`: a `HostProblem` or the device's.  A fold is a 0/1 vector multiplied
    into c.  The grid is walked from the largest l2 down, every fit starting from its fold's previous solution; a grid of one
    value is not cross-validated."""
    y = np.asarray(y).astype(bool)
    N = y.shape[0]
    c = np.ones(N) if c is None else np.asarray(c, np.float64)
    grid = [float(v) for v in l2_grid]
    if not grid or any(not (v > 0.0 and np.isfinite(v)) for v in grid):
        raise ValueError(f"triage: every l2 must be positive and finite (got {list(l2_grid)})")
    P = problem.P
    iterations, all_ok = 0, True
    table: List[Tuple[float, float]] = []
    oof_at: Dict[float, np.ndarray] = {}
    if len(grid) > 1:
        fold = stratified_folds(y, folds, seed, usable)
        masks = [np.where(fold == k, 0.0, c) for k in range(int(folds))]
        starts: List[Optional[np.ndarray]] = [None] * int(folds)
        losses: Dict[float, float] = {}
        for l2 in sorted(set(grid), reverse=True):
            oof = np.full(N, np.nan)
            for k in range(int(folds)):
                ck = masks[k]
                fit = fit_logistic(lambda w, lam: problem.stats(w, ck, lam), P, l2, max_iterations=max_iterations, w0=starts[k])
                starts[k] = fit.w
                iterations += fit.iterations
                all_ok = all_ok and fit.converged
                z, _ = problem.score(fit.w)
                oof[fold == k] = z[fold == k]
            oof_at[l2] = oof
            losses[l2] = log_loss(oof, y, np.where(fold >= 0, c, 0.0))
        table = [(l2, losses[l2]) for l2 in grid]
        chosen = choose_l2(table)
    else:
        chosen = grid[0]
    final = fit_logistic(lambda w, lam: problem.stats(w, c, lam), P, chosen, max_iterations=max_iterations)
    iterations += final.iterations
    return CrossValidation(final.w, chosen, final.converged, table, oof_at.get(chosen, np.full(N, np.nan)), final, iterations,
                           all_ok and final.converged)


# ------------------------------------------------------------------------------------------------
# the file
class TriageModel(NamedTuple):
    w: np.ndarray             # float64 [D + 2]
    shift: np.ndarray         # float64 [D + 1]
    scale: np.ndarray         # float64 [D + 1]
    l2: float
    dim: int                  # D
    site: str
    model_class: str
    fingerprint: str
    num_accepted: int
    num_dismissed: int
    cv_l2: np.ndarray         # float64 [G]: the grid (empty: --l2 was given)
    cv_log_loss: np.ndarray   # float64 [G]: the out-of-fold log-loss at each
    converged: bool

    def save(self, path) -> None:
        with open(path, "wb") as f:  # a file object: np.savez appends no suffix
            np.savez(f, format_version=np.int64(FORMAT_VERSION), w=self.w, shift=self.shift, scale=self.scale, l2=np.float64(self.l2),
                     dim=np.int64(self.dim), site=np.str_(self.site), model_class=np.str_(self.model_class),
                     fingerprint=np.str_(self.fingerprint), num_accepted=np.int64(self.num_accepted),
                     num_dismissed=np.int64(self.num_dismissed), cv_l2=self.cv_l2, cv_log_loss=self.cv_log_loss,
                     converged=np.bool_(self.converged))

    @classmethod
    def load(cls, path) -> "TriageModel":
        with np.load(path, allow_pickle=False) as z:
            if int(z["format_version"]) != FORMAT_VERSION:
                raise ValueError(f"{path}: triage format {int(z['format_version'])}; this version reads {FORMAT_VERSION}")
            m = cls(z["w"], z["shift"], z["scale"], float(z["l2"]), int(z["dim"]), str(z["site"]), str(z["model_class"]),
                    str(z["fingerprint"]), int(z["num_accepted"]), int(z["num_dismissed"]), z["cv_l2"], z["cv_log_loss"],
                    bool(z["converged"]))
        D = m.dim
        if any(a.dtype != np.float64 for a in (m.w, m.shift, m.scale, m.cv_l2, m.cv_log_loss)) or m.w.shape != (D + 2,) \
                or m.shift.shape != (D + 1,) or m.scale.shape != (D + 1,) or m.cv_l2.shape != m.cv_log_loss.shape or not 1 <= D <= MAX_D:
            raise ValueError(f"{path}: inconsistent triage arrays")
        return m

    def check_model(self, model_class: str, dim: int, fingerprint: str) -> Optional[str]:
        """DimensionMismatch for embeddings of another size; otherwise a warning text when the re-ranker was fitted on another
        model's embeddings (class or weights), None when it is this one."""
        if int(dim) != self.dim:
            raise DimensionMismatch(f"the triage file was fitted on embeddings of size {self.dim} ({self.model_class}); the model's "
                                    f"are of size {int(dim)}")
        if fingerprint != self.fingerprint or model_class != self.model_class:
            return (f"the triage file was fitted with other weights ({self.model_class} {self.fingerprint[:12]}) than the model's "
                    f"({model_class} {fingerprint[:12]}): it ranks embeddings of another model")
        return None


# ------------------------------------------------------------------------------------------------
# ranking
def rank_order(prob, logprob, position) -> np.ndarray:
    """The order of a ranked scan: triage probability descending, then log-probability descending, then position; rows without
    a probability (NaN) last, among themselves by the same two later keys."""
    prob, logprob = np.asarray(prob, np.float64), np.asarray(logprob, np.float64)
    missing = np.isnan(prob)
    return np.lexsort((np.asarray(position), -logprob, -np.where(missing, 0.0, prob), missing))


def probability_histogram(prob) -> List[int]:
    """ten bins of width 0.1 over the probabilities that exist; 1.0 falls into the last"""
    prob = np.asarray(prob, np.float64)
    prob = prob[~np.isnan(prob)]
    return np.bincount(np.minimum((prob * 10.0).astype(np.int64), 9), minlength=10).tolist()
