"""The NumPy twin of the review-queue kernels (csrc/bl_review.hip), the exact selection they are measured against, and the
records behind buglab/models/review.py.  BEYOND THE REFERENCE, which has no counterpart.

A review queue is k-center greedy (farthest-point) selection: given a budget of B reviews and what was reviewed already, every
pick is the warning least like everything reviewed or queued so far (Gonzalez 1985; Sener & Savarese 2018).  The arithmetic,
stated once in include/buglab_hip.h ("Review queue") and repeated here, on `_similar.quantize_host`'s int8 images q [M, Dp] of
ONE row space -- first the L reviewed rows, then the N candidates:

  norm      n_i = sum_d q_id^2, int32 and exact, 0 for an invalid row
  affinity  a(i, j) = (double)(idot |idot|) / (double)(n_i n_j), idot = sum_d q_id q_jd: both products in int64 and below 2^53,
            ONE IEEE quotient; the signed squared cosine of the images, a(i, i) == 1.0
  cover     per row (best, near), -2.0 / -1 for "no centre yet"; a centre j applied to a valid row i replaces them iff
            a(i, j) > best_i; a set of centres gives (greater affinity, then lower centre index)
  pick      among rows with eligible != 0, n > 0 and best < stop (= S S) the lowest best, the lowest index among equals; none:
            the queue has ended, this pick and all later ones are -1 and the state stays.  Otherwise (s, best_s, near_s) is
            recorded and centre s applied to every valid row.
Every output is a function of the input alone: the device equals this bit for bit for every launch geometry -- picks, pick
affinities, pick neighbours, final best and near.
"""
from __future__ import annotations

from typing import Any, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from buglab.models._similar import MAX_D

MAX_ROWS = 1 << 20     # BL_REVIEW_MAX_ROWS
MAX_BUDGET = 16384     # BL_REVIEW_MAX_BUDGET
NO_CENTRE = -2.0       # best of a row that no centre covers
_BLOCK_ELEMENTS = 1 << 23  # rows x centres per block of cover_host (memory, not arithmetic)

END_BUDGET, END_MAX_SIMILARITY, END_NOTHING_LEFT = "budget", "max-similarity", "nothing-left"


def stop_of(max_similarity: float) -> float:
    """stop = S S of a greatest similarity S in (0, 1]; ValueError for any other value, NaN included."""
    S = float(max_similarity)
    if not 0.0 < S <= 1.0:
        raise ValueError(f"review: --max-similarity must be in (0, 1] (got {max_similarity})")
    return S * S


def cosine_of(affinity) -> np.ndarray:
    """The cosine behind an affinity (a signed squared cosine): sign(a) sqrt(|a|); NaN for "no centre yet"."""
    a = np.asarray(affinity, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(a < -1.0, np.nan, np.sign(a) * np.sqrt(np.abs(a)))


# ------------------------------------------------------------------------------------------------
# the twin
def _image(q, what: str) -> np.ndarray:
    q = np.asarray(q, np.int8)
    if q.ndim != 2 or q.shape[1] % 64 or not 64 <= q.shape[1] <= MAX_D or q.shape[0] > MAX_ROWS:
        raise ValueError(f"{what}: q {q.shape} must be [M <= {MAX_ROWS}, Dp], Dp a multiple of 64 up to {MAX_D}")
    return q


def norms_host(q) -> np.ndarray:
    """bl_review_norms in NumPy: q int8 [M, Dp] -> int32 [M]."""
    q = _image(q, "norms_host").astype(np.int32)
    return (q * q).sum(axis=1, dtype=np.int32)


def _affinity(idot: np.ndarray, ni: np.ndarray, nj) -> np.ndarray:
    """idot int64, ni, nj int64 (broadcast) -> one rounded quotient; the caller masks the pairs with a zero norm"""
    with np.errstate(invalid="ignore", divide="ignore"):
        return (idot * np.abs(idot)).astype(np.float64) / (ni * nj).astype(np.float64)


def _idot(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """integer dot products through fp32 BLAS: every product and every partial sum is an integer of magnitude at most
    512 * 127^2 < 2^24, so the result is exact whatever the order"""
    return np.rint(a @ b).astype(np.int64)


def cover_host(q, n, centres_q, centres_n, best=None, near=None, first_id: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """bl_review_cover_i8 in NumPy -> (best float64 [M], near int32 [M]); `best` / `near`: the state to combine with (copied)."""
    q, qc = _image(q, "cover_host"), _image(centres_q, "cover_host")
    n, nc = np.asarray(n, np.int64).reshape(-1), np.asarray(centres_n, np.int64).reshape(-1)
    M, L = q.shape[0], qc.shape[0]
    if q.shape[1] != qc.shape[1] or n.shape != (M,) or nc.shape != (L,):
        raise ValueError(f"cover_host: q {q.shape}, n {n.shape}, centres_q {qc.shape} and centres_n {nc.shape} do not fit")
    best = np.full(M, NO_CENTRE, np.float64) if best is None else np.array(best, np.float64)
    near = np.full(M, -1, np.int32) if near is None else np.array(near, np.int32)
    live = np.flatnonzero(nc > 0)  # ascending: the first maximum is the lower index
    if live.shape[0] == 0 or M == 0:
        return best, near
    qc_live, nc_live = qc[live].astype(np.float32).T.copy(), nc[live]
    step = max(_BLOCK_ELEMENTS // live.shape[0], 1)
    for i0 in range(0, M, step):
        rows = slice(i0, min(i0 + step, M))
        a = _affinity(_idot(q[rows].astype(np.float32), qc_live), n[rows, None], nc_live[None, :])
        j = np.argmax(np.where(n[rows, None] > 0, a, -np.inf), axis=1)
        aj, idj = a[np.arange(j.shape[0]), j], (int(first_id) + live[j]).astype(np.int32)
        b, c = best[rows], near[rows]
        take = (n[rows] > 0) & ((c < 0) | (aj > b) | ((aj == b) & (idj < c)))
        best[rows], near[rows] = np.where(take, aj, b), np.where(take, idj, c)
    return best, near


def greedy_host(q, n, best, near, budget: int, eligible=None, stop: float = 1.0
                ) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """bl_review_greedy in NumPy -> (picks int32 [B], pick_affinity float64 [B], pick_near int32 [B], best float64 [M], near
    int32 [M]); the state comes in as `best` / `near` (copied)."""
    q = _image(q, "greedy_host")
    M, B = q.shape[0], int(budget)
    n = np.asarray(n, np.int64).reshape(-1)
    best, near = np.array(best, np.float64).reshape(-1), np.array(near, np.int32).reshape(-1)
    if not 0 <= B <= MAX_BUDGET or not 0.0 < float(stop) <= 1.0:
        raise ValueError(f"greedy_host: need 0 <= budget <= {MAX_BUDGET} and stop in (0, 1] (got {budget}, {stop})")
    if n.shape != (M,) or best.shape != (M,) or near.shape != (M,):
        raise ValueError(f"greedy_host: n {n.shape}, best {best.shape} and near {near.shape} must be [{M}]")
    valid = n > 0
    open_ = valid if eligible is None else valid & (np.asarray(eligible).reshape(-1) != 0)
    picks, aff, pnear = np.full(B, -1, np.int32), np.zeros(B, np.float64), np.full(B, -1, np.int32)
    qf = q.astype(np.float32)
    for k in range(B):
        key = np.where(open_ & (best < stop), best, np.inf)
        s = int(np.argmin(key)) if M else 0  # the first minimum: the lowest index among equals
        if M == 0 or not key[s] < np.inf:
            break  # the queue has ended: the state stays
        picks[k], aff[k], pnear[k] = s, best[s], near[s]
        a = _affinity(_idot(qf, qf[s]), n, n[s])
        take = valid & (a > best)  # strict: a pick never displaces an equal earlier centre
        best[take], near[take] = a[take], s
    return picks, aff, pnear, best, near


def greedy_exact_host(c, num_reviewed: int, budget: int, eligible=None, stop: float = 1.0, first: Optional[int] = None
                      ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The same selection on the fp32 rows themselves, in fp64: c float32 [M, D] centred rows, the first `num_reviewed` of them
    the initial centres; `first`: a row that is picked and applied before the greedy starts (the cold start).  -> (picks int32
    [<= B], not padded; best float64 [M]: the signed squared cosine to the nearest centre at the end; valid bool [M]).  Used
    only to measure what the int8 images cost: nothing on the device equals it."""
    x = np.asarray(c, np.float64)
    M, L = x.shape[0], int(num_reviewed)
    with np.errstate(invalid="ignore", over="ignore"):
        s2 = (x * x).sum(axis=1)
    valid = np.isfinite(s2) & (s2 > 0.0)
    x = np.where(valid[:, None], x, 0.0)
    s2 = np.where(valid, s2, 1.0)
    best = np.full(M, NO_CENTRE, np.float64)

    def apply(rows: np.ndarray) -> None:
        rows = rows[valid[rows]]
        for j0 in range(0, rows.shape[0], 1024):
            j = rows[j0:j0 + 1024]
            d = x @ x[j].T
            a = ((d * np.abs(d)) / (s2[:, None] * s2[None, j])).max(axis=1)
            np.maximum(best, np.where(valid, a, NO_CENTRE), out=best)

    apply(np.arange(L))
    open_ = valid if eligible is None else valid & (np.asarray(eligible).reshape(-1) != 0)
    picks: List[int] = []
    if first is not None and int(budget) > 0:
        picks.append(int(first))
        apply(np.asarray([int(first)]))
    while len(picks) < int(budget):
        key = np.where(open_ & (best < stop), best, np.inf)
        s = int(np.argmin(key)) if M else 0
        if M == 0 or not key[s] < np.inf:
            break
        picks.append(s)
        apply(np.asarray([s]))
    return np.asarray(picks, np.int32), best, valid


def worst_covered(best, open_) -> float:
    """The affinity of the worst-covered open row (NaN: there is none)."""
    best, open_ = np.asarray(best, np.float64), np.asarray(open_, bool)
    return float(best[open_].min()) if open_.any() else float("nan")


def most_confident(logprobs, open_, budget: int) -> np.ndarray:
    """The `budget` open rows of the greatest log-probability, the lower index among equals: the obvious order."""
    logprobs, rows = np.asarray(logprobs, np.float64), np.flatnonzero(np.asarray(open_, bool))
    return rows[np.argsort(-logprobs[rows], kind="stable")[:max(int(budget), 0)]].astype(np.int64)


# ------------------------------------------------------------------------------------------------
# records
class Selection(NamedTuple):
    """What `review.queue_embeddings` returns for L reviewed rows and N candidates; row indices are in the one row space,
    candidates L .. L + N - 1."""

    picks: np.ndarray            # int32 [P]: the picks made, in order (P <= budget)
    pick_affinity: np.ndarray    # float64 [P]: the pick's best when it was taken (-2.0: no centre covered it)
    pick_near: np.ndarray        # int32 [P]: its nearest earlier item then: a reviewed row < L, an earlier pick, or -1
    pick_similarity: np.ndarray  # float64 [P]: the cosine to that item, re-scored in fp64 from the fp32 rows (0.0: none)
    best: np.ndarray             # float64 [M]: the final cover state
    near: np.ndarray             # int32 [M]
    valid: np.ndarray            # bool [M]
    open: np.ndarray             # bool [M]: eligible, valid candidates
    num_reviewed: int
    budget: int
    stop: float
    end: str                     # END_BUDGET, END_MAX_SIMILARITY or END_NOTHING_LEFT
    confident_worst: float       # the worst-covered open row's affinity had the `budget` most confident been reviewed instead
    mean: np.ndarray             # float32 [D]: what was subtracted from the candidates

    @property
    def worst(self) -> float:
        return worst_covered(self.best, self.open)

    @property
    def stands_for(self) -> np.ndarray:
        """per pick: how many open rows have it as their nearest item"""
        return np.bincount(self.near[self.open & (self.near >= 0)], minlength=self.best.shape[0])[self.picks]


def end_reason(num_picks: int, budget: int, num_open: int, stop: float = 1.0) -> str:
    """Why the queue ended: the budget was spent; or --max-similarity S < 1 was given and every open warning left is at least
    that similar to something reviewed or queued; or nothing is left -- every open warning was queued, or, at the default
    S = 1, what remains are exact copies (cosine 1 of the images) of reviewed or queued warnings, which the report counts as
    `num_left_as_copies`."""
    if num_picks >= budget:
        return END_BUDGET
    return END_MAX_SIMILARITY if num_open > num_picks and stop < 1.0 else END_NOTHING_LEFT


def coverage_curve(pick_affinity, final_worst: float) -> List[Dict[str, Any]]:
    """The cosine of the worst-covered open warning after 1, 2, 4, ... picks and after the last: the affinity of pick k + 1 IS the
    worst cover after k picks, so only the last point needs the final state."""
    aff = np.asarray(pick_affinity, np.float64)
    P = aff.shape[0]
    after = sorted({k for k in (1 << np.arange(0, 15)).tolist() if k < P} | ({P} if P else set()))
    out = []
    for k in after:
        a = aff[k] if k < P else final_worst
        out.append({"picks": int(k), "worst_similarity": None if np.isnan(a) or a < -1.0 else float(cosine_of(a))})
    return out


class QueuedWarning(NamedTuple):
    rank: int
    position: int
    node: int
    label: str
    filename: str
    package: str
    logprob: float
    triage_probability: Optional[float]    # None: no triage model, or an embedding that is not finite
    nearest: Optional[Dict[str, Any]]      # {"reviewed": index entry, "similarity"} or {"rank": earlier rank, "similarity"}; None: nothing earlier
    stands_for: int                        # eligible warnings whose nearest reviewed or queued item this is

    def record(self) -> Dict[str, Any]:
        out = {"rank": self.rank, "position": self.position, "node": self.node, "label": self.label, "filename": self.filename,
               "package": self.package, "logprob": self.logprob, "nearest": self.nearest, "stands_for": self.stands_for}
        if self.triage_probability is not None:
            out["triage_probability"] = self.triage_probability
        return out


class ReviewQueue(NamedTuple):
    warnings: List[QueuedWarning]
    summary: Dict[str, Any]


def _cos(a: float) -> Optional[float]:
    return None if np.isnan(a) or a < -1.0 else float(cosine_of(a))


def report(sel: Selection, num_samples: int, num_rejected: int, num_without_site: int, num_below_confidence: int,
           num_outside_band: Optional[int]) -> Dict[str, Any]:
    """The run's numbers: counts, the picks made, why the queue ended, the coverage curve, and the same worst-covered cosine for
    "review the `budget` most confident instead"."""
    L = sel.num_reviewed
    worst = sel.worst
    out: Dict[str, Any] = {"budget": int(sel.budget), "num_samples": int(num_samples), "num_rejected": int(num_rejected),
                           "num_without_site": int(num_without_site), "num_below_confidence": int(num_below_confidence),
                           "num_reviewed": int(L), "num_warnings": int(sel.best.shape[0] - L),
                           "num_invalid_embeddings": int((~sel.valid[L:]).sum()), "num_eligible": int(sel.open.sum()),
                           "num_picked": int(sel.picks.shape[0]), "end": sel.end,
                           "num_left_as_copies": int((sel.open & (sel.best >= 1.0)).sum() - sel.picks.shape[0]), "max_similarity": float(np.sqrt(sel.stop)),
                           "worst_similarity": _cos(worst), "coverage": coverage_curve(sel.pick_affinity, worst),
                           "most_confident_worst_similarity": _cos(sel.confident_worst)}
    if num_outside_band is not None:
        out["num_outside_band"] = int(num_outside_band)
    both = not np.isnan(worst) and not np.isnan(sel.confident_worst)
    out["beats_most_confident"] = bool(worst > sel.confident_worst) if both else None
    return out
