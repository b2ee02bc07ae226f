"""The NumPy twin of the warning-tracking kernels (csrc/bl_track.hip) and the records behind buglab/models/track.py.  BEYOND THE
REFERENCE, which has no counterpart.

Tracking is a ONE-TO-ONE matching of the warnings of two scans.  The arithmetic, stated once in include/buglab_hip.h ("Warning
tracking") and repeated here, on `_similar.quantize_host`'s int8 images in ONE row space -- L old rows, a `SiteIndex`'s
embeddings, already centred; N new rows, centred with the index's mean:

  norm        n_i = sum_d q_id^2, `_review.norms_host`'s: int32 and exact, 0 for an invalid row
  affinity    review's: a(i, j) = (double)(idot |idot|) / (double)(n_i n_j), both products in int64, ONE IEEE quotient
  admissible  a pair (old i, new j) with n_i > 0, n_j > 0, a(i, j) >= floor (= S S for --min-similarity S in (0, 1]) and, when
              keys are given, key_old[i] == key_new[j]
  matching    repeatedly the first admissible pair of two unmatched rows in the order (greater affinity, then lower old index,
              then lower new index); stop when none is left.  The unique stable matching under that order.
  rounds      the device's way: every open row of either side finds its best admissible open row of the other (the lower index
              among equals), EVERY pair that chose each other is matched, a round that matches nothing ends the matching.

`match_host` is the SEQUENTIAL definition -- it collects the admissible pairs in row blocks, orders them and walks the order --
deliberately another algorithm than the device's, so that equality is a real check; `rounds_host` is bl_track_match's twin, call
for call.  Every output is a function of the input alone.
"""
from __future__ import annotations

from typing import Any, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from buglab.models._review import MAX_ROWS, _affinity, _idot, _image

NO_PARTNER = -2.0          # best of a row that found nothing admissible
MAX_ROUNDS = 4096          # BL_TRACK_MAX_ROUNDS
_BLOCK_ELEMENTS = 1 << 23  # pairs per block (memory, not arithmetic)

STATUS_NEW, STATUS_PERSISTING, STATUS_GONE = "new", "persisting", "gone"
WITHIN = ("none", "file", "package")


def floor_of(min_similarity: float) -> float:
    """floor = S S of a least similarity S in (0, 1]; ValueError for any other value, NaN included."""
    S = float(min_similarity)
    if not 0.0 < S <= 1.0:
        raise ValueError(f"track: --min-similarity must be in (0, 1] (got {min_similarity})")
    return S * S


def _check_floor(what: str, floor: float) -> float:
    floor = float(floor)
    if not 0.0 < floor <= 1.0:
        raise ValueError(f"{what}: floor must be in (0, 1]: the square of a similarity in (0, 1] (got {floor})")
    return floor


# ------------------------------------------------------------------------------------------------
# the twin
def _sides(what: str, qx, nx, qy, ny, keyx, keyy):
    qx, qy = _image(qx, what), _image(qy, what)
    nx, ny = np.asarray(nx, np.int64).reshape(-1), np.asarray(ny, np.int64).reshape(-1)
    if qx.shape[1] != qy.shape[1] or nx.shape != (qx.shape[0],) or ny.shape != (qy.shape[0],):
        raise ValueError(f"{what}: images {qx.shape} / {qy.shape} and norms {nx.shape} / {ny.shape} do not fit")
    if (keyx is None) != (keyy is None):
        raise ValueError(f"{what}: the keys of both sides come together")
    if keyx is not None:
        keyx, keyy = np.asarray(keyx, np.int32).reshape(-1), np.asarray(keyy, np.int32).reshape(-1)
        if keyx.shape != nx.shape or keyy.shape != ny.shape:
            raise ValueError(f"{what}: keys {keyx.shape} / {keyy.shape} must be [{nx.shape[0]}] / [{ny.shape[0]}]")
    return qx, nx, qy, ny, keyx, keyy


def _open(mask, n: int) -> np.ndarray:
    return np.ones(n, bool) if mask is None else np.asarray(mask).reshape(-1) != 0


def best_host(qx, nx, qy, ny, floor: float, keyx=None, keyy=None, openx=None, openy=None) -> Tuple[np.ndarray, np.ndarray]:
    """bl_track_best_i8 in NumPy -> (best float64 [X], arg int32 [X]): per open row of the first side the best admissible open row
    of the second, the lower index among equals; (-2.0, -1) for none and for a row that is not open."""
    what = "best_host"
    qx, nx, qy, ny, keyx, keyy = _sides(what, qx, nx, qy, ny, keyx, keyy)
    floor = _check_floor(what, floor)
    X, Y = qx.shape[0], qy.shape[0]
    best, arg = np.full(X, NO_PARTNER, np.float64), np.full(X, -1, np.int32)
    rows = np.flatnonzero(_open(openx, X) & (nx > 0))
    cols = np.flatnonzero(_open(openy, Y) & (ny > 0))  # ascending: the first maximum is the lower index
    if rows.shape[0] == 0 or cols.shape[0] == 0:
        return best, arg
    qy_t, ny_c = qy[cols].astype(np.float32).T.copy(), ny[cols]
    step = max(_BLOCK_ELEMENTS // cols.shape[0], 1)
    for i0 in range(0, rows.shape[0], step):
        r = rows[i0:i0 + step]
        a = _affinity(_idot(qx[r].astype(np.float32), qy_t), nx[r, None], ny_c[None, :])
        ok = a >= floor
        if keyx is not None:
            ok &= keyx[r, None] == keyy[None, cols]
        a = np.where(ok, a, -np.inf)
        j = np.argmax(a, axis=1)
        aj = a[np.arange(j.shape[0]), j]
        found = aj > -np.inf
        best[r[found]], arg[r[found]] = aj[found], cols[j[found]]
    return best, arg


def fresh_state(L: int, N: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(match_old int32 [L], match_new int32 [N], match_aff float64 [N]) of a matching that has not begun"""
    return np.full(L, -1, np.int32), np.full(N, -1, np.int32), np.zeros(N, np.float64)


def rounds_host(q_old, n_old, q_new, n_new, floor: float, state=None, max_rounds: int = 64, key_old=None, key_new=None
                ) -> Tuple[Tuple[np.ndarray, np.ndarray, np.ndarray], np.ndarray]:
    """bl_track_match in NumPy: up to `max_rounds` rounds of mutual best from `state` (copied; None: fresh) ->
    ((match_old, match_new, match_aff), status int32 [4]: rounds of this call that matched something | pairs matched by this call
    | whether the matching has ended | open new rows left)."""
    what = "rounds_host"
    q_old, n_old, q_new, n_new, key_old, key_new = _sides(what, q_old, n_old, q_new, n_new, key_old, key_new)
    floor = _check_floor(what, floor)
    if not 1 <= int(max_rounds) <= MAX_ROUNDS:
        raise ValueError(f"{what}: max_rounds must be in [1, {MAX_ROUNDS}] (got {max_rounds})")
    L, N = q_old.shape[0], q_new.shape[0]
    m_old, m_new, m_aff = fresh_state(L, N) if state is None else (np.array(state[0], np.int32), np.array(state[1], np.int32),
                                                                  np.array(state[2], np.float64))
    if m_old.shape != (L,) or m_new.shape != (N,) or m_aff.shape != (N,):
        raise ValueError(f"{what}: the state must be [{L}], [{N}], [{N}]")
    rounds = pairs = ended = 0
    for _ in range(int(max_rounds)):
        open_old, open_new = m_old < 0, m_new < 0
        _, arg_old = best_host(q_old, n_old, q_new, n_new, floor, key_old, key_new, open_old, open_new)
        best_new, arg_new = best_host(q_new, n_new, q_old, n_old, floor, key_new, key_old, open_new, open_old)
        j = np.flatnonzero(arg_new >= 0)
        j = j[arg_old[arg_new[j]] == j]  # the pairs that chose each other
        if j.shape[0] == 0:
            ended = 1
            break
        m_old[arg_new[j]], m_new[j], m_aff[j] = j, arg_new[j], best_new[j]
        rounds, pairs = rounds + 1, pairs + int(j.shape[0])
    return (m_old, m_new, m_aff), np.asarray([rounds, pairs, ended, int((m_new < 0).sum())], np.int32)


def admissible_pairs_host(q_old, n_old, q_new, n_new, floor: float, key_old=None, key_new=None
                          ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Every admissible pair as (old int64 [P], new int64 [P], affinity float64 [P]), collected in row blocks, in no
    particular order that matters."""
    L = q_old.shape[0]
    cols = np.flatnonzero(n_new > 0)
    rows = np.flatnonzero(n_old > 0)
    out_i: List[np.ndarray] = [np.zeros(0, np.int64)]
    out_j: List[np.ndarray] = [np.zeros(0, np.int64)]
    out_a: List[np.ndarray] = [np.zeros(0, np.float64)]
    if L == 0 or cols.shape[0] == 0 or rows.shape[0] == 0:
        return out_i[0], out_j[0], out_a[0]
    q_t, n_c = q_new[cols].astype(np.float32).T.copy(), n_new[cols]
    step = max(_BLOCK_ELEMENTS // cols.shape[0], 1)
    for i0 in range(0, rows.shape[0], step):
        r = rows[i0:i0 + step]
        a = _affinity(_idot(q_old[r].astype(np.float32), q_t), n_old[r, None], n_c[None, :])
        ok = a >= floor
        if key_old is not None:
            ok &= key_old[r, None] == key_new[None, cols]
        bi, bj = np.nonzero(ok)
        out_i.append(r[bi].astype(np.int64)), out_j.append(cols[bj].astype(np.int64)), out_a.append(a[bi, bj])
    return np.concatenate(out_i), np.concatenate(out_j), np.concatenate(out_a)


def match_host(q_old, n_old, q_new, n_new, floor: float, key_old=None, key_new=None
               ) -> Tuple[np.ndarray, np.ndarray, np.ndarray, int]:
    """The SEQUENTIAL definition -> (match_old int32 [L], match_new int32 [N], match_aff float64 [N], rounds): all admissible
    pairs in the order (greater affinity, lower old index, lower new index), each taken when both of its rows are still
    unmatched.  `rounds` is what the rounds of mutual best need for the same matching (`rounds_host`, run to its end)."""
    what = "match_host"
    q_old, n_old, q_new, n_new, key_old, key_new = _sides(what, q_old, n_old, q_new, n_new, key_old, key_new)
    floor = _check_floor(what, floor)
    m_old, m_new, m_aff = fresh_state(q_old.shape[0], q_new.shape[0])
    pi, pj, pa = admissible_pairs_host(q_old, n_old, q_new, n_new, floor, key_old, key_new)
    order = np.lexsort((pj, pi, -pa))
    for i, j, a in zip(pi[order].tolist(), pj[order].tolist(), pa[order].tolist()):
        if m_old[i] < 0 and m_new[j] < 0:
            m_old[i], m_new[j], m_aff[j] = j, i, a
    rounds, state = 0, None
    while True:
        state, status = rounds_host(q_old, n_old, q_new, n_new, floor, state, 64, key_old, key_new)
        rounds += int(status[0])
        if status[2]:
            break
    return m_old, m_new, m_aff, rounds


# ------------------------------------------------------------------------------------------------
# records
class Matching(NamedTuple):
    """What `track.match_embeddings` returns for L old and N new rows."""

    match_old: np.ndarray    # int32 [L]: the new row an old row is matched to, -1: gone
    match_new: np.ndarray    # int32 [N]: the old row a new row is matched to, -1: new
    affinity: np.ndarray     # float64 [N]: the affinity of the images of a matched pair (0.0: unmatched)
    similarity: np.ndarray   # float64 [N]: its cosine, re-scored in fp64 from the fp32 rows (0.0: unmatched)
    rounds: int              # rounds of mutual best that matched something
    floor: float
    valid_old: np.ndarray    # bool [L]
    valid_new: np.ndarray    # bool [N]

    @property
    def num_matched(self) -> int:
        return int((self.match_new >= 0).sum())


class TrackedWarning(NamedTuple):
    status: str              # "new", "persisting" or "gone"
    position: int
    node: int
    label: str
    filename: str
    package: str
    logprob: Optional[float]         # None for a gone warning: the index keeps no log-probability
    previous: Optional[Dict[str, Any]]  # persisting: the index entry (with its tag) and "similarity"; gone: the index entry
    tag: str                         # the tag this warning carries (into --write-index; a gone one: the tag it had)

    def record(self) -> Dict[str, Any]:
        if self.status == STATUS_GONE:
            return {"status": STATUS_GONE, **self.previous}
        out: Dict[str, Any] = {"status": self.status, "position": self.position, "node": self.node, "label": self.label,
                               "filename": self.filename, "package": self.package, "logprob": self.logprob}
        if self.previous is not None:
            out["previous"] = self.previous
        return out


class TrackedScan(NamedTuple):
    warnings: List[TrackedWarning]   # the listed warnings of DATA in input order, then the gone ones in index order
    summary: Dict[str, Any]
    index: Any                       # the new scan as a SiteIndex (tags inherited), what --write-index saves
    hidden: List[TrackedWarning]     # the persisting warnings --hide-tag left out


def within_keys(within: str, old_paths: Sequence[str], old_packages: Sequence[str], new_paths: Sequence[str],
                new_packages: Sequence[str]) -> Tuple[Optional[np.ndarray], Optional[np.ndarray]]:
    """int32 keys of both sides, numbered over the union of both sides in sorted order; (None, None) for "none"."""
    if within not in WITHIN:
        raise ValueError(f"track: --within must be one of {WITHIN} (got {within!r})")
    if within == "none":
        return None, None
    old, new = (old_paths, new_paths) if within == "file" else (old_packages, new_packages)
    old, new = [str(v) for v in old], [str(v) for v in new]
    number = {name: k for k, name in enumerate(sorted(set(old) | set(new)))}
    return np.asarray([number[v] for v in old], np.int32).reshape(-1), np.asarray([number[v] for v in new], np.int32).reshape(-1)


def report(warnings: Sequence[TrackedWarning], hidden: Sequence[TrackedWarning], matching: Matching, within: str, num_samples: int,
           num_rejected: int, num_without_site: int, num_below_confidence: int, other_weights: bool) -> Dict[str, Any]:
    """The run's numbers: the counts of new, persisting, gone and hidden, the same per tag, the rounds, the floor and `within`,
    the samples that gave no warning, and the lowest listed cosine."""
    count = lambda status: sum(1 for w in warnings if w.status == status)
    by_tag: Dict[str, Dict[str, int]] = {}
    for w, status in [(w, w.status) for w in warnings] + [(w, "hidden") for w in hidden]:
        by_tag.setdefault(w.tag, {STATUS_NEW: 0, STATUS_PERSISTING: 0, STATUS_GONE: 0, "hidden": 0})[status] += 1
    listed = [w.previous["similarity"] for w in warnings if w.status == STATUS_PERSISTING]
    return {"num_samples": int(num_samples), "num_rejected": int(num_rejected), "num_without_site": int(num_without_site),
            "num_below_confidence": int(num_below_confidence), "num_old": int(matching.match_old.shape[0]),
            "num_warnings": int(matching.match_new.shape[0]), "num_invalid_embeddings": int((~matching.valid_new).sum()),
            "num_new": count(STATUS_NEW), "num_persisting": count(STATUS_PERSISTING), "num_gone": count(STATUS_GONE),
            "num_hidden": len(hidden), "by_tag": {tag: by_tag[tag] for tag in sorted(by_tag)}, "rounds": int(matching.rounds),
            "min_similarity": float(np.sqrt(matching.floor)), "floor": float(matching.floor), "within": within,
            "lowest_listed_similarity": min(listed) if listed else None, "other_weights": bool(other_weights)}


__all__ = ["MAX_ROWS", "MAX_ROUNDS", "NO_PARTNER", "Matching", "TrackedWarning", "TrackedScan", "floor_of", "best_host", "rounds_host",
           "match_host", "admissible_pairs_host", "fresh_state", "within_keys", "report"]
