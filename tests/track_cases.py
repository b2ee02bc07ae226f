"""Shared by tests/test_track_host.py and tests/test_track_gpu.py: a literal restatement of the warning-tracking arithmetic in
Python integers and Fractions (include/buglab_hip.h, "Warning tracking": affinity, admissible pairs, the sequential matching,
the rounds of mutual best) and the cases.  Nothing here imports the code under test; rows are quantised by
tests/similar_cases.py's own restatement."""
from __future__ import annotations

import functools
from fractions import Fraction

import numpy as np

from tests.group_cases import heavy_tailed_rows, mixed_rows
from tests.review_cases import images_of, norms_ref, repeated_rows
from tests.similar_cases import drawn_rows, quantize_ref

NO_PARTNER = -2.0


# ------------------------------------------------------------------------------------------------ the restatement
def affinities_ref(q_old, n_old, q_new, n_new):
    """a [L][N] as Python floats, None where a norm is not > 0.  idot is an exact integer (an int64 product of the images: no
    rounding anywhere), both products are Python integers below 2^53, and the quotient of the two is rounded ONCE: a Fraction's
    float is the correctly rounded quotient, which is what one IEEE division of the two exactly converted integers gives."""
    idot = (np.asarray(q_old, np.int64) @ np.asarray(q_new, np.int64).T).tolist()
    out = []
    for i, ni in enumerate(int(v) for v in n_old):
        row = []
        for j, nj in enumerate(int(v) for v in n_new):
            if ni > 0 and nj > 0:
                d = int(idot[i][j])
                num, den = d * abs(d), ni * nj
                assert abs(num) < 2 ** 53 and 0 < den < 2 ** 53
                row.append(float(Fraction(num, den)))
            else:
                row.append(None)
        out.append(row)
    return out


def transposed(aff, L, N):
    return [[aff[i][j] for i in range(L)] for j in range(N)]


def admissible_ref(aff, i, j, floor, key_old=None, key_new=None):
    a = aff[i][j]
    return a is not None and a >= floor and (key_old is None or int(key_old[i]) == int(key_new[j]))


def best_ref(aff, X, Y, floor, keyx=None, keyy=None, openx=None, openy=None):
    """per open row of the first side (best, arg): greater affinity, then the lower index; (-2.0, -1) for none and for a row
    that is not open"""
    best, arg = np.full(X, NO_PARTNER, np.float64), np.full(X, -1, np.int32)
    for i in range(X):
        if openx is not None and not openx[i]:
            continue
        for j in range(Y):
            if openy is not None and not openy[j]:
                continue
            if admissible_ref(aff, i, j, floor, keyx, keyy) and (arg[i] < 0 or aff[i][j] > best[i]):
                best[i], arg[i] = aff[i][j], j
    return best, arg


def fresh(L, N):
    return np.full(L, -1, np.int32), np.full(N, -1, np.int32), np.zeros(N, np.float64)


def match_ref(aff, L, N, floor, key_old=None, key_new=None):
    """the SEQUENTIAL definition: the admissible pairs in the order (greater affinity, lower old index, lower new index), each
    taken when both of its rows are still unmatched -> (match_old, match_new, match_aff)"""
    pairs = sorted((-aff[i][j], i, j) for i in range(L) for j in range(N) if admissible_ref(aff, i, j, floor, key_old, key_new))
    m_old, m_new, m_aff = fresh(L, N)
    for neg, i, j in pairs:
        if m_old[i] < 0 and m_new[j] < 0:
            m_old[i], m_new[j], m_aff[j] = j, i, -neg
    return m_old, m_new, m_aff


def match_literal_ref(aff, L, N, floor, key_old=None, key_new=None):
    """the definition word for word, for small cases: REPEATEDLY search all pairs for the first of the order"""
    m_old, m_new, m_aff = fresh(L, N)
    while True:
        first = None
        for i in range(L):
            for j in range(N):
                if m_old[i] < 0 and m_new[j] < 0 and admissible_ref(aff, i, j, floor, key_old, key_new) \
                        and (first is None or aff[i][j] > aff[first[0]][first[1]]):  # (i, j) ascends: ties keep the earlier pair
                    first = (i, j)
        if first is None:
            return m_old, m_new, m_aff
        i, j = first
        m_old[i], m_new[j], m_aff[j] = j, i, aff[i][j]


def rounds_ref(aff, L, N, floor, key_old=None, key_new=None, state=None, max_rounds=1 << 30):
    """rounds of mutual best from `state` -> ((match_old, match_new, match_aff), [rounds that matched something, pairs matched,
    ended, open new rows left], [pairs per round])"""
    m_old, m_new, m_aff = fresh(L, N) if state is None else tuple(np.array(s) for s in state)
    aff_t = transposed(aff, L, N)
    rounds = pairs = ended = 0
    per_round = []
    for _ in range(max_rounds):
        open_old, open_new = m_old < 0, m_new < 0
        _, arg_old = best_ref(aff, L, N, floor, key_old, key_new, open_old, open_new)
        best_new, arg_new = best_ref(aff_t, N, L, floor, key_new, key_old, open_new, open_old)
        mutual = [(int(arg_new[j]), j) for j in range(N) if arg_new[j] >= 0 and arg_old[arg_new[j]] == j]
        if not mutual:
            ended = 1
            break
        for i, j in mutual:
            m_old[i], m_new[j], m_aff[j] = j, i, best_new[j]
        rounds, pairs = rounds + 1, pairs + len(mutual)
        per_round.append(len(mutual))
    return (m_old, m_new, m_aff), np.asarray([rounds, pairs, ended, int((m_new < 0).sum())], np.int32), per_round


def blocking_pairs(aff, L, N, floor, m_old, m_new, key_old=None, key_new=None):
    """the admissible pairs in which EACH side would come before its partner (or has none): a stable matching has none"""
    def before(a, idx, partner_a, partner_idx):  # (a, idx) comes before the partner in that row's order
        return partner_idx < 0 or a > partner_a or (a == partner_a and idx < partner_idx)

    out = []
    for i in range(L):
        for j in range(N):
            if not admissible_ref(aff, i, j, floor, key_old, key_new) or m_old[i] == j:
                continue
            pi, pj = int(m_old[i]), int(m_new[j])
            if before(aff[i][j], j, aff[i][pi] if pi >= 0 else 0.0, pi) and before(aff[i][j], i, aff[pj][j] if pj >= 0 else 0.0, pj):
                out.append((i, j))
    return out


# ------------------------------------------------------------------------------------------------ cases
def keys3(n, shift=0):
    return ((np.arange(n) + shift) % 3).astype(np.int32)


def every_third_closed(n, first=2):
    o = np.ones(n, np.uint8)
    o[first::3] = 0
    return o


def _both_sides(x_old, x_new):
    """int8 images and norms of both sides in one row space (not centred: a zero row stays invalid)"""
    zero = np.zeros(x_old.shape[1], np.float32)
    q_old, q_new = quantize_ref(x_old, zero)[1], quantize_ref(x_new, zero)[1]
    return q_old, norms_ref(q_old), q_new, norms_ref(q_new)


@functools.lru_cache(maxsize=None)
def best_case(D, X=150, Y=37):
    """X rows of `mixed_rows` (copies among them, rows 1, 4, 7 invalid) against Y rows made of them: a third exact copies, the
    rest with noise, rows 1, 4, 7 invalid again -> (q_x, n_x, q_y, n_y, aff)"""
    x = mixed_rows(X, D, seed=3 * D + 2)
    rng = np.random.default_rng(D)
    y = x[rng.integers(0, X, size=Y)].copy()
    noisy = np.arange(Y) % 3 != 0
    y[noisy] += (0.3 * rng.standard_normal((int(noisy.sum()), D))).astype(np.float32)
    y[[1, 4, 7]] = x[[1, 4, 7]]
    q_x, n_x, q_y, n_y = _both_sides(x, y)
    return q_x, n_x, q_y, n_y, affinities_ref(q_x, n_x, q_y, n_y)


@functools.lru_cache(maxsize=None)
def match_case(L=150, N=131, D=100, seed=11):
    """an old scan of `mixed_rows` and a new one: 100 of the old rows in another order, every fourth an exact copy and the others
    with noise, then 31 fresh rows; rows 1, 4, 7 of the old scan and 2, 5 of the new are invalid -> (q_old, n_old, q_new, n_new,
    aff)"""
    rng = np.random.default_rng(seed)
    old = mixed_rows(L, D, seed=seed)
    kept = rng.permutation(L)[:N - 31]
    new = old[kept].copy()
    noisy = np.arange(new.shape[0]) % 4 != 0
    scale = np.where(np.arange(int(noisy.sum())) % 2 == 0, 0.2, 0.6)[:, None]  # cosines of about 0.98 and 0.86: a floor decides
    new[noisy] += (scale * rng.standard_normal((int(noisy.sum()), D))).astype(np.float32)
    new = np.concatenate([new, drawn_rows(31, D, seed + 1)])
    new[[2, 5]] = 0.0
    q_old, n_old, q_new, n_new = _both_sides(old, new)
    return q_old, n_old, q_new, n_new, affinities_ref(q_old, n_old, q_new, n_new)


def prototype_case(seed, L=14, N=12, invalid=True):
    """int8 images drawn from 6 prototypes with entries in -3 .. 3 in a few columns: almost every pair ties with another.  Zero
    rows are the invalid ones -> (q_old, n_old, q_new, n_new, aff)"""
    rng = np.random.default_rng(seed)
    proto = rng.integers(-3, 4, size=(6, 5)).astype(np.int8)
    proto[(proto == 0).all(axis=1), 0] = 1

    def side(n):
        q = np.zeros((n, 64), np.int8)
        q[:, :5] = proto[rng.integers(0, 6, size=n)]
        if invalid and n > 3:
            q[rng.integers(0, n, size=2)] = 0
        return q, norms_ref(q)

    q_old, n_old = side(L)
    q_new, n_new = side(N)
    return q_old, n_old, q_new, n_new, affinities_ref(q_old, n_old, q_new, n_new)


@functools.lru_cache(maxsize=None)
def chain_case(k=7):
    """k old and k new points in a plane at alternating angles o_0 < n_0 < o_1 < n_1 < ... with strictly decreasing gaps: every
    old point prefers the new point after it, every new point the old point after it, so only the LAST pair is mutual -- and
    again in every round among what is left: k rounds of one pair each -> (q_old, n_old, q_new, n_new, aff)"""
    gaps = np.arange(2 * k, 1, -1, dtype=np.float64)  # 2 k - 1 gaps in the ratio 2 k : ... : 2, scaled to a span of 80 degrees
    angles = np.deg2rad(np.concatenate([[0.0], np.cumsum(gaps * (80.0 / gaps.sum()))]))
    x = np.zeros((2 * k, 64), np.float32)
    x[:, 0], x[:, 1] = np.cos(angles), np.sin(angles)
    q_old, n_old, q_new, n_new = _both_sides(x[0::2], x[1::2])
    return q_old, n_old, q_new, n_new, affinities_ref(q_old, n_old, q_new, n_new)


@functools.lru_cache(maxsize=None)
def copies_case():
    """10 distinct rows five times on both sides: every affinity of a pattern with itself is 1.0, the index order decides"""
    x = repeated_rows()
    q, n = images_of(x, center=False)
    return q, n, q.copy(), n.copy(), affinities_ref(q, n, q, n)


@functools.lru_cache(maxsize=None)
def ragged_case():
    """1100 old rows against 77 of them as new rows: more than one row tile on either side, ragged last tiles"""
    q, n = images_of(heavy_tailed_rows(1100, 100, seed=4))
    q_new, n_new = q[1000:1077].copy(), n[1000:1077].copy()
    return q, n, q_new, n_new, affinities_ref(q, n, q_new, n_new)
