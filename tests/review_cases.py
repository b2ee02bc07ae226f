"""Shared by tests/test_review_host.py and tests/test_review_gpu.py: a literal, loop-by-loop restatement of the review-queue
arithmetic in Python integers (include/buglab_hip.h, "Review queue": items norm, affinity, cover, pick) and the cases.  Nothing
here imports the code under test; the rows are quantised by tests/similar_cases.py's own restatement."""
from __future__ import annotations

import functools
from operator import mul

import numpy as np

from tests.group_cases import heavy_tailed_rows, mixed_rows
from tests.similar_cases import drawn_rows, quantize_ref

NO_CENTRE = np.float64(-2.0)


# ------------------------------------------------------------------------------------------------ the restatement
def norms_ref(q):
    return np.asarray([sum(int(v) * int(v) for v in row) for row in q], np.int32)


def _ints(q):
    return [[int(v) for v in row] for row in q]


def affinity_ref(qi, qj, ni, nj) -> np.float64:
    """qi, qj: lists of Python integers.  Both products are exact integers below 2^53, so both conversions are exact; then ONE
    IEEE quotient"""
    idot = sum(map(mul, qi, qj))
    num, den = idot * abs(idot), int(ni) * int(nj)
    assert abs(num) < 2 ** 53 and 0 < den < 2 ** 53
    return np.float64(num) / np.float64(den)


def cover_ref(q, n, qc, nc, best=None, near=None, first_id=0):
    """every centre applied to every valid row: greater affinity, then the lower centre index -- the caller's state included"""
    M = len(q)
    best = np.full(M, NO_CENTRE, np.float64) if best is None else np.array(best, np.float64)
    near = np.full(M, -1, np.int32) if near is None else np.array(near, np.int32)
    rows, centres = _ints(q), _ints(qc)
    for i in range(M):
        if not n[i] > 0:
            continue
        for j in range(len(centres)):
            if not nc[j] > 0:
                continue
            a, ident = affinity_ref(rows[i], centres[j], n[i], nc[j]), first_id + j
            if near[i] < 0 or a > best[i] or (a == best[i] and ident < near[i]):
                best[i], near[i] = a, ident
    return best, near


def greedy_ref(q, n, best, near, budget, eligible=None, stop=1.0):
    """-> (picks, pick affinities, pick neighbours, best, near)"""
    M = len(q)
    best, near = np.array(best, np.float64), np.array(near, np.int32)
    rows = _ints(q)
    picks, aff, pnear = np.full(budget, -1, np.int32), np.zeros(budget, np.float64), np.full(budget, -1, np.int32)
    for k in range(budget):
        s = -1
        for i in range(M):  # the lowest best, the lowest index among equals
            if (eligible is None or eligible[i] != 0) and n[i] > 0 and best[i] < stop and (s < 0 or best[i] < best[s]):
                s = i
        if s < 0:
            break  # the queue has ended: the state stays
        picks[k], aff[k], pnear[k] = s, best[s], near[s]
        for i in range(M):
            if n[i] > 0:
                a = affinity_ref(rows[i], rows[s], n[i], n[s])
                if a > best[i]:
                    best[i], near[i] = a, s
    return picks, aff, pnear, best, near


# ------------------------------------------------------------------------------------------------ cases
def images_of(x, center=True):
    """(q int8 [M, Dp], n int32 [M]) of rows x: centred with the mean of the finite rows, quantised by the restatement"""
    x = np.asarray(x, np.float32)
    finite = np.isfinite(x).all(axis=1)
    mean = x[finite].astype(np.float64).mean(axis=0).astype(np.float32) if center and finite.any() else np.zeros(x.shape[1], np.float32)
    _, q, _, _ = quantize_ref(x, mean)
    return q, norms_ref(q)


ROWS = {"mixed": mixed_rows, "heavy": heavy_tailed_rows}


@functools.lru_cache(maxsize=None)
def cover_case(D, M=150, L=37):
    """M rows of `mixed_rows`, the first L of them the centres: every fifth row is a copy of an earlier one, so centres tie and
    the lower index must win; rows 1, 4, 7 are invalid, as rows and as centres.  -> (q, n, qc, nc, best, near) with the restated
    cover"""
    q, n = images_of(mixed_rows(M, D, seed=3 * D + 1), center=False)  # not centred: the zero row stays invalid
    qc, nc = q[:L].copy(), n[:L].copy()
    best, near = cover_ref(q, n, qc, nc)
    return q, n, qc, nc, best, near


def every_third_out(M, L=0):
    e = np.ones(M, np.uint8)
    e[:L] = 0
    e[2::3] = 0
    return e


@functools.lru_cache(maxsize=None)
def greedy_case(kind, M=300, D=100, B=40, L=20, stop=1.0, seed=5):
    """the first L rows are reviewed already; every third row and the reviewed ones are not eligible
    -> (q, n, eligible, best0, near0, (picks, affinities, neighbours, best, near))"""
    q, n = images_of(ROWS[kind](M, D, seed))
    eligible = every_third_out(M, L)
    best0, near0 = cover_ref(q, n, q[:L], n[:L])
    return q, n, eligible, best0, near0, greedy_ref(q, n, best0, near0, B, eligible, stop)


def repeated_rows(distinct=10, times=5, D=64, seed=9):
    """`distinct` drawn rows, the whole block repeated `times` times"""
    return np.tile(drawn_rows(distinct, D, seed), (times, 1))


def clustered_rows(N, D, clusters, seed, noise=0.3):
    """clusters of very different sizes (a geometric law) around drawn centres: most warnings are one of a few patterns"""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((clusters, D))
    member = np.minimum(rng.geometric(0.25, size=N) - 1, clusters - 1)
    return (centres[member] + noise * rng.standard_normal((N, D))).astype(np.float32), member
