"""Shared by tests/test_group_host.py and tests/test_group_gpu.py: a literal, loop-by-loop restatement of the warning-grouping
arithmetic (include/buglab_hip.h, "Warning grouping": items edge, filter, groups) and the cases.  Nothing here imports the code
under test; the rows are quantised by tests/similar_cases.py's own restatement or by the caller."""
from __future__ import annotations

import numpy as np

from tests.similar_cases import drawn_rows, lane_dot, with_invalid_rows


def thresholds_ref(S):
    s2 = np.float64(S) * np.float64(S)
    return s2, ((np.float64(16.0) * np.float64(16129.0) * np.float64(16129.0)) * s2) * (np.float64(1.0) - np.float64(2.0) ** -40)


def row_l1_ref(q):
    return np.asarray([sum(abs(int(v)) for v in row) for row in q], np.int32)


def link_ref(c, q, sumsq, r, S):
    """ALL pairs, none filtered: -> (label, degree, num_candidates, num_edges, lost) where `lost` lists the edges the filter
    would have dropped (it must be empty) and the labels come from the edges themselves, by a naive union-find."""
    N, D = c.shape
    s2, K = thresholds_ref(S)
    l1 = row_l1_ref(q)
    parent = list(range(N))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    degree = np.zeros(N, np.int32)
    num_candidates = num_edges = 0
    lost = []
    for i in range(N):
        for j in range(i + 1, N):
            if not (r[i] > 0 and r[j] > 0):
                continue
            idot = sum(int(a) * int(b) for a, b in zip(q[i], q[j]))  # Python integers: exact
            A = 4 * idot + 2 * (int(l1[i]) + int(l1[j])) + D
            assert A * A < 2 ** 53
            candidate = A > 0 and bool((np.float64(A) * np.float64(A)) * (np.float64(r[i]) * np.float64(r[j])) >= K)
            dot = lane_dot(c[i], c[j])
            edge = bool(dot > 0.0) and bool(dot * dot >= s2 * (np.float64(sumsq[i]) * np.float64(sumsq[j])))
            num_candidates += candidate
            if edge and not candidate:
                lost.append((i, j))
            if edge:
                num_edges += 1
                degree[i] += 1
                degree[j] += 1
                a, b = find(i), find(j)
                if a != b:
                    parent[max(a, b)] = min(a, b)
    label = np.asarray([find(x) for x in range(N)], np.int32)
    return label, degree, num_candidates, num_edges, lost


# ------------------------------------------------------------------------------------------------ cases
def mixed_rows(N, D, seed, noise=0.35):
    """a few centres with noise around them: the cosine of two rows of one centre is about 1 / (1 + noise^2), 0.89 by default, so
    at S = 0.9 some pairs link, some pass the filter and fail the re-score, and most pass neither; every fifth row is a copy of
    an earlier one (the links that stay at S = 1), and rows 1, 4, 7 are invalid"""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((max(N // 8, 1), D))
    x = (centres[np.arange(N) % centres.shape[0]] + noise * rng.standard_normal((N, D))).astype(np.float32)
    for n in range(5, N, 5):
        x[n] = x[rng.integers(0, n)]
    return with_invalid_rows(x, seed)


def heavy_tailed_rows(N, D, seed):
    """Student-t (2 degrees of freedom) noise around a few centres: rows whose largest entry dwarfs the rest, where the int8
    image is at its coarsest"""
    rng = np.random.default_rng(seed)
    centres = rng.standard_t(2, size=(max(N // 6, 1), D))
    return (centres[np.arange(N) % centres.shape[0]] * (1.0 + 0.2 * rng.standard_t(2, size=(N, D)))).astype(np.float32)


def chain_rows(N=200, D=128, step=16, cos_step=0.95, seed=3):
    """rows 0, step, 2 step, ... turn by acos(cos_step) each in the plane of the first two columns, so neighbours in the chain
    link at S = 0.9 and rows two apart (cosine 0.805) do not; every other row is random in the remaining columns, unrelated to
    all.  Not to be centred.  -> (rows, the chain's row indices)"""
    x = drawn_rows(N, D, seed)
    x[:, :2] = 0.0
    chain = np.arange(0, N, step)
    theta = np.arccos(cos_step)
    for k, n in enumerate(chain):
        x[n] = 0.0
        x[n, 0], x[n, 1] = np.cos(k * theta), np.sin(k * theta)
    return x, chain
