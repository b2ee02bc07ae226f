"""Shared by tests/test_similar_host.py and tests/test_similar_gpu.py: a literal, loop-by-loop restatement of the similar-bug
search arithmetic (include/buglab_hip.h, "Similar-bug search": items centre, row, quantise, key, search, re-score), the cases,
and a bitwise comparison.  Nothing here imports the code under test."""
from __future__ import annotations

import numpy as np

WAVE = 64
MAX_CANDIDATES = 16


def assert_equal_bits(got, want, what=""):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, i, g.dtype, w.dtype, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            gb = np.ascontiguousarray(g).reshape(-1).view(np.uint8).reshape(g.size, -1)
            wb = np.ascontiguousarray(w).reshape(-1).view(np.uint8).reshape(w.size, -1)
            diff = np.flatnonzero((gb != wb).any(axis=1))
            raise AssertionError(f"{what}: output {i} differs at {diff.shape[0]} of {g.size} places; the first is {diff[0]}: "
                                 f"{g.reshape(-1)[diff[0]]!r} vs {w.reshape(-1)[diff[0]]!r}")


# ------------------------------------------------------------------------------------------------ the restatement
def lane_dot(x, y) -> np.float64:
    """sum_d x_d y_d as one wave forms it: lane l owns the quads q % 64 == l, adds its columns' products in ascending order to
    a sum that starts at +0.0; then the xor butterfly, strides 32 .. 1"""
    D = len(x)
    lanes = [np.float64(0.0) for _ in range(WAVE)]
    for d in range(D):  # ascending d visits every lane's columns in ascending order
        lane = (d // 4) % WAVE
        lanes[lane] = lanes[lane] + np.float64(x[d]) * np.float64(y[d])
    o = WAVE // 2
    while o > 0:
        lanes = [lanes[l] + lanes[l ^ o] for l in range(WAVE)]
        o //= 2
    return lanes[0]


def quantize_ref(x, mean):
    x, mean = np.asarray(x, np.float32), np.asarray(mean, np.float32)
    N, D = x.shape
    Dp = (D + 63) // 64 * 64
    c, q = np.zeros((N, D), np.float32), np.zeros((N, Dp), np.int8)
    sumsq, r = np.zeros(N, np.float64), np.zeros(N, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for n in range(N):
            for d in range(D):
                c[n, d] = np.float32(np.float64(x[n, d]) - np.float64(mean[d]))
            amax, finite = np.float32(0.0), True
            for d in range(D):
                a = abs(c[n, d])
                finite = finite and bool(a < np.float32(np.inf))
                if a > amax:
                    amax = a
            if not finite or not amax > 0:
                continue
            s = lane_dot(c[n], c[n])
            scale = np.float64(127.0) / np.float64(amax)
            for d in range(D):
                q[n, d] = np.int8(np.rint(np.float64(c[n, d]) * scale))
            sumsq[n], r[n] = s, (np.float64(amax) * np.float64(amax)) / s
    return c, q, sumsq, r


def search_ref(qx, rx, qy, ry, C):
    Q, N = qx.shape[0], qy.shape[0]
    out_idx, out_key = np.full((Q, C), -1, np.int32), np.zeros((Q, C), np.float64)
    for i in range(Q):
        if not rx[i] > 0:
            continue
        found = []
        for j in range(N):
            if not ry[j] > 0:
                continue
            idot = sum(int(a) * int(b) for a, b in zip(qx[i], qy[j]))  # Python integers: exact
            assert abs(idot) < 2 ** 31
            key = np.float64(idot * abs(idot)) * np.float64(ry[j])     # an integer below 2^53 converts exactly; one rounded product
            found.append((-key, j, key))
        found.sort(key=lambda t: (t[0], t[1]))  # greater key, or the same key at the lower index
        for place, (_, j, key) in enumerate(found[:C]):
            out_idx[i, place], out_key[i, place] = j, key
    return out_idx, out_key


def rescore_ref(cx, cy, sumsq_y, cand, k):
    Q, C = cand.shape
    out_idx, out_dot = np.full((Q, k), -1, np.int32), np.zeros((Q, k), np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for i in range(Q):
            found = []
            for place in range(C):
                j = int(cand[i, place])
                if not 0 <= j < cy.shape[0] or not sumsq_y[j] > 0:
                    continue
                dot = lane_dot(cx[i], cy[j])
                key2 = (dot * abs(dot)) / np.float64(sumsq_y[j])
                if key2 != key2:
                    continue
                found.append((-key2, j, place, dot))
            found.sort(key=lambda t: t[:3])
            for place, (_, j, _, dot) in enumerate(found[:k]):
                out_idx[i, place], out_dot[i, place] = j, dot
    return out_idx, out_dot


# ------------------------------------------------------------------------------------------------ cases
def drawn_rows(N, D, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((N, D)) * scale).astype(np.float32)


def tie_rows(N, D, seed):
    """a {-1, 0, 1} alphabet with every third row a copy of an earlier one: exact key ties are the rule, the index decides"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-1, 2, size=(N, D)).astype(np.float32)
    for n in range(2, N, 3):
        x[n] = x[rng.integers(0, n)]
    return x


def with_invalid_rows(x, seed):
    """rows 1, 4, 7 (where they exist) become a zero row, a NaN row and an inf row"""
    x = x.copy()
    for n, v in ((1, 0.0), (4, np.nan), (7, np.inf)):
        if n < x.shape[0]:
            x[n] = 0.0
            x[n, (seed + n) % x.shape[1]] = v
    return x


def brute_force_top(x, y, k):
    """the k nearest rows of x (by cosine, fp64, the lower index among equals) of every row of y, and the cosines"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    cos = (y @ x.T) / np.sqrt((y * y).sum(1)[:, None] * (x * x).sum(1)[None, :])
    order = np.argsort(-cos, axis=1, kind="stable")[:, :k]
    return order, np.take_along_axis(cos, order, axis=1)


def embed_case():
    """A handmade flat output and layout with B = 5 samples, D = 6: (flat, loc_idx, loc_off, cand_rows, h, truth).
    sample 0: three candidates, the second wins                   -> predicted place 1
    sample 1: NO_BUG wins (skip_nobug: the first of two equal candidates)  -> none / place 0
    sample 2: a NaN that would win; an out-of-range flat index     -> place 2
    sample 3: one candidate whose row of h is out of range         -> none
    sample 4: no candidates at all (NO_BUG only)                   -> none
    truth: 2, -1, 0, 0, 5 (the last out of range)"""
    nan = np.float32(np.nan)
    #                  candidates (flat 0 .. 8)                             NO_BUG (flat 9 .. 13)
    flat = np.array([-2.0, -0.5, -0.5, -1.5, -1.5, nan, -2.0, -2.5, -0.1, -1.0, -0.2, -4.0, -5.0, 0.0, 7.0, 8.0], np.float32)
    loc_idx = np.array([0, 1, 2, 9,   3, 4, 10,   5, 99, 6, 7, 11,   8, 12,   13], np.int32)
    loc_off = np.array([0, 4, 7, 12, 14, 15], np.int32)
    cand_rows = np.array([3, 0, 5, 2, 2, 1, 4, 6, 40], np.int32)  # the last points outside h
    rng = np.random.default_rng(7)
    h = rng.standard_normal((7, 6)).astype(np.float32)
    truth = np.array([2, -1, 0, 0, 5], np.int32)
    return flat, loc_idx, loc_off, cand_rows, h, truth
