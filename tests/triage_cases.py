"""Shared inputs of the warning-triage tests (tests/test_triage_host.py, tests/test_triage_gpu.py): drawn rows, the weightings
and the hard cases of the Newton statistics, and the twin's results for them, computed once per case and not changed."""
from __future__ import annotations

from functools import lru_cache
from typing import Dict, Tuple

import numpy as np

# (N, D): the smallest shapes at which the tiling can go wrong.  P = D + 2 = 6, 16 (one tile exactly), 32 (two), 64, 66 (just over
# four tiles: a second block of tiles), 128, 514 (the cap: 33 tiles, 9 blocks).  N = 1 and 3 are below one MFMA k-step of 4 rows,
# 67, 130, 513 and 4099 are no multiples of 4; the slice rule (S = min(64, ceil(N / 128)), ceil(N / S) rounded up to 4 rows each)
# gives 130 -> 2 slices (68 + 62), 513 -> 5 (4 x 104 + 97), 1000 -> 8 (7 x 128 + 104), 4099 -> 33 (32 x 128 + 3).
STAT_SHAPES = [(1, 4), (3, 14), (67, 30), (130, 62), (1000, 64), (4099, 126), (513, 512)]
WEIGHTINGS = ("ones", "fold", "balance")
HARD_CASES = ("zero_slice", "single_class", "non_finite", "far_margins")
L2 = 0.75


def drawn_rows(N: int, D: int, seed: int) -> Tuple[np.ndarray, np.ndarray]:
    """embeddings with unequal column scales and offsets, and log-probabilities of probabilities in (0.01, 1)"""
    rng = np.random.default_rng(seed)
    x = (rng.normal(size=(N, D)) * rng.uniform(0.2, 3.0, size=D)[None, :] + rng.normal(size=D)[None, :]).astype(np.float32)
    return x, np.log(rng.uniform(0.01, 1.0, size=N)).astype(np.float32)


def problem(N: int, D: int, seed: int = 0) -> Dict[str, np.ndarray]:
    """rows, labels that follow a direction plus noise, shift / scale of the rows, and a weight vector with margins of a few units"""
    from buglab.models import _triage as R

    rng = np.random.default_rng(1000 + seed)
    x, lp = drawn_rows(N, D, seed)
    y = (x.astype(np.float64) @ rng.normal(size=D) + rng.normal(size=N) > 0.0)
    if N >= 2:
        y[0], y[1] = True, False  # both classes, whatever the draw
    shift, scale = R.standardise(x, lp) if N > 1 else (np.zeros(D + 1), np.ones(D + 1))
    w = rng.normal(size=D + 2) * (2.0 / np.sqrt(D + 2))
    return {"x": x, "logprob": lp, "y": y.astype(np.uint8), "shift": shift, "scale": scale, "w": w}


def weights(kind: str, y: np.ndarray):
    from buglab.models import _triage as R

    if kind == "ones":
        return None
    if kind == "fold":  # the 0/1 vector of a fit that leaves fold 0 out
        return (R.stratified_folds(y, 5, 3) != 0).astype(np.float64) if y.shape[0] >= 2 else np.ones(y.shape[0])
    if kind == "balance":
        return R.balance_weights(y)
    raise ValueError(kind)


def hard_case(kind: str) -> Tuple[Dict[str, np.ndarray], object]:
    """(problem, c) of one of the hard cases, at (1000, 64): 8 slices of 128 rows"""
    from buglab.models import _triage as R

    p = problem(1000, 64, seed=7)
    c = None
    if kind == "zero_slice":  # every weight of slice 2 (rows 256 .. 383) is zero
        assert R.slices(1000) == (8, 128)
        c = np.ones(1000)
        c[256:384] = 0.0
    elif kind == "single_class":
        p["y"] = np.ones(1000, np.uint8)
    elif kind == "non_finite":
        p["x"][5, 3], p["x"][700, 63] = np.nan, np.nan
        p["logprob"][129] = np.inf
    elif kind == "far_margins":  # the margins reach +-800
        z = R.margins_host(R.features_host(p["x"], p["logprob"], p["shift"], p["scale"])[0], p["w"])
        p["w"] = p["w"] * (800.0 / np.abs(z).max())
    else:
        raise ValueError(kind)
    return p, c


@lru_cache(maxsize=None)
def twin_stats(N: int, D: int, weighting: str):
    """(problem, c, Stats, (abs H, abs g, abs L), (margin, probability)) of a drawn shape: the twin, once"""
    from buglab.models import _triage as R

    p = problem(N, D, seed=N + D)
    c = weights(weighting, p["y"])
    st, abs_sums = R.newton_stats_host(p["x"], p["logprob"], p["shift"], p["scale"], p["w"], p["y"], c, L2, with_abs=True)
    return p, c, st, abs_sums, R.score_host(p["x"], p["logprob"], p["shift"], p["scale"], p["w"])


@lru_cache(maxsize=None)
def twin_hard(kind: str):
    from buglab.models import _triage as R

    p, c = hard_case(kind)
    st, abs_sums = R.newton_stats_host(p["x"], p["logprob"], p["shift"], p["scale"], p["w"], p["y"], c, L2, with_abs=True)
    return p, c, st, abs_sums, R.score_host(p["x"], p["logprob"], p["shift"], p["scale"], p["w"])


def summation_bound(N: int, abs_sum):
    """2 (N + 16) 2^-52 sum_i |t_i|: the any-order summation bound N u sum |t_i| (u = 2^-53) taken once for the device's order
    and once for the twin's, plus the few roundings inside a term; derived, not measured"""
    return 2.0 * (N + 16) * 2.0 ** -52 * np.asarray(abs_sum)


def ulps_apart(a, b) -> np.ndarray:
    """the distance of two float64 arrays in units in the last place (of the same sign, or both zero)"""
    ia, ib = np.asarray(a, np.float64).view(np.int64), np.asarray(b, np.float64).view(np.int64)
    return np.abs(ia - ib)


def learnable(N: int, D: int, seed: int, noise: float = 1.0):
    """rows whose label follows ONE linear direction of the embedding plus noise; the log-probability knows nothing"""
    rng = np.random.default_rng(seed)
    x, lp = drawn_rows(N, D, seed)
    direction = rng.normal(size=D)
    direction /= np.linalg.norm(direction)
    signal = ((x - x.mean(axis=0)) / x.std(axis=0)).astype(np.float64) @ direction
    return x, lp, signal + noise * rng.normal(size=N) > 0.0


def unlearnable(N: int, D: int, seed: int):
    rng = np.random.default_rng(seed)
    x, lp = drawn_rows(N, D, seed)
    return x, lp, rng.uniform(size=N) < 0.5
