"""Shared inputs of the drift-detection tests (tests/test_drift_host.py, tests/test_drift_gpu.py): the shapes at which the fused
kernel can go wrong, their fp64 reference (computed once per case and left unchanged), a NumPy fp32 restatement of the plain
materialising computation, and the error measure and p-value band of the GPU tests.

Shapes (n, m, D, R).  The kernel's tiles are 64 rows i (16 per wave), chunks of 32 rows j, groups of 16 mask rows (64, 128 or 256
per workgroup) and 64 columns of D:
  edge     (150, 107, 64, 199)  N = 257 is one past a row tile, R + 2 = 201 no multiple of a column tile
  exact    (64, 64, 40, 63)     exact row tiles and a padded D
  least    (2, 2, 32, 1)        the smallest case
  shifted  (300, 212, 128, 255) a 0.15 mean shift on the second sample: the test must reject at 1 / (R + 1)
  wide     (40, 37, 200, 31)    D padded to 256: the widest form that keeps the next chunk of rows j in registers
  widest   (33, 32, 512, 17)    the largest D: the form that stages a chunk in place, in more than 64 KB of LDS
Variants of the first three: `dup` two identical rows across the samples (distance exactly 0, and a rounded distance that may
come out negative), `far` one row at 1e3 times the scale (kernel values underflow to 0).

The seeds are chosen so that the fp64 p-value does not move when MMD2_0 moves by tau (test_drift_host.py checks it with the
NumPy fp32 restatement as the stand-in for the GPU yardstick): the band [p_lo, p_hi] is then at most 2 / (R + 1) wide.
"""
from __future__ import annotations

from functools import lru_cache
from typing import Dict, NamedTuple, Tuple

import numpy as np

from buglab.models import _drift as Dr

EPS = 2.0 ** -23
MARGIN = 4.0  # what tests/test_attn_stream_gpu.py allows a differently ordered fp32 accumulation


class Case(NamedTuple):
    n: int
    m: int
    D: int
    R: int
    seed: int            # of the subsets
    data_seed: int
    shift: float = 0.0   # added to every coordinate of the second sample
    variant: str = "plain"


SHAPES: Dict[str, Case] = {
    "edge": Case(150, 107, 64, 199, seed=3, data_seed=11),
    "exact": Case(64, 64, 40, 63, seed=5, data_seed=12),
    "least": Case(2, 2, 32, 1, seed=7, data_seed=13),
    "shifted": Case(300, 212, 128, 255, seed=9, data_seed=14, shift=0.15),
    "wide": Case(40, 37, 200, 31, seed=2, data_seed=15),
    "widest": Case(33, 32, 512, 17, seed=4, data_seed=16),
}
VARIANTS = ("plain", "dup", "far")
CASES: Dict[str, Case] = {**SHAPES, **{f"{name}-{v}": SHAPES[name]._replace(variant=v) for name in ("edge", "exact", "least")
                                        for v in VARIANTS[1:]}}


def rows(case: Case) -> Tuple[np.ndarray, np.ndarray]:
    """(x_ref [n, D], x_new [m, D]) fp32, drawn; the variant's rows planted"""
    rng = np.random.default_rng(case.data_seed)
    x = rng.standard_normal((case.n, case.D)).astype(np.float32)
    y = (rng.standard_normal((case.m, case.D)) + case.shift).astype(np.float32)
    if case.variant == "dup":
        y[case.m - 1] = x[0]  # one row of each sample: the same point
        x[1] = x[0]
    elif case.variant == "far":
        y[0] = (1e3 * y[0]).astype(np.float32)
    return x, y


class Reference(NamedTuple):
    z: np.ndarray        # float32 [N, D]
    s: float
    masks: np.ndarray    # uint8 [R + 1, N]
    A: np.ndarray        # fp64 from here on
    B: np.ndarray
    S: float
    u0: np.ndarray
    rho: np.ndarray
    mmd2: np.ndarray

    @property
    def unit(self) -> float:
        """S / N^2: the size of the terms that cancel in MMD2"""
        return self.S / float(self.z.shape[0]) ** 2


@lru_cache(maxsize=None)
def reference(name: str) -> Reference:
    case = CASES[name]
    x, y = rows(case)
    z = np.concatenate([x, y])
    s = Dr.bandwidth_host(z)
    masks = Dr.subsets_host(case.n + case.m, case.n, case.R, case.seed)
    A, B, S, u0, rho = Dr.permutation_sums_host(z, case.n, masks, s)
    out = Reference(z, s, masks, A, B, S, u0, rho, Dr.mmd2(A, B, S, case.n, case.m))
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def sums_fp32_numpy(z: np.ndarray, n: int, masks: np.ndarray, s: float):
    """The plain computation in fp32 NumPy: mm, exp, mm with K materialised -> (A, B, S, u0, rho) as fp64 arrays of fp32
    results.  The CPU stand-in for the GPU tests' torch yardstick."""
    z = np.asarray(z, np.float32)
    a = np.asarray(masks).astype(np.float32)
    sq = (z * z).sum(axis=1, dtype=np.float32)
    d2 = np.maximum(sq[:, None] + sq[None, :] - np.float32(2.0) * (z @ z.T), np.float32(0.0))
    K = np.exp(-d2 / np.float32(s)).astype(np.float32)
    U = K @ a.T
    A = (a.T * U).sum(axis=0, dtype=np.float32)
    B = U.sum(axis=0, dtype=np.float32)
    rho = K.sum(axis=1, dtype=np.float32)
    return A.astype(np.float64), B.astype(np.float64), float(rho.sum(dtype=np.float32)), U[:, 0].astype(np.float64), rho.astype(np.float64)


def err_mmd2(ref: Reference, A, B, S, n: int, m: int) -> float:
    """max_r |MMD2_r - MMD2_r^64| / (S^64 / N^2)"""
    return float(np.abs(Dr.mmd2(A, B, S, n, m) - ref.mmd2).max() / ref.unit)


def err_of(got, want) -> float:
    """the largest error of a vector of sums against its own magnitude"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / np.abs(want).max())


def bound(err_yardstick: float) -> float:
    return MARGIN * max(err_yardstick, EPS)


def p_band(ref: Reference, tau: float) -> Tuple[float, float]:
    """the fp64 p-values counted with >= MMD2_0 + tau and with >= MMD2_0 - tau"""
    null, R1 = ref.mmd2[1:], float(ref.mmd2.shape[0])
    return (1 + int((null >= ref.mmd2[0] + tau).sum())) / R1, (1 + int((null >= ref.mmd2[0] - tau).sum())) / R1
