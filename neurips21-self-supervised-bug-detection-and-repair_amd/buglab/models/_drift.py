"""The NumPy twin of the drift-detection kernels (csrc/bl_drift.hip), the statistic's formulas and the report behind
buglab/models/drift.py.  BEYOND THE REFERENCE, which has no counterpart.

A two-sample permutation test of the kernel maximum mean discrepancy (MMD) between a reference sample of site embeddings and
the sites of the data about to be scanned.  The contract, stated once in include/buglab_hip.h, over the pooled rows
Z = [X_ref ; X_new] (fp32 [N, D], N = n + m, n, m >= 2):

  bandwidth  s = scale * 2 (mean_i |z_i|^2 - |mean_i z_i|^2) in fp64; 0 ("no spread") when the bracket is at most 2^-40 of
             mean_i |z_i|^2
  kernel     k(x, y) = exp(-max(|x - y|^2, 0) / s)
  subsets    a_0[i] = 1 iff i < n; for r = 1 .. R, a_r[i] = 1 iff fewer than n rows precede (key_i, i) in lexicographic order,
             key_i = mix(base + (r << 32) + i) in wrapping uint64 with `_compare`'s splitmix64 -- `subsets_host`, equal to the
             device bit for bit
  sums       U = K A;  A_r = a_r^T K a_r;  B_r = a_r^T K 1;  S = 1^T K 1  -- `permutation_sums_host`, in fp64: the reference
             the device's fp32-class sums are measured against
  statistic  MMD2_r = A_r / n^2 + (S - 2 B_r + A_r) / m^2 - 2 (B_r - A_r) / (n m): the biased V-statistic
  p-value    (1 + #{r >= 1 : MMD2_r >= MMD2_0}) / (R + 1)
  witness    f_i = U[i, 0] / n - (rho_i - U[i, 0]) / m for a scanned row i >= n, rho = K 1: the most negative are the samples
             least like the reference
"""
from __future__ import annotations

from typing import Any, Callable, Dict, List, NamedTuple, Optional, Tuple

import numpy as np

from buglab.models._compare import _GOLDEN, _mix

NO_SPREAD = 2.0 ** -40   # DR_NO_SPREAD
MAX_D = 512              # BL_DRIFT_MAX_D
MAX_PERMUTATIONS = 65533  # BL_DRIFT_MAX_PERMUTATIONS


# ------------------------------------------------------------------------------------------------
# the twin
def subset_keys(seed: int, r: int, N: int) -> np.ndarray:
    """The uint64 keys of rows 0 .. N - 1 in permutation r >= 1: they depend on (seed, r, i) alone."""
    with np.errstate(over="ignore"):
        base = _mix(np.asarray(np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF) * _GOLDEN + _GOLDEN))
        return _mix(base + (np.uint64(int(r)) << np.uint64(32)) + np.arange(int(N), dtype=np.uint64))


def subsets_host(N: int, n: int, R: int, seed: int, key_fn: Optional[Callable[[int, int, int], np.ndarray]] = None) -> np.ndarray:
    """bl_drift_subsets in NumPy -> uint8 [R + 1, N]: row r is a_r, the r-th column of the test's 0/1 matrix.  `key_fn(seed, r, N)`
    replaces the keys (for tests: a forced tie)."""
    N, n, R = int(N), int(n), int(R)
    if not (2 <= n <= N - 2) or R < 1:
        raise ValueError(f"subsets_host: need 2 <= n <= N - 2 and R >= 1 (got n {n}, N {N}, R {R})")
    keys_of = subset_keys if key_fn is None else key_fn
    out = np.zeros((R + 1, N), np.uint8)
    out[0, :n] = 1
    for r in range(1, R + 1):
        keys = np.asarray(keys_of(seed, r, N), np.uint64)
        out[r, np.argsort(keys, kind="stable")[:n]] = 1  # stable: equal keys keep their index order, the lower row first
    return out


def bandwidth_host(z, scale: float = 1.0) -> float:
    """bl_drift_bandwidth's s in NumPy (fp64), 0.0 when there is no spread."""
    z = np.asarray(z, np.float32).astype(np.float64)
    meansq = float((z * z).sum(axis=1).mean())
    mean = z.mean(axis=0)
    spread = meansq - float(mean @ mean)
    return float(scale) * 2.0 * spread if spread > meansq * NO_SPREAD else 0.0


def kernel_rows_host(z64: np.ndarray, norms: np.ndarray, lo: int, hi: int, s: float) -> np.ndarray:
    """rows lo .. hi - 1 of K in fp64"""
    if not s > 0.0:
        return np.ones((hi - lo, z64.shape[0]), np.float64)
    d2 = norms[lo:hi, None] + norms[None, :] - 2.0 * (z64[lo:hi] @ z64.T)
    return np.exp(-np.maximum(d2, 0.0) / s)


def permutation_sums_host(z, n: int, masks, s: float, block: int = 1024) -> Tuple[np.ndarray, np.ndarray, float, np.ndarray, np.ndarray]:
    """bl_drift_permutation_sums in fp64 -> (A [R + 1], B [R + 1], S, u0 [N] = U[:, 0], rho [N] = K 1).  masks: uint8 [R + 1, N]
    (`subsets_host`).  K is formed `block` rows at a time."""
    z64 = np.asarray(z, np.float32).astype(np.float64)
    a = np.asarray(masks).astype(np.float64)  # [R + 1, N]
    N = z64.shape[0]
    if a.ndim != 2 or a.shape[1] != N:
        raise ValueError(f"permutation_sums_host: masks {a.shape} must be [R + 1, {N}]")
    norms = (z64 * z64).sum(axis=1)
    A, B = np.zeros(a.shape[0]), np.zeros(a.shape[0])
    u0, rho = np.zeros(N), np.zeros(N)
    for lo in range(0, N, block):
        hi = min(lo + block, N)
        K = kernel_rows_host(z64, norms, lo, hi, s)
        U = K @ a.T                       # [rows, R + 1]
        A += (a[:, lo:hi].T * U).sum(axis=0)
        B += U.sum(axis=0)
        u0[lo:hi], rho[lo:hi] = U[:, 0], K.sum(axis=1)
    return A, B, float(rho.sum()), u0, rho


def mmd2(A, B, S, n: int, m: int) -> np.ndarray:
    """MMD2_r from (A_r, B_r, S), in fp64."""
    A, B, S, n, m = np.asarray(A, np.float64), np.asarray(B, np.float64), float(S), float(n), float(m)
    return A / (n * n) + (S - 2.0 * B + A) / (m * m) - 2.0 * (B - A) / (n * m)


def p_value(stats) -> float:
    """(1 + #{r >= 1 : MMD2_r >= MMD2_0}) / (R + 1)"""
    stats = np.asarray(stats, np.float64)
    return float(1 + int((stats[1:] >= stats[0]).sum())) / float(stats.shape[0])


def witness(u0, rho, n: int, m: int) -> np.ndarray:
    """f_i of the scanned rows i >= n, float64 [m]"""
    u0, rho = np.asarray(u0, np.float64), np.asarray(rho, np.float64)
    return u0[n:] / float(n) - (rho[n:] - u0[n:]) / float(m)


def outliers(f, k: int) -> np.ndarray:
    """the k scanned rows with the most negative witness, most negative first, the lower row among equals"""
    f = np.asarray(f, np.float64)
    return np.argsort(f, kind="stable")[:max(int(k), 0)].astype(np.int64)


# ------------------------------------------------------------------------------------------------
# the report
class DriftReport(NamedTuple):
    n: int                      # reference rows
    m: int                      # scanned rows
    dim: int
    bandwidth: float            # s; 0.0: no spread
    statistic: float            # MMD2_0
    p_value: float
    alpha: float
    drift: bool                 # p_value <= alpha
    num_permutations: int
    seed: int
    null_mean: float            # of MMD2_1 .. MMD2_R
    null_q95: float
    outliers: List[Dict[str, Any]]  # position among the scanned rows and witness value, most negative first
    null: np.ndarray            # MMD2_1 .. MMD2_R (not in the record)
    witness: np.ndarray         # f of every scanned row (not in the record)
    num_samples: int = 0
    num_rejected: int = 0
    num_without_site: int = 0

    def record(self) -> Dict[str, Any]:
        return {"n": self.n, "m": self.m, "dim": self.dim, "bandwidth": self.bandwidth, "no_spread": not self.bandwidth > 0.0,
                "mmd2": self.statistic, "p_value": self.p_value, "alpha": self.alpha, "drift": self.drift,
                "num_permutations": self.num_permutations, "seed": self.seed, "null_mean": self.null_mean, "null_q95": self.null_q95,
                "num_samples": self.num_samples, "num_rejected": self.num_rejected, "num_without_site": self.num_without_site,
                "outliers": self.outliers}


def make_report(n: int, m: int, dim: int, s: float, A, B, S, u0, rho, alpha: float, seed: int, top_k: int) -> DriftReport:
    """The report from the sums, whoever computed them (fp64 on the host from here on)."""
    R = int(np.asarray(A).shape[0]) - 1
    if s > 0.0:
        stats, f = mmd2(A, B, S, n, m), witness(u0, rho, n, m)
        p = p_value(stats)
    else:  # no spread: every row is the same point
        stats, f, p = np.zeros(R + 1), np.zeros(m), 1.0
    top = outliers(f, top_k)
    return DriftReport(int(n), int(m), int(dim), float(s), float(stats[0]), p, float(alpha), bool(p <= alpha), R, int(seed),
                       float(stats[1:].mean()), float(np.quantile(stats[1:], 0.95)),
                       [{"position": int(i), "witness": float(f[i])} for i in top], stats[1:].copy(), f)


def drift_host(x_ref, x_new, num_permutations: int = 1000, seed: int = 0, alpha: float = 0.05, bandwidth_scale: float = 1.0,
               top_k: int = 20) -> DriftReport:
    """The whole test in NumPy on embeddings that already exist (both centred alike)."""
    x_ref, x_new = np.asarray(x_ref, np.float32), np.asarray(x_new, np.float32)
    check_samples(x_ref.shape, x_new.shape, num_permutations)
    z = np.concatenate([x_ref, x_new])
    n, m = x_ref.shape[0], x_new.shape[0]
    s = bandwidth_host(z, bandwidth_scale)
    masks = subsets_host(n + m, n, num_permutations, seed)
    A, B, S, u0, rho = permutation_sums_host(z, n, masks, s)
    return make_report(n, m, z.shape[1], s, A, B, S, u0, rho, alpha, seed, top_k)


def check_samples(ref_shape, new_shape, num_permutations: int) -> None:
    if len(ref_shape) != 2 or len(new_shape) != 2 or ref_shape[1] != new_shape[1]:
        raise ValueError(f"drift: the samples {tuple(ref_shape)} and {tuple(new_shape)} must be [n, D] and [m, D]")
    if ref_shape[0] < 2 or new_shape[0] < 2:
        raise ValueError(f"drift: both samples need at least 2 rows (got {ref_shape[0]} and {new_shape[0]})")
    if not 1 <= ref_shape[1] <= MAX_D or not 1 <= int(num_permutations) <= MAX_PERMUTATIONS:
        raise ValueError(f"drift: need 1 <= D <= {MAX_D} and 1 <= permutations <= {MAX_PERMUTATIONS} (got D {ref_shape[1]}, "
                         f"{num_permutations} permutations)")
