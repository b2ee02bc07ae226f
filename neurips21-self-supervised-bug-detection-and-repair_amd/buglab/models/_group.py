"""The NumPy twin of the warning-grouping kernels (csrc/bl_group.hip), the host side of a grouping and the records behind
buglab/models/group.py.  BEYOND THE REFERENCE, which has no counterpart.

The groups are the connected components of "cosine of the centred site embeddings >= S" (single linkage at S).  The arithmetic,
stated once in include/buglab_hip.h ("Warning grouping") and repeated here, on `_similar.quantize_host`'s outputs c, q, sumsq, r:

  l1       l1_i = sum_d |q_id|, int32 and exact
  host     s2 = S S;  K = ((16 16129^2) s2) (1 - 2^-40), in double
  filter   idot = sum_d q_id q_jd (exact);  A = 4 idot + 2 (l1_i + l1_j) + D in int64;
           (i, j), i < j, both valid (r > 0), is a CANDIDATE iff A > 0 and ((double)A (double)A) (r_i r_j) >= K
  edge     dot = sum_d c_id c_jd in `_explain.node_scores_host`'s order (`_similar.rescore_host`'s dot);
           a candidate is an EDGE iff dot > 0.0 and dot dot >= s2 (sumsq_i sumsq_j)
  groups   label_i = the smallest row of i's component of the edge graph (an invalid row is alone); degree_i = edges at i;
           num_candidates, num_edges
Every output is a function of the input alone, whatever the order in which the pairs are visited: the device equals this bit
for bit for every launch geometry, the counters included.  The filter loses no edge (DESIGN.md has the derivation).
"""
from __future__ import annotations

from typing import Any, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from buglab.models._explain import node_scores_host
from buglab.models._similar import MAX_D, padded_dim

MAX_N = 1 << 19  # BL_GROUP_MAX_N
_RESCORE_CHUNK = 1 << 16  # candidate pairs per node_scores_host call (memory, not arithmetic)


def thresholds(similarity: float) -> Tuple[float, float]:
    """(s2, K) of a similarity S in (0, 1]; ValueError for any other value, NaN included."""
    S = float(similarity)
    if not 0.0 < S <= 1.0:
        raise ValueError(f"group: the similarity must be in (0, 1] (got {similarity})")
    s2 = S * S
    return s2, ((16.0 * 16129.0 * 16129.0) * s2) * (1.0 - 2.0 ** -40)


# ------------------------------------------------------------------------------------------------
# the twin
def row_l1_host(q) -> np.ndarray:
    """bl_group_row_l1 in NumPy: q int8 [N, Dp] -> int32 [N]."""
    q = np.asarray(q, np.int8)
    if q.ndim != 2 or q.shape[1] % 64 or not 64 <= q.shape[1] <= MAX_D:
        raise ValueError(f"row_l1_host: q {q.shape} must be [N, Dp], Dp a multiple of 64 up to {MAX_D}")
    return np.abs(q.astype(np.int32)).sum(axis=1, dtype=np.int32)


def labels_host(parent) -> np.ndarray:
    """bl_group_labels in NumPy: parent int32 [N] with parent[x] <= x -> every row's root, int32 [N].  An entry outside
    [0, row) ends the walk there."""
    parent = np.asarray(parent, np.int64).reshape(-1)
    rows = np.arange(parent.shape[0], dtype=np.int64)
    up = np.where((parent >= 0) & (parent < rows), parent, rows)  # roots, and garbage, point at themselves
    label = up.copy()
    while True:
        nxt = up[label]
        if np.array_equal(nxt, label):
            return label.astype(np.int32)
        label = nxt


def candidate_pairs(q, r, l1, D: int, K: float, i0: int, i1: int) -> Tuple[np.ndarray, np.ndarray]:
    """the filter on rows i0 .. i1 - 1 against every later row -> (i, j), i < j, in row-major order"""
    r = np.asarray(r, np.float64)
    # integer dot products through fp64 BLAS: every product and every partial sum is an integer below 2^53, so the result is exact
    idot = np.rint(np.asarray(q[i0:i1], np.float64) @ np.asarray(q[i0:], np.float64).T).astype(np.int64)
    A = 4 * idot + 2 * (l1[i0:i1, None].astype(np.int64) + l1[None, i0:].astype(np.int64)) + int(D)
    Af = A.astype(np.float64)  # exact: |A| < 2^26
    passes = (A > 0) & ((Af * Af) * (r[i0:i1, None] * r[None, i0:]) >= K)  # A^2 < 2^53: exact; two rounded products
    passes &= (r[i0:i1, None] > 0.0) & (r[None, i0:] > 0.0)
    passes &= np.arange(i0, i1)[:, None] < np.arange(i0, q.shape[0])[None, :]
    ii, jj = np.nonzero(passes)
    return ii + i0, jj + i0


def link_host(c, q, sumsq, r, l1, similarity: float, block: int = 256) -> Tuple[np.ndarray, np.ndarray, int, int]:
    """bl_group_link + bl_group_labels in NumPy -> (label int32 [N], degree int32 [N], num_candidates, num_edges)."""
    s2, K = thresholds(similarity)
    c, q = np.asarray(c, np.float32), np.asarray(q, np.int8)
    sumsq, r = np.asarray(sumsq, np.float64).reshape(-1), np.asarray(r, np.float64).reshape(-1)
    l1 = np.asarray(l1, np.int32).reshape(-1)
    if c.ndim != 2 or q.ndim != 2 or not 1 <= c.shape[1] <= MAX_D or q.shape != (c.shape[0], padded_dim(c.shape[1])):
        raise ValueError(f"link_host: c {c.shape} must be [N, 1 <= D <= {MAX_D}] and q {q.shape} [N, Dp]")
    N, D = c.shape
    if N > MAX_N or sumsq.shape != (N,) or r.shape != (N,) or l1.shape != (N,):
        raise ValueError(f"link_host: sumsq {sumsq.shape}, r {r.shape} and l1 {l1.shape} must be [N = {N} <= {MAX_N}]")
    root = np.arange(N, dtype=np.int64)  # fully compressed between blocks: every row's current root
    degree = np.zeros(N, np.int64)
    num_candidates = num_edges = 0
    for i0 in range(0, N, int(block)):
        ii, jj = candidate_pairs(q, r, l1, D, K, i0, min(i0 + int(block), N))
        num_candidates += int(ii.shape[0])
        for lo in range(0, ii.shape[0], _RESCORE_CHUNK):
            ci, cj = ii[lo:lo + _RESCORE_CHUNK], jj[lo:lo + _RESCORE_CHUNK]
            with np.errstate(invalid="ignore", over="ignore"):
                dot = node_scores_host(c[ci], c[cj])
                edge = (dot > 0.0) & (dot * dot >= s2 * (sumsq[ci] * sumsq[cj]))  # three rounded products, one compare
            ei, ej = ci[edge], cj[edge]
            num_edges += int(ei.shape[0])
            degree += np.bincount(ei, minlength=N) + np.bincount(ej, minlength=N)
            root = _union(root, ei, ej)
    return root.astype(np.int32), degree.astype(np.int32), num_candidates, num_edges


def _union(root: np.ndarray, ei: np.ndarray, ej: np.ndarray) -> np.ndarray:
    """a plain union-find on the edges' current roots, the smaller root winning; `root` comes in and goes out fully compressed"""
    a, b = root[ei], root[ej]
    apart = a != b
    if not apart.any():
        return root
    pairs = np.unique(np.stack([a[apart], b[apart]], axis=1), axis=0)
    up: Dict[int, int] = {}

    def find(x: int) -> int:
        while up.get(x, x) != x:
            x = up[x]
        return x

    for x, y in pairs.tolist():
        x, y = find(x), find(y)
        if x != y:
            up[max(x, y)] = min(x, y)
    if up:
        moved = np.fromiter(up.keys(), np.int64, len(up))
        target = np.asarray([find(x) for x in moved.tolist()], np.int64)
        table = np.arange(root.shape[0], dtype=np.int64)
        table[moved] = target
        root = table[root]
    return root


def group_rows_host(rows, mean, similarity: float) -> Tuple[np.ndarray, np.ndarray, int, int, np.ndarray, np.ndarray]:
    """The whole join in NumPy: rows [N, D] minus `mean` -> (label, degree, num_candidates, num_edges, c, sumsq)."""
    from buglab.models._similar import quantize_host

    c, q, sumsq, r = quantize_host(rows, mean)
    label, degree, nc, ne = link_host(c, q, sumsq, r, row_l1_host(q), similarity)
    return label, degree, nc, ne, c, sumsq


# ------------------------------------------------------------------------------------------------
# the host side of a grouping
class Members(NamedTuple):
    members: np.ndarray      # int64: the group's rows in input order
    representative: int      # the row a reviewer looks at
    size: int


def groups_from_labels(label, degree, logprob=None) -> List[Members]:
    """The groups of a labelling, on the host after the one copy back.  A group's representative is its member of the greatest
    degree, then of the greatest site log-probability, then of the lowest index; the groups come by size descending, then by
    representative ascending."""
    label, degree = np.asarray(label, np.int64).reshape(-1), np.asarray(degree, np.int64).reshape(-1)
    N = label.shape[0]
    logprob = np.zeros(N, np.float64) if logprob is None else np.asarray(logprob, np.float64).reshape(-1)
    if degree.shape != (N,) or logprob.shape != (N,):
        raise ValueError(f"groups_from_labels: degree {degree.shape} and logprob {logprob.shape} must be [{N}]")
    if N == 0:
        return []
    by_group = np.argsort(label, kind="stable")  # members in input order within a group
    starts = np.flatnonzero(np.r_[True, np.diff(label[by_group]) != 0])
    # within a group: greater degree, then greater log-probability, then lower index (lexsort: the last key decides first)
    best = np.lexsort((np.arange(N), -logprob, -degree, label))
    first_of = best[np.flatnonzero(np.r_[True, np.diff(label[best]) != 0])]
    out = [Members(by_group[a:b], int(rep), int(b - a)) for a, b, rep in zip(starts, np.r_[starts[1:], N], first_of)]
    out.sort(key=lambda g: (-g.size, g.representative))
    return out


class Grouping(NamedTuple):
    """What `group.group_embeddings` returns for N rows."""

    label: np.ndarray            # int32 [N]
    degree: np.ndarray           # int32 [N]
    num_candidates: int
    num_edges: int
    groups: List[Members]
    similarity: np.ndarray       # float64 [N]: the cosine of every row to its group's representative (0.0 for an invalid row)
    valid: np.ndarray            # bool [N]
    mean: np.ndarray             # float32 [D]: what was subtracted (zeros: not centred)


# ------------------------------------------------------------------------------------------------
# records
class WarningGroup(NamedTuple):
    id: int
    size: int
    representative: Dict[str, Any]   # position, node, label, filename, package, logprob
    members: List[Dict[str, Any]]    # in input order: position, node, label, filename, similarity (the cosine to the representative)
    scouts: List[str]                # the members' scouts ("" unless the sites are the true ones)
    resembles: Optional[Dict[str, Any]] = None  # with --index: the index entry nearest to the representative, and the cosine

    def record(self) -> Dict[str, Any]:
        out = {"id": self.id, "size": self.size, **self.representative, "members": self.members}
        if self.resembles is not None:
            out["resembles"] = self.resembles
        return out


class WarningGroups(NamedTuple):
    groups: List[WarningGroup]       # those of at least --min-group-size members
    summary: Dict[str, Any]          # `report`: of ALL groups


def report(sizes: Sequence[int], scouts_by_group: Sequence[Sequence[str]], similarity: float, num_samples: int, num_rejected: int,
           num_without_site: int, num_below_confidence: int, num_invalid: int, num_candidates: int, num_edges: int) -> Dict[str, Any]:
    """The run's numbers: counts, the groups' sizes, the join's counters, the share of warnings a reviewer is spared, and, where
    the sites carry scouts, the share of the groups (of two members or more) whose members share one scout."""
    sizes = np.asarray(list(sizes), np.int64)
    warnings = int(sizes.sum())
    out: Dict[str, Any] = {"similarity": float(similarity), "num_samples": int(num_samples), "num_rejected": int(num_rejected),
                           "num_without_site": int(num_without_site), "num_below_confidence": int(num_below_confidence),
                           "num_warnings": warnings, "num_invalid_embeddings": int(num_invalid), "num_groups": int(sizes.shape[0]),
                           "num_singletons": int((sizes == 1).sum()), "largest_group": int(sizes.max(initial=0)),
                           "num_candidates": int(num_candidates), "num_edges": int(num_edges),
                           "spared": 1.0 - sizes.shape[0] / warnings if warnings else 0.0}
    histogram: Dict[str, int] = {}
    for name, lo, hi in (("1", 1, 1), ("2", 2, 2), ("3-4", 3, 4), ("5-9", 5, 9), ("10-99", 10, 99), ("100-999", 100, 999),
                         ("1000+", 1000, None)):
        histogram[name] = int(((sizes >= lo) & ((sizes <= hi) if hi is not None else True)).sum())
    out["size_histogram"] = histogram
    labelled = [s for s in scouts_by_group if len(s) >= 2 and all(s)]
    if labelled:
        out["labelled"] = {"num_groups": len(labelled), "one_scout": sum(len(set(s)) == 1 for s in labelled) / len(labelled)}
    return out
