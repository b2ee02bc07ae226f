"""The NumPy twin of the similar-bug search kernels (csrc/bl_similar.hip), the records and the index file format behind
buglab/models/similar.py.  BEYOND THE REFERENCE, which has no counterpart.

A SITE is one candidate location of one sample; its embedding is the row of the head input `h` behind that candidate.  The
arithmetic, stated once in include/buglab_hip.h and repeated by every function here, equal to the kernels bit for bit
(Dp = D rounded up to a multiple of 64):

  centre    c_d = (float)((double)x_d - (double)mean_d)
  row       amax = max |c_d|; sumsq = sum c_d c_d in fp64 in `_explain.node_scores_host`'s order; INVALID if a c_d is not finite
            or amax == 0: q = 0, sumsq = 0, r = 0, never a candidate, no neighbours as a query
  quantise  q_d = (int8)rint((double)c_d * (127.0 / (double)amax)); r = (amax amax) / sumsq
  key       idot = sum qx_d qy_d (exact); key = (double)(idot |idot|) * r_y, the product idot |idot| formed in int64
  search    the first C valid index rows by (greater key, lower index), -1 padded
  re-score  dot = sum cx_d cy_d as sumsq; key2 = (dot |dot|) / sumsq_y; the first k by (greater key2, lower index, earlier place)
  cosine    dot / sqrt(sumsq_x sumsq_y), clipped to [-1, 1], on the host
"""
from __future__ import annotations

import hashlib
from typing import Any, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from buglab.models._explain import node_scores_host

MAX_D = 512          # BL_SIM_MAX_D
MAX_CANDIDATES = 16  # BL_SIM_MAX_CANDIDATES
SITE_MODES = ("predicted", "truth")
FORMAT_VERSION = 1


def padded_dim(D: int) -> int:
    return (int(D) + 63) // 64 * 64


# ------------------------------------------------------------------------------------------------
# the twin
def embed_sites_host(flat, loc_idx, loc_off, cand_rows, h, mode: str = "predicted", truth=None, skip_nobug: bool = False
                     ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """bl_sim_embed_sites in NumPy -> (rows float32 [B, D], place int32 [B], logprob float32 [B])."""
    if mode not in SITE_MODES:
        raise ValueError(f"embed_sites_host: mode must be one of {SITE_MODES} (got {mode!r})")
    flat, h = np.asarray(flat, np.float32).reshape(-1), np.asarray(h, np.float32)
    loc_idx, cand_rows = np.asarray(loc_idx, np.int64).reshape(-1), np.asarray(cand_rows, np.int64).reshape(-1)
    off = np.clip(np.asarray(loc_off, np.int64).reshape(-1), 0, loc_idx.shape[0])
    B, D = off.shape[0] - 1, h.shape[1]
    rows, place, logprob = np.zeros((B, D), np.float32), np.full(B, -1, np.int32), np.zeros(B, np.float32)
    for b in range(B):
        lo, n = int(off[b]), max(int(off[b + 1]) - int(off[b]), 0)
        if mode == "truth":
            p = int(truth[b])
        else:
            p, best = -1, 0.0
            for j in range(n - 1 if skip_nobug else n):
                f = int(loc_idx[lo + j])
                v = float(flat[f]) if 0 <= f < flat.shape[0] else float("nan")
                if v != v:
                    continue
                if p < 0 or v > best:  # ascending j: the first maximum stays
                    p, best = j, v
        if not 0 <= p < n - 1:
            continue
        f = int(loc_idx[lo + p])
        if not (0 <= f < cand_rows.shape[0] and f < flat.shape[0]):
            continue
        row = int(cand_rows[f])
        if not 0 <= row < h.shape[0]:
            continue
        rows[b], place[b], logprob[b] = h[row], p, flat[f]
    return rows, place, logprob


def quantize_host(x, mean) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """bl_sim_quantize in NumPy -> (c float32 [N, D], q int8 [N, Dp], sumsq float64 [N], r float64 [N])."""
    x, mean = np.asarray(x, np.float32), np.asarray(mean, np.float32).reshape(-1)
    if x.ndim != 2 or not 1 <= x.shape[1] <= MAX_D or mean.shape[0] != x.shape[1]:
        raise ValueError(f"quantize_host: x {x.shape} must be [N, 1 <= D <= {MAX_D}] and mean {mean.shape} [D]")
    N, D = x.shape
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        c = (x.astype(np.float64) - mean.astype(np.float64)[None, :]).astype(np.float32)
        a = np.abs(c)
        finite = np.isfinite(c).all(axis=1)
        amax = np.where(finite, np.where(np.isnan(a), 0.0, a).max(axis=1, initial=0.0), 0.0).astype(np.float32)
        valid = finite & (amax > 0)
        q = np.zeros((N, padded_dim(D)), np.int8)
        sumsq, r = np.zeros(N, np.float64), np.zeros(N, np.float64)
        if valid.any():
            cv, am = c[valid], amax[valid].astype(np.float64)
            s = node_scores_host(cv, cv)
            q[valid, :D] = np.rint(cv.astype(np.float64) * (127.0 / am)[:, None]).astype(np.int8)  # half to even
            sumsq[valid], r[valid] = s, (am * am) / s
    return c, q, sumsq, r


def coarse_keys(qx, qy, ry) -> np.ndarray:
    """key [Q, N] float64 of every (query, index row) pair; an invalid index row's column is meaningless"""
    # integer dot products through fp64 BLAS: every product and every partial sum is an integer below 2^53, so the result is exact
    idot = np.rint(np.asarray(qx, np.float64) @ np.asarray(qy, np.float64).T).astype(np.int64)
    return (idot * np.abs(idot)).astype(np.float64) * np.asarray(ry, np.float64)[None, :]  # int64 product (up to 7e13), one rounded product


def search_host(qx, rx, qy, ry, candidates: int = MAX_CANDIDATES, block: int = 256) -> Tuple[np.ndarray, np.ndarray]:
    """bl_sim_search_i8 in NumPy -> (index int32 [Q, C], -1 padded; key float64 [Q, C], 0.0 padded)."""
    C = int(candidates)
    if not 1 <= C <= MAX_CANDIDATES:
        raise ValueError(f"search_host: candidates must be in [1, {MAX_CANDIDATES}] (got {candidates})")
    qx, qy = np.asarray(qx, np.int8), np.asarray(qy, np.int8)
    rx, ry = np.asarray(rx, np.float64).reshape(-1), np.asarray(ry, np.float64).reshape(-1)
    Q = qx.shape[0]
    live = np.flatnonzero(ry > 0.0)  # ascending: a stable sort keeps the lower index first among equal keys
    out_idx, out_key = np.full((Q, C), -1, np.int32), np.zeros((Q, C), np.float64)
    if live.shape[0] == 0:
        return out_idx, out_key
    qy_live, ry_live = qy[live], ry[live]
    for q0 in range(0, Q, block):
        key = coarse_keys(qx[q0:q0 + block], qy_live, ry_live)
        order = np.argsort(-key, axis=1, kind="stable")[:, :C]
        n = order.shape[1]
        for i in range(key.shape[0]):
            if rx[q0 + i] > 0.0:
                out_idx[q0 + i, :n], out_key[q0 + i, :n] = live[order[i]], key[i, order[i]]
    return out_idx, out_key


def rescore_host(cx, cy, sumsq_y, cand, k: int) -> Tuple[np.ndarray, np.ndarray]:
    """bl_sim_rescore in NumPy -> (index int32 [Q, k], -1 padded; dot float64 [Q, k], 0.0 padded)."""
    cx, cy = np.asarray(cx, np.float32), np.asarray(cy, np.float32)
    sumsq_y, cand = np.asarray(sumsq_y, np.float64).reshape(-1), np.asarray(cand, np.int64)
    Q, C = cand.shape
    k = int(k)
    if not 1 <= C <= MAX_CANDIDATES or not 1 <= k <= C:
        raise ValueError(f"rescore_host: need 1 <= k <= C <= {MAX_CANDIDATES} (got k {k}, C {C})")
    N = cy.shape[0]
    out_idx, out_dot = np.full((Q, k), -1, np.int32), np.zeros((Q, k), np.float64)
    present = (cand >= 0) & (cand < N)
    present[present] = sumsq_y[cand[present]] > 0.0
    qi, ci = np.nonzero(present)
    if qi.shape[0] == 0:
        return out_idx, out_dot
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        rows = cand[qi, ci]
        dot = node_scores_host(cx[qi], cy[rows])
        key2 = (dot * np.abs(dot)) / sumsq_y[rows]  # one rounded product, one rounded quotient
    keep = ~np.isnan(key2)
    qi, rows, dot, key2 = qi[keep], rows[keep], dot[keep], key2[keep]  # (still by query, then by place in the list)
    order = np.lexsort((rows, -key2, qi))  # stable: the place decides last
    qi, rows, dot = qi[order], rows[order], dot[order]
    start = np.searchsorted(qi, np.arange(Q))
    rank = np.arange(qi.shape[0]) - start[qi]
    top = rank < k
    out_idx[qi[top], rank[top]], out_dot[qi[top], rank[top]] = rows[top], dot[top]
    return out_idx, out_dot


def similarity(dot, sumsq_x, sumsq_y) -> np.ndarray:
    """The cosine of a neighbour: dot / sqrt(sumsq_x sumsq_y), clipped to [-1, 1]; 0 where there is no neighbour (a sum 0)."""
    dot, prod = np.asarray(dot, np.float64), np.asarray(sumsq_x, np.float64) * np.asarray(sumsq_y, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(prod > 0.0, np.clip(dot / np.sqrt(prod), -1.0, 1.0), 0.0)


def find_neighbours_host(x, mean, index_c, k: int, candidates: int):
    """The whole search in NumPy: queries x [Q, D] against the centred index rows -> (idx [Q, k], dot [Q, k], sumsq_x [Q],
    sumsq_y [N])."""
    cx, qx, sx, rx = quantize_host(x, mean)
    cy, qy, sy, ry = quantize_host(index_c, np.zeros(index_c.shape[1], np.float32))
    cand, _ = search_host(qx, rx, qy, ry, candidates)
    idx, dot = rescore_host(cx, cy, sy, cand, k)
    return idx, dot, sx, sy


# ------------------------------------------------------------------------------------------------
# records
class SiteEmbeddings(NamedTuple):
    """The sites of a run, one entry per sample WITH a site, in input order."""

    rows: np.ndarray         # float32 [n, D]
    positions: np.ndarray    # int64 [n]: input positions
    nodes: np.ndarray        # int32 [n]: the site's node in its datapoint's graph
    logprobs: np.ndarray     # float32 [n]: the site's location log-probability
    labels: List[str]        # graph.nodes[node]
    paths: List[str]
    packages: List[str]
    scouts: List[str]        # the scout of the true rewrite; "" when the site is predicted or the sample carries no bug
    num_samples: int         # samples read
    num_rejected: int        # of them, refused by `tensorize`
    num_without_site: int    # of the accepted ones, without a site


def site_metadata(point: Dict[str, Any], place: int) -> Tuple[int, str, str, str]:
    """(node, label, path, package) of the site at `place` of the datapoint's location entries (np.unique(reference_nodes))"""
    graph = point["graph"]
    node = int(np.unique(np.asarray(graph["reference_nodes"], dtype=np.int64))[int(place)])
    return node, str(graph["nodes"][node]), str(graph.get("path", "")), str(point.get("package_name", ""))


def truth_place(point: Dict[str, Any]) -> int:
    """the place of the true bug's location among the sample's location entries, -1: no bug or no label"""
    target = point.get("target_fix_action_idx")
    if target is None:
        return -1
    _, inverse = np.unique(np.asarray(point["graph"]["reference_nodes"], dtype=np.int64), return_inverse=True)
    return int(inverse[int(target)])


def true_scout(point: Dict[str, Any]) -> str:
    target = point.get("target_fix_action_idx")
    return "" if target is None else str(point["candidate_rewrite_metadata"][int(target)][0])


def model_fingerprint(nn) -> str:
    """SHA-1 over the names and the bytes of the module's `state_dict`, in its order."""
    sha = hashlib.sha1()
    for name, value in nn.state_dict().items():
        sha.update(name.encode("utf-8"))
        sha.update(value.detach().cpu().contiguous().numpy().tobytes())
    return sha.hexdigest()


class DimensionMismatch(ValueError):
    """The index was built from embeddings of another size than the model's."""


class SiteIndex(NamedTuple):
    embeddings: np.ndarray   # float32 [N, D], centred
    mean: np.ndarray         # float32 [D]: what was subtracted (zeros: not centred)
    positions: np.ndarray    # int64 [N]
    nodes: np.ndarray        # int32 [N]
    labels: np.ndarray       # str [N]
    paths: np.ndarray        # str [N]
    packages: np.ndarray     # str [N]
    scouts: np.ndarray       # str [N]
    tags: np.ndarray         # str [N]
    model_class: str
    dim: int
    fingerprint: str

    @property
    def size(self) -> int:
        return int(self.embeddings.shape[0])

    def entry(self, i: int) -> Dict[str, Any]:
        i = int(i)
        return {"entry": i, "position": int(self.positions[i]), "node": int(self.nodes[i]), "label": str(self.labels[i]),
                "filename": str(self.paths[i]), "package": str(self.packages[i]), "scout": str(self.scouts[i]), "tag": str(self.tags[i])}

    def save(self, path) -> None:
        with open(path, "wb") as f:  # a file object: np.savez appends no suffix
            np.savez(f, format_version=np.int64(FORMAT_VERSION), embeddings=self.embeddings, mean=self.mean, positions=self.positions,
                     nodes=self.nodes, labels=_text(self.labels), paths=_text(self.paths), packages=_text(self.packages),
                     scouts=_text(self.scouts), tags=_text(self.tags), model_class=np.str_(self.model_class), dim=np.int64(self.dim),
                     fingerprint=np.str_(self.fingerprint))

    @classmethod
    def load(cls, path) -> "SiteIndex":
        with np.load(path, allow_pickle=False) as z:
            if int(z["format_version"]) != FORMAT_VERSION:
                raise ValueError(f"{path}: index format {int(z['format_version'])}; this version reads {FORMAT_VERSION}")
            index = cls(z["embeddings"], z["mean"], z["positions"], z["nodes"], z["labels"], z["paths"], z["packages"], z["scouts"],
                        z["tags"], str(z["model_class"]), int(z["dim"]), str(z["fingerprint"]))
        N, D = index.embeddings.shape
        if index.embeddings.dtype != np.float32 or index.mean.dtype != np.float32 or index.mean.shape != (D,) or D != index.dim \
                or any(a.shape != (N,) for a in index[2:9]):
            raise ValueError(f"{path}: inconsistent index arrays")
        return index

    def check_model(self, model_class: str, dim: int, fingerprint: str) -> Optional[str]:
        """DimensionMismatch for embeddings of another size; otherwise a warning text when the index was built with another
        model (class or weights), None when it is this one."""
        if int(dim) != self.dim:
            raise DimensionMismatch(f"the index holds embeddings of size {self.dim} (built with {self.model_class}); the model's are of "
                                    f"size {int(dim)}")
        if fingerprint != self.fingerprint or model_class != self.model_class:
            return (f"the index was built with other weights ({self.model_class} {self.fingerprint[:12]}) than the model's "
                    f"({model_class} {fingerprint[:12]}): similarities compare embeddings of two models")
        return None


def _text(values) -> np.ndarray:
    return np.asarray(list(values), dtype=np.str_) if len(values) else np.zeros(0, dtype="<U1")


def column_mean(rows: np.ndarray) -> np.ndarray:
    """The fp32 mean of the finite rows, summed in fp64 on the host (zeros when there is none)."""
    rows = np.asarray(rows, np.float32)
    finite = np.isfinite(rows).all(axis=1)
    if not finite.any():
        return np.zeros(rows.shape[1], np.float32)
    return rows[finite].astype(np.float64).mean(axis=0).astype(np.float32)


def centre(rows: np.ndarray, mean: np.ndarray) -> np.ndarray:
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(rows, np.float32).astype(np.float64) - np.asarray(mean, np.float32).astype(np.float64)[None, :]).astype(np.float32)


def make_index(sites: SiteEmbeddings, tag: Optional[str], center: bool, model_class: str, fingerprint: str) -> SiteIndex:
    D = int(sites.rows.shape[1])
    mean = column_mean(sites.rows) if center else np.zeros(D, np.float32)
    n = sites.rows.shape[0]
    return SiteIndex(centre(sites.rows, mean), mean, np.asarray(sites.positions, np.int64), np.asarray(sites.nodes, np.int32),
                     _text(sites.labels), _text(sites.paths), _text(sites.packages), _text(sites.scouts), _text([tag or ""] * n),
                     str(model_class), D, str(fingerprint))


class Neighbours(NamedTuple):
    """What `find_similar` yields per sample with a site."""

    position: int
    node: int
    label: str
    logprob: float
    scout: str                     # of the query's true rewrite, "" when unlabelled or clean
    valid: bool                    # False: the embedding was invalid (not finite, or zero after centring): no neighbours
    neighbours: List[Dict[str, Any]]  # in order: the index entry's metadata and "similarity"

    def record(self) -> Dict[str, Any]:
        return {"position": self.position, "node": self.node, "label": self.label, "logprob": self.logprob, "neighbours": self.neighbours}


def neighbour_list(index: SiteIndex, idx: np.ndarray, sim: np.ndarray, min_similarity: Optional[float]) -> List[Dict[str, Any]]:
    out = []
    for i, s in zip(idx, sim):
        if i < 0 or (min_similarity is not None and not s >= min_similarity):
            continue
        out.append(dict(index.entry(i), similarity=float(s)))
    return out


def report(found: Sequence[Neighbours], num_samples: int, num_rejected: int, num_without_site: int) -> Dict[str, Any]:
    """The run's numbers: counts, the distribution of the top-1 similarity, and, where the queries are labelled, the share of
    them whose nearest neighbour carries the scout of the query's true rewrite."""
    top1 = np.asarray([f.neighbours[0]["similarity"] for f in found if f.neighbours], np.float64)
    out: Dict[str, Any] = {"num_samples": int(num_samples), "num_with_site": len(found), "num_rejected": int(num_rejected),
                           "num_without_site": int(num_without_site), "num_invalid_embeddings": sum(not f.valid for f in found),
                           "num_with_neighbours": int(top1.shape[0])}
    if top1.shape[0]:
        qs = np.quantile(top1, [0.0, 0.1, 0.25, 0.5, 0.75, 0.9, 1.0])
        out["top1_similarity"] = {"mean": float(top1.mean()), **{name: float(v) for name, v in zip(("min", "p10", "p25", "median", "p75", "p90", "max"), qs)}}
    labelled = [f for f in found if f.scout and f.neighbours]
    if labelled:
        out["labelled"] = {"num_queries": len(labelled),
                           "top1_same_scout": sum(f.neighbours[0]["scout"] == f.scout for f in labelled) / len(labelled)}
    return out
