"""The index arrays, the differentiable forward and the NumPy twin of the attribution kernels (csrc/bl_explain.hip) behind
buglab/models/explain.py and `visualize.py --explain`.

An ATTRIBUTION of node n is a_n = sum_d G[n, d] * x[n, d]: x [N, D] the node embedder's output (eval mode, no dropout), G the
gradient of the explained log-probability with respect to it -- gradient x input; with M > 1 steps the mean of that over the
gradients at alpha_m * x, alpha_m = (m - 1/2) / M: integrated gradients from the all-zero baseline by the midpoint rule.
`input_gradients` is the one place the differentiable forward and `torch.autograd.grad` live; `hip_ops.attribute_node_scores` /
`attribute_topk` reduce and select on the device; `node_scores_host` / `topk_host` do the same arithmetic in NumPy, in the
same order, and are equal to the kernels bit for bit.

COLUMN OWNERSHIP of the dot product (include/buglab_hip.h::bl_attr_node_scores): columns go in quads, quad q = columns 4q ..
4q + 3; lane l of 64 owns the quads with q % 64 == l and adds its columns' products (exact in fp64) to its own sum, which
starts at +0.0, in ascending column order; the 64 lane sums go through the xor butterfly, strides 32 .. 1."""
from __future__ import annotations

from contextlib import contextmanager
from typing import Any, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

MAX_K = 32  # BL_EXPLAIN_MAX_K
WAVE = 64
THREADS = 256  # of bl_attr_topk's workgroup


class ExplainIndices(NamedTuple):
    """int32 arrays of one predict minibatch of B graphs."""

    node_off: np.ndarray    # [B + 1]  graph b owns the nodes node_off[b] : node_off[b + 1] of the minibatch
    rw_idx: np.ndarray      # [total_rw]  flat index of every rewrite, by original rewrite index (as SuggestIndices)
    rw_loc_idx: np.ndarray  # [total_rw]  flat index of the location entry of the rewrite's reference node, -1: no key
    rw_off: np.ndarray      # [B + 1]
    nobug_idx: np.ndarray   # [B]  flat index of NO_BUG's location entry


def explain_indices(num_nodes_per_graph, num_nodes: int, suggest_ix, datapoints: Optional[Sequence[Any]] = None,
                    node_to_graph=None) -> ExplainIndices:
    """`num_nodes_per_graph` [B] and `num_nodes` of the collated minibatch, `suggest_ix` the minibatch's `SuggestIndices`.
    Asserts what the node indices of a record rest on: the collator keeps graphs contiguous and in node order (node_to_graph ==
    repeat(arange(B), n_per_graph); compared where the caller has `node_to_graph` on the host, else through the node count), and a
    graph has as many nodes as its datapoint lists (after add_open_vocab_nodes_and_edges, which `tensorize` has run)."""
    n_per_graph = np.asarray(num_nodes_per_graph, dtype=np.int64).reshape(-1)
    B = n_per_graph.shape[0]
    assert (n_per_graph >= 0).all() and int(n_per_graph.sum()) == int(num_nodes), "the graphs' node counts do not add up to the minibatch's"
    if node_to_graph is not None:
        assert np.array_equal(np.asarray(node_to_graph, dtype=np.int64).reshape(-1), np.repeat(np.arange(B, dtype=np.int64), n_per_graph)), \
            "the collator no longer keeps a minibatch's graphs contiguous and in node order"
    assert suggest_ix.rw_off.shape[0] == B + 1 and suggest_ix.nobug_idx.shape[0] == B
    if datapoints is not None:
        assert len(datapoints) == B and all(len(p["graph"]["nodes"]) == int(n) for p, n in zip(datapoints, n_per_graph))
    node_off = np.zeros(B + 1, dtype=np.int64)
    np.cumsum(n_per_graph, out=node_off[1:])
    assert node_off[-1] < 2 ** 31
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    return ExplainIndices(i32(node_off), i32(suggest_ix.rw_idx), i32(suggest_ix.rw_loc_idx), i32(suggest_ix.rw_off),
                          i32(suggest_ix.nobug_idx))


def chosen_flat_indices(entry: np.ndarray, ix: ExplainIndices) -> np.ndarray:
    """The sources of the explained entries in the flat output, int32 [B, 2], -1 = absent: a rewrite e of sample b reads
    (rw_loc_idx, rw_idx)[rw_off[b] + e], NO_BUG (e == the sample's rewrite count) reads nobug_idx[b], no entry (e < 0) nothing.
    The driver does the same with device ops."""
    entry = np.asarray(entry, dtype=np.int64).reshape(-1)
    B = entry.shape[0]
    n_rw = np.diff(ix.rw_off.astype(np.int64))
    out = np.full((B, 2), -1, dtype=np.int32)
    for b in range(B):
        e = int(entry[b])
        if e < 0:
            continue
        if e >= n_rw[b]:
            out[b, 0] = ix.nobug_idx[b]
        else:
            out[b] = (ix.rw_loc_idx[int(ix.rw_off[b]) + e], ix.rw_idx[int(ix.rw_off[b]) + e])
    return out


# ------------------------------------------------------------------------------------------------
# the twin
def _butterfly(v: np.ndarray) -> np.ndarray:
    """bl_wave_sum_f64 over the last axis (64 lanes): every lane's value after the xor butterfly, strides 32 .. 1"""
    lanes = np.arange(WAVE)
    o = WAVE // 2
    while o > 0:
        v = v + v[..., lanes ^ o]
        o //= 2
    return v


def node_scores_host(x, g, score=None, weight: float = 1.0) -> np.ndarray:
    """bl_attr_node_scores in NumPy: float64 [N] = weight * dot_n, added to `score` when one is given (a new array either way)."""
    x, g = np.asarray(x, dtype=np.float32), np.asarray(g, dtype=np.float32)
    if x.ndim != 2 or x.shape != g.shape or x.shape[1] < 1:
        raise ValueError(f"node_scores_host: x {x.shape} and g {g.shape} must both be [N, D >= 1]")
    N, D = x.shape
    quads = (D + 3) // 4
    passes = (quads + WAVE - 1) // WAVE
    with np.errstate(invalid="ignore", over="ignore"):
        prod = np.zeros((N, passes * WAVE * 4), dtype=np.float64)  # (a column that does not exist adds +0.0 to a sum that is never -0.0)
        prod[:, :D] = x.astype(np.float64) * g.astype(np.float64)  # exact
        prod = prod.reshape(N, passes, WAVE, 4)
        lane = np.zeros((N, WAVE), dtype=np.float64)
        for p in range(passes):  # a lane's columns in ascending order: its quads by pass, a quad's columns 0 .. 3
            for j in range(4):
                lane = lane + prod[:, p, :, j]
        t = np.float64(weight) * _butterfly(lane)[:, 0]
        if score is None:
            return t
        score = np.asarray(score, dtype=np.float64)
        if score.shape != (N,):
            raise ValueError(f"node_scores_host: score {score.shape} must be [{N}]")
        return score + t


def _block_sum(values: np.ndarray) -> float:
    """one value per node of a graph -> the sum as bl_attr_topk forms it: thread t of 256 adds nodes t, t + 256, .. in that order,
    the butterfly in each of the 4 waves, the waves' sums in wave order"""
    n = values.shape[0]
    rows = (n + THREADS - 1) // THREADS
    padded = np.zeros(rows * THREADS, dtype=np.float64)
    padded[:n] = values
    acc = np.zeros(THREADS, dtype=np.float64)
    for row in padded.reshape(rows, THREADS):
        acc = acc + row
    waves = _butterfly(acc.reshape(THREADS // WAVE, WAVE))[:, 0]
    total = waves[0]
    for w in waves[1:]:
        total = total + w
    return total


def topk_host(score, node_off, k: int, by_abs: bool = True) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """bl_attr_topk in NumPy -> (node int32 [B, k], -1 padded: indices within the graph; score float64 [B, k], 0.0 padded; sums
    float64 [2, B] = sum a | sum |a|).  Offsets are clamped into [0, N] as on the device."""
    if not 1 <= int(k) <= MAX_K:
        raise ValueError(f"topk_host: k must be in [1, {MAX_K}] (got {k})")
    k = int(k)
    score = np.asarray(score, dtype=np.float64).reshape(-1)
    off = np.clip(np.asarray(node_off, dtype=np.int64).reshape(-1), 0, score.shape[0])
    B = off.shape[0] - 1
    node, picked, sums = np.full((B, k), -1, np.int32), np.zeros((B, k), np.float64), np.zeros((2, B), np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            a = score[off[b]:max(off[b + 1], off[b])]
            sums[0, b], sums[1, b] = _block_sum(a), _block_sum(np.abs(a))
            key = np.abs(a) if by_abs else a
            at = np.flatnonzero(~np.isnan(key))
            at = at[np.argsort(-key[at], kind="stable")][:k]  # stable: the lower index first among equals
            node[b, :at.shape[0]], picked[b, :at.shape[0]] = at, a[at]
    return node, picked, sums


# ------------------------------------------------------------------------------------------------
# the differentiable forward
SUPPORTED = ("gnn-mlp", "ggnn")


def require_graph_model(model, nn, what: str) -> None:
    """Attributions are to the node embedder's output of a graph model: refuses ensembles (their own error), the sequence
    models and the GREAT var-misuse model, before any GPU work."""
    from buglab.controllers import _batching as Bt
    from buglab.models.ensemble.wrapper import EnsembleWrapper
    from buglab.models.gnn import GnnBugLabModel, GnnBugLabModule
    from buglab.models.seqmodel import SeqBugLabModule

    if isinstance(model, EnsembleWrapper):
        Bt.require_single_model(model, what)  # raises
    if not isinstance(model, GnnBugLabModel) or isinstance(nn, SeqBugLabModule) or not (nn is None or isinstance(nn, GnnBugLabModule)):
        raise NotImplementedError(f"{what}: node attributions are implemented for the graph models {SUPPORTED[0]} and {SUPPORTED[1]} "
                                  f"only (got {type(model).__name__}): not for the seq-* models, not for the GREAT var-misuse model")
    Bt.require_single_model(model, what)


@contextmanager
def frozen_parameters(nn):
    """For the duration no parameter asks for a gradient and none has a `.grad` a kernel could add into (hip_ops accumulates
    directly into the `.grad` of parameters an optimiser opted in): afterwards every `requires_grad` flag and every `.grad` --
    the same tensor, or None -- is what it was, also when the body raises."""
    state = [(p, p.requires_grad, p.grad) for p in nn.parameters()]
    try:
        for p, _, _ in state:
            p.requires_grad_(False)
            p.grad = None
        yield
    finally:
        for p, flag, grad in state:
            p.grad = grad
            p.requires_grad_(flag)


def flat_output(nn, mb, input_transform=None):
    """The raw, uncalibrated flat output [loc | text | var | swap] of `flat_prediction_output`'s two calls, NOT detached;
    `input_transform` is handed to GraphNeuralNetwork.forward through a shallow copy of the minibatch's graph_data."""
    import torch

    graph_data = mb["graph_data"] if input_transform is None else dict(mb["graph_data"], input_transform=input_transform)
    _, loc_lp, enc_out, _ = nn.compute_localization_logprobs(graph_data)
    swap_lp, text_lp, var_lp, _ = nn._compute_repair_logprobs(
        enc_out, mb["target_rewrites"], mb["rewrite_to_location_group"], mb["candidate_symbol_to_location_group"],
        mb["swapped_pair_to_call_location_group"], mb["repair_group_ptr"], mb["repair_group_items"])
    flat = torch.cat([t.reshape(-1).float() for t in (loc_lp, text_lp, var_lp, swap_lp)])
    assert mb.get("prediction_layout") is None or flat.shape[0] == mb["prediction_layout"].flat_size
    return flat


def objective_of(flat, flat_indices):
    """f_b = the fp64 sum of the (at most two) flat entries flat_indices[b] names, -1 = absent; float64 [B].  Device ops only."""
    import torch

    idx = flat_indices.long()
    present = idx >= 0
    picked = flat[idx.clamp(min=0).reshape(-1)].reshape(idx.shape).double()
    return torch.where(present, picked, torch.zeros_like(picked)).sum(dim=1)


def input_gradients(nn, mb, flat_indices, alpha: float = 1.0):
    """-> (x, G, objective): x float32 [N, D] the node embedder's output in eval mode (detached); objective float64 [B], f_b
    evaluated at the input alpha * x from the model's raw, uncalibrated flat output (`flat_indices` int32 [B, 2] on the device,
    -1 = absent: the sum of the entries it names); G float32 [N, D] the gradient of sum_b f_b at alpha * x.  Graphs of a
    minibatch do not interact (LayerNorm is per node, the localisation pooling per graph), so the rows of G that belong to
    graph b are the gradient of f_b alone.  One forward, one `torch.autograd.grad`; the parameters are frozen for the duration
    (`frozen_parameters`), so no weight gradient is returned or accumulated anywhere."""
    import torch

    from buglab.models import hip_ops

    seen: List[Any] = []
    alpha = float(alpha)

    def transform(h):
        seen.append(h.detach())
        seen.append((alpha * seen[0]).requires_grad_())  # a new leaf (alpha == 1: the same bits)
        return seen[1]

    was_training = nn.training
    nn.eval()
    try:
        with frozen_parameters(nn), torch.enable_grad():
            objective = objective_of(flat_output(nn, mb, transform), flat_indices)
            (G,) = torch.autograd.grad(objective.sum(), seen[1])
            hip_ops.join_side_stream()  # before this minibatch's gradient buffers can be recycled
    finally:
        nn.train(was_training)
    return seen[0], G, objective.detach()


def objective_at(nn, mb, flat_indices, alpha: Optional[float] = None):
    """f_b at alpha * x (None: at x, the model's own forward) with no backward pass; float64 [B].  Call under torch.no_grad()."""
    transform = None if alpha is None else (lambda h: float(alpha) * h)
    return objective_of(flat_output(nn, mb, transform), flat_indices)
