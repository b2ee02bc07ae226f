#!/usr/bin/env python
"""
Usage:
    explain.py [options] MODEL_FILENAME DATA_PATH OUT_PATH

Options:
    --top-k=<K>                Attributed nodes listed per sample, 1 <= K <= 32. [default: 10]
    --steps=<M>                1: gradient x input; M > 1: integrated gradients, M midpoint steps from the zero input. [default: 1]
    --rank=<R>                 Explain the suggestion at this position of suggest.py's ranking. [default: 0]
    --signed                   List the nodes by attribution, descending, instead of by its magnitude.
    --assume-buggy             NO_BUG is never the explained suggestion.
    --limit-num-elements=<num> Limit the number of elements to explain.
    --sequential               Do not parallelize data loading. Makes debugging easier.
    --host                     Reduce and select with the NumPy twin on copied arrays (the same forward and backward passes).
    -h --help                  Show this screen.

BEYOND THE REFERENCE, which shows what was flagged and nothing about why.  For each sample: which graph nodes the model's
log-probability of one suggested fix rests on.  The fix is the entry at position `--rank` of suggest.py's joint ranking
(calibrated values are ranked where the checkpoint carries a calibration).  What is attributed is the MODEL'S OWN
log-probability of that entry, f = location log-probability + rewrite log-probability (NO_BUG: its location log-probability)
from the raw output -- not the calibrated one: a calibration rescales a sample's distributions, it changes which entry is
ranked where and leaves the attributions of a given entry to the model as it was trained.

With x [N, D] the node embedder's output (eval mode, no dropout) and G = df/dx, node n gets a_n = sum_d G[n, d] x[n, d]
(`--steps 1`, gradient x input), or the mean of that over the gradients at alpha_m x, alpha_m = (m - 1/2) / M (`--steps M`,
integrated gradients from the all-zero baseline by the midpoint rule; then `baseline` = f at the zero input is reported too,
and sum a_n approaches f(x) - f(0) as M grows).  One backward pass serves a whole minibatch: graphs do not interact (LayerNorm
is per node, the localisation pooling per graph), so the gradient of sum_b f_b with respect to graph b's rows is that of f_b.

The forward and backward passes are the training kernels; what follows them is csrc/bl_explain.hip: the fp64 reduction of x
and G to one number per node, accumulated over the steps (hip_ops.attribute_node_scores), and the per-graph sums and first K
nodes (hip_ops.attribute_topk).  The results stay on the device for the whole run and are copied back once.  OUT_PATH
receives JSON lines (gzip when the name ends in .gz), one record per sample `tensorize` accepts, in input order.  A sample
with fewer than `--rank` + 1 rankable entries gets a record with "explained": null and no attributions.  Only the graph models
gnn-mlp and ggnn are supported.
"""
import argparse
import sys
from pathlib import Path
from typing import Any, Callable, Dict, Iterable, Iterator, List, NamedTuple, Optional

if __package__ in (None, ""):
    sys.path.insert(0, str(Path(__file__).resolve().parents[2]))

import numpy as np
import torch

from buglab.models import _explain as E
from buglab.models import _suggest as S
from buglab.models._cli import open_model, require_gpu, write_records
from buglab.models._suggest import Ranked
from buglab.models.suggest import suggestion_record


def node_kinds(graph, nodes: Iterable[int]) -> List[str]:
    """"token": an endpoint of a NextToken edge; "subtoken": the target of a HasSubtoken edge; "other" otherwise"""
    nodes = [int(n) for n in nodes]
    if not nodes:
        return []
    edges = graph["edges"]
    tokens = {int(v) for e in edges.get("NextToken", ()) for v in (e[0], e[1])}
    subtokens = {int(e[1]) for e in edges.get("HasSubtoken", ())}
    return ["token" if n in tokens else "subtoken" if n in subtokens else "other" for n in nodes]


class Explanation(NamedTuple):
    """One sample's answer: its position in the input, the datapoint, the head of its ranking (rank + 1 entries at most), and
    the attributions of the entry at `rank`."""

    position: int
    datapoint: Any
    ranked: Ranked
    rank: int
    steps: int
    objective: float           # f(x)
    baseline: Optional[float]  # f(0), with steps > 1
    total: float               # sum a_n over the graph's nodes
    abs_total: float           # sum |a_n|
    nodes: List[int]           # indices into datapoint["graph"]["nodes"], in listing order
    scores: List[float]        # their a_n

    @property
    def explained(self) -> bool:
        return len(self.ranked.entries) > self.rank

    def record(self) -> Dict[str, Any]:
        if not self.explained:
            return {"position": self.position, "explained": None, "steps": self.steps, "attributions": []}
        graph = self.datapoint["graph"]
        out: Dict[str, Any] = {"position": self.position,
                               "explained": suggestion_record(self.position, self.datapoint, self.ranked)["suggestions"][self.rank],
                               "objective": self.objective, "sum": self.total, "abs_sum": self.abs_total, "steps": self.steps}
        if self.baseline is not None:
            out["baseline"] = self.baseline
        out["attributions"] = [{"node": n, "label": graph["nodes"][n], "kind": kind, "score": a,
                                "share": abs(a) / self.abs_total if self.abs_total > 0 else 0.0}
                               for n, a, kind in zip(self.nodes, self.scores, node_kinds(graph, self.nodes))]
        return out

    def influences(self) -> List[Dict[str, Any]]:
        """the `influences` list of a visualize.py snippet"""
        return [{"label": a["label"], "kind": a["kind"], "share": a["share"]} for a in self.record()["attributions"]]


def _chosen_on_device(entry: torch.Tensor, ix: Dict[str, torch.Tensor]) -> torch.Tensor:
    """_explain.chosen_flat_indices with device ops: int32 [B, 2]"""
    rw_off = ix["rw_off"].long()
    e = entry.long()
    n_rw = rw_off[1:] - rw_off[:-1]
    is_rw = (e >= 0) & (e < n_rw)
    is_nobug = (e >= 0) & ~is_rw
    minus = torch.full_like(ix["nobug_idx"], -1)
    if ix["rw_idx"].shape[0] == 0:
        return torch.stack([torch.where(is_nobug, ix["nobug_idx"], minus), minus], dim=1)
    at = (rw_off[:-1] + e).clamp(0, ix["rw_idx"].shape[0] - 1)
    first = torch.where(is_rw, ix["rw_loc_idx"][at], torch.where(is_nobug, ix["nobug_idx"], minus))
    return torch.stack([first, torch.where(is_rw, ix["rw_idx"][at], minus)], dim=1)


def _explain_run(model, nn, data, device, k, steps, rank, signed, assume_buggy, host, parallelize, rejected, capacity
                 ) -> Iterator[Explanation]:
    from buglab.controllers import _batching as Bt
    from buglab.models import hip_ops
    from buglab.models._calibrate import apply_to_flat

    device = torch.device(device)
    R = rank + 1

    def extend(layout, points, dev, mb):
        six = S.suggest_indices(layout, points, mb.get("node_mappings"))
        gd = mb["graph_data"]
        eix = E.explain_indices(gd["num_nodes_per_graph"], int(gd["num_nodes"]), six, points)
        fields = hip_ops.SUGGEST_INDEX_FIELDS
        tensors = Bt.to_device_i32([getattr(six, f) for f in fields] + [eix.node_off], dev)
        return {"ix": dict(zip(fields + ("node_off",), tensors)), "points": points, "node_off": eix.node_off}

    one, per_k, per_rank, pair = (Bt.SAMPLES,), (Bt.SAMPLES, k), (Bt.SAMPLES, R), (2, Bt.SAMPLES)
    out = Bt.RunColumns(device, Bt.run_capacity(capacity, data, 1 << 12),
                        [("score", "float64", per_k), ("sums", "float64", pair), ("objective", "float64", one), ("baseline", "float64", one),
                         ("logprob", "float64", per_rank), ("node", "int32", per_k), ("entry", "int32", per_rank), ("rank", "int32", pair)])
    points: List[Any] = []
    positions: List[int] = []
    host_parts: List[Any] = []  # --host: (node, score, sums) of every minibatch
    nn.eval()
    with torch.no_grad(), model._tensorize_all_location_rewrites():
        for mb, tags in Bt.prediction_minibatches(model, ((d, i) for i, d in enumerate(data)), device, parallelize, extend, rejected,
                                                  extend_sees_minibatch=True):
            ix = mb["selfsup"]["ix"]
            B = len(mb["selfsup"]["points"])
            assert len(tags) == B
            n = out.reserve(B)
            # which entry: the ranking of suggest.py, on calibrated values where the checkpoint carries a calibration
            raw = E.flat_output(nn, mb)
            flat = raw
            if mb.get("confidence_calibration") is not None:
                flat = raw.clone()
                apply_to_flat(mb["confidence_calibration"], flat, mb)
            hip_ops.rank_suggestions(flat, ix, out["rank"], out["entry"], out["logprob"], n, k=R, skip_nobug=assume_buggy)
            chosen = _chosen_on_device(out["entry"][n:n + B, rank], ix)
            out["objective"][n:n + B].copy_(E.objective_of(raw, chosen))  # of the raw output: the model's own log-probability
            # the attributions: one backward per step, two small launches after it
            score = None
            for m in range(1, steps + 1):
                x, G, _ = E.input_gradients(nn, mb, chosen, 1.0 if steps == 1 else (m - 0.5) / steps)
                if host:
                    score = E.node_scores_host(x.cpu().numpy(), G.cpu().numpy(), score, 1.0 / steps)
                    continue
                if score is None:
                    score = torch.empty(x.shape[0], dtype=torch.float64, device=device)
                hip_ops.attribute_node_scores(x, G, score, weight=1.0 / steps, accumulate=m > 1)
            if steps > 1:
                out["baseline"][n:n + B].copy_(E.objective_at(nn, mb, chosen, 0.0))
            if host:
                host_parts.append(E.topk_host(score, mb["selfsup"]["node_off"], k, not signed))
            else:
                hip_ops.attribute_topk(score, ix["node_off"], out["node"], out["score"], out["sums"], n, k=k, by_abs=not signed)
            points.extend(mb["selfsup"]["points"]), positions.extend(tags)
    got = out.to_host()  # the one copy (and the one synchronisation) of the run
    if host and host_parts:
        got["node"] = np.concatenate([p[0] for p in host_parts])
        got["score"] = np.concatenate([p[1] for p in host_parts])
        got["sums"] = np.concatenate([p[2] for p in host_parts], axis=1)
    for b in range(out.n):
        listed = int((got["entry"][b] >= 0).sum())
        ranked = Ranked(got["entry"][b, :listed].tolist(), got["logprob"][b, :listed].tolist(), int(got["rank"][0, b]),
                        int(got["rank"][1, b]))
        shown = int((got["node"][b] >= 0).sum()) if listed > rank else 0
        yield Explanation(positions[b], points[b], ranked, rank, steps, float(got["objective"][b]),
                          float(got["baseline"][b]) if steps > 1 else None, float(got["sums"][0, b]), float(got["sums"][1, b]),
                          got["node"][b, :shown].tolist(), got["score"][b, :shown].tolist())


def explain(model, nn, data: Iterable[Any], device, k: int = 10, *, steps: int = 1, rank: int = 0, signed: bool = False,
            assume_buggy: bool = False, host: bool = False, parallelize: bool = True,
            rejected: Optional[Callable[[int], None]] = None, capacity: Optional[int] = None) -> Iterator[Explanation]:
    """The node attributions of the suggestion at position `rank` of `suggest`'s ranking, for every datapoint of `data` that
    `tensorize` accepts, in input order; `rejected(position)` is called for the others.  Attributions are of the model's own
    log-probability of that entry (the raw output), not of the calibrated one; the ranking uses the calibrated values where the
    checkpoint carries a calibration.  `steps` 1: gradient x input; M > 1: integrated gradients over M midpoint steps from the
    zero input.  Graph models (gnn-mlp, ggnn) only: ensembles, the seq-* models and the GREAT var-misuse model are refused
    before any GPU work.  Yields after the run's one copy back; every parameter's `.grad` and `requires_grad` is left as it was.
    `capacity`: the samples the result buffers (`RunColumns`) start with, by default `len(data)`, or 1 << 12 for a stream."""
    E.require_graph_model(model, nn, "explain")
    if not 1 <= int(k) <= E.MAX_K:
        raise ValueError(f"explain: k must be in [1, {E.MAX_K}] (got {k})")
    if int(steps) != steps or int(steps) < 1:
        raise ValueError(f"explain: steps must be an integer >= 1 (got {steps})")
    if int(rank) != rank or not 0 <= int(rank) < S.MAX_K:
        raise ValueError(f"explain: rank must be in [0, {S.MAX_K - 1}] (got {rank})")
    rejected = rejected or (lambda position: None)
    return _explain_run(model, nn, data, device, int(k), int(steps), int(rank), bool(signed), bool(assume_buggy), bool(host),
                        parallelize, rejected, capacity)


def run(arguments) -> int:
    from buglab.runtime.richpath import RichPath
    from buglab.utils.msgpackutils import load_all_msgpack_l_gz

    lim = None if arguments["--limit-num-elements"] is None else int(arguments["--limit-num-elements"])
    data = load_all_msgpack_l_gz(RichPath.create(arguments["DATA_PATH"]), shuffle=False, limit_num_yielded_elements=lim)  # a stream
    require_gpu(None, "explain.py")
    model, nn, device, _ = open_model(arguments["MODEL_FILENAME"])
    refused: List[int] = []
    found = explain(model, nn, data, device, int(arguments["--top-k"]), steps=int(arguments["--steps"]), rank=int(arguments["--rank"]),
                    signed=bool(arguments.get("--signed")), assume_buggy=bool(arguments.get("--assume-buggy")),
                    host=bool(arguments.get("--host")), parallelize=not arguments.get("--sequential"), rejected=refused.append)
    count = write_records((x.record() for x in found), arguments["OUT_PATH"])
    print(f"explain.py: {count} samples explained, {len(refused)} rejected by tensorize", file=sys.stderr)
    return count


if __name__ == "__main__":
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("MODEL_FILENAME")
    p.add_argument("DATA_PATH")
    p.add_argument("OUT_PATH")
    p.add_argument("--top-k", default=10, type=int)
    p.add_argument("--steps", default=1, type=int)
    p.add_argument("--rank", default=0, type=int)
    p.add_argument("--signed", action="store_true")
    p.add_argument("--assume-buggy", action="store_true")
    p.add_argument("--limit-num-elements", default=None)
    p.add_argument("--sequential", action="store_true")
    p.add_argument("--host", action="store_true")
    ns = p.parse_args()
    run({"MODEL_FILENAME": ns.MODEL_FILENAME, "DATA_PATH": ns.DATA_PATH, "OUT_PATH": ns.OUT_PATH, "--top-k": ns.top_k, "--steps": ns.steps,
         "--rank": ns.rank, "--signed": ns.signed, "--assume-buggy": ns.assume_buggy, "--limit-num-elements": ns.limit_num_elements,
         "--sequential": ns.sequential, "--host": ns.host})
