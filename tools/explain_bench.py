#!/usr/bin/env python
"""What explanations cost on one GPU (buglab/models/explain.py), at the benchmark's graph shape (bench.py: 64 graphs of 2000
nodes and 10000 messages, 16 edge types, hidden 128, 8 layers).

    python tools/explain_bench.py [--graphs G] [--repeats K] [--out FILE]

On a `gnn-mlp` detector (random weights: the rates depend on the shapes, not on what the model learnt), per minibatch, for
`--steps 1` (gradient x input) and `--steps 16` (integrated gradients), after a warm-up, median of K runs bracketed by device
synchronisations:
  1. forward + backward: the `input_gradients` calls of the steps (existing kernels; NO_BUG's log-probability is explained);
  2. the two new kernels: one bl_attr_node_scores per step and one bl_attr_topk (k = 10); and, from HIP events around 20
     launches, bl_attr_node_scores alone with the rate of its algorithmic bytes 2 N D 4 (compare tools/hbm_bench.py on the same
     machine; the operands of one minibatch may fit the last-level cache);
  3. the twin: the copies of x and G to the host, `node_scores_host` per step and one `topk_host`.
The device results must equal the twin's bytes.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "neurips21-self-supervised-bug-detection-and-repair_amd"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from buglab.data.collate import collate_samples, to_device  # noqa: E402
from buglab.data.synthetic import make_samples  # noqa: E402
from buglab.models import _explain as E  # noqa: E402
from buglab.models import hip_ops  # noqa: E402
from buglab.models.gnn import build_gnn_mlp_module  # noqa: E402


def _timed_ms(fn, repeats):
    times, out = [], None
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    return {"median_ms": round(statistics.median(times), 3), "min_ms": round(min(times), 3), "max_ms": round(max(times), 3)}, out


def _kernel_ms(fn, launches=20):
    fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(launches):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / launches


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--graphs", type=int, default=64)
    p.add_argument("--nodes", type=int, default=2000)
    p.add_argument("--messages", type=int, default=10000)
    p.add_argument("--types", type=int, default=16)
    p.add_argument("--hidden", type=int, default=128)
    p.add_argument("--layers", type=int, default=8)
    p.add_argument("--top-k", type=int, default=10)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    dev = torch.device("cuda")
    samples = make_samples(a.graphs, seed=1000, num_nodes=a.nodes, num_messages=a.messages, num_edge_types=a.types)
    mb_np = collate_samples(samples, a.types)
    mb = to_device(mb_np, dev)
    torch.manual_seed(1)
    nn_ = build_gnn_mlp_module(a.hidden, a.layers, a.types, dropout_rate=0.2).to(dev).eval()
    B, k = a.graphs, a.top_k
    C = int(mb_np["graph_data"]["reference_node_ids"]["candidate_nodes"].shape[0])
    chosen = torch.stack([torch.arange(C, C + B, dtype=torch.int32), torch.full((B,), -1, dtype=torch.int32)], dim=1).to(dev)  # NO_BUG
    node_off_np = np.concatenate([[0], np.cumsum(mb_np["graph_data"]["num_nodes_per_graph"])]).astype(np.int32)
    node_off = torch.from_numpy(node_off_np).to(dev)
    N = int(node_off_np[-1])
    out = (torch.empty((B, k), dtype=torch.int32, device=dev), torch.empty((B, k), dtype=torch.float64, device=dev),
           torch.empty((2, B), dtype=torch.float64, device=dev))
    score = torch.empty(N, dtype=torch.float64, device=dev)
    r = {"graphs": B, "nodes": N, "messages": int(mb_np["graph_data"]["msg_src"].shape[0]), "hidden": a.hidden, "layers": a.layers, "top_k": k,
         "repeats": a.repeats, "device": torch.cuda.get_device_name(0)}
    alphas = lambda steps: [1.0] if steps == 1 else [(m - 0.5) / steps for m in range(1, steps + 1)]
    for steps in (1, 16):
        passes = lambda: [E.input_gradients(nn_, mb, chosen, alpha)[:2] for alpha in alphas(steps)]
        passes()  # warm-up
        t_model, grads = _timed_ms(passes, a.repeats)

        def on_device():
            for m, (x, G) in enumerate(grads):
                hip_ops.attribute_node_scores(x, G, score, weight=1.0 / steps, accumulate=m > 0)
            hip_ops.attribute_topk(score, node_off, *out, 0, k=k)
            return tuple(t.cpu().numpy() for t in out)

        def on_host():
            s = None
            for x, G in grads:
                s = E.node_scores_host(x.cpu().numpy(), G.cpu().numpy(), s, 1.0 / steps)
            return E.topk_host(s, node_off_np, k)

        on_device()
        t_dev, got = _timed_ms(on_device, a.repeats)
        t_twin, want = _timed_ms(on_host, max(1, a.repeats // 2))
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got, want))  # bit for bit
        r[f"steps_{steps}"] = {"forward_backward": t_model, "attribution_kernels_and_copy_back": t_dev, "twin_with_copies": t_twin}
    x, G = grads[0]
    D = int(x.shape[1])
    ms = _kernel_ms(lambda: hip_ops.attribute_node_scores(x, G, score))
    r["bl_attr_node_scores"] = {"N": N, "D": D, "ms": round(ms, 4), "bytes": 2 * N * D * 4, "GB_per_s": round(2 * N * D * 4 / ms / 1e6, 1)}
    r["bl_attr_topk"] = {"ms": round(_kernel_ms(lambda: hip_ops.attribute_topk(score, node_off, *out, 0, k=k)), 4)}
    print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)


if __name__ == "__main__":
    main()
