#!/usr/bin/env python
"""Throughput of the two self-supervision services on one GPU (buglab.controllers), on synthetic BugLab samples.

    python tools/selfsup_bench.py [--samples N] [--reference-samples R] [--repeats K] [--out FILE]

Per model family (`gnn-mlp`, `seq-great`):
  * scoring: graphs/s of `score_rewrites` over N records (NO_BUG + 4 rewritten graphs each), against the reference's call
    pattern on the SAME model and data -- `predict` on the graphs of one record at a time, every prediction value copied to
    the host, the true fix's log-probability picked in Python (reference detectordatascoringworker.py:99-130) -- on R records;
  * selection: datapoints/s of `select_rewrites` over N datapoints, against `predict` on one datapoint at a time plus
    `calculate_selection_distribution` and `np.random.choice(..., replace=False)` (reference bugselectorserver.py:120-150).
Every timing follows a warm-up pass, is bracketed by device synchronisations and is repeated K times: the median and the
spread (min .. max) are reported.  parallelize=True for the batched services; the reference pattern runs sequentially, as
its servers do.  Prints one JSON line per family.
"""
import argparse
import copy
import json
import os
import statistics
import sys
import tempfile
import time
from pathlib import Path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "neurips21-self-supervised-bug-detection-and-repair_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from buglab.controllers.bugselector import calculate_selection_distribution, select_rewrites  # noqa: E402
from buglab.controllers.detectorscoring import score_rewrites  # noqa: E402
from buglab.data.synthetic import make_buglab_seq_dataset, make_scoring_records  # noqa: E402
from buglab.models.modelregistry import load_model  # noqa: E402

SPECS = {
    "gnn-mlp": {"modelName": "gnn-mlp", "hidden_state_size": 128, "dropout_rate": 0.1},
    "seq-great": {"modelName": "seq-great", "hidden_state_size": 128, "num_layers": 4, "num_heads": 8, "intermediate_dimension_size": 512,
                  "dropout_rate": 0.1},
}


def _timed(fn, data, repeats):
    """-> (times of `repeats` runs of fn over a fresh deep copy of data, items yielded per run)"""
    times, n = [], 0
    for _ in range(repeats):
        points = copy.deepcopy(data)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = sum(1 for _ in fn(points))
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return times, n


def _rate(count, times):
    return {"median": round(count / statistics.median(times), 1), "min": round(count / max(times), 1), "max": round(count / min(times), 1)}


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--samples", type=int, default=400)
    p.add_argument("--reference-samples", type=int, default=60)
    p.add_argument("--warmup-samples", type=int, default=60)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--families", default="gnn-mlp,seq-great")
    p.add_argument("--out", default=None)
    args = p.parse_args()
    dev = torch.device("cuda")
    data = make_buglab_seq_dataset(args.samples, seed=1)
    records = make_scoring_records(data, seed=2)
    graphs_per_record = sum(len(r["rewrites"]) for r in records) / len(records)
    results = []
    with tempfile.TemporaryDirectory() as tmp:
        for family in args.families.split(","):
            model = load_model(SPECS[family], Path(tmp) / f"{family}.pkl.gz")[0]
            model.compute_metadata(copy.deepcopy(data))
            torch.manual_seed(1)
            nn_ = model.build_neural_module().cuda().eval()

            def score_batched(recs):
                return score_rewrites(model, nn_, recs, dev, parallelize=True)

            def score_one_record_at_a_time(recs):
                for rec in recs:
                    idxs = [-1 if k == "NO_BUG" else int(k) for k in rec["rewrites"]]
                    out = [-float("inf")] * (len(rec["original"]["graph"]["reference_nodes"]) + 1)
                    preds = list(model.predict([g for g, _ in rec["rewrites"].values()], nn_, dev, False))
                    for i, (point, loc, rw) in enumerate(preds):
                        t = point["target_fix_action_idx"]
                        out[idxs[i]] = float(loc[-1] if t is None else loc[point["graph"]["reference_nodes"][t]] + rw[t])
                    rec["original"]["candidate_rewrite_logprobs"] = out
                    yield rec["original"]

            def select_batched(points):
                return select_rewrites(model, nn_, points, dev, seed=1, parallelize=True)

            def select_one_at_a_time(points):
                for d in points:
                    point, loc, rw = next(iter(model.predict([d], nn_, dev, False)))
                    g = [r + loc[n] for r, n in zip(rw, point["graph"]["reference_nodes"])] + [loc[-1]]
                    dist = calculate_selection_distribution(g, 1.0, 0.02)
                    picked = np.random.choice(range(len(g)), size=min(4, len(g)), replace=False, p=dist)
                    yield point, {("NO_BUG" if i == len(g) - 1 else str(i)): float(g[i]) for i in picked}

            r = {"family": family, "records": len(records), "graphs_per_record": graphs_per_record, "repeats": args.repeats,
                 "reference_records": args.reference_samples}
            for name, batched, single, full, part, per_item in (
                    ("scoring_graphs_per_s", score_batched, score_one_record_at_a_time, records, records[:args.reference_samples], graphs_per_record),
                    ("selection_datapoints_per_s", select_batched, select_one_at_a_time, data, data[:args.reference_samples], 1.0)):
                warm = full[:args.warmup_samples]
                _timed(batched, warm, 1)
                tb, nb = _timed(batched, full, args.repeats)
                _timed(single, warm[:10], 1)
                ts, ns = _timed(single, part, args.repeats)
                r[name] = {"batched": _rate(nb * per_item, tb), "one_request_at_a_time": _rate(ns * per_item, ts),
                           "speedup_of_medians": round((nb / statistics.median(tb)) / (ns / statistics.median(ts)), 2)}
            print(json.dumps(r), flush=True)
            results.append(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
