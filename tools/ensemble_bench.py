#!/usr/bin/env python
"""Ensemble predict throughput on one GPU (buglab.models.ensemble), on synthetic BugLab samples.

    python tools/ensemble_bench.py [--samples N] [--reference-samples R] [--out FILE]

Reports, per ensemble (M = 1, 2, 3 `gnn-mlp` members; a mixed `gnn-mlp` + `seq-great` pair):
  * graphs/s of `EnsembleWrapper.predict` over N samples (one minibatch for all members, one combine launch);
  * the members' own `predict` times over the same samples, summed, and the ratio ensemble / sum;
  * graphs/s of the reference's scheme (reference ensemble/wrapper.py:33-40: every member's `predict` on a one-sample list,
    one sample at a time), timed through the members' own `predict` on R samples -- for comparison only.
Every timing is preceded by a warm-up pass and bracketed by device synchronisations; parallelize=True as evaluate.py runs it.
The combine kernel's own time comes from a separate `rocprofv3 --kernel-trace --stats -- python tools/ensemble_bench.py` run.
Prints one JSON line per ensemble.
"""
import argparse
import copy
import json
import os
import sys
import tempfile
import time
from pathlib import Path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "neurips21-self-supervised-bug-detection-and-repair_amd"))

import torch  # noqa: E402

from buglab.data.synthetic import make_buglab_seq_dataset  # noqa: E402
from buglab.models.ensemble.wrapper import EnsembleModuleWrapper, EnsembleWrapper  # noqa: E402
from buglab.models.modelregistry import load_model  # noqa: E402

SPECS = {
    "gnn-mlp": {"modelName": "gnn-mlp", "hidden_state_size": 128, "dropout_rate": 0.1},
    "seq-great": {"modelName": "seq-great", "hidden_state_size": 128, "num_layers": 4, "num_heads": 8, "intermediate_dimension_size": 512,
                  "dropout_rate": 0.1},
}


def _member(family, data, seed, tmp):
    model = load_model(SPECS[family], Path(tmp) / f"{family}_{seed}.pkl.gz")[0]
    model.compute_metadata(copy.deepcopy(data))
    torch.manual_seed(seed)
    return model, model.build_neural_module().cuda().eval()


def _timed(fn, data):
    points = copy.deepcopy(data)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = sum(1 for _ in fn(points))
    torch.cuda.synchronize()
    return time.perf_counter() - t0, n


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--samples", type=int, default=1000)
    p.add_argument("--reference-samples", type=int, default=100)
    p.add_argument("--warmup-samples", type=int, default=150)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    dev = torch.device("cuda")
    data = make_buglab_seq_dataset(args.samples, seed=1)
    warm = make_buglab_seq_dataset(args.warmup_samples, seed=2)
    results = []
    with tempfile.TemporaryDirectory() as tmp:
        pool = {("gnn-mlp", s): _member("gnn-mlp", data, s, tmp) for s in (1, 2, 3)}
        pool[("seq-great", 4)] = _member("seq-great", data, 4, tmp)
        for name, keys in (("gnn-mlp x1", [("gnn-mlp", 1)]), ("gnn-mlp x2", [("gnn-mlp", 1), ("gnn-mlp", 2)]),
                           ("gnn-mlp x3", [("gnn-mlp", 1), ("gnn-mlp", 2), ("gnn-mlp", 3)]),
                           ("gnn-mlp + seq-great", [("gnn-mlp", 1), ("seq-great", 4)])):
            members = [pool[k] for k in keys]
            ens = EnsembleWrapper([m for m, _ in members], "avg")
            ens_nn = EnsembleModuleWrapper([n for _, n in members])
            run_ens = lambda pts: ens.predict(iter(pts), ens_nn, dev, True)
            _timed(run_ens, warm)
            t_ens, n_ens = _timed(run_ens, data)
            t_members = 0.0
            for model, nn_ in members:
                run = lambda pts, m=model, n=nn_: m.predict(iter(pts), n, dev, True)
                _timed(run, warm)
                t_members += _timed(run, data)[0]
            ref_data = data[:args.reference_samples]

            def one_by_one(pts):
                for d in pts:
                    for model, nn_ in members:
                        yield from model.predict([d], nn_, dev, False)

            _timed(one_by_one, warm[:10])
            t_ref, _ = _timed(one_by_one, ref_data)
            r = {"ensemble": name, "members": len(members), "samples": n_ens, "ensemble_graphs_per_s": round(n_ens / t_ens, 1),
                 "ensemble_s": round(t_ens, 4), "sum_member_predict_s": round(t_members, 4),
                 "ratio_to_sum_of_members": round(t_ens / t_members, 3),
                 "reference_scheme_graphs_per_s": round(len(ref_data) / t_ref, 1),
                 "speedup_over_reference_scheme": round((n_ens / t_ens) / (len(ref_data) / t_ref), 1)}
            print(json.dumps(r), flush=True)
            results.append(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
