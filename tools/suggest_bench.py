#!/usr/bin/env python
"""What ranked suggestions cost on one GPU (buglab/models/suggest.py, evaluate.py --top-k), on a synthetic shard of BugLab graphs.

    python tools/suggest_bench.py [--samples N] [--repeats K] [--top-k K] [--out FILE]

On a `gnn-mlp` detector (random weights: the rates depend on the shapes, not on what the model learnt), sequential collate, after
a warm-up pass, bracketed by device synchronisations, median of K runs:
  * the ranking of a run alone, on the flat outputs of its predict minibatches (forwarded once, kept on the device):
    device = one bl_rank_suggestions launch per minibatch into run-long buffers and one copy back; twin = `rank_host` on the same
    flat outputs copied to the host beforehand (the copy is timed apart).  The two must give the same bytes;
  * `evaluate_on_device(top_k=K)` against plain `evaluate_on_device` on the same data: what --top-k adds to an evaluation;
  * `suggest` on the device against `suggest(host=True)`: the whole tool, forward included;
  * the kernel alone (HIP events around 20 launches) on one 50-sample minibatch, at k = 1, K and 32.
Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
from pathlib import Path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "neurips21-self-supervised-bug-detection-and-repair_amd"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from buglab.controllers import _batching as Bt  # noqa: E402
from buglab.data.synthetic import make_report_dataset  # noqa: E402
from buglab.models import _suggest as S  # noqa: E402
from buglab.models import hip_ops  # noqa: E402
from buglab.models.evaluate import evaluate_on_device  # noqa: E402
from buglab.models.modelregistry import load_model  # noqa: E402
from buglab.models.suggest import suggest  # noqa: E402

SPEC = {"modelName": "gnn-mlp", "hidden_state_size": 128, "dropout_rate": 0.1}


def _timed(fn, repeats):
    times, out = [], None
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return {"median_s": round(statistics.median(times), 5), "min_s": round(min(times), 5), "max_s": round(max(times), 5)}, out


def _kernel_ms(fn, launches=20):
    fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(launches):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return round(start.elapsed_time(stop) / launches, 4)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--samples", type=int, default=2000)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--top-k", type=int, default=5)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    dev = torch.device("cuda")
    n, k = args.samples, args.top_k
    with tempfile.TemporaryDirectory() as tmp:
        data = make_report_dataset(n, seed=1, kind="graph")
        model = load_model(SPEC, Path(tmp) / "m.pkl.gz")[0]
        model.compute_metadata(iter(data))
        torch.manual_seed(1)
        nn_ = model.build_neural_module().cuda().eval()
        fields = hip_ops.SUGGEST_INDEX_FIELDS

        # ---- the ranking alone, on the run's flat outputs
        run = []  # (flat on the device, indices on the host, indices on the device, B)
        with torch.no_grad(), model._tensorize_all_location_rewrites():
            extend = lambda layout, points, d: S.suggest_indices(layout, points)
            for mb, _ in Bt.prediction_minibatches(model, ((x, None) for x in data), dev, False, extend, lambda tag: None):
                ix = mb["selfsup"]
                run.append((Bt.flat_prediction_output(nn_, mb), ix, dict(zip(fields, Bt.to_device_i32([getattr(ix, f) for f in fields], dev))),
                            int(ix.tgt_rw.shape[0])))
        total = sum(B for _, _, _, B in run)
        rank = torch.empty((2, total), dtype=torch.int32, device=dev)
        entry = torch.empty((total, k), dtype=torch.int32, device=dev)
        logprob = torch.empty((total, k), dtype=torch.float64, device=dev)

        def on_device():
            at = 0
            for flat, _, dev_ix, B in run:
                hip_ops.rank_suggestions(flat, dev_ix, rank, entry, logprob, at, k=k)
                at += B
            return rank.cpu().numpy(), entry.cpu().numpy(), logprob.cpu().numpy()

        t_copy, flats = _timed(lambda: [flat.cpu().numpy() for flat, _, _, _ in run], args.repeats)

        def on_host():
            parts = [S.rank_host(flat, ix, k) for flat, (_, ix, _, _) in zip(flats, run)]
            return np.concatenate([r for r, _, _ in parts], axis=1), np.concatenate([e for _, e, _ in parts]), np.concatenate([v for _, _, v in parts])

        on_device()  # warm-up
        t_dev, got = _timed(on_device, args.repeats)
        t_twin, want = _timed(on_host, args.repeats)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want))  # bit for bit, padding included
        r = {"samples": total, "minibatches": len(run), "top_k": k, "repeats": args.repeats, "device": torch.cuda.get_device_name(0),
             "rewrites": int(sum(ix.rw_idx.shape[0] for _, ix, _, _ in run)), "locations": int(sum(ix.loc_idx.shape[0] for _, ix, _, _ in run)),
             "ranking_device": t_dev, "ranking_twin": t_twin, "flat_copy_to_host": t_copy}

        # ---- what --top-k adds to an evaluation on the device
        plain = lambda: evaluate_on_device(model, nn_, data, dev, parallelize=False).format()
        ranked = lambda: (lambda rep: rep.format() + rep.format_top_k())(evaluate_on_device(model, nn_, data, dev, parallelize=False, top_k=k))
        plain(), ranked()
        r["evaluate_on_device"], text = _timed(plain, args.repeats)
        r["evaluate_on_device_top_k"], text_k = _timed(ranked, args.repeats)
        assert text_k.startswith(text)

        # ---- the tool, forward included
        records = lambda host: [s.ranked for s in suggest(model, nn_, data, dev, k, host=host, parallelize=False)]
        records(False), records(True)
        r["suggest_device_path"], a = _timed(lambda: records(False), args.repeats)
        r["suggest_host_path"], b = _timed(lambda: records(True), args.repeats)
        assert a == b

        # ---- the kernel alone, on the first minibatch
        flat, ix, dev_ix, B = run[0]
        r["kernel"] = {"samples": B, "rewrites": int(ix.rw_idx.shape[0]), "locations": int(ix.loc_idx.shape[0])}
        rk = torch.empty((2, B), dtype=torch.int32, device=dev)
        for kk in sorted({1, k, 32}):
            e, v = torch.empty((B, kk), dtype=torch.int32, device=dev), torch.empty((B, kk), dtype=torch.float64, device=dev)
            r["kernel"][f"ms_k{kk}"] = _kernel_ms(lambda: hip_ops.rank_suggestions(flat, dev_ix, rk, e, v, 0, k=kk))
    print(json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(r, f, indent=1)


if __name__ == "__main__":
    main()
