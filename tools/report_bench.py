#!/usr/bin/env python
"""Time of a bug report on one GPU (buglab/models/visualize.py::scan), on synthetic BugLab graphs with source.

    python tools/report_bench.py [--samples N[,N...]] [--repeats K] [--top-k 50] [--out FILE]

Per size N, on a `gnn-mlp` detector (random weights: every rate below depends on the shapes, not on what the model learnt):
  * device path: `scan(only_incorrect=True, order_by_confidence=True, show_top_k=K)` -- summarise and order on the device,
    build the contexts of the K shown samples, render them;
  * host path, the only way without `scan`: `model.predict` (every log-probability copied to the host) + the per-sample
    restatement of the reference's loop (tests/visualize_ref.py), which builds EVERY sample's context before it filters, sorts
    and cuts, as the reference renders every snippet; then the same rendering of the K shown;
  both with the same model, data and minibatches, sequential collate, after a warm-up pass, bracketed by device
  synchronisations, median and spread of K runs;
  * the same two with no filter (every sample shown): the share of filtered-out samples is what the gap should grow with;
  * the two kernels alone (HIP events around 20 launches): bl_report_summarize on one 50-sample minibatch of this data,
    bl_report_order on N keys and on 2^17 keys.
Prints one JSON line per size.
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
from buglab.models import _report as R  # noqa: E402
from buglab.models import hip_ops  # noqa: E402
from buglab.models.modelregistry import load_model  # noqa: E402
from buglab.models.visualize import report_to_html, scan  # noqa: E402
from tests import visualize_ref as VR  # noqa: E402

SPEC = {"modelName": "gnn-mlp", "hidden_state_size": 128, "dropout_rate": 0.1}


def _timed(fn, repeats):
    times, out = [], None
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return {"median_s": round(statistics.median(times), 4), "min_s": round(min(times), 4), "max_s": round(max(times), 4)}, out


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
    p.add_argument("--samples", default="500,2000")
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--top-k", type=int, default=50)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    dev = torch.device("cuda")
    results = []
    with tempfile.TemporaryDirectory() as tmp:
        for n in (int(x) for x in args.samples.split(",")):
            data = make_report_dataset(n, seed=1, kind="graph")
            model = load_model(SPEC, Path(tmp) / "m.pkl.gz")[0]
            model.compute_metadata(iter(data))
            torch.manual_seed(1)
            nn_ = model.build_neural_module().cuda().eval()

            def device_path(only_incorrect, k):
                report = scan(model, nn_, iter(data), dev, parallelize=False, only_incorrect=only_incorrect, order_by_confidence=True, show_top_k=k)
                return report, report_to_html(report.snippets)

            def host_path(only_incorrect, k):
                contexts, shown, everything = VR.report(list(model.predict(iter(data), nn_, dev, False)), only_incorrect, True, k)
                return (contexts, shown, everything), report_to_html(contexts)

            r = {"samples": n, "top_k": args.top_k, "repeats": args.repeats, "device": torch.cuda.get_device_name(0)}
            device_path(True, args.top_k), host_path(True, args.top_k)  # warm-up
            for name, only_incorrect, k in (("filtered_top_k", True, args.top_k), ("everything_shown", False, 0)):
                td, (report, page_d) = _timed(lambda: device_path(only_incorrect, k), args.repeats)
                th, ((contexts, shown, everything), page_h) = _timed(lambda: host_path(only_incorrect, k), args.repeats)
                assert report.selected.tolist() == shown and page_d == page_h  # the two paths write the same page
                r[name] = {"device_path": td, "host_path": th, "shown": len(shown), "scanned": report.num_scanned,
                           "wrong": int(report.is_wrong.sum()), "host_over_device_medians": round(th["median_s"] / td["median_s"], 2)}

            # the kernels alone
            with torch.no_grad(), model._tensorize_all_location_rewrites():
                extend = lambda layout, points, d: R.report_indices(layout, points)[0]
                mb, _ = next(iter(Bt.prediction_minibatches(model, ((x, None) for x in data[:50]), dev, False, extend, lambda tag: None)))
                flat = Bt.flat_prediction_output(nn_, mb)
            ix = mb["selfsup"]
            dev_ix = dict(zip(hip_ops.REPORT_INDEX_FIELDS, Bt.to_device_i32([getattr(ix, f) for f in hip_ops.REPORT_INDEX_FIELDS], dev)))
            r["summarize_kernel"] = {"ms": _kernel_ms(lambda: hip_ops.report_summarize(flat, dev_ix)), "samples": int(ix.nobug_idx.shape[0]),
                                     "rewrites": int(ix.rw_idx.shape[0]), "groups": int(ix.grp_loc.shape[0]), "flat_size": int(flat.shape[0])}
            keys, keep = torch.from_numpy(report.prediction_logprob).to(dev), torch.from_numpy(report.is_wrong.astype(np.int32)).to(dev)
            big = torch.from_numpy(np.random.default_rng(0).normal(size=2 ** 17)).to(dev)
            lib = hip_ops.load_library()

            def order(k_, m_):
                out, cnt = torch.empty(k_.shape[0], dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
                return lambda: lib.bl_report_order(k_.data_ptr(), m_.data_ptr(), k_.shape[0], args.top_k, 1, out.data_ptr(), cnt.data_ptr(), None)

            r["order_kernel_ms"] = {str(n): _kernel_ms(order(keys, keep)), str(2 ** 17): _kernel_ms(order(big, torch.ones(2 ** 17, dtype=torch.int32, device=dev)), 3)}
            print(json.dumps(r), flush=True)
            results.append(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"results": results}, f, indent=1)


if __name__ == "__main__":
    main()
