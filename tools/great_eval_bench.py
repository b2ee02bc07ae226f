#!/usr/bin/env python
"""Throughput of an evaluation run of the GREAT var-misuse model on one GPU (buglab/models/evaluategreat.py), on synthetic GREAT
records.

    python tools/great_eval_bench.py [--samples N] [--repeats K] [--min-len A] [--max-len B] [--out FILE]

The default configuration of buglab/models/traingreat.py (10 prenorm layers, 8 heads, FF 2048, D 512; random weights: the rates
depend on the shapes, not on what the model learnt), minibatches of 30, the same model, data and minibatches for both paths,
sequential collate, after a warm-up pass, bracketed by device synchronisations, median of K runs:
  * host judge:   `evaluate_great(..., on_device=False)` -- every minibatch's logits copied to the host (one synchronisation per
    minibatch) and judged by the NumPy twin; then `format()`;
  * device judge: `evaluate_great(...)` -- bl_varmisuse_predict per minibatch, the records copied back once; then `format()`;
  * the prediction head alone (HIP events around 20 calls) at B 30, L 512, D 512, next to the training head's forward.
The two reports must be the same text.  Prints one JSON line.
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

import torch  # noqa: E402

from buglab.data.synthetic_great import make_great_records  # noqa: E402
from buglab.models import hip_ops  # noqa: E402
from buglab.models.evaluategreat import evaluate_great  # noqa: E402
from buglab.models.traingreat import default_model  # noqa: E402


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


def _head_alone():
    B, L, D = 30, 512, 512
    dev = "cuda"
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B * L, D, generator=g).to(dev)
    ln_g, ln_b = torch.ones(D, device=dev), torch.zeros(D, device=dev)
    W, bias = (torch.randn(D, 2, generator=g) / D ** 0.5).to(dev), torch.zeros(2, device=dev)
    lens_att = torch.minimum(torch.randint(L // 2, L + 1, (B,), generator=g) + 1, torch.tensor(L)).to(torch.int32).to(dev)
    err = torch.where(torch.arange(B) % 2 == 0, torch.tensor(5), torch.tensor(0)).to(torch.int32).to(dev)
    cand, tgt = torch.zeros(B, L, dtype=torch.bool), torch.zeros(B, L, dtype=torch.bool)
    cand[:, 1:200:7] = True
    tgt[:, 8] = True
    cand, tgt = cand.to(dev), tgt.to(dev)
    out_d = torch.empty((hip_ops.VARMISUSE_RECORD_D, B), dtype=torch.float64, device=dev)
    out_i = torch.empty((hip_ops.VARMISUSE_RECORD_I, B), dtype=torch.int32, device=dev)
    stats = torch.zeros(hip_ops.VARMISUSE_STATS, dtype=torch.float64, device=dev)
    return {"B": B, "L": L, "D": D,
            "predict_ms": _kernel_ms(lambda: hip_ops.varmisuse_predict(x, ln_g, ln_b, W, bias, lens_att, err, cand, tgt, out_d, out_i, 0)),
            "training_forward_ms": _kernel_ms(lambda: hip_ops.varmisuse_head(x, ln_g, ln_b, W, bias, lens_att, err, cand, tgt, stats))}


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--samples", type=int, default=600)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--min-len", type=int, default=200)
    p.add_argument("--max-len", type=int, default=512)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    dev = torch.device("cuda")
    n = args.samples
    data = make_great_records(n, seed=1, min_len=args.min_len, max_len=args.max_len)
    model = default_model()
    model.compute_metadata(data)
    torch.manual_seed(1)
    nn_ = model.build_neural_module().cuda().eval()

    host_path = lambda: evaluate_great(model, nn_, data, dev, parallelize=False, on_device=False).format()
    device_path = lambda: evaluate_great(model, nn_, data, dev, parallelize=False).format()
    host_path(), device_path()  # warm-up
    th, text_h = _timed(host_path, args.repeats)
    td, text_d = _timed(device_path, args.repeats)
    r = {"samples": n, "repeats": args.repeats, "minibatch_size": 30, "lengths": [args.min_len, args.max_len],
         "device": torch.cuda.get_device_name(0), "host_judge": th, "device_judge": td,
         "host_samples_per_s": round(n / th["median_s"], 1), "device_samples_per_s": round(n / td["median_s"], 1),
         "host_over_device": round(th["median_s"] / td["median_s"], 3), "same_report": text_h == text_d, "head_alone": _head_alone()}
    print(json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(r, f, indent=1)
    assert text_h == text_d  # the two paths print the same report


if __name__ == "__main__":
    main()
