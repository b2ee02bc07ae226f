#!/usr/bin/env python
"""The threshold-curve bootstrap on one GPU against its NumPy twin, on the same synthetic outcome words and bins.

    python tools/operating_point_bench.py [--samples N] [--replicates R] [--rounds K] [--twin-replicates R] [--out FILE]

No model: n random packed words (buglab/models/_compare.py::pack_outcomes says what they hold) and, per model, bins drawn
uniformly from 0 .. G (G: the sample passes no threshold), for M in {1, 2} and G in {64, 256, 1024}; and one shape with the
worst bin contention (every sample in bin 0 with the flags of a right warning).  Timed per shape:
  * the kernel alone: HIP events around one hip_ops.bootstrap_curve_counts call (csrc/bl_bootstrap.hip) of R replicates, no copy;
  * device: the resampling as buglab/models/operatingpoint.py runs it -- words and bins go up, the counts of every call come
    back; HIP events around all of it;
  * bl_bootstrap_counts (the scalar metrics' kernel) on the same words, n and R with K = 8 scouts, for the per-draw comparison;
  * the twin (`curve_counts_host`: NumPy, chunked over replicates): wall clock for --twin-replicates replicates, once, SCALED to
    R (its work is linear in the replicates; the line says so).
The rounds are interleaved -- every round times every shape once, after one warm-up round -- and the medians are reported.  No
speed bar: the twin's time on the same machine is the yardstick.  The two must give the same counts.  Prints one JSON line.
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

from buglab.models import _operatingpoint as P  # noqa: E402
from buglab.models import hip_ops, operatingpoint  # noqa: E402

SHAPES = [(M, G, "uniform") for M in (1, 2) for G in (64, 256, 1024)] + [(1, 64, "one_bin")]
SCALAR_SCOUTS = 8


def make_inputs(n, M, G, layout, seed):
    """`uniform`: random flags, bins uniform over 0 .. G.  `one_bin`: the worst bin contention -- every sample buggy, warned and
    right, all in bin 0, so that every lane of every add hits one of two LDS words."""
    rng = np.random.default_rng(seed)
    if layout == "one_bin":
        return np.full(n, 0x77777700 | 1, np.uint32), np.zeros((M, n), np.int16)
    words = rng.integers(0, 1 << (8 + 4 * M), size=n, dtype=np.uint64).astype(np.uint32)
    words = (words & ~np.uint32(0xFF)) | rng.integers(0, SCALAR_SCOUTS, size=n).astype(np.uint32)
    return words, rng.integers(0, G + 1, size=(M, n)).astype(np.int16)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--samples", type=int, default=100000)
    p.add_argument("--replicates", type=int, default=2000)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--twin-replicates", type=int, default=40)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("operating_point_bench: no ROCm GPU visible; nothing is timed without one")
    n, R = args.samples, args.replicates

    def timed(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        out = fn()
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop), out

    cases = []
    for M, G, layout in SHAPES:
        words, bins = make_inputs(n, M, G, layout, seed=1)
        d_words, d_bins = torch.from_numpy(words.view(np.int32)).to("cuda"), torch.from_numpy(bins).to("cuda")
        per_call = min(R, operatingpoint.replicates_per_call(M, G))
        cases.append({"M": M, "G": G, "layout": layout, "words": words, "bins": bins, "per_call": per_call, "kernel": [], "device": [], "scalar": [],
                      "run_kernel": (lambda w=d_words, b=d_bins, M=M, G=G, k=per_call,
                                     o=torch.empty((per_call, P.num_columns(M, G)), dtype=torch.int32, device="cuda"):
                                     hip_ops.bootstrap_curve_counts(w, b, M, G, 0, 0, k, out=o)),
                      "run_device": (lambda w=words, b=bins, M=M, G=G: operatingpoint.curve_counts_device(w, b, M, G, 0, R, "cuda")),
                      "run_scalar": (lambda w=d_words, M=M, k=per_call,
                                     o=torch.empty((per_call, SCALAR_SCOUTS + M * (4 + 2 * SCALAR_SCOUTS)), dtype=torch.int32, device="cuda"):
                                     hip_ops.bootstrap_counts(w, M, SCALAR_SCOUTS, 0, 0, k, out=o))})
    for rnd in range(args.rounds + 1):  # round 0 warms up: the code object, the allocator's blocks
        for c in cases:
            for name in ("kernel", "device", "scalar"):
                ms, out = timed(c["run_" + name])
                if rnd:
                    c[name].append(ms)
                if name == "device":
                    c["counts"] = out

    shapes, same = [], True
    twin_R = min(R, args.twin_replicates)
    for c in cases:
        t0 = time.perf_counter()
        twin = P.curve_counts_host(c["words"], c["bins"], c["M"], c["G"], 0, 0, twin_R)
        twin_s = time.perf_counter() - t0
        agree = bool(np.array_equal(twin, c["counts"][:twin_R]))
        same = same and agree
        med = lambda v: statistics.median(v)
        kernel_ms, device_ms, scalar_ms = med(c["kernel"]), med(c["device"]), med(c["scalar"])
        draws = n * c["per_call"]
        shapes.append({
            "models": c["M"], "bins": c["G"], "layout": c["layout"], "replicates_per_call": c["per_call"],
            "kernel_ms": round(kernel_ms, 3), "kernel_min_ms": round(min(c["kernel"]), 3),
            "kernel_ns_per_draw_and_model": round(kernel_ms * 1e6 / (draws * c["M"]), 4),
            "device_ms": round(device_ms, 3), "device_min_ms": round(min(c["device"]), 3),
            "scalar_kernel_ms": round(scalar_ms, 3), "curve_over_scalar_kernel": round(kernel_ms / scalar_ms, 2),
            "twin_s": round(twin_s, 3), "twin_scaled_to_replicates_s": round(twin_s * R / twin_R, 3),
            "twin_over_device": round(twin_s * R / twin_R * 1e3 / device_ms, 1), "counts_agree": agree})
    result = {"bench": "operating_point", "samples": n, "replicates": R, "rounds": args.rounds, "scalar_scouts": SCALAR_SCOUTS,
              "twin_replicates": twin_R, "twin_note": f"the twin was timed at {twin_R} replicates and scaled linearly to {R}",
              "shapes": shapes, "counts_agree": same}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not same:
        raise SystemExit("operating_point_bench: the device's counts and the twin's differ")


if __name__ == "__main__":
    main()
