#!/usr/bin/env python
"""The paired bootstrap's resampling on one GPU against its NumPy twin, on the same synthetic outcome words.

    python tools/compare_bench.py [--samples N] [--replicates R] [--models M] [--scouts K] [--rounds K] [--twin-replicates R]
                                  [--out FILE]

No model: n random packed words (buglab/models/_compare.py::pack_outcomes says what they hold), as a comparison of M models
over n samples with K scouts would pack them.  Timed:
  * device: the whole resampling as buglab/models/compare.py runs it -- the words are on the device, hip_ops.bootstrap_counts
    (csrc/bl_bootstrap.hip) in calls of at most 4096 replicates, each call's counts copied back; HIP events around all of it,
    after one warm-up run; median and minimum of the rounds;
  * the kernel alone: HIP events around one call of 4096 replicates, no copy;
  * the twin (`bootstrap_counts_host`: NumPy, chunked over replicates): wall clock for --twin-replicates replicates, once,
    SCALED to R (its work is linear in the replicates; the line says so).
No speed bar: the twin's time on the same machine is the yardstick.  The two must give the same counts.  Prints one JSON line.
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

from buglab.models import _compare as C  # noqa: E402
from buglab.models import compare, hip_ops  # noqa: E402


def make_words(n, M, K, seed):
    rng = np.random.default_rng(seed)
    words = rng.integers(0, 1 << (8 + 4 * M), size=n, dtype=np.uint64).astype(np.uint32)
    return (words & ~np.uint32(0xFF)) | rng.integers(0, K, size=n).astype(np.uint32)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--samples", type=int, default=100000)
    p.add_argument("--replicates", type=int, default=10000)
    p.add_argument("--models", type=int, default=2)
    p.add_argument("--scouts", type=int, default=8)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--twin-replicates", type=int, default=500)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("compare_bench: no ROCm GPU visible; nothing is timed without one")
    n, R, M, K = args.samples, args.replicates, args.models, args.scouts
    words = make_words(n, M, K, seed=1)
    d_words = torch.from_numpy(words.view(np.int32)).to("cuda")

    def timed(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        out = fn()
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop), out

    run = lambda: compare.bootstrap_counts_device(words, M, K, 0, R, "cuda")
    run()  # warm-up: the code object, the allocator's blocks
    rounds = [timed(run) for _ in range(args.rounds)]
    times = [t for t, _ in rounds]
    counts = rounds[-1][1]
    per_call = min(R, compare.REPLICATES_PER_CALL)
    buffer = torch.empty((per_call, C.num_columns(M, K)), dtype=torch.int32, device="cuda")
    kernel = [timed(lambda: hip_ops.bootstrap_counts(d_words, M, K, 0, 0, per_call, out=buffer))[0] for _ in range(args.rounds)]

    twin_R = min(R, args.twin_replicates)
    t0 = time.perf_counter()
    twin = C.bootstrap_counts_host(words, M, K, 0, 0, twin_R)
    twin_s = time.perf_counter() - t0
    same = bool(np.array_equal(twin, counts[:twin_R]))
    twin_scaled_s = twin_s * R / twin_R
    device_ms = statistics.median(times)
    result = {
        "bench": "compare", "samples": n, "replicates": R, "models": M, "scouts": K, "draws": n * R,
        "device_ms": {"median": round(device_ms, 3), "min": round(min(times), 3), "max": round(max(times), 3), "rounds": args.rounds},
        "kernel_ms_per_call": {"replicates": per_call, "median": round(statistics.median(kernel), 3), "min": round(min(kernel), 3)},
        "device_draws_per_s": round(n * R / (device_ms * 1e-3)),
        "twin_s": round(twin_s, 3), "twin_replicates": twin_R, "twin_scaled_to_replicates_s": round(twin_scaled_s, 3),
        "twin_note": f"the twin was timed at {twin_R} replicates and scaled linearly to {R}",
        "twin_over_device": round(twin_scaled_s * 1e3 / device_ms, 1), "counts_agree": same,
    }
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not same:
        raise SystemExit("compare_bench: the device's counts and the twin's differ")


if __name__ == "__main__":
    main()
