#!/usr/bin/env python
"""What FDR-controlled warnings cost on one GPU (buglab/models/fdr.py; csrc/bl_fdr.hip), device against the NumPy twin.

    python tools/fdr_bench.py [--samples N] [--reference N] [--repeats K] [--fdr Q] [--out FILE]

Scores and reference are standard normal fp32 draws, a fifth of the scores shifted down by 3 (the discoveries).  After a
warm-up, bracketed by device synchronisations, median of K runs:
  * device = one bl_fdr_counts call over all N scores (nobug_idx the identity), one bl_fdr_bh, and the copy back of
    [q-values | counts | flags | cutoff]; the two entry points are also timed apart with HIP events;
  * twin = `counts_host` + `bh_host` on the same arrays.  The two must give the same bytes;
  * bl_fdr_counts on one predict minibatch of 50 samples (HIP events around 20 launches): what a run pays per minibatch;
  * bl_fdr_bh on the contended layouts: every count equal (one bin), and every count n_ref (the top bin, kept in registers);
    and on the same counts scaled to 16000 bins (the LDS table) and to 16001 (global adds): the two sides of that switch.
Prints one JSON line.
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

from buglab.models import _fdr as F  # noqa: E402
from buglab.models import hip_ops  # noqa: E402


def _timed(fn, repeats):
    times, out = [], None
    fn()  # warm-up
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return {"median_ms": round(1e3 * statistics.median(times), 4), "min_ms": round(1e3 * min(times), 4),
            "max_ms": round(1e3 * max(times), 4)}, out


def _kernel_ms(fn, repeats, launches=20):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(launches):
            fn()
        stop.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(stop) / launches)
    return round(statistics.median(times), 4)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--samples", type=int, default=1_000_000)
    p.add_argument("--reference", type=int, default=100_000)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--fdr", type=float, default=0.1)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fdr_bench: no ROCm GPU visible")
    N, n_ref, q, dev = args.samples, args.reference, args.fdr, torch.device("cuda")
    rng = np.random.default_rng(0)
    ref = np.sort(rng.standard_normal(n_ref).astype(np.float32))
    scores = rng.standard_normal(N).astype(np.float32)
    scores[:N // 5] -= np.float32(3.0)
    identity = np.arange(N, dtype=np.int32)
    d_ref, d_scores, d_identity = (torch.from_numpy(a).to(dev) for a in (ref, scores, identity))
    out_score = torch.empty(N, dtype=torch.float32, device=dev)
    out_count = torch.empty(N, dtype=torch.int32, device=dev)
    workspace = torch.empty(hip_ops.fdr_bh_workspace_bytes(n_ref), dtype=torch.uint8, device=dev)

    def device_run():
        hip_ops.fdr_counts(d_scores, d_identity, d_ref, out_score, out_count, 0)
        cutoff, flag, qv, _ = hip_ops.fdr_bh(out_count, n_ref, q, workspace)
        return torch.cat([qv.view(torch.int32), out_count, flag, cutoff]).cpu()

    def twin_run():
        _, count = F.counts_host(scores, identity, ref)
        return (count,) + F.bh_host(count, n_ref, q)

    device, blob = _timed(device_run, args.repeats)
    twin, (count, cutoff, flag, qv, _) = _timed(twin_run, args.repeats)
    agree = (blob[:2 * N].view(torch.float64).numpy().tobytes() == qv.tobytes() and blob[2 * N:3 * N].numpy().tobytes() == count.tobytes()
             and blob[3 * N:4 * N].numpy().tobytes() == flag.tobytes() and blob[4 * N:].numpy().tolist() == cutoff.tolist())

    B = 50
    mb_idx = d_identity[:B].contiguous()
    result = {
        "bench": "fdr", "samples": N, "reference": n_ref, "fdr": q, "repeats": args.repeats, "device": torch.cuda.get_device_name(0),
        "flagged": int(cutoff[1]), "device_run": device, "twin_run": twin,
        "twin_over_device": round(twin["median_ms"] / device["median_ms"], 1), "outputs_agree": bool(agree),
        "counts_kernel_ms": _kernel_ms(lambda: hip_ops.fdr_counts(d_scores, d_identity, d_ref, out_score, out_count, 0), args.repeats),
        "bh_ms": _kernel_ms(lambda: hip_ops.fdr_bh(out_count, n_ref, q, workspace), args.repeats),
        "counts_one_minibatch_of_50_ms": _kernel_ms(lambda: hip_ops.fdr_counts(d_scores, mb_idx, d_ref, out_score, out_count, 0), args.repeats),
    }
    for name, value in (("one_bin", n_ref // 2), ("top_bin", n_ref)):
        same = torch.full((N,), value, dtype=torch.int32, device=dev)
        result[f"bh_{name}_ms"] = _kernel_ms(lambda: hip_ops.fdr_bh(same, n_ref, q, workspace), args.repeats)
    # the same distribution of counts on either side of the switch from the LDS table (16000 bins) to global adds (16001)
    for bins in (1024, 16000, 16001):
        small = torch.from_numpy((count.astype(np.int64) * bins // (n_ref + 1)).astype(np.int32)).to(dev)
        result[f"bh_{bins}_bins_ms"] = _kernel_ms(lambda: hip_ops.fdr_bh(small, bins - 1, q, workspace), args.repeats)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w", encoding="utf-8") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
