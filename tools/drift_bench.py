#!/usr/bin/env python
"""What the drift test costs on one GPU (buglab/models/drift.py; csrc/bl_drift.hip).

    python tools/drift_bench.py [--rows N ...] [--dim D] [--permutations R] [--repeats K] [--twin-max N] [--torch-max N] [--out FILE]

Per pooled size N (n = N / 2 reference rows, standard normal; the other half shifted by 0.05 per column), after a warm-up,
bracketed by device synchronisations, median of K runs:
  * device = `drift_between` on rows already on the device: the bandwidth, the subsets, the fused permutation sums and the one
    copy back; the three entry points are also timed apart with HIP events, the sums for every column-tile setting;
  * twin   = the same in NumPy fp64 (`_drift.drift_host`), at N up to --twin-max, one run;
  * torch  = plain fp32 on the same GPU with K materialised (mm, exp, mm against the device's own mask), at N up to --torch-max;
and the peak allocation of the device path and of the torch version (`torch.cuda.max_memory_allocated` above what was held
before).  Where the twin ran: the error of the device's and of torch's MMD2 against it, relative to S / N^2.
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

from buglab.models import _drift as Dr  # noqa: E402
from buglab.models import drift as T  # noqa: E402
from buglab.models import hip_ops  # noqa: E402


def _timed(fn, repeats, warm=True):
    times, out = [], None
    if warm:
        fn()
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return {"median_ms": round(1e3 * statistics.median(times), 3), "min_ms": round(1e3 * min(times), 3),
            "max_ms": round(1e3 * max(times), 3)}, out


def _kernel_ms(fn, repeats, launches=3):
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


def _peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - before) / 2 ** 20, 1), out


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--rows", type=int, nargs="+", default=[2_000, 8_000, 20_000, 50_000])
    p.add_argument("--dim", type=int, default=128)
    p.add_argument("--permutations", type=int, default=1000)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--twin-max", type=int, default=8_000, help="largest N the NumPy twin is timed on")
    p.add_argument("--torch-max", type=int, default=50_000, help="largest N the materialising torch version is timed on")
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("drift_bench: no ROCm GPU visible")
    dev, D, R = torch.device("cuda"), args.dim, args.permutations
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.set_float32_matmul_precision("highest")
    result = {"bench": "drift", "D": D, "permutations": R, "repeats": args.repeats, "device": torch.cuda.get_device_name(0), "runs": []}
    for N in args.rows:
        n = N // 2
        rng = np.random.default_rng(N)
        z = rng.standard_normal((N, D)).astype(np.float32)
        z[n:] += 0.05
        d_z = torch.from_numpy(z).to(dev)
        d_ref, d_new = d_z[:n], d_z[n:]
        run = {"N": N, "n": n}
        run["device_peak_MiB"], report = _peak_mib(lambda: T.drift_between(d_ref, d_new, dev, R, 0))
        run["device_run"], report = _timed(lambda: T.drift_between(d_ref, d_new, dev, R, 0), args.repeats)
        run["p_value"], run["mmd2"] = report.p_value, report.statistic
        bandwidth, rownorm = hip_ops.drift_bandwidth(d_z)
        mask = hip_ops.drift_subsets(N, n, R, 0, dev)
        run["bandwidth_ms"] = _kernel_ms(lambda: hip_ops.drift_bandwidth(d_z), args.repeats)
        run["subsets_ms"] = _kernel_ms(lambda: hip_ops.drift_subsets(N, n, R, 0, dev), args.repeats)
        shift = T.kernel_shift(1.0)
        run["sums_ms_by_col_tiles"] = {str(ct): _kernel_ms(lambda: hip_ops.drift_permutation_sums(d_z, rownorm, mask, n, bandwidth, shift, col_tiles=ct),
                                                           args.repeats, 1 if N > 20_000 else 3) for ct in (4, 8, 16)}
        sums_ms = min(run["sums_ms_by_col_tiles"].values())
        run["sums_tflops_second_product"] = round(2.0 * N * N * (R + 2) / (sums_ms * 1e-3) / 1e12, 1)  # of K A alone, one term per entry
        a = mask[:R + 1, :N].float()

        def torch_run():
            sq = (d_z * d_z).sum(dim=1)
            K = torch.exp(-(sq[:, None] + sq[None, :] - 2.0 * (d_z @ d_z.T)).clamp_min_(0.0) / float(bandwidth.cpu()[0]))
            U = K @ a.T
            rho = K.sum(dim=1)
            return torch.cat([(a.T * U).sum(dim=0), U.sum(dim=0), rho.sum()[None]]).cpu()

        if N <= args.torch_max:
            run["torch_peak_MiB"], _ = _peak_mib(torch_run)
            run["torch_materialised"], t_sums = _timed(torch_run, args.repeats)
            run["torch_over_device"] = round(run["torch_materialised"]["median_ms"] / run["device_run"]["median_ms"], 2)
        if N <= args.twin_max:
            run["twin_run"], host = _timed(lambda: Dr.drift_host(z[:n], z[n:], R, 0), 1, warm=False)
            run["twin_over_device"] = round(run["twin_run"]["median_ms"] / run["device_run"]["median_ms"], 1)
            want = np.concatenate([[host.statistic], host.null])
            masks = mask[:R + 1, :N].cpu().numpy()
            unit = Dr.permutation_sums_host(z, n, masks[:1], host.bandwidth)[2] / float(N) ** 2
            run["err_device"] = float(np.abs(np.concatenate([[report.statistic], report.null]) - want).max() / unit)
            if N <= args.torch_max:
                t = t_sums.double().numpy()
                run["err_torch"] = float(np.abs(Dr.mmd2(t[:R + 1], t[R + 1:2 * R + 2], t[2 * R + 2], n, N - n) - want).max() / unit)
            run["p_value_twin"] = host.p_value
        result["runs"].append(run)
        print(json.dumps(run), file=sys.stderr, flush=True)  # progress: the result line comes last, on stdout
        del d_z, mask, a
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w", encoding="utf-8") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
