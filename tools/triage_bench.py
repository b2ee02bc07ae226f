#!/usr/bin/env python
"""What warning triage costs on one GPU (buglab/models/triage.py; csrc/bl_triage.hip).

    python tools/triage_bench.py [--rows N ...] [--dims D ...] [--repeats K] [--fit-repeats K] [--twin-fit-max CELLS] [--out FILE]

Input, per (N, D): synthetic rows whose label follows one direction plus noise (N in 10^3, 10^4, 10^5 x D in 128, 512 by default).
Timing, after one warm-up, bracketed by device synchronisations, medians:
  * stats: ONE `hip_ops.triage_newton_stats` call with the copy back of its P^2 + P + 4 doubles (what a Newton iteration costs),
    and the four launches alone with HIP events;
  * twin: `_triage.HostProblem.stats` on the same rows (standardised once, outside the timing);
  * torch: fp64 on the device over rows standardised beforehand: z = X w, p, then `X.T @ (s[:, None] * X)` and `X.T @ r`, with the
    same copy back;
  * fit: the whole default fit, 5 folds x the default grid and the final fit, on the device and -- up to --twin-fit-max cells
    (N x D; the twin takes minutes beyond) -- in the twin, median of --fit-repeats runs.
Reports the largest |H_device - H_twin| as a share of the summation bound 2 (N + 16) 2^-52 sum |terms|.  Prints one JSON line.
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

from buglab.models import _triage as R  # noqa: E402
from buglab.models import hip_ops  # noqa: E402
from buglab.models import triage as T  # noqa: E402


def _timed(fn, repeats, sync=True):
    times, out = [], None
    fn()  # warm-up
    for _ in range(repeats):
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        if sync:
            torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return {"median_ms": round(1e3 * statistics.median(times), 3), "min_ms": round(1e3 * min(times), 3),
            "max_ms": round(1e3 * max(times), 3)}, out


def _kernel_ms(fn, repeats):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(stop))
    return round(statistics.median(times), 3)


def _rows(N, D, seed=0):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((N, D)) * rng.uniform(0.5, 2.0, size=D) + rng.standard_normal(D)).astype(np.float32)
    lp = np.log(rng.uniform(0.01, 1.0, size=N)).astype(np.float32)
    direction = rng.standard_normal(D) / np.sqrt(D)
    y = (x.astype(np.float64) - x.mean(axis=0)) @ direction + rng.standard_normal(N) > 0.0
    return x, lp, y


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, nargs="+", default=[1000, 10000, 100000])
    ap.add_argument("--dims", type=int, nargs="+", default=[128, 512])
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--fit-repeats", type=int, default=5)
    ap.add_argument("--twin-fit-max", type=int, default=10000 * 128, help="The twin's whole fit is timed up to this many cells (N x D).")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    l2 = 1.0
    cases = []
    for D in args.dims:
        for N in args.rows:
            x, lp, y = _rows(N, D)
            shift, scale = R.standardise(x, lp)
            w = np.random.default_rng(1).standard_normal(D + 2) / np.sqrt(D + 2)
            P = D + 2
            case = {"N": N, "D": D, "slices": hip_ops.triage_slices(N)[0], "workspace_mb": round(hip_ops.triage_workspace_bytes(N, D) / 2 ** 20, 1)}

            problem = T.DeviceProblem(x, lp, y, shift, scale, dev)
            d_w = torch.from_numpy(w).to(dev)
            launch = lambda: hip_ops.triage_newton_stats(problem.x, problem.logprob, problem.shift, problem.scale, d_w, problem.y, None, l2,
                                                         workspace=problem.workspace, out=problem.out)
            case["stats_device"], st_dev = _timed(lambda: problem.stats(w, None, l2), args.repeats)
            case["stats_kernels_ms"] = _kernel_ms(launch, args.repeats)

            host = R.HostProblem(x, lp, y, shift, scale)
            case["stats_twin"], (st_twin, (abs_h, _, _)) = _timed(lambda: host.stats(w, None, l2, with_abs=True), 3 if N * D > 10 ** 7 else args.repeats,
                                                                  sync=False)
            bound = 2.0 * (N + 16) * 2.0 ** -52 * abs_h
            case["h_error_over_bound"] = float((np.abs(st_dev.H - st_twin.H) / bound).max())
            case["h_symmetric"] = bool((st_dev.H == st_dev.H.T).all())

            X = torch.from_numpy(host.phi).to(dev)
            d_y = torch.from_numpy(y.astype(np.float64)).to(dev)
            ridge = torch.full((P,), l2, dtype=torch.float64, device=dev)
            ridge[-1] = 0.0

            def torch_route():
                z = X @ d_w
                p = torch.sigmoid(z)
                s = p * (1.0 - p)
                H = X.T @ (s[:, None] * X) + torch.diag(ridge)
                g = X.T @ (p - d_y) + ridge * d_w
                L = (torch.nn.functional.softplus(z) - d_y * z).sum()
                return torch.cat([H.reshape(-1), g, L[None]]).cpu()

            case["stats_torch_fp64"], _ = _timed(torch_route, args.repeats)
            del X

            case["fit_device"], fit_dev = _timed(lambda: T.fit_triage_embeddings(x, lp, y, device=dev), args.fit_repeats)
            case["fit_device_newton_iterations"] = fit_dev.report["newton_iterations"]
            case["fit_l2"] = fit_dev.model.l2
            if N * D <= args.twin_fit_max:
                case["fit_twin"], fit_host = _timed(lambda: T.fit_triage_embeddings(x, lp, y, host=True), args.fit_repeats, sync=False)
                case["fit_same_l2"] = bool(fit_host.model.l2 == fit_dev.model.l2)
                case["fit_device_faster"] = bool(case["fit_device"]["median_ms"] < case["fit_twin"]["median_ms"])
            cases.append(case)
            print(json.dumps(case), file=sys.stderr, flush=True)
    line = json.dumps({"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "fit_repeats": args.fit_repeats, "cases": cases})
    print(line)
    if args.out:
        with open(args.out, "w", encoding="utf-8") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
