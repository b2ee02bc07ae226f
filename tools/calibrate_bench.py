#!/usr/bin/env python
"""The calibration fit on one GPU against its NumPy twin, on the same synthetic pool.

    python tools/calibrate_bench.py [--samples N] [--repeats K] [--out FILE]

The pool is what `buglab/models/calibrate.py` collects from N validation samples: per sample 2 .. 60 location log-probabilities
(NO_BUG last) of an over-confident detector that is biased towards NO_BUG, the truth drawn from the distribution it sharpened;
for the buggy half a repair group of 2 .. 12 rewrites.  Timed, after a warm-up fit:
  * device fit: `K.fit_calibration` over hip_ops.conf_loc_stats / conf_group_stats (csrc/bl_confidence.hip), HIP events around
    the whole fit -- every Newton evaluation is one launch pair and one copy of six (three) doubles; median of K;
  * one stats evaluation alone (HIP events around 20 launches);
  * the twin's fit (`K.fit_host`, buglab/models/_calibrate.py: NumPy fp64, one Python iteration per segment): wall clock, once.
No speed bar: the twin's time on the same machine is the yardstick.  The two fits must agree.  Prints one JSON line.
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

from buglab.models import _calibrate as K  # noqa: E402
from buglab.models import hip_ops  # noqa: E402


def _log_softmax(x):
    return x - (x.max() + np.log(np.exp(x - x.max()).sum()))


def make_pools(n, seed, sharpen=3.0, shift=1.5):
    rng = np.random.default_rng(seed)

    def pool(count, lo, hi, nobug):
        vals, lens, tgt = [], [], []
        for _ in range(count):
            k = int(rng.integers(lo, hi + 1))
            logp = _log_softmax(rng.standard_normal(k))
            tgt.append(int(rng.choice(k, p=np.exp(logp))))
            z = sharpen * logp
            if nobug:
                z[-1] += shift
            vals.append(_log_softmax(z).astype(np.float32))
            lens.append(k)
        off = np.zeros(count + 1, np.int32)
        np.cumsum(lens, out=off[1:])
        return K.Pool(np.concatenate(vals), off, np.asarray(tgt, np.int32))

    return pool(n, 2, 60, True), pool(n // 2, 2, 12, False)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--samples", type=int, default=20000)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("calibrate_bench: no ROCm GPU visible; nothing is timed without one")
    dev = torch.device("cuda")
    loc, rw = make_pools(args.samples, seed=1)
    d_loc = tuple(torch.from_numpy(a).to(dev) for a in loc)
    d_rw = tuple(torch.from_numpy(a).to(dev) for a in rw)
    n, nb = int(loc.tgt.shape[0]), int(rw.tgt.shape[0])
    n_bug_free = int(np.sum(loc.tgt == np.diff(loc.off) - 1))
    evaluations = [0]

    def loc_fn(beta, bias):
        evaluations[0] += 1
        return hip_ops.conf_loc_stats(*d_loc, beta, bias).cpu().numpy()

    def group_fn(beta):
        evaluations[0] += 1
        return hip_ops.conf_group_stats(*d_rw, beta).cpu().numpy()

    device_fit = lambda: K.fit_calibration(loc_fn, n, n_bug_free, group_fn, nb)
    device_fit()  # warm-up: code objects, the allocator's blocks
    times = []
    for _ in range(args.repeats):
        evaluations[0] = 0
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        cal, details = device_fit()
        stop.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(stop))

    def kernel_ms(fn, launches=20):
        fn()
        torch.cuda.synchronize()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(launches):
            fn()
        stop.record()
        torch.cuda.synchronize()
        return round(start.elapsed_time(stop) / launches, 4)

    t0 = time.perf_counter()
    twin, twin_details = K.fit_host(loc, rw)
    twin_s = time.perf_counter() - t0
    same = (abs(cal.beta - twin.beta) <= 1e-9 and abs(cal.no_bug_bias - twin.no_bug_bias) <= 1e-9
            and abs(cal.repair_beta - twin.repair_beta) <= 1e-9 and cal.converged and twin.converged)
    result = {
        "bench": "calibrate", "samples": n, "location_entries": int(loc.vals.shape[0]), "repair_groups": nb,
        "repair_entries": int(rw.vals.shape[0]),
        "device_fit_ms": {"median": round(statistics.median(times), 3), "min": round(min(times), 3), "max": round(max(times), 3)},
        "device_stats_evaluations": evaluations[0],
        "newton_iterations": [details["localization"]["iterations"], details["repair"]["iterations"]],
        "loc_stats_launch_ms": kernel_ms(lambda: hip_ops.conf_loc_stats(*d_loc, cal.beta, cal.no_bug_bias)),
        "group_stats_launch_ms": kernel_ms(lambda: hip_ops.conf_group_stats(*d_rw, cal.repair_beta)),
        "twin_fit_s": round(twin_s, 3), "twin_over_device": round(twin_s * 1e3 / statistics.median(times), 1),
        "calibration": {"beta": cal.beta, "no_bug_bias": cal.no_bug_bias, "repair_beta": cal.repair_beta},
        "fits_agree": bool(same),
    }
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not same:
        raise SystemExit(f"calibrate_bench: the device fit {cal} and the twin's {twin} differ")


if __name__ == "__main__":
    main()
