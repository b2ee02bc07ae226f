#!/usr/bin/env python
"""What warning grouping costs on one GPU and how sharp its integer filter is (buglab/models/group.py; csrc/bl_group.hip).

    python tools/group_bench.py [--rows N ...] [--dim 128] [--similarity 0.9] [--groups 4] [--group-size 2000] [--repeats K]
                                [--twin-max N] [--torch-max N] [--one-group N] [--out FILE]

Input, per N: --groups clusters of --group-size rows each among standard normal rows that resemble nothing.  A cluster is a
centre plus noise x standard normal: the even ones with noise 0.18 (cosines of about 0.97: one fully linked group at 0.9), the
odd ones with noise 0.33 (cosines of about 0.9: the borderline, where the filter passes pairs that the re-score rejects).  All
rows share an offset of 3 standard deviations per column, which the centring removes.  The largest N defaults to the cap,
BL_GROUP_MAX_N.
Timing, after a warm-up, bracketed by device synchronisations, median of K runs:
  * device = quantise (centred in place), row l1, link, labels, the copy back of [label | degree | counters]; the link kernel
    is also timed alone with HIP events, for several numbers of slices;
  * twin = `_group.group_rows_host` on the same rows (up to --twin-max rows); labels, degrees and counters must be the same bytes;
  * torch = blockwise fp32 `torch.mm` of the normalised centred rows, a threshold, the edges gathered with `nonzero`, then
    minimum-label propagation with pointer jumping until nothing changes (up to --torch-max rows).
The case that is slow by construction: --one-group N rows of ONE tight cluster, not centred (their mean is the centre): one
group, every pair re-scored and hooked.
Reports candidates per edge.  Prints one JSON line.
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

from buglab.models import _group as G  # noqa: E402
from buglab.models import _similar as S  # noqa: E402
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


def _clustered(N, D, groups, group_size, seed=0, offset=True):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, D))
    size = min(group_size, N // max(groups, 1))
    members = rng.permutation(N)[:groups * size].reshape(groups, size) if size else np.zeros((0, 0), np.int64)
    for g in range(members.shape[0]):
        x[members[g]] = rng.standard_normal(D) + (0.33 if g % 2 else 0.18) * rng.standard_normal((size, D))
    return (x + (3.0 * rng.standard_normal(D) if offset else 0.0)).astype(np.float32)


def _torch_groups(d_rows, d_mean, similarity, block=4096):
    c = d_rows - d_mean
    u = c / c.norm(dim=1, keepdim=True).clamp_min(1e-30)
    N = u.shape[0]
    src, dst = [], []
    for i0 in range(0, N, block):
        hit = torch.mm(u[i0:i0 + block], u[i0:].T) >= similarity
        ii, jj = torch.nonzero(torch.triu(hit, diagonal=1), as_tuple=True)
        src.append(ii + i0), dst.append(jj + i0)
    src, dst = torch.cat(src), torch.cat(dst)
    label = torch.arange(N, device=u.device)
    while True:
        new = label.clone()
        new.scatter_reduce_(0, dst, label[src], "amin")
        new.scatter_reduce_(0, src, label[dst], "amin")
        new = new[new]  # pointer jumping
        if bool((new == label).all()):
            return label, int(src.shape[0])
        label = new


def _measure(x, similarity, repeats, with_twin, with_torch, slices_sweep, center=True):
    dev = torch.device("cuda")
    N, D = x.shape
    mean = S.column_mean(x) if center else np.zeros(x.shape[1], np.float32)
    d_x, d_mean = torch.from_numpy(x).to(dev), torch.from_numpy(mean).to(dev)

    def device_run():
        c, q, sumsq, r = hip_ops.similar_quantize(d_x, d_mean)
        parent, degree, counters = hip_ops.group_link(c, q, sumsq, r, hip_ops.group_row_l1(q), similarity)
        return torch.cat([hip_ops.group_labels(parent), degree, counters.view(torch.int32)]).cpu().numpy()

    run = {"N": N, "D": D, "similarity": similarity, "slices": hip_ops.group_link_slices(N)}
    run["device_run"], blob = _timed(device_run, repeats)
    label, degree, counters = blob[:N], blob[N:2 * N], blob[2 * N:].view(np.int64)
    run["num_candidates"], run["num_edges"] = int(counters[0]), int(counters[1])
    run["candidates_per_edge"] = round(counters[0] / max(int(counters[1]), 1), 4)
    sizes = np.bincount(label)
    run["num_groups"], run["largest_group"] = int((sizes > 0).sum()), int(sizes.max())
    c, q, sumsq, r = hip_ops.similar_quantize(d_x, d_mean)
    l1 = hip_ops.group_row_l1(q)
    run["quantize_ms"] = _kernel_ms(lambda: hip_ops.similar_quantize(d_x, d_mean), repeats)
    run["row_l1_ms"] = _kernel_ms(lambda: hip_ops.group_row_l1(q), repeats)
    run["link_ms"] = _kernel_ms(lambda: hip_ops.group_link(c, q, sumsq, r, l1, similarity), repeats)
    run["link_ms_by_slices"] = {str(s): _kernel_ms(lambda: hip_ops.group_link(c, q, sumsq, r, l1, similarity, s), repeats) for s in slices_sweep}
    parent = hip_ops.group_link(c, q, sumsq, r, l1, similarity)[0]
    run["labels_ms"] = _kernel_ms(lambda: hip_ops.group_labels(parent), repeats)
    run["int8_tops"] = round(N * N * ((D + 63) // 64 * 64) / (run["link_ms"] * 1e-3) / 1e12, 2)  # 2 x N^2 / 2 x Dp
    if with_torch:
        run["torch_mm_label_propagation"], (t_label, t_edges) = _timed(lambda: _torch_groups(d_x, d_mean, similarity), max(repeats // 2, 1))
        run["torch_over_device"] = round(run["torch_mm_label_propagation"]["median_ms"] / run["device_run"]["median_ms"], 2)
        run["torch_edges"] = t_edges  # fp32 cosines: pairs at the threshold may differ from the exact join's
        run["torch_same_partition"] = bool((t_label.cpu().numpy() == label).all())
    if with_twin:
        t0 = time.perf_counter()
        t_label, t_degree, nc, ne, _, _ = G.group_rows_host(x, mean, similarity)
        run["twin_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
        run["twin_over_device"] = round(run["twin_ms"] / run["device_run"]["median_ms"], 1)
        run["outputs_agree"] = bool(t_label.tobytes() == label.tobytes() and t_degree.tobytes() == degree.tobytes()
                                    and (nc, ne) == (run["num_candidates"], run["num_edges"]))
    return run


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--rows", type=int, nargs="+", default=[10_000, 100_000, hip_ops.GROUP_MAX_N])
    p.add_argument("--dim", type=int, default=128)
    p.add_argument("--similarity", type=float, default=0.9)
    p.add_argument("--groups", type=int, default=4)
    p.add_argument("--group-size", type=int, default=2000)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--twin-max", type=int, default=100_000, help="largest N the NumPy twin is timed on")
    p.add_argument("--torch-max", type=int, default=100_000, help="largest N the torch baseline is timed on")
    p.add_argument("--one-group", type=int, default=10_000, help="rows of the one-group case (0: skip it)")
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("group_bench: no ROCm GPU visible")
    result = {"bench": "group", "repeats": args.repeats, "device": torch.cuda.get_device_name(0), "runs": []}
    for N in args.rows:
        x = _clustered(N, args.dim, args.groups, args.group_size)
        run = _measure(x, args.similarity, args.repeats, N <= args.twin_max, N <= args.torch_max, (1, 4, 16, 64))
        result["runs"].append(run)
        print(json.dumps(run), file=sys.stderr, flush=True)  # progress: the result line comes last, on stdout
    if args.one_group:
        N = args.one_group
        x = _clustered(N, args.dim, 1, N, offset=False)
        result["one_group"] = _measure(x, args.similarity, max(args.repeats // 2, 1), False, N <= args.torch_max, (1, 16, 64), center=False)
        print(json.dumps(result["one_group"]), file=sys.stderr, flush=True)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w", encoding="utf-8") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
