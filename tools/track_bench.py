#!/usr/bin/env python
"""What tracking the warnings of two scans costs on one GPU (buglab/models/track.py; csrc/bl_track.hip).

    python tools/track_bench.py [--shapes ROWS,D ...] [--repeats K] [--twin-max ROWS] [--min-similarity S] [--out FILE]

Input, per (ROWS, D): an old scan of ROWS rows in 50 clusters (noise 0.3); the new scan keeps 90 % of them with a little more
noise (0.05), in another order, and adds 10 % fresh rows of the same clusters -- most warnings persist, some are gone, some are
new.  Both sides are quantised once, outside the timed part.  Timing, after a warm-up, in windows bracketed by device
synchronisations that hold as many runs as fill 50 ms; median of K windows with the least and the greatest, per run:
  * device: the whole matching from a fresh state -- `track_match` calls of 16 rounds until the status says it has ended, with
    the four status words copied back per call; the matches per round come from a further, untimed run in calls of ONE round;
  * the twin `_track.match_host` (up to --twin-max rows a side: it orders ALL admissible pairs), whose matching and rounds must
    be the same bytes;
  * a plain torch route on the device: rounds of blockwise fp32 `mm` of the normalised rows, masked with the open rows and the
    floor, `max` along both axes, the mutual pairs matched, one `.item()` per round to see the end.  fp32 cosines: it may part
    ways with the int8 images at a near tie, so the number of equal matches is reported, not asserted;
  * for scale, `similar_search` (16 candidates) of the new rows in the old ones at the same sizes: one directional top-k.
The ratios are reported whichever way they fall.  Prints one JSON line.
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

from buglab.models import _track as T  # noqa: E402
from buglab.models import hip_ops  # noqa: E402

DEV = "cuda"


def _timed(fn, repeats, window_ms=50.0):
    """median, least and greatest time of one call; a timed window holds as many calls as fill `window_ms` (sized on a first,
    warm window), because a single sub-millisecond call measures the clock and the scheduler as much as the work"""
    def window(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / calls, out

    fn()  # warm-up
    once, out = window(1)
    calls = max(1, min(1000, int(window_ms * 1e-3 / max(once, 1e-6))))
    times = []
    for _ in range(repeats):
        t, out = window(calls)
        times.append(t)
    return {"median_ms": round(1e3 * statistics.median(times), 3), "min_ms": round(1e3 * min(times), 3),
            "max_ms": round(1e3 * max(times), 3), "calls_per_window": calls}, out


def two_scans(rows, D, seed=0, clusters=50, dropped=0.1, fresh=0.1):
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((clusters, D))
    old = centres[rng.integers(0, clusters, size=rows)] + 0.3 * rng.standard_normal((rows, D))
    kept = rng.permutation(rows)[:rows - int(dropped * rows)]
    new = np.concatenate([old[kept] + 0.05 * rng.standard_normal((kept.shape[0], D)),
                          centres[rng.integers(0, clusters, size=int(fresh * rows))] + 0.3 * rng.standard_normal((int(fresh * rows), D))])
    return old.astype(np.float32), new.astype(np.float32)


def _images(x, mean):
    d_x = torch.from_numpy(x).to(DEV)
    c, q, sumsq, r = hip_ops.similar_quantize(d_x, mean)
    return c, q, r, hip_ops.review_norms(q)


def _fresh(L, N):
    return (torch.full((L,), -1, dtype=torch.int32, device=DEV), torch.full((N,), -1, dtype=torch.int32, device=DEV),
            torch.zeros(N, dtype=torch.float64, device=DEV))


def _device_match(q_old, n_old, q_new, n_new, floor, workspace, slices, max_rounds=16, per_round=None):
    state = _fresh(q_old.shape[0], q_new.shape[0])
    rounds = 0
    while True:
        status = hip_ops.track_match(q_old, n_old, q_new, n_new, floor, *state, max_rounds=max_rounds, slices=slices, workspace=workspace).cpu()
        rounds += int(status[0])
        if per_round is not None and int(status[1]):
            per_round.append(int(status[1]))
        if int(status[2]):
            return state, rounds


def _torch_match(u_old, u_new, cos_floor, block=8192):
    L, N = u_old.shape[0], u_new.shape[0]
    m_old = torch.full((L,), -1, dtype=torch.int64, device=DEV)
    m_new = torch.full((N,), -1, dtype=torch.int64, device=DEV)
    ninf = torch.full((), float("-inf"), dtype=torch.float32, device=DEV)
    rounds = 0
    while True:
        open_old, open_new = m_old < 0, m_new < 0
        arg_old = torch.full((L,), -1, dtype=torch.int64, device=DEV)
        best_new = torch.full((N,), float("-inf"), dtype=torch.float32, device=DEV)
        arg_new = torch.full((N,), -1, dtype=torch.int64, device=DEV)
        for i0 in range(0, L, block):
            i1 = min(i0 + block, L)
            s = torch.mm(u_old[i0:i1], u_new.T)
            s = torch.where(open_old[i0:i1, None] & open_new[None, :] & (s >= cos_floor), s, ninf)
            v, j = s.max(dim=1)
            arg_old[i0:i1] = torch.where(v > ninf, j, arg_old[i0:i1])
            v, i = s.max(dim=0)
            take = v > best_new  # strict: the lower old index among equals
            best_new, arg_new = torch.where(take, v, best_new), torch.where(take, i + i0, arg_new)
        j = torch.nonzero(arg_new >= 0).reshape(-1)
        j = j[arg_old[arg_new[j]] == j]
        if j.numel() == 0:  # the one synchronisation of a round
            return m_old, m_new, rounds
        m_old[arg_new[j]], m_new[j] = j, arg_new[j]
        rounds += 1


def measure(rows, D, repeats, with_twin, min_similarity):
    x_old, x_new = two_scans(rows, D)
    zero = torch.zeros(D, dtype=torch.float32, device=DEV)
    c_old, q_old, r_old, n_old = _images(x_old, zero)
    c_new, q_new, r_new, n_new = _images(x_new, zero)
    L, N, floor = x_old.shape[0], x_new.shape[0], T.floor_of(min_similarity)
    slices = hip_ops.track_slices(min(L, N), max(L, N))
    ws = torch.empty((int(hip_ops.load_library().bl_track_match_workspace_bytes(L, N, slices)) + 7) // 8, dtype=torch.float64, device=DEV)
    run = {"L": L, "N": N, "D": D, "min_similarity": min_similarity, "slices": slices, "workspace_mb": round(ws.numel() * 8 / 2 ** 20, 1)}
    run["device"], (state, rounds) = _timed(lambda: _device_match(q_old, n_old, q_new, n_new, floor, ws, slices), repeats)
    got = [t.cpu().numpy() for t in state]
    run["rounds"], run["matched"] = rounds, int((got[1] >= 0).sum())
    per_round = []
    _device_match(q_old, n_old, q_new, n_new, floor, ws, slices, max_rounds=1, per_round=per_round)
    run["matches_per_round"] = per_round
    u_old = c_old / c_old.norm(dim=1, keepdim=True).clamp_min(1e-30)
    u_new = c_new / c_new.norm(dim=1, keepdim=True).clamp_min(1e-30)
    run["torch"], (t_old, t_new, t_rounds) = _timed(lambda: _torch_match(u_old, u_new, float(min_similarity)), repeats)
    run["torch_rounds"] = t_rounds
    run["torch_over_device"] = round(run["torch"]["median_ms"] / run["device"]["median_ms"], 2)
    run["torch_same_matches"] = round(float((t_new.cpu().numpy() == got[1]).mean()), 4)  # fp32 against int8 images
    run["similar_search_16"], _ = _timed(lambda: hip_ops.similar_search(q_new, r_new, q_old, r_old, 16), repeats)
    if with_twin:
        h = [t.cpu().numpy() for t in (q_old, n_old, q_new, n_new)]
        t0 = time.perf_counter()
        want = T.match_host(*h, floor)
        run["twin_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
        run["twin_over_device"] = round(run["twin_ms"] / run["device"]["median_ms"], 1)
        run["outputs_agree"] = all(a.tobytes() == b.tobytes() for a, b in zip(got, want[:3])) and want[3] == rounds
    return run


def _shape(text):
    rows, D = (int(v) for v in text.split(","))
    return rows, D


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--shapes", type=_shape, nargs="*", default=[(10_000, 128), (10_000, 512), (100_000, 128), (100_000, 512)])
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--twin-max", type=int, default=10_000, help="largest ROWS the NumPy twin is timed on")
    p.add_argument("--min-similarity", type=float, default=0.9)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("track_bench: no ROCm GPU visible")
    result = {"bench": "track", "repeats": args.repeats, "device": torch.cuda.get_device_name(0), "match": []}
    for rows, D in args.shapes:
        entry = measure(rows, D, args.repeats, rows <= args.twin_max, args.min_similarity)
        print(json.dumps(entry), file=sys.stderr, flush=True)  # progress: the result line comes last, on stdout
        result["match"].append(entry)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w", encoding="utf-8") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
