#!/usr/bin/env python
"""What the similar-bug search costs on one GPU and what its int8 stage loses (buglab/models/similar.py; csrc/bl_similar.hip).

    python tools/similar_bench.py [--index N ...] [--queries Q] [--dims D ...] [--top-k 5] [--repeats K] [--no-model] [--out FILE]

Timing, per index size N and embedding size D (rows = standard normal plus a shared offset of 3 standard deviations per
column, centred; queries = a drawn row plus 0.7 x standard normal); after a warm-up, bracketed by device synchronisations,
median of K runs:
  * device = quantise the queries, search the first 16 candidates on the int8 images, re-score in fp64, copy [dot | idx] back
    (the index's int8 image is built once, outside the timed region, as `find_similar` builds it once per run); the three
    entry points are also timed apart with HIP events, the search also for every number of index slices from 1 to 64;
  * twin = the same in NumPy (`_similar.quantize_host`, `search_host`, `rescore_host`), at index sizes up to --twin-max;
    the two must give the same bytes;
  * torch = `torch.mm` of the centred fp32 rows, a division by the norms, `torch.topk`, the copy back.
With 50 queries (one predict minibatch) the search is timed for every number of slices once more.
Recall@k of the two-stage search against exact fp64 brute force for C in {k, 8, 16}: on the synthetic rows above, and (unless
--no-model) on the site embeddings of an untrained seeded gnn-mlp over `make_report_dataset` (index: 400 samples, predicted
sites with NO_BUG left out; queries: 200 others).
Prints one JSON line.
"""
import argparse
import copy
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
    return {"median_ms": round(1e3 * statistics.median(times), 4), "min_ms": round(1e3 * min(times), 4),
            "max_ms": round(1e3 * max(times), 4)}, out


def _kernel_ms(fn, repeats, launches=10):
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


def _synthetic(N, Q, D, seed=0):
    rng = np.random.default_rng(seed)
    base = rng.standard_normal(D) * 3.0
    x = (rng.standard_normal((N, D)) + base).astype(np.float32)
    y = (x[rng.integers(0, N, Q)] + 0.7 * rng.standard_normal((Q, D))).astype(np.float32)
    mean = S.column_mean(x)
    return S.centre(x, mean), y, mean


def _exact_top(index_c, queries_c, k, block=64):
    """exact fp64 brute force on the device (fp64 GEMM), the lower index among equal cosines"""
    x = torch.from_numpy(index_c).cuda().double()
    xn = x / x.norm(dim=1, keepdim=True).clamp_min(1e-300)
    out = []
    for q0 in range(0, queries_c.shape[0], block):
        y = torch.from_numpy(queries_c[q0:q0 + block]).cuda().double()
        cos = (y / y.norm(dim=1, keepdim=True).clamp_min(1e-300)) @ xn.T
        out.append(torch.sort(cos, dim=1, descending=True, stable=True).indices[:, :k].cpu().numpy())
    return np.concatenate(out)


def _recall(index_c, queries, mean, k):
    """recall@k of the device's two-stage search against exact brute force, for C in {k, 8, 16}"""
    dev = torch.device("cuda")
    cy, qy, sy, ry = hip_ops.similar_quantize(torch.from_numpy(index_c).to(dev), torch.zeros(index_c.shape[1], device=dev))
    cx, qx, sx, rx = hip_ops.similar_quantize(torch.from_numpy(queries).to(dev), torch.from_numpy(mean).to(dev))
    valid = (sx > 0).cpu().numpy()
    exact = _exact_top(index_c, cx.cpu().numpy(), k)
    out = {}
    for C in sorted({k, 8, 16}):
        if C < k:
            continue
        cand, _ = hip_ops.similar_search(qx, rx, qy, ry, C)
        idx = hip_ops.similar_rescore(cx, cy, sy, cand, k)[0].cpu().numpy()
        hits = [len(set(exact[i]) & set(idx[i])) / min(k, index_c.shape[0]) for i in np.flatnonzero(valid)]
        out[f"C={C}"] = round(float(np.mean(hits)), 5) if hits else None
    return out, int(valid.sum())


def _model_embeddings():
    from buglab.data.synthetic import make_report_dataset
    from buglab.models import similar as T
    from buglab.models.modelregistry import load_model

    pool, data = make_report_dataset(400, seed=18), make_report_dataset(200, seed=17)
    with tempfile.TemporaryDirectory() as tmp:
        model = load_model({"modelName": "gnn-mlp", "hidden_state_size": 128, "num_layers": 4, "dropout_rate": 0.1},
                           Path(tmp) / "m.pkl.gz")[0]
        model.compute_metadata(copy.deepcopy(pool + data))
        torch.manual_seed(5)
        nn = model.build_neural_module().to("cuda")
        index = T.build_site_index(model, nn, pool, "cuda", "predicted", assume_buggy=True, parallelize=False)
        queries = T.embed_sites(model, nn, data, "cuda", "predicted", assume_buggy=True, parallelize=False)
    return index.embeddings, queries.rows, index.mean


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--index", type=int, nargs="+", default=[20_000, 200_000, 1_000_000])
    p.add_argument("--queries", type=int, default=1000)
    p.add_argument("--dims", type=int, nargs="+", default=[128, 256])
    p.add_argument("--top-k", type=int, default=5)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--twin-max", type=int, default=200_000, help="largest index the NumPy twin is timed on")
    p.add_argument("--no-model", action="store_true")
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("similar_bench: no ROCm GPU visible")
    dev, k, Q = torch.device("cuda"), args.top_k, args.queries
    result = {"bench": "similar", "queries": Q, "top_k": k, "repeats": args.repeats, "device": torch.cuda.get_device_name(0), "runs": []}
    for D in args.dims:
        for N in args.index:
            index_c, y, mean = _synthetic(N, Q, D)
            d_y, d_mean = torch.from_numpy(y).to(dev), torch.from_numpy(mean).to(dev)
            d_index = torch.from_numpy(index_c).to(dev)
            cy, qy, sy, ry = hip_ops.similar_quantize(d_index, torch.zeros(D, device=dev))
            norms = d_index.norm(dim=1)

            def device_run():
                cx, qx, sx, rx = hip_ops.similar_quantize(d_y, d_mean)
                cand, _ = hip_ops.similar_search(qx, rx, qy, ry, 16)
                idx, dot = hip_ops.similar_rescore(cx, cy, sy, cand, k)
                return torch.cat([dot.reshape(-1).view(torch.int32), idx.reshape(-1)]).cpu()

            def torch_run():
                c = d_y - d_mean
                cos = torch.mm(c, d_index.T) / norms[None, :]
                return torch.topk(cos, k, dim=1).indices.cpu()

            run = {"N": N, "D": D, "slices": hip_ops.similar_search_slices(Q, N)}
            run["device_run"], blob = _timed(device_run, args.repeats)
            run["torch_mm_topk"], t_idx = _timed(torch_run, args.repeats)
            run["torch_over_device"] = round(run["torch_mm_topk"]["median_ms"] / run["device_run"]["median_ms"], 2)
            cx, qx, sx, rx = hip_ops.similar_quantize(d_y, d_mean)
            cand, _ = hip_ops.similar_search(qx, rx, qy, ry, 16)
            run["quantize_queries_ms"] = _kernel_ms(lambda: hip_ops.similar_quantize(d_y, d_mean), args.repeats)
            run["quantize_index_ms"] = _kernel_ms(lambda: hip_ops.similar_quantize(d_index, torch.zeros(D, device=dev)), args.repeats, 3)
            run["search_ms"] = _kernel_ms(lambda: hip_ops.similar_search(qx, rx, qy, ry, 16), args.repeats)
            run["search_ms_by_slices"] = {str(S_): _kernel_ms(lambda: hip_ops.similar_search(qx, rx, qy, ry, 16, slices=S_), args.repeats)
                                          for S_ in (1, 2, 4, 8, 16, 32, 64)}
            run["rescore_ms"] = _kernel_ms(lambda: hip_ops.similar_rescore(cx, cy, sy, cand, k), args.repeats)
            run["int8_tops"] = round(2.0 * Q * N * ((D + 63) // 64 * 64) / (run["search_ms"] * 1e-3) / 1e12, 2)
            idx = blob[2 * Q * k:].numpy().reshape(Q, k)
            run["top1_agrees_with_torch"] = round(float((idx[:, 0] == t_idx[:, 0].numpy()).mean()), 4)
            if N <= args.twin_max:
                def twin_run():
                    a, b, c, d = S.quantize_host(y, mean)
                    return S.rescore_host(a, index_c, sy_h, S.search_host(b, d, qy_h, ry_h, 16)[0], k)

                _, qy_h, sy_h, ry_h = S.quantize_host(index_c, np.zeros(D, np.float32))
                run["twin_run"], (t_i, t_d) = _timed(twin_run, max(args.repeats // 2, 1))
                run["twin_over_device"] = round(run["twin_run"]["median_ms"] / run["device_run"]["median_ms"], 1)
                run["outputs_agree"] = bool(idx.tobytes() == t_i.tobytes()
                                            and blob[:2 * Q * k].view(torch.float64).numpy().tobytes() == t_d.tobytes())
            run["recall_at_k"], _ = _recall(index_c, y, mean, k)
            result["runs"].append(run)
            print(json.dumps(run), file=sys.stderr, flush=True)  # progress: the result line comes last, on stdout
            del d_index, cy, qy, sy, ry
    # few queries: how far cutting the index into slices fills the chip (one predict minibatch of 50 sites)
    result["few_queries"] = []
    for N in args.index[:2]:
        index_c, y, mean = _synthetic(N, 50, args.dims[0])
        cy, qy, sy, ry = hip_ops.similar_quantize(torch.from_numpy(index_c).to(dev), torch.zeros(args.dims[0], device=dev))
        cx, qx, sx, rx = hip_ops.similar_quantize(torch.from_numpy(y).to(dev), torch.from_numpy(mean).to(dev))
        result["few_queries"].append({"N": N, "Q": 50, "D": args.dims[0], "default_slices": hip_ops.similar_search_slices(50, N),
                                      "search_ms_by_slices": {str(S_): _kernel_ms(lambda: hip_ops.similar_search(qx, rx, qy, ry, 16, slices=S_),
                                                                                    args.repeats) for S_ in (1, 2, 4, 8, 16, 32, 64)}})
        print(json.dumps(result["few_queries"][-1]), file=sys.stderr, flush=True)
    if not args.no_model:
        index_c, rows, mean = _model_embeddings()
        recall, valid = _recall(index_c, rows, mean, k)
        result["model_embeddings"] = {"model": "gnn-mlp, hidden 128, untrained, seeded", "index": int(index_c.shape[0]),
                                      "queries": int(rows.shape[0]), "valid_queries": valid, "D": int(index_c.shape[1]), "recall_at_k": recall}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w", encoding="utf-8") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
