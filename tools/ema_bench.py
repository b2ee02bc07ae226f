#!/usr/bin/env python
"""What weight averaging costs a training step, on one GPU.

    python tools/ema_bench.py [--steps K] [--rounds R] [--warmup W] [--out FILE]

The workload is bench.py's default gnn-mlp configuration (64 graphs of 2 000 nodes / 10 000 messages, 16 edge types, hidden 128,
8 layers, dropout 0.2, 40 candidate locations; the same resident minibatch, the same step: restore the parameters, forward,
backward, fused clip + Adam, on the trainer's step stream).  Reported:
  * the step time with averaging off (bit for bit the default step: bl_adam_clip_step) and on (bl_adam_clip_step_ema, decay
    0.999), INTERLEAVED -- R rounds of K steps each, off then on, the median over the rounds of each -- so that clock and thermal
    drift hit both alike;
  * the two optimiser kernels alone at the model's parameter count (HIP events around 200 calls each, outside the step), with
    the bytes they move: 28 and 36 per parameter;
  * one `averaged_parameters()` enter + exit (two buffer exchanges, two pack invalidations; host time with a synchronisation,
    and the exchange kernel alone);
  * the calls into the library per step, off and on (averaging adds none).
No bar is fixed.  Prints one JSON line.
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

from buglab.models import hip_ops  # noqa: E402


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("ema_bench: no ROCm GPU visible; nothing is timed without one")
    from buglab.data.collate import collate_samples, to_device
    from buglab.data.synthetic import make_samples
    from buglab.models.gnn import build_gnn_mlp_module
    from buglab.runtime.optim import FlatAdam

    device = torch.device("cuda")
    hip_ops.load_library()
    hip_ops.use_step_stream(device)
    torch.manual_seed(0)
    mb = to_device(collate_samples(make_samples(64, seed=1000, num_nodes=2000, num_messages=10000, num_edge_types=16), 16), device)
    module = build_gnn_mlp_module(128, 8, 16, dropout_rate=0.2, dropout_base_seed=0, embedder_dropout_rate=0.0).to(device).train()
    opt = FlatAdam(module.parameters())
    start_params = opt.flat_param.clone()
    opt.enable_averaging(0.999)
    average = opt.ema  # "off" takes the buffer away: FlatAdam then calls exactly what it calls without averaging

    def step():
        opt.zero_grad()
        opt.flat_param.copy_(start_params)
        hip_ops.invalidate_weight_packs()
        loss = module(**mb)
        loss.backward()
        opt.step()
        return loss

    def run(on, steps):
        opt.ema = average if on else None
        torch.cuda.synchronize()
        calls, t0 = hip_ops.CALL_COUNT, time.perf_counter()
        for _ in range(steps):
            loss = step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3, (hip_ops.CALL_COUNT - calls) / steps, float(loss.detach())

    for on in (False, True):
        run(on, args.warmup)
    off_rows, on_rows = [], []
    for _ in range(args.rounds):
        off_rows.append(run(False, args.steps))
        on_rows.append(run(True, args.steps))
    opt.ema = average

    def entry_ms(fn, launches=200):
        fn()
        torch.cuda.synchronize()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(launches):
            fn()
        stop.record()
        torch.cuda.synchronize()
        return round(start.elapsed_time(stop) / launches, 4)

    # the optimiser kernels alone, on buffers of the model's parameter count (zero gradient: values stay finite for any number of calls)
    n = opt.numel
    bufs = [torch.zeros(n, device=device) for _ in range(5)]
    sqn = torch.zeros(1, device=device)
    adam = entry_ms(lambda: hip_ops.adam_clip_step(bufs[0], bufs[1], bufs[2], bufs[3], sqn, step=5))
    adam_ema = entry_ms(lambda: hip_ops.adam_clip_step_ema(bufs[0], bufs[1], bufs[2], bufs[3], bufs[4], sqn, one_minus_decay=0.001, step=5))
    swap = entry_ms(lambda: hip_ops.swap_buffers(bufs[0], bufs[4]))

    def enter_exit():
        with opt.averaged_parameters():
            pass

    enter_exit()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(50):
        enter_exit()
    torch.cuda.synchronize()
    enter_exit_ms = (time.perf_counter() - t0) / 50 * 1e3

    med = lambda rows, k: statistics.median(r[k] for r in rows)
    spread = lambda rows: {"median": round(med(rows, 0), 3), "min": round(min(r[0] for r in rows), 3), "max": round(max(r[0] for r in rows), 3)}
    result = {
        "bench": "ema", "parameters": n, "steps_per_round": args.steps, "rounds": args.rounds,
        "step_ms_off": spread(off_rows), "step_ms_on": spread(on_rows), "step_ms_delta": round(med(on_rows, 0) - med(off_rows, 0), 3),
        "library_calls_per_step": {"off": med(off_rows, 1), "on": med(on_rows, 1)},
        "adam_clip_step_ms": adam, "adam_clip_step_ema_ms": adam_ema, "kernel_ms_delta": round(adam_ema - adam, 4),
        "bytes_per_call": {"adam_clip_step": 28 * n, "adam_clip_step_ema": 36 * n, "swap_f32": 16 * n},
        "swap_f32_ms": swap, "averaged_parameters_enter_exit_ms": round(enter_exit_ms, 4),
        "loss": {"off": off_rows[-1][2], "on": on_rows[-1][2]},
    }
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
