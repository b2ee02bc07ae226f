#!/usr/bin/env python
"""What the distillation term costs a training step, on one GPU.

    python tools/distill_bench.py [--steps K] [--rounds R] [--warmup W] [--out FILE]

The workload is bench.py's default gnn-mlp configuration (64 graphs of 2 000 nodes / 10 000 messages, 16 edge types, hidden 128,
8 layers, dropout 0.2, 40 candidate locations; the same resident minibatch, the same step: restore the parameters, forward,
backward, fused clip + Adam, on the trainer's step stream) with synthetic teacher arrays: a random normalised distribution over
every location segment and every repair group of the minibatch.  Reported:
  * the step time with the term off (weight 0: bit for bit the default step) and on (weight 0.5, temperature 2), INTERLEAVED --
    R rounds of K steps each, off then on, the median over the rounds of each -- so that clock and thermal drift hit both alike;
  * the two entry points' own times (HIP events around 50 calls each, outside the step): bl_distill_fwd = the segment kernel
    + the fixed-order sums, bl_distill_bwd = one elementwise kernel;
  * the calls into the library per step, off and on (the term adds two), and the sizes B, C, G, R.
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

import numpy as np  # noqa: E402
import torch  # noqa: E402

from buglab.models import hip_ops  # noqa: E402


def _log_softmax(x):
    return x - (x.max() + np.log(np.exp(x - x.max()).sum()))


def teacher_arrays(mb, seed, device):
    rng = np.random.default_rng(seed)
    cptr = mb["graph_data"]["candidate_ptr"].cpu().numpy()
    gptr, gitems = mb["repair_group_ptr"].cpu().numpy(), mb["repair_group_items"].cpu().numpy()
    B, C, R = cptr.shape[0] - 1, int(cptr[-1]), gitems.shape[0]
    tl, tr = np.zeros(C + B, np.float32), np.zeros(R, np.float32)
    for b in range(B):
        t = _log_softmax(2.0 * rng.standard_normal(cptr[b + 1] - cptr[b] + 1)).astype(np.float32)
        tl[cptr[b]:cptr[b + 1]], tl[C + b] = t[:-1], t[-1]
    for g in np.flatnonzero(np.diff(gptr)):
        tr[gitems[gptr[g]:gptr[g + 1]]] = _log_softmax(2.0 * rng.standard_normal(gptr[g + 1] - gptr[g])).astype(np.float32)
    sizes = {"B": B, "C": C, "G": int(gptr.shape[0]) - 1, "R": R, "non_empty_groups": int(np.count_nonzero(np.diff(gptr)))}
    return {"teacher_loc_logprobs": torch.from_numpy(tl).to(device), "teacher_repair_logprobs": torch.from_numpy(tr).to(device)}, sizes


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("distill_bench: no ROCm GPU visible; nothing is timed without one")
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
    teacher, sizes = teacher_arrays(mb, 5, device)

    def step():
        opt.zero_grad()
        opt.flat_param.copy_(start_params)
        hip_ops.invalidate_weight_packs()
        loss = module(**mb, **teacher)
        loss.backward()
        opt.step()
        return loss

    def run(weight, steps):
        module.set_distillation(weight, 2.0)
        torch.cuda.synchronize()
        calls, t0 = hip_ops.CALL_COUNT, time.perf_counter()
        for _ in range(steps):
            loss = step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3, (hip_ops.CALL_COUNT - calls) / steps, float(loss.detach())

    for weight in (0.0, 0.5):
        run(weight, args.warmup)
    off, on = [], []
    for _ in range(args.rounds):
        off.append(run(0.0, args.steps))
        on.append(run(0.5, args.steps))
    module.set_distillation(0.0, 1.0)

    # the entry points alone, on the step's own scores / logits sizes
    scores = torch.randn(sizes["C"], device=device) * 3
    logits = torch.randn(sizes["R"], device=device) * 3
    cptr, gptr, gitems = mb["graph_data"]["candidate_ptr"], mb["repair_group_ptr"], mb["repair_group_items"]
    delta, _ = hip_ops.distill_fwd(scores, logits, teacher["teacher_loc_logprobs"], teacher["teacher_repair_logprobs"], cptr, gptr, gitems, 2.0)
    g_kl = torch.ones(2, device=device)

    def entry_ms(fn, launches=50):
        fn()
        torch.cuda.synchronize()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(launches):
            fn()
        stop.record()
        torch.cuda.synchronize()
        return round(start.elapsed_time(stop) / launches, 4)

    med = lambda rows, k: statistics.median(r[k] for r in rows)
    result = {
        "bench": "distill", **sizes, "steps_per_round": args.steps, "rounds": args.rounds,
        "step_ms_off": {"median": round(med(off, 0), 3), "min": round(min(r[0] for r in off), 3), "max": round(max(r[0] for r in off), 3)},
        "step_ms_on": {"median": round(med(on, 0), 3), "min": round(min(r[0] for r in on), 3), "max": round(max(r[0] for r in on), 3)},
        "step_ms_delta": round(med(on, 0) - med(off, 0), 3),
        "library_calls_per_step": {"off": med(off, 1), "on": med(on, 1)},
        "distill_fwd_ms": entry_ms(lambda: hip_ops.distill_fwd(scores, logits, teacher["teacher_loc_logprobs"],
                                                               teacher["teacher_repair_logprobs"], cptr, gptr, gitems, 2.0)),
        "distill_bwd_ms": entry_ms(lambda: hip_ops.distill_bwd(delta, sizes["C"], g_kl, 2.0)),
        "loss": {"off": off[-1][2], "on": on[-1][2]},
    }
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
