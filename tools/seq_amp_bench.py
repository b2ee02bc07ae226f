#!/usr/bin/env python
"""Training-step time of `seq-great` at BASELINE configs[4] (hidden 256, 5 layers, 8 heads, FF 1024, 32 sequences x 512 tokens, dropout
0.1 -- bench.py's `--model seq-great` workload) with the projection GEMMs as bf16x6 (default) and as bf16x1
(hip_ops.set_seq_gemm_mode("bf16x1"), what `train.py --amp` sets for the sequence models).

Each mode: its own module / minibatch / optimiser from the same seed, `--warmup` untimed steps, then `--steps` steps between two HIP
events on the step's stream; the two modes alternate `--rounds` times and the median round is reported (the clock of a shared
package drifts over seconds).  Every step restores the start parameters, as bench.py's steps do.  Prints ONE JSON line.

    python tools/seq_amp_bench.py [--steps 20] [--warmup 5] [--rounds 3] [--graphs 32] [--seq-len 512]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "neurips21-self-supervised-bug-detection-and-repair_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--graphs", type=int, default=32)
    ap.add_argument("--seq-len", type=int, default=512)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--layers", type=int, default=5)
    ap.add_argument("--types", type=int, default=8)
    ap.add_argument("--dropout", type=float, default=0.1)
    a = ap.parse_args(argv)

    import torch

    from buglab.data.collate import to_device
    from buglab.data.synthetic import make_samples
    from buglab.models import hip_ops
    from buglab.models.layers.messagepassing import SubtokenEmbedder
    from buglab.models.seqmodel import SeqBugLabModule, SeqTensorizedSample, SequenceEncoder, collate_sequences
    from buglab.runtime.optim import FlatAdam

    if not torch.cuda.is_available():
        raise SystemExit("seq_amp_bench.py: no ROCm GPU visible")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    hip_ops.load_library()
    hip_ops.use_step_stream(device)

    def workload():
        torch.manual_seed(0)
        samples = make_samples(a.graphs, seed=1000, num_nodes=a.seq_len, num_messages=2 * a.seq_len, num_edge_types=a.types)
        mb = to_device(collate_sequences([SeqTensorizedSample(s, {}, ()) for s in samples], a.types), device)
        enc = SequenceEncoder(SubtokenEmbedder(15000, a.hidden, 6, a.dropout), a.hidden, a.types, a.layers, 8, 4 * a.hidden, a.dropout,
                              layer_type="great")
        module = SeqBugLabModule(enc, 48).to(device).train()
        module._dropout_base_seed = 0
        opt = FlatAdam(module.parameters())
        start = opt.flat_param.clone()

        def step():
            opt.zero_grad()
            opt.flat_param.copy_(start)
            hip_ops.invalidate_weight_packs()
            loss = module(**mb)
            loss.backward()
            opt.step()
            return loss

        return step

    def timed(step, mode):
        prev = hip_ops.set_seq_gemm_mode(mode)
        try:
            assert hip_ops.seq_gemm_mode() == mode
            for _ in range(a.warmup):
                step()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                loss = step()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / a.steps, float(loss.detach())
        finally:
            hip_ops.set_seq_gemm_mode(prev)

    steps = {m: workload() for m in ("bf16x6", "bf16x1")}
    ms = {m: [] for m in steps}
    loss = {}
    for _ in range(a.rounds):
        for m in steps:
            t, loss[m] = timed(steps[m], m)
            ms[m].append(t)
    med = {m: statistics.median(v) for m, v in ms.items()}
    out = {"tool": "seq_amp_bench", "model": "seq-great", "hidden": a.hidden, "layers": a.layers, "heads": 8, "ff": 4 * a.hidden,
           "sequences": a.graphs, "seq_len": a.seq_len, "dropout": a.dropout, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds,
           "step_ms": {m: round(v, 4) for m, v in med.items()}, "step_ms_rounds": {m: [round(t, 4) for t in v] for m, v in ms.items()},
           "sequences_per_s": {m: round(a.graphs / (v * 1e-3), 1) for m, v in med.items()},
           "bf16x1_over_bf16x6": round(med["bf16x1"] / med["bf16x6"], 4), "last_loss": {m: round(v, 6) for m, v in loss.items()},
           "device": torch.cuda.get_device_name(device)}
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
