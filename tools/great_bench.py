#!/usr/bin/env python
"""GREAT var-misuse model timings on one MI355X (buglab/models/greatreimplementation.py):
  * the output head (hip_ops.varmisuse_head, csrc/bl_varmisuse_head.hip) forward and backward at B 30, L 512, D 512, next to a
    torch-op restatement of the reference's head (greatreimplementation.py:143-174, :202-214, with its host reads) on the same GPU;
  * one training step (forward + backward + optimiser) of the default configuration (10 prenorm layers, 8 heads, FF 2048,
    D 512) on synthetic GREAT records, minibatch 30.
Prints which attention path the layers take and one JSON line with the numbers.
    python tools/great_bench.py [--iters N] [--steps N]"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "neurips21-self-supervised-bug-detection-and-repair_amd")]

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

HBM_BYTES_PER_S = 5.0e12  # the fraction below is reported against 5 TB/s


def _time(fn, iters):
    """Median of `iters` timings (ms) of fn() between two events."""
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def torch_head(x, g, b, W, bias, lens_att, err, cand, tgt, B, L, counters):
    """The reference's head as torch ops, with its host reads of the metric counters (`int(...)`, `float(...)`, `if num_buggy`)."""
    D = x.shape[1]
    logits = F.layer_norm(x.view(B, L, D), (D,), g, b, 1e-5) @ W + bias
    mask = torch.arange(L, device=x.device)[None, :] >= lens_att[:, None]
    logits = logits.masked_fill(mask[:, :, None], -math.inf)
    loc = logits[:, :, 0]
    ptr = torch.log_softmax(logits[:, :, 1].masked_fill(~cand, -math.inf), dim=-1)
    loc_loss = F.cross_entropy(loc, err)
    with torch.no_grad():
        ok = loc.argmax(-1) == err
        buggy = err != 0
        counters[0] += int(ok.sum())
        counters[1] += float(loc_loss) * B
        num_buggy = buggy.sum()
        counters[2] += int(num_buggy)
    if num_buggy > 0:
        lp = torch.logsumexp(ptr[buggy].masked_fill(~tgt[buggy], -math.inf), dim=-1)
        rep = -lp.mean()
        with torch.no_grad():
            counters[3] += int(tgt[buggy][torch.arange(int(num_buggy), device=x.device), ptr[buggy].argmax(-1)].sum())
        return loc_loss + rep
    return loc_loss


def head_bench(iters):
    from buglab.models import hip_ops

    B, L, D = 30, 512, 512
    dev = "cuda"
    g = torch.Generator(device="cpu").manual_seed(0)
    x = torch.randn(B * L, D, generator=g).to(dev).requires_grad_(True)
    ln_g, ln_b = torch.ones(D, device=dev, requires_grad=True), torch.zeros(D, device=dev, requires_grad=True)
    W = (torch.randn(D, 2, generator=g) / D ** 0.5).to(dev).requires_grad_(True)
    bias = torch.zeros(2, device=dev, requires_grad=True)
    lens = torch.randint(L // 2, L + 1, (B,), generator=g)
    lens_att = torch.minimum(lens + 1, torch.tensor(L)).to(torch.int32).to(dev)
    err = torch.where(torch.arange(B) % 2 == 0, torch.tensor(5), torch.tensor(0)).to(torch.int32).to(dev)
    cand = torch.zeros(B, L, dtype=torch.bool)
    cand[:, 1:200:7] = True
    tgt = torch.zeros(B, L, dtype=torch.bool)
    tgt[:, 8] = True
    cand, tgt = cand.to(dev), tgt.to(dev)
    stats = torch.zeros(hip_ops.VARMISUSE_STATS, dtype=torch.float64, device=dev)
    state = {}

    def fwd():
        state["loss"] = hip_ops.varmisuse_head(x, ln_g, ln_b, W, bias, lens_att, err, cand, tgt, stats)[0]

    def fwd_bwd():
        fwd()
        state["loss"].backward()

    for _ in range(5):
        fwd_bwd()
    t_fwd = _time(fwd, iters)
    t_bwd = _time(fwd_bwd, iters) - t_fwd  # (a hip_ops graph is backpropagated once: backward = forward + backward - forward)
    counters = [0, 0.0, 0, 0]
    err64 = err.long()
    lens64 = lens_att.long()

    def tfwd():
        state["tl"] = torch_head(x, ln_g, ln_b, W, bias, lens64, err64, cand, tgt, B, L, counters)

    def tfwd_bwd():
        tfwd()
        state["tl"].backward()

    for _ in range(3):
        tfwd_bwd()
    t_tfwd = _time(tfwd, iters)
    t_tbwd = _time(tfwd_bwd, iters) - t_tfwd
    n = B * L
    fwd_bytes = n * D * 4 + n * (8 + 8 + 2)               # x read; logits, mean / rstd written; masks read
    bwd_bytes = 2 * n * D * 4 + n * (8 + 8 + 2)           # x read, g_x written; logits, mean / rstd, masks read
    return {"B": B, "L": L, "D": D, "head_fwd_us": 1e3 * t_fwd, "head_bwd_us": 1e3 * t_bwd,
            "head_fwd_hbm_fraction": fwd_bytes / (t_fwd * 1e-3) / HBM_BYTES_PER_S,
            "head_bwd_hbm_fraction": bwd_bytes / (t_bwd * 1e-3) / HBM_BYTES_PER_S,
            "torch_head_fwd_us": 1e3 * t_tfwd, "torch_head_bwd_us": 1e3 * t_tbwd}


def step_bench(steps, warmup):
    from buglab.data.synthetic_great import make_great_records
    from buglab.models import hip_ops
    from buglab.models.traingreat import default_model
    from buglab.models.utils import LinearWarmupScheduler, optimizer

    B = 30
    model = default_model()
    recs = make_great_records(B * 4, seed=0, min_len=200, max_len=512)
    model.compute_metadata(recs)
    nn = model.build_neural_module().cuda().train()
    opt = optimizer(nn.parameters())
    opt.clip = 0.25
    LinearWarmupScheduler(opt)
    mbs = [model.finalize_minibatch({"samples": [model.tensorize(r) for r in recs[k : k + B]]}, "cuda") for k in range(0, len(recs), B)]
    layer = nn.seq_layers[0]
    mb0 = mbs[0]
    Bm, L, _ = mb0["token_ids"].shape
    fused_probs = bool(hip_ops.load_library().bl_rel_attn_probs_ok(L, layer.head_dim, layer.num_edge_types))
    path = "one-call layer (bl_great_layer)" if layer.fused_call_ok(Bm, L) else (
        "op-by-op, fused attention probabilities" if fused_probs else "op-by-op, unfused attention (bias / softmax / products)")
    print(f"attention path: {path}  (L={L}, dk={layer.head_dim}, T={layer.num_edge_types}, bl_rel_attn_probs_ok={int(fused_probs)})")
    hip_ops.use_step_stream("cuda")

    def step(mb):
        opt.zero_grad()
        loss = nn(**mb)
        loss.backward()
        opt.step()
        return loss

    for k in range(warmup):
        step(mbs[k % len(mbs)])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(steps):
        loss = step(mbs[k % len(mbs)])
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    return {"step_ms": 1e3 * dt, "step_samples_per_s": B / dt, "step_L": int(L), "attention_path": path, "last_loss": float(loss)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "great_bench needs a GPU"
    out = {"device": torch.cuda.get_device_name(0)}
    out.update(head_bench(a.iters))
    out.update(step_bench(a.steps, a.warmup))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
