#!/usr/bin/env python
"""Headline benchmark: training graphs/sec of the gnn-mlp detector hot path on MI355X.

    python bench.py --gpus 1 --steps 10 --warmup 3
    python bench.py --gpus 1 --steps 10 --warmup 3 --full            # + every secondary measurement (below)
    python bench.py --gpus 1 --steps 10 --warmup 3 --dump-outputs DIR  # + the last timed step's results as DIR/*.npy
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W
    python bench.py --gpus N ...            # no launcher: re-runs itself under torch.distributed.run (self_launch)
    python bench.py --gpus 2 --dry-launch   # launcher self-test, CPU / gloo when no GPU is visible

One "step" = forward + backward + gradient all-reduce (N > 1) + clip + Adam on one minibatch of
synthetic PyPI-shaped code graphs that is already resident in HBM, every step from the same
seeded parameters (so that its outputs are reproducible; see make_step).  Workload at every N (weak
scaling): BASELINE.json configs[1] per GPU -- gnn-mlp, hidden 128, 8 MP layers, 16 edge types,
64 graphs x (2000 nodes, 10000 messages), dropout 0.2, fp32.  Rank 0 prints ONE JSON line with
the contract's fields (`value`, `ms_per_step` of the --steps timed steps, ...).  A plain run does
only that: set up, warm up, time, dump (--dump-outputs), print.  --full adds, after the timed
steps, `roofline` (dominant kernel kind of a serial profiling pass, priced against the ceiling
that binds), `box` (what this chip delivers: step clock / power, calibration kernels),
`predict_graphs_per_s` (forward only), `also` (configs[2] shard, the reference's 30 000-node
regime, the other activation placement, the bf16x6 split, configs[4] seq-great) and
`cpu_baseline` (CPU oracle through ModelTrainer.train); without it those fields are null.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(ROOT, "neurips21-self-supervised-bug-detection-and-repair_amd")
for _p in (ROOT, PKG):
    if _p not in sys.path:
        sys.path.insert(0, _p)

MFMA_F32_PEAK_TFLOPS = 157.3  # /opt/skills/guides/MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 dense peak
MFMA_BF16_PEAK_TFLOPS = 2500.0  # same guide: dense bf16 MFMA peak
# The message-passing GEMMs compute fp32-accurate products as SIX bf16 MFMA terms (csrc/bl_gemm_x6.hip),
# so their ceiling in algorithmic (2 M N K) FLOP/s is the bf16 pipe's peak / 6.
MFMA_X6_PEAK_TFLOPS = MFMA_BF16_PEAK_TFLOPS / 6.0
# ... or, since round 6, as THREE fp16 MFMA terms over two fp16 planes per operand (csrc/bl_gemm_h3.hip; the fp16 pipe's dense
# peak equals the bf16 one's): ceiling = peak / 3.
MFMA_H3_PEAK_TFLOPS = MFMA_BF16_PEAK_TFLOPS / 3.0
HBM_PEAK_GBS = 8000.0
REF_SCLK_MHZ, CLOCK_EXPONENT = 2250.0, 0.4  # box.value_at_ref_sclk (calibrate_rooflines)


# rocprofv3 kernel names of the timed GEMM kinds (for the committed PMC traffic file)
_KIND_TO_KERNEL = {
    "gemm_rows_x6_grouped": ["void gemm_rows_x6_kernel<false, -1>", "void gemm_rows_x6w_kernel<false>"],
    "gemm_rows_nk_routed_x6_grouped": ["void gemm_rows_x6_kernel<true, -1>", "void gemm_rows_x6w_kernel<true>"],
    "gemm_wgrad_routed_x6": ["void gemm_wgrad_x6_wide_kernel<true, true>", "void gemm_wgrad_x6_kernel<true>"],
    # the message GEMM / routed input gradient run as the 128 x 128 kernel (hidden-128 layers) or the wide 128 x 256 one
    # (>= 256 output columns: csrc/bl_gemm_x6w.hip) -- one kind, two kernels
    "msg_gemm_x6": ["void gemm_rows_x6_kernel<false, -1>", "void gemm_rows_x6w_kernel<false>"],
    "msg_dgrad_x6": ["void gemm_rows_x6_kernel<true, -1>", "void gemm_rows_x6w_kernel<true>"],
    "msg_wgrad_x6": ["void gemm_wgrad_x6_wide_kernel<true, true>", "void gemm_wgrad_x6_kernel<true>"],
    # (<MASKED / ROUTED, ONE>: the second parameter -- the one-term --amp form -- came late in round 6; older summaries hold the short names)
    "msg_gemm_h3": ["void gemm_rows_h3_kernel<false, false>", "void gemm_rows_h3_kernel<false>"],
    "msg_dgrad_h3": ["void gemm_rows_h3_kernel<true, false>", "void gemm_rows_h3_kernel<true>"],
    "msg_wgrad_h3": ["void gemm_wgrad_h3_kernel<true, false>", "void gemm_wgrad_h3_kernel<true>"],
}


def _pmc_record(path, kind):
    """The record of `kind` in a committed PMC summary: the launch-weighted mean over the kind's kernels that the file holds
    (counters are per-launch averages per kernel name)."""
    with open(path) as f:
        kernels = json.load(f).get("kernels", {})
    recs = [kernels[name] for name in _KIND_TO_KERNEL.get(kind, []) if name in kernels]
    if not recs:
        return None
    n = sum(r.get("launches", 1) for r in recs)
    out = {"launches": n}
    for key in set().union(*recs) - {"launches", "mfma_busy_frac", "l2_hit_rate"}:
        out[key] = sum(r.get(key, 0.0) * r.get("launches", 1) for r in recs) / n
    if "SQ_VALU_MFMA_BUSY_CYCLES" in out and out.get("GRBM_GUI_ACTIVE"):
        out["mfma_busy_frac"] = out["SQ_VALU_MFMA_BUSY_CYCLES"] / (out["GRBM_GUI_ACTIVE"] / 8.0 * 1024.0)
    elif len(recs) == 1 and "mfma_busy_frac" in recs[0]:
        out["mfma_busy_frac"] = recs[0]["mfma_busy_frac"]
    return out


def measured_traffic(kind):
    """HBM-side bytes per launch of `kind` from the newest committed PMC summary under profiles/
    (separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes over this same bench command; FETCH_SIZE is
    doubled as MI355X_MICROARCH.md prescribes for 16 B/lane reads on gfx950).  None if there is no file."""
    import glob

    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "*_bench_hbm_traffic.json")))
    if not files or kind not in _KIND_TO_KERNEL:
        return None, None
    rec = _pmc_record(files[-1], kind)
    if not rec:
        return None, None
    byts = (2.0 * rec.get("FETCH_SIZE_KB_per_launch", 0.0) + rec.get("WRITE_SIZE_KB_per_launch", 0.0)) * 1024.0
    return byts, os.path.relpath(files[-1], ROOT)


def algorithmic_work_per_graph(H, layers, N, E, T, B):
    """SURVEY.md section 8d formulas: forward FLOPs and compulsory HBM bytes of the MP stack per graph."""
    flop = 0.0
    byts = 0.0
    for li in range(layers):
        din, dm, dout = (2 * H, 2 * H, H) if li % 4 == 3 else (H, H, H)
        flop += 2.0 * E * (2 * din) * dm + 2.0 * N * dm * dout
        theta = T * 2 * din * dm + dm * dout + 2 * dm + dout
        byts += 4.0 * N * din + 8.0 * E + 4.0 * N * dout + 4.0 * theta / B
    return flop, byts


def message_gemm_bytes_per_step(H, layers, N, E, T, packed_bytes_per_elem):
    """Algorithmic HBM bytes per training step of the three message-GEMM kinds (operands read once, results written once), summed
    over the layers: packed rows of the layer input / of the node gradient (`packed_bytes_per_elem`: 4 for f16x2, 6 for bf16x3),
    the per-type weights, the index arrays, the routing bitmask, and the fp32 result -- [E, Dm] pre-activations (forward),
    [E, 2 Din] input-gradient rows (routed input gradient), [T, 2 Din, Dm] weight gradient."""
    out = {"fwd": 0.0, "dgrad": 0.0, "wgrad": 0.0}
    for li in range(layers):
        din, dm = (2 * H, 2 * H) if li % 4 == 3 else (H, H)
        w = 4.0 * T * 2 * din * dm
        out["fwd"] += packed_bytes_per_elem * N * din + w + 8.0 * E + 4.0 * E * dm
        out["dgrad"] += packed_bytes_per_elem * N * dm + w + 4.0 * E + E * dm / 8.0 + 4.0 * E * 2 * din
        out["wgrad"] += packed_bytes_per_elem * N * (din + dm) + 12.0 * E + E * dm / 8.0 + w
    return out


def dataflow_bytes_per_step(H, layers, N, E, T, packed_bytes_per_elem, vocab=15000):
    """Algorithmic bytes of ONE TRAINING STEP of the gnn-mlp stack as the dataflow is built: every launch's
    operands read once and its results written once, summed over the launches of a layer's forward and backward call and over the
    layers, plus the optimiser.  Unlike SURVEY 8d's compulsory bytes (a layer's inputs, outputs and parameters only: the figure a
    perfectly fused layer would move) this counts the E-sized fp32 intermediates the gather -> GEMM -> segmented-reduce formulation
    materialises -- [E, Dm] messages, [E, 2 Din] input-gradient rows -- and the packed operand copies; it does NOT count re-reads
    (a gathered row fetched once per message that uses it), which is what `roofline.traffic` measures.  Embedder and heads
    (< 1 % of the bytes) are left out.  -> (total, {kind: bytes})"""
    pk, d3 = packed_bytes_per_elem, 6.0  # message operands: f16x2 = 4 / bf16x3 = 6 bytes per element; dense node update: bf16x3
    msg = message_gemm_bytes_per_step(H, layers, N, E, T, pk)
    kinds = {"msg_gemm": msg["fwd"], "msg_dgrad": msg["dgrad"], "msg_wgrad": msg["wgrad"], "pack_rows": 0.0, "segment_max_ln": 0.0,
             "dense_fwd": 0.0, "node_update_bwd": 0.0, "dense_wgrad": 0.0, "node_grad_sums": 0.0}
    theta = vocab * H
    for li in range(layers):
        din, dm, dout = (2 * H, 2 * H, H) if li % 4 == 3 else (H, H, H)
        theta += T * 2 * din * dm + dm * dout + 2 * dm + dout
        kinds["pack_rows"] += (4.0 + pk) * N * din + (4.0 + pk) * N * dm          # layer input (forward), node gradient gq (backward)
        kinds["segment_max_ln"] += 4.0 * E * dm + 4.0 * N + (4.0 + 4.0 + d3) * N * dm + E * dm / 8.0 + 8.0 * N  # messages, CSR; aggregate, act', LN out (packed), routing bits, mean / rstd
        kinds["dense_fwd"] += d3 * N * dm + d3 * dm * dout + 4.0 * N * dout
        kinds["node_update_bwd"] += 2 * 4.0 * N * dout + 2 * 4.0 * N * dm + 8.0 * N + d3 * N * dout + 4.0 * N * dm  # g_out, h_out, aggregate, act', stats -> g_z (packed), gq
        kinds["dense_wgrad"] += d3 * N * (dm + dout) + 4.0 * dm * dout
        kinds["node_grad_sums"] += 4.0 * E * 2 * din + 8.0 * E + 8.0 * N + 4.0 * N * din
    kinds["adam_clip"] = (4.0 + 4.0 + 16.0 + 12.0) * theta  # zero fill, norm, read p / g / m / v, write p / m / v
    return sum(kinds.values()), kinds


def attach_message_gemm_bytes(kern, a, prof_steps):
    """gives the message-GEMM kinds of a profile table their algorithmic bytes, so that build_roofline can price them against BOTH
    ceilings and report the one that binds (with f16x3 the routed input gradient -- 57 FLOP/B -- is below the 104 FLOP/B ridge)"""
    if getattr(a, "model", "gnn-mlp") != "gnn-mlp":
        return kern
    for split, per_elem in (("h3", 4.0), ("x6", 6.0)):
        by = message_gemm_bytes_per_step(a.hidden, a.layers, a.nodes * a.graphs, a.messages * a.graphs, a.types, per_elem)
        for kind, key in ((f"msg_gemm_{split}", "fwd"), (f"msg_dgrad_{split}", "dgrad"), (f"msg_wgrad_{split}", "wgrad")):
            # (only when the kind ran for every layer: in bf16x6 mode the vector-unit path takes six of the eight input gradients)
            if kind in kern and kern[kind]["launches"] == prof_steps * a.layers:
                kern[kind]["alg_bytes"] = by[key] * prof_steps
    return kern


def build_roofline(kern, kern_overlap, prof_steps, serial_step_s, per_gpu_rate, fwd_flop, fwd_bytes, brief=False, dataflow=None,
                   graphs_per_step=0):
    """The `roofline` object of a bench line from the HIP-event tables of the profiling passes (hip_ops.KernelTimer).
    Dominant kernel = largest EXCLUSIVE time per step among the MFMA GEMM kinds of the serial pass (msg_dgrad_nodes runs
    on the vector units / LDS: listed with its non-zero FLOP rate, not a candidate; seq-great's attention kernels stream
    [B H L, L] score-sized matrices -- kinds that carry algorithmic bytes are candidates too, priced against the HBM peak).
    brief: the short form attached to an `also` entry (no per-kind tables)."""
    gemm = {k: v for k, v in kern.items() if (v["flop"] > 0 or v.get("bytes", 0) > 0) and v["ms"] > 0 and not k.endswith(("_nodes", "_vec"))}
    if not gemm:
        return None
    dom = max(gemm, key=lambda k: gemm[k]["ms"])
    d = kern[dom]
    x6, h3 = "x6" in dom, "h3" in dom
    mfma_peak = MFMA_H3_PEAK_TFLOPS if h3 else MFMA_X6_PEAK_TFLOPS if x6 else MFMA_F32_PEAK_TFLOPS
    hbm = d.get("bytes", 0) > 0
    both = None
    if not hbm and d["flop"] > 0 and d.get("alg_bytes", 0) > 0:
        # a GEMM kind with known algorithmic bytes: the ceiling that binds is the one whose minimum time is larger
        t_mfma, t_hbm = d["flop"] / (mfma_peak * 1e12), d["alg_bytes"] / (HBM_PEAK_GBS * 1e9)
        both = {"flop_per_byte": round(d["flop"] / d["alg_bytes"], 1), "ridge_flop_per_byte": round(mfma_peak * 1e12 / (HBM_PEAK_GBS * 1e9), 1),
                "frac_of_mfma_ceiling": round(d["flop"] / (d["ms"] * 1e-3) / 1e12 / mfma_peak, 4),
                "frac_of_hbm_ceiling": round(d["alg_bytes"] / (d["ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                "algorithmic_bytes_per_launch": round(d["alg_bytes"] / d["launches"])}
        if t_hbm > t_mfma:
            hbm = True
            d = dict(d, bytes=d["alg_bytes"])
    achieved = d["bytes"] / (d["ms"] * 1e-3) / 1e9 if hbm else d["flop"] / (d["ms"] * 1e-3) / 1e12
    peak = HBM_PEAK_GBS if hbm else mfma_peak
    traffic, traffic_src = measured_traffic(dom)
    per_step = lambda table: {k: {"ms_per_step": round(v["ms"] / prof_steps, 3),
                                  **({"tflops": round(v["flop"] / (v["ms"] * 1e-3) / 1e12, 2)} if v["flop"] > 0 and v["ms"] > 0 else {}),
                                  **({"gbs": round(v["bytes"] / (v["ms"] * 1e-3) / 1e9, 1)} if v.get("bytes", 0) > 0 and v["ms"] > 0 else {}),
                                  **({"overlapped": True} if v.get("overlapped") else {})} for k, v in sorted(table.items(), key=lambda kv: -kv[1]["ms"])}
    roof = {
        "bound": "hbm" if hbm else "mfma",
        "kernel": dom,
        "achieved": round(achieved, 2),
        "peak": round(peak, 1),
        "peak_basis": ("HBM3E peak; achieved = algorithmic bytes of the launch (operands read once, results written once) / its duration"
                       if hbm else "dense fp16 MFMA peak 2500 TF/s / 3 (f16x3: three fp16 MFMA terms per fp32-accurate product)"
                       if h3 else "dense bf16 MFMA peak 2500 TF/s / 6 (bf16x6: six bf16 MFMA terms per fp32-accurate product)"
                       if x6 else "dense fp32 MFMA peak"),
        "unit": "GB/s" if hbm else "TFLOP/s",
        "frac": round(achieved / peak, 4),
        **({"both_ceilings": both} if both else {}),
        **({} if hbm else {"frac_of_fp32_mfma_peak": round(achieved / MFMA_F32_PEAK_TFLOPS, 4),
                            "frac_of_bf16x6_ceiling": round(achieved / MFMA_X6_PEAK_TFLOPS, 4)}),
        "avg_launch_ms": round(d["ms"] / d["launches"], 4),
        "launches_per_step": d["launches"] / prof_steps,
        "share_of_serial_gpu_time": round(d["ms"] / sum(v["ms"] for v in kern.values()), 4),
        "serial_ms_per_step": round(1e3 * serial_step_s, 3),
        # whole-step view against both ceilings: training ~ 3x forward work
        "step_frac_of_mfma_x6_roofline": round(per_gpu_rate * 3 * fwd_flop / (MFMA_X6_PEAK_TFLOPS * 1e12), 4),
        "step_frac_of_mfma_h3_roofline": round(per_gpu_rate * 3 * fwd_flop / (MFMA_H3_PEAK_TFLOPS * 1e12), 4),
    }
    if dataflow is not None and graphs_per_step > 0:
        # whole step against the HBM ceiling by the bytes its dataflow moves (dataflow_bytes_per_step): steps per second x bytes per step
        roof["step_dataflow_gb"] = round(dataflow[0] / 1e9, 2)
        roof["step_frac_of_hbm_roofline_dataflow_bytes"] = round(per_gpu_rate / graphs_per_step * dataflow[0] / (HBM_PEAK_GBS * 1e9), 4)
    mfma_busy = measured_mfma_busy(dom)
    if mfma_busy is not None:
        roof["mfma_busy_frac"], roof["mfma_busy_source"] = mfma_busy
    if brief:
        top = sorted(gemm, key=lambda k: -gemm[k]["ms"])[:4]
        roof["top_kernels_serial"] = {k: per_step(kern)[k] for k in top}
        return roof
    roof.update({
        "traffic": None if traffic is None else round(traffic),
        "traffic_unit": "bytes per launch (2 x FETCH_SIZE + WRITE_SIZE; Infinity-Cache hits included)",
        "traffic_source": traffic_src,
        "measured": f"HIP events around every launch, {prof_steps} serial steps (side stream off) after the timed region: exclusive kernel time",
        "kernels_serial": per_step(kern),
        "kernels_as_timed": per_step(kern_overlap),
        "step_frac_of_mfma_f32_roofline": round(per_gpu_rate * 3 * fwd_flop / (MFMA_F32_PEAK_TFLOPS * 1e12), 4),
        "step_frac_of_hbm_roofline_compulsory_bytes": round(per_gpu_rate * 3 * fwd_bytes / (HBM_PEAK_GBS * 1e9), 4),
    })
    if dataflow is not None:
        roof["step_dataflow_gb_by_kind"] = {k: round(v / 1e9, 2) for k, v in sorted(dataflow[1].items(), key=lambda kv: -kv[1])}
    return roof


def calibrate_rooflines(box, roof, also, per_gpu_rate):
    """Adds the per-box view to the rooflines: `frac_calibrated` = achieved / the ceiling THIS box reached on the library's fixed
    calibration kernels (dense bf16 MFMA loop / 6 for a bf16x6 kernel; the HBM copy for an HBM-bound one) instead of the paper
    peak, and to `box` the headline per calibrated unit (graphs/s per calibrated bf16 PFLOP/s): two boxes that differ in the
    clock they sustain agree on it far better than on the raw rate."""
    def one(r):
        if not r:
            return
        if r["bound"] == "hbm":
            r["peak_calibrated"] = round(1e3 * box["hbm_calib_tbs"], 1)
        elif "f16x3" in r.get("peak_basis", ""):
            r["peak_calibrated"] = round(box["mfma_calib_tflops"] / 3.0, 1)
        elif "bf16x6" in r.get("peak_basis", ""):
            r["peak_calibrated"] = round(box["mfma_calib_tflops"] / 6.0, 1)
        else:
            return
        r["frac_calibrated"] = round(r["achieved"] / r["peak_calibrated"], 4)
    def step(r):
        if r and "step_frac_of_hbm_roofline_dataflow_bytes" in r:
            r["step_frac_of_hbm_calibrated_dataflow_bytes"] = round(r["step_frac_of_hbm_roofline_dataflow_bytes"] * HBM_PEAK_GBS / (1e3 * box["hbm_calib_tbs"]), 4)
    one(roof)
    step(roof)
    for entry in (also or {}).values():
        one(entry.get("roofline"))
        step(entry.get("roofline"))
    box["value_per_calibrated_pflops"] = round(per_gpu_rate / (box["mfma_calib_tflops"] / 1e3), 1)
    # the headline at a reference step clock: the step's kernels follow the shader clock with an exponent of ~0.4 (round 5 measured
    # 7.6 % more clock -> 2.9 % less GEMM time, profiles/r05x_mixed_clock.log; four boxes of round 6 with a 2.4 % raw spread agree to
    # 1.2 % this way)
    if box.get("sclk_mhz_step"):
        box["ref_sclk_mhz"] = REF_SCLK_MHZ
        box["value_at_ref_sclk"] = round(per_gpu_rate * (REF_SCLK_MHZ / box["sclk_mhz_step"]) ** CLOCK_EXPONENT, 1)
    box["mfma_calib_frac_of_paper_peak"] = round(box["mfma_calib_tflops"] / MFMA_BF16_PEAK_TFLOPS, 4)
    box["hbm_calib_frac_of_paper_peak"] = round(1e3 * box["hbm_calib_tbs"] / HBM_PEAK_GBS, 4)


def measured_mfma_busy(kind):
    """Matrix-pipe busy fraction of `kind`'s kernel from the newest committed SQ counter summary under profiles/
    (`*_pmc_sq.json`: SQ_VALU_MFMA_BUSY_CYCLES / (GRBM_GUI_ACTIVE x 4 SIMDs x CUs), a separate rocprofv3 --pmc pass over
    this same bench command).  None if there is no such file."""
    import glob

    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r0[4-9]*_pmc_sq.json")))
    if not files or kind not in _KIND_TO_KERNEL:
        return None
    rec = _pmc_record(files[-1], kind)
    if not rec or rec.get("mfma_busy_frac") is None:
        return None
    return round(float(rec["mfma_busy_frac"]), 4), os.path.relpath(files[-1], ROOT)


def cpu_baseline(args, seconds_budget=20.0, graphs_per_minibatch=8):
    """SURVEY section 8(d)'s protocol within a ~20 s budget: the CPU oracle (a restatement: the reference's ptgnn stack is not
    installable) driven through the kept training entry -- synthetic *.msgpack.l.gz shard -> registry model -> metadata pass ->
    ModelTrainer.train on CPU (oracle/cpu_train.py) -- one 8-graph minibatch of BASELINE-sized graphs per epoch, fp32, a warm-up
    epoch and then up to five timed ones (median); reading + tensorising + collating is timed apart."""
    from oracle.cpu_train import run_cpu_train

    return run_cpu_train(seconds_budget=seconds_budget, graphs_per_minibatch=graphs_per_minibatch, nodes_per_graph=args.nodes,
                         hidden=args.hidden, num_layers=args.layers, dropout=args.dropout, placement=getattr(args, "placement", "aggregated"))


def cpu_baseline_seq(args, seconds_budget=25.0):
    """seq-great on the CPU oracle (oracle/seq_oracle.py: the reference's own transformer layers restated and pinned,
    heads as in the graph model): forward + backward of a 2-sequence minibatch, fp32, all host cores."""
    import torch

    from buglab.data.synthetic import make_samples
    from buglab.models.seqmodel import SeqTensorizedSample, collate_sequences
    from oracle import buglab_oracle as O
    from oracle import great_oracle as G
    from oracle import seq_oracle as SO

    nb, D, T = 2, args.hidden, args.types
    mb = collate_sequences([SeqTensorizedSample(s, {}, ()) for s in make_samples(nb, seed=123, num_nodes=args.seq_len,
                                                                                    num_messages=2 * args.seq_len, num_edge_types=T)], T)
    cfg = G.GreatConfig(d_model=D, num_heads=8, num_layers=args.layers, dim_feedforward=4 * D, num_edge_types=T)
    g = torch.Generator().manual_seed(0)
    r = lambda *shape: (torch.randn(*shape, generator=g) * 0.05)
    p = {k: v for k, v in O.init_params(O.OracleConfig(hidden=D, num_layers=4, num_edge_types=T), seed=0).items() if not k.startswith("mp.")}
    p.update({"positional_encoding": r(1, 5000, D), "input_norm.weight": torch.ones(D), "input_norm.bias": torch.zeros(D)})
    for i in range(args.layers):
        pre = f"layers.{i}."
        p.update({pre + "self_attn._selfatt_head_transforms.weight": r(3 * D, D), pre + "self_attn._out_proj.weight": r(D, D),
                  pre + "self_attn._edge_attention_biases.weight": r(T, D), pre + "self_attn._reverse_edge_attention_biases.weight": r(T, D),
                  pre + "linear1.weight": r(4 * D, D), pre + "linear1.bias": r(4 * D), pre + "linear2.weight": r(D, 4 * D),
                  pre + "linear2.bias": r(D), pre + "norm1.weight": torch.ones(D), pre + "norm1.bias": torch.zeros(D),
                  pre + "norm2.weight": torch.ones(D), pre + "norm2.bias": torch.zeros(D)})
    leaves = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    t_spent, n_steps, step = 0.0, 0, 0
    default_threads = torch.get_num_threads()
    torch.set_num_threads(min(16, os.cpu_count() or 8))  # (many small ops: 16 threads beat one per core on a many-core host, see cpu_baseline)
    while True:
        t0 = time.perf_counter()
        for v in leaves.values():
            v.grad = None
        SO.forward_loss(leaves, mb, cfg)["loss"].backward()
        dt = time.perf_counter() - t0
        step += 1
        if step > 1:
            t_spent += dt
            n_steps += 1
        if step >= 2 and (t_spent + dt > seconds_budget or n_steps >= 3):
            break
    used = torch.get_num_threads()
    torch.set_num_threads(default_threads)
    return {"value": round(nb * n_steps / t_spent, 3), "unit": "graphs/s", "cores": used, "kind": "port",
            "sample": f"{n_steps} forward+backward passes of {nb} sequences ({args.seq_len} tokens, H{D}, {args.layers} layers) on the CPU oracle, dropout 0"}


def self_launch(nproc: int) -> int:
    """Re-run this very command line under `python -m torch.distributed.run --nproc-per-node nproc` and return its exit
    code.  The children see WORLD_SIZE and take the normal path; rank 0's JSON line goes to our stdout unchanged."""
    import socket
    import subprocess

    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s_:
        s_.bind(("127.0.0.1", 0))
        port = s_.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC only on this driver (RCCL / cross-process tensors)
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // nproc)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def dry_launch(expected_world: int) -> int:
    """Proves the launch path without touching a kernel: every rank joins the process group (RCCL when a GPU is
    visible, gloo otherwise), the ranks all-reduce their rank numbers, rank 0 prints one JSON line."""
    import torch
    import torch.distributed as dist

    from buglab.runtime import distributed as D

    on_gpu = torch.cuda.is_available()
    rank, world, device = D.init_from_env("cuda" if on_gpu else "cpu")
    total = float(rank)
    if world > 1:
        t = torch.tensor([float(rank)], device=device)
        dist.all_reduce(t)
        total = float(t.item())
        dist.barrier()
    ok = world == expected_world and total == world * (world - 1) / 2.0
    if rank == 0:
        print(json.dumps({"dry_launch": True, "ok": ok, "n_gpus": world, "backend": dist.get_backend() if world > 1 else None,
                          "rank_sum": total}), flush=True)
    if world > 1:
        dist.destroy_process_group()
    return 0 if ok else 1


DUMP_BUDGET_BYTES = 60 << 20  # array data of one --dump-outputs directory (.npy headers on top stay far below 64 MB in all)


def step_outputs(module, loss):
    """What a caller of the timed step holds after it: the loss, the parameters the optimiser wrote and the gradients the
    backward pass computed (name -> tensor)."""
    out = {"loss": loss.detach()}
    for name, p in module.named_parameters():
        out[f"param.{name}"] = p.detach()
        if p.grad is not None:
            out[f"grad.{name}"] = p.grad.detach()
    return out


def dump_outputs(out_dir, arrays, budget_bytes=DUMP_BUDGET_BYTES, seed=0):
    """Writes each tensor of `arrays` as out_dir/<name>.npy in float32, `budget_bytes` of data in all.  The smallest arrays
    are written whole; one larger than its share of what is left becomes a fixed, seeded sample of its flattened elements
    (the same positions on every run, in increasing order)."""
    import numpy as np
    import torch

    os.makedirs(out_dir, exist_ok=True)
    left = budget_bytes // 4
    todo = sorted(arrays.items(), key=lambda kv: (kv[1].numel(), kv[0]))
    for i, (name, t) in enumerate(todo):
        share = left // (len(todo) - i)
        t = t.float()
        if t.numel() > share:
            pick = torch.randperm(t.numel(), generator=torch.Generator().manual_seed(seed))[:share].sort().values
            t = t.reshape(-1)[pick.to(t.device)]
        a = t.cpu().numpy()
        np.save(os.path.join(out_dir, f"{name}.npy"), a)
        left -= a.size


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--model", default="gnn-mlp", choices=["gnn-mlp", "seq-great", "seq-transformer", "seq-gru"],
                    help="gnn-mlp: BASELINE configs[1] (default).  seq-great: BASELINE configs[4], relational transformer, "
                         "hidden 256, 5 layers, 8 heads, FF 1024, sequences of --seq-len tokens")
    ap.add_argument("--seq-len", type=int, default=512)
    ap.add_argument("--hidden", type=int, default=None, help="default 128 (gnn-mlp) / 256 (seq-great)")
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--types", type=int, default=16)
    ap.add_argument("--graphs", type=int, default=None, help="graphs (sequences) per GPU (weak scaling); default 64 / 32")
    ap.add_argument("--nodes", type=int, default=2000)
    ap.add_argument("--messages", type=int, default=10000)
    ap.add_argument("--dropout", type=float, default=0.2)
    ap.add_argument("--degree", default="uniform", choices=["uniform", "powerlaw"], help="in-degree law (powerlaw = BASELINE config c4, max 512)")
    ap.add_argument("--placement", default="aggregated", choices=["aggregated", "message"],
                    help="where the message activation (GELU) sits relative to the max aggregation: on the aggregated [N, Dm] tensor "
                         "(default: ptgnn's order as recollected, DESIGN.md section 2) or on every message before the max (rounds 1-5)")
    ap.add_argument("--aggregation", default="max", choices=["max", "sum", "mean"],
                    help="message aggregation: max (the reference's recipe, gnnlayerdefs.py:11,21 -- the headline) or ptgnn's sum / mean")
    ap.add_argument("--msg-gemm", default="f16x3", choices=["f16x3", "bf16x6", "f16x1"],
                    help="operand split of the message GEMMs (forward, weight gradient, routed input gradient): two fp16 planes / three MFMA "
                         "terms with power-of-two tensor scales (default, csrc/bl_gemm_h3.hip) or three bf16 planes / six terms (rounds 2-5)")
    ap.add_argument("--serial", action="store_true", help="weight-gradient GEMMs on the main stream everywhere (no side-stream overlap): the run "
                    "whose rocprofv3 --kernel-trace --stats averages are the exclusive kernel times the roofline quotes")
    ap.add_argument("--full", action="store_true", help="after the timed steps also measure the roofline (two profiling passes), the box "
                    "calibration, the forward-only rate, the `also` configurations and the CPU baseline (each can be left out by its --no-* "
                    "option); a plain run measures the headline only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps write the last step's loss, updated "
                    f"parameters and gradients as DIR/<name>.npy (float32; {DUMP_BUDGET_BYTES >> 20} MiB of data at most: larger arrays "
                    "as a fixed, seeded sample)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-box", action="store_true", help="skip the box calibration (MFMA loop, HBM copy, clock / power sampling) after the timed region")
    ap.add_argument("--unfused-node-bwd", action="store_true", help="A/B: the node update's backward chain as three kernels "
                    "(act backward, dense input gradient, LayerNorm backward) instead of bl_node_update_bwd")
    ap.add_argument("--default-stream", action="store_true", help="A/B: run the steps on the default stream instead of the trainer's "
                    "high-priority step stream (hip_ops.use_step_stream)")
    ap.add_argument("--wgrad-kcap", type=int, default=0, help="A/B: rows per workgroup flush of the bf16x6 weight-gradient GEMMs "
                    "(hip_ops.set_wgrad_kchunk_cap); 0 = the library's default")
    ap.add_argument("--no-overlap", action="store_true", help="N > 1: one gradient all-reduce per step instead of layer-wise buckets behind backward")
    ap.add_argument("--no-also", action="store_true", help="skip the extra configurations reported under `also` (configs[2] shard, seq-great)")
    ap.add_argument("--no-predict", action="store_true", help="skip the forward-only passes after the timed training steps (profiling)")
    ap.add_argument("--dry-launch", action="store_true", help="launcher self-test: start the --gpus ranks, initialise the process group "
                    "(gloo on CPU when there is no GPU), all-reduce one number, print one JSON line and exit -- no kernels")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` without a launcher: become the launcher.  One process per GPU under
        # torch.distributed.run on this node, rendezvous on 127.0.0.1 (the container host name may not resolve).
        sys.exit(self_launch(args.gpus))
    if args.dry_launch:
        sys.exit(dry_launch(args.gpus))
    seq = args.model.startswith("seq-")  # seq-great = BASELINE configs[4]; seq-transformer / seq-gru: the registry's other sequence encoders, same workload
    if args.hidden is None:
        args.hidden = 256 if seq else 128
    if args.graphs is None:
        args.graphs = 32 if seq else 64
    if seq:
        args.layers, args.types, args.dropout = (5 if args.layers == 8 else args.layers), (8 if args.types == 16 else args.types), 0.1

    import torch
    import torch.distributed as dist

    from buglab.data.collate import collate_samples, to_device
    from buglab.data.synthetic import make_samples
    from buglab.models import hip_ops
    from buglab.models.gnn import build_gnn_mlp_module
    from buglab.runtime import distributed as D
    from buglab.runtime.optim import FlatAdam

    rank, world, device = D.init_from_env("cuda")
    if world != args.gpus and rank == 0:  # the launcher decides; the line reports what actually ran (n_gpus = world)
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: running and reporting n_gpus={world}", file=sys.stderr)
    hip_ops.load_library()  # fail loudly if the HIP extension is missing
    hip_ops.set_msg_gemm_mode(args.msg_gemm)
    if args.serial:
        hip_ops.USE_SIDE_STREAM = False
    if args.wgrad_kcap:
        hip_ops.set_wgrad_kchunk_cap(args.wgrad_kcap)
    if args.unfused_node_bwd:
        hip_ops.set_fused_node_bwd(False)

    def build_workload(a):
        """(module, minibatch, optimiser) of one configuration: resident synthetic minibatch, random-init weights."""
        torch.manual_seed(0)  # identical initial weights on every rank
        if a.model.startswith("seq-"):
            # BASELINE configs[4]: every sequence has --seq-len tokens (1-6 subtokens each), 2 relations per token over 8 edge
            # kinds, 40 candidate locations and the usual rewrite candidates; laid out by the product's own padded collator
            from buglab.models.layers.messagepassing import SubtokenEmbedder
            from buglab.models.seqmodel import SeqBugLabModule, SeqTensorizedSample, SequenceEncoder, collate_sequences

            samples = make_samples(a.graphs, seed=1000 + rank, num_nodes=a.seq_len, num_messages=2 * a.seq_len, num_edge_types=a.types)
            mb_ = to_device(collate_sequences([SeqTensorizedSample(s, {}, ()) for s in samples], a.types), device)
            enc = SequenceEncoder(SubtokenEmbedder(15000, a.hidden, 6, a.dropout), a.hidden, a.types, a.layers, 8,
                                  4 * a.hidden, a.dropout, layer_type=a.model[4:])
            module_ = SeqBugLabModule(enc, 48).to(device).train()
            module_._dropout_base_seed = rank
        else:
            samples = make_samples(a.graphs, seed=1000 + rank, num_nodes=a.nodes, num_messages=a.messages, num_edge_types=a.types,
                                   degree=a.degree, max_degree=512)
            mb_ = to_device(collate_samples(samples, a.types), device)
            # what the registry's gnn() builds: layer dropout a.dropout, node-embedder dropout 0 (reference modelregistry.py:79-82)
            module_ = build_gnn_mlp_module(a.hidden, a.layers, a.types, dropout_rate=a.dropout, dropout_base_seed=rank,
                                           embedder_dropout_rate=0.0, message_activation_placement=a.placement,
                                           message_aggregation_function=a.aggregation).to(device).train()
        opt_ = FlatAdam(module_.parameters())
        if world > 1:
            opt_.broadcast_parameters(0)  # what the trainer does before its first step
            if hasattr(module_, "overlap_parameter_groups") and not args.no_overlap:
                opt_.set_overlap_groups(module_.overlap_parameter_groups())  # layer-wise gradient buckets behind the backward pass
        return module_, mb_, opt_

    def make_step(module_, mb_, opt_, graphs):
        # Every step trains from the same parameters, so that a run's outputs are the same in every run up to the rounding of
        # the kernels' unordered fp32 atomics.  Chained updates would carry that rounding into the next step's parameters,
        # where the max aggregation turns last-bit differences into other winners: two runs of 25 chained steps differ by
        # ~1 % in their gradients.  The restore is one device copy of the flat parameter buffer; Adam's moments, its step
        # count and the dropout seeds advance as in training.
        start_params = opt_.flat_param.clone()

        def step_():
            opt_.zero_grad()  # (joins the side stream: nothing reads the parameters any more)
            opt_.flat_param.copy_(start_params)
            hip_ops.invalidate_weight_packs()
            if world > 1:
                opt_.begin_data_parallel_step(graphs)
            loss_ = module_(**mb_)
            loss_.backward()
            if world > 1:
                # the trainer's data-parallel step: ONE all-reduce of [graphs x gradient | graphs, has-batch flag], the fused
                # clip + Adam divides by the global graph count on the device
                opt_.step_data_parallel(graphs)
            else:
                opt_.step()
            return loss_
        return step_

    def timed(step_, steps, warmup):
        for _ in range(warmup):
            step_()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        t0_ = time.perf_counter()
        for _ in range(steps):
            loss_ = step_()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        return D.max_over_ranks(time.perf_counter() - t0_, device), loss_

    prof_steps = max(3, min(args.steps, 10))

    def profile_pass(step_, side_stream: bool):
        prev = hip_ops.USE_SIDE_STREAM
        hip_ops.USE_SIDE_STREAM = side_stream and not args.serial
        try:
            step_()
            torch.cuda.synchronize()
            with hip_ops.KernelTimer() as timer:
                tp0 = time.perf_counter()
                for _ in range(prof_steps):
                    step_()
                torch.cuda.synchronize()
                wall = time.perf_counter() - tp0
                return timer.summary(), wall / prof_steps
        finally:
            hip_ops.USE_SIDE_STREAM = prev

    def fwd_work(a):
        """(forward FLOPs, compulsory forward bytes) per graph / sequence of configuration `a` (SURVEY 8d / 8f formulas)."""
        if a.model == "seq-gru":
            # per sequence and layer: input projections of both directions 2 L D (6 Hh) + recurrent products 2 L 2 Hh (3 Hh), Hh = D / 2
            Ls, Dh = a.seq_len, a.hidden
            return a.layers * (2.0 * Ls * Dh * 3 * Dh + 2.0 * Ls * Dh * 3 * (Dh // 2)), a.layers * (3 * 4.0 * Ls * Dh) + 4.0 * a.layers * 4.5 * Dh * Dh / a.graphs
        if a.model.startswith("seq-"):
            # per sequence and layer: QKV + output projections 8 L D^2, feed-forward 4 L D FF, Q.K^T + P.V 4 L^2 D (~5.4 GFLOP)
            Ls, Dh, FFd = a.seq_len, a.hidden, 4 * a.hidden
            n_par = a.layers * (4 * Dh * Dh + 2 * Dh * FFd)
            return (a.layers * (8.0 * Ls * Dh * Dh + 4.0 * Ls * Dh * FFd + 4.0 * Ls * Ls * Dh),
                    a.layers * (3 * 4.0 * Ls * Dh) + 4.0 * n_par / a.graphs)
        return algorithmic_work_per_graph(a.hidden, a.layers, a.nodes, a.messages, a.types, a.graphs)

    def dataflow_of(a):
        """bytes one training step of configuration `a` moves as the dataflow is built (gnn-mlp with the max aggregation and an
        fp32-accurate split of the message GEMMs; None otherwise)"""
        if a.model != "gnn-mlp" or a.aggregation != "max" or a.msg_gemm not in ("f16x3", "bf16x6"):
            return None
        return dataflow_bytes_per_step(a.hidden, a.layers, a.nodes * a.graphs, a.messages * a.graphs, a.types, 4.0 if a.msg_gemm == "f16x3" else 6.0)

    def side_config(**over):
        """One more BASELINE configuration, timed the same way (warm-up, barrier + synchronize on both sides, max over
        ranks) AFTER the headline run, on its own model and minibatch: reported under `also`, never as `value`."""
        import copy
        import gc

        a = copy.copy(args)
        for k, v in over.items():
            setattr(a, k, v)
        m_, mb2_, o_ = build_workload(a)
        st_ = make_step(m_, mb2_, o_, a.graphs)
        prev_mode = hip_ops.set_msg_gemm_mode(a.msg_gemm)
        try:
            el_, _ = timed(st_, args.steps, args.warmup)
            kern_, serial_s_ = profile_pass(st_, False)  # exclusive kernel times of this configuration (after its timed region)
            hip_ops.join_side_stream()
            torch.cuda.synchronize()
        finally:
            hip_ops.set_msg_gemm_mode(prev_mode)
        del m_, mb2_, o_, st_
        gc.collect()
        torch.cuda.empty_cache()
        unit = "sequences/s" if a.model.startswith("seq-") else "graphs/s"
        rate_ = a.graphs * world * args.steps / el_
        return {"value": round(rate_, 2), "unit": unit, "ms_per_step": round(1e3 * el_ / args.steps, 3),
                "per_gpu": a.graphs, "n_gpus": world,
                "roofline": build_roofline(attach_message_gemm_bytes(kern_, a, prof_steps), {}, prof_steps, serial_s_, rate_ / world, *fwd_work(a),
                                           brief=True, dataflow=dataflow_of(a), graphs_per_step=a.graphs)}

    if not args.default_stream:
        hip_ops.use_step_stream(device)  # what ModelTrainer.train does before its first step
    module, mb, opt = build_workload(args)

    step = make_step(module, mb, opt, args.graphs)

    for _ in range(args.warmup):
        step()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    calls0 = hip_ops.CALL_COUNT
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = step()
    host_issue_s = time.perf_counter() - t0  # the host has ISSUED every step; the device drains its queue until the synchronize below
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = D.max_over_ranks(time.perf_counter() - t0, device)
    calls_per_step = (hip_ops.CALL_COUNT - calls0) / args.steps
    last_loss = float(loss.detach())
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, step_outputs(module, loss))  # before any further step overwrites them

    # Per-kernel durations, measured live with HIP events on the stream each kernel is launched on (the C library
    # brackets every launch inside its per-layer entry points, hip_ops.KernelTimer the rest).  Two more passes over
    # the same resident minibatch, OUTSIDE the timed region so that ~200 event records per step do not perturb it:
    #   (a) as timed: weight-gradient GEMMs on the side stream next to the input-gradient chain -- their event spans
    #       overlap and are flagged;
    #   (b) serial (side stream off): every span is exclusive kernel time.  The roofline entry is taken from (b):
    #       the kernel with the largest exclusive share of the step.
    if args.full:
        kern_overlap, _ = profile_pass(step, True)      # every rank steps (the optimiser all-reduces); rank 0 reports
        kern, serial_step_s = profile_pass(step, False)
        if world > 1:
            dist.barrier()

    # What this box delivers (outside the timed region, rank 0's device): boxes of the pool differ by several
    # per cent in the clock they hold at the package power limit.  (i) shader clock + package power sampled through librocm_smi64
    # while plain training steps run (no event records), (ii) two fixed kernels of the library: a dense bf16 MFMA loop from
    # registers and a 2 GiB HBM copy.  The roofline entry carries `frac_calibrated` = achieved / (this box's calibrated ceiling).
    box = None
    if args.full and not args.no_box:
        from buglab.models.hip_ops.calibration import SmiSampler, box_calibration

        torch.cuda.synchronize()
        with SmiSampler() as smi:
            for _ in range(max(args.steps, 30)):
                step()
            torch.cuda.synchronize()
        box = box_calibration(device)
        under_load = smi.summary()
        box["sclk_mhz_step"] = None if under_load is None else under_load["sclk_mhz"]
        box["power_w_step"] = None if under_load is None else under_load["power_w"]
        box["smi"] = None if under_load is None else {k: under_load[k] for k in ("samples", "smi_device", "source")}
        box["device"] = torch.cuda.get_device_name(device)
        if world > 1:
            dist.barrier()

    # forward-only ("predict": localization + repair log-probabilities, eval mode) on the same batch --
    # SURVEY section 8d asks for it next to the training rate; outside the timed training region
    module.eval()
    predict_elapsed = None
    with torch.no_grad():
        def predict_pass():
            _, _, gout, _ = module.compute_localization_logprobs(mb["graph_data"])
            module._compute_repair_logprobs(gout, mb["target_rewrites"], mb["rewrite_to_location_group"],
                                            mb["candidate_symbol_to_location_group"], mb["swapped_pair_to_call_location_group"],
                                            mb["repair_group_ptr"], mb["repair_group_items"])
        if args.full and not args.no_predict:
            predict_pass()
            torch.cuda.synchronize()
            tp = time.perf_counter()
            for _ in range(args.steps):
                predict_pass()
            torch.cuda.synchronize()
            predict_elapsed = D.max_over_ranks(time.perf_counter() - tp, device)
    module.train()

    # The other BASELINE configurations the driver's one command should also put a number on (every rank runs them: the
    # optimiser all-reduces): configs[2]'s per-GPU shard (hidden 256, 32 graphs per GPU -- 256 graphs over 8 GPUs) and, on
    # one GPU, configs[4] (seq-great).  Each on its own model / minibatch after the headline run has been measured.
    also = {}
    if args.full and not args.no_also and not seq and args.hidden == 128 and args.degree == "uniform":
        hip_ops.join_side_stream()
        torch.cuda.synchronize()
        del module, mb, opt, step
        import gc

        gc.collect()
        torch.cuda.empty_cache()
        also["configs[2] gnn-mlp hidden=256 layers=8 edge_types=16 batch=32 graphs/GPU"] = side_config(hidden=256, graphs=32)
        # the reference's own minibatch regime: stop_extending_minibatch_after_num_nodes = 30000 (modelregistry.py:53) = 15 graphs of 2000 nodes
        also["reference minibatch regime: configs[1] model, batch=15 graphs/GPU (30000 nodes: modelregistry.py:53)"] = side_config(graphs=15)
        other = "message" if args.placement == "aggregated" else "aggregated"
        also[f"configs[1] with message_activation_placement={other} (the non-default placement of the one unpinned spec point)"] = side_config(placement=other)
        if args.aggregation == "max":
            # BASELINE.json's north_star words the layers as "gather -> MLP -> scatter-sum"; the reference's recipe aggregates by max
            # (gnnlayerdefs.py:11,21: the headline).  The sum form of the same model, for that wording:
            also["configs[1] with message_aggregation_function=sum (ptgnn's other aggregation; the reference's recipe passes max)"] = side_config(aggregation="sum")
        if args.msg_gemm == "f16x3":
            also["configs[1] with the message GEMMs as bf16x6 (three bf16 planes, six MFMA terms: rounds 2-5)"] = side_config(msg_gemm="bf16x6")
            # `train.py --amp` (reference train.py:8,106): fp16 operands, one MFMA term -- REDUCED PRECISION, outside the 1e-4 parity bound, reported
            # for users of that flag only (its roofline fractions are priced as if it were f16x3 and mean nothing)
            also["configs[1] under train.py --amp (message GEMMs with fp16 operands, one MFMA term, fp32 accumulation: reduced precision, not the headline)"] = dict(side_config(msg_gemm="f16x1"), reduced_precision=True)
        if world == 1:
            also["configs[4] seq-great hidden=256 layers=5 heads=8 ff=1024 batch=32 sequences x 512 tokens"] = side_config(
                model="seq-great", hidden=256, graphs=32, layers=5, types=8, dropout=0.1)
            # the registry's two other sequence encoders on the same workload (reference modelregistry.py:135-136; torch.nn layers there)
            for other in ("seq-transformer", "seq-gru"):
                also[f"{other} hidden=256 layers=5 batch=32 sequences x 512 tokens (registry model outside BASELINE's configs)"] = side_config(
                    model=other, hidden=256, graphs=32, layers=5, types=8, dropout=0.1)

    if rank == 0:
        total_graphs = args.graphs * world * args.steps
        fwd_flop, fwd_bytes = fwd_work(args)
        value = total_graphs / elapsed
        roof = None
        if args.full:
            roof = build_roofline(attach_message_gemm_bytes(kern, args, prof_steps), kern_overlap, prof_steps, serial_step_s, value / world,
                                  fwd_flop, fwd_bytes, dataflow=dataflow_of(args), graphs_per_step=args.graphs)
        if box is not None:
            calibrate_rooflines(box, roof, also, value / world)
        line = {
            "metric": "code-graphs/sec (train: fwd+bwd+optimizer)",
            "value": round(value, 2),
            "unit": "graphs/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(1e3 * elapsed / args.steps, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            # fp32 storage / accumulation; matrix-core products as split terms: message GEMMs two fp16 planes x three terms (or bf16x6),
            # dense node update / sequence-model projections three bf16 planes x six terms
            "dtype": ("f32 (f16x3 / bf16x6 split products)" if args.msg_gemm == "f16x3" and not seq else
                      "f16 operands / f32 accumulation in the message GEMMs (--amp; REDUCED PRECISION), f32 elsewhere" if args.msg_gemm == "f16x1" and not seq
                      else "f32 (bf16x6 split products)"),
            "data": "synthetic",
            "config": {
                "workload": (f"{args.model} {'relational transformer' if args.model == 'seq-great' else 'encoder (torch.nn arithmetic on the HIP path)'} hidden={args.hidden} layers={args.layers} heads=8 ff={4 * args.hidden} "
                             f"edge_kinds={args.types} batch={args.graphs} sequences/GPU x {args.seq_len} tokens dropout={args.dropout}") if seq else
                            (f"gnn-mlp hidden={args.hidden} layers={args.layers} edge_types={args.types} "
                             f"batch={args.graphs} graphs/GPU x ({args.nodes} nodes, {args.messages} msgs) dropout={args.dropout}"
                             + (" power-law in-degree (max 512)" if args.degree == "powerlaw" else "")),
                **({} if seq else {"message_activation_placement": args.placement, "message_gemm_split": args.msg_gemm,
                                   "message_aggregation_function": args.aggregation}),
                "global_batch": args.graphs * world,
                "parallelism": f"dp{world}",
                "loss_last_step": round(last_loss, 5),
                "c_abi_calls_per_step": round(calls_per_step, 1),
                # host time to issue a step (Python + autograd + C calls + launches); close to ms_per_step = the host, not the device, paces the run
                "host_issue_ms_per_step": round(1e3 * host_issue_s / args.steps, 3),
            },
            "predict_graphs_per_s": None if predict_elapsed is None else round(args.graphs * world * args.steps / predict_elapsed, 1),  # forward-only, eval mode
            "roofline": roof,
            "box": box,
            "also": also or None,
            "full": args.full,
            "cpu_baseline": None if (not args.full or args.no_cpu_baseline or world > 1) else (cpu_baseline_seq(args) if args.model == "seq-great" else None if seq else cpu_baseline(args)),
        }
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
