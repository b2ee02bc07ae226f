#!/usr/bin/env python
"""
Usage:
    visualize.py [options] MODEL_FILENAME DATA_PATH OUT_HTML

Options:
    --minibatch-size=<size>    Accepted for command-line compatibility (the reference parses and ignores it too).
    --sequential               Do not parallelize data loading. Makes debugging easier.
    --num-elements=<num>       The number of elements to visualize [default: 1000]
    --sample-pct=<num>         The percent of elements to keep from the input data. Valid for num-elements. [default: 1.]
    --only-no-bug              Print only snippets that have NO_BUG inserted.
    --only-incorrect           Print only snippets where the model has predicted something wrong.
    --order-by-confidence      Order by probability of the predicted action.
    --show-only-top-k=<num>    Show only the top-k. If k is zero, then show all. [default: 0]
    --min-confidence=<p>       Show only warnings (a location is predicted) whose probability is at least p.
    --at-operating-point       The same, at the checkpoint's warning operating point (buglab/models/operatingpoint.py).
    --explain=<K>              Under each shown snippet, the K graph nodes its first suggestion rests on most (explain.py; graph models).
    --report-json=<path>       Also write the report as data (the contexts the page is rendered from).
    --restore-path=<path>      Accepted for command-line compatibility (unused by the reference's run()).
    --quiet                    Accepted for command-line compatibility.
    --debug                    Accepted for command-line compatibility.
    --aml, --azure-info=<path> Refused: Azure ML / Azure storage are not available here.
    -h --help                  Show this screen.

Counterpart of reference buglab/models/visualize.py: run a trained detector over a data set and write an HTML page of code
snippets with the predicted location, the predicted rewrite, their probabilities, the ground truth and a "mistake" mark.
Works for every single model of the registry; an ensemble is refused (`scan` runs on a single detector model; ensembles
(EnsembleWrapper) are not supported here).

The reference copies every log-probability to the host and renders EVERY snippet before --only-incorrect drops most of them
and before the sort.  Here `scan` summarises each predict minibatch on the device (hip_ops.report_summarize,
csrc/bl_report.hip: predicted location, best rewrite per code range, confidence, mistake flag, in fp64 from the flat fp32
output), keeps the confidences and flags of all samples in device buffers, orders and cuts them there once
(hip_ops.report_order), copies back the verdicts, and only then gathers the log-probabilities of the SELECTED samples and
builds their snippets.  Each minibatch's flat output stays on the device until the order is known: --num-elements bounds that
memory (a few thousand floats per sample).

Where this differs from the reference ("Bug reports"): --show-only-top-k cuts (the reference's slice is not
assigned); `show_top_k` is a parameter of `predictions_to_html`, not a module global; any registry model; within one
segment, ranges are listed by (start, end) rather than in set order; ensembles are refused.
"""
from __future__ import annotations

import argparse
import html
import json
import sys
from itertools import islice
from pathlib import Path
from typing import Any, Dict, Iterable, Iterator, List, NamedTuple, Optional, Sequence, Tuple

if __package__ in (None, ""):
    sys.path.insert(0, str(Path(__file__).resolve().parents[2]))

import numpy as np

from buglab.models import _report as R
from buglab.utils.text import text_to_range_segments

PREDICTIONS_CHUNK = 50  # `predictions_to_report` summarises this many triples at a time


class Report(NamedTuple):
    snippets: List[Dict[str, Any]]  # the contexts of the selected samples, in report order
    selected: np.ndarray            # [len(snippets)] their indices among the scanned samples
    is_wrong: np.ndarray            # [n] bool, every scanned sample
    prediction_logprob: np.ndarray  # [n] float64, every scanned sample
    warned: Optional[np.ndarray] = None  # [n] bool, every scanned sample: a location was predicted, not NO_BUG
    confidence: Optional[np.ndarray] = None  # [n] float64: the predicted location's log-probability, what `evaluate` thresholds

    @property
    def num_scanned(self) -> int:
        return int(self.is_wrong.shape[0])


def _percent(logprob: float) -> str:
    return f"{np.exp(logprob):.1%}"


def snippet_context(datapoint, keys: Sequence[int], location_values: Sequence[float], rewrite_values: Sequence[float],
                    groups: R.SampleGroups, best_rw: Sequence[int], best_range_logprob: Sequence[float], pred_loc: int,
                    is_wrong: bool, prediction_logprob: float, no_bug_logprob: float) -> Dict[str, Any]:
    """The reference's per-snippet dict (visualize.py:154-165) with the snippet as `segments` instead of rendered markup: a
    plain segment is {"text"}, an annotated one the dict of :138-143 with the per-range dicts of :113-130."""
    graph = datapoint["graph"]
    rewrites = datapoint["candidate_rewrites"]
    target = datapoint["target_fix_action_idx"]
    target_action = "NO_BUG" if target is None else rewrites[target]
    group_of = {r: g for g, r in enumerate(groups.ranges)}
    members: List[List[int]] = [[] for _ in groups.ranges]
    for i, g in enumerate(groups.rw_grp.tolist()):
        members[g].append(i)

    def range_data(rng) -> Dict[str, Any]:
        g = group_of[rng]
        predicted_action = rewrites[int(best_rw[g])]
        is_ground = g == groups.tgt_grp
        at = int(groups.grp_loc[g])
        range_logprob = location_values[at] if at >= 0 else float("nan")
        (sl, sc), (el, ec) = rng
        return {
            "range": f"({sl},{sc})-({el},{ec})",
            "assigned_prob": _percent(range_logprob),
            "best_range_logprob": float(best_range_logprob[g]),
            "rewrites": [{"is_correct": bool(is_ground and rewrites[i] == target_action),
                          "is_predicted": bool(is_ground and rewrites[i] == predicted_action),
                          "rewrite": str(rewrites[i]), "prob": _percent(rewrite_values[i])} for i in members[g]],
            "is_ground_range": is_ground,
            "is_predicted_range": at == pred_loc,
        }

    segments = []
    for text, ranges in text_to_range_segments(graph["text"], graph["code_range"], groups.ranges):
        if not ranges:
            segments.append({"text": text})
            continue
        data = [range_data(r) for r in ranges]
        segments.append({"text": text, "target_ranges": data,
                         "contains_ground_range": any(t["is_ground_range"] for t in data),
                         "contains_predicted_range": any(t["is_predicted_range"] for t in data)})
    path = graph["path"]
    if "/site-packages/" in path:
        path = path[path.find("/site-packages/") + len("/site-packages/"):]
    return {"filename": path, "package": datapoint["package_name"], "segments": segments, "target_action": str(target_action),
            "no_bug_prob": _percent(no_bug_logprob), "is_wrong": bool(is_wrong), "prediction_logprob": float(prediction_logprob),
            "prediction_prob": _percent(prediction_logprob)}


# ------------------------------------------------------------------------------------------------
class _Chunk(NamedTuple):
    """One summarised minibatch, until the order is known."""

    datapoints: List[Any]
    ix: R.ReportIndices          # host copy of the index arrays
    groups: List[R.SampleGroups]
    keys: List[List[int]]
    src: Any                     # the flat output: a device tensor, or a NumPy array on the host path
    best_rw: Any                 # [total_grp] as src
    best_range: Any              # [total_grp]


def _build_snippets(chunks: List[_Chunk], starts: List[int], order: np.ndarray, sample_i: np.ndarray, sample_d: np.ndarray
                    ) -> List[Dict[str, Any]]:
    """The contexts of the samples of `order` (indices among all scanned samples).  The values of the selected samples leave
    the device in three copies for the whole report: their location and rewrite log-probabilities, the best rewrite and the
    best log-probability of their groups."""
    where = np.searchsorted(np.asarray(starts[1:], dtype=np.int64), order, side="right")  # chunk of every selected sample
    val_parts, rw_parts, range_parts, slices = [], [], [], {}
    n_val = n_grp = 0
    for c in sorted(set(where.tolist())):
        ch, ix = chunks[c], chunks[c].ix
        vi, gi = [], []
        for s in sorted(int(o) - starts[c] for o in order[where == c]):
            lo, hi, r0, r1, g0, g1 = (int(x) for x in (ix.loc_off[s], ix.loc_off[s + 1], ix.rw_off[s], ix.rw_off[s + 1],
                                                       ix.grp_off[s], ix.grp_off[s + 1]))
            vi += [ix.loc_idx[lo:hi], ix.rw_idx[r0:r1]]
            gi.append(np.arange(g0, g1))
            slices[starts[c] + s] = (n_val, hi - lo, r1 - r0, n_grp, g1 - g0)
            n_val += hi - lo + r1 - r0
            n_grp += g1 - g0
        vi, gi = np.concatenate(vi).astype(np.int64), np.concatenate(gi).astype(np.int64)
        if isinstance(ch.src, np.ndarray):
            val_parts.append(ch.src[vi]), rw_parts.append(ch.best_rw[gi]), range_parts.append(ch.best_range[gi])
        else:
            import torch

            dev = lambda a: torch.from_numpy(a).to(ch.src.device, non_blocking=True)
            val_parts.append(ch.src[dev(vi)]), rw_parts.append(ch.best_rw[dev(gi)]), range_parts.append(ch.best_range[dev(gi)])
    if not val_parts:
        return []
    if isinstance(val_parts[0], np.ndarray):
        values, rws, ranges = np.concatenate(val_parts), np.concatenate(rw_parts), np.concatenate(range_parts)
    else:
        import torch

        values, rws, ranges = (torch.cat(p).cpu().numpy() for p in (val_parts, rw_parts, range_parts))
    values = values.astype(np.float64).tolist()  # Python floats made from the fp32 values, as `predict` yields them
    rws, ranges = rws.tolist(), ranges.tolist()
    snippets = []
    for o, c in zip(order.tolist(), where.tolist()):
        s = o - starts[c]
        v0, n_loc, n_rw, q0, n_g = slices[o]
        ch = chunks[c]
        snippets.append(snippet_context(ch.datapoints[s], ch.keys[s], values[v0:v0 + n_loc], values[v0 + n_loc:v0 + n_loc + n_rw],
                                        ch.groups[s], rws[q0:q0 + n_g], ranges[q0:q0 + n_g], int(sample_i[0, o]),
                                        bool(sample_i[2, o]), float(sample_d[0, o]), float(sample_d[1, o])))
    return snippets


def warning_threshold(model, min_confidence: Optional[float] = None, at_operating_point: bool = False) -> Optional[float]:
    """The log-probability a warning must reach to be shown, or None (no filter): log(min_confidence), the checkpoint's
    operating point, or the larger of the two."""
    found = []
    if min_confidence is not None:
        if not 0 <= min_confidence <= 1:
            raise ValueError(f"--min-confidence takes a probability in [0, 1] (got {min_confidence})")
        found.append(float(np.log(min_confidence)) if min_confidence > 0 else -np.inf)
    if at_operating_point:
        point = getattr(model, "warning_operating_point", None)
        if point is None:
            raise ValueError("--at-operating-point: the checkpoint carries no warning operating point; fit one with "
                             "python -m buglab.models.operatingpoint")
        found.append(float(point.threshold_logprob))
    return max(found) if found else None


def _location_confidence(src, loc_idx, loc_off, pred_loc):
    """The confidence `evaluate` thresholds, float64 [B]: the log-probability of each sample's predicted LOCATION (NO_BUG is the
    last one) -- not `prediction_logprob`, which adds the best rewrite's.  NumPy arrays or tensors of one device alike; a sample
    without a location entry gets NaN."""
    if isinstance(src, np.ndarray):
        first, end = loc_off[:-1].astype(np.int64), loc_off[1:].astype(np.int64)
        at = np.clip(np.minimum(first + pred_loc, end - 1), 0, max(loc_idx.shape[0] - 1, 0))
        if loc_idx.shape[0] == 0:
            return np.full(first.shape[0], np.nan)
        return np.where(end > first, src[loc_idx[at]].astype(np.float64), np.nan)
    import torch

    first, end = loc_off[:-1].long(), loc_off[1:].long()
    if loc_idx.shape[0] == 0:
        return torch.full((first.shape[0],), float("nan"), dtype=torch.float64, device=src.device)
    at = torch.minimum(first + pred_loc.long(), end - 1).clamp_(0, loc_idx.shape[0] - 1)
    value = src[loc_idx[at].long()].double()
    return torch.where(end > first, value, torch.full_like(value, float("nan")))


def _finish_host(chunks: List[_Chunk], parts_i: List[np.ndarray], parts_d: List[np.ndarray], only_incorrect: bool,
                 order_by_confidence: bool, show_top_k: int, min_logprob: Optional[float] = None) -> Report:
    n_per = [len(c.datapoints) for c in chunks]
    starts = np.concatenate([[0], np.cumsum(n_per)]).astype(np.int64).tolist()
    sample_i = np.concatenate(parts_i, axis=1) if parts_i else np.zeros((3, 0), np.int32)
    sample_d = np.concatenate(parts_d, axis=1) if parts_d else np.zeros((2, 0), np.float64)
    confidence = np.concatenate([_location_confidence(np.asarray(c.src), np.asarray(c.ix.loc_idx), np.asarray(c.ix.loc_off), si[0])
                                 for c, si in zip(chunks, parts_i)]) if parts_i else np.zeros(0, np.float64)
    keep = sample_i[2] if only_incorrect else np.ones(sample_i.shape[1], np.int32)
    if min_logprob is not None:
        keep = ((keep != 0) & (sample_i[1] == 0) & (confidence >= min_logprob)).astype(np.int32)
    order = R.order_host(sample_d[0], keep, order_by_confidence, show_top_k)
    return Report(_build_snippets(chunks, starts, order, sample_i, sample_d), order, sample_i[2] != 0, sample_d[0].copy(),
                  sample_i[1] == 0, confidence)


def triples_indices(triples: Sequence[Tuple[Any, Dict[int, float], List[float]]]
                    ) -> Tuple[np.ndarray, R.ReportIndices, List[R.SampleGroups], List[List[int]]]:
    """`predict` triples as one minibatch of the report kernels: -> (flat float64 values: per sample its locations in dict
    order, then its rewrites; the index arrays over them; each sample's groups; each sample's location keys)."""
    src, groups, keys = [], [], []
    loc_off, rw_off = [0], [0]
    for point, location_logprobs, rewrite_logprobs in triples:
        k = list(location_logprobs)
        if not k or k[-1] != R.NO_BUG_NODE:
            raise ValueError("predictions_to_report: NO_BUG (-1) must be the last key of a sample's location log-probabilities")
        if len(rewrite_logprobs) != len(point["graph"]["reference_nodes"]):
            raise ValueError("predictions_to_report: one rewrite log-probability per candidate rewrite expected")
        src.append(np.fromiter((location_logprobs[x] for x in k), np.float64, len(k)))
        src.append(np.asarray(rewrite_logprobs, dtype=np.float64).reshape(-1))
        loc_off.append(len(k))
        rw_off.append(len(rewrite_logprobs))
        groups.append(R.sample_groups(point, k))
        keys.append(k)
    n_loc, n_rw = np.asarray(loc_off[1:]), np.asarray(rw_off[1:])
    base = np.concatenate([[0], np.cumsum(n_loc + n_rw)])[:-1]
    loc_idx = np.concatenate([b0 + np.arange(n) for b0, n in zip(base, n_loc)])
    rw_idx = np.concatenate([b0 + nl + np.arange(n) for b0, nl, n in zip(base, n_loc, n_rw)])
    ix = R.assemble(loc_idx, np.cumsum(loc_off), rw_idx.astype(np.int64), np.cumsum(rw_off), groups)
    return np.concatenate(src), ix, groups, keys


def predictions_to_report(predictions: Iterable[Tuple[Any, Dict[int, float], List[float]]], only_show_incorrect_predictions: bool = False,
                          order_results_by_confidence: bool = False, show_top_k: int = 0, min_logprob: Optional[float] = None) -> Report:
    """The report of `predict` triples that already exist (the model explorer's use), through the NumPy twins of the two
    kernels.  The location order of a sample is the key order of its dict; NO_BUG (-1) must be its last key, as every
    `predict` here yields it.  `min_logprob`: keep only the warnings whose predicted location has at least that log-probability."""
    chunks, parts_i, parts_d = [], [], []
    it = iter(predictions)
    while True:
        triples = list(islice(it, PREDICTIONS_CHUNK))
        if not triples:
            break
        flat, ix, groups, keys = triples_indices(triples)
        best_rw, best_range, si, sd = R.summarize_host(flat, ix)
        chunks.append(_Chunk([t[0] for t in triples], ix, groups, keys, flat, best_rw, best_range))
        parts_i.append(si), parts_d.append(sd)
    return _finish_host(chunks, parts_i, parts_d, only_show_incorrect_predictions, order_results_by_confidence, int(show_top_k),
                        min_logprob)


def scan(model, nn, data: Iterable[Any], device, *, parallelize: bool = False, only_incorrect: bool = False,
         order_by_confidence: bool = False, show_top_k: int = 0, min_confidence: Optional[float] = None,
         at_operating_point: bool = False, explain: int = 0) -> Report:
    """Run `model` over `data` (datapoints) and report: which samples are shown, in which order, and their contexts.  The
    samples the model's `tensorize` rejects are skipped, as `predict` skips them.  `min_confidence` (a probability) and
    `at_operating_point` (the model's `warning_operating_point`) keep only the warnings at or above that confidence.
    `explain` = K > 0: a second pass over the shown samples only (buglab/models/explain.py, graph models) gives each shown
    snippet's context an "influences" list: the K nodes the model's log-probability of its first suggestion rests on most."""
    import torch

    from buglab.controllers import _batching as Bt
    from buglab.models import hip_ops

    Bt.require_single_model(model, "scan")
    min_logprob = warning_threshold(model, min_confidence, at_operating_point)
    device = torch.device(device)
    on_gpu = device.type == "cuda"

    def extend(layout, points, dev, mb):
        ix, groups, keys = R.report_indices(layout, points, mb.get("node_mappings"))
        out = {"host": (points, ix, groups, keys)}
        if on_gpu:
            out["device"] = dict(zip(hip_ops.REPORT_INDEX_FIELDS, Bt.to_device_i32([getattr(ix, f) for f in hip_ops.REPORT_INDEX_FIELDS], dev)))
        return out

    chunks, parts_i, parts_d, parts_c = [], [], [], []
    nn.eval()
    with torch.no_grad(), model._tensorize_all_location_rewrites():
        for mb, _tags in Bt.prediction_minibatches(model, ((d, None) for d in data), device, parallelize, extend, lambda tag: None,
                                                   extend_sees_minibatch=True):
            flat = Bt.flat_prediction_output(nn, mb)
            points, ix, groups, keys = mb["selfsup"]["host"]
            if on_gpu:
                best_rw, best_range, si, sd = hip_ops.report_summarize(flat, mb["selfsup"]["device"])
                parts_c.append(_location_confidence(flat, mb["selfsup"]["device"]["loc_idx"], mb["selfsup"]["device"]["loc_off"], si[0]))
            else:
                flat = flat.numpy()
                best_rw, best_range, si, sd = R.summarize_host(flat, ix)
            chunks.append(_Chunk(points, ix, groups, keys, flat, best_rw, best_range))
            parts_i.append(si), parts_d.append(sd)
    if not on_gpu:
        return _finish_host(chunks, parts_i, parts_d, only_incorrect, order_by_confidence, int(show_top_k), min_logprob)
    starts = np.concatenate([[0], np.cumsum([len(c.datapoints) for c in chunks])]).astype(np.int64).tolist()
    if not chunks:
        return Report([], np.zeros(0, np.int32), np.zeros(0, bool), np.zeros(0, np.float64), np.zeros(0, bool), np.zeros(0, np.float64))
    sample_i, sample_d = torch.cat(parts_i, dim=1).contiguous(), torch.cat(parts_d, dim=1).contiguous()  # the growing buffers
    confidence = torch.cat(parts_c)
    keep = sample_i[2] if only_incorrect else torch.ones_like(sample_i[2])
    if min_logprob is not None:
        keep = ((keep != 0) & (sample_i[1] == 0) & (confidence >= min_logprob)).to(torch.int32)
    order = hip_ops.report_order(sample_d[0], keep, by_confidence=order_by_confidence, k=int(show_top_k)).cpu().numpy()
    sample_i, sample_d = sample_i.cpu().numpy(), sample_d.cpu().numpy()  # the verdicts: 3 int32 and 2 doubles per sample
    snippets = _build_snippets(chunks, starts, order, sample_i, sample_d)
    if explain:
        _add_influences(model, nn, chunks, starts, order, snippets, device, int(explain))
    return Report(snippets, order, sample_i[2] != 0, sample_d[0].copy(), sample_i[1] == 0, confidence.cpu().numpy())


def _add_influences(model, nn, chunks: List[_Chunk], starts: List[int], order: np.ndarray, snippets: List[Dict[str, Any]], device, k: int) -> None:
    """`--explain K`: the shown samples, and only they, go through buglab/models/explain.py once more (gradient x input of the
    first suggestion); each context gets "influences": [{"label", "kind", "share"}]."""
    from buglab.models.explain import explain

    where = np.searchsorted(np.asarray(starts[1:], dtype=np.int64), order, side="right")
    shown = [chunks[c].datapoints[o - starts[c]] for o, c in zip(order.tolist(), where.tolist())]
    found = {x.position: x for x in explain(model, nn, shown, device, k, parallelize=False)}
    for position, ctx in enumerate(snippets):
        ctx["influences"] = found[position].influences() if position in found else []


# ------------------------------------------------------------------------------------------------
_STYLE = """
body { font-family: sans-serif; margin: 1.5em; color: #1d1d1f; }
section.snippet { border: 1px solid #c8c8cc; border-radius: 6px; margin: 0 0 1.5em 0; padding: 0.6em 1em; }
section.snippet.wrong { border-left: 6px solid #b3261e; }
section.snippet h2 { font-size: 1em; margin: 0.2em 0; }
.package { color: #5b5b66; }
.mistake { color: #ffffff; background: #b3261e; border-radius: 3px; padding: 0 0.4em; margin-left: 0.6em; }
ul.facts { list-style: none; padding: 0; margin: 0.3em 0; }
ul.facts li { display: inline-block; margin-right: 1.5em; }
pre.code { background: #f4f4f6; padding: 0.6em; overflow-x: auto; }
mark.seg { background: #fff1b8; }
mark.seg.predicted { background: #ffc9a8; }
mark.seg.ground { outline: 2px solid #1b7f3b; }
mark.seg sup { font-size: 0.7em; }
ol.annotations > li { margin-bottom: 0.5em; }
table.range { border-collapse: collapse; margin: 0.2em 0 0.4em 0; }
table.range caption { text-align: left; }
table.range td, table.range th { border: 1px solid #c8c8cc; padding: 0.1em 0.5em; }
tr.correct td.rewrite { font-weight: bold; color: #1b7f3b; }
.ground-mark { color: #1b7f3b; font-weight: bold; }
.predicted-mark { color: #a34a00; font-weight: bold; }
"""


def _snippet_html(index: int, ctx: Dict[str, Any]) -> str:
    e = html.escape
    out = [f'<section class="snippet{" wrong" if ctx["is_wrong"] else ""}" id="snippet-{index}">',
           f'<h2><span class="package">{e(str(ctx["package"]))}</span> <span class="filename">{e(str(ctx["filename"]))}</span>'
           + ('<span class="mistake">mistake</span>' if ctx["is_wrong"] else "") + "</h2>",
           '<ul class="facts">',
           f'<li>Target: <code class="target-action">{e(ctx["target_action"])}</code></li>',
           f'<li>NO_BUG: <span class="no-bug-prob">{e(ctx["no_bug_prob"])}</span></li>',
           f'<li>Prediction: <span class="prediction-prob">{e(ctx["prediction_prob"])}</span></li>',
           "</ul>", '<pre class="code">']
    code, notes = [], []
    for seg in ctx["segments"]:
        if "target_ranges" not in seg:
            code.append(e(seg["text"]))
            continue
        n = len(notes) + 1
        cls = "seg" + (" ground" if seg["contains_ground_range"] else "") + (" predicted" if seg["contains_predicted_range"] else "")
        code.append(f'<mark class="{cls}" id="snippet-{index}-seg-{n}">{e(seg["text"])}<sup>{n}</sup></mark>')
        note = [f'<li class="segment"><code class="segment-text">{e(seg["text"])}</code>']
        for t in seg["target_ranges"]:
            marks = ('<span class="ground-mark">ground truth</span> ' if t["is_ground_range"] else "") + \
                    ('<span class="predicted-mark">predicted</span>' if t["is_predicted_range"] else "")
            note.append(f'<table class="range"><caption><span class="range-span">{e(t["range"])}</span> '
                        f'location <span class="assigned-prob">{e(t["assigned_prob"])}</span> {marks}</caption>')
            for rw in t["rewrites"]:
                flags = ('<span class="ground-mark">correct</span> ' if rw["is_correct"] else "") + \
                        ('<span class="predicted-mark">predicted</span>' if rw["is_predicted"] else "")
                note.append(f'<tr class="rewrite-row{" correct" if rw["is_correct"] else ""}"><td class="rewrite">{e(rw["rewrite"])}</td>'
                            f'<td class="prob">{e(rw["prob"])}</td><td class="flags">{flags}</td></tr>')
            note.append("</table>")
        note.append("</li>")
        notes.append("".join(note))
    out.append("".join(code) + "</pre>")
    if "influences" in ctx:  # (--explain only)
        out.append('<p class="influences">influenced by: '
                   + ", ".join(f'<span class="influence {e(str(i["kind"]))}">{e(str(i["label"]))} ({i["share"]:.0%})</span>' for i in ctx["influences"])
                   + "</p>")
    out.append('<ol class="annotations">' + "".join(notes) + "</ol>")
    out.append("</section>")
    return "\n".join(out)


def report_to_html(snippets: Sequence[Dict[str, Any]], include_header: bool = True) -> str:
    body = "\n".join(_snippet_html(i, ctx) for i, ctx in enumerate(snippets))
    if not include_header:
        return body + "\n"
    return ('<!DOCTYPE html>\n<html lang="en">\n<head>\n<meta charset="utf-8">\n<title>BugLab report</title>\n<style>' + _STYLE
            + f'</style>\n</head>\n<body>\n<h1>BugLab report</h1>\n<p class="summary">{len(snippets)} snippets</p>\n' + body + "\n</body>\n</html>\n")


def predictions_to_html(predictions, only_show_incorrect_predictions: bool = False, order_results_by_confidence: bool = False,
                        include_header: bool = True, show_top_k: int = 0) -> str:
    """The reference's signature, plus `show_top_k` (there a module global)."""
    report = predictions_to_report(predictions, only_show_incorrect_predictions, order_results_by_confidence, show_top_k)
    return report_to_html(report.snippets, include_header)


def report_to_json(report: Report) -> str:
    return json.dumps({"num_scanned": report.num_scanned, "num_wrong": int(report.is_wrong.sum()),
                       "selected": [int(i) for i in report.selected], "snippets": report.snippets}, indent=1, sort_keys=True) + "\n"


# ------------------------------------------------------------------------------------------------
def sampled(data: Iterable[Any], num_elements: int, sampling_rate: float) -> Iterator[Any]:
    """The first `num_elements` of `data`, each element kept with probability `sampling_rate`."""
    if sampling_rate == 1.0:
        yield from islice(data, num_elements)
        return
    taken = 0
    for element in data:
        if np.random.rand() < sampling_rate:
            yield element
            taken += 1
            if taken >= num_elements:
                break


def parse_args(argv=None) -> argparse.Namespace:
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("MODEL_FILENAME", help="A trained single model (`*.pkl.gz`); ensembles are refused.")
    p.add_argument("DATA_PATH", help="A folder of `*.msgpack.l.gz` files.")
    p.add_argument("OUT_HTML")
    p.add_argument("--minibatch-size", default=300)
    p.add_argument("--sequential", action="store_true")
    p.add_argument("--num-elements", type=int, default=1000)
    p.add_argument("--sample-pct", type=float, default=1.0)
    p.add_argument("--only-no-bug", action="store_true")
    p.add_argument("--only-incorrect", action="store_true")
    p.add_argument("--order-by-confidence", action="store_true")
    p.add_argument("--show-only-top-k", type=int, default=0)
    p.add_argument("--min-confidence", type=float, default=None)
    p.add_argument("--at-operating-point", action="store_true")
    p.add_argument("--explain", type=int, default=0, metavar="K",
                   help="Under each shown snippet, the K graph nodes its first suggestion rests on most (graph models; a second pass "
                        "over the shown samples only).")
    p.add_argument("--report-json", default=None)
    p.add_argument("--restore-path", default=None)
    p.add_argument("--quiet", action="store_true")
    p.add_argument("--debug", action="store_true")
    p.add_argument("--aml", action="store_true")
    p.add_argument("--azure-info", default=None)
    args = p.parse_args(argv)
    if args.aml or args.azure_info is not None:
        p.error("--aml / --azure-info: Azure ML and Azure storage are not available in this build")
    return args


def run(args: argparse.Namespace) -> Report:
    from buglab.models._cli import open_model, require_gpu
    from buglab.runtime.richpath import RichPath
    from buglab.utils.msgpackutils import load_all_msgpack_l_gz

    require_gpu(None, "visualize.py")
    data = sampled(load_all_msgpack_l_gz(RichPath.create(args.DATA_PATH), shuffle=args.sample_pct < 1), args.num_elements, args.sample_pct)
    if args.only_no_bug:
        data = (d for d in data if d["target_fix_action_idx"] is None)
    model, nn, device, _ = open_model(args.MODEL_FILENAME)
    report = scan(model, nn, data, device, parallelize=not args.sequential, only_incorrect=args.only_incorrect,
                  order_by_confidence=args.order_by_confidence, show_top_k=args.show_only_top_k, min_confidence=args.min_confidence,
                  at_operating_point=args.at_operating_point, explain=args.explain)
    with open(args.OUT_HTML, "w", encoding="utf-8") as f:
        f.write(report_to_html(report.snippets))
    if args.report_json is not None:
        with open(args.report_json, "w", encoding="utf-8") as f:
            f.write(report_to_json(report))
    if not args.quiet:
        print(f"Scanned {report.num_scanned} samples ({int(report.is_wrong.sum())} mistakes); {len(report.snippets)} shown.")
    return report


if __name__ == "__main__":
    run(parse_args())
