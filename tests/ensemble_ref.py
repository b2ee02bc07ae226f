"""Float64 NumPy restatement of the reference's ensemble combination (buglab/models/ensemble/wrapper.py:33-89) and of the
pre-layout un-batching of basemodel.py:240-346, for the ensemble tests (tests only)."""
from collections import defaultdict

import numpy as np


def _first_max(loc):
    """Python's max(d, key=d.get) over the dict's order."""
    keys = list(loc)
    best = keys[0]
    for k in keys[1:]:
        if loc[k] > loc[best]:
            best = k
    return best


def _avg(locs, rws):
    w = -np.log(len(rws))
    out_loc = {k: v + w for k, v in locs[0].items()}
    for loc in locs[1:]:
        for k, v in loc.items():
            out_loc[k] = np.logaddexp(out_loc[k], v + w)
    out_rw = [v + w for v in rws[0]]
    for rw in rws[1:]:
        for i, v in enumerate(rw):
            out_rw[i] = np.logaddexp(out_rw[i], v + w)
    return out_loc, out_rw


def combine(kind, member_preds):
    """member_preds: per member, None or (location dict, rewrite list) for ONE sample -> (location dict, rewrite list) or None
    when no member predicts it.  Location dicts are walked in their own order (pass canonically ordered dicts)."""
    present = [p for p in member_preds if p is not None]
    if not present:
        return None
    locs, rws = [p[0] for p in present], [p[1] for p in present]
    with np.errstate(all="ignore"):
        if kind == "avg":
            return _avg(locs, rws)
        picks = [_first_max(loc) for loc in locs]
        if all(p == picks[0] for p in picks[1:]):
            return _avg(locs, rws)
        out = {k: -np.inf for k in locs[0]}
        out[-1] = 0.0
        return out, list(rws[0])


def canonical(loc):
    """Location dict in the canonical order: nodes ascending, NO_BUG last."""
    return {**{k: loc[k] for k in sorted(k for k in loc if k != -1)}, -1: loc[-1]}


def combine_predictions(kind, per_member_results, datapoints):
    """per_member_results: per member, {id(datapoint): (loc, rw)} from the member's own predict -> the ensemble's triples,
    in data order, samples no member predicts skipped."""
    out = []
    for d in datapoints:
        preds = [r.get(id(d)) for r in per_member_results]
        preds = [None if p is None else (canonical(p[0]), p[1]) for p in preds]
        c = combine(kind, preds)
        if c is not None:
            out.append((d, c[0], c[1]))
    return out


def unbatch_dicts(mb, ids, loc_lp, swap_lp, num_samples, datapoints, text_lp, var_lp, node_mappings=None):
    """The un-batching of basemodel.py:240-346 as dict and list operations (what `_iter_per_sample_results` computed before it
    gathered through `prediction_layout`); NumPy inputs."""
    per_sample_loc = [loc_lp[ids == b] for b in range(num_samples)]

    def by_group(logprobs, groups):
        d = defaultdict(list)
        for g, lp in zip(np.asarray(groups).tolist(), np.asarray(logprobs).tolist()):
            d[g].append(lp)
        return d

    swap_g = by_group(swap_lp, mb["swapped_pair_to_call_location_group"])
    text_g = by_group(text_lp, mb["rewrite_to_location_group"])
    var_g = by_group(var_lp, mb["candidate_symbol_to_location_group"])
    next_group = 0
    for b in range(num_samples):
        point = datapoints[b]
        ref_nodes = point["graph"]["reference_nodes"]
        cand_nodes = np.unique(ref_nodes)
        if node_mappings is not None:
            cand_nodes = np.array([node_mappings[b][k] for k in cand_nodes])
        dist = per_sample_loc[b]
        location_logprobs = {int(n): float(lp) for n, lp in zip(cand_nodes, dist)}
        location_logprobs[-1] = float(dist[-1])
        flat_swap, flat_text, flat_var = [], [], []
        for _ in range(len(np.unique(ref_nodes))):
            flat_swap.extend(swap_g[next_group])
            flat_text.extend(text_g[next_group])
            flat_var.extend(var_g[next_group])
            next_group += 1
        rewrite_probs = [None] * len(point["candidate_rewrites"])
        for idxs, lps in ((mb["text_rewrite_original_idxs"][b], flat_text), (mb["candidate_rewrite_original_idxs"][b], flat_var),
                          (mb["pair_rewrite_original_idx"][b], flat_swap)):
            for i, lp in zip(idxs, lps):
                rewrite_probs[i] = lp
        if node_mappings is not None:
            reverse = defaultdict(list)
            for old, new in node_mappings[b].items():
                if old in ref_nodes:
                    reverse[new].append(old)
            remapped = {}
            for n, p in location_logprobs.items():
                for node in (reverse[n] if n >= 0 else [n]):
                    remapped[node] = p
            location_logprobs = remapped
        yield point, location_logprobs, rewrite_probs
