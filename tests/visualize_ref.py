"""A direct per-sample restatement of the bug report (reference buglab/models/visualize.py:55-170) on `predict` triples, with
dicts keyed by ranges and nodes as the reference has them and none of the product's index arrays: what `scan` on the device
and `report_indices` are compared with.  tests/test_visualize_host.py pins this restatement to the recorded reference contexts
(tests/golden/visualize_contexts.json.gz), so it is not its own judge.  The only product code used is the text cutting of
buglab/utils/text.py, which the same test pins to the recorded segmentation."""
import math

import numpy as np

from buglab.utils.text import as_range, non_empty, relative_range, text_to_range_segments


def percent(x):
    return f"{np.exp(x):.1%}"


def sample_context(datapoint, location_logprobs, rewrite_logprobs):
    graph = datapoint["graph"]
    nodes, rewrites = graph["reference_nodes"], datapoint["candidate_rewrites"]
    ranges = [as_range(r) for r in datapoint["candidate_rewrite_ranges"]]
    assert len(rewrite_logprobs) == len(nodes)
    node_at, actions_at = {}, {}
    for node, rewrite, rng, lp in zip(nodes, rewrites, ranges, rewrite_logprobs):
        node_at[rng] = node
        actions_at.setdefault(rng, []).append((rewrite, lp))
    predicted_node = max(location_logprobs, key=lambda k: location_logprobs[k])
    target = datapoint["target_fix_action_idx"]
    ground_node, target_action, target_range = (-1, "NO_BUG", None) if target is None else (nodes[target], rewrites[target], ranges[target])
    wrong, confidence, segments = ground_node != predicted_node, -math.inf, []
    for text, here in text_to_range_segments(graph["text"], graph["code_range"], node_at):
        if not here:
            segments.append({"text": text})
            continue
        data = []
        for rng in here:
            predicted_action = max(actions_at[rng], key=lambda x: x[1])[0]
            is_ground, is_predicted = target_range == rng, node_at[rng] == predicted_node
            range_lp = location_logprobs.get(node_at[rng], math.nan)
            data.append({"range": f"({rng[0][0]},{rng[0][1]})-({rng[1][0]},{rng[1][1]})", "assigned_prob": percent(range_lp),
                         "best_range_logprob": range_lp + max(lp for _, lp in actions_at[rng]),
                         "rewrites": [{"is_correct": is_ground and rw == target_action, "is_predicted": is_ground and rw == predicted_action,
                                       "rewrite": str(rw), "prob": percent(lp)} for rw, lp in actions_at[rng]],
                         "is_ground_range": is_ground, "is_predicted_range": is_predicted})
            if is_ground:
                wrong = True if not is_predicted else target_action != predicted_action
        segments.append({"text": text, "target_ranges": data, "contains_ground_range": any(t["is_ground_range"] for t in data),
                         "contains_predicted_range": any(t["is_predicted_range"] for t in data)})
        confidence = max(confidence, max(t["best_range_logprob"] for t in data))
    path = graph["path"]
    cut = path.find("/site-packages/")
    return {"filename": path if cut < 0 else path[cut + len("/site-packages/"):], "package": datapoint["package_name"], "segments": segments,
            "target_action": str(target_action), "no_bug_prob": percent(location_logprobs[-1]), "is_wrong": bool(wrong),
            "prediction_logprob": confidence, "prediction_prob": percent(confidence)}


def report(predictions, only_incorrect=False, by_confidence=False, top_k=0):
    """-> (contexts in report order, their indices among the predictions, every sample's context)"""
    everything = [sample_context(*triple) for triple in predictions]
    shown = [i for i, c in enumerate(everything) if c["is_wrong"] or not only_incorrect]
    if by_confidence:
        shown = sorted(shown, key=lambda i: -everything[i]["prediction_logprob"])
    if top_k > 0:
        shown = shown[:top_k]
    return [everything[i] for i in shown], shown, everything


def sample_arrays(datapoint, keys):
    """What `report_indices` says about one sample, from dicts: {rw_grp, rw_eq_target, grp_loc, grp_shown, tgt_grp, ground_loc}.
    `keys`: the sample's location keys in order; a location entry is a position in it."""
    nodes, rewrites = datapoint["graph"]["reference_nodes"], datapoint["candidate_rewrites"]
    ranges = [as_range(r) for r in datapoint["candidate_rewrite_ranges"]]
    distinct = list(dict.fromkeys(ranges))
    last_node = {rng: node for node, rng in zip(nodes, ranges)}
    base = as_range(datapoint["graph"]["code_range"])
    widened = [non_empty(relative_range(base, r)) for r in distinct]
    target = datapoint["target_fix_action_idx"]
    return {
        "rw_grp": [distinct.index(r) for r in ranges],
        "rw_eq_target": [int(target is not None and rw == rewrites[target]) for rw in rewrites],
        "grp_loc": [list(keys).index(last_node[r]) for r in distinct],
        "grp_shown": [int(w not in widened[g + 1:]) for g, w in enumerate(widened)],
        "tgt_grp": -1 if target is None else distinct.index(ranges[target]),
        "ground_loc": list(keys).index(-1 if target is None else nodes[target]),
    }
