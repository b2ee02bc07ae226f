"""Float64 restatements, written for the tests, of the arithmetic of the reference's two self-supervision services
(buglab/controllers/bugselectorserver.py:120-150, detectordatascoringworker.py:118-130) and of Gumbel top-k sampling.  They
work on what the pinned `predict` returns: ({node: logprob, -1: NO_BUG}, [rewrite logprob]) of Python floats."""
import itertools
import math

import numpy as np


def selection_logprobs(datapoint, location_logprobs, rewrite_logprobs):
    """per rewrite: its log-probability + that of its reference node; NO_BUG's appended"""
    out = [rw + location_logprobs[node] for rw, node in zip(rewrite_logprobs, datapoint["graph"]["reference_nodes"])]
    out.append(location_logprobs[-1])
    return out


def selection_distribution(logprobs, temperature, uniform):
    g = np.asarray(logprobs, dtype=np.float64)
    if uniform:
        return np.ones(g.shape[0]) * (1 / g.shape[0])
    with np.errstate(all="ignore"):
        e = np.exp(g / temperature)
        return e / e.sum()


def entropy(p):
    with np.errstate(all="ignore"):
        return float(-np.sum(p * np.log(p)))


def gumbel_keys(p, u):
    with np.errstate(all="ignore"):
        return np.log(p) - np.log(-np.log(np.asarray(u, dtype=np.float64)))


def gumbel_topk(p, u, k):
    """-> (the min(k, #{p > 0}) entries with the largest keys, in descending key order, ties to the lower index;
    the smallest gap between neighbouring keys among the winners and the first loser)"""
    keys = gumbel_keys(p, u)
    eligible = [i for i in range(len(p)) if p[i] > 0]
    ranked = sorted(eligible, key=lambda i: (-keys[i], i))
    kb = min(k, len(ranked))
    top = ranked[:kb + 1]
    gaps = [keys[a] - keys[b] for a, b in zip(top, top[1:])]
    return ranked[:kb], (min(gaps) if gaps else math.inf)


def target_logprob(datapoint, location_logprobs, rewrite_logprobs):
    target = datapoint["target_fix_action_idx"]
    if target is None:
        return float(location_logprobs[-1])
    return float(location_logprobs[datapoint["graph"]["reference_nodes"][target]] + rewrite_logprobs[target])


def inclusion_probabilities(p, k=2):
    """P(entry i is among k = 2 draws without replacement, each proportional to p among what is left): the ordered pairs"""
    assert k == 2
    p = np.asarray(p, dtype=np.float64)
    inc = np.zeros(len(p))
    for i, j in itertools.permutations(range(len(p)), 2):
        pr = p[i] * p[j] / (1.0 - p[i])
        inc[i] += pr
        inc[j] += pr
    return inc
