#!/usr/bin/env python
"""Golden outputs of the REFERENCE's ensemble combination (buglab/models/ensemble/wrapper.py:33-89), run unmodified from
the reference checkout (`REF` below; build container only) on members that replay stored predictions:

    python tests/golden/make_golden_ensemble.py       # rewrites tests/golden/ensemble_predictions.json.gz

`EnsembleWrapper.predict` calls every member's `predict` on one-sample lists; here each member is a fake whose `predict`
yields its stored `(datapoint, {node: logprob, -1: NO_BUG}, [rewrite logprob])` triple for that sample, or nothing (the
member has no prediction for it).  Member values are float32 numbers, as the members' own outputs are.  The cases cover
both kinds, M = 1, 2, 3, members missing from some samples, a sample no member predicts, exact location ties (agreeing
and disagreeing arg-maxes), -inf entries and NaN entries.
"""
import gzip
import json
import os
import sys

import numpy as np

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
import make_golden as MG  # noqa: E402

NINF = float("-inf")


def f32(x):
    return float(np.float32(x))


def make_member_predictions(rng, nodes, n_rw):
    lp = rng.normal(size=len(nodes) + 1) * 2.0
    lp = lp - np.log(np.exp(lp).sum())
    rw = rng.normal(size=n_rw) - 1.0
    return [f32(v) for v in lp], [f32(v) for v in rw]


def make_case(name, kind, M, n_samples, seed, special=True):
    """-> {"kind", "M", "samples": [{"nodes": [...], "n_rw": k, "members": [None | [loc values (nodes..., NO_BUG), rewrites]]}]}"""
    rng = np.random.default_rng(seed)
    samples = []
    for i in range(n_samples):
        nodes = sorted(rng.choice(np.arange(3, 90), size=int(rng.integers(2, 9)), replace=False).tolist())
        n_rw = int(rng.integers(1, 13))
        members = [list(make_member_predictions(rng, nodes, n_rw)) for _ in range(M)]
        if special:
            r = i % 8
            if r == 1 and M > 1:  # a member has no prediction for this sample
                members[int(rng.integers(0, M))] = None
            elif r == 2:  # nobody predicts it: the reference skips the sample
                members = [None] * M
            elif r == 3:  # exact tie at the top, every member's first maximum the same node (agreement)
                for mem in members:
                    top = max(mem[0]) + 0.25
                    mem[0][0] = mem[0][1] = f32(top)
            elif r == 4 and M > 1:  # exact tie at the top, the members' first maxima differ (disagreement under consensus)
                for j, mem in enumerate(members):
                    top = max(mem[0]) + 0.25
                    mem[0][j % 2] = mem[0][2 if len(nodes) > 2 else 1 - j % 2] = f32(top)
                    if j % 2 == 1:
                        mem[0][0] = f32(top - 1.0)
            elif r == 5:  # -inf entries: one location in every member (logaddexp(-inf, -inf) = -inf), one rewrite in one
                for mem in members:
                    mem[0][0] = NINF
                members[0][1][0] = NINF
            elif r == 6:  # NaN: a rewrite of member 0; a location of the last member (not its first entry)
                members[0][1][-1] = float("nan")
                members[-1][0][1] = float("nan")
            elif r == 7:  # NaN as the FIRST location entry of member 0: Python's max keeps it
                members[0][0][0] = float("nan")
            elif r == 0 and M > 1:  # all members agree on the arg-max node
                for mem in members:
                    mem[0][-2] = f32(max(mem[0]) + 1.0)
        samples.append({"nodes": nodes, "n_rw": n_rw, "members": members})
    return {"name": name, "kind": kind, "M": M, "samples": samples}


def to_json_dict(d):
    return [[int(k), float(v)] for k, v in d.items()]


def main():
    MG._install_stubs()
    sys.path.insert(0, REF)
    from buglab.models.ensemble.wrapper import EnsembleModuleWrapper, EnsembleWrapper  # noqa: reference code

    cases = []
    for kind in ("avg", "consensus"):
        for M in (1, 2, 3):
            cases.append(make_case(f"{kind}_m{M}", kind, M, 24, seed=100 * M + (kind == "consensus")))
    cases.append(make_case("consensus_m3_plain", "consensus", 3, 16, seed=7, special=False))

    for case in cases:
        M, samples = case["M"], case["samples"]

        def member(m):
            def predict(data, nn, device, parallelize):
                for point in data:
                    mem = samples[point["id"]]["members"][m]
                    if mem is None:
                        continue
                    loc = dict(zip(samples[point["id"]]["nodes"] + [-1], mem[0]))
                    yield point, loc, list(mem[1])

            return type("Member", (), {"predict": staticmethod(predict)})()

        ens = EnsembleWrapper([member(m) for m in range(M)], case["kind"])
        points = [{"id": i} for i in range(len(samples))]
        with np.errstate(all="ignore"):
            out = list(ens.predict(iter(points), EnsembleModuleWrapper([None] * M), "cpu", False))
        case["expected"] = [{"id": p["id"], "location_logprobs": to_json_dict(loc), "rewrite_logprobs": [float(v) for v in rw]}
                            for p, loc, rw in out]
        print(f"{case['name']}: {len(samples)} samples, {len(out)} predictions")
    with gzip.open(os.path.join(OUT, "ensemble_predictions.json.gz"), "wt") as f:
        json.dump({"numpy": np.__version__, "cases": cases}, f)


if __name__ == "__main__":
    main()
