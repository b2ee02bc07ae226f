#!/usr/bin/env python
"""Golden outputs of the REFERENCE's bug-selection arithmetic (buglab/controllers/bugselectorserver.py:22-75), run unmodified
from the reference checkout (`REF` below; build container only):

    python tests/golden/make_golden_selfsup.py       # rewrites tests/golden/selfsup_selection.json.gz

`calculate_selection_distribution` on lists of log-probabilities (float32 numbers, as a model's outputs are): temperatures
1, 0.5 and 3, the epsilon branch forced (epsilon 1: `np.random.rand() < 1` always) or excluded (epsilon 0), -inf entries,
one-candidate samples, strongly peaked samples, n in the thousands; and `BugSelectionStats.add` / `.report()` on those
distributions with fixed selections.  The module's imports that do not exist in the build container (zmq, dpu_utils, the
model-sync client, the logging helpers) are stubbed: none of them is touched by the two things called here.
"""
import contextlib
import gzip
import io
import json
import os
import sys
import types

import numpy as np

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
import make_golden as MG  # noqa: E402

NINF = float("-inf")
SCOUTS = ["BinaryOperatorRewriteScout", "VariableMisuseRewriteScout", "ArgSwapRewriteScout", "LiteralRewriteScout",
          "ComparisonOperatorRewriteScout"]


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def install_service_stubs():
    anything = type("Anything", (), {"__init__": lambda self, *a, **k: None, "__getattr__": lambda self, n: (lambda *a, **k: None)})
    _stub("zmq", Context=anything, Socket=anything, REP=0, REQ=1)
    _stub("dpu_utils")
    _stub("dpu_utils.utils", run_and_debug=lambda f, debug: f())
    _stub("buglab.data.modelsync", MockModelSyncClient=anything, ModelSyncClient=anything)
    _stub("buglab.utils.logging", MetricProvider=anything, configure_logging=lambda *a, **k: None)


def f32(x):
    return float(np.float32(x))


def make_logprobs(rng, n, kind):
    """n rewrite entries + NO_BUG, roughly normalised log-probabilities as a selector gives them"""
    raw = rng.normal(size=n + 1) * (4.0 if kind == "peaked" else 1.5)
    lp = [f32(v) for v in raw - np.log(np.exp(raw).sum())]
    if kind == "neginf" and n >= 2:
        lp[0] = NINF
        lp[n // 2] = NINF
    return lp


def main():
    MG._install_stubs()
    install_service_stubs()
    sys.path.insert(0, REF)
    from buglab.controllers.bugselectorserver import BugSelectionStats, calculate_selection_distribution  # noqa: reference code

    rng = np.random.default_rng(20211206)
    cases = []
    sizes = [0, 1, 2, 5, 11, 40, 130, 299, 1000, 4095]
    for temperature in (1.0, 0.5, 3.0):
        for epsilon in (0.0, 1.0):
            for n in sizes:
                for kind in ("plain", "peaked", "neginf"):
                    if kind == "neginf" and (n < 2 or epsilon == 1.0):
                        continue
                    if n >= 1000 and (kind == "peaked" or temperature == 3.0):
                        continue
                    lp = make_logprobs(rng, n, kind)
                    with np.errstate(all="ignore"):
                        p = calculate_selection_distribution(logprobs=lp, temperature=temperature, epsilon=epsilon)
                    cases.append({"temperature": temperature, "epsilon": epsilon, "kind": kind, "logprobs": lp,
                                  "distribution": [float(v) for v in p]})

    # BugSelectionStats on the small samples: fixed metadata and selections
    stats = BugSelectionStats()
    added = []
    for ci, case in enumerate(cases):
        n = len(case["logprobs"]) - 1
        if not 2 <= n <= 40 or case["kind"] == "neginf":
            continue
        metadata = [[SCOUTS[int(rng.integers(0, len(SCOUTS)))], None] for _ in range(n)]
        picks = sorted(rng.choice(n + 1, size=min(4, n + 1), replace=False).tolist())
        selected = {("NO_BUG" if i == n else str(i)): case["logprobs"][i] for i in picks}
        selected.setdefault("NO_BUG", case["logprobs"][n])
        stats.add({"candidate_rewrite_metadata": metadata}, np.asarray(case["distribution"]), selected)
        added.append({"case": ci, "candidate_rewrite_metadata": metadata, "selected": selected})
    state = {"available_rewrite_frequency": dict(stats.available_rewrite_frequency),
             "selected_rewrite_frequency": dict(stats.selected_rewrite_frequency), "entropy_sum": float(stats.entropy_sum),
             "uniform_baseline_entropy_sum": float(stats.uniform_baseline_entropy_sum), "total_samples": stats.total_samples}
    printed = io.StringIO()
    with contextlib.redirect_stdout(printed):
        report = stats.report()
    out = {"numpy": np.__version__, "cases": cases,
           "stats": {"added": added, "state": state, "report": report, "printed": printed.getvalue()}}
    with gzip.open(os.path.join(OUT, "selfsup_selection.json.gz"), "wt") as f:
        json.dump(out, f)
    print(f"{len(cases)} distributions, {len(added)} samples in the statistics")


if __name__ == "__main__":
    main()
