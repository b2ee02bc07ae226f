"""CPU: the device evaluation path's host half -- `eval_indices` + `judge_host` (the NumPy twin of csrc/bl_evaluate.hip) against
`_iter_per_sample_results` -> `judge_sample` on the models' real tensorise / collate path, and `ColumnarEvaluationReport` against
`EvaluationReport`, text for text, on the predictions recorded from the reference (tests/golden/evaluate_reports.json.gz)."""
import gzip
import json
import os

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.test_visualize_host import _minibatch, _model, _unbatched_by_the_model, bits

with gzip.open(os.path.join(ROOT, "tests", "golden", "evaluate_reports.json.gz"), "rt") as f:
    FIXTURE = json.load(f)

FAMILIES = ["gnn-mlp", "seq-great"]


def _case(family, points):
    """-> (minibatch, EvalIndices, flat_size) of `points` through the model's own tensorise / collate"""
    from buglab.models import _evaluate as E
    from buglab.models.basemodel import prediction_layout

    model = _model(family, points)
    mb = _minibatch(model, points)
    layout = prediction_layout(mb)
    return model, mb, E.eval_indices(layout, points, mb.get("node_mappings")), layout.flat_size


def _dataset(family, n=14, seed=21):
    from buglab.data.synthetic import make_report_dataset

    return make_report_dataset(n, seed=seed, kind="seq" if family.startswith("seq") else "graph")


def _tied_values(rng, n, low=0.02):
    """fp32 log-probabilities on a grid of a few levels: exact ties are common"""
    return (np.round(np.log(rng.uniform(low, 1.0, size=n)) * 2) / 2).astype(np.float32)


def _assert_same(outcomes, confidence, verdict, exact=True):
    for b, o in enumerate(outcomes):
        want_rgl = -1 if o.repair_given_location is None else int(o.repair_given_location)
        assert verdict[:, b].tolist() == [int(o.warned), int(o.location_correct), want_rgl, int(o.repaired)], b
        assert o.has_bug == (want_rgl >= 0)
        if exact:
            assert bits(float(confidence[b])) == bits(o.confidence), b


@pytest.mark.parametrize("family", FAMILIES)
def test_twin_equals_the_host_path(family):
    from buglab.models import _evaluate as E
    from buglab.models.evaluate import judge_sample

    data = _dataset(family)
    model, mb, ix, flat_size = _case(family, data)
    assert all(a.dtype == np.int32 for a in ix)
    if family.startswith("seq"):  # two reference nodes on one token: one flat index, two keys
        shared = [b for b in range(len(data)) if len(set(ix.loc_idx[ix.loc_off[b]:ix.loc_off[b + 1]].tolist())) < ix.loc_off[b + 1] - ix.loc_off[b]]
        assert shared
    warned = located = repaired = none_rewrite = 0
    for seed in range(6):
        rng = np.random.default_rng(seed)
        flat = _tied_values(rng, flat_size)
        flat[rng.uniform(size=flat_size) < (0.1 if seed < 4 else 0.6)] = -np.inf
        results = _unbatched_by_the_model(model, mb, data, flat)
        assert len(results) == len(data)
        for b, (point, loc, rw) in enumerate(results):  # the arrays name what predict yields
            lo, hi, r0, r1 = ix.loc_off[b], ix.loc_off[b + 1], ix.rw_off[b], ix.rw_off[b + 1]
            assert flat[ix.loc_idx[lo:hi]].tolist() == list(loc.values()) and flat[ix.rw_idx[r0:r1]].tolist() == rw
            nodes = np.unique(point["graph"]["reference_nodes"]).tolist()
            assert [nodes[k] if k >= 0 else -1 for k in ix.key_node[lo:hi].tolist()] == list(loc)
            assert [nodes[k] for k in ix.rw_node[r0:r1].tolist()] == list(point["graph"]["reference_nodes"])
            assert int(ix.tgt_rw[b]) == (-1 if point["target_fix_action_idx"] is None else point["target_fix_action_idx"])
        outcomes = [judge_sample(*t) for t in results]
        confidence, verdict = E.judge_host(flat, ix)
        assert confidence.dtype == np.float64 and verdict.dtype == np.int32 and verdict.shape == (4, len(data))
        _assert_same(outcomes, confidence, verdict)
        warned += sum(o.warned for o in outcomes)
        located += sum(o.location_correct for o in outcomes)
        repaired += sum(o.repaired and o.has_bug for o in outcomes)
        none_rewrite += sum(o.has_bug and o.location_correct and not o.repaired for o in outcomes)
    assert warned and located and repaired and none_rewrite  # the draws reach every branch


@pytest.mark.parametrize("family", FAMILIES)
def test_twin_with_assume_buggy(family):
    """integer fields equal; the host renormalises with torch's fp32 logsumexp and the twin in fp64: 1e-5 is fp32 rounding of a
    sum of at most 64 terms of magnitude <= 20"""
    from buglab.models import _evaluate as E
    from buglab.models.evaluate import judge_sample

    everything = _dataset(family, n=24)
    buggy = [d for d in everything if d["target_fix_action_idx"] is not None]
    assert len(buggy) >= 8
    model, mb, ix, flat_size = _case(family, buggy)
    assert int(np.diff(ix.loc_off).max()) <= 64
    for seed in range(3):
        rng = np.random.default_rng(10 + seed)
        flat = _tied_values(rng, flat_size, low=np.exp(-20.0))
        assert flat.min() >= -20.0 and flat.max() <= 0.0
        results = _unbatched_by_the_model(model, mb, buggy, flat)
        outcomes = [judge_sample(*t, assume_buggy=True) for t in results]
        confidence, verdict = E.judge_host(flat, ix, assume_buggy=True)
        _assert_same(outcomes, confidence, verdict, exact=False)
        assert all(o.warned for o in outcomes)
        worst = np.abs(confidence - np.array([o.confidence for o in outcomes])).max()
        print(f"\n[evaluate] {family} assume_buggy: worst |twin - host| confidence {worst:.3e}")
        assert worst <= 1e-5
    # a sample without a bug is refused, as the host path's assertion refuses it
    _, _, mixed, mixed_size = _case(family, everything[:4])
    assert (mixed.tgt_rw < 0).any()
    with pytest.raises(AssertionError):
        E.judge_host(np.zeros(mixed_size, np.float32), mixed, assume_buggy=True)
    # and so is one with nothing but NO_BUG to choose from
    alone = E.EvalIndices(*(np.asarray(a, np.int32) for a in ([0], [0, 1], [-1], [1], [0, 1], [0], [0])))
    with pytest.raises(ValueError):
        E.judge_host(np.zeros(2, np.float32), alone, assume_buggy=True)


def test_twin_rules_on_handcrafted_samples():
    """NaNs, all -inf, a target whose node has no key, an index outside src"""
    from buglab.models import _evaluate as E

    nan, inf = np.nan, np.inf
    #             0    1    2    3     4     5    6    7    8
    src = np.array([nan, -1.0, -0.5, -inf, -inf, -2.0, nan, -0.5, -3.0], np.float32)
    ix = lambda loc, key, rw, node, tgt: E.EvalIndices(*(np.asarray(a, np.int32) for a in (loc, [0, len(loc)], key, rw, [0, len(rw)], node, [tgt])))

    def run(*a):
        confidence, verdict = E.judge_host(src, ix(*a))
        return [float(confidence[0])] + verdict[:, 0].tolist()

    # a NaN in front wins the location; at its node every rewrite is -inf -> none; the target (same node) is not repaired
    conf, warned, loc_ok, rgl, rep = run([0, 2, 1], [0, 1, -1], [3, 4, 5], [0, 0, 1], 0)
    assert np.isnan(conf) and (warned, loc_ok, rgl, rep) == (1, 1, 0, 0)
    # a NaN elsewhere never wins; the tie -0.5 / -0.5 goes to the first key; a NaN rewrite never wins, the tie goes to the lower index
    conf, warned, loc_ok, rgl, rep = run([2, 0, 7, 1], [1, 0, 2, -1], [6, 7, 2, 8], [1, 1, 1, 0], 1)
    assert conf == -0.5 and (warned, loc_ok, rgl, rep) == (1, 1, 1, 1)
    conf, warned, loc_ok, rgl, rep = run([2, 0, 7, 1], [1, 0, 2, -1], [6, 7, 2, 8], [1, 1, 1, 0], 2)
    assert (warned, loc_ok, rgl, rep) == (1, 1, 0, 0)
    # the target's node (dense id 1) has no key: never location correct, its best rewrite is still found
    conf, warned, loc_ok, rgl, rep = run([2, 1], [0, -1], [5, 7, 8], [0, 1, 1], 1)
    assert conf == -0.5 and (warned, loc_ok, rgl, rep) == (1, 0, 1, 0)
    # NO_BUG predicted for correct code: location correct and "repaired" (none == none); for buggy code neither
    assert run([5, 2], [0, -1], [1], [0], -1)[1:] == [0, 1, -1, 1]
    assert run([5, 2], [0, -1], [1], [0], 0)[1:] == [0, 0, 1, 0]
    # only NO_BUG, no rewrites; an index outside src reads as NaN
    assert run([7], [-1], [], [], -1) == [-0.5, 0, 1, -1, 1]
    conf, warned, loc_ok, rgl, rep = run([99, 2], [0, -1], [5], [0], 0)
    assert np.isnan(conf) and (warned, loc_ok, rgl, rep) == (1, 1, 1, 1)


def _outcomes(case, assume_buggy):
    from buglab.models.evaluate import judge_sample

    return [judge_sample(d, {int(k): v for k, v in lp}, rw, assume_buggy) for d, lp, rw in case["predictions"]]


@pytest.mark.parametrize("eval_only_no_bug", [False, True])
@pytest.mark.parametrize("case", FIXTURE["cases"], ids=lambda c: c["name"])
def test_columnar_report_is_the_host_report(case, eval_only_no_bug):
    from buglab.models.evaluate import ColumnarEvaluationReport, EvaluationReport

    outcomes = _outcomes(case, case["flags"].get("--assume-buggy", False))
    host = EvaluationReport(outcomes, eval_only_no_bug)
    columns = ColumnarEvaluationReport.from_outcomes(outcomes, eval_only_no_bug)
    got, want = columns.summary(), host.summary()
    assert list(got) == list(want)
    for k in want:
        assert type(got[k]) is type(want[k]) and (got[k] == want[k] or (got[k] != got[k] and want[k] != want[k])), k
    assert columns.per_scout() == host.per_scout() and list(columns.per_scout()["localization"]) == list(host.per_scout()["localization"])
    assert len(columns.outcomes) == len(host.outcomes) and sorted(map(repr, columns.outcomes)) == sorted(map(repr, host.outcomes))
    if not host.outcomes:  # nothing to rank: both refuse alike
        with pytest.raises(ValueError):
            host.format()
        with pytest.raises(ValueError):
            columns.format()
        return
    assert columns.format() == host.format()


@pytest.mark.parametrize("eval_only_no_bug", [False, True])
def test_columnar_report_from_the_twins_columns(eval_only_no_bug):
    """the way `evaluate_on_device` builds it: columns from the judge, has_bug and scout ids from the host"""
    from buglab.models import _evaluate as E
    from buglab.models.evaluate import ColumnarEvaluationReport, EvaluationReport, judge_sample

    data = _dataset("gnn-mlp", n=30, seed=4)
    model, mb, ix, flat_size = _case("gnn-mlp", data)
    flat = _tied_values(np.random.default_rng(1), flat_size)
    outcomes = [judge_sample(*t) for t in _unbatched_by_the_model(model, mb, data, flat)]
    confidence, verdict = E.judge_host(flat, ix)
    names = ["NoBug"]
    scout = []
    for o in outcomes:
        if o.scout not in names:
            names.append(o.scout)
        scout.append(names.index(o.scout))
    columns = ColumnarEvaluationReport(confidence, [o.has_bug for o in outcomes], verdict[0] != 0, verdict[1] != 0, verdict[2],
                                       verdict[3] != 0, scout, names, eval_only_no_bug)
    assert columns.format() == EvaluationReport(outcomes, eval_only_no_bug).format()
    assert len(names) > 2  # several scouts, in an order that is not the sorted one the report prints
    assert names[1:] != sorted(names[1:]) or len(names) == 2


def test_on_device_refuses_ensembles():
    from buglab.models.ensemble.wrapper import EnsembleWrapper
    from buglab.models.evaluate import evaluate_on_device

    with pytest.raises(TypeError, match="ensembles"):
        evaluate_on_device(EnsembleWrapper.__new__(EnsembleWrapper), None, [], "cpu")


def test_c_entry_point_reports_argument_errors_without_a_gpu():
    import ctypes

    from buglab.models import hip_ops

    lib = hip_ops.load_library()
    err = lambda: lib.bl_last_error().decode()
    i, d, f = (ctypes.c_int32 * 8)(), (ctypes.c_double * 8)(), (ctypes.c_float * 8)()
    P = lambda a: ctypes.cast(a, ctypes.c_void_p)
    judge = lambda src, n_src, B, out, offset, capacity: lib.bl_eval_judge(src, n_src, P(i), P(i), P(i), 2, P(i), P(i), P(i), 2, P(i), B, 0,
                                                                             P(d), out, offset, capacity, None)
    assert judge(None, 8, 1, P(i), 0, 2) != 0 and "null" in err()
    assert judge(P(f), 8, 1, None, 0, 2) != 0 and "null" in err()
    assert judge(P(f), 8, -1, P(i), 0, 2) != 0 and "negative" in err()
    assert judge(P(f), 2 ** 31, 1, P(i), 0, 2) != 0 and "int32" in err()
    assert judge(P(f), 8, 2, P(i), 1, 2) != 0 and "do not fit" in err()
    assert judge(P(f), 8, 1, P(i), -1, 2) != 0 and "do not fit" in err()
    assert lib.bl_eval_judge(*([None, 0] + [None, None, None, 0] * 2 + [None, 0, 0, None, None, 0, 0, None])) == 0  # nothing to do
