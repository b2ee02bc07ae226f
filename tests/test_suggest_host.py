"""CPU: ranked suggestions without a GPU -- the NumPy twin of csrc/bl_suggest.hip (buglab/models/_suggest.py::rank_host) against
a literal Python restatement of the contract, `suggest_indices` on the models' real tensorise / collate path with the twin
against `suggestions_of_prediction` on the triples `_iter_per_sample_results` yields, the launcher's argument checks (before any
HIP call), `evaluate`'s host path with and without --top-k, and the suggestion tool's host path and records.

No tolerance anywhere: every output is an integer, a selected fp64 sum of two fp32 values, or a count."""
import ctypes
import gzip
import json
import math

import numpy as np
import pytest

from tests import suggest_cases as C
from tests.test_evaluate_golden import FIXTURE, _predictions
from tests.test_visualize_host import _minibatch, _model, _unbatched_by_the_model, bits

FAMILIES = ["gnn-mlp", "seq-great"]


# ------------------------------------------------------------------------------------------------ the twin
@pytest.mark.parametrize("skip_nobug", [False, True])
@pytest.mark.parametrize("k", [1, 5, 32])
def test_twin_equals_the_restatement_on_handcrafted_segments(k, skip_nobug):
    from buglab.models._suggest import rank_host

    src, ix, _ = C.handcrafted()
    C.assert_equal_bits(rank_host(src, ix, k, skip_nobug), C.restate(src, ix, k, skip_nobug))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_twin_equals_the_restatement_on_drawn_segments(seed):
    from buglab.models._suggest import rank_host

    src, ix = C.drawn(seed)
    for k, skip_nobug in ((1, False), (5, True), (32, False)):
        got = rank_host(src, ix, k, skip_nobug)
        C.assert_equal_bits(got, C.restate(src, ix, k, skip_nobug), (seed, k, skip_nobug))
    rank = got[0]
    assert (rank[0] == -1).any() and (rank[0] == 0).any() and (rank[0] > 1).any() and (rank[1] == -1).any() and (rank[1] > 0).any()


def test_the_rules_stated_once():
    """what the handmade samples are there for, as literal numbers, so that twin and restatement cannot share a mistake"""
    from buglab.models._suggest import rank_host

    src, ix, at = C.handcrafted()
    rank, entry, logprob = rank_host(src, ix, 5)
    skipped = rank_host(src, ix, 5, skip_nobug=True)
    row = lambda name, a=entry: a[at[name]].tolist()
    ranks = lambda name, r=rank: r[:, at[name]].tolist()
    inf = math.inf
    assert row("nobug_only") == [0, -1, -1, -1, -1] and row("nobug_only", logprob) == [-0.5, -inf, -inf, -inf, -inf]
    assert ranks("nobug_only") == [0, 0] and ranks("nobug_only", skipped[0]) == [-1, -1]
    assert row("nobug_only", skipped[1]) == [-1] * 5
    # rewrite 1 = -2.0 + -0.5, NO_BUG (entry 3) = -0.25
    assert row("few_rankable") == [3, 1, -1, -1, -1] and row("few_rankable", logprob)[:2] == [-0.25, -2.5]
    assert ranks("few_rankable") == [1, 2] and row("few_rankable", skipped[1]) == [1, -1, -1, -1, -1]
    assert ranks("few_rankable", skipped[0]) == [0, 1]
    assert row("tie_waves")[:4] == [63, 64, 256, 0] and ranks("tie_waves") == [1, 0]
    assert row("tie_all") == [0, 1, 2, 3, 4] and ranks("tie_all") == [4, 0]  # node 0's location: first of two equal ones
    assert ranks("tie_nobug_truth") == [6, 2]  # NO_BUG is the last entry: every equal one precedes it
    # rewrites 0 and 5 are at the NaN location, 1 is NaN, 3 is -inf, 4 is at the -inf location: only rewrite 2 and NO_BUG are left
    assert row("nan_inf") == [2, 6, -1, -1, -1] and row("nan_inf", logprob)[:2] == [-0.75, -1.5] and ranks("nan_inf") == [-1, -1]
    assert ranks("truth_not_rankable") == [-1, 0] and ranks("truth_nobug_not_rankable") == [-1, -1]
    assert ranks("no_bug") == [0, 0] and ranks("no_bug", skipped[0]) == [-1, -1]
    # rewrites 1 and 3 are at nodes without a key: NaN; rewrite 0 = -1.0, rewrite 2 = -1.2, NO_BUG (entry 4) = -2.0
    assert row("target_without_key") == [0, 2, 4, -1, -1] and ranks("target_without_key") == [-1, -1]
    assert ranks("target_out_of_range") == [-1, -1]
    assert row("out_of_range_indices") == [0, 4, -1, -1, -1] and ranks("out_of_range_indices") == [0, 0]
    with pytest.raises(ValueError):
        rank_host(src, ix, 0)
    with pytest.raises(ValueError):
        rank_host(src, ix, 33)


# ------------------------------------------------------------------------------------------------ the index arrays
def _dataset(family, n=14, seed=21):
    from buglab.data.synthetic import make_report_dataset

    return make_report_dataset(n, seed=seed, kind="seq" if family.startswith("seq") else "graph")


def _tied_values(rng, n):
    return (np.round(np.log(rng.uniform(0.02, 1.0, size=n)) * 2) / 2).astype(np.float32)


def _assert_ranked(ranked, rank, entry, logprob, b):
    listed = len(ranked.entries)
    assert entry[b, :listed].tolist() == ranked.entries and (entry[b, listed:] == -1).all(), b
    assert [bits(x) for x in logprob[b, :listed].tolist()] == [bits(x) for x in ranked.logprobs] and (logprob[b, listed:] == -np.inf).all(), b
    assert rank[:, b].tolist() == [ranked.truth_rank, ranked.truth_location_rank], b


@pytest.mark.parametrize("family", FAMILIES)
def test_indices_and_twin_equal_the_triples(family):
    from buglab.models import _evaluate as E
    from buglab.models import _suggest as S
    from buglab.models.basemodel import prediction_layout

    data = _dataset(family)
    model = _model(family, data)
    mb = _minibatch(model, data)
    layout = prediction_layout(mb)
    assert (mb.get("node_mappings") is not None) == family.startswith("seq")
    ix = S.suggest_indices(layout, data, mb.get("node_mappings"))
    assert all(a.dtype == np.int32 and a.flags["C_CONTIGUOUS"] for a in ix)
    ev = E.eval_indices(layout, data, mb.get("node_mappings"))
    for name in E.EvalIndices._fields:  # one upload serves both kernels
        assert getattr(ix, name).tolist() == getattr(ev, name).tolist(), name
    assert (ix.rw_loc_idx >= 0).all() and ix.nobug_idx.tolist() == ix.loc_idx[ix.loc_off[1:] - 1].tolist()
    seen = set()
    for seed in range(4):
        rng = np.random.default_rng(seed)
        flat = _tied_values(rng, layout.flat_size)
        flat[rng.uniform(size=layout.flat_size) < 0.1] = -np.inf
        results = _unbatched_by_the_model(model, mb, data, flat)
        for b, (point, loc, rw) in enumerate(results):  # rw_loc_idx names location_logprobs[reference_nodes[i]]
            r0, r1 = ix.rw_off[b], ix.rw_off[b + 1]
            assert flat[ix.rw_loc_idx[r0:r1]].tolist() == [loc[n] for n in point["graph"]["reference_nodes"]]
        for k, assume_buggy in ((1, False), (5, False), (5, True), (32, False)):
            rank, entry, logprob = S.rank_host(flat, ix, k, skip_nobug=assume_buggy)
            for b, triple in enumerate(results):
                ranked = S.suggestions_of_prediction(*triple, k, assume_buggy)
                _assert_ranked(ranked, rank, entry, logprob, b)
                seen.update(("none",) if ranked.truth_rank < 0 else ("first",) if ranked.truth_rank == 0 else ("later",))
                seen.update(("nobug",) if len(triple[0]["graph"]["reference_nodes"]) in ranked.entries else ())
    assert seen == {"none", "first", "later", "nobug"}  # the draws reach the branches


def test_a_reference_node_without_a_location_key():
    """no model of the registry leaves one out (`location_entries` asserts it), so the key is taken away here: the node's
    rewrites get rw_loc_idx -1, are NaN and never listed, and a target there has no rank -- as on the triple without that key"""
    from buglab.models import _report as R
    from buglab.models import _suggest as S
    from buglab.models.basemodel import prediction_layout

    data = _dataset("gnn-mlp", n=6)
    model = _model("gnn-mlp", data)
    mb = _minibatch(model, data)
    layout = prediction_layout(mb)
    loc_idx, keys = R.location_entries(layout, data, None)
    b = next(i for i, p in enumerate(data) if p["target_fix_action_idx"] is not None and len(keys[i]) > 2)
    gone = int(data[b]["graph"]["reference_nodes"][data[b]["target_fix_action_idx"]])
    j = keys[b].index(gone)
    keys = [list(ks) for ks in keys]
    del keys[b][j]
    at = int(layout.loc_off[b]) + j
    loc_off = layout.loc_off.copy()
    loc_off[b + 1:] -= 1
    ix = S.indices_from_keys(np.delete(loc_idx, at), loc_off, layout.rw_idx, layout.rw_off, data, keys)
    r0 = int(ix.rw_off[b])
    at_gone = np.asarray(data[b]["graph"]["reference_nodes"]) == gone
    assert ((ix.rw_loc_idx[r0:int(ix.rw_off[b + 1])] == -1) == at_gone).all() and at_gone.any()
    flat = _tied_values(np.random.default_rng(5), layout.flat_size)
    results = _unbatched_by_the_model(model, mb, data, flat)
    del results[b][1][gone]
    rank, entry, logprob = S.rank_host(flat, ix, 32)
    for i, triple in enumerate(results):
        _assert_ranked(S.suggestions_of_prediction(*triple, 32), rank, entry, logprob, i)
    assert rank[:, b].tolist() == [-1, -1] and not set(np.flatnonzero(at_gone).tolist()) & set(entry[b].tolist())


# ------------------------------------------------------------------------------------------------ the launcher's checks
def test_argument_errors_without_a_gpu():
    from buglab.models import hip_ops

    lib = hip_ops.load_library()
    f = (ctypes.c_float * 64)()
    d = (ctypes.c_double * 64)()
    i = (ctypes.c_int32 * 64)()
    fp, dp, ip = (ctypes.cast(x, ctypes.c_void_p) for x in (f, d, i))

    def call(src=fp, n_src=64, rw=(ip, ip, ip), total_rw=4, nobug=ip, tgt=ip, loc=(ip, ip, ip), total_loc=4, rw_node=ip, B=2, K=5, entry=ip,
             logprob=dp, rank=ip, offset=0, capacity=2):
        return lib.bl_rank_suggestions(src, n_src, rw[0], rw[1], rw[2], total_rw, nobug, tgt, loc[0], loc[1], loc[2], total_loc, rw_node, B, K,
                                       0, entry, logprob, rank, offset, capacity, None)

    EINVAL, ERANGE = -1, -2

    def refused(rc, want, *words):
        msg = lib.bl_last_error()
        assert rc == want, (rc, msg)
        for w in (b"bl_rank_suggestions",) + words:
            assert w in msg, (w, msg)

    refused(call(K=0), EINVAL, b"K = 0")
    refused(call(K=-3), EINVAL)
    refused(call(K=33), ERANGE, b"BL_SUGGEST_MAX_K")
    for null in ("src", "nobug", "tgt", "rw_node", "entry", "logprob", "rank"):
        refused(call(**{null: None}), EINVAL, b"null")
    refused(call(rw=(ip, None, ip)), EINVAL, b"null")
    refused(call(rw=(ip, ip, None)), EINVAL, b"null")
    refused(call(loc=(ip, ip, None)), EINVAL, b"null")
    refused(call(offset=1), EINVAL, b"do not fit")      # offset + B > capacity
    refused(call(capacity=1), EINVAL, b"do not fit")
    refused(call(offset=-1, capacity=8), EINVAL, b"do not fit")
    refused(call(B=-1), EINVAL, b"negative")
    refused(call(total_rw=-1), EINVAL, b"negative")
    refused(call(n_src=1 << 31), ERANGE, b"int32")
    refused(call(total_rw=(1 << 31) - 1), ERANGE, b"int32")  # NO_BUG's entry index would not fit
    assert call(B=0, capacity=0) == 0  # an empty minibatch is not an error -- and launches nothing
    assert hip_ops.SUGGEST_MAX_K == 32 and "rank_suggestions" in hip_ops.services.__all__


# ------------------------------------------------------------------------------------------------ evaluate --top-k, host path
def _point(nodes, scouts, target):
    return {"graph": {"reference_nodes": nodes}, "candidate_rewrite_metadata": [[s, 0] for s in scouts], "target_fix_action_idx": target}


def _small_predictions():
    """six samples whose ranks are counted by hand below (values are exact in fp32)"""
    A, B = "ScoutA", "ScoutB"
    return [
        # joint values: 3 -> -0.5-0.25, -0.5-2.0; 9 -> -1.0-0.125; NO_BUG -4.0.  The truth (rewrite 2) is second: rank 1; location 9 is second: 1
        (_point([3, 3, 9], [A, A, B], 2), {3: -0.5, 9: -1.0, -1: -4.0}, [-0.25, -2.0, -0.125]),
        # the truth (rewrite 0) is first; its location too
        (_point([3, 3, 9], [A, A, B], 0), {3: -0.5, 9: -1.0, -1: -4.0}, [-0.25, -2.0, -0.125]),
        # the truth (rewrite 1) is fourth of four: rank 3; location 3 is first: 0
        (_point([3, 3, 9], [A, A, B], 1), {3: -0.5, 9: -1.0, -1: -2.0}, [-0.25, -2.0, -0.125]),
        # no bug: NO_BUG (-0.75) ties with rewrite 0 and comes after it: rank 1; as a location it is second of three: 1
        (_point([3, 9], [A, B], None), {3: -0.5, 9: -3.0, -1: -0.75}, [-0.25, -0.125]),
        # no bug, NO_BUG first on both counts
        (_point([3, 9], [A, B], None), {3: -2.5, 9: -3.0, -1: -0.125}, [-0.25, -0.125]),
        # the truth's rewrite is -inf: no rank; its location 9 is first
        (_point([3, 9], [A, B], 1), {3: -2.5, 9: -0.25, -1: -3.0}, [-0.25, -math.inf]),
    ]


def test_evaluate_host_path_with_top_k():
    from buglab.models.evaluate import EvaluationReport, evaluate_predictions, judge_sample, report_to_json

    predictions = _small_predictions()
    plain = evaluate_predictions(predictions)
    report = evaluate_predictions(predictions, top_k=3)
    assert report.format() == plain.format()  # the report itself is unchanged ...
    text = report.format() + report.format_top_k()
    assert text.startswith(plain.format()) and len(text) > len(plain.format())  # ... and the block follows it
    s = report.top_k
    assert s["k"] == 3 and s["num_samples"] == {"all": 6, "buggy": 4, "correct": 2}
    # joint ranks 1 0 3 1 0 -1, location ranks 1 0 0 1 0 0
    assert s["joint"]["histogram"] == [[-1, 1], [0, 2], [1, 2], [3, 1]] and s["location"]["histogram"] == [[0, 4], [1, 2]]
    assert s["joint"]["within"] == {"all": [2, 4, 4], "buggy": [1, 2, 2], "correct": [1, 2, 2]}
    assert s["location"]["within"] == {"all": [4, 6, 6], "buggy": [3, 4, 4], "correct": [1, 2, 2]}
    assert s["joint"]["mrr"] == {"all": (0.5 + 1 + 0.25 + 0.5 + 1 + 0) / 6, "buggy": (0.5 + 1 + 0.25 + 0) / 4, "correct": 0.75}
    assert s["location"]["mrr"] == {"all": 5 / 6, "buggy": 3.5 / 4, "correct": 0.75}
    assert s["per_scout"] == {"ScoutA": {"joint": 1, "location": 2, "total": 2}, "ScoutB": {"joint": 1, "location": 2, "total": 2}}
    block = report.format_top_k()
    assert "Fix (Localization & Repair) within top 1: 33.33% (2/6)  buggy 25.00% (1/4)  non-buggy 50.00% (1/2)" in block
    assert "Location within top 2: 100.00% (6/6)  buggy 100.00% (4/4)  non-buggy 100.00% (2/2)" in block
    assert "Fix (Localization & Repair) mean reciprocal rank: 0.5417  buggy 0.4375  non-buggy 0.7500" in block
    assert "\tScoutA: 50.0% (1/2) | 100.0% (2/2)" in block and "not the Accuracy above" in block
    blob = json.loads(report_to_json(report))
    assert blob["top_k"] == s and {k: v for k, v in blob.items() if k != "top_k"} == json.loads(report_to_json(plain))
    # the report's own verdicts on the same samples, for the record: `repaired` is another question than joint rank 0
    assert [judge_sample(*t).repaired for t in predictions] == [False, True, False, False, True, False]
    # --eval-only-no-bug and --assume-buggy reach the ranking as they reach the judge
    clean = evaluate_predictions(predictions, eval_only_no_bug=True, top_k=2).top_k
    assert clean["num_samples"] == {"all": 2, "buggy": 0, "correct": 2} and clean["joint"]["within"]["all"] == [1, 2] and clean["per_scout"] == {}
    assert clean["joint"]["mrr"]["buggy"] != clean["joint"]["mrr"]["buggy"]  # NaN: no such sample
    buggy = evaluate_predictions([t for t in predictions if t[0]["target_fix_action_idx"] is not None], assume_buggy=True, top_k=1).top_k
    assert buggy["joint"]["histogram"] == [[-1, 1], [0, 1], [1, 1], [2, 1]]  # sample 2: NO_BUG no longer precedes the truth
    with pytest.raises(ValueError):
        evaluate_predictions(predictions, top_k=0)
    assert EvaluationReport([]).format_top_k() == ""


@pytest.mark.parametrize("case", FIXTURE["cases"], ids=lambda c: c["name"])
def test_evaluate_without_the_flag_is_todays_report(case):
    from buglab.models.evaluate import EvaluationReport, evaluate_predictions, judge_sample, report_to_json

    flags = case["flags"]
    assume_buggy, only_no_bug = flags.get("--assume-buggy", False), flags.get("--eval-only-no-bug", False)
    report = evaluate_predictions(_predictions(case), assume_buggy, only_no_bug)
    today = EvaluationReport([judge_sample(*t, assume_buggy) for t in _predictions(case)
                              if not (only_no_bug and t[0]["target_fix_action_idx"] is not None)])
    assert report.top_k is None and report.format_top_k() == ""
    assert report.format() + report.format_top_k() == today.format()
    assert report_to_json(report) == report_to_json(today) and "top_k" not in json.loads(report_to_json(report))
    if FIXTURE["numpy"] == np.__version__:  # same array printer: the text the reference's loop printed
        assert report.format() == case["report"]
    with_block = evaluate_predictions(_predictions(case), assume_buggy, only_no_bug, top_k=3)
    assert with_block.format() == today.format() and with_block.top_k["num_samples"]["all"] == today.summary()["num_samples"]


# ------------------------------------------------------------------------------------------------ the suggestion tool, host path
class _DrawnForward:
    """A real untrained gnn-mlp (its tensorise, collate and un-batching) whose forward is replaced by drawn values: this file
    runs without a GPU and the models have no CPU forward.  tests/test_suggest_gpu.py runs the real forward."""

    def __init__(self, model, reject):
        self.model, self.reject = model, reject

    def predict(self, data, trained_nn, device, parallelize):
        from buglab.models.basemodel import prediction_layout

        kept = [d for d in data if id(d) not in self.reject]
        for lo in range(0, len(kept), 5):
            points = kept[lo:lo + 5]
            mb = _minibatch(self.model, points)
            flat = _tied_values(np.random.default_rng(lo), prediction_layout(mb).flat_size)
            yield from _unbatched_by_the_model(self.model, mb, points, flat)


def test_suggest_host_path_and_records(tmp_path):
    from buglab.models import suggest as T

    data = _dataset("gnn-mlp", n=13)
    rejected_points = {id(data[4]), id(data[12])}
    model = _DrawnForward(_model("gnn-mlp", data), rejected_points)
    refused = []
    found = list(T.suggest(model, None, data, "cpu", 4, host=True, parallelize=False, rejected=refused.append))
    assert [s.position for s in found] == [0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11] and refused == [4, 12]  # input order
    assert all(s.datapoint is data[s.position] for s in found)
    records = [s.record() for s in found]
    out = tmp_path / "suggestions.jsonl.gz"
    assert T.write_records(records, out) == 11
    with gzip.open(out, "rt", encoding="utf-8") as f:
        read_back = [json.loads(line) for line in f]
    assert read_back == json.loads(json.dumps(records))
    labelled = 0
    for s, r in zip(found, records):
        point, n = s.datapoint, len(s.datapoint["graph"]["reference_nodes"])
        assert r["position"] == s.position and r["package"] == point["package_name"] and point["graph"]["path"].endswith(r["filename"])
        listed = r["suggestions"]
        assert 1 <= len(listed) <= 4 and [x["rank"] for x in listed] == list(range(len(listed)))
        probabilities = [x["probability"] for x in listed]
        assert probabilities == sorted(probabilities, reverse=True) and probabilities == [math.exp(x["logprob"]) for x in listed]
        assert r["mass"] == sum(probabilities)  # (drawn values are no distribution: `mass <= 1` is the next test's)
        for x in listed:
            if x["kind"] == "no_bug":
                assert x["rewrite_index"] is None and x["reference_node"] is None
            else:
                i = x["rewrite_index"]
                assert x["kind"] == "rewrite" and 0 <= i < n and x["reference_node"] == point["graph"]["reference_nodes"][i]
                assert x["candidate_rewrite"] == point["candidate_rewrites"][i] and x["candidate_rewrite_range"] == point["candidate_rewrite_ranges"][i]
                assert x["candidate_rewrite_metadata"] == point["candidate_rewrite_metadata"][i]
        # the truth's rank is consistent with the list
        truth = n if point["target_fix_action_idx"] is None else point["target_fix_action_idx"]
        entries = [n if x["kind"] == "no_bug" else x["rewrite_index"] for x in listed]
        assert r["target_fix_action_idx"] == point["target_fix_action_idx"]
        if 0 <= r["truth_rank"] < len(listed):
            assert entries[r["truth_rank"]] == truth
            labelled += 1
        else:
            assert truth not in entries
    assert labelled
    # --min-probability cuts the list, never the ranks
    everything = sorted(x["probability"] for r in records for x in r["suggestions"])
    least = everything[len(everything) // 2]
    cut = [s.record(min_probability=least) for s in found]
    assert all(all(x["probability"] >= least for x in r["suggestions"]) for r in cut)
    assert any(len(c["suggestions"]) < len(r["suggestions"]) for c, r in zip(cut, records))
    assert [(c["truth_rank"], c["truth_location_rank"]) for c in cut] == [(r["truth_rank"], r["truth_location_rank"]) for r in records]
    # a sample without a label carries no rank
    unlabelled = {k: v for k, v in data[0].items() if k != "target_fix_action_idx"}
    assert "truth_rank" not in T.suggestion_record(0, unlabelled, found[0].ranked)
    with pytest.raises(ValueError):
        T.suggest(model, None, data, "cpu", 33, host=True)


def test_mass_is_a_probability_when_the_values_are():
    """`mass <= 1` holds when the model's values are log-probabilities: location and rewrite log-softmaxes as the heads form
    them, here in NumPy.  The bound: an entry that matters has log-probabilities of magnitude below 20 (beyond that it adds less
    than e^-20), an fp32 value of that magnitude is off by at most 20 * 2^-24 = 1.2e-6 from rounding and by about as much from an
    fp32 log-sum-exp, and an entry adds two of them: each probability, and so the mass, is off by less than 5e-6 relative; the
    fp64 exp and the sum of at most 32 terms add 1e-14.  1e-5."""
    from buglab.models._suggest import suggestions_of_prediction
    from buglab.models.suggest import suggestion_record

    rng = np.random.default_rng(0)
    log_softmax = lambda x: x - np.log(np.exp(x).sum())
    for _ in range(20):
        nodes = sorted(rng.choice(50, size=int(rng.integers(1, 6)), replace=False).tolist())
        loc = log_softmax(rng.normal(size=len(nodes) + 1)).astype(np.float32)
        refs, rw = [], []
        for node in nodes:
            m = int(rng.integers(1, 5))
            refs += [node] * m
            rw += log_softmax(rng.normal(size=m)).astype(np.float32).tolist()
        point = {"graph": {"reference_nodes": refs, "path": "p.py"}, "package_name": "pkg", "candidate_rewrites": [None] * len(refs),
                 "candidate_rewrite_ranges": [None] * len(refs), "candidate_rewrite_metadata": [None] * len(refs), "target_fix_action_idx": None}
        ranked = suggestions_of_prediction(point, dict(zip(nodes + [-1], loc.tolist())), rw, 32)
        record = suggestion_record(0, point, ranked)
        assert len(refs) + 1 <= 32 and abs(record["mass"] - 1.0) <= 1e-5  # every entry is listed: the whole distribution
        assert suggestion_record(0, point, suggestions_of_prediction(point, dict(zip(nodes + [-1], loc.tolist())), rw, 3))["mass"] <= 1.0 + 1e-5
