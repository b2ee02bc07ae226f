"""CPU: the self-supervision services' host side (buglab.controllers; reference bugselectorserver.py,
detectordatascoringworker.py) -- the selection distribution and statistics against the reference's own
(tests/golden/selfsup_selection.json.gz, made by tests/golden/make_golden_selfsup.py), the services' gather indices against the
dict-based un-batching of `_iter_per_sample_results` plus the reference's formulas, the record handling of `score_rewrites`
around a model whose outputs are a lookup table, CLI arguments, and the two C entry points' argument errors."""
import contextlib
import copy
import ctypes
import gzip
import io
import json
import math
import os
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import selfsup_ref as R
from tests.conftest import ROOT

SEQ_SPEC = {"hidden_state_size": 32, "num_layers": 1, "num_heads": 4, "intermediate_dimension_size": 48, "dropout_rate": 0.1}

with gzip.open(os.path.join(ROOT, "tests", "golden", "selfsup_selection.json.gz"), "rt") as f:
    FIXTURE = json.load(f)


def _model(family, data):
    from buglab.models.modelregistry import load_model

    spec = dict(SEQ_SPEC, modelName=family) if family.startswith("seq") else {"modelName": family, "hidden_state_size": 32, "dropout_rate": 0.1}
    model = load_model(spec, Path("/tmp/_bl_selfsup_host.pkl.gz"))[0]
    model.compute_metadata(copy.deepcopy(data))
    return model


def _data(family, n, seed):
    from buglab.data.synthetic import make_buglab_dataset, make_buglab_seq_dataset

    return make_buglab_seq_dataset(n, seed=seed) if family.startswith("seq") else make_buglab_dataset(n, seed=seed)


# ------------------------------------------------------------------------------------------------------------------------------
def test_selection_distribution_equals_the_reference():
    from buglab.controllers.bugselector import calculate_selection_distribution

    assert len(FIXTURE["cases"]) > 100
    for case in FIXTURE["cases"]:
        with np.errstate(all="ignore"):
            got = np.asarray(calculate_selection_distribution(case["logprobs"], case["temperature"], case["epsilon"]), dtype=np.float64)
        want = np.asarray(case["distribution"], dtype=np.float64)
        assert got.shape == want.shape
        assert (np.isnan(got) == np.isnan(want)).all()
        fin = ~np.isnan(want)
        np.testing.assert_allclose(got[fin], want[fin], rtol=1e-15, atol=0)
        # the restatement the GPU tests compare the kernel with agrees too (vectorised exp, pairwise sum: a few ulp)
        mine = R.selection_distribution(case["logprobs"], case["temperature"], uniform=case["epsilon"] == 1.0)
        np.testing.assert_allclose(mine[fin], want[fin], rtol=1e-13, atol=0)


def test_selection_statistics_equal_the_reference():
    from buglab.controllers.bugselector import BugSelectionStats

    ref = FIXTURE["stats"]
    by_kernel, by_numpy = BugSelectionStats(), BugSelectionStats()
    for a in ref["added"]:
        p = np.asarray(FIXTURE["cases"][a["case"]]["distribution"])
        sample = {"candidate_rewrite_metadata": a["candidate_rewrite_metadata"]}
        by_numpy.add(sample, p, a["selected"])
        by_kernel.add(sample, None, a["selected"], entropy=R.entropy(p))  # what select_rewrites passes: the entropy alone
    for stats in (by_numpy, by_kernel):
        assert stats.total_samples == ref["state"]["total_samples"] == len(ref["added"]) > 20
        assert dict(stats.available_rewrite_frequency) == ref["state"]["available_rewrite_frequency"]  # exactly
        assert dict(stats.selected_rewrite_frequency) == ref["state"]["selected_rewrite_frequency"]
        assert stats.entropy_sum == pytest.approx(ref["state"]["entropy_sum"], rel=1e-12)
        assert stats.uniform_baseline_entropy_sum == pytest.approx(ref["state"]["uniform_baseline_entropy_sum"], rel=1e-12)
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            report = stats.report()
        assert out.getvalue() == ref["printed"]
        assert report == pytest.approx(ref["report"], rel=1e-12)
        assert stats.total_samples == 0 and not stats.available_rewrite_frequency  # report() resets, as the reference


def test_random_fallback_selection():
    import random

    from buglab.controllers.bugselector import select_random_rewrites

    got = select_random_rewrites(list(range(9)), 4, random.Random(1))
    assert got["NO_BUG"] == 0.1 and len(got) == 5 and set(got.values()) == {0.1}
    assert all(k == "NO_BUG" or 0 <= int(k) < 9 for k in got)
    assert select_random_rewrites([1, 2], 4, random.Random(1)) == {"NO_BUG": 1 / 3, "0": 1 / 3, "1": 1 / 3}  # fewer than 4: all of them
    assert select_random_rewrites([], 4) == {"NO_BUG": 1.0}


# ------------------------------------------------------------------------------------------------------------------------------
def _minibatch(model, graphs):
    with model._tensorize_all_location_rewrites():
        samples = [model.tensorize(g) for g in graphs]
        assert all(s is not None for s in samples)
        return model.collate_minibatch({"samples": samples})


def _unbatched_by_the_model(model, mb, graphs, flat):
    """`_iter_per_sample_results` (the dict-based un-batching every predict uses) on a flat output given as NumPy parts"""
    gd = mb["graph_data"]
    B = len(graphs)
    ids = np.concatenate([np.asarray(gd["reference_node_graph_idx"]["candidate_nodes"]).astype(np.int64), np.arange(B)])
    sizes = [ids.shape[0]] + [int(np.asarray(mb[k]).shape[0]) for k in
                              ("rewrite_to_location_group", "candidate_symbol_to_location_group", "swapped_pair_to_call_location_group")]
    assert sum(sizes) == flat.shape[0]
    loc, text, var, swap = np.split(flat, np.cumsum(sizes)[:-1])
    plain = {k: v for k, v in mb.items() if k != "prediction_layout"}
    return list(model._iter_per_sample_results(plain, ids, loc, swap, B, graphs, text, var, node_mappings=mb.get("node_mappings")))


@pytest.mark.parametrize("family", ["gnn-mlp", "seq-great"])
def test_gather_indices_pick_what_the_reference_formulas_pick(family):
    from buglab.controllers._batching import selfsup_indices
    from buglab.data.synthetic import make_scoring_records
    from buglab.models.basemodel import prediction_layout

    data = _data(family, 9, seed=12)
    model = _model(family, data)
    graphs = [g for r in make_scoring_records(data, seed=3) for g, _ in r["rewrites"].values()]
    assert any(g["target_fix_action_idx"] is None for g in graphs) and any(g["target_fix_action_idx"] is not None for g in graphs)
    mb = _minibatch(model, graphs)
    layout = prediction_layout(mb)
    ix = selfsup_indices(layout, graphs)
    flat = np.arange(layout.flat_size, dtype=np.float32)  # every value is its own index (exact in fp32)
    results = _unbatched_by_the_model(model, mb, graphs, flat)
    assert len(results) == len(graphs)
    for b, (point, loc, rw) in enumerate(results):
        r0, r1 = layout.rw_off[b], layout.rw_off[b + 1]
        # selector: rewrite_logprob + location_logprobs[reference node]; NO_BUG: location_logprobs[-1]
        want = R.selection_logprobs(point, loc, rw)
        got = (flat[layout.rw_idx[r0:r1]].astype(np.float64) + flat[ix.rw_loc_idx[r0:r1]]).tolist() + [float(flat[ix.nobug_idx[b]])]
        assert got == want
        assert [int(i) for i in ix.rw_loc_idx[r0:r1]] == [int(loc[n]) for n in point["graph"]["reference_nodes"]]
        # scoring: the true fix
        t = point["target_fix_action_idx"]
        assert int(ix.tgt_loc[b]) == int(loc[-1] if t is None else loc[point["graph"]["reference_nodes"][t]])
        assert int(ix.tgt_rw[b]) == (-1 if t is None else int(rw[t]))
        got_score = float(flat[ix.tgt_loc[b]]) + (float(flat[ix.tgt_rw[b]]) if ix.tgt_rw[b] >= 0 else 0.0)
        assert got_score == R.target_logprob(point, loc, rw)


# ------------------------------------------------------------------------------------------------------------------------------
class _LookupModule:
    def eval(self):
        return self


def _lookup_scoring(monkeypatch, model, records, parallelize=False):
    """score_rewrites on the CPU around a 'model' whose flat output is a lookup table (value = 0.25 * index - 100): the real
    tensorise / minibatch / collate path, the forward and the kernel replaced by NumPy.  -> (scored originals, {id(graph):
    expected score} from `_iter_per_sample_results` + the reference's formula on the same minibatches, minibatch sizes)"""
    from buglab.controllers import _batching as Bt
    from buglab.controllers.detectorscoring import score_rewrites
    from buglab.models import hip_ops

    seen, expected, sizes = {}, {}, []
    real_indices = Bt.selfsup_indices

    def indices(layout, points):
        seen[id(layout)] = points
        return real_indices(layout, points)

    def flat_output(nn_, mb):
        layout = mb["prediction_layout"]
        flat = np.arange(layout.flat_size, dtype=np.float32) * np.float32(0.25) - np.float32(100.0)
        points = seen.pop(id(layout))
        sizes.append(len(points))
        for point, loc, rw in _unbatched_by_the_model(model, mb, points, flat):
            expected[id(point)] = R.target_logprob(point, loc, rw)
        return torch.from_numpy(flat)

    def score_targets(src, tgt_loc, tgt_rw):
        s = src.double()
        return s[tgt_loc.long()] + torch.where(tgt_rw >= 0, s[tgt_rw.clamp(min=0).long()], torch.zeros((), dtype=torch.float64))

    monkeypatch.setattr(Bt, "selfsup_indices", indices)
    monkeypatch.setattr(Bt, "flat_prediction_output", flat_output)
    monkeypatch.setattr(hip_ops, "score_targets", score_targets)
    out = list(score_rewrites(model, _LookupModule(), iter(records), "cpu", parallelize=parallelize))
    return out, expected, sizes


@pytest.mark.parametrize("parallelize", [False, True])
def test_score_rewrites_record_handling(monkeypatch, caplog, parallelize):
    from buglab.data.synthetic import make_scoring_records

    data = _data("gnn-mlp", 30, seed=8)
    model = _model("gnn-mlp", data)
    records = make_scoring_records(data, seed=5)  # 30 records x (NO_BUG + 4 rewrites) = 150 graphs: three minibatches of 50
    assert all(len(r["rewrites"]) == 5 for r in records)
    rejected = records[2]["rewrites"][list(records[2]["rewrites"])[1]][0]
    none_key = list(records[4]["rewrites"])[2]
    records[4]["rewrites"][none_key] = (None, 0.1)
    records[6]["rewrites"] = {}                     # nothing to score: every slot -inf
    del records[7]["rewrites"]["NO_BUG"]
    real_tensorize = model.tensorize
    monkeypatch.setattr(model, "tensorize", lambda d: None if d is rejected else real_tensorize(d))
    with caplog.at_level("ERROR"):
        out, expected, sizes = _lookup_scoring(monkeypatch, model, records, parallelize)
    assert "None element for graph" in caplog.text and str(none_key) in caplog.text
    assert [o is r["original"] for o, r in zip(out, records)] == [True] * len(records)  # every record, in input order
    assert sizes[0] == 50 and len(sizes) == 3 and sum(sizes) == 150 - 8  # 1 rejected, 1 None, 5 + 1 removed; records span minibatches
    for k, (original, record) in enumerate(zip(out, records)):
        scores = original["candidate_rewrite_logprobs"]
        n = len(original["graph"]["reference_nodes"])
        assert len(scores) == n + 1
        want = [-math.inf] * (n + 1)
        for key, (graph, _) in record["rewrites"].items():
            if graph is None or graph is rejected:
                continue
            want[-1 if key == "NO_BUG" else int(key)] = expected[id(graph)]
        assert scores == want, k
        assert all(isinstance(v, float) for v in scores)
    assert out[6]["candidate_rewrite_logprobs"] == [-math.inf] * (len(out[6]["graph"]["reference_nodes"]) + 1)
    assert out[7]["candidate_rewrite_logprobs"][-1] == -math.inf
    assert sum(math.isfinite(v) for v in out[0]["candidate_rewrite_logprobs"]) == 5


def test_score_rewrites_rejects_duplicate_and_foreign_indices(monkeypatch):
    from buglab.data.synthetic import make_scoring_records

    data = _data("gnn-mlp", 2, seed=8)
    model = _model("gnn-mlp", data)
    rec = make_scoring_records(data, seed=5)[0]
    first = next(k for k in rec["rewrites"] if k != "NO_BUG")
    dup = {"original": rec["original"], "rewrites": dict(rec["rewrites"], **{"0" + first: rec["rewrites"][first]})}  # "03" and "3"
    with pytest.raises(ValueError, match="duplicate"):
        _lookup_scoring(monkeypatch, model, [dup])
    foreign = {"original": rec["original"], "rewrites": {"999": rec["rewrites"][first]}}
    with pytest.raises(ValueError, match="outside"):
        _lookup_scoring(monkeypatch, model, [foreign])


def test_ensembles_are_refused():
    from buglab.controllers.bugselector import select_rewrites
    from buglab.controllers.detectorscoring import score_rewrites
    from buglab.models.ensemble.wrapper import EnsembleWrapper

    member = type("M", (), {"predict": lambda *a: iter(())})()
    ens = EnsembleWrapper([member], "avg")
    with pytest.raises(TypeError, match="ensembles"):
        next(score_rewrites(ens, _LookupModule(), [], "cpu"))
    with pytest.raises(TypeError, match="ensembles"):
        next(select_rewrites(ens, _LookupModule(), [], "cpu"))


def test_scored_records_round_trip_through_files_reproducibly(tmp_path):
    from buglab.controllers._batching import save_msgpack_l_gz_reproducibly
    from buglab.controllers.detectorscoring import load_records
    from buglab.data.synthetic import make_scoring_records

    records = make_scoring_records(_data("gnn-mlp", 3, seed=1), seed=2)
    save_msgpack_l_gz_reproducibly(records, tmp_path / "a.msgpack.l.gz")
    save_msgpack_l_gz_reproducibly(records, tmp_path / "b.msgpack.l.gz")
    assert (tmp_path / "a.msgpack.l.gz").read_bytes() == (tmp_path / "b.msgpack.l.gz").read_bytes()
    back = list(load_records(tmp_path))
    assert len(back) == 6 and list(back[0]["rewrites"]) == list(records[0]["rewrites"])
    graph, prob = back[0]["rewrites"]["NO_BUG"]
    assert graph["target_fix_action_idx"] is None and prob == records[0]["rewrites"]["NO_BUG"][1]


# ------------------------------------------------------------------------------------------------------------------------------
def test_cli_arguments():
    from buglab.controllers import bugselector, detectorscoring

    a = bugselector.parse_args(["m.pkl.gz", "data", "out.msgpack.l.gz"])
    assert (a.num_rewrites_per_sample, a.temperature_scaling, a.epsilon, a.seed, a.sequential) == (4, 1.0, 0.02, None, False)
    a = bugselector.parse_args(["m.pkl.gz", "data", "out.msgpack.l.gz", "--num-rewrites-per-sample", "7", "--temperature-scaling", "2.5",
                                "--epsilon", "0", "--seed", "11", "--sequential"])
    assert (a.MODEL_FILENAME, a.DATA_PATH, a.OUT_FILENAME) == ("m.pkl.gz", "data", "out.msgpack.l.gz")
    assert (a.num_rewrites_per_sample, a.temperature_scaling, a.epsilon, a.seed, a.sequential) == (7, 2.5, 0.0, 11, True)
    b = detectorscoring.parse_args(["m.pkl.gz", "records", "out.msgpack.l.gz", "--sequential"])
    assert (b.MODEL_FILENAME, b.RECORDS_PATH, b.OUT_FILENAME, b.sequential) == ("m.pkl.gz", "records", "out.msgpack.l.gz", True)
    with pytest.raises(SystemExit):
        detectorscoring.parse_args(["m.pkl.gz"])
    with pytest.raises(SystemExit):
        bugselector.parse_args(["m.pkl.gz", "data", "out", "--num-rewrites-per-sample", "many"])


def test_select_rewrites_checks_its_arguments():
    from buglab.controllers.bugselector import select_rewrites

    data = _data("gnn-mlp", 2, seed=8)
    model = _model("gnn-mlp", data)
    with pytest.raises(ValueError, match="num_rewrites_per_sample"):
        next(select_rewrites(model, _LookupModule(), data, "cpu", num_rewrites_per_sample=33))
    with pytest.raises(ValueError, match="num_rewrites_per_sample"):
        next(select_rewrites(model, _LookupModule(), data, "cpu", num_rewrites_per_sample=0))
    with pytest.raises(ValueError, match="temperature"):
        next(select_rewrites(model, _LookupModule(), data, "cpu", temperature=0.0))


def test_c_entry_points_report_argument_errors_without_a_gpu():
    from buglab.models import hip_ops

    lib = hip_ops.load_library()
    f = (ctypes.c_float * 8)()
    i = (ctypes.c_int32 * 8)()
    d = (ctypes.c_double * 16)()
    P = lambda a: ctypes.cast(a, ctypes.c_void_p)
    err = lambda: lib.bl_last_error().decode()
    EINVAL, ERANGE = -1, -2

    assert lib.bl_score_targets(None, 8, P(i), P(i), 2, P(d), None) == EINVAL and "null" in err()
    assert lib.bl_score_targets(P(f), 8, P(i), None, 2, P(d), None) == EINVAL and "null" in err()
    assert lib.bl_score_targets(P(f), 8, P(i), P(i), 2, None, None) == EINVAL and "null" in err()
    assert lib.bl_score_targets(P(f), 8, P(i), P(i), -1, P(d), None) == EINVAL and "negative" in err()
    assert lib.bl_score_targets(P(f), -8, P(i), P(i), 1, P(d), None) == EINVAL and "negative" in err()
    assert lib.bl_score_targets(P(f), 2 ** 31, P(i), P(i), 1, P(d), None) == ERANGE and "int32" in err()
    assert lib.bl_score_targets(None, 0, None, None, 0, None, None) == 0  # nothing to do

    def sample(src=P(f), n_src=8, rw_idx=P(i), rw_loc=P(i), rw_off=P(i), total_rw=2, nobug=P(i), B=1, u_eps=P(d), u=P(d), T=1.0, eps=0.0,
               K=4, lp=P(d), p=P(d), ent=P(d), sel=P(i)):
        return lib.bl_selector_sample(src, n_src, rw_idx, rw_loc, rw_off, total_rw, nobug, B, u_eps, u, T, eps, K, lp, p, ent, sel, None)

    assert sample(K=33) == ERANGE and "at most 32" in err()
    assert sample(K=0) == EINVAL and "at least 1" in err()
    assert sample(B=-1) == EINVAL and "negative" in err()
    assert sample(total_rw=-2) == EINVAL and "negative" in err()
    assert sample(n_src=-1) == EINVAL and "negative" in err()
    assert sample(T=0.0) == EINVAL and "temperature" in err()
    assert sample(T=float("nan")) == EINVAL and "temperature" in err()
    for name in ("src", "rw_off", "nobug", "u_eps", "u", "lp", "p", "ent", "sel", "rw_idx", "rw_loc"):
        assert sample(**{name: None}) == EINVAL and "null" in err(), name
    assert sample(n_src=2 ** 31) == ERANGE and "int32" in err()
    assert sample(B=0, src=None, rw_off=None) == 0
