"""CPU: the bug report (buglab/models/visualize.py, buglab/models/_report.py, buglab/utils/text.py) against the contexts
recorded from the reference (tests/golden/visualize_contexts.json.gz, made by tests/golden/make_golden_visualize.py): strings
equal, floats bit-equal, snippet order equal; and `report_indices` against the dict-based restatement of
tests/visualize_ref.py, which the same fixture pins."""
import copy
import gzip
import json
import os
import struct
from html.parser import HTMLParser
from pathlib import Path

import numpy as np
import pytest

from tests import visualize_ref as VR
from tests.conftest import ROOT

SEQ_SPEC = {"hidden_state_size": 32, "num_layers": 1, "num_heads": 4, "intermediate_dimension_size": 48, "dropout_rate": 0.1}
FLAGS = [(False, False), (False, True), (True, False), (True, True)]

with gzip.open(os.path.join(ROOT, "tests", "golden", "visualize_contexts.json.gz"), "rt") as f:
    FIXTURE = json.load(f)


def fixture_predictions():
    return [(s["datapoint"], dict(zip(s["location_keys"], s["location_logprobs"])), list(s["rewrite_logprobs"])) for s in FIXTURE["samples"]]


def bits(x):
    return struct.pack("<d", x)


def assert_same_context(got, want, where):
    """strings equal, floats bit-equal; plain segments without text carry nothing (the recording cannot tell them from the gap
    between two annotated segments) and are dropped on both sides; within a segment the ranges are compared as sets"""
    assert set(got) == set(want), where
    for k in ("filename", "package", "target_action", "no_bug_prob", "prediction_prob"):
        assert got[k] == want[k] and isinstance(got[k], str), (where, k)
    assert got["is_wrong"] is want["is_wrong"], where
    assert bits(got["prediction_logprob"]) == bits(want["prediction_logprob"]), where
    seg = lambda c: [s for s in c["segments"] if "target_ranges" in s or s["text"]]
    gs, ws = seg(got), seg(want)
    assert [s["text"] for s in gs] == [s["text"] for s in ws], where
    for a, b in zip(gs, ws):
        assert set(a) == set(b), where
        if "target_ranges" not in a:
            continue
        assert a["contains_ground_range"] is b["contains_ground_range"] and a["contains_predicted_range"] is b["contains_predicted_range"]
        ta, tb = (sorted(s["target_ranges"], key=lambda t: t["range"]) for s in (a, b))
        assert [t["range"] for t in ta] == [t["range"] for t in tb], where
        for x, y in zip(ta, tb):
            assert set(x) == set(y)
            assert bits(x["best_range_logprob"]) == bits(y["best_range_logprob"]), (where, x["range"])
            for k in ("assigned_prob", "rewrites", "is_ground_range", "is_predicted_range"):
                assert x[k] == y[k], (where, x["range"], k)
            assert all(type(r["is_correct"]) is bool and type(r["is_predicted"]) is bool for r in x["rewrites"])


def test_fixture_has_the_cases_it_promises():
    samples, contexts = FIXTURE["samples"], FIXTURE["contexts"]
    assert len(samples) == len(contexts) >= 40
    assert any(len(s["rewrite_logprobs"]) >= 3000 for s in samples)
    assert any(s["datapoint"]["target_fix_action_idx"] is None for s in samples)
    assert any(c["is_wrong"] for c in contexts) and any(not c["is_wrong"] for c in contexts)
    assert any("/site-packages/" in s["datapoint"]["graph"]["path"] for s in samples)
    assert any(s["location_keys"][:-1] != sorted(s["location_keys"][:-1]) for s in samples)  # a sequence model's key order
    assert any(len(set(s["location_logprobs"])) < len(s["location_logprobs"]) for s in samples)  # exact ties
    assert all(s["location_keys"][-1] == -1 for s in samples)
    everything = list(range(len(samples)))
    assert FIXTURE["runs"]["only_incorrect=0,order_by_confidence=0"] == everything
    assert sorted(FIXTURE["runs"]["only_incorrect=0,order_by_confidence=1"]) == everything
    assert FIXTURE["runs"]["only_incorrect=1,order_by_confidence=0"] == [i for i in everything if contexts[i]["is_wrong"]]


@pytest.mark.parametrize("only_incorrect,by_confidence", FLAGS)
def test_contexts_equal_the_reference(only_incorrect, by_confidence):
    from buglab.models.visualize import predictions_to_report

    want = FIXTURE["runs"][f"only_incorrect={int(only_incorrect)},order_by_confidence={int(by_confidence)}"]
    report = predictions_to_report(fixture_predictions(), only_incorrect, by_confidence)
    assert report.selected.tolist() == want  # snippet order
    assert report.is_wrong.tolist() == [c["is_wrong"] for c in FIXTURE["contexts"]]
    assert [bits(x) for x in report.prediction_logprob.tolist()] == [bits(c["prediction_logprob"]) for c in FIXTURE["contexts"]]
    assert len(report.snippets) == len(want)
    for ctx, i in zip(report.snippets, want):
        assert_same_context(ctx, FIXTURE["contexts"][i], FIXTURE["samples"][i]["name"])


@pytest.mark.parametrize("only_incorrect,by_confidence", FLAGS)
def test_the_restatement_equals_the_reference(only_incorrect, by_confidence):
    want = FIXTURE["runs"][f"only_incorrect={int(only_incorrect)},order_by_confidence={int(by_confidence)}"]
    contexts, shown, _ = VR.report(fixture_predictions(), only_incorrect, by_confidence)
    assert shown == want
    for ctx, i in zip(contexts, want):
        assert_same_context(ctx, FIXTURE["contexts"][i], FIXTURE["samples"][i]["name"])


def test_top_k_cuts_after_ordering():
    from buglab.models.visualize import predictions_to_report

    full = FIXTURE["runs"]["only_incorrect=1,order_by_confidence=1"]
    for k in (1, 5, len(full), len(full) + 5):
        assert predictions_to_report(fixture_predictions(), True, True, show_top_k=k).selected.tolist() == full[:k]
    assert predictions_to_report(fixture_predictions(), False, False, show_top_k=3).selected.tolist() == [0, 1, 2]
    assert predictions_to_report([], True, True).snippets == []


def test_text_segments_equal_the_recorded_segmentation():
    from buglab.utils.text import get_text_in_range, text_to_range_segments

    for s in FIXTURE["samples"]:
        p = s["datapoint"]
        got = text_to_range_segments(p["graph"]["text"], p["graph"]["code_range"], p["candidate_rewrite_ranges"])
        assert [[t, [[list(a), list(b)] for a, b in r]] for t, r in got] == s["segmentation"], s["name"]
        assert "".join(t for t, _ in got) == p["graph"]["text"]
    text = "ab\ncd\rX\nef"
    assert get_text_in_range(text, ((1, 1), (1, 2))) == "b" and get_text_in_range(text, ((1, 1), (2, 3))) == "b\ncd\r"
    assert get_text_in_range(text, ((0, 0), (3, 1))) == "ab\ncd\rX\ne" and get_text_in_range(text, ((2, 2), (float("inf"), float("inf")))) == "\rX\nef"
    assert get_text_in_range(text, ((5, 0), (6, 1))) == ""


def test_order_host_equals_pythons_stable_sort():
    from buglab.models._report import order_host

    rng = np.random.default_rng(5)
    for n in (0, 1, 2, 63, 500):
        for density in (0.0, 0.3, 1.0):
            keys = np.round(rng.normal(size=n) * 2) / 2  # many ties
            keys[rng.uniform(size=n) < 0.2] = -np.inf
            keep = (rng.uniform(size=n) < density).astype(np.int32)
            kept = [i for i in range(n) if keep[i]]
            want = sorted(kept, key=lambda i: -keys[i])
            for k in (0, 1, n, n + 5):
                assert order_host(keys, keep, True, k).tolist() == (want[:k] if k > 0 else want)
                assert order_host(keys, keep, False, k).tolist() == (kept[:k] if k > 0 else kept)
    assert order_host([1.0, np.nan, -np.inf, 2.0, np.nan], [1] * 5, True).tolist() == [3, 0, 2, 1, 4]  # NaN: after -inf, input order


# ------------------------------------------------------------------------------------------------------------------------------
class _Blocks(HTMLParser):
    """the page as nested (tag, classes, text) records per snippet"""

    def __init__(self):
        super().__init__(convert_charrefs=True)
        self.stack, self.snippets, self.texts = [], [], []

    def handle_starttag(self, tag, attrs):
        cls = dict(attrs).get("class", "").split()
        if tag == "section" and "snippet" in cls:
            self.snippets.append({"classes": cls, "items": []})
        if tag not in ("meta", "br"):
            self.stack.append((tag, cls, []))

    def handle_endtag(self, tag):
        assert self.stack and self.stack[-1][0] == tag, (tag, [s[0] for s in self.stack])
        t, cls, text = self.stack.pop()
        if self.snippets and t != "section":
            self.snippets[-1]["items"].append((t, cls, "".join(text)))

    def handle_data(self, data):
        for _, _, text in self.stack:
            text.append(data)


def test_html_shows_every_context():
    from buglab.models.visualize import predictions_to_html, predictions_to_report, report_to_html

    report = predictions_to_report(fixture_predictions(), True, True)
    page = predictions_to_html(fixture_predictions(), True, True)
    assert page == report_to_html(report.snippets) and page.startswith("<!DOCTYPE html>")
    parser = _Blocks()
    parser.feed(page)
    parser.close()
    assert not parser.stack
    assert len(parser.snippets) == len(report.snippets) > 10
    for block, ctx in zip(parser.snippets, report.snippets):
        items = block["items"]
        one = lambda cls: [text for _, c, text in items if cls in c]
        assert one("package") == [ctx["package"]] and one("filename") == [ctx["filename"]]
        assert (one("mistake") != []) == ctx["is_wrong"] == ("wrong" in block["classes"])
        assert one("no-bug-prob") == [ctx["no_bug_prob"]] and one("target-action") == [ctx["target_action"]]
        assert one("prediction-prob") == [ctx["prediction_prob"]]
        code = [text for tag, c, text in items if tag == "pre" and "code" in c]
        annotated = [s for s in ctx["segments"] if "target_ranges" in s]
        assert len(code) == 1 and len(one("seg")) == len(annotated) == len(one("segment"))
        assert one("segment-text") == [s["text"] for s in annotated]
        ranges = [t for s in annotated for t in s["target_ranges"]]
        assert one("range-span") == [t["range"] for t in ranges] and one("assigned-prob") == [t["assigned_prob"] for t in ranges]
        tables = [text for tag, c, text in items if tag == "caption"]
        assert len(tables) == len(ranges)
        assert ["ground truth" in t for t in tables] == [t["is_ground_range"] for t in ranges]
        rows = [r for t in ranges for r in t["rewrites"]]
        assert one("rewrite") == [r["rewrite"] for r in rows] and one("prob") == [r["prob"] for r in rows]
        flags = one("flags")
        assert ["correct" in f for f in flags] == [r["is_correct"] for r in rows]
        assert ["predicted" in f for f in flags] == [r["is_predicted"] for r in rows]
    # everything that comes from the data is escaped: the text holds <, & and quotes
    assert any("<" in s["text"] and "&" in s["text"] for c in report.snippets for s in c["segments"])
    body = predictions_to_html(fixture_predictions(), True, True, include_header=False)
    assert "<html" not in body and body.count("<section") == len(report.snippets)
    assert predictions_to_html(fixture_predictions(), True, True, show_top_k=2).count("<section") == 2


# ------------------------------------------------------------------------------------------------------------------------------
def _model(family, data):
    from buglab.models.modelregistry import load_model

    spec = dict(SEQ_SPEC, modelName=family) if family.startswith("seq") else {"modelName": family, "hidden_state_size": 32, "dropout_rate": 0.1}
    model = load_model(spec, Path("/tmp/_bl_visualize_host.pkl.gz"))[0]
    model.compute_metadata(copy.deepcopy(data))
    return model


def _minibatch(model, graphs):
    with model._tensorize_all_location_rewrites():
        samples = [model.tensorize(g) for g in graphs]
        assert all(s is not None for s in samples)
        return model.collate_minibatch({"samples": samples})


def _unbatched_by_the_model(model, mb, graphs, flat):
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
def test_report_indices_equal_the_restatement(family):
    """the real tensorise / collate path of the model; a flat output drawn from a coarse grid (exact ties); every array of
    `report_indices` against the dicts of visualize_ref, and the NumPy twin of the kernel against its report"""
    from buglab.data.synthetic import make_report_dataset
    from buglab.models import _report as R
    from buglab.models.basemodel import prediction_layout

    data = make_report_dataset(14, seed=21, kind="seq" if family.startswith("seq") else "graph")
    shapes = [r for p in data for r in p["candidate_rewrite_ranges"]]
    assert any(a == b for a, b in shapes) and any(a[0] != b[0] for a, b in shapes)  # empty and multi-line ranges
    assert all(p["graph"]["code_range"][0][0] > 1 and p["graph"]["code_range"][0][1] > 0 and "\n" in p["graph"]["text"] for p in data)
    model = _model(family, data)
    mb = _minibatch(model, data)
    layout = prediction_layout(mb)
    ix, groups, keys = R.report_indices(layout, data, mb.get("node_mappings"))
    rng = np.random.default_rng(3)
    flat = (np.round(np.log(rng.uniform(0.02, 1.0, size=layout.flat_size)) * 4) / 4).astype(np.float32)
    results = _unbatched_by_the_model(model, mb, data, flat)
    assert len(results) == len(data)
    hidden = 0
    for b, (point, loc, rw) in enumerate(results):
        assert list(loc) == keys[b]  # the key order of the dict predict yields
        lo, hi, r0, r1, g0, g1 = ix.loc_off[b], ix.loc_off[b + 1], ix.rw_off[b], ix.rw_off[b + 1], ix.grp_off[b], ix.grp_off[b + 1]
        assert flat[ix.loc_idx[lo:hi]].tolist() == list(loc.values()) and flat[ix.rw_idx[r0:r1]].tolist() == rw
        assert flat[ix.nobug_idx[b]] == loc[-1]
        want = VR.sample_arrays(point, list(loc))
        assert ix.rw_grp[r0:r1].tolist() == want["rw_grp"] and ix.rw_eq_target[r0:r1].tolist() == want["rw_eq_target"]
        assert ix.grp_loc[g0:g1].tolist() == want["grp_loc"] and ix.grp_shown[g0:g1].tolist() == want["grp_shown"]
        assert int(ix.tgt_grp[b]) == want["tgt_grp"] and int(ix.ground_loc[b]) == want["ground_loc"]
        hidden += want["grp_shown"].count(0)
        for g in range(g0, g1):  # the CSR is the grouping again: the group's rewrites, ascending
            members = ix.grp_rw[ix.grp_rw_off[g]:ix.grp_rw_off[g + 1]]
            assert (members - r0).tolist() == [i for i, x in enumerate(want["rw_grp"]) if x == g - g0]
    assert hidden > 0  # colliding ranges occur
    assert int(ix.grp_rw_off[-1]) == int(ix.rw_off[-1]) and all(a.dtype == np.int32 for a in ix)
    # summarize_host on these arrays == the restatement's report
    best_rw, best_range, si, sd = R.summarize_host(flat, ix)
    _, _, everything = VR.report(results)
    assert si[2].tolist() == [int(c["is_wrong"]) for c in everything]
    assert [bits(x) for x in sd[0].tolist()] == [bits(c["prediction_logprob"]) for c in everything]
    for b, (point, loc, rw) in enumerate(results):
        assert int(si[0, b]) == list(loc).index(max(loc, key=loc.get)) and float(sd[1, b]) == loc[-1]
        assert int(si[1, b]) == int(max(loc, key=loc.get) == -1)


def test_scan_refuses_ensembles_and_cli_arguments():
    from buglab.models import visualize
    from buglab.models.ensemble.wrapper import EnsembleWrapper

    with pytest.raises(TypeError, match="ensembles"):
        visualize.scan(EnsembleWrapper.__new__(EnsembleWrapper), None, [], "cpu")
    a = visualize.parse_args(["m.pkl.gz", "data", "out.html"])
    assert (a.num_elements, a.sample_pct, a.show_only_top_k, a.only_incorrect, a.order_by_confidence, a.only_no_bug, a.report_json) == \
        (1000, 1.0, 0, False, False, False, None)
    a = visualize.parse_args(["--only-incorrect", "--order-by-confidence", "--show-only-top-k", "50", "--num-elements=20", "--sequential",
                              "--report-json", "r.json", "--minibatch-size", "10", "--quiet", "--debug", "m", "d", "o"])
    assert a.only_incorrect and a.order_by_confidence and a.show_only_top_k == 50 and a.num_elements == 20 and a.report_json == "r.json"
    with pytest.raises(SystemExit):
        visualize.parse_args(["--aml", "m", "d", "o"])
    assert "ensembles" in visualize.__doc__


def test_c_entry_points_report_argument_errors_without_a_gpu():
    import ctypes

    from buglab.models import hip_ops

    lib = hip_ops.load_library()
    err = lambda: lib.bl_last_error().decode()
    i, d, f = (ctypes.c_int32 * 8)(), (ctypes.c_double * 8)(), (ctypes.c_float * 8)()
    P = lambda a: ctypes.cast(a, ctypes.c_void_p)
    summarize = lambda src, n_src, B, out_i: lib.bl_report_summarize(src, n_src, P(i), P(i), 2, P(i), P(i), 2, P(i), P(i), P(i), P(i), P(i), P(i), 1,
                                                                       P(i), P(i), P(i), B, P(i), P(d), out_i, P(d), None)
    assert summarize(None, 8, 1, P(i)) != 0 and "null" in err()
    assert summarize(P(f), 8, 1, None) != 0 and "null" in err()
    assert summarize(P(f), 8, -1, P(i)) != 0 and "negative" in err()
    assert summarize(P(f), 2 ** 31, 1, P(i)) != 0 and "int32" in err()
    assert lib.bl_report_summarize(*([None, 0] + [None, None, 0] * 2 + [None] * 6 + [0] + [None] * 3 + [0] + [None] * 5)) == 0  # nothing to do
    assert lib.bl_report_order(P(d), P(i), -1, 0, 1, P(i), P(i), None) != 0 and "negative" in err()
    assert lib.bl_report_order(None, P(i), 4, 0, 1, P(i), P(i), None) != 0 and "null" in err()
    assert lib.bl_report_order(P(d), P(i), 4, 0, 1, P(i), None, None) != 0 and "null" in err()
    assert lib.bl_report_order(P(d), P(i), 2 ** 20 + 1, 0, 1, P(i), P(i), None) != 0 and "at most" in err()
