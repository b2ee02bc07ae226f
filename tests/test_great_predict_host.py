"""CPU: prediction and evaluation with the GREAT var-misuse model, host side -- the NumPy twin of the prediction head
(buglab/models/_great_predict.py) against a float64 torch restatement of the reference's head (greatreimplementation.py:202-214,
:143-168), `tensorize_for_prediction` and the collate keyword, the report assembly of buglab/models/evaluategreat.py, and the C ABI
of csrc/bl_varmisuse_predict.hip (symbols, argument errors).  Nothing here touches a GPU."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests.conftest import PKG, ROOT
from tests.test_great_varmisuse_gpu import _head_case, ref_head

HEADER = os.path.join(ROOT, "include", "buglab_hip.h")
LIB = os.path.join(PKG, "buglab", "models", "hip_ops", "libbuglab_hip.so")
SMALL = {"num_layers": 2, "num_heads": 4, "intermediate_dimension": 96, "dropout_rate": 0.0}
HEAD_CASES = [  # the four cases of tests/test_great_varmisuse_gpu.py::test_head_matches_float64_restatement
    dict(D=64, B=3, L=23, seed=0, full_lengths=True),
    dict(D=128, B=4, L=37, seed=1, no_bug=True),
    dict(D=512, B=5, L=64, seed=2, ties=True),
    dict(D=512, B=30, L=130, seed=3),
]


@pytest.fixture(scope="module")
def built_lib():
    if not os.path.exists(LIB):
        import __graft_entry__ as g

        g.build()
    return LIB


def restated_records(logits32, B, L, err, tgt):
    """The record of include/buglab_hip.h::bl_varmisuse_predict from torch's own log_softmax / argmax / logsumexp in float64, on
    the masked logits [B * L, 2] (-inf where masked, as `ref_head` returns them)."""
    lg = torch.as_tensor(logits32).double().reshape(B, L, 2)
    loc, ptr = lg[:, :, 0], lg[:, :, 1]
    cand = ptr > -math.inf
    loc_lp = torch.log_softmax(loc, dim=-1)
    ptr_lp = torch.log_softmax(ptr, dim=-1)  # (a row without a candidate is NaN: selected away below)
    pred = loc.argmax(-1)
    out_d = torch.empty(7, B, dtype=torch.float64)
    out_i = torch.empty(4, B, dtype=torch.int32)
    rows = torch.arange(B)
    out_d[0] = torch.logsumexp(loc, dim=-1)
    out_d[1] = torch.logsumexp(ptr, dim=-1)
    out_d[2] = loc_lp[rows, pred]
    out_d[3] = loc_lp[:, 0]
    out_d[4] = loc_lp[rows, err.long()]
    out_i[0] = pred
    out_i[2] = pred == err.long()
    for b in range(B):
        if cand[b].any():
            r = int(ptr[b].argmax())
            out_d[5, b], out_i[1, b], out_i[3, b] = ptr_lp[b, r], r, int(tgt[b, r])
        else:
            out_d[5, b], out_i[1, b], out_i[3, b] = math.nan, -1, 0
        both = cand[b] & tgt[b]
        out_d[6, b] = torch.logsumexp(ptr_lp[b][both], dim=-1) if both.any() else -math.inf  # :161
    return out_d.numpy(), out_i.numpy()


def assert_records_agree(got_d, got_i, want_d, want_i, tol=1e-12):
    assert got_i.dtype == np.int32 and got_d.dtype == np.float64
    assert np.array_equal(got_i, want_i)
    assert np.array_equal(np.isnan(got_d), np.isnan(want_d))
    assert np.array_equal(np.isneginf(got_d), np.isneginf(want_d)) and not np.isposinf(got_d).any()
    fin = np.isfinite(want_d)
    assert np.abs(got_d[fin] - want_d[fin]).max() <= tol


def edge_case(seed=4):
    """B 4, L 19: sample 1 has no candidate at all, the only target of sample 2 is not a candidate."""
    x, ln_g, ln_b, W, bias, lens_att, err, cand, tgt = _head_case(D=32, B=4, L=19, seed=seed)
    cand[1] = False
    tgt[2] = False
    free = [p for p in range(1, int(lens_att[2])) if not cand[2, p]]
    tgt[2, free[0]] = True
    err[2] = int(torch.nonzero(cand[2])[0])
    return x, ln_g, ln_b, W, bias, lens_att, err, cand, tgt


@pytest.mark.parametrize("case", HEAD_CASES + ["edge"], ids=lambda c: c if isinstance(c, str) else f"D{c['D']}B{c['B']}L{c['L']}")
def test_twin_matches_float64_restatement(case):
    from buglab.models._great_predict import judge_great_host

    tensors = edge_case() if case == "edge" else _head_case(**case)
    x, ln_g, ln_b, W, bias, lens_att, err, cand, tgt = tensors
    B = lens_att.shape[0]
    L = x.shape[0] // B
    logits32 = ref_head(x, ln_g, ln_b, W, bias, lens_att, err, cand, tgt, B, L)[0].float().numpy()
    got_d, got_i = judge_great_host(logits32, L, lens_att.numpy(), err.numpy(), tgt.numpy())
    want_d, want_i = restated_records(logits32, B, L, err, tgt)
    assert got_d.shape == (7, B) and got_i.shape == (4, B)
    assert_records_agree(got_d, got_i, want_d, want_i)
    if case == "edge":
        assert got_i[1, 1] == -1 and math.isnan(got_d[5, 1]) and got_d[1, 1] == -math.inf and got_d[6, 1] == -math.inf
        assert got_i[1, 2] >= 0 and got_d[6, 2] == -math.inf and got_i[3, 2] == 0
    elif case.get("ties"):
        assert got_i[0, 0] == 3 and got_i[2, 0] == 0  # two equal largest logits at 3 and 7, the error at 7: the first index wins
    elif case.get("no_bug"):
        assert (got_d[6] == -math.inf).all()
    # exp of the localization log-probabilities sums to 1
    lg = logits32.reshape(B, L, 2).astype(np.float64)
    assert np.abs(np.exp(lg[:, :, 0] - got_d[0][:, None]).sum(1) - 1).max() < 1e-12


def test_twin_first_index_on_a_pointer_tie_and_nan_never_wins():
    from buglab.models._great_predict import judge_great_host

    L = 6
    lg = np.full((L, 2), -np.inf, dtype=np.float32)
    lg[:5, 0] = [0.5, np.nan, 2.0, 2.0, 1.0]
    lg[[1, 2, 4], 1] = [1.5, 1.5, -3.0]
    tgt = np.zeros(L, dtype=np.uint8)
    tgt[2] = 1
    d, i = judge_great_host(lg, L, [5], [3], tgt)
    assert i[:, 0].tolist() == [2, 1, 0, 0]
    assert np.isnan(d[0, 0]) and np.isfinite(d[1, 0])  # a NaN logit poisons its column's sum, not the other column
    assert abs(d[5, 0] - (1.5 - d[1, 0])) == 0 and abs(d[6, 0] - d[5, 0]) < 1e-15


# ---- tensorize_for_prediction and the collate keyword ---------------------------------------------------------------------------
def _rec(tokens, edges=(), err=0, cands=(), targets=()):
    return {"source_tokens": list(tokens), "edges": [list(e) for e in edges], "error_location": err, "repair_candidates": list(cands),
            "repair_targets": list(targets), "has_bug": err > 0, "bug_kind": 1, "bug_kind_name": "VARIABLE_MISUSE", "provenances": []}


def _model(**kw):
    from buglab.models.greatreimplementation import GreatVarMisuse

    return GreatVarMisuse(dict(SMALL), vocab_size=64, embedding_dim=64, **kw)


def test_tensorize_for_prediction_masks_and_string_candidates():
    m = _model(max_length=8)
    m.compute_metadata([_rec(["a"] * 6, edges=[(0, 1, 1, "x")])])
    t = m.tensorize_for_prediction(_rec(["a"] * 5, err=0, cands=["x", 2, "y", 4]), labelled=True)
    assert t.error_location == 0 and t.repair_candidates_mask.tolist() == [False, False, True, False, True]
    assert t.repair_targets_mask.dtype == bool and not t.repair_targets_mask.any()
    assert m.tensorize(_rec(["a"] * 5, err=0, cands=["x", 2])).repair_candidates_mask is None  # `tensorize` stays as it is
    buggy = _rec(["a"] * 5, err=2, cands=[2, 3], targets=[3, 4])
    t = m.tensorize_for_prediction(buggy, labelled=True)
    assert t.error_location == 2 and t.repair_targets_mask.tolist() == [False, False, False, True, True]
    u = m.tensorize_for_prediction(buggy, labelled=False)  # labels are not read
    assert u.error_location == 0 and not u.repair_targets_mask.any() and u.repair_candidates_mask.tolist() == t.repair_candidates_mask.tolist()
    assert m.tensorize_for_prediction(_rec(["a"] * 9), labelled=False) is None


def test_collate_keyword_copies_masks_of_no_bug_samples():
    m = _model()
    recs = [_rec(["x", "y", "z", "x"], edges=[(0, 1, 7, "a")], err=0, cands=[1, "s", 3]),
            _rec(["fooBar", "x", "y", "x", "z"], edges=[(3, 2, 4, "b")], err=3, cands=[1, 3], targets=[1, 4])]
    m.compute_metadata(recs * 5)
    ts = [m.tensorize_for_prediction(r, labelled=True) for r in recs]
    on = m.collate_samples(ts, masks_for_all_samples=True)
    off = m.collate_samples(ts)
    assert on["candidate_mask"][0].tolist() == [0, 1, 0, 1, 0, 0, 0, 0] and not off["candidate_mask"][0].any()
    assert on["candidate_mask"][1].tolist() == off["candidate_mask"][1].tolist() == [0, 1, 0, 1, 0, 0, 0, 0]
    assert on["target_mask"][1].tolist() == [0, 1, 0, 0, 1, 0, 0, 0] and not on["target_mask"][0].any()
    for k in on:
        if k != "candidate_mask":
            assert np.array_equal(on[k], off[k]), k
    # the default collate of `tensorize`'s samples is what it was: None masks are never read
    base = m.collate_samples([m.tensorize(r) for r in recs])
    for k in base:
        assert np.array_equal(base[k], off[k]), k
    assert np.array_equal(m.collate_samples([m.tensorize(r) for r in recs], masks_for_all_samples=True)["candidate_mask"], base["candidate_mask"])


def test_rejection_rule_is_tensorize_s():
    from buglab.data.synthetic_great import make_great_records

    m = _model(max_length=100)  # (some of the synthetic records are longer)
    recs = make_great_records(64, seed=7)
    m.compute_metadata(recs)
    recs = recs + [_rec(["a"] * 101, err=0, cands=[1]), _rec(["a"] * 6, err=2, cands=[2, 3], targets=[4, 5])]
    a =[m.tensorize(r) is None for r in recs]
    b = [m.tensorize_for_prediction(r, labelled=True) is None for r in recs]
    assert a == b and a[-2:] == [True, True] and 0 < sum(a[:-2]) < 64
    c = [m.tensorize_for_prediction(r, labelled=False) is None for r in recs]
    assert c == [len(r["source_tokens"]) > 100 for r in recs] and c[-1] is False


def test_predict_exists_on_a_constructed_model_and_ensembles_refuse_it():
    from buglab.models.ensemble.wrapper import EnsembleWrapper
    from buglab.models.greatreimplementation import GreatVarMisuse, VarMisusePrediction

    m = _model()
    assert callable(m.predict) and m.predict.__func__ is GreatVarMisuse._predict
    assert not hasattr(GreatVarMisuse.__new__(GreatVarMisuse), "predict")  # needs the vocabularies of a constructed model
    assert VarMisusePrediction._fields == ("predicted_location", "location_logprob", "no_bug_logprob", "predicted_repair",
                                           "repair_logprob", "localization_logprobs", "repair_logprobs")
    with pytest.raises(ValueError, match="predict"):
        EnsembleWrapper([m], "avg")


# ---- report assembly --------------------------------------------------------------------------------------------------------------
def _hand_made_evaluation():
    from buglab.models.evaluategreat import GreatEvaluation

    #            pred rep loc_ok rep_ok   err  kind
    table = [(0, 4, 1, 0, 0, "NoBug"),            # correct code, silent
             (5, 2, 0, 1, 0, "NoBug"),            # correct code, false alarm
             (3, 7, 1, 1, 3, "VARIABLE_MISUSE"),  # found and repaired
             (3, 6, 1, 0, 3, "VARIABLE_MISUSE"),  # found, wrong repair
             (0, 2, 0, 1, 9, "VARIABLE_MISUSE"),  # missed (no bug predicted), repair would be right
             (4, -1, 0, 0, 2, "OTHER_KIND"),      # wrong place, no candidate
             (8, 3, 1, 1, 8, "OTHER_KIND")]
    n = len(table)
    out_i = np.array([[t[k] for t in table] for k in range(4)], dtype=np.int32)
    out_d = np.zeros((7, n))
    out_d[2] = np.log([0.9, 0.6, 0.8, 0.7, 0.55, 0.3, 0.95])   # confidence
    out_d[4] = np.log([0.9, 0.2, 0.8, 0.7, 0.25, 0.1, 0.95])   # log-probability of the error location
    out_d[6] = np.log([1.0, 1.0, 0.5, 0.25, 0.6, 1.0, 0.75])
    out_d[6, 5] = -np.inf
    return GreatEvaluation(out_d, out_i, np.array([t[4] for t in table]), [t[5] for t in table], skipped=3), table


def test_report_blocks_match_direct_counts_and_the_outcome_list_report():
    from buglab.models.evaluate import EvaluationReport, SampleOutcome

    ev, table = _hand_made_evaluation()
    outcomes = []
    for k, (pred, rep, loc_ok, rep_ok, err, kind) in enumerate(table):
        buggy = err != 0
        outcomes.append(SampleOutcome(float(ev.out_d[2, k]), buggy, pred != 0, bool(loc_ok), bool(rep_ok) if buggy else None,
                                      bool(loc_ok) and (not buggy or bool(rep_ok)), kind))
    assert ev.report().format() == EvaluationReport(outcomes).format()
    assert ev.report().summary() == EvaluationReport(outcomes).summary()
    counts = ev.counts()
    assert counts["samples"] == 7 and counts["buggy_samples"] == 5
    assert counts["localization_hits"] == 4 and counts["buggy_localization_hits"] == 3
    assert counts["repair_hits"] == 3  # buggy samples whose predicted repair is a target
    assert abs(counts["localization_loss_sum"] + np.log([0.9, 0.2, 0.8, 0.7, 0.25, 0.1, 0.95]).sum()) < 1e-12
    assert counts["repair_loss_sum"] == math.inf  # sample 5 has no candidate that is a target (an evaluation rejects such a record)
    mt = ev.metrics()
    assert list(mt)[:7] == ["Localization Accuracy", "Localization Accuracy (Buggy)", "Localization Accuracy (NoBug)", "Repair Accuracy",
                            "Localization Loss", "Repair Loss", "Num samples"]
    assert mt["Num samples"] == 7 and mt["Localization Accuracy"] == 4 / 7 and mt["Repair Accuracy"] == 3 / 5
    assert mt["Classification Accuracy"] == 5 / 7           # warned == buggy for samples 0, 2, 3, 5, 6
    assert mt["Localization+Repair Accuracy (Buggy)"] == 2 / 5
    assert mt["False Alarm Rate"] == 1 / 2
    text = ev.format()
    assert "Skipped records: 3" in text and "Classification Accuracy: 0.7143" in text and "OTHER_KIND: 50.0%  (1/2)" in text
    import json

    assert ev.unreachable_error_locations() == 0 and "outside the unmasked" not in text
    lost = ev._replace(out_d=np.where(np.arange(7)[:, None] == 4, -np.inf, ev.out_d))  # every error location masked away
    assert lost.unreachable_error_locations() == 7 and lost.counts()["localization_loss_sum"] == math.inf
    assert "(their localization loss is inf): 7" in lost.format()
    data = json.loads(ev.to_json())
    assert data["skipped"] == 3 and data["summary"]["num_samples"] == 7 and data["metrics"]["Num samples"] == 7
    lines = [json.loads(line) for line in ev.prediction_lines()]
    assert len(lines) == 7 and lines[5]["predicted_repair"] is None and lines[2]["predicted_location"] == 3


def test_module_metrics_keep_their_names():
    from buglab.models.greatreimplementation import metrics_from_stats

    m = _model()
    m.compute_metadata([_rec(["a"], edges=[(0, 0, 1, "x")])])
    nn = m.build_neural_module()
    nn.metric_stats.copy_(torch.tensor([10, 6, 2, 4, 1, 5.0, 2.0, 3]))
    got = nn._module_metrics()
    assert got == metrics_from_stats(10, 6, 2, 4, 1, 5.0, 2.0)
    assert got["Localization Accuracy"] == 0.6 and got["Repair Accuracy"] == 0.25 and got["Localization Loss"] == 0.5 and got["Num samples"] == 10


# ---- C ABI --------------------------------------------------------------------------------------------------------------------------
def test_symbol_in_header_exports_and_ctypes_table(built_lib):
    from buglab.models import hip_ops

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", built_lib], capture_output=True, text=True, check=True).stdout
    assert "bl_varmisuse_predict" in set(re.findall(r"\b(bl_[a-z0-9_]+)\s*\(", src))
    assert "bl_varmisuse_predict" in set(re.findall(r" T (bl_[a-z0-9_]+)", nm))
    assert "bl_varmisuse_predict" in hip_ops.EXPORTED_SYMBOLS
    assert "greatreimplementation.py:176-214" in open(HEADER).read()
    assert callable(hip_ops.varmisuse_predict) and (hip_ops.VARMISUSE_RECORD_D, hip_ops.VARMISUSE_RECORD_I) == (7, 4)


def test_argument_errors_without_gpu(built_lib):
    from buglab.models import hip_ops

    lib = hip_ops.load_library()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    d = hip_ops.bl_varmisuse_head_t()
    d.B, d.L, d.D, d.ln_eps = 2, 5, 64, 1e-5
    d.x = d.ln_g = d.ln_b = d.W = d.bias = d.lens_att = d.error_location = d.candidate_mask = d.target_mask = p
    ok = lambda rc, text: rc != 0 and text in lib.bl_last_error()
    assert ok(lib.bl_varmisuse_predict(None, p, p, p, 0, 8, None), b"null descriptor")
    assert ok(lib.bl_varmisuse_predict(ctypes.byref(d), None, p, p, 0, 8, None), b"null output")
    assert ok(lib.bl_varmisuse_predict(ctypes.byref(d), p, None, p, 0, 8, None), b"null output")
    assert ok(lib.bl_varmisuse_predict(ctypes.byref(d), p, p, None, 0, 8, None), b"null output")
    assert ok(lib.bl_varmisuse_predict(ctypes.byref(d), p, p, p, 7, 8, None), b"do not fit")   # offset + B > capacity
    assert ok(lib.bl_varmisuse_predict(ctypes.byref(d), p, p, p, -1, 8, None), b"do not fit")
    assert ok(lib.bl_varmisuse_predict(ctypes.byref(d), p, p, p, 0, -1, None), b"do not fit")
    d.target_mask = None
    assert ok(lib.bl_varmisuse_predict(ctypes.byref(d), p, p, p, 0, 8, None), b"null input")
    d.target_mask, d.D = p, 66
    assert ok(lib.bl_varmisuse_predict(ctypes.byref(d), p, p, p, 0, 8, None), b"multiple of 4")
    d.D = 2048
    assert ok(lib.bl_varmisuse_predict(ctypes.byref(d), p, p, p, 0, 8, None), b"multiple of 4")
    d.D, d.B = 64, -3
    assert ok(lib.bl_varmisuse_predict(ctypes.byref(d), p, p, p, 0, 8, None), b"B (-3)")
