"""CPU: warning operating points' host side (buglab/models/_operatingpoint.py, operatingpoint.py and the flags of visualize,
evaluate, compare and calibrate) -- the NumPy twin of bl_bootstrap_curve_counts against the ranking `ColumnarEvaluationReport`
does, the threshold grid, the choice of the point on constructed counts, the checkpoint field, the unchanged default outputs and
the C entry point's argument checks.

No tolerance anywhere: the counts are integers, and the six ratios are compared with the running ratios of the ranking as
float64 values (NaN where both are undefined)."""
import copy
import ctypes
import json
import logging
import os
import pickle
import re
import subprocess

import numpy as np
import pytest

from buglab.models import _compare as C
from buglab.models import _operatingpoint as P
from tests.conftest import PKG, ROOT

HEADER = os.path.join(ROOT, "include", "buglab_hip.h")
LIB = os.path.join(PKG, "buglab", "models", "hip_ops", "libbuglab_hip.so")


def _columns(n, seed, levels=40):
    """random outcome columns: confidences from `levels` values (ties), unwarned samples, warned NO_BUG samples, and flag
    combinations no model produces (an unwarned sample whose location is right)"""
    from buglab.models.evaluate import ColumnarEvaluationReport

    rng = np.random.default_rng(seed)
    grid = -np.sort(rng.exponential(1.0, size=levels))
    has_bug = rng.uniform(size=n) < 0.6
    scout = np.where(has_bug, rng.integers(1, 4, size=n), 0)
    confidence = grid[rng.integers(0, levels, size=n)]
    warned = (rng.uniform(size=n) < 0.7) & (confidence > confidence.min())  # the least confident samples pass no threshold
    return ColumnarEvaluationReport(confidence, has_bug, warned, rng.uniform(size=n) < 0.5,
                                    rng.integers(-1, 2, size=n), rng.uniform(size=n) < 0.3, scout, ["NoBug", "a", "b", "c"])


def _rows(report, rows):
    from buglab.models.compare import _rows_of

    return _rows_of(report, rows)


def _ranked_reference(report, thresholds):
    """-> (num_buggy, counts int64 [5, G], ratios {curve: float64 [G]}) from the ranking of `ColumnarEvaluationReport.curves()`
    and the cumulative sums and running ratios of `_curves_of_ranked`, read at the last ranked position whose confidence is at
    least the threshold (before the first position: nothing is counted)."""
    neg = lambda c: -c.astype(np.int8)
    order = np.lexsort((neg(report.repair_given_location), neg(report.location_correct), neg(report.warned), neg(report.has_bug),
                        -report.confidence))
    has_bug, warned, loc_ok = report.has_bug[order], report.warned[order], report.location_correct[order]
    repair_ok, confidence = report.repair_given_location[order] == 1, report.confidence[order]
    assert (np.diff(confidence) <= 0).all()
    num_buggy = int(has_bug.sum())
    lead = lambda mask: np.concatenate([[0], np.cumsum(mask)])
    det_true, det_false = lead(has_bug & loc_ok), lead(warned & ~loc_ok)
    full_true, full_false = lead(has_bug & loc_ok & repair_ok), lead(warned & (~loc_ok | ~repair_ok))
    false_alarms = lead(warned & ~has_bug)
    with np.errstate(divide="ignore", invalid="ignore"):
        running = {
            "fdr": det_false / (det_true + det_false),
            "detection_precision": det_true / (det_true + det_false),
            "detection_recall": det_true / num_buggy,
            "no_bug_precision": 1 - false_alarms / (num_buggy + 1e-10),
            "precision": full_true / (full_true + full_false),
            "recall": full_true / num_buggy,
        }
    at = np.array([int((confidence >= t).sum()) for t in thresholds], dtype=np.int64)  # 1 + the last position, 0 for none
    counts = np.stack([c[at] for c in (det_true, det_false, full_true, full_false, false_alarms)])
    return num_buggy, counts, {k: v[at] for k, v in running.items()}


def _check_row(row, report, thresholds):
    G = len(thresholds)
    num_buggy, counts, ratios = _ranked_reference(report, thresholds)
    assert row[0] == num_buggy
    assert np.array_equal(row[1:].reshape(5, G), counts)
    got = P.curves_from_counts(row[None, :], 1, G)
    assert list(got) == list(P.CURVES) == list(ratios)
    for name in P.CURVES:
        assert got[name].shape == (1, 1, G) and got[name].dtype == np.float64
        np.testing.assert_array_equal(got[name][0, 0], ratios[name], err_msg=name)  # exact; NaN where both are undefined


@pytest.mark.parametrize("max_bins", [1024, 7])
def test_twin_counts_are_the_cumulative_sums_of_the_ranking(max_bins):
    report = _columns(300, seed=1)
    thresholds = P.curve_grid(report.confidence, report.warned, max_bins)
    G = thresholds.shape[0]
    assert G == (7 if max_bins == 7 else np.unique(report.confidence[report.warned]).shape[0]) and G > 1
    assert (~report.warned & report.has_bug & report.location_correct).any() and (report.warned & ~report.has_bug).any()
    packed, _, _ = C.pack_outcomes([report])
    bins = P.bin_of(report.confidence, thresholds)[None, :]
    assert bins.dtype == np.int16 and bins.min() == 0 and bins.max() == G
    point = P.curve_counts_point(packed, bins, 1, G)
    assert point.shape == (1, P.num_columns(1, G)) == (1, 1 + 5 * G) and point.dtype == np.int32
    _check_row(point[0], report, thresholds)
    R, seed = 20, 11
    counts = P.curve_counts_host(packed, bins, 1, G, seed, 0, R)
    assert counts.shape == (R, 1 + 5 * G) and counts.dtype == np.int32
    draws = C.draw_indices(seed, R, 300)
    for r in range(R):
        _check_row(counts[r], _rows(report, draws[r]), thresholds)
    assert np.array_equal(counts, np.concatenate([P.curve_counts_host(packed, bins, 1, G, seed, 0, 8),
                                                  P.curve_counts_host(packed, bins, 1, G, seed, 8, 12)]))
    assert (np.diff(counts[:, 1:].reshape(R, 5, G), axis=2) >= 0).all()  # cumulative over the bins


def test_twin_counts_every_model_over_the_same_draws():
    a, b = _columns(257, seed=2), _columns(257, seed=3)
    b = type(a)(b.confidence, a.has_bug, b.warned, b.location_correct, b.repair_given_location, b.repaired, a.scout, a.scout_names)
    packed, _, _ = C.pack_outcomes([a, b])
    grids = [P.curve_grid(r.confidence, r.warned, 16) for r in (a, b)]
    bins = np.stack([P.bin_of(r.confidence, g) for r, g in zip((a, b), grids)])
    both = P.curve_counts_host(packed, bins, 2, 16, 5, 3, 6)
    for m, r in enumerate((a, b)):
        alone = P.curve_counts_host(C.pack_outcomes([r])[0], bins[m:m + 1], 1, 16, 5, 3, 6)
        assert np.array_equal(both[:, 0], alone[:, 0])
        assert np.array_equal(both[:, 1 + 80 * m:1 + 80 * (m + 1)], alone[:, 1:])
    # a bin outside [0, G) passes no threshold
    wild = bins.copy()
    wild[0, ::2] = 16
    wild[1, ::3] = -1
    bad = wild.copy()
    bad[0, ::2] = 999
    assert np.array_equal(P.curve_counts_host(packed, wild, 2, 16, 5, 0, 3), P.curve_counts_host(packed, bad, 2, 16, 5, 0, 3))
    for kw in ({"M": 0}, {"M": 7}, {"G": 0}, {"G": 1025}):
        with pytest.raises(ValueError, match="must be in"):
            P.curve_counts_host(packed, bins, **{"M": 2, "G": 16, **kw}, seed=0, r0=0, R=1)
    with pytest.raises(ValueError, match="bins"):
        P.curve_counts_host(packed, bins[:1], 2, 16, 0, 0, 1)


def test_curve_grid_and_bin_of():
    conf = np.log(np.array([0.9, 0.5, 0.5, 0.7, 0.2, 0.95, 0.1, np.nan]))
    warned = np.array([1, 1, 1, 1, 0, 0, 1, 1], dtype=bool)
    few = P.curve_grid(conf, warned, 16)  # fewer distinct confidences than max_bins: all of them, descending
    assert few.tolist() == np.log([0.9, 0.7, 0.5, 0.1]).tolist() and few.dtype == np.float64
    bins = P.bin_of(conf, few)
    assert bins.dtype == np.int16 and bins.tolist() == [0, 2, 2, 1, 3, 0, 3, 4]  # equal to a threshold: passes it; NaN: none
    assert P.bin_of(np.log([0.05]), few).tolist() == [4]  # below every threshold: G
    many = np.log(np.linspace(0.01, 0.99, 99))
    cut = P.curve_grid(many, np.ones(99, bool), 10)  # more than max_bins: evenly spaced by rank, both ends included
    distinct = np.unique(many)[::-1]
    assert cut.shape == (10,) and cut[0] == distinct[0] and cut[-1] == distinct[-1] and (np.diff(cut) < 0).all()
    assert cut.tolist() == distinct[[0, 10, 21, 32, 43, 54, 65, 76, 87, 98]].tolist()
    assert P.curve_grid(many, np.ones(99, bool), 1).tolist() == [distinct[-1]]
    assert P.curve_grid(many, np.ones(99, bool), 99).tolist() == distinct.tolist()
    none = P.curve_grid(conf, np.zeros(8, bool), 16)  # no warned sample
    assert none.shape == (0,) and P.bin_of(conf, none).tolist() == [0] * 8  # G = 0: every sample is in bin G
    with pytest.raises(ValueError, match="max_bins"):
        P.curve_grid(conf, warned, 1025)
    with pytest.raises(ValueError, match="descending"):
        P.bin_of(conf, few[::-1])


def _constructed(full_true, full_false, R, num_buggy=100, empty_first=0):
    """point counts [1, C] and R replicates equal to them; the first `empty_first` replicates raise no warning at threshold 0"""
    G = len(full_true)
    point = np.zeros((1, P.num_columns(1, G)), np.int32)
    point[0, 0] = num_buggy
    table = point[0, 1:].reshape(5, G)
    table[0], table[2], table[3] = full_true, full_true, full_false
    table[1] = full_false
    reps = np.repeat(point, R, axis=0)
    view = reps[:, 1:].reshape(R, 5, G)
    view[:empty_first, :, 0] = 0
    return point, reps


def test_choose_operating_point_on_constructed_counts():
    thresholds = np.log([0.9, 0.8, 0.6, 0.3])
    point, reps = _constructed([5, 30, 60, 70], [0, 2, 10, 40], R=100)  # precision 1, 0.9375, 0.857, 0.636; warnings 5, 32, 70, 110
    choose = lambda **kw: P.choose_operating_point(point, reps, thresholds, **{"target": 0.85, "num_samples": 400, "seed": 3, **kw})
    op = choose()
    assert op.threshold_logprob == thresholds[2] and op.num_warnings == 70  # the largest qualifying g, not the most precise
    assert (op.curve, op.target, op.confidence, op.num_samples, op.num_replicates, op.seed, op.grid_size, op.calibrated) == \
        ("precision", 0.85, 0.95, 400, 100, 3, 4, False)
    assert op.precision._replace(se=0.0) == C.Interval(60 / 70, 0.0, 60 / 70, 60 / 70, 0) and op.precision.se < 1e-15  # std of equal values
    assert op.recall.point == 0.6
    assert choose(target=0.9).threshold_logprob == thresholds[1]
    assert choose(target=0.99) is None  # threshold 0 reaches it with 5 warnings: too few
    assert choose(target=0.99, min_warnings=5).threshold_logprob == thresholds[0]
    assert choose(target=0.2, min_warnings=111) is None
    assert choose(target=1.01, min_warnings=0) is None  # unreachable
    assert choose(curve="detection_precision", calibrated=True)._replace(curve="precision", calibrated=False, recall=op.recall) == op
    # an undefined replicate counts as precision 0: with 10 of 100 the 5 % quantile at threshold 0 is 0, with 2 of 100 it is 1
    _, some = _constructed([5, 30, 60, 70], [0, 2, 10, 40], R=100, empty_first=10)
    assert P.lower_bounds(some, 4, "precision", 0.95)[0] == 0.0
    assert P.choose_operating_point(point, some, thresholds, target=0.99, min_warnings=5) is None
    _, few = _constructed([5, 30, 60, 70], [0, 2, 10, 40], R=100, empty_first=2)
    op = P.choose_operating_point(point, few, thresholds, target=0.99, min_warnings=5)
    assert op.threshold_logprob == thresholds[0] and op.precision.num_undefined == 2 and op.precision.low == 1.0
    assert P.choose_operating_point(point[:, :1], reps[:, :1], [], target=0.1) is None  # an empty grid
    with pytest.raises(ValueError, match="curve"):
        choose(curve="recall")
    bands = P.curve_bands(point, some, 1, 4, 0.9)
    assert len(bands) == 1 and list(bands[0]) == list(P.CURVES) and len(bands[0]["precision"]) == 4
    assert bands[0]["precision"][0] == C.Interval(1.0, 0.0, 1.0, 1.0, 10) and bands[0]["no_bug_precision"][3].num_undefined == 0
    blob = P.bands_to_dict(bands[0], thresholds)
    assert blob["thresholds_logprob"] == thresholds.tolist() and blob["curves"]["precision"]["num_undefined"] == [10, 0, 0, 0]


def test_fit_from_report_with_the_twin():
    from buglab.models import operatingpoint as O

    report = _columns(400, seed=7)
    details = {}
    point = O.fit_from_report(report, target_precision=0.05, num_replicates=50, seed=2, max_bins=16, min_warnings=1, host_bootstrap=True,
                              details=details)
    assert isinstance(point, P.OperatingPoint) and point.grid_size == 16 and point.num_samples == 400 and point.num_replicates == 50
    thresholds = P.curve_grid(report.confidence, report.warned, 16)
    packed = C.pack_outcomes([report])[0]
    bins = P.bin_of(report.confidence, thresholds)[None, :]
    want = P.choose_operating_point(P.curve_counts_point(packed, bins, 1, 16), P.curve_counts_host(packed, bins, 1, 16, 2, 0, 50), thresholds,
                                    target=0.05, min_warnings=1, num_samples=400, seed=2)
    assert point == want and details["operating_point"] == point.to_dict()
    assert json.loads(json.dumps(details))["curve_bands"]["thresholds_logprob"] == thresholds.tolist()
    text = O.format_details(details)
    assert f"warn at probability >= {np.exp(point.threshold_logprob):.6f}" in text and text.count("\n") <= 5 + O.TABLE_ROWS
    # an unreachable target: the best lower bound and where it was reached
    details = {}
    assert O.fit_from_report(report, target_precision=1.0, num_replicates=50, max_bins=16, host_bootstrap=True, details=details) is None
    best = details["best_lower_bound"]
    bound = P.lower_bounds(P.curve_counts_host(packed, bins, 1, 16, 0, 0, 50), 16, "precision", 0.95)
    assert best == {"lower_bound": float(bound.max()), "threshold_logprob": float(thresholds[int(np.argmax(bound))])}
    assert "No threshold qualifies" in O.format_details(details) and f"{100 * best['lower_bound']:.2f}%" in O.format_details(details)
    # no warned sample: G = 0, nothing qualifies
    silent = type(report)(report.confidence, report.has_bug, np.zeros(400, bool), report.location_correct, report.repair_given_location,
                          report.repaired, report.scout, report.scout_names)
    details = {}
    assert O.fit_from_report(silent, target_precision=0.01, num_replicates=5, host_bootstrap=True, details=details) is None
    assert details["grid_size"] == 0 and details["best_lower_bound"] is None and "warned on no sample" in O.format_details(details)
    a = O.parse_args(["m", "valid", "out", "--target-precision", "0.9"])
    assert (a.MODEL, a.VALID_DATA, a.OUT_MODEL, a.target_precision, a.curve, a.confidence, a.num_replicates, a.seed, a.max_bins,
            a.min_warnings, a.limit_num_elements, a.sequential, a.host_bootstrap, a.report_json) == \
        ("m", "valid", "out", 0.9, "precision", 0.95, 2000, 0, 256, 20, None, False, False, None)
    assert O.replicates_per_call(1, 256) == 4096 and O.replicates_per_call(6, 1024) == (1 << 24) // 30721 and O.EXIT_NOTHING_QUALIFIES == 2


def test_compare_curves_are_additive():
    from buglab.models.compare import compare_reports, parse_args

    a, b = _columns(200, seed=4), _columns(200, seed=5)
    b = type(a)(b.confidence, a.has_bug, b.warned, b.location_correct, b.repair_given_location, b.repaired, a.scout, a.scout_names)
    kw = dict(num_replicates=30, seed=6, host_bootstrap=True)
    plain, curved = compare_reports([a, b], **kw), compare_reports([a, b], curves=True, max_bins=8, **kw)
    assert plain.format() == curved.format() and "curve_bands" not in plain.to_dict()
    blob = curved.to_dict()
    assert json.dumps({k: v for k, v in blob.items() if k != "curve_bands"}, sort_keys=True) == json.dumps(plain.to_dict(), sort_keys=True)
    assert len(blob["curve_bands"]) == 2
    for m, r in enumerate((a, b)):  # each model on its own grid, over the scalar metrics' draws
        thresholds = P.curve_grid(r.confidence, r.warned, 8)
        packed, bins = C.pack_outcomes([r])[0], P.bin_of(r.confidence, thresholds)[None, :]
        bands = P.curve_bands(P.curve_counts_point(packed, bins, 1, 8), P.curve_counts_host(packed, bins, 1, 8, 6, 0, 30), 1, 8, 0.95)
        assert json.dumps(blob["curve_bands"][m]) == json.dumps(P.bands_to_dict(bands[0], thresholds))
    ns = parse_args(["data", "m", "--curves", "--max-bins", "64"])
    assert ns.curves and ns.max_bins == 64 and not parse_args(["data", "m"]).curves


# ------------------------------------------------------------------------------------------------------------------------------
def _operating_point(threshold=-0.25):
    iv = C.Interval(0.9, 0.01, 0.88, 0.92, 0)
    return P.OperatingPoint(threshold, "precision", 0.85, 0.95, iv, iv._replace(point=0.4), 70, 400, 2000, 0, 256, False)


def test_checkpoint_field_and_calibrate_drops_it(tmp_path, caplog):
    import torch

    from buglab.data.synthetic import make_buglab_dataset
    from buglab.models import calibrate
    from buglab.models.modelregistry import load_model
    from buglab.runtime.neuralmodel import AbstractNeuralModel

    graphs = make_buglab_dataset(6, seed=3)
    model = load_model({"modelName": "gnn-mlp", "hidden_state_size": 32, "dropout_rate": 0.1}, tmp_path / "m.pkl.gz")[0]
    model.compute_metadata(copy.deepcopy(graphs))
    nn_ = torch.nn.Linear(2, 2)  # the checkpoint format is (model, module); the module is not what this is about
    assert "_warning_operating_point" not in vars(model) and model.warning_operating_point is None
    model.save(tmp_path / "plain.pkl.gz", nn_)
    plain, _ = AbstractNeuralModel.restore_model(tmp_path / "plain.pkl.gz", "cpu")
    assert "_warning_operating_point" not in vars(plain) and plain.warning_operating_point is None  # as a checkpoint from before
    with caplog.at_level(logging.WARNING):
        assert calibrate.drop_operating_point(plain) is False and not caplog.records
    point = _operating_point()
    model.warning_operating_point = point
    model.save(tmp_path / "point.pkl.gz", nn_)
    restored, _ = AbstractNeuralModel.restore_model(tmp_path / "point.pkl.gz", "cpu")
    assert restored.warning_operating_point == point and isinstance(restored.warning_operating_point, P.OperatingPoint)
    assert restored.confidence_calibration is None
    again = pickle.loads(pickle.dumps(point))
    assert again == point and all(type(v) in (float, str, int, bool, C.Interval) for v in again)
    assert json.loads(json.dumps(point.to_dict()))["precision"]["low"] == 0.88
    with caplog.at_level(logging.WARNING):
        assert calibrate.drop_operating_point(restored) is True
    assert restored.warning_operating_point is None
    assert len(caplog.records) == 1 and "fitted on other confidences" in caplog.records[0].getMessage()


def test_default_outputs_are_unchanged():
    """Without the new flags `evaluate`'s text and data and `visualize`'s selection are those of the same call before; with
    them, the selection is the host's filter of the unfiltered report and the block's counts are `curve_counts_point`'s."""
    from buglab.models import evaluate, visualize
    from buglab.models.visualize import predictions_to_report
    from tests.test_evaluate_golden import FIXTURE, _predictions
    from tests.test_visualize_host import FLAGS, fixture_predictions

    case = next(c for c in FIXTURE["cases"] if not any(c["flags"].values()))
    report = evaluate.evaluate_predictions(_predictions(case))
    text, blob = report.format(), evaluate.report_to_json(report)
    columns = evaluate.ColumnarEvaluationReport.from_outcomes(report.outcomes)
    warned_conf = np.sort(columns.confidence[columns.warned])
    assert warned_conf.shape[0] >= 2
    point = _operating_point(float(warned_conf[warned_conf.shape[0] // 2]))
    at = evaluate.at_operating_point(report, point)
    assert report.format() == text and evaluate.report_to_json(report) == blob == evaluate.report_to_json(report, None)
    assert "at_operating_point" not in json.loads(blob)
    with_at = json.loads(evaluate.report_to_json(report, at))
    assert with_at.pop("at_operating_point") == json.loads(json.dumps(at)) and json.dumps(with_at) == json.dumps(json.loads(blob))
    shown = columns.warned & (columns.confidence >= point.threshold_logprob)
    assert 0 < shown.sum() < columns.warned.sum()
    packed = C.pack_outcomes([columns])[0]
    counts = P.curve_counts_point(packed, P.bin_of(columns.confidence, [point.threshold_logprob])[None, :], 1, 1)[0]
    assert [at["num_buggy_samples"]] + [at[c] for c in P.COUNTERS] == counts.tolist()
    assert at["num_warnings"] == int(shown.sum()) == at["det_true"] + at["det_false"] == at["full_true"] + at["full_false"]
    block = evaluate.format_at_operating_point(at)
    assert f"{at['num_warnings']} warnings on {len(report.outcomes)} samples" in block and "Precision (Detect and Repair)" in block

    shown_conf = sorted(max(loc.values()) for _, loc, _ in fixture_predictions() if max(loc, key=loc.get) != -1)
    cut_at = shown_conf[len(shown_conf) // 2]  # the median warning's confidence: equal to a sample's, which passes
    for only_incorrect, by_confidence in FLAGS:
        before = predictions_to_report(fixture_predictions(), only_incorrect, by_confidence)
        same = predictions_to_report(fixture_predictions(), only_incorrect, by_confidence, min_logprob=None)
        assert before.selected.tolist() == same.selected.tolist() and before.snippets == same.snippets
        assert before.warned.tolist() == [max(loc, key=loc.get) != -1 for _, loc, _ in fixture_predictions()]
        cut = predictions_to_report(fixture_predictions(), only_incorrect, by_confidence, min_logprob=cut_at)
        assert before.confidence.tolist() == [max(loc.values()) for _, loc, _ in fixture_predictions()]  # what `evaluate` thresholds
        keep = before.warned & (before.confidence >= cut_at)
        assert cut.selected.tolist() == [i for i in before.selected.tolist() if keep[i]] and len(cut.snippets) == len(cut.selected)
    assert 0 < len(predictions_to_report(fixture_predictions(), min_logprob=cut_at).selected) < len(shown_conf)

    class Carrier:
        warning_operating_point = None

    assert visualize.warning_threshold(Carrier()) is None
    assert visualize.warning_threshold(Carrier(), min_confidence=0.5) == float(np.log(0.5))
    with pytest.raises(ValueError, match="no warning operating point"):
        visualize.warning_threshold(Carrier(), at_operating_point=True)
    Carrier.warning_operating_point = point
    assert visualize.warning_threshold(Carrier(), at_operating_point=True) == point.threshold_logprob
    assert visualize.warning_threshold(Carrier(), 1.0, True) == 0.0 and visualize.warning_threshold(Carrier(), 0.0) == -np.inf
    ns = visualize.parse_args(["m", "data", "out.html"])
    assert ns.min_confidence is None and ns.at_operating_point is False
    ns = visualize.parse_args(["m", "data", "out.html", "--min-confidence", "0.8", "--at-operating-point"])
    assert ns.min_confidence == 0.8 and ns.at_operating_point is True


# ------------------------------------------------------------------------------------------------------------------------------
def test_entry_point_is_exported_and_reports_argument_errors_without_a_gpu():
    from buglab.models import hip_ops

    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint bl_bootstrap_curve_counts\s*\(", header) and "#define BL_CURVE_MAX_BINS 1024" in header
    lib = hip_ops.load_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    assert " T bl_bootstrap_curve_counts" in nm and "bl_bootstrap_curve_counts" in hip_ops.EXPORTED_SYMBOLS
    words, bins, out = (ctypes.c_uint32 * 16)(), (ctypes.c_int16 * 32)(), (ctypes.c_int32 * 256)()
    p, b, o = (ctypes.cast(x, ctypes.c_void_p) for x in (words, bins, out))
    call = lambda packed=p, bins=b, n=16, M=2, G=3, seed=0, r0=0, R=4, out=o: lib.bl_bootstrap_curve_counts(packed, bins, n, M, G, seed, r0, R,
                                                                                                         out, None)
    BL_EINVAL, BL_ERANGE = -1, -2
    for kw, word in (({"packed": None}, b"null"), ({"bins": None}, b"null"), ({"out": None}, b"null"), ({"n": 0}, b"n must be"),
                     ({"R": -1}, b"negative"), ({"r0": -1}, b"negative"), ({"M": 0}, b"models"), ({"M": 7}, b"models"), ({"G": 0}, b"bins"),
                     ({"G": 1025}, b"bins")):
        assert call(**kw) == BL_EINVAL and word in lib.bl_last_error(), kw
    assert call(n=2 ** 31) == BL_ERANGE and b"int32" in lib.bl_last_error()
    assert call(R=0) == 0  # a no-op: nothing is launched
    assert hip_ops.CURVE_MAX_BINS == P.MAX_BINS == 1024 and hip_ops.CURVE_COUNTERS == len(P.COUNTERS) == 5
