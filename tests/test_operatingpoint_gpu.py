"""GPU: warning operating points on the MI355X -- the threshold-curve counts of bl_bootstrap_curve_counts (csrc/bl_bootstrap.hip)
against the NumPy twin (buglab/models/_operatingpoint.py, which tests/test_operatingpoint_host.py pins to the ranking of
`ColumnarEvaluationReport`), paired with bl_bootstrap_counts over the same draws, run-to-run and however a run is cut into
calls, inside guard bands; `fit_operating_point` with the device's counts against the twin's on a sequence model, the CLI, and
the consumers of the checkpoint's operating point (`visualize`, `evaluate`).

No tolerance anywhere: every output of the kernel is an integer count, and the reports are compared as text."""
import copy
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from tests.conftest import PKG
from tests.guard_bands import guarded

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEQ_SPEC = {"hidden_state_size": 64, "num_layers": 2, "num_heads": 4, "intermediate_dimension_size": 96, "dropout_rate": 0.1,
            "modelName": "seq-great"}  # the tiny spec of tests/test_compare_gpu.py


def _words(n, seed):
    """random packed words: every flag bit of every model in use (combinations no model produces included), scout ids 0 .. 3"""
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    return (w & ~np.uint32(0xFF)) | rng.integers(0, 4, size=n).astype(np.uint32)


def _bins(M, n, G, seed):
    return np.random.default_rng(seed).integers(0, G + 1, size=(M, n)).astype(np.int16)  # G: passes no threshold


def _dev(words):
    return torch.from_numpy(words.view(np.int32)).to(DEV)


def _counts(words, bins, M, G, seed, r0, R, **kw):
    from buglab.models import hip_ops

    return hip_ops.bootstrap_curve_counts(_dev(words), torch.from_numpy(bins).to(DEV), M, G, seed, r0, R, **kw)


# n, M, G, R, r0: every value of n {1, 63, 257, 5000}, M {1, 2, 6}, G {1, 2, 64, 1024}, R {1, 37, 300}, r0 {0, 1000} with the
# others varied; 257 and 5000 are more than one stride of the workgroup, 63 less than a wave; G = 1024 gives every thread four
# bins to scan, 64 leaves three waves without a bin, 300 (beyond the listed values) ends inside a thread's pair of bins
CASES = [(1, 1, 1, 1, 0), (1, 6, 1024, 37, 1000), (63, 2, 2, 300, 0), (63, 1, 64, 1, 1000), (257, 6, 1, 37, 0), (257, 2, 1024, 300, 1000),
         (5000, 1, 2, 37, 1000), (5000, 6, 64, 300, 0), (5000, 2, 1, 1, 0), (257, 3, 64, 37, 0), (5000, 2, 1024, 37, 0), (257, 1, 300, 37, 1000)]


@pytest.mark.parametrize("n,M,G,R,r0", CASES)
def test_counts_equal_the_twin(n, M, G, R, r0):
    from buglab.models import _operatingpoint as P

    words, bins = _words(n, seed=n + M + G), _bins(M, n, G, seed=n + G)
    want = P.curve_counts_host(words, bins, M, G, 7, r0, R)
    got = _counts(words, bins, M, G, 7, r0, R)
    assert got.dtype == torch.int32 and tuple(got.shape) == (R, 1 + M * 5 * G)
    assert torch.equal(got.cpu(), torch.from_numpy(want))


def test_extreme_bins():
    from buglab.models import _operatingpoint as P

    n, M, G, R = 5000, 2, 64, 20
    every = np.full(n, 0x77700 | 1, np.uint32)  # has_bug, and warned | loc_ok | rep_ok of models 0 and 1 (and of model 2)
    first = np.zeros((M, n), np.int16)  # all samples in bin 0 with every flag set: every lane adds to the same three words
    got = _counts(every, first, M, G, 1, 0, R).cpu().numpy()
    assert np.array_equal(got, P.curve_counts_host(every, first, M, G, 1, 0, R))
    table = got[:, 1:].reshape(R, M, 5, G)
    assert (got[:, 0] == n).all() and (table[:, :, [0, 2]] == n).all() and (table[:, :, [1, 3, 4]] == 0).all()
    words = _words(n, seed=2)
    nowhere = np.full((M, n), G, np.int16)  # all samples in bin G: only column 0 is non-zero
    got = _counts(words, nowhere, M, G, 1, 0, R).cpu().numpy()
    assert (got[:, 1:] == 0).all() and (got[:, 0] > 0).all()
    assert np.array_equal(got, P.curve_counts_host(words, nowhere, M, G, 1, 0, R))
    rising = np.stack([(np.arange(n) * (G + 1) // n), (np.arange(n) % (G + 1))]).astype(np.int16)  # bins that rise with the position
    assert rising.min() == 0 and rising.max() == G
    assert np.array_equal(_counts(words, rising, M, G, 1, 0, R).cpu().numpy(), P.curve_counts_host(words, rising, M, G, 1, 0, R))
    wild = rising.copy()
    wild[0, ::5], wild[1, ::7] = -1, 30000  # outside [0, G]: no threshold passed, nothing written anywhere
    assert np.array_equal(_counts(words, wild, M, G, 1, 0, R).cpu().numpy(), P.curve_counts_host(words, wild, M, G, 1, 0, R))


def test_paired_with_the_scalar_kernel():
    """The same words, seed and replicates: the two kernels count the same draws."""
    from buglab.models import _compare as C
    from buglab.models import hip_ops

    n, M, G, K, R, r0, seed = 5000, 3, 64, 4, 37, 1000, 9
    words = _words(n, seed=4)
    for m in range(M):  # as every model judges: a warning on correct code is a wrong location (loc_ok there means "NO_BUG predicted")
        false_alarm = ((words & 0xFF) == 0) & ((words >> np.uint32(8 + 4 * m)) & 1 != 0)
        words = np.where(false_alarm, words & ~np.uint32(2 << (8 + 4 * m)), words)
    bins = _bins(M, n, G - 1, seed=5)  # every sample passes the last threshold
    assert bins.max() == G - 1
    curve = _counts(words, bins, M, G, seed, r0, R).cpu().numpy()
    scalar = hip_ops.bootstrap_counts(_dev(words), M, K, seed, r0, R).cpu().numpy()
    assert np.array_equal(curve[:, 0], n - scalar[:, 0])  # num_buggy = n - scout_total[0]
    drawn = words[C.draw_indices(seed, np.arange(r0, r0 + R), n)]
    table = curve[:, 1:].reshape(R, M, 5, G)
    for m in range(M):
        f = drawn >> np.uint32(8 + 4 * m)
        shown = ((f & 1) != 0) | (((drawn & 0xFF) != 0) & ((f & 2) != 0))  # warned | (has_bug & loc_ok)
        assert np.array_equal(table[:, m, 0, G - 1] + table[:, m, 1, G - 1], shown.sum(axis=1))


def test_same_bits_every_call_and_however_the_run_is_cut():
    n, M, G = 5000, 2, 64
    words, bins = _words(n, seed=3), _bins(M, n, G, seed=3)
    whole = _counts(words, bins, M, G, 5, 0, 300)
    assert torch.equal(whole, _counts(words, bins, M, G, 5, 0, 300))
    assert torch.equal(whole, torch.cat([_counts(words, bins, M, G, 5, 0, 100), _counts(words, bins, M, G, 5, 100, 200)]))
    assert not torch.equal(whole, _counts(words, bins, M, G, 6, 0, 300))  # another seed, other draws
    assert tuple(_counts(words, bins, M, G, 5, 0, 0).shape) == (0, 1 + M * 5 * G)
    with pytest.raises(ValueError, match="1 <= M <= 6"):
        _counts(words, np.zeros((7, n), np.int16), 7, G, 5, 0, 10)
    with pytest.raises(ValueError, match="1 <= G <= 1024"):
        _counts(words, bins, M, 1025, 5, 0, 10)
    with pytest.raises(ValueError, match="1 <= G <= 1024"):
        _counts(words, bins, M, 0, 5, 0, 10)
    with pytest.raises(ValueError, match="bins"):
        _counts(words, bins[:1], M, G, 5, 0, 10)
    with pytest.raises(ValueError, match="out .* must be"):
        _counts(words, bins, M, G, 5, 0, 10, out=torch.empty((5, 1 + M * 5 * G), dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="out .* must be"):
        _counts(words, bins, M, G, 5, 0, 10, out=torch.empty((10, M * 5 * G), dtype=torch.int32, device=DEV))


def test_nothing_outside_the_operands_is_written():
    from buglab.models import _operatingpoint as P
    from buglab.models import hip_ops

    n, M, G, R, spare = 257, 3, 70, 37, 6
    cols = 1 + M * 5 * G
    words, bins = _words(n, seed=9), _bins(M, n, G, seed=9)
    g_in = guarded(1, n, ld=n, dtype=torch.int32, device=DEV, any_width=True)
    g_in.fill(_dev(words)[None, :])
    g_bins = guarded(M, n, ld=n, dtype=torch.int16, device=DEV, any_width=True)
    g_bins.fill(torch.from_numpy(bins).to(DEV))
    g_out = guarded(R + spare, cols, ld=cols, dtype=torch.int32, device=DEV, any_width=True)
    packed, d_bins, out = g_in.view[0], g_bins.view, g_out.view
    assert packed.is_contiguous() and d_bins.is_contiguous() and out.is_contiguous()
    got = hip_ops.bootstrap_curve_counts(packed, d_bins, M, G, 2, 1000, R, out=out)
    assert got.data_ptr() == out.data_ptr()
    g_in.assert_untouched("packed"), g_bins.assert_untouched("bins"), g_out.assert_untouched("out")
    assert torch.equal(g_in.payload()[0].cpu(), torch.from_numpy(words.view(np.int32)))
    assert torch.equal(g_bins.payload().cpu(), torch.from_numpy(bins))
    assert torch.equal(out[:R].cpu(), torch.from_numpy(P.curve_counts_host(words, bins, M, G, 2, 1000, R)))
    assert bool((g_out.bits.view(torch.int32)[g_out.offset + R * cols:g_out.offset + (R + spare) * cols] == g_out.pattern).all())  # rows beyond R


# ------------------------------------------------------------------------------------------------------------------------------
def _member(folder, data, seed):
    """An untrained seq-great checkpoint.  Untrained, it predicts NO_BUG on every synthetic sample (no warning, an empty grid);
    it carries a confidence calibration whose NO_BUG bias makes it warn, which `evaluate_on_device` applies, so the operating
    point is fitted on calibrated confidences and says so."""
    from buglab.models._calibrate import ConfidenceCalibration
    from buglab.models.modelregistry import load_model

    path = folder / f"seq_great_{seed}.pkl.gz"
    model = load_model(dict(SEQ_SPEC), path)[0]
    model.compute_metadata(copy.deepcopy(data))
    model.confidence_calibration = ConfidenceCalibration(1.0, -2.0, 1.0)
    torch.manual_seed(seed)
    model.save(path, model.build_neural_module())
    return path


def _restore(path):
    from buglab.runtime.neuralmodel import AbstractNeuralModel

    return AbstractNeuralModel.restore_model(Path(path), torch.device(DEV))


def test_operating_point_end_to_end(tmp_path, monkeypatch, capsys):
    """An untrained seq-great model on 40 synthetic samples read back from a shard as the command reads them: the fit with the
    device's counts against the twin's, the command in a child process, and the consumers of the checkpoint it writes."""
    # the msgpack reader in Python, here and in the child process, as tests/test_compare_gpu.py does for the sequence models
    monkeypatch.setenv("BUGLAB_NATIVE_READER", "0")
    from buglab.data.synthetic import make_buglab_seq_dataset
    from buglab.models import _compare as C
    from buglab.models import _operatingpoint as P
    from buglab.models import evaluate, visualize
    from buglab.models import operatingpoint as O
    from buglab.utils.msgpackutils import load_all_msgpack_l_gz, save_msgpack_l_gz

    made = make_buglab_seq_dataset(40, seed=41)
    (tmp_path / "valid").mkdir()
    save_msgpack_l_gz(made, tmp_path / "valid" / "d.msgpack.l.gz")
    path = _member(tmp_path, made, 2)
    data = list(load_all_msgpack_l_gz(tmp_path / "valid"))
    model, nn_ = _restore(path)
    device = torch.device(DEV)

    # the target: from the point-estimate curve, checked on the host (the twin) before anything is asked of the device
    report = evaluate.evaluate_on_device(model, nn_, data, device, parallelize=False)
    curve, R, seed, max_bins = "detection_precision", 200, 3, 16
    thresholds = P.curve_grid(report.confidence, report.warned, max_bins)
    G = thresholds.shape[0]
    assert report.confidence.shape[0] == 40 and G >= 1  # the model warns somewhere
    packed, bins = C.pack_outcomes([report])[0], P.bin_of(report.confidence, thresholds)[None, :]
    point_counts = P.curve_counts_point(packed, bins, 1, G)
    at_all_warnings = float(np.nan_to_num(P.curves_from_counts(point_counts, 1, G)[curve][0, 0, G - 1]))
    twin_counts = P.curve_counts_host(packed, bins, 1, G, seed, 0, R)
    for target in (0.5 * at_all_warnings, 0.25 * at_all_warnings, 0.0):  # an untrained model: whatever its lower bound reaches
        expected = P.choose_operating_point(point_counts, twin_counts, thresholds, curve=curve, target=target, min_warnings=1,
                                            num_samples=40, seed=seed)
        if expected is not None:
            break
    assert expected is not None

    kw = dict(target_precision=target, curve=curve, num_replicates=R, seed=seed, max_bins=max_bins, min_warnings=1, parallelize=False)
    on_device, on_host = {}, {}
    point = O.fit_operating_point(model, nn_, data, device, details=on_device, **kw)
    assert model.warning_operating_point == point == expected._replace(calibrated=True) and isinstance(point, P.OperatingPoint)
    twin_model, twin_nn = _restore(path)
    assert O.fit_operating_point(twin_model, twin_nn, data, device, host_bootstrap=True, details=on_host, **kw) == point
    assert json.dumps(on_device, sort_keys=True) == json.dumps(on_host, sort_keys=True)
    assert np.array_equal(O.curve_counts_device(packed, bins, 1, G, seed, R, device), twin_counts)

    # the command, in a child process
    out, blob = tmp_path / "with_point.pkl.gz", tmp_path / "report.json"
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    command = [sys.executable, "-m", "buglab.models.operatingpoint", str(path), str(tmp_path / "valid"), str(out), "--target-precision",
               repr(target), "--curve", curve, "--num-replicates", str(R), "--seed", str(seed), "--max-bins", str(max_bins),
               "--min-warnings", "1", "--sequential", "--report-json", str(blob)]
    r = subprocess.run(command, cwd=PKG, capture_output=True, text=True, timeout=420, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout == O.format_details(on_device)
    assert blob.read_text() == json.dumps(on_device, indent=1, sort_keys=True) + "\n"
    with_point, nn_point = _restore(out)
    assert with_point.warning_operating_point == point and _restore(path)[0].warning_operating_point is None
    # a target no threshold reaches: the best lower bound is printed, nothing is written, exit status 2
    nowhere, no_blob = tmp_path / "nowhere.pkl.gz", tmp_path / "nowhere.json"
    unreachable = command[:5] + [str(nowhere), "--target-precision", "1.01"] + command[8:-1] + [str(no_blob)]
    r = subprocess.run(unreachable, cwd=PKG, capture_output=True, text=True, timeout=420, env=env)
    assert r.returncode == 2, r.stderr[-3000:]
    assert "No threshold qualifies" in r.stdout and "best lower bound reached" in r.stdout
    assert not nowhere.exists() and not no_blob.exists()

    # visualize at the operating point: exactly the warnings at or above the threshold, in the unfiltered report's order
    everything = visualize.scan(with_point, nn_point, data, device, order_by_confidence=True)
    shown = visualize.scan(with_point, nn_point, data, device, order_by_confidence=True, at_operating_point=True)
    assert np.array_equal(everything.warned, report.warned) and np.array_equal(everything.confidence, report.confidence)
    keep = everything.warned & (everything.confidence >= point.threshold_logprob)
    assert 0 < keep.sum() == point.num_warnings
    assert shown.selected.tolist() == [i for i in everything.selected.tolist() if keep[i]]
    assert shown.snippets == [s for i, s in zip(everything.selected.tolist(), everything.snippets) if keep[i]]
    with_point.warning_operating_point = point._replace(threshold_logprob=float(thresholds[G // 2]))  # a threshold that cuts
    fewer = visualize.scan(with_point, nn_point, data, device, at_operating_point=True, only_incorrect=True)
    keep_fewer = everything.is_wrong & everything.warned & (report.confidence >= thresholds[G // 2])
    assert fewer.selected.tolist() == np.flatnonzero(keep_fewer).tolist() and 0 < keep_fewer.sum() < 40
    with_point.warning_operating_point = point
    by_probability = visualize.scan(with_point, nn_point, data, device, min_confidence=float(np.exp(point.threshold_logprob)) * (1 + 1e-9))
    assert set(by_probability.selected.tolist()) <= set(np.flatnonzero(keep).tolist())
    with pytest.raises(ValueError, match="no warning operating point"):
        visualize.scan(model.__class__.__new__(model.__class__), nn_point, data, device, at_operating_point=True)

    # evaluate at the operating point: the counts of curve_counts_point at that one threshold
    at = evaluate.at_operating_point(report, point)
    g = int(np.flatnonzero(thresholds == point.threshold_logprob)[0])
    assert [at["num_buggy_samples"]] + [at[c] for c in P.COUNTERS] == [int(point_counts[0, 0])] + point_counts[0, 1:].reshape(5, G)[:, g].tolist()
    assert at["num_warnings"] == point.num_warnings and at["detection_precision"] == point.precision.point
    capsys.readouterr()
    evaluate.run({"MODEL_FILENAME": str(out), "TEST_DATA_PATH": str(tmp_path / "valid"), "--assume-buggy": False, "--eval-only-no-bug": False,
                  "--limit-num-elements": None, "--sequential": True, "--on-device": True, "--report-json": str(blob),
                  "--at-operating-point": True})
    text = capsys.readouterr().out
    head, _, block = text.partition("At the warning operating point")
    printed = json.loads(blob.read_text())["at_operating_point"]
    assert block and head.startswith("=" * 34) and evaluate.format_at_operating_point(printed) in text
    assert printed["threshold_logprob"] == point.threshold_logprob and printed["num_samples"] == 40
    assert printed == json.loads(json.dumps(at))  # the command reads the shard in another order; the verdicts are the samples' own
