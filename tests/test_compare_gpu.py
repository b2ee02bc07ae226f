"""GPU: the paired bootstrap comparison on the MI355X -- the counts of csrc/bl_bootstrap.hip against the NumPy twin
(buglab/models/_compare.py, which tests/test_compare_host.py pins to the written contract and to `ColumnarEvaluationReport`),
run-to-run and however a run is cut into calls, inside guard bands; `compare_models` with the device's counts against the
twin's, on two sequence models (one of which drops samples) and their ensemble; the CLI.

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
            "modelName": "seq-great"}


def _words(n, K, seed, any_scout=False):
    """random packed words: every flag bit of every model in use, the scout ids all of 0 .. K - 1 (`any_scout`: the whole byte,
    ids beyond K included -- they must enter no table)"""
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    if not any_scout:
        w = (w & ~np.uint32(0xFF)) | rng.integers(0, K, size=n).astype(np.uint32)
    return w


def _device(words):
    return torch.from_numpy(words.view(np.int32)).to(DEV)


# n, M, K, R, r0: every value of n {1, 63, 257, 5000}, M {1, 2, 6}, K {1, 3, 64}, R {1, 37, 300}, r0 {0, 1000} with the others
# varied; 257 and 5000 are more than one stride of the workgroup, 63 less than a wave; 70 000 words are 280 KB: more than a CU's LDS
CASES = [(1, 1, 1, 1, 0), (1, 6, 64, 37, 1000), (63, 2, 3, 300, 0), (63, 1, 64, 1, 1000), (257, 6, 1, 37, 0), (257, 2, 64, 300, 1000),
         (5000, 1, 3, 37, 1000), (5000, 6, 64, 300, 0), (5000, 2, 1, 1, 0), (257, 3, 3, 37, 0), (70000, 2, 8, 8, 0), (70000, 5, 64, 8, 1000)]


@pytest.mark.parametrize("n,M,K,R,r0", CASES)
def test_counts_equal_the_twin(n, M, K, R, r0):
    from buglab.models import _compare as C
    from buglab.models import hip_ops

    words = _words(n, K, seed=n + M + K)
    want = C.bootstrap_counts_host(words, M, K, 7, r0, R)
    got = hip_ops.bootstrap_counts(_device(words), M, K, 7, r0, R)
    assert got.dtype == torch.int32 and tuple(got.shape) == (R, K + M * (4 + 2 * K))
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    assert int(want[:, :K].sum()) == R * n  # every draw is in exactly one scout column


def test_scout_ids_beyond_k_enter_no_table():
    from buglab.models import _compare as C
    from buglab.models import hip_ops

    words = _words(1000, 3, seed=1, any_scout=True)
    assert (words & 0xFF).max() > 64
    want = C.bootstrap_counts_host(words, 2, 3, 0, 0, 20)
    assert torch.equal(hip_ops.bootstrap_counts(_device(words), 2, 3, 0, 0, 20).cpu(), torch.from_numpy(want))
    assert int(want[:, :3].sum()) < 20 * 1000


def test_same_bits_every_call_and_however_the_run_is_cut():
    from buglab.models import hip_ops

    words = _device(_words(5000, 8, seed=3))
    whole = hip_ops.bootstrap_counts(words, 2, 8, 5, 0, 300)
    assert torch.equal(whole, hip_ops.bootstrap_counts(words, 2, 8, 5, 0, 300))
    cut = torch.cat([hip_ops.bootstrap_counts(words, 2, 8, 5, 0, 100), hip_ops.bootstrap_counts(words, 2, 8, 5, 100, 200)])
    assert torch.equal(whole, cut)
    assert not torch.equal(whole, hip_ops.bootstrap_counts(words, 2, 8, 6, 0, 300))  # another seed, other draws
    assert tuple(hip_ops.bootstrap_counts(words, 2, 8, 5, 0, 0).shape) == (0, 8 + 2 * 20)
    with pytest.raises(ValueError, match="1 <= M <= 6"):
        hip_ops.bootstrap_counts(words, 7, 8, 5, 0, 10)
    with pytest.raises(ValueError, match="must be"):
        hip_ops.bootstrap_counts(words, 2, 8, 5, 0, 10, out=torch.empty((5, 48), dtype=torch.int32, device=DEV))


def test_nothing_outside_the_operands_is_written():
    from buglab.models import _compare as C
    from buglab.models import hip_ops

    n, M, K, R, spare = 257, 3, 5, 37, 6
    cols = K + M * (4 + 2 * K)
    words = _words(n, K, seed=9)
    g_in = guarded(1, n, ld=n, dtype=torch.int32, device=DEV, any_width=True)
    g_in.fill(_device(words)[None, :])
    g_out = guarded(R + spare, cols, ld=cols, dtype=torch.int32, device=DEV, any_width=True)
    packed, out = g_in.view[0], g_out.view
    assert packed.is_contiguous() and out.is_contiguous()
    got = hip_ops.bootstrap_counts(packed, M, K, 2, 1000, R, out=out)
    assert got.data_ptr() == out.data_ptr()
    g_in.assert_untouched("packed")
    g_out.assert_untouched("out")
    assert torch.equal(g_in.payload()[0].cpu(), torch.from_numpy(words.view(np.int32)))
    assert torch.equal(out[:R].cpu(), torch.from_numpy(C.bootstrap_counts_host(words, M, K, 2, 1000, R)))
    assert bool((g_out.bits.view(torch.int32)[g_out.offset + R * cols:g_out.offset + (R + spare) * cols] == g_out.pattern).all())  # rows beyond R


# ------------------------------------------------------------------------------------------------------------------------------
def _member(folder, data, seed, **extra):
    from buglab.models.modelregistry import load_model

    path = folder / f"seq_great_{seed}.pkl.gz"
    model = load_model(dict(SEQ_SPEC, **extra), path)[0]
    model.compute_metadata(copy.deepcopy(data))
    torch.manual_seed(seed)
    model.save(path, model.build_neural_module())
    return path


def _restore(path):
    from buglab.runtime.neuralmodel import AbstractNeuralModel

    return AbstractNeuralModel.restore_model(Path(path), torch.device(DEV))


def test_compare_models_end_to_end(tmp_path, monkeypatch):
    """Two seq-great models (the second rejects the samples beyond 50 tokens) and their `avg` ensemble, on 40 samples read back
    from a shard as the command reads them."""
    # the msgpack reader in Python, here and in the child process: the sequence models' token projection rejects the synthetic
    # sequence samples as the native reader presents them (tests/test_calibrate_gpu.py does the same)
    monkeypatch.setenv("BUGLAB_NATIVE_READER", "0")
    from buglab.data.synthetic import make_buglab_seq_dataset
    from buglab.models.compare import compare_models
    from buglab.models.evaluate import EvaluationReport, evaluate_predictions
    from buglab.utils.msgpackutils import load_all_msgpack_l_gz, save_msgpack_l_gz

    made = make_buglab_seq_dataset(40, seed=41)
    (tmp_path / "test").mkdir()
    save_msgpack_l_gz(made, tmp_path / "test" / "d.msgpack.l.gz")
    paths = [_member(tmp_path, made, 1), _member(tmp_path, made, 2, max_seq_size=50)]
    ens = tmp_path / "ens.pkl.gz"
    r = subprocess.run([sys.executable, "-m", "buglab.models.ensemble", str(ens), "avg"] + [str(p) for p in paths], cwd=PKG,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    paths.append(ens)
    names = [str(p) for p in paths]
    data = list(load_all_msgpack_l_gz(tmp_path / "test"))
    models = [_restore(p) for p in paths]
    device = torch.device(DEV)
    kw = dict(num_replicates=200, seed=3, parallelize=False, names=names)
    on_device = compare_models(models, data, device, **kw)
    on_host = compare_models(models, data, device, host_bootstrap=True, **kw)
    assert on_device.to_json() == on_host.to_json()

    # what each model kept, by its own predict on the host path
    position_of = {id(d): i for i, d in enumerate(data)}
    predicted = []
    for model, nn_ in models:
        triples = list(model.predict(iter(data), nn_, device, False))
        predicted.append({position_of[id(d)]: (d, loc, rw) for d, loc, rw in triples})
    kept = [len(p) for p in predicted]
    assert kept[0] == 40 and 0 < kept[1] < 40 and kept[2] == 40  # the ensemble answers where any member does
    assert [m["num_dropped"] for m in on_device.models] == [0, 40 - kept[1], 0] and [m["name"] for m in on_device.models] == names
    paired = sorted(set(predicted[0]) & set(predicted[1]) & set(predicted[2]))
    assert on_device.num_paired == len(paired) == kept[1] and on_device.num_replicates == 200
    # the point estimates: summary() of the host path's report over the paired samples
    for m, p in enumerate(predicted):
        summary = EvaluationReport(evaluate_predictions([p[i] for i in paired]).outcomes).summary()
        assert 0 < summary["num_buggy_samples"] < summary["num_samples"] == len(paired)
        for name in ("accuracy", "bug_detection_accuracy", "bug_detection_false_negatives", "bug_detection_false_positives",
                     "localization_accuracy", "repair_accuracy_given_location", "repair_accuracy", "bug_detection_recall", "no_bug_precision"):
            iv = on_device.metrics[name][m]
            assert iv.point == summary[name], (name, m)
            assert iv.low <= iv.high and (iv.se == iv.se or iv.num_undefined == 200)
    assert sorted(on_device.mcnemar) == [1, 2] and sorted(on_device.deltas["accuracy"]) == [1, 2]
    assert "McNemar (exact) on repaired, model 2 vs model 0" in on_device.format()

    # the command, in a child process
    blob = tmp_path / "report.json"
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "buglab.models.compare", str(tmp_path / "test")] + names
                       + ["--num-replicates", "200", "--seed", "3", "--sequential", "--report-json", str(blob)], cwd=PKG,
                       capture_output=True, text=True, timeout=420, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout == on_device.format()
    assert blob.read_text() == on_device.to_json()
    assert json.loads(blob.read_text())["num_paired"] == len(paired)
