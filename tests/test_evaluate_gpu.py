"""GPU: evaluation on the MI355X -- the judge kernel of csrc/bl_evaluate.hip against its NumPy twin (buglab/models/_evaluate.py,
which tests/test_evaluate_columns_host.py pins to `judge_sample`) bit for bit on handcrafted and drawn minibatches, its offset
writes into run-long buffers, `assume_buggy`; `evaluate_on_device` against `model.predict` + `evaluate_predictions` text for
text; the CLI.

Tolerances.  Without assume_buggy there is none: every output is a selected fp32 value or an integer.  With it the confidence
is an fp64 log-sum-exp on both sides: max / exp / sum / log over n <= 64 terms err by about (n + 4) * 2^-53 ~ 8e-15, and 1e-12
leaves that a 100x margin."""
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

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEQ_SPEC = '{"hidden_state_size": 64, "num_layers": 2, "num_heads": 4, "intermediate_dimension_size": 96}'
GNN_SPEC = '{"hidden_state_size": 64, "num_layers": 4}'
NAN, INF = float("nan"), float("inf")


def _minibatch(samples):
    """samples: (location values, key nodes, rewrite values, rewrite nodes, target) -> (src fp32, EvalIndices); every value
    gets its own place in src"""
    from buglab.models._evaluate import EvalIndices

    src, loc_idx, key_node, rw_idx, rw_node, loc_off, rw_off, tgt = [], [], [], [], [], [0], [0], []
    for loc, keys, rw, nodes, target in samples:
        assert len(loc) == len(keys) and len(rw) == len(nodes)
        loc_idx += range(len(src), len(src) + len(loc))
        src += list(loc)
        rw_idx += range(len(src), len(src) + len(rw))
        src += list(rw)
        key_node += list(keys)
        rw_node += list(nodes)
        loc_off.append(len(loc_idx))
        rw_off.append(len(rw_idx))
        tgt.append(target)
    i32 = lambda a: np.asarray(a, dtype=np.int32)
    return np.asarray(src, dtype=np.float32), EvalIndices(i32(loc_idx), i32(loc_off), i32(key_node), i32(rw_idx), i32(rw_off), i32(rw_node), i32(tgt))


def _device_indices(ix):
    from buglab.controllers._batching import to_device_i32
    from buglab.models import hip_ops

    return dict(zip(hip_ops.EVAL_INDEX_FIELDS, to_device_i32([getattr(ix, f) for f in hip_ops.EVAL_INDEX_FIELDS], DEV)))


def _judge(src, ix, assume_buggy=False, capacity=None, offset=0, into=None):
    from buglab.models import hip_ops

    B = ix.tgt_rw.shape[0]
    capacity = B if capacity is None else capacity
    conf, verdict = into if into is not None else (torch.full((capacity,), 123.0, dtype=torch.float64, device=DEV),
                                                   torch.full((4, capacity), 77, dtype=torch.int32, device=DEV))
    hip_ops.eval_judge(torch.from_numpy(src).to(DEV), _device_indices(ix), conf, verdict, offset, assume_buggy=assume_buggy)
    return conf, verdict


def _assert_bit_equal(conf, verdict, want_conf, want_verdict):
    assert verdict.dtype == want_verdict.dtype and verdict.tolist() == want_verdict.tolist()
    nan = np.isnan(want_conf)
    assert conf.dtype == want_conf.dtype and (np.isnan(conf) == nan).all()
    assert conf[~nan].tobytes() == want_conf[~nan].tobytes()


def _handcrafted():
    many_loc = [-3.0 - 0.01 * i for i in range(70)]
    many_loc[66] = many_loc[68] = -0.25  # the maximum in the second wave, and again behind it
    many_rw = [-2.0 - 0.001 * i for i in range(300)]
    many_rw[299] = -0.5  # beyond the workgroup's first stride
    return [
        # 0  nothing but NO_BUG, no rewrites
        ([-0.5], [-1], [], [], -1),
        # 1  ties: the first key of the location maximum, the lowest index of the rewrite maximum; a NaN inside never wins
        ([-1.0, NAN, -0.5, -0.5, -2.0], [2, 0, 1, 3, -1], [-1.0, -0.25, NAN, -0.25, -0.25, 0.0], [0, 1, 1, 1, 1, 3], 1),
        # 2  every rewrite at the predicted node is -inf: "none", so not repaired although the location is right
        ([-0.1, -3.0, -4.0], [0, 1, -1], [-INF, -INF, -1.0], [0, 0, 1], 0),
        # 3  a NaN in front wins; a NaN rewrite never does; the target's node (2) has no key but its best rewrite is found
        ([NAN, -0.5, -1.0], [0, 1, -1], [NAN, -2.0, -1.0, -0.75], [0, 0, 2, 2], 3),
        # 4  correct code, NO_BUG predicted: location correct and repaired
        ([-2.0, -3.0, -0.1], [0, 1, -1], [-0.5, -0.5], [0, 1], -1),
        # 5  correct code that warns; 70 entries, the maximum at entry 66
        (many_loc + [-1.0], list(range(70)) + [-1], [-0.5] * 70, list(range(70)), -1),
        # 6  300 rewrites at one node, the maximum at index 299
        ([-0.2, -2.0], [0, -1], many_rw, [0] * 300, 299),
    ]


def test_kernel_equals_the_twin_on_handcrafted_samples():
    from buglab.models import _evaluate as E

    src, ix = _minibatch(_handcrafted())
    assert ix.tgt_rw.shape[0] == 7
    want_conf, want_verdict = E.judge_host(src, ix)
    # what the samples are there for, stated once so that the twin cannot hide a shared mistake
    assert want_verdict.T.tolist() == [[0, 1, -1, 1], [1, 1, 1, 1], [1, 1, 0, 0], [1, 0, 1, 0], [0, 1, -1, 1], [1, 0, -1, 0], [1, 1, 1, 1]]
    assert np.isnan(want_conf[3]) and want_conf[[0, 1, 2, 4, 5, 6]].tolist() == [float(np.float32(x)) for x in (-0.5, -0.5, -0.1, -0.1, -0.25, -0.2)]
    runs = []
    for _ in range(2):
        conf, verdict = _judge(src, ix)
        runs.append((conf.cpu().numpy(), verdict.cpu().numpy()))
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()  # run to run
    _assert_bit_equal(*runs[0], want_conf, want_verdict)


@pytest.mark.parametrize("seed", [0, 1])
def test_kernel_equals_the_twin_on_drawn_minibatches(seed):
    """50 samples on a coarse grid (ties everywhere), -inf and NaN sprinkled in, up to 600 locations and 900 rewrites"""
    from buglab.models import _evaluate as E

    rng = np.random.default_rng(seed)
    samples = []
    for b in range(50):
        n_nodes = int(rng.integers(300, 600)) if b % 10 == 0 else int(rng.integers(1, 12))
        keys = rng.permutation(n_nodes)[:n_nodes if b % 10 == 0 else int(rng.integers(1, n_nodes + 1))].tolist()  # some nodes have no key
        n_rw = int(rng.integers(0, 900 if b % 10 == 5 else 40))
        nodes = rng.integers(0, n_nodes, size=n_rw).tolist()
        draw = lambda n: np.where(rng.uniform(size=n) < 0.15, -INF, np.where(rng.uniform(size=n) < 0.03, NAN, np.round(np.log(rng.uniform(0.02, 1.0, size=n)) * 2) / 2))
        target = int(rng.integers(0, n_rw)) if n_rw and rng.uniform() < 0.6 else -1
        samples.append((draw(len(keys) + 1).tolist(), keys + [-1], draw(n_rw).tolist(), nodes, target))
    src, ix = _minibatch(samples)
    want_conf, want_verdict = E.judge_host(src, ix)
    assert len({tuple(v) for v in want_verdict.T.tolist()}) >= 5  # the draws reach the verdicts there are
    assert int(np.diff(ix.loc_off).max()) > 256 and int(np.diff(ix.rw_off).max()) > 256  # more than one stride of the workgroup
    conf, verdict = _judge(src, ix)
    _assert_bit_equal(conf.cpu().numpy(), verdict.cpu().numpy(), want_conf, want_verdict)


def test_offset_writes_into_run_long_buffers():
    from buglab.models import _evaluate as E
    from buglab.models import hip_ops

    first, second = _minibatch(_handcrafted()), _minibatch(_handcrafted()[::-1][:5])
    buffers = _judge(*first, capacity=20, offset=3)
    _judge(*second, offset=12, into=buffers)
    conf, verdict = buffers[0].cpu().numpy(), buffers[1].cpu().numpy()
    for (src, ix), at in ((first, 3), (second, 12)):
        B = ix.tgt_rw.shape[0]
        want_conf, want_verdict = E.judge_host(src, ix)
        _assert_bit_equal(conf[at:at + B], verdict[:, at:at + B], want_conf, want_verdict)
    untouched = np.r_[0:3, 10:12, 17:20]
    assert (conf[untouched] == 123.0).all() and (verdict[:, untouched] == 77).all()
    # a minibatch that does not fit is refused before anything is launched
    with pytest.raises(ValueError, match="do not fit"):
        _judge(*first, offset=14, into=buffers)
    with pytest.raises(ValueError, match="inconsistent shapes"):
        hip_ops.eval_judge(torch.from_numpy(first[0]).to(DEV), dict(_device_indices(first[1]), key_node=torch.zeros(1, dtype=torch.int32, device=DEV)),
                           *buffers, 0)
    assert buffers[0].cpu().numpy().tobytes() == conf.tobytes() and buffers[1].cpu().numpy().tobytes() == verdict.tobytes()  # nothing was written


def test_kernel_with_assume_buggy():
    from buglab.models import _evaluate as E

    rng = np.random.default_rng(7)
    samples = []
    for b in range(40):
        n_nodes = (2, 64, 63, 1)[b] if b < 4 else int(rng.integers(1, 65))  # at most 64 entries besides NO_BUG
        values = rng.uniform(-20.0, 0.0, size=n_nodes + 1)
        if b % 3 == 0:
            values = np.round(values)  # ties
        n_rw = int(rng.integers(1, 30))
        samples.append((values.tolist(), rng.permutation(n_nodes).tolist() + [-1], rng.uniform(-20.0, 0.0, size=n_rw).tolist(),
                        rng.integers(0, n_nodes, size=n_rw).tolist(), int(rng.integers(0, n_rw))))
    src, ix = _minibatch(samples)
    assert src.min() >= -20.0 and src.max() <= 0.0 and int(np.diff(ix.loc_off).max()) == 65
    want_conf, want_verdict = E.judge_host(src, ix, assume_buggy=True)
    assert (want_verdict[0] == 1).all() and want_conf[3] == 0.0  # one candidate: log-probability 0 once NO_BUG is gone
    runs = []
    for _ in range(2):
        conf, verdict = _judge(src, ix, assume_buggy=True)
        runs.append((conf.cpu().numpy(), verdict.cpu().numpy()))
    assert runs[0][0].tobytes() == runs[1][0].tobytes()
    conf, verdict = runs[0]
    assert verdict.tolist() == want_verdict.tolist()
    worst = np.abs(conf - want_conf).max()
    print(f"\n[evaluate] assume_buggy: worst |kernel - twin| confidence {worst:.3e}")
    assert worst <= 1e-12
    # NO_BUG is really left out: raising it above everything changes nothing
    src2 = src.copy()
    src2[ix.loc_idx[ix.loc_off[1:] - 1]] = 0.0
    conf2, verdict2 = _judge(src2, ix, assume_buggy=True)
    assert conf2.cpu().numpy().tobytes() == conf.tobytes() and verdict2.cpu().numpy().tolist() == verdict.tolist()


# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """family -> (model file, data, data folder): as tests/test_visualize_gpu.py::trained -- gnn-mlp briefly trained on the
    synthetic data, seq-great with seeded weights"""
    from buglab.data.synthetic import make_report_dataset
    from buglab.models import train
    from buglab.models.modelregistry import load_model
    from buglab.utils.msgpackutils import save_msgpack_l_gz

    out = {}
    root = tmp_path_factory.mktemp("gnn_mlp")
    data = make_report_dataset(230, seed=31, kind="graph")
    for name, part in (("train", data[:80]), ("valid", data[80:100]), ("test", data[100:])):
        (root / name).mkdir()
        save_msgpack_l_gz(part, root / name / "x.msgpack.l.gz")
    path = root / "detector.pkl.gz"
    train.run(train.parse_args(["gnn-mlp", str(root / "train"), str(root / "valid"), str(path), "--max-num-epochs", "2", "--minibatch-size", "16",
                                "--quiet", "--sequential", "--model-spec", GNN_SPEC]))
    out["gnn-mlp"] = (path, data[100:], root / "test")
    root = tmp_path_factory.mktemp("seq_great")
    data = make_report_dataset(230, seed=31, kind="seq")
    path = root / "detector.pkl.gz"
    model = load_model(dict(json.loads(SEQ_SPEC), modelName="seq-great", dropout_rate=0.1), path)[0]
    model.compute_metadata(copy.deepcopy(data))
    torch.manual_seed(5)
    model.save(path, model.build_neural_module())
    out["seq-great"] = (path, data[100:], None)
    return out


def _restore(path):
    from buglab.runtime.neuralmodel import AbstractNeuralModel

    return AbstractNeuralModel.restore_model(Path(path), torch.device(DEV))


def _twin_report(model, nn_, data, assume_buggy):
    """`evaluate_on_device` with the NumPy twin in the kernel's place: the same minibatches and forward, the flat output copied
    to the host"""
    from buglab.controllers import _batching as Bt
    from buglab.models import _evaluate as E
    from buglab.models.evaluate import ColumnarEvaluationReport

    extend = lambda layout, points, dev, mb: (E.eval_indices(layout, points, mb.get("node_mappings")), points)
    confs, verdicts, points = [], [], []
    nn_.eval()
    with torch.no_grad(), model._tensorize_all_location_rewrites():
        for mb, _ in Bt.prediction_minibatches(model, ((d, None) for d in data), torch.device(DEV), False, extend, lambda tag: None,
                                               extend_sees_minibatch=True):
            conf, verdict = E.judge_host(Bt.flat_prediction_output(nn_, mb).cpu().numpy(), mb["selfsup"][0], assume_buggy)
            confs.append(conf), verdicts.append(verdict), points.extend(mb["selfsup"][1])
    conf, verdict = np.concatenate(confs), np.concatenate(verdicts, axis=1)
    scouts = ["NoBug" if p["target_fix_action_idx"] is None else p["candidate_rewrite_metadata"][p["target_fix_action_idx"]][0] for p in points]
    names = ["NoBug"] + sorted(set(scouts) - {"NoBug"})
    return ColumnarEvaluationReport(conf, [s != "NoBug" for s in scouts], verdict[0] != 0, verdict[1] != 0, verdict[2], verdict[3] != 0,
                                    [names.index(s) for s in scouts], names)


@pytest.mark.parametrize("family", ["gnn-mlp", "seq-great"])
def test_on_device_report_is_the_host_report(family, trained):
    from buglab.models.evaluate import evaluate_on_device, evaluate_predictions

    path, data, _ = trained[family]
    model, nn_ = _restore(path)
    device = torch.device(DEV)
    predictions = list(model.predict(iter(data), nn_, device, False))
    assert len(predictions) == len(data) == 130  # three minibatches
    host = evaluate_predictions(predictions)
    report = evaluate_on_device(model, nn_, data, device, parallelize=False)
    assert report.format() == host.format()
    s = host.summary()
    assert 0 < s["num_buggy_samples"] < s["num_samples"] == 130
    # a stream of unknown length, collated in worker threads
    assert evaluate_on_device(model, nn_, iter(data), device, parallelize=True, capacity=1).format() == host.format()
    # --eval-only-no-bug
    clean = evaluate_predictions(predictions, eval_only_no_bug=True)
    assert clean.summary()["num_samples"] == s["num_samples"] - s["num_buggy_samples"]
    assert evaluate_on_device(model, nn_, data, device, eval_only_no_bug=True, parallelize=False).format() == clean.format()

    # --assume-buggy on the buggy samples: the host renormalises in fp32 (torch.logsumexp), the kernel in fp64, so the counts
    # are the host's and the curves are the twin's
    buggy = [d for d in data if d["target_fix_action_idx"] is not None]
    host = evaluate_predictions(model.predict(iter(buggy), nn_, device, False), assume_buggy=True).format()
    report = evaluate_on_device(model, nn_, buggy, device, assume_buggy=True, parallelize=False)
    text = report.format()
    head = lambda t: t[:t.index("x = np.")]
    assert head(text) == head(host) and "Repair Accuracy Given Location" in head(text)
    twin = _twin_report(model, nn_, buggy, assume_buggy=True)
    gaps = np.diff(np.sort(twin.confidence))
    print(f"\n[evaluate] {family} assume_buggy: smallest gap between two confidences {gaps.min():.3e}")
    assert gaps.min() >= 1e-6  # no rank can flip on a difference of 1e-12
    assert np.abs(report.confidence - twin.confidence).max() <= 1e-12
    got, want = report.summary(), twin.summary()  # (without correct code two of the ratios are NaN)
    assert list(got) == list(want) and all(got[k] == want[k] or (got[k] != got[k] and want[k] != want[k]) for k in want)
    assert report.per_scout() == twin.per_scout()
    got, want = report.curves(), twin.curves()
    assert list(got) == list(want)
    for name in want:
        np.testing.assert_allclose(got[name], want[name], rtol=0, atol=1e-9, equal_nan=True, err_msg=name)
    with pytest.raises(AssertionError):  # a sample without a bug, as the host path's assertion
        evaluate_on_device(model, nn_, data[:10], device, assume_buggy=True, parallelize=False)


def _cli(args, timeout=420):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "buglab.models.evaluate"] + [str(a) for a in args], cwd=PKG, capture_output=True, text=True,
                          timeout=timeout, env=env)


def test_cli_on_device_prints_the_report_and_writes_it_as_data(trained, tmp_path):
    from buglab.models.evaluate import evaluate_on_device
    from buglab.utils.msgpackutils import load_all_msgpack_l_gz

    path, _, folder = trained["gnn-mlp"]
    blob = tmp_path / "report.json"
    r = _cli([path, folder, "--on-device", "--report-json", blob])
    assert r.returncode == 0, r.stderr[-3000:]
    model, nn_ = _restore(path)
    report = evaluate_on_device(model, nn_, list(load_all_msgpack_l_gz(folder)), DEV)  # the samples as evaluate.py reads them back
    assert r.stdout == report.format()
    data = json.loads(blob.read_text())
    s = report.summary()
    assert s["num_samples"] == 130
    assert {k: data["summary"][k] for k in s if k.startswith("num_")} == {k: v for k, v in s.items() if k.startswith("num_")}
    assert data["per_scout"] == report.per_scout() and sorted(data["curves"]) == sorted(report.curves())
    assert all(len(v) == 100 for v in data["curves"].values())


def test_cli_on_device_refuses_an_ensemble(trained, tmp_path):
    path, _, folder = trained["gnn-mlp"]
    ens = tmp_path / "ens.pkl.gz"
    r = subprocess.run([sys.executable, "-m", "buglab.models.ensemble", str(ens), "avg", str(path)], cwd=PKG, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = _cli([ens, folder, "--on-device"])
    assert r.returncode != 0 and "Accuracy" not in r.stdout
    assert "TypeError" in r.stderr and "ensembles (EnsembleWrapper) are not supported here" in r.stderr
