"""GPU: model ensembles (buglab.models.ensemble) on the MI355X -- the combine kernel against the reference's own combination
(tests/golden/ensemble_predictions.json.gz, made by tests/golden/make_golden_ensemble.py), ensembles of one member against
the member's own predict, mixed ensembles against a float64 restatement of reference ensemble/wrapper.py:33-89 applied to
the members' own predictions, evaluate.py on an ensemble file, and run-to-run reproducibility."""
import copy
import gzip
import json
import math
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import ensemble_ref as R
from tests.conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

SEQ_SPEC = {"hidden_state_size": 64, "num_layers": 2, "num_heads": 4, "intermediate_dimension_size": 96, "dropout_rate": 0.1}


def _spec(family, **extra):
    if family.startswith("seq"):
        return dict(SEQ_SPEC, modelName=family, **extra)
    return dict({"modelName": family, "hidden_state_size": 64, "dropout_rate": 0.1}, **extra)


def _member(tmp_path, family, data, seed, **extra):
    from buglab.models.modelregistry import load_model

    path = tmp_path / f"{family}_{seed}.pkl.gz"
    model = load_model(_spec(family, **extra), path)[0]
    model.compute_metadata(copy.deepcopy(data))
    torch.manual_seed(seed)
    nn_ = model.build_neural_module()
    model.save(path, nn_)
    return path


def _restore(path):
    from buglab.runtime.neuralmodel import AbstractNeuralModel

    return AbstractNeuralModel.restore_model(Path(path), torch.device("cuda"))


def _build_ensemble(tmp_path, kind, paths, name="ens.pkl.gz"):
    out = tmp_path / name
    r = subprocess.run([sys.executable, "-m", "buglab.models.ensemble", str(out), kind] + [str(p) for p in paths], cwd=PKG,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return out


def _predict(path, data, parallelize=False):
    model, nn_ = _restore(path)
    return list(model.predict(iter(data), nn_, torch.device("cuda"), parallelize))


def _assert_close(got, want, atol=1e-12):
    assert len(got) == len(want)
    for (p, gl, gr), (q, wl, wr) in zip(got, want):
        assert p is q
        assert list(gl) == list(wl)
        a, b = np.array(list(gl.values()), np.float64), np.array(list(wl.values()), np.float64)
        np.testing.assert_allclose(a, b, rtol=0, atol=atol, equal_nan=True)
        assert (np.isneginf(a) == np.isneginf(b)).all()
        np.testing.assert_allclose(np.array(gr, np.float64), np.array(wr, np.float64), rtol=0, atol=atol, equal_nan=True)


# ------------------------------------------------------------------------------------------------------------------------------
with gzip.open(os.path.join(ROOT, "tests", "golden", "ensemble_predictions.json.gz"), "rt") as f:
    FIXTURE = json.load(f)


def _wide_case(kind):
    """A case in the fixture's format whose samples have 65 location entries (64 nodes and NO_BUG: one more than a wave), which
    the fixture's samples (at most 9) never reach; expected values from the float64 restatement (tests/ensemble_ref.py) on the
    fp32 inputs.  Sample 0: every member's maximum is the entry past the wave, so there is consensus; sample 1: one member's
    maximum is tied with an earlier entry, so the first-maximum rule breaks it; sample 2: a member is absent, and another has
    a NaN and a -inf among its entries."""
    rng = np.random.default_rng(65)
    M, n_nodes, n_rw = 3, 64, 70
    nodes = sorted(rng.choice(500, n_nodes, replace=False).tolist())
    samples = []
    for s in range(3):
        members = []
        for m in range(M):
            loc = rng.normal(-3.0, 1.0, n_nodes + 1).astype(np.float32)
            rw = rng.normal(-2.0, 1.0, n_rw).astype(np.float32)
            loc[64] = 2.0 + m  # the greatest, in lane 0's second round
            if s == 1 and m == 1:
                loc[7] = loc[64]
            if s == 2 and m == 1:
                loc[5], loc[9], rw[3] = np.nan, -np.inf, -np.inf
            members.append(None if (s == 2 and m == 0) else [loc.tolist(), rw.tolist()])
        samples.append({"nodes": nodes, "n_rw": n_rw, "members": members})
    expected = []
    for i, s in enumerate(samples):
        preds = [None if mem is None else (dict(zip(nodes + [-1], mem[0])), mem[1]) for mem in s["members"]]
        loc, rw = R.combine(kind, preds)
        expected.append({"id": i, "location_logprobs": [[k, float(v)] for k, v in loc.items()], "rewrite_logprobs": [float(v) for v in rw]})
    return {"name": f"{kind}_m3_65_entries", "M": M, "kind": kind, "samples": samples, "expected": expected}


@pytest.mark.parametrize("case", FIXTURE["cases"] + [_wide_case("avg"), _wide_case("consensus")], ids=lambda c: c["name"])
def test_combine_kernel_reproduces_the_reference(case):
    from buglab.models import hip_ops

    M, samples = case["M"], case["samples"]
    kept = [i for i, s in enumerate(samples) if any(m is not None for m in s["members"])]
    assert [e["id"] for e in case["expected"]] == kept  # the reference skips a sample no member predicts
    src, loc_idx, rw_idx = [], [[] for _ in range(M)], [[] for _ in range(M)]
    loc_off, rw_off = [0], [0]
    for i in kept:
        s = samples[i]
        for m, mem in enumerate(s["members"]):
            if mem is None:
                loc_idx[m] += [-1] * (len(s["nodes"]) + 1)
                rw_idx[m] += [-1] * s["n_rw"]
                continue
            n = sum(len(x) for x in src)
            loc_idx[m] += list(range(n, n + len(mem[0])))
            rw_idx[m] += list(range(n + len(mem[0]), n + len(mem[0]) + len(mem[1])))
            src.append(np.asarray(mem[0] + mem[1], dtype=np.float32))
        loc_off.append(loc_off[-1] + len(s["nodes"]) + 1)
        rw_off.append(rw_off[-1] + s["n_rw"])
    dev = lambda a, dt: torch.tensor(np.asarray(a), dtype=dt, device="cuda")
    out = hip_ops.ensemble_combine(dev(np.concatenate(src), torch.float32), dev(loc_idx, torch.int32), dev(loc_off, torch.int32),
                                   dev(rw_idx, torch.int32), dev(rw_off, torch.int32), case["kind"])
    got = out.cpu().numpy()
    assert out.dtype == torch.float64
    for b, e in enumerate(case["expected"]):
        want_loc = dict((int(k), v) for k, v in e["location_logprobs"])
        nodes = samples[e["id"]]["nodes"] + [-1]
        assert set(want_loc) == set(nodes)
        w = np.array([want_loc[k] for k in nodes])
        g = got[loc_off[b]:loc_off[b + 1]]
        wr, gr = np.array(e["rewrite_logprobs"]), got[loc_off[-1] + rw_off[b]:loc_off[-1] + rw_off[b + 1]]
        for gg, ww in ((g, w), (gr, wr)):
            assert (np.isnan(gg) == np.isnan(ww)).all() and (np.isneginf(gg) == np.isneginf(ww)).all(), (case["name"], b)
            fin = np.isfinite(ww)
            np.testing.assert_allclose(gg[fin], ww[fin], rtol=0, atol=1e-12, err_msg=f"{case['name']} sample {b}")


@pytest.mark.parametrize("family", ["gnn-mlp", "ggnn", "seq-great", "seq-rat"])
def test_ensemble_of_one_member_is_bit_identical_to_the_member(tmp_path, family):
    from buglab.data.synthetic import make_buglab_dataset, make_buglab_seq_dataset

    data = make_buglab_seq_dataset(60, seed=21) if family.startswith("seq") else make_buglab_dataset(60, seed=21)
    path = _member(tmp_path, family, data, 4)
    own = _predict(path, copy.deepcopy(data))
    points = copy.deepcopy(data)
    ens = _predict(_build_ensemble(tmp_path, "avg", [path]), points)
    assert len(ens) == len(own) == len(data)
    for (p, gl, gr), (q, wl, wr) in zip(ens, own):
        assert p["graph"]["reference_nodes"] == q["graph"]["reference_nodes"]
        assert gl == wl and gr == wr  # every value, bit for bit (dict equality compares floats exactly)
        assert list(gl)[-1] == -1 and list(gl)[:-1] == sorted(gl)[1:]


def _mixed_members(tmp_path, n=70, max_seq_size=45):
    from buglab.data.synthetic import make_buglab_seq_dataset

    data = make_buglab_seq_dataset(n, seed=31)
    paths = [_member(tmp_path, "gnn-mlp", data, 1), _member(tmp_path, "gnn-mlp", data, 2),
             _member(tmp_path, "seq-great", data, 3, max_seq_size=max_seq_size)]  # drops out of the longer samples
    return data, paths


def _restated(kind, paths, data, chunk=50, load=None):
    """Each member's own predict, run over the same chunks of samples the ensemble batches together (50 samples: the gnn-mlp
    members accept every sample), so that every member sees the same minibatches as inside the ensemble -- a sequence
    member's padded length, and so its fp32 outputs, depend on which samples share its minibatch."""
    own = []
    for p in paths:
        points = load() if load is not None else copy.deepcopy(data)
        pos = {id(pt): i for i, pt in enumerate(points)}
        by_index = {i: None for i in range(len(data))}
        for lo in range(0, len(points), chunk):
            for pt, l, r in _predict(p, points[lo:lo + chunk]):
                by_index[pos[id(pt)]] = (l, r)
        own.append(by_index)
    assert all(own[0][i] is not None for i in range(len(data)))
    want = []
    for i in range(len(data)):
        c = R.combine(kind, [None if o[i] is None else (R.canonical(o[i][0]), o[i][1]) for o in own])
        if c is not None:
            want.append((i, c[0], c[1]))
    return want, own


@pytest.mark.parametrize("kind", ["avg", "consensus"])
def test_mixed_ensemble_matches_the_restated_reference(tmp_path, kind):
    data, paths = _mixed_members(tmp_path)
    want, own = _restated(kind, paths, data)
    assert any(o is None for o in own[2].values()) and any(o is not None for o in own[2].values())
    points = copy.deepcopy(data)
    got = _predict(_build_ensemble(tmp_path, kind, paths), points, parallelize=True)
    pos = {id(pt): i for i, pt in enumerate(points)}
    assert [pos[id(p)] for p, _, _ in got] == [i for i, _, _ in want]
    _assert_close(got, [(points[i], l, r) for i, l, r in want])


def test_evaluate_runs_on_an_ensemble_file(tmp_path):
    from buglab.data.synthetic import make_buglab_seq_dataset
    from buglab.models import evaluate
    from buglab.utils.msgpackutils import load_all_msgpack_l_gz, save_msgpack_l_gz

    # one minibatch of at most 50 samples, every member in every sample: evaluate.py shuffles the data, and the composition of
    # each member's minibatch is then the same as in the restatement's own predict
    data, paths = _mixed_members(tmp_path, n=50, max_seq_size=400)
    buggy = [d for d in make_buglab_seq_dataset(40, seed=33) if d["target_fix_action_idx"] is not None]
    ens = _build_ensemble(tmp_path, "avg", paths)
    for name, points, assume_buggy in (("all", data, False), ("buggy", buggy, True)):
        (tmp_path / name).mkdir()
        save_msgpack_l_gz(points, tmp_path / name / "d.msgpack.l.gz")
        summary = evaluate.run({"MODEL_FILENAME": str(ens), "TEST_DATA_PATH": str(tmp_path / name), "--assume-buggy": assume_buggy,
                                "--eval-only-no-bug": False, "--limit-num-elements": None, "--sequential": True})
        # the members' own predictions on the samples as evaluate.py reads them back (the shard reader's graphs)
        load = lambda d=tmp_path / name: list(load_all_msgpack_l_gz(d))
        loaded = load()
        want, _ = _restated("avg", paths, loaded, load=load)
        ref = evaluate.evaluate_predictions([(loaded[i], l, r) for i, l, r in want], assume_buggy=assume_buggy).summary()
        assert summary["num_samples"] == len(want) > 0
        for k, v in ref.items():
            assert (math.isnan(v) and math.isnan(summary[k])) or summary[k] == pytest.approx(v, abs=1e-12), k


def test_two_runs_are_bit_identical(tmp_path):
    data, paths = _mixed_members(tmp_path)
    ens = _build_ensemble(tmp_path, "consensus", paths)
    a = [(l, r) for _, l, r in _predict(ens, copy.deepcopy(data), parallelize=True)]
    b = [(l, r) for _, l, r in _predict(ens, copy.deepcopy(data), parallelize=False)]
    assert len(a) == len(b) > 0
    for (la, ra), (lb, rb) in zip(a, b):
        assert list(la) == list(lb)
        assert np.array_equal(np.array(list(la.values())), np.array(list(lb.values())), equal_nan=True)
        assert np.array_equal(np.array(ra), np.array(rb), equal_nan=True)
