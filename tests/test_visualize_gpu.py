"""GPU: the bug report on the MI355X -- the two kernels of csrc/bl_report.hip against the contexts recorded from the reference
(tests/golden/visualize_contexts.json.gz) and against Python's stable sort, bit for bit; `scan` on the device against
`model.predict` followed by the dict-based restatement of tests/visualize_ref.py on the host; the CLI.

End to end, which comparison and why: `scan` forms the minibatches `predict` forms, so for graph models everything is compared
bit for bit, with no tolerance path.  For sequence models a sample's fp32 log-probabilities may depend on what shares its
minibatch ("Self-supervision services": seq-great at most 3.6e-7 on these log-probabilities); a sample whose values
are not bit-equal takes the tolerance path (SEQ_LOGPROB_BOUND), the orders must agree wherever no two keys are closer than that
bound, and fewer than 1 % of the samples may take the tolerance path at all (asserted; the share is printed).
"""
import copy
import gzip
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import visualize_ref as VR
from tests.conftest import PKG, ROOT
from tests.test_visualize_host import FLAGS, assert_same_context, bits, fixture_predictions

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEQ_LOGPROB_BOUND = 3.6e-7  # DESIGN.md, "Self-supervision services": seq-great across minibatch compositions
SEQ_SPEC = '{"hidden_state_size": 64, "num_layers": 2, "num_heads": 4, "intermediate_dimension_size": 96}'
GNN_SPEC = '{"hidden_state_size": 64, "num_layers": 4}'

with gzip.open(os.path.join(ROOT, "tests", "golden", "visualize_contexts.json.gz"), "rt") as f:
    FIXTURE = json.load(f)


def _device_indices(ix):
    from buglab.controllers._batching import to_device_i32
    from buglab.models import hip_ops

    return dict(zip(hip_ops.REPORT_INDEX_FIELDS, to_device_i32([getattr(ix, f) for f in hip_ops.REPORT_INDEX_FIELDS], DEV)))


# ------------------------------------------------------------------------------------------------------------------------------
def test_summarize_kernel_reproduces_the_reference():
    from buglab.models import _report as R
    from buglab.models import hip_ops
    from buglab.models.visualize import triples_indices

    triples = fixture_predictions()
    flat64, ix, groups, keys = triples_indices(triples)
    flat = flat64.astype(np.float32)
    assert (flat.astype(np.float64) == flat64).all()  # every recorded log-probability is an fp32 number
    src = torch.from_numpy(flat).to(DEV)
    dev_ix = _device_indices(ix)
    outs = [[t.cpu().numpy() for t in hip_ops.report_summarize(src, dev_ix)] for _ in range(2)]
    torch.cuda.synchronize()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(*outs))  # run to run
    best_rw, best_range, si, sd = outs[0]
    contexts = FIXTURE["contexts"]
    assert si[2].tolist() == [int(c["is_wrong"]) for c in contexts]
    assert [bits(x) for x in sd[0].tolist()] == [bits(c["prediction_logprob"]) for c in contexts]
    checked = 0
    for b, ((point, loc, rw), ctx) in enumerate(zip(triples, contexts)):
        assert int(si[0, b]) == list(loc).index(max(loc, key=lambda k: loc[k]))  # the reference's own expression
        assert int(si[1, b]) == int(max(loc, key=lambda k: loc[k]) == -1) and float(sd[1, b]) == loc[-1]
        g0 = int(ix.grp_off[b])
        by_range = {f"({r[0][0]},{r[0][1]})-({r[1][0]},{r[1][1]})": g0 + g for g, r in enumerate(groups[b].ranges)}
        members = {g: [i for i, x in enumerate(groups[b].rw_grp.tolist()) if x == g - g0] for g in by_range.values()}
        for seg in ctx["segments"]:
            for t in seg.get("target_ranges", ()):
                g = by_range[t["range"]]
                assert bits(float(best_range[g])) == bits(t["best_range_logprob"]), (ctx["package"], t["range"])
                local = [rw[i] for i in members[g]]
                assert int(best_rw[g]) == members[g][local.index(max(local))]  # first maximum, as max(..., key=) picks
                if t["is_ground_range"]:  # the recorded "predicted" marks name the rewrite VALUE the reference predicts
                    predicted = point["candidate_rewrites"][int(best_rw[g])]
                    assert [r["is_predicted"] for r in t["rewrites"]] == [point["candidate_rewrites"][i] == predicted for i in members[g]]
                checked += 1
    assert checked > 500
    # the groups the page does not show (colliding ranges) and everything else: the NumPy twin, which the host tests pin
    host = R.summarize_host(flat, ix)
    for got, want in zip(outs[0], host):
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000, 4097, 2 ** 17 + 3])
def test_order_kernel_equals_pythons_stable_sort(n):
    from buglab.models import hip_ops

    rng = np.random.default_rng(n + 1)
    keys = np.round(rng.normal(size=n) * 3) / 4 if n < 5000 else np.round(rng.normal(size=n) * 300) / 4  # ties at every size
    keys[rng.uniform(size=n) < 0.15] = -np.inf
    dkeys = torch.from_numpy(keys).to(DEV)
    by_key = sorted(range(n), key=lambda i: -keys[i])  # Python's stable sort of everything; a kept subset keeps this order
    for density in (0.0, 0.02, 0.5, 1.0):
        keep = (rng.uniform(size=n) < density).astype(np.int32) if 0.0 < density < 1.0 else np.full(n, int(density), np.int32)
        dkeep = torch.from_numpy(keep).to(DEV)
        want_sorted = [i for i in by_key if keep[i]]
        want_input = [i for i in range(n) if keep[i]]
        for k in (0, 1, n, n + 5):
            if n > 5000 and k not in (0, 1):
                continue
            got = hip_ops.report_order(dkeys, dkeep, by_confidence=True, k=k).cpu().numpy()
            assert got.dtype == np.int32 and got.tolist() == (want_sorted[:k] if k > 0 else want_sorted)
            again = hip_ops.report_order(dkeys, dkeep, by_confidence=True, k=k).cpu().numpy()
            assert got.tobytes() == again.tobytes()
            plain = hip_ops.report_order(dkeys, dkeep, by_confidence=False, k=k).cpu().numpy()
            assert plain.tolist() == (want_input[:k] if k > 0 else want_input)


def test_order_kernel_full_k_at_the_largest_size():
    from buglab.models import hip_ops

    n = 2 ** 17 + 3
    rng = np.random.default_rng(2)
    keys = np.round(rng.normal(size=n) * 50) / 4
    keys[::7] = -np.inf
    keep = (rng.uniform(size=n) < 0.5).astype(np.int32)
    want = [i for i in sorted(range(n), key=lambda i: -keys[i]) if keep[i]]
    for k in (n, n + 5, 50):
        got = hip_ops.report_order(torch.from_numpy(keys).to(DEV), torch.from_numpy(keep).to(DEV), by_confidence=True, k=k).cpu().tolist()
        assert got == want[:k]


# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """family -> (model file, data, data folder): a detector on the synthetic data with source; gnn-mlp briefly trained"""
    from buglab.data.synthetic import make_report_dataset
    from buglab.models import train
    from buglab.utils.msgpackutils import save_msgpack_l_gz

    from buglab.models.modelregistry import load_model

    out = {}
    root = tmp_path_factory.mktemp("gnn_mlp")
    data = make_report_dataset(230, seed=31, kind="graph")
    for name, part in (("train", data[:80]), ("valid", data[80:100]), ("scan", data[100:])):
        (root / name).mkdir()
        save_msgpack_l_gz(part, root / name / "x.msgpack.l.gz")
    path = root / "detector.pkl.gz"
    train.run(train.parse_args(["gnn-mlp", str(root / "train"), str(root / "valid"), str(path), "--max-num-epochs", "2", "--minibatch-size", "16",
                                "--quiet", "--sequential", "--model-spec", GNN_SPEC]))
    out["gnn-mlp"] = (path, data[100:], root / "scan")
    # seq-great as the self-supervision GPU tests set their sequence models up: metadata from the data, seeded weights, saved
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


def _compare(family, report, predictions, only_incorrect, by_confidence, top_k):
    """`scan`'s report against predict + the restatement -> the number of samples that took the tolerance path"""
    contexts, shown, everything = VR.report(predictions, only_incorrect, by_confidence, top_k)
    assert report.num_scanned == len(predictions)  # no sample predict yields is skipped
    exact = family.startswith("gnn")
    want_keys = np.array([c["prediction_logprob"] for c in everything])
    same = np.array([bits(a) == bits(b) for a, b in zip(report.prediction_logprob.tolist(), want_keys.tolist())])
    loose = 0
    if exact:
        assert same.all() and report.is_wrong.tolist() == [c["is_wrong"] for c in everything]
        assert report.selected.tolist() == shown
        for ctx, want, i in zip(report.snippets, contexts, shown):
            assert_same_context(ctx, want, (family, i))
        return 0
    loose = int((~same).sum())
    assert np.abs(report.prediction_logprob[~same] - want_keys[~same]).max(initial=0.0) <= SEQ_LOGPROB_BOUND
    if loose == 0:
        assert report.is_wrong.tolist() == [c["is_wrong"] for c in everything] and report.selected.tolist() == shown
        for ctx, want, i in zip(report.snippets, contexts, shown):
            assert_same_context(ctx, want, (family, i))
    else:  # equal selections only where no two keys are closer than the bound
        gaps = np.diff(np.sort(want_keys[np.isfinite(want_keys)]))
        if not (by_confidence and ((gaps > 0) & (gaps <= 2 * SEQ_LOGPROB_BOUND)).any()) and \
                report.is_wrong.tolist() == [c["is_wrong"] for c in everything]:
            assert report.selected.tolist() == shown
    return loose


@pytest.mark.parametrize("family", ["gnn-mlp", "seq-great"])
def test_scan_equals_predict_and_the_restatement(family, trained, monkeypatch):
    from buglab.models.visualize import sampled, scan

    path, data, _ = trained[family]
    model, nn_ = _restore(path)
    predict = lambda points: list(model.predict(iter(points), nn_, torch.device(DEV), False))
    predictions = predict(data)
    assert len(predictions) == len(data) == 130  # three minibatches
    loose = total = 0
    for only_incorrect, by_confidence in FLAGS:
        for top_k in (0, 7):
            report = scan(model, nn_, iter(data), DEV, parallelize=by_confidence, only_incorrect=only_incorrect,
                          order_by_confidence=by_confidence, show_top_k=top_k)
            loose += _compare(family, report, predictions, only_incorrect, by_confidence, top_k)
            total += len(predictions)
            assert all(p is q for (p, _, _), q in zip(predictions, data))
    wrong = sum(VR.sample_context(*t)["is_wrong"] for t in predictions)
    assert 0 < wrong  # --only-incorrect has something to keep (and, with 130 samples, something to drop is not required)
    # --num-elements smaller than the data; --only-no-bug
    few = list(sampled(iter(data), 70, 1.0))
    assert len(few) == 70
    loose += _compare(family, scan(model, nn_, iter(few), DEV, only_incorrect=True, order_by_confidence=True), predict(few), True, True, 0)
    clean = [d for d in data if d["target_fix_action_idx"] is None]
    assert 0 < len(clean) < len(data)
    loose += _compare(family, scan(model, nn_, iter(clean), DEV, order_by_confidence=True), predict(clean), False, True, 0)
    total += 70 + len(clean)
    # a sample tensorize rejects is skipped, as predict skips it
    real, victim = model.tensorize, data[5]
    monkeypatch.setattr(model, "tensorize", lambda d: None if d is victim else real(d))
    rest = predict(data)
    assert len(rest) == len(data) - 1
    loose += _compare(family, scan(model, nn_, iter(data), DEV, only_incorrect=True, order_by_confidence=True, show_top_k=20), rest, True, True, 20)
    total += len(rest)
    print(f"\n[visualize] {family}: {loose} of {total} compared samples took the tolerance path ({loose / total:.2%})")
    assert loose / total < 0.01


def test_cli_writes_the_page_and_the_data_reproducibly(trained, tmp_path):
    path, data, folder = trained["gnn-mlp"]
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    outs = []
    for i, extra in enumerate((["--sequential"], [])):
        page, blob = tmp_path / f"report_{i}.html", tmp_path / f"report_{i}.json"
        r = subprocess.run([sys.executable, "-m", "buglab.models.visualize", str(path), str(folder), str(page), "--report-json", str(blob),
                            "--only-incorrect", "--order-by-confidence", "--show-only-top-k", "12", "--num-elements", "100"] + extra,
                           cwd=PKG, capture_output=True, text=True, timeout=420, env=env)
        assert r.returncode == 0, r.stderr[-3000:]
        assert "Scanned 100 samples" in r.stdout
        outs.append((page.read_bytes(), blob.read_bytes()))
    assert outs[0] == outs[1]
    report = json.loads(outs[0][1])
    assert report["num_scanned"] == 100 and 0 < len(report["snippets"]) <= 12 and len(report["selected"]) == len(report["snippets"])
    assert all(s["is_wrong"] for s in report["snippets"])
    keys = [s["prediction_logprob"] for s in report["snippets"]]
    assert keys == sorted(keys, reverse=True)
    assert outs[0][0].count(b"<section") == len(report["snippets"]) and outs[0][0].count(b'class="mistake"') == len(report["snippets"])
