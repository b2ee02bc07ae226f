"""GPU: the self-supervision services (buglab.controllers) on the MI355X -- `score_rewrites` against a float64 restatement of
reference detectordatascoringworker.py:118-130 that goes through the pinned `predict`; the selection kernel's arithmetic
against the reference's own distributions (tests/golden/selfsup_selection.json.gz) and a float64 restatement; its draws against
a host restatement of Gumbel top-k on the same uniforms, and against the exact inclusion probabilities of successive sampling;
`select_rewrites` on a model; and the loop end to end through the two CLIs and `train.py --selector`.

Scoring, which comparison and why ("Self-supervision services"): every model is compared BIT FOR BIT with the
restatement run on the same minibatches (the graphs of all records, 50 at a time -- what `score_rewrites` forms).  Against the
restatement that predicts ONE RECORD AT A TIME, as the reference does, the comparison is bit for bit for the families listed in
BATCH_INDEPENDENT and within LOGPROB_ATOL for the others: a sequence minibatch is padded to its longest sample and a graph
minibatch's segment reductions are tiled over all its graphs, so a sample's fp32 values may depend on what shares its
minibatch.  LOGPROB_ATOL = 1e-4 is the bound the existing predict tests put on a sample's fp32 log-probabilities
(normalisation within 1e-4: test_train_cli_gpu.py, test_seq_gru_gpu.py, test_seq_transformer_gpu.py); no existing test
compares predictions across minibatch compositions, so there is no tighter figure to take over.
"""
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

from tests import selfsup_ref as R
from tests.conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

SEQ_SPEC = {"hidden_state_size": 64, "num_layers": 2, "num_heads": 4, "intermediate_dimension_size": 96, "dropout_rate": 0.1}
LOGPROB_ATOL = 1e-4
BATCH_INDEPENDENT = ("gnn-mlp", "ggnn")  # measured on the MI355X on these records: 0 of 130 scores differ (seq-great 3.6e-7, seq-gru 2.4e-7)
DEV = "cuda"

with gzip.open(os.path.join(ROOT, "tests", "golden", "selfsup_selection.json.gz"), "rt") as f:
    FIXTURE = json.load(f)


def _spec(family, **extra):
    if family.startswith("seq"):
        return dict(SEQ_SPEC, modelName=family, **extra)
    return dict({"modelName": family, "hidden_state_size": 64, "dropout_rate": 0.1}, **extra)


def _data(family, n, seed):
    from buglab.data.synthetic import make_buglab_dataset, make_buglab_seq_dataset

    return make_buglab_seq_dataset(n, seed=seed) if family.startswith("seq") else make_buglab_dataset(n, seed=seed)


def _random_model(family, data, seed):
    from buglab.models.modelregistry import load_model

    model = load_model(_spec(family), Path("/tmp/_bl_selfsup_gpu.pkl.gz"))[0]
    model.compute_metadata(copy.deepcopy(data))
    torch.manual_seed(seed)
    return model, model.build_neural_module().to(DEV).eval()


def _predict(model, nn_, graphs):
    return list(model.predict(iter(graphs), nn_, torch.device(DEV), False))


# ------------------------------------------------------------------------------------------------------------------------------
# scoring
def _restated_scores(model, nn_, records, per_record):
    """reference detectordatascoringworker.py:99-130 on the pinned predict: one record per predict call (`per_record`), or the
    graphs of all records in the minibatches score_rewrites forms (50 graphs per predict call)"""
    out = [[-math.inf] * (len(r["original"]["graph"]["reference_nodes"]) + 1) for r in records]
    stream = [(k, -1 if key == "NO_BUG" else int(key), graph) for k, r in enumerate(records) for key, (graph, _) in r["rewrites"].items()]
    chunks = [[s for s in stream if s[0] == k] for k in range(len(records))] if per_record else \
        [stream[i:i + 50] for i in range(0, len(stream), 50)]
    for chunk in chunks:
        preds = _predict(model, nn_, [g for _, _, g in chunk])
        assert len(preds) == len(chunk)
        for (k, idx, graph), (point, loc, rw) in zip(chunk, preds):
            assert point is graph
            out[k][idx] = R.target_logprob(point, loc, rw)
    return out


@pytest.mark.parametrize("family", ["gnn-mlp", "ggnn", "seq-great", "seq-gru"])
def test_scoring_equals_the_restated_reference(family):
    from buglab.controllers.detectorscoring import score_rewrites
    from buglab.data.synthetic import make_scoring_records

    data = _data(family, 26, seed=41)
    model, nn_ = _random_model(family, data, seed=5)
    records = make_scoring_records(data, seed=6)  # 26 x 5 graphs: three minibatches, records spanning them
    got = [o["candidate_rewrite_logprobs"] for o in score_rewrites(model, nn_, copy.deepcopy(records), DEV, parallelize=True)]
    assert len(got) == len(records) and sum(math.isfinite(v) for g in got for v in g) == 26 * 5
    same = _restated_scores(model, nn_, copy.deepcopy(records), per_record=False)
    assert got == same  # fp64, bit for bit
    alone = _restated_scores(model, nn_, copy.deepcopy(records), per_record=True)
    fin = np.isfinite(np.concatenate(alone))
    assert (fin == np.isfinite(np.concatenate(got))).all()
    diff = np.abs(np.concatenate(got)[fin] - np.concatenate(alone)[fin])
    print(f"\n[selfsup] {family}: batched vs one record at a time: max |diff| {diff.max():.3e}, {int((diff > 0).sum())} of {diff.size} differ")
    assert diff.max() <= LOGPROB_ATOL
    if family in BATCH_INDEPENDENT:
        assert got == alone
    again = [o["candidate_rewrite_logprobs"] for o in score_rewrites(model, nn_, copy.deepcopy(records), DEV, parallelize=False)]
    assert again == got  # run to run, with and without the collate workers


# ------------------------------------------------------------------------------------------------------------------------------
# the selection kernel on given values
def _launch(samples, u_eps, u, temperature, epsilon, k):
    """samples: [(rewrite values, their location values, NO_BUG value)] fp32 -> per sample (logprob, p, entropy, selected)"""
    from buglab.models import hip_ops

    src, rw_idx, rw_loc, rw_off, nobug = [], [], [], [0], []
    pos = 0
    for rw, loc, nb in samples:
        n = len(rw)
        src += [np.asarray(rw, np.float32), np.asarray(loc, np.float32), np.asarray([nb], np.float32)]
        rw_idx += range(pos, pos + n)
        rw_loc += range(pos + n, pos + 2 * n)
        nobug.append(pos + 2 * n)
        pos += 2 * n + 1
        rw_off.append(rw_off[-1] + n)
    dev = lambda a, dt: torch.tensor(np.asarray(a), dtype=dt, device=DEV)
    logprob, p, ent, sel = hip_ops.selector_sample(
        dev(np.concatenate(src), torch.float32), dev(rw_idx, torch.int32), dev(rw_loc, torch.int32), dev(rw_off, torch.int32),
        dev(nobug, torch.int32), dev(u_eps, torch.float64), dev(u, torch.float64), temperature=temperature, epsilon=epsilon, k=k)
    torch.cuda.synchronize()
    logprob, p, ent, sel = logprob.cpu().numpy(), p.cpu().numpy(), ent.cpu().numpy(), sel.cpu().numpy()
    out = []
    for b in range(len(samples)):
        lo, hi = rw_off[b] + b, rw_off[b + 1] + b + 1
        out.append((logprob[lo:hi], p[lo:hi], float(ent[b]), sel[b].tolist(), (lo, hi)))
    return out


def _assert_rel(got, want, rel, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert (np.isnan(got) == np.isnan(want)).all(), what
    fin = ~np.isnan(want)
    assert (np.abs(got[fin] - want[fin]) <= rel * np.abs(want[fin])).all(), (what, float(np.max(np.abs(got[fin] - want[fin]) / np.maximum(np.abs(want[fin]), 1e-300))))


def _fixture_groups():
    groups = {}
    for case in FIXTURE["cases"]:
        groups.setdefault((case["temperature"], case["epsilon"]), []).append(case)
    return sorted(groups.items())


@pytest.mark.parametrize("key,cases", _fixture_groups(), ids=[f"T{k[0]}_eps{k[1]}" for k, _ in _fixture_groups()])
def test_selection_arithmetic_and_draws_on_the_reference_cases(key, cases):
    """One launch per (temperature, epsilon) of the fixture: the reference's own distributions, and the draws."""
    temperature, epsilon = key
    rng = np.random.default_rng(77)
    K = 4
    # the rewrite's value is the fixture's log-probability and its location's is 0: g is the fixture's number exactly
    samples = [(c["logprobs"][:-1], [0.0] * (len(c["logprobs"]) - 1), c["logprobs"][-1]) for c in cases]
    total = sum(len(c["logprobs"]) for c in cases)
    u = rng.random(total)
    out = _launch(samples, [0.5] * len(cases), u, temperature, epsilon, K)  # 0.5 < epsilon only for the forced-uniform cases
    left_out = 0
    for c, (logprob, p, ent, sel, (lo, hi)) in zip(cases, out):
        what = (c["kind"], len(c["logprobs"]))
        assert np.array_equal(logprob, np.asarray(c["logprobs"], np.float64)), what
        _assert_rel(p, c["distribution"], 1e-12, what)                       # the reference's own numbers
        want_p = R.selection_distribution(c["logprobs"], temperature, uniform=epsilon == 1.0)
        _assert_rel(p, want_p, 1e-12, what)
        _assert_rel([ent], [R.entropy(want_p)], 1e-12, what)
        want_sel, gap = R.gumbel_topk(want_p, u[lo:hi], K)
        assert len(want_sel) == min(K, int((want_p > 0).sum()))
        picked = [i for i in sel if i >= 0]
        assert len(picked) == len(want_sel) and sel[len(picked):] == [-1] * (K - len(picked)) and len(set(picked)) == len(picked)
        if gap < 1e-9:
            left_out += 1
            continue
        assert picked == want_sel, what
    assert left_out == 0  # this seed's host keys have no gap below 1e-9 (checked when the test was written); 1 % would be allowed


def test_selection_arithmetic_on_sums_of_two_values():
    """g = rewrite value + location value in fp64 from fp32 inputs, exactly; many samples of mixed sizes in one launch,
    including samples longer than the kernel's key cache (2048 entries)"""
    rng = np.random.default_rng(5)
    sizes = [0, 1, 3, 17, 64, 255, 256, 257, 700, 2047, 2048, 2049, 3000, 4095] + rng.integers(1, 300, size=40).tolist()
    samples = []
    for n in sizes:
        loc = rng.normal(size=n).astype(np.float32) - 2
        samples.append(((rng.normal(size=n) * 1.5 - 3).astype(np.float32), loc, np.float32(-1.5)))
    total = sum(sizes) + len(sizes)
    u, u_eps = rng.random(total), rng.random(len(sizes))
    T, eps, K = 0.7, 0.3, 6
    out = _launch(samples, u_eps, u, T, eps, K)
    assert (u_eps < eps).any() and (u_eps >= eps).any()
    left_out = 0
    for b, ((rw, loc, nb), (logprob, p, ent, sel, (lo, hi))) in enumerate(zip(samples, out)):
        g = np.concatenate([rw.astype(np.float64) + loc.astype(np.float64), [np.float64(nb)]])
        assert np.array_equal(logprob, g), b
        want_p = R.selection_distribution(g, T, uniform=u_eps[b] < eps)
        _assert_rel(p, want_p, 1e-12, b)
        _assert_rel([ent], [R.entropy(want_p)], 1e-12, b)
        want_sel, gap = R.gumbel_topk(want_p, u[lo:hi], K)
        if gap < 1e-9:
            left_out += 1
            continue
        assert [i for i in sel if i >= 0] == want_sel, b
        assert sel[len(want_sel):] == [-1] * (K - len(want_sel))
    assert left_out == 0


def test_draws_follow_successive_sampling_and_shrink_with_zero_entries():
    p = np.array([0.35, 0.05, 0.2, 0.1, 0.25, 0.05])
    N, K = 20000, 2
    lp = np.log(p).astype(np.float32)
    p32 = np.exp(lp.astype(np.float64))
    p32 /= p32.sum()
    rng = np.random.default_rng(2021)
    samples = [(lp[:-1], np.zeros(5, np.float32), lp[-1])] * N
    out = _launch(samples, [0.5] * N, rng.random(6 * N), 1.0, 0.0, K)
    sel = np.array([s[3] for s in out])
    assert sel.shape == (N, K) and (sel >= 0).all() and (sel < 6).all() and (sel[:, 0] != sel[:, 1]).all()
    freq = np.array([(sel == i).any(axis=1).mean() for i in range(6)])
    q = R.inclusion_probabilities(p32, K)
    sd = np.sqrt(q * (1 - q) / N)
    print(f"\n[selfsup] inclusion frequencies {freq.round(4).tolist()} vs exact {q.round(4).tolist()} ({((freq - q) / sd).round(2).tolist()} sd)")
    assert (np.abs(freq - q) <= 5 * sd).all()
    first = np.array([(sel[:, 0] == i).mean() for i in range(6)])  # the first draw alone is a draw from p
    assert (np.abs(first - p32) <= 5 * np.sqrt(p32 * (1 - p32) / N)).all()

    # entries of probability zero are never drawn, and k_b shrinks to what is left
    ninf = np.float32(-np.inf)
    zeros = [(np.array([ninf, -1.0, ninf, ninf], np.float32), np.zeros(4, np.float32), np.float32(-0.5)),   # 2 of 5 entries
             (np.array([ninf], np.float32), np.zeros(1, np.float32), np.float32(-0.1)),                     # NO_BUG alone
             (np.zeros(0, np.float32), np.zeros(0, np.float32), np.float32(0.0))]                           # no candidate at all
    out = _launch(zeros, [0.5] * 3, rng.random(5 + 2 + 1), 1.0, 0.0, 4)
    assert sorted(out[0][3][:2]) == [1, 4] and out[0][3][2:] == [-1, -1]
    assert out[1][3] == [1, -1, -1, -1] and out[2][3] == [0, -1, -1, -1]
    assert out[2][1].tolist() == [1.0] and out[2][2] == 0.0
    assert math.isnan(out[0][2])  # 0 * log 0 = nan, as NumPy in the reference's statistics


# ------------------------------------------------------------------------------------------------------------------------------
# select_rewrites on a model
@pytest.mark.parametrize("family", ["gnn-mlp", "seq-great"])
def test_select_rewrites_on_a_model(family, monkeypatch):
    from buglab.controllers.bugselector import BugSelectionStats, select_rewrites

    data = _data(family, 70, seed=9)
    model, nn_ = _random_model(family, data, seed=3)
    stats = BugSelectionStats()
    points = copy.deepcopy(data)
    got = list(select_rewrites(model, nn_, points, DEV, num_rewrites_per_sample=4, temperature=2.0, epsilon=0.1, seed=123,
                               parallelize=True, stats=stats))
    assert [p is q for (p, _), q in zip(got, points)] == [True] * len(points)
    # the values are the reference's generator_rewrite_logprobs, bit for bit, on the same minibatches (50 + 20)
    ref_points = copy.deepcopy(data)
    preds = _predict(model, nn_, ref_points[:50]) + _predict(model, nn_, ref_points[50:])
    entropy_sum = 0.0
    for (point, reply), (q, loc, rw) in zip(got, preds):
        g = R.selection_logprobs(q, loc, rw)
        n = len(q["candidate_rewrites"])
        assert "NO_BUG" in reply and 4 <= len(reply) <= 5 and all(isinstance(v, float) for v in reply.values())
        assert reply == {k: g[n if k == "NO_BUG" else int(k)] for k in reply}
    assert stats.total_samples == len(data)
    again = list(select_rewrites(model, nn_, copy.deepcopy(data), DEV, num_rewrites_per_sample=4, temperature=2.0, epsilon=0.1, seed=123,
                                 parallelize=False))
    assert [r for _, r in again] == [r for _, r in got] and [list(r) for _, r in again] == [list(r) for _, r in got]
    other = list(select_rewrites(model, nn_, copy.deepcopy(data), DEV, num_rewrites_per_sample=4, temperature=2.0, epsilon=0.1, seed=124))
    assert [list(r) for _, r in other] != [list(r) for _, r in got]
    report = stats.report()
    assert 0.0 < report["entropy"] <= report["uniform_baseline_entropy"] + 1e-9

    # a datapoint the model's tensorize rejects gets the random fallback, in its place
    victim_at = 7
    fresh = copy.deepcopy(data)
    real = model.tensorize
    monkeypatch.setattr(model, "tensorize", lambda d: None if d is fresh[victim_at] else real(d))
    mixed = list(select_rewrites(model, nn_, fresh, DEV, seed=123))
    assert len(mixed) == len(fresh) and mixed[victim_at][0] is fresh[victim_at]
    n = len(fresh[victim_at]["candidate_rewrites"])
    assert set(mixed[victim_at][1].values()) == {1 / (n + 1)} and len(mixed[victim_at][1]) == min(4, n) + 1


# ------------------------------------------------------------------------------------------------------------------------------
# the loop, from files
def _cli(module, *args):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", module] + [str(a) for a in args], cwd=PKG, capture_output=True, text=True, timeout=420, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def test_select_score_train_from_files(tmp_path, caplog):
    from buglab.controllers._batching import save_msgpack_l_gz_reproducibly
    from buglab.data.synthetic import make_buglab_dataset, make_scoring_records
    from buglab.models import train
    from buglab.utils.msgpackutils import load_msgpack_l_gz, save_msgpack_l_gz

    data = make_buglab_dataset(120, seed=17)
    for name, part in (("train", data[:80]), ("valid", data[80:100]), ("pool", data[100:])):
        (tmp_path / name).mkdir()
        save_msgpack_l_gz(part, tmp_path / name / "x.msgpack.l.gz")
    spec = '{"hidden_state_size": 64, "num_layers": 4}'
    detector, selector = tmp_path / "detector.pkl.gz", tmp_path / "selector.pkl.gz"
    for path in (detector, selector):
        train.run(train.parse_args(["gnn-mlp", str(tmp_path / "train"), str(tmp_path / "valid"), str(path), "--max-num-epochs", "2",
                                    "--minibatch-size", "16", "--quiet", "--sequential", "--model-spec", spec]))
        assert path.exists()

    # select: twice with one seed -> the same bytes; another seed -> another selection
    outs = [tmp_path / f"selected_{i}.msgpack.l.gz" for i in range(3)]
    stdout = _cli("buglab.controllers.bugselector", selector, tmp_path / "pool", outs[0], "--seed", "5", "--sequential")
    _cli("buglab.controllers.bugselector", selector, tmp_path / "pool", outs[1], "--seed", "5")
    _cli("buglab.controllers.bugselector", selector, tmp_path / "pool", outs[2], "--seed", "6", "--sequential")
    assert "Avg Entropy" in stdout and "NO_REWRITE" in stdout
    assert outs[0].read_bytes() == outs[1].read_bytes() != outs[2].read_bytes()
    selections = [s["selected_rewrites"] for s in load_msgpack_l_gz(outs[0], native=False)]
    assert len(selections) == 20 and all("NO_BUG" in s and 4 <= len(s) <= 5 for s in selections)

    # [external rewriting] -> records -> score: twice -> the same bytes
    records = make_scoring_records(data[100:], seed=1, selections=selections)
    (tmp_path / "records").mkdir()
    save_msgpack_l_gz_reproducibly(records, tmp_path / "records" / "r.msgpack.l.gz")
    scored = [tmp_path / "scored" / "s.msgpack.l.gz", tmp_path / "scored_again.msgpack.l.gz"]
    scored[0].parent.mkdir()
    assert "Scored 20 records" in _cli("buglab.controllers.detectorscoring", detector, tmp_path / "records", scored[0], "--sequential")
    _cli("buglab.controllers.detectorscoring", detector, tmp_path / "records", scored[1])
    assert scored[0].read_bytes() == scored[1].read_bytes()
    originals = list(load_msgpack_l_gz(scored[0], native=False))
    for original, selection in zip(originals, selections):
        lp = original["candidate_rewrite_logprobs"]
        n = len(original["candidate_rewrites"])
        assert len(lp) == n + 1
        assert {i for i, v in enumerate(lp) if math.isfinite(v)} == {n if k == "NO_BUG" else int(k) for k in selection}
        assert all(v <= 0 for v in lp)

    # one epoch of the selector on the scored originals: the generator-loss branch reports a loss and no repair loss
    with caplog.at_level("INFO"):
        train.run(train.parse_args(["gnn-mlp", str(tmp_path / "scored"), str(tmp_path / "scored"), str(selector), "--restore-path", str(selector),
                                    "--max-num-epochs", "1", "--minibatch-size", "10", "--quiet", "--sequential", "--selector"]))
    epochs = [r.getMessage() for r in caplog.records if "Train metrics" in r.getMessage()]
    assert epochs and "'Loss'" in epochs[-1] and "Repair Loss" not in epochs[-1], epochs
    loss = float(epochs[-1].split("'Loss':")[1].split("}")[0].split(",")[0])
    assert math.isfinite(loss)
