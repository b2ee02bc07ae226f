"""CPU: warning triage without a GPU -- the NumPy twin of csrc/bl_triage.hip (buglab/models/_triage.py) against torch fp64
autograd, the Newton driver's stop rule and monotone loss, the folds, the metrics against plain loops, what the re-ranker learns
and what it must not, the file, the command line's exit statuses and its order, and the C entry points' argument errors."""
import ctypes
import json
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

from tests import triage_cases as C


# ------------------------------------------------------------------------------------------------ 1. the twin against autograd
def _autograd(phi, y, c, w, l2, far=False):
    """L, g, H of the definition by torch fp64 autograd; softplus as logaddexp(0, z) (torch's own softplus switches to the
    identity above 20).  `far`: as relu(z) + log1p(exp(-|z|)) instead, whose second derivative autograd can form at |z| = 800,
    where logaddexp's double backward overflows -- but which has a kink at z == 0, so only there."""
    import torch

    t_phi, t_y, t_c = (torch.from_numpy(np.ascontiguousarray(a, np.float64)) for a in (phi, y, c))

    def loss(tw):
        z = t_phi @ tw
        soft = torch.relu(z) + torch.log1p(torch.exp(-z.abs())) if far else torch.logaddexp(torch.zeros_like(z), z)
        return (t_c * (soft - t_y * z)).sum() + 0.5 * l2 * (tw[:-1] ** 2).sum()

    tw = torch.from_numpy(np.ascontiguousarray(w, np.float64)).requires_grad_(True)
    L = loss(tw)
    (g,) = torch.autograd.grad(L, tw)
    H = torch.autograd.functional.hessian(loss, tw.detach())
    return float(L.detach()), g.numpy(), H.numpy()


@pytest.mark.parametrize("case", ["drawn", "zero_w", "weighted", "single_class", "far_margins", "non_finite"])
def test_twin_equals_autograd(case):
    from buglab.models import _triage as R

    N, D = 40, 10  # P = 12
    p = C.problem(N, D, seed=3)
    c = None
    if case == "zero_w":
        p["w"] = np.zeros(D + 2)
    elif case == "weighted":
        c = np.random.default_rng(4).uniform(0.0, 3.0, size=N)
        c[::7] = 0.0
    elif case == "single_class":
        p["y"] = np.zeros(N, np.uint8)
    elif case == "far_margins":
        z = R.margins_host(R.features_host(p["x"], p["logprob"], p["shift"], p["scale"])[0], p["w"])
        p["w"] = p["w"] * (800.0 / np.abs(z).max())
    elif case == "non_finite":
        p["x"][3, 2], p["logprob"][11] = np.nan, -np.inf
    st = R.newton_stats_host(p["x"], p["logprob"], p["shift"], p["scale"], p["w"], p["y"], c, C.L2)
    phi, ok = R.features_host(p["x"], p["logprob"], p["shift"], p["scale"])
    cc = np.where(ok, np.ones(N) if c is None else c, 0.0)
    L, g, H = _autograd(phi, p["y"], cc, p["w"], C.L2, far=case == "far_margins")
    assert (st.used, st.skipped) == (int(ok.sum()), N - int(ok.sum())) and st.csum == pytest.approx(cc.sum(), rel=1e-15)
    assert st.skipped == (2 if case == "non_finite" else 0)
    # autograd forms 1 - p by subtraction, an absolute error of a few 2^-53 per row whatever p is, so the tolerance is absolute per
    # row: 1e-13 (450 x 2^-53) of sum_n c_n |phi_ni| |phi_nj|.  A dropped row moves an entry by about 0.1 / N of that sum.
    a = np.abs(phi)
    assert np.isfinite(st.L) and np.isfinite(st.H).all() and np.isfinite(st.g).all()
    assert (np.abs(st.H - H) <= 1e-13 * (a.T @ (cc[:, None] * a)) + 1e-300).all()
    assert (np.abs(st.g - g) <= 1e-13 * (a.T @ cc) + 1e-13 * C.L2 * np.abs(p["w"])).all()
    z = phi @ p["w"]
    assert abs(st.L - L) <= 1e-13 * float((cc * (np.abs(z) + 1.0)).sum() + C.L2 * (p["w"] ** 2).sum())
    assert (st.H == st.H.T).all()
    if case == "far_margins":
        zz, prob = R.score_host(p["x"], p["logprob"], p["shift"], p["scale"], p["w"])
        assert np.abs(zz).max() == pytest.approx(800.0, rel=1e-12) and set(prob[np.abs(zz) > 750.0].tolist()) <= {0.0, 1.0}
        s, r, loss, _, _ = R.HostProblem(p["x"], p["logprob"], p["y"], p["shift"], p["scale"]).terms(p["w"], None)
        assert np.isfinite(loss).all() and (s >= 0.0).all() and (s[np.abs(zz) > 750.0] == 0.0).all() and np.isfinite(r).all()


def test_margins_are_the_lane_owned_dot_product():
    """`margins_host` against the definition written as plain loops: 64 lane sums, quads dealt round-robin, the xor butterfly"""
    from buglab.models import _triage as R

    rng = np.random.default_rng(0)
    for P in (3, 4, 6, 255, 256, 257, 514):
        phi, w = rng.normal(size=(2, P)), rng.normal(size=P)
        want = []
        for row in phi:
            lanes = [0.0] * 64
            for col in range(P):
                lanes[(col // 4) % 64] += w[col] * row[col]  # ascending columns: a lane's quads come in ascending order
            o = 32
            while o:
                lanes = [lanes[l] + lanes[l ^ o] for l in range(64)]
                o //= 2
            want.append(lanes[0])
        assert R.margins_host(phi, w).tolist() == want, P


def test_standardise_and_constant_columns():
    from buglab.models import _triage as R

    x, lp = C.drawn_rows(50, 6, seed=1)
    x[:, 2] = 4.5  # a constant column
    x[7, 0] = np.inf  # a row that takes no part
    shift, scale = R.standardise(x, lp)
    ok = np.arange(50) != 7
    cols = np.concatenate([x[ok].astype(np.float64), lp[ok].astype(np.float64)[:, None]], axis=1)
    assert shift.tolist() == cols.mean(axis=0).tolist() and scale[2] == 0.0 and shift.dtype == scale.dtype == np.float64
    phi, finite = R.features_host(x, lp, shift, scale)
    assert finite.tolist() == ok.tolist() and not phi[7].any() and (phi[ok, -1] == 1.0).all() and not phi[:, 2].any()
    assert np.allclose(phi[ok][:, [0, 1, 3, 4, 5, 6]].std(axis=0), 1.0) and np.allclose(phi[ok][:, :-1].mean(axis=0), 0.0, atol=1e-12)


# ------------------------------------------------------------------------------------------------ 2. the fit
@pytest.mark.parametrize("kind", ["separable", "noisy", "balanced"])
def test_fit_reaches_the_stop_rule_and_never_raises_the_loss(kind):
    from buglab.models import _triage as R

    x, lp, y = C.learnable(300, 8, seed=5, noise=0.0 if kind == "separable" else 1.0)
    if kind == "separable":
        assert 50 < y.sum() < 250
    shift, scale = R.standardise(x, lp)
    problem = R.HostProblem(x, lp, y, shift, scale)
    c = R.balance_weights(y) if kind == "balanced" else None
    fit = R.fit_logistic(lambda w, l2: problem.stats(w, c, l2), problem.P, 0.1)
    assert fit.converged and 2 <= fit.iterations < 50 and len(fit.losses) == fit.iterations + 1
    assert all(b <= a for a, b in zip(fit.losses, fit.losses[1:])) and fit.losses[-1] < fit.losses[0]
    # the gradient again, from the definition and without the twin's dot product
    cc = np.ones(300) if c is None else c
    z = problem.phi @ fit.w
    g = problem.phi.T @ (cc * (1.0 / (1.0 + np.exp(-z)) - y)) + 0.1 * np.concatenate([fit.w[:-1], [0.0]])
    assert np.abs(g).max() <= 1e-9 * max(1.0, cc.sum())
    # too few iterations: reported, not hidden
    short = R.fit_logistic(lambda w, l2: problem.stats(w, c, l2), problem.P, 0.1, max_iterations=1)
    assert not short.converged and short.iterations == 1
    with pytest.raises(ValueError):
        R.fit_logistic(lambda w, l2: problem.stats(w, c, l2), problem.P, 0.0)


# ------------------------------------------------------------------------------------------------ 3. the folds
def test_folds_are_stratified_and_a_function_of_the_seed():
    from buglab.models import _triage as R

    rng = np.random.default_rng(2)
    y = rng.uniform(size=103) < 0.3
    usable = np.ones(103, bool)
    usable[[4, 50]] = False
    fold = R.stratified_folds(y, 5, 11, usable)
    assert fold.dtype == np.int32 and (fold[~usable] == -1).all() and set(fold[usable].tolist()) == {0, 1, 2, 3, 4}
    for cls in (False, True):
        sizes = np.bincount(fold[usable & (y == cls)], minlength=5)
        assert sizes.max() - sizes.min() <= 1 and sizes.sum() == int((usable & (y == cls)).sum())
    assert fold.tolist() == R.stratified_folds(y, 5, 11, usable).tolist()
    assert fold.tolist() != R.stratified_folds(y, 5, 12, usable).tolist()
    # the order within a class is the splitmix64 key's, as `_compare` draws: row 0's key at seed 0, written out
    from buglab.models._compare import _GOLDEN, _U, _mix

    with np.errstate(over="ignore"):
        base = _mix(np.asarray(_U(11) * _GOLDEN + _GOLDEN))
        key = _mix(np.arange(103, dtype=np.uint64) + base)
    rows = np.flatnonzero(usable & y)
    assert fold[rows[np.lexsort((rows, key[rows]))]].tolist() == [i % 5 for i in range(rows.shape[0])]
    with pytest.raises(ValueError):
        R.stratified_folds(y, 1, 0)


# ------------------------------------------------------------------------------------------------ 4. the metrics
def test_auc_counts_pairs_with_ties_and_the_ridge_choice():
    from buglab.models import _triage as R

    rng = np.random.default_rng(3)
    score = np.round(rng.normal(size=60) * 2.0) / 2.0  # many ties
    y = rng.uniform(size=60) < 0.4
    pairs = sum(1.0 if a > b else (0.5 if a == b else 0.0) for a in score[y] for b in score[~y])
    assert R.auc(score, y) == pytest.approx(pairs / (y.sum() * (~y).sum()), rel=1e-14)
    assert R.auc(np.array([3.0, 2.0, 1.0, 0.0]), np.array([1, 1, 0, 0])) == 1.0 and R.auc(np.zeros(6), np.array([1, 0, 1, 0, 0, 0])) == 0.5
    assert np.isnan(R.auc(score, np.ones(60, bool)))
    assert R.auc(np.array([2.0, np.nan, 1.0]), np.array([1, 0, 0])) == 1.0  # a row without a score is left out
    assert R.precision_at(np.array([5.0, 4.0, 3.0, 2.0, 1.0, 0.0, -1.0, -2.0, -3.0, -4.0]), np.array([1, 0, 1, 1, 0, 0, 0, 0, 0, 0]), 0.25) \
        == pytest.approx(2.0 / 3.0)
    assert R.precision_at(np.arange(10.0), np.arange(10) == 9, 0.10) == 1.0
    # the lowest loss; a tie goes to the larger l2; a loss that is not finite never wins
    assert R.choose_l2([(0.01, 0.5), (0.1, 0.3), (1.0, 0.4)]) == 0.1
    assert R.choose_l2([(0.01, 0.3), (0.1, 0.3), (1.0, 0.4)]) == 0.1
    assert R.choose_l2([(10.0, 0.3), (0.1, 0.3), (1.0, 0.3)]) == 10.0
    assert R.choose_l2([(0.01, float("nan")), (0.1, 0.9)]) == 0.1
    with pytest.raises(ValueError):
        R.choose_l2([(1.0, float("nan"))])
    assert len(R.DEFAULT_L2_GRID) == 11 and R.DEFAULT_L2_GRID[0] == 0.01 and R.DEFAULT_L2_GRID[-1] == 1000.0
    assert R.DEFAULT_L2_GRID[1] == pytest.approx(10.0 ** -1.5)
    assert R.log_loss(np.array([0.0, 800.0, -800.0]), np.array([1, 1, 0])) == pytest.approx(np.log(2.0) / 3.0)


def test_rank_order_is_the_three_key_rule():
    from buglab.models import _triage as R

    prob = np.array([0.2, 0.9, np.nan, 0.9, 0.9, 0.2, np.nan])
    logprob = np.array([-1.0, -2.0, -0.1, -1.0, -1.0, -1.0, -0.5])
    position = np.array([10, 11, 12, 14, 13, 9, 15])
    assert R.rank_order(prob, logprob, position).tolist() == [4, 3, 1, 5, 0, 2, 6]
    assert R.probability_histogram(np.array([0.0, 0.05, 0.1, 0.55, 0.999, 1.0, np.nan])) == [2, 1, 0, 0, 0, 1, 0, 0, 0, 2]


# ------------------------------------------------------------------------------------------------ 5. what it learns
def test_it_learns_a_direction_and_nothing_from_noise():
    """Seen on the CPU before these values were fixed (N = 600, D = 16, 5 folds, the default grid).  Learnable rows at noise 1.0:
    out-of-fold AUC 0.836 / 0.808 / 0.807 for the seeds 21 / 23 / 24, short of 0.9, which is why the noise here is 0.5: AUC
    0.940 / 0.930 / 0.922 (seed 21 is used: 0.940, precision in the top 10 % 1.0, l2 = 1) against 0.472 / 0.518 / 0.486 for the
    log-probability alone.  Labels independent of the rows: 0.539 / 0.533 / 0.495 for the seeds 22 / 25 / 26 (seed 22 is used),
    with l2 = 316 or 1000 chosen."""
    from buglab.models import triage as T

    x, lp, y = C.learnable(600, 16, seed=21, noise=0.5)
    fit = T.fit_triage_embeddings(x, lp, y, host=True)
    r = fit.report
    assert fit.model.converged and r["all_folds_converged"] and r["folds"] == 5 and len(r["cv"]) == 11
    assert r["triage"]["auc"] >= 0.9 and r["triage"]["auc"] > r["baseline_logprob"]["auc"] and r["beats_baseline"]
    assert r["triage"]["precision_at_10"] > r["baseline_logprob"]["precision_at_10"]
    x, lp, y = C.unlearnable(600, 16, seed=22)
    r = T.fit_triage_embeddings(x, lp, y, host=True).report
    assert 0.4 <= r["triage"]["auc"] <= 0.6
    assert r["l2"] >= 100.0  # nothing to learn: the strongest ridges win


# ------------------------------------------------------------------------------------------------ 6. the file and the command line
def _fitted(D=5, **changes):
    from buglab.models._triage import TriageModel

    rng = np.random.default_rng(8)
    m = TriageModel(rng.normal(size=D + 2), rng.normal(size=D + 1), rng.uniform(0.5, 2.0, size=D + 1), 0.1, D, "predicted", "GnnBugLabModel",
                    "ab" * 20, 40, 35, np.array([0.1, 1.0]), np.array([0.41, 0.43]), True)
    return m._replace(**changes)


def test_the_file_round_trips_without_pickled_code(tmp_path):
    from buglab.models._triage import DimensionMismatch, TriageModel

    m = _fitted()
    m.save(tmp_path / "t.npz")
    back = TriageModel.load(tmp_path / "t.npz")
    for a, b in zip(m, back):
        assert (a.tobytes() == b.tobytes() and a.dtype == b.dtype) if isinstance(a, np.ndarray) else (a == b and type(a) is type(b))
    with np.load(tmp_path / "t.npz", allow_pickle=False) as z:  # every array loads with pickling refused
        assert {"w", "shift", "scale", "l2", "dim", "site", "model_class", "fingerprint", "cv_l2", "cv_log_loss", "converged"} <= set(z.files)
    assert back.check_model("GnnBugLabModel", 5, "ab" * 20) is None and "other weights" in back.check_model("GnnBugLabModel", 5, "cd" * 20)
    with pytest.raises(DimensionMismatch, match="size 5"):
        back.check_model("GnnBugLabModel", 32, "ab" * 20)
    _fitted(w=np.zeros(3)).save(tmp_path / "bad.npz")
    with pytest.raises(ValueError, match="inconsistent"):
        TriageModel.load(tmp_path / "bad.npz")


@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory):
    """an untrained gnn-mlp (hidden size 32) saved as a checkpoint, and the synthetic data it was set up with"""
    import torch

    from buglab.data.synthetic import make_report_dataset
    from tests.test_visualize_host import _model

    data = make_report_dataset(120, seed=35)
    model = _model("gnn-mlp", data)
    torch.manual_seed(1)
    path = tmp_path_factory.mktemp("triage_host") / "detector.pkl.gz"
    model.save(path, model.build_neural_module())
    return path, data


def test_rank_with_a_file_of_another_size_is_exit_status_2_before_any_data_is_read(checkpoint, tmp_path, capsys):
    from buglab.models import triage as T

    path, _ = checkpoint
    _fitted(D=5).save(tmp_path / "other.npz")
    # the data path does not exist and no GPU is asked for: the check comes first
    status = T.run(T.parse_args(["rank", str(path), str(tmp_path / "other.npz"), str(tmp_path / "nowhere"), str(tmp_path / "out.jsonl")]))
    assert status == T.EXIT_DIMENSION_MISMATCH == 2 and "size 5" in capsys.readouterr().err and not (tmp_path / "out.jsonl").exists()


class _DrawnSites:
    """The embedding step replaced by drawn values: this file runs without a GPU and the models have no CPU forward
    (tests/test_triage_gpu.py runs the real one).  A sample's embedding, place 0 and log-probability depend on its path alone;
    everything after the embedding step -- metadata, fit, scores, order, records -- is the real code."""

    D = 32

    @staticmethod
    def of(point):
        rng = np.random.default_rng(zlib.crc32(point["graph"]["path"].encode()))
        return rng.normal(size=_DrawnSites.D).astype(np.float32), np.float32(np.log(rng.uniform(0.05, 1.0)))

    @classmethod
    def collect(cls, model, nn, data, device, site, assume_buggy, host, parallelize):
        from buglab.models.similar import _Sites

        points = list(data)
        drawn = [cls.of(p) for p in points]
        rows = np.stack([d[0] for d in drawn]) if drawn else None
        return _Sites(list(range(len(points))), points, rows, np.zeros(len(points), np.int32), np.asarray([d[1] for d in drawn], np.float32),
                      len(points), 0)

    @classmethod
    def embed(cls, model, nn, data, device, site, **options):
        from buglab.models import similar

        found = cls.collect(model, nn, data, device, site, False, True, False)
        return similar._with_metadata(found, *similar._copy_back(found, cls.D), site)


def test_command_line_fit_then_rank_on_the_host(checkpoint, tmp_path, monkeypatch, capsys):
    from buglab.models import triage as T
    from buglab.models._triage import TriageModel

    path, data = checkpoint
    verdicts, scan = data[:80], data[80:] + [data[85]]  # one sample twice: equal probabilities and log-probabilities
    accepted = [p for p in verdicts if _DrawnSites.of(p)[0][0] > 0.0]
    dismissed = [p for p in verdicts if not _DrawnSites.of(p)[0][0] > 0.0]
    assert len(accepted) >= 20 and len(dismissed) >= 20
    sets = {"yes": accepted, "no": dismissed, "few": accepted[:6], "scan": scan}
    real_open = T._open_model
    monkeypatch.setattr(T, "_open_model", lambda p: real_open(p)[:3] + (True,))  # the untrained model itself; the GPU is not asked for
    monkeypatch.setattr(T, "_read_data", lambda p, limit: sets[p][:limit])
    monkeypatch.setattr(T, "_embed_sites", _DrawnSites.embed)
    monkeypatch.setattr(T, "_collect_sites", _DrawnSites.collect)

    out = tmp_path / "triage.npz"
    assert T.run(T.parse_args(["fit", str(path), str(out), "--accepted", "few", "--dismissed", "no", "--host"])) == T.EXIT_TOO_FEW_VERDICTS == 2
    assert "6 accepted" in capsys.readouterr().err and not out.exists()
    report = tmp_path / "fit.json"
    status = T.run(T.parse_args(["fit", str(path), str(out), "--accepted", "yes", "--dismissed", "no", "--host", "--sequential", "--seed", "3",
                                 "--report-json", str(report)]))
    assert status == 0 and "triage fit:" in capsys.readouterr().out
    fitted = TriageModel.load(out)
    r = json.loads(report.read_text())
    assert (fitted.dim, fitted.num_accepted, fitted.num_dismissed) == (32, len(accepted), len(dismissed)) and fitted.converged
    assert fitted.model_class == "GnnBugLabModel" and len(fitted.fingerprint) == 40 and fitted.l2 in fitted.cv_l2 and fitted.site == "predicted"
    assert r["path"] == "host" and r["converged"] and r["triage"]["auc"] > 0.8 > r["baseline_logprob"]["auc"] and r["accepted"]["num_samples"] == len(accepted)

    listed = tmp_path / "ranked.jsonl"
    summary = tmp_path / "rank.json"
    assert T.run(T.parse_args(["rank", str(path), str(out), "scan", str(listed), "--host", "--report-json", str(summary)])) == 0
    records = [json.loads(line) for line in listed.read_text().splitlines()]
    assert len(records) == 41 and set(records[0]) == {"position", "node", "label", "filename", "package", "logprob", "triage_probability"}
    keys = [(-r["triage_probability"], -r["logprob"], r["position"]) for r in records]
    assert keys == sorted(keys) and sorted(r["position"] for r in records) == list(range(41))
    twice = [r for r in records if r["position"] in (5, 40)]  # equal on both keys: the position decides
    assert [r["position"] for r in twice] == [5, 40] and twice[0]["triage_probability"] == twice[1]["triage_probability"]
    # the order means something: the sites the stub would have accepted come first
    first = [_DrawnSites.of(scan[r["position"]])[0][0] > 0.0 for r in records[:10]]
    assert sum(first) >= 8
    s = json.loads(summary.read_text())
    assert s["num_warnings"] == s["num_listed"] == 41 and sum(s["probability_histogram"]) == 41 and 0.0 < s["share_above_half"] < 1.0
    assert T.run(T.parse_args(["rank", str(path), str(out), "scan", str(listed), "--host", "--top-k", "7", "--min-triage-probability", "0.5"])) == 0
    top = [json.loads(line) for line in listed.read_text().splitlines()]
    assert top == records[:7] and all(r["triage_probability"] >= 0.5 for r in top)


def test_refusals_and_arguments():
    from buglab.models import triage as T
    from buglab.models.ensemble.wrapper import EnsembleWrapper
    from buglab.models.greatreimplementation import GreatVarMisuse

    ensemble = EnsembleWrapper.__new__(EnsembleWrapper)
    great = GreatVarMisuse({"num_layers": 2, "num_heads": 4, "intermediate_dimension": 96, "dropout_rate": 0.0}, vocab_size=64, embedding_dim=64)
    for model, word in ((ensemble, "ensembles"), (great, "GreatVarMisuse")):
        with pytest.raises(TypeError, match=word):
            T.fit_triage(model, None, [], [], "cpu")
        with pytest.raises(TypeError, match=word):
            T.rank_warnings(model, None, _fitted(), [], "cpu")
    a = T.parse_args(["fit", "m", "o", "--accepted", "a", "b", "--dismissed", "d"])
    assert (a.accepted, a.dismissed, a.folds, a.seed, a.l2, a.l2_grid, a.balance, a.min_per_class, a.max_iterations, a.site, a.host) \
        == (["a", "b"], ["d"], 5, 0, None, None, False, 10, 50, "predicted", False)
    assert T.parse_args(["fit", "m", "o", "--accepted", "a", "--dismissed", "d", "--l2-grid", "0.1,1,10"]).l2_grid == [0.1, 1.0, 10.0]
    for bad in (["--l2", "0"], ["--l2", "1", "--l2-grid", "1,2"], ["--folds", "1"], ["--l2-grid", "1,-2"]):
        with pytest.raises(SystemExit):
            T.parse_args(["fit", "m", "o", "--accepted", "a", "--dismissed", "d"] + bad)
    b = T.parse_args(["rank", "m", "t", "d", "o", "--min-confidence", "0.2", "--top-k", "9"])
    assert (b.min_confidence, b.min_triage_probability, b.top_k, b.site) == (0.2, None, 9, "predicted")
    assert "BEYOND THE REFERENCE" in T.__doc__
    x, lp, y = C.learnable(40, 4, seed=1)
    with pytest.raises(T.TooFewVerdicts, match="at least 30"):
        T.fit_triage_embeddings(x, lp, y, host=True, min_per_class=30)
    with pytest.raises(ValueError, match="not both"):
        T.fit_triage_embeddings(x, lp, y, host=True, l2=1.0, l2_grid=[1.0])
    with pytest.raises(ValueError):
        T.fit_triage_embeddings(np.zeros((4, 513), np.float32), lp[:4], y[:4], host=True)
    one = T.fit_triage_embeddings(x, lp, y, host=True, l2=2.0, min_per_class=5)  # a fixed ridge: no cross-validation
    assert one.model.l2 == 2.0 and one.model.cv_l2.shape == (0,) and "triage" not in one.report and one.report["folds"] == 0


# ------------------------------------------------------------------------------------------------ 7. the ABI
def test_entry_points_check_before_any_hip_call():
    """host-side argument checks of the hip_ops wrappers (plain ValueErrors, no GPU needed) and of the C entry points: a bad call
    never reaches a kernel"""
    import torch

    from buglab.models import _triage as R
    from buglab.models import hip_ops
    from tests.conftest import PKG, ROOT

    header = open(os.path.join(ROOT, "include", "buglab_hip.h")).read()
    assert "#define BL_TRIAGE_MAX_D 512" in header and hip_ops.TRIAGE_MAX_D == R.MAX_D == hip_ops.SIM_MAX_D == 512
    assert "#define BL_TRIAGE_MAX_SLICES 64" in header and hip_ops.TRIAGE_MAX_SLICES == R.MAX_SLICES == 64
    assert re.search(r"Warning triage.*BEYOND THE REFERENCE", header)
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, "buglab", "models", "hip_ops", "libbuglab_hip.so")],
                        capture_output=True, text=True, check=True).stdout
    for name in ("bl_triage_workspace_bytes", "bl_triage_newton_stats", "bl_triage_score"):
        assert f" T {name}" in nm and name in hip_ops.EXPORTED_SYMBOLS

    f32, f64 = (lambda *s: torch.zeros(*s)), (lambda *s: torch.zeros(*s, dtype=torch.float64))
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)
    with pytest.raises(ValueError, match=r"D <= 512"):
        hip_ops.triage_newton_stats(f32(2, 513), f32(2), f64(514), f64(514), f64(515), u8(2), None, 1.0)
    with pytest.raises(ValueError, match="logprob"):
        hip_ops.triage_newton_stats(f32(2, 8), f32(3), f64(9), f64(9), f64(10), u8(2), None, 1.0)
    with pytest.raises(ValueError, match="shift"):
        hip_ops.triage_score(f32(2, 8), f32(2), f64(8), f64(9), f64(10))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="l2"):
            hip_ops.triage_newton_stats(f32(2, 8), f32(2), f64(9), f64(9), f64(10), u8(2), None, bad)
    with pytest.raises(ValueError, match=r"c must be"):
        hip_ops.triage_newton_stats(f32(2, 8), f32(2), f64(9), f64(9), f64(10), u8(2), f64(3), 1.0)
    with pytest.raises((hip_ops.HipOpsUnavailable, ValueError), match="GPU"):  # a well-formed call gets as far as the device check
        hip_ops.triage_newton_stats(f32(2, 8), f32(2), f64(9), f64(9), f64(10), u8(2), None, 1.0)
    with pytest.raises((hip_ops.HipOpsUnavailable, ValueError), match="GPU"):
        hip_ops.triage_score(f32(2, 8), f32(2), f64(9), f64(9), f64(10))
    with pytest.raises(ValueError):
        hip_ops.triage_workspace_bytes(4, 513)
    # the slice rule and the workspace, restated: s and r per row, 4 scalars per 64 rows, per slice a padded g and the tiles of H
    assert [hip_ops.triage_slices(n) for n in (0, 1, 128, 129, 130, 513, 1000, 4099, 8192, 8193, 100000)] \
        == [(1, 0), (1, 4), (1, 128), (2, 68), (2, 68), (5, 104), (8, 128), (33, 128), (64, 128), (64, 132), (64, 1564)]
    for N, D in ((1, 4), (130, 62), (4099, 126), (513, 512), (100000, 512)):
        S, tiles = hip_ops.triage_slices(N)[0], (D + 2 + 15) // 16
        want = 8 * (2 * N + 4 * ((N + 63) // 64) + S * 16 * tiles + S * (tiles * (tiles + 1) // 2) * 256)
        assert hip_ops.triage_workspace_bytes(N, D) == want and R.slices(N) == hip_ops.triage_slices(N)

    lib = hip_ops.load_library()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 4)  # 4-byte aligned and no more
    odd1 = ctypes.c_void_p(p.value + 2)
    assert lib.bl_triage_workspace_bytes(-1, 8) == -1 and lib.bl_triage_workspace_bytes(4, 513) == -1 and lib.bl_triage_workspace_bytes(4, 0) == -1
    need = lib.bl_triage_workspace_bytes(4, 8)
    big = 1 << 30
    stats = lambda x=p, ldx=8, lp=p, sh=p, sc=p, w=p, y=p, c=None, N=4, D=8, lam=1.0, ws=p, wsb=big, H=p, g=p, s=p: \
        lib.bl_triage_newton_stats(x, ldx, lp, sh, sc, w, y, c, N, D, lam, ws, wsb, H, g, s, None)
    err = lib.bl_last_error
    assert stats(N=-1) == -1 and b"N >= 0" in err()
    assert stats(D=0) == -1 and b"D >= 1" in err()
    assert stats(D=513, ldx=513) == -2 and b"BL_TRIAGE_MAX_D" in err()
    assert stats(ldx=7) == -1 and b"row stride" in err()
    for null in ("x", "lp", "sh", "sc", "w", "y", "ws", "H", "g", "s"):
        assert stats(**{null: None}) == -1 and b"null" in err(), null
    for name in ("sh", "sc", "w", "c", "H", "g", "s", "ws"):
        assert stats(**{name: odd}) == -1 and b"aligned" in err(), name
    for name in ("x", "lp"):
        assert stats(**{name: odd1}) == -1 and b"4-byte aligned" in err(), name
    for lam in (0.0, -2.0, float("nan"), float("inf")):
        assert stats(lam=lam) == -1 and b"lambda" in err(), lam
    assert stats(wsb=need - 1) == -1 and str(need).encode() in err() and b"workspace" in err()
    assert stats(N=0, x=None, lp=None, y=None, ws=None, wsb=0, H=None, g=None, s=None) == 0  # nothing to launch

    score = lambda x=p, ldx=8, lp=p, sh=p, sc=p, w=p, N=4, D=8, m=p, pr=p: lib.bl_triage_score(x, ldx, lp, sh, sc, w, N, D, m, pr, None)
    assert score(N=-1) == -1 and b"N >= 0" in err()
    assert score(D=513, ldx=513) == -2 and b"BL_TRIAGE_MAX_D" in err()
    assert score(ldx=7) == -1 and b"row stride" in err()
    for null in ("x", "lp", "sh", "sc", "w", "m", "pr"):
        assert score(**{null: None}) == -1 and b"null" in err(), null
    for name in ("sh", "w", "m", "pr"):
        assert score(**{name: odd}) == -1 and b"aligned" in err(), name
    assert score(N=0) == 0 and score(N=0, x=None, lp=None, m=None, pr=None) == 0
