"""CPU: fitted ensembles (the `weighted` kind; buglab/models/ensemble/_weights.py, fit.py) -- the NumPy twin's gradients against
central finite differences, its combination against the `avg` fold at the identity parameters, the projected BFGS fit and its
degenerate cases, the three C entry points' argument errors, and what `EnsembleWrapper` and the command line accept."""
import copy
import ctypes
import pickle
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import ensemble_ref as R
from tests import ensemble_weights_fixtures as X

THETA, BETA, PHI = (0.3, 0.7, -1.1), (0.8, 1.3, 2.0), (-0.2, 0.5, 1.5)
# central differences of a smooth fp64 function: truncation h^2 f''' / 6 ~ 1e-10 and rounding eps |F| / h ~ 1e-9 at h = 1e-5.
# Every component is measured on its own scale, the sum of the absolute values of the terms it is added up from (the twin's
# second return value), so that a wrong small component cannot hide under a large one.
FD_STEP, FD_BOUND = 1e-5, 1e-6


def _central(f, x):
    g = np.zeros(x.shape[0])
    for k in range(x.shape[0]):
        e = np.zeros(x.shape[0])
        e[k] = FD_STEP
        g[k] = (f(x + e) - f(x - e)) / (2 * FD_STEP)
    return g


def test_twin_gradients_match_central_differences():
    from buglab.models.ensemble import _weights as W

    loc, rw = X.edge_pools()
    lengths = np.diff(loc.off)
    assert loc.vals.shape[0] == 3 and 1 in lengths and 65 in lengths and (loc.present == 0).any()
    assert np.isneginf(loc.vals[loc.present[:, 1] != 0][:, loc.off[1]:loc.off[2]]).any()
    M = 3
    x = np.array(THETA + BETA)
    got, scale = W.loc_stats(loc, x[:M], x[M:])
    fd = _central(lambda v: W.loc_stats(loc, v[:M], v[M:])[0][0], x)
    assert np.isfinite(got).all() and (scale[1:] > 0).all()
    err = np.abs(got[1:] - fd) / scale[1:]
    print(f"[ensemble weights] location gradient {got[1:]} finite differences {fd} error per component, on its own scale {err}")
    assert (err < FD_BOUND).all()
    assert abs(got[1:1 + M].sum()) < 1e-12 * M * loc.tgt.shape[0]  # only differences of weights matter
    got, scale = W.rw_stats(rw, PHI)
    fd = _central(lambda v: W.rw_stats(rw, v)[0][0], np.array(PHI))
    err = np.abs(got[1:] - fd) / scale[1:]
    print(f"[ensemble weights] rewrite gradient {got[1:]} finite differences {fd} error per component, on its own scale {err}")
    assert np.isfinite(got).all() and (err < FD_BOUND).all()


@pytest.mark.parametrize("beta", [BETA, (1.0, 1.3, 1.0), (1.0, 1.0, 1.0)], ids=["scaled", "mixed", "as they are"])
def test_the_fitted_objective_is_the_predicted_values(beta):
    """The loss the fit minimises (`loc_stats` / `rw_stats`: first maximum, log1p) and the values `predict` emits
    (`combine_weighted`: the logaddexp fold) are two statements of one model: F = -sum of the combined value at every target, also
    under the rule that a beta of exactly 1 leaves a member's values as they are.  The two differ in the rounding of a few fp64
    operations per sample."""
    from buglab.models.ensemble import _weights as W

    loc, rw = X.edge_pools()
    M, total = loc.vals.shape
    S = loc.tgt.shape[0]
    buggy = np.flatnonzero(loc.tgt != np.diff(loc.off) - 1)  # the samples the rewrite pool was made for, in its order
    assert rw.vals.shape == (M, buggy.shape[0]) and (rw.present == loc.present[:, buggy]).all()
    here = np.repeat(loc.present != 0, np.diff(loc.off), axis=1)
    loc_idx = np.where(here, np.arange(M * total).reshape(M, total), -1).astype(np.int32)
    rw_idx = np.where(rw.present != 0, M * total + np.arange(rw.vals.size).reshape(rw.vals.shape), -1).astype(np.int32)
    rw_off = np.concatenate([[0], np.cumsum(np.isin(np.arange(S), buggy))]).astype(np.int32)  # a buggy sample's one rewrite: the truth
    src = np.concatenate([loc.vals.reshape(-1), rw.vals.reshape(-1)])
    out_loc, out_rw = W.combine_weighted(src, loc_idx, loc.off, rw_idx, rw_off, THETA, beta, PHI)
    F_loc, F_rw = W.loc_stats(loc, THETA, beta)[0][0], W.rw_stats(rw, PHI)[0][0]
    want_loc, want_rw = -out_loc[loc.off[:-1] + loc.tgt].sum(), -out_rw.sum()
    print(f"[ensemble weights] F_loc {F_loc:.17g} from the combined values {want_loc:.17g}; F_rw {F_rw:.17g} / {want_rw:.17g}")
    assert np.isfinite([F_loc, F_rw]).all()
    assert abs(F_loc - want_loc) <= 1e-12 * max(1.0, abs(F_loc)) and abs(F_rw - want_rw) <= 1e-12 * max(1.0, abs(F_rw))


def test_identity_parameters_combine_as_avg_and_any_parameters_normalise():
    from buglab.models.ensemble import _weights as W

    samples = X.wide_samples(with_unpredicted=True)
    gather = X.gather_arrays(samples)
    ident = W.EnsembleWeights.identity(3)
    assert ident.is_identity
    out_loc, out_rw = W.combine_weighted(*gather, ident.theta, ident.beta, ident.phi)
    loc_off, rw_off = gather[2], gather[4]
    for b, s in enumerate(samples):
        g_loc, g_rw = out_loc[loc_off[b]:loc_off[b + 1]], out_rw[rw_off[b]:rw_off[b + 1]]
        preds = [None if mem is None else (dict(enumerate(mem[0].astype(np.float64).tolist())), mem[1].astype(np.float64).tolist())
                 for mem in s["members"]]
        want = R.combine("avg", preds)
        if want is None:
            assert np.isnan(g_loc).all() and np.isnan(g_rw).all() and g_loc.shape[0] == 7
            continue
        for got, ref in ((g_loc, np.array(list(want[0].values()))), (g_rw, np.array(want[1]))):
            assert (np.isnan(got) == np.isnan(ref)).all() and (np.isneginf(got) == np.isneginf(ref)).all()
            fin = np.isfinite(ref)
            assert (np.abs(got[fin] - ref[fin]) <= 1e-12 * np.maximum(1.0, np.abs(ref[fin]))).all(), b
    # every member rescaled (no beta is 1): each location segment is a distribution again.  The NaN entry is left out: a NaN
    # stays a NaN, as in `avg`
    clean = X.wide_samples()
    clean[2]["members"][1][0][5] = -4.0
    gather = X.gather_arrays(clean)
    out_loc, _ = W.combine_weighted(*gather, THETA, BETA, PHI)
    for b in range(len(clean)):
        total = np.exp(out_loc[gather[2][b]:gather[2][b + 1]]).sum()
        assert abs(total - 1.0) <= 1e-12, (b, total)


@pytest.mark.parametrize("fit_temperature", [True, False])
def test_fit_never_raises_the_loss_and_ends_at_a_stationary_point_or_on_the_box(fit_temperature):
    from buglab.models import _calibrate as K
    from buglab.models.ensemble import _weights as W

    loc, rw = X.fit_pools()
    M, S, Sb = 3, loc.tgt.shape[0], rw.vals.shape[1]
    weights, details = W.fit_host(loc, rw, fit_temperature=fit_temperature)
    ident = W.EnsembleWeights.identity(M)
    start = (W.loc_stats(loc, ident.theta, ident.beta)[0][0], W.rw_stats(rw, ident.phi)[0][0])
    end_loc, end_rw = W.loc_stats(loc, weights.theta, weights.beta)[0], W.rw_stats(rw, weights.phi)[0]
    print(f"[ensemble weights] fit {weights} start {start} end {end_loc[0]}, {end_rw[0]}")
    assert end_loc[0] <= start[0] and end_rw[0] <= start[1]
    assert end_loc[0] < start[0] - 1.0 and end_rw[0] < start[1] - 1.0  # and on this data by far
    assert weights.fitted_on == (S, Sb)
    assert weights.nll_before == (start[0] / S, start[1] / Sb) and weights.nll_after == (end_loc[0] / S, end_rw[0] / Sb)
    assert weights.theta[0] == 0.0 and weights.phi[0] == 0.0
    if not fit_temperature:
        assert weights.beta == (1.0, 1.0, 1.0)
    for x, lo, hi in zip(weights.theta + weights.beta + weights.phi, [W.WEIGHT_BOX[0]] * M + [K.BETA_BOX[0]] * M + [W.WEIGHT_BOX[0]] * M,
                         [W.WEIGHT_BOX[1]] * M + [K.BETA_BOX[1]] * M + [W.WEIGHT_BOX[1]] * M):
        assert lo <= x <= hi
    for head, grad, x, boxes, n, fixed in (
            ("localization", end_loc[1:], np.array(weights.theta + weights.beta), [W.WEIGHT_BOX] * M + [K.BETA_BOX] * M, S,
             [0] + ([] if fit_temperature else [M, M + 1, M + 2])),
            ("rewrite", end_rw[1:], np.array(weights.phi), [W.WEIGHT_BOX] * M, Sb, [0])):
        d = details[head]
        on_box = [k for k in range(x.shape[0]) if k not in fixed and x[k] in boxes[k]]
        assert on_box == list(d["on_box"])
        free = [k for k in range(x.shape[0]) if k not in fixed and k not in on_box]
        norm = np.abs(grad[free]).max() if free else 0.0
        print(f"[ensemble weights] {head}: iterations {d['iterations']} evaluations {d['evaluations']} free gradient {norm:.3e} "
              f"tolerance {K.GRADIENT_TOLERANCE * n:.3e} on the box {on_box}")
        assert norm <= K.GRADIENT_TOLERANCE * n or on_box
        assert d["converged"] and d["iterations"] <= K.MAX_ITERATIONS


def test_degenerate_data_keeps_the_identity_parameters_and_says_so():
    from buglab.models.ensemble import _weights as W

    loc, rw = X.fit_pools(absent_member=2)
    weights, _ = W.fit_host(loc, rw)
    assert (weights.theta[2], weights.beta[2], weights.phi[2]) == (0.0, 1.0, 0.0)
    assert weights.theta[1] != 0.0 and weights.beta[1] != 1.0 and weights.phi[1] != 0.0
    assert W.note_member_absent(2, "fitting") in weights.notes
    loc, rw = X.fit_pools(buggy=False)
    assert rw.vals.shape == (3, 0)
    weights, details = W.fit_host(loc, rw)
    assert weights.phi == (0.0, 0.0, 0.0) and W.NOTE_NO_BUGGY in weights.notes and weights.fitted_on == (48, 0)
    assert details["rewrite"]["evaluations"] == 0 and np.isnan(weights.nll_after[1])
    assert weights.nll_after[0] <= weights.nll_before[0]


def test_optimiser_holds_a_parameter_on_its_box():
    """A weight that wants to leave the box stops on it (a finite value), and the others are still fitted."""
    from buglab.models.ensemble import _weights as W

    target = np.array([0.5, 40.0, -3.0])  # a quadratic bowl whose minimum lies outside the box in x[1]
    stats = lambda x: (float(((x - target) ** 2).sum()), 2.0 * (x - target))
    fit = W.bfgs_fit(stats, 1, [0.0, 0.0, 0.0], [(0.5, 0.5), W.WEIGHT_BOX, W.WEIGHT_BOX])
    assert fit.x[0] == 0.5 and fit.x[1] == 20.0 and fit.x[2] == pytest.approx(-3.0, abs=1e-8)
    assert fit.converged and fit.on_box == (1,) and fit.loss <= fit.start_loss


def test_launchers_report_argument_errors_without_touching_the_gpu():
    """The three entry points validate everything before their first HIP call: BL_EINVAL (-1) / BL_ERANGE (-2) and a message."""
    from buglab.models import hip_ops

    lib = hip_ops.load_library()
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    dbl = lambda *v: (ctypes.c_double * len(v))(*v)
    zeros, ones = dbl(0, 0), dbl(1, 1)
    nan, inf = float("nan"), float("inf")

    def loc(M=2, S=1, total=8, vals=p, present=p, seg_off=p, tgt=p, theta=zeros, beta=ones, partials=p, out=p):
        return lib.bl_ens_loc_stats(vals, total, present, seg_off, tgt, M, S, theta, beta, partials, out, None)

    def rw(M=2, S=1, vals=p, present=p, phi=zeros, partials=p, out=p):
        return lib.bl_ens_rw_stats(vals, present, M, S, phi, partials, out, None)

    def combine(M=2, B=1, n_src=16, total_loc=4, total_rw=4, src=p, loc_idx=p, loc_off=p, rw_idx=p, rw_off=p, theta=zeros, beta=ones,
                phi=zeros, out_loc=p, out_rw=p):
        return lib.bl_ensemble_combine_weighted(src, n_src, loc_idx, loc_off, total_loc, rw_idx, rw_off, total_rw, M, B, theta, beta,
                                                phi, out_loc, out_rw, None)

    for call, kwargs, rc, text in (
        (loc, {"M": 0}, -1, b"at least 1"),
        (loc, {"M": 17}, -2, b"at most 16"),
        (loc, {"S": -1}, -1, b"negative size"),
        (loc, {"total": -5}, -1, b"negative size"),
        (loc, {"M": 4, "total": 1 << 30, "theta": dbl(0, 0, 0, 0), "beta": dbl(1, 1, 1, 1)}, -2, b"int32"),
        (loc, {"theta": None}, -1, b"null theta"),
        (loc, {"beta": None}, -1, b"null beta"),
        (loc, {"theta": dbl(0, nan)}, -1, b"theta must be finite"),
        (loc, {"theta": dbl(0, 20.5)}, -1, b"box"),
        (loc, {"beta": dbl(1, 0.0)}, -1, b"beta must be finite"),
        (loc, {"beta": dbl(inf, 1)}, -1, b"box"),
        (loc, {"vals": None}, -1, b"null vals"),
        (loc, {"present": None}, -1, b"null"),
        (loc, {"tgt": None}, -1, b"null"),
        (loc, {"out": None}, -1, b"null"),
        (rw, {"M": 0}, -1, b"at least 1"),
        (rw, {"M": 17}, -2, b"at most 16"),
        (rw, {"S": -2}, -1, b"negative size"),
        (rw, {"S": (1 << 31) - 8}, -2, b"int32"),
        (rw, {"phi": None}, -1, b"null phi"),
        (rw, {"phi": dbl(0, -inf)}, -1, b"phi must be finite"),
        (rw, {"phi": dbl(-21.0, 0)}, -1, b"box"),
        (rw, {"vals": None}, -1, b"null"),
        (rw, {"partials": None}, -1, b"null"),
        (combine, {"M": 0}, -1, b"at least 1"),
        (combine, {"M": 17}, -2, b"at most 16"),
        (combine, {"total_loc": -3}, -1, b"negative size"),
        (combine, {"B": -1}, -1, b"negative size"),
        (combine, {"M": 4, "total_loc": 1 << 30, "theta": dbl(0, 0, 0, 0), "beta": dbl(1, 1, 1, 1), "phi": dbl(0, 0, 0, 0)}, -2, b"int32"),
        (combine, {"n_src": 1 << 31}, -2, b"int32"),
        (combine, {"theta": None}, -1, b"null theta"),
        (combine, {"beta": dbl(1, nan)}, -1, b"beta must be finite"),
        (combine, {"phi": dbl(0, 1e3)}, -1, b"box"),
        (combine, {"src": None}, -1, b"null"),
        (combine, {"loc_off": None}, -1, b"null"),
        (combine, {"rw_idx": None}, -1, b"null"),
    ):
        assert call(**kwargs) == rc, (call.__name__, kwargs, lib.bl_last_error())
        assert text in lib.bl_last_error(), (call.__name__, kwargs, lib.bl_last_error())
        assert b"bl_ens" in lib.bl_last_error()  # the entry point names itself
    # nothing to do: no launch, no error -- also where nothing but the parameters is given
    assert loc(S=0, total=0, vals=None, present=None, seg_off=None, tgt=None, partials=None, out=None) == 0
    assert rw(S=0, vals=None, present=None, partials=None, out=None) == 0
    assert combine(B=0, total_loc=0, total_rw=0, src=None, loc_idx=None, rw_idx=None, out_loc=None, out_rw=None) == 0
    # the facade has no CPU fallback, and the kinds of ensemble_combine are what they were
    i = torch.zeros((2, 1), dtype=torch.int32)
    with pytest.raises(hip_ops.HipOpsUnavailable):
        hip_ops.ens_rw_stats(torch.zeros((2, 1), dtype=torch.float32), i, [0.0, 0.0])
    with pytest.raises(hip_ops.HipOpsUnavailable):
        hip_ops.ens_loc_stats(torch.zeros((2, 3), dtype=torch.float32), i, torch.zeros(2, dtype=torch.int32),
                              torch.zeros(1, dtype=torch.int32), [0, 0], [1, 1])
    assert hip_ops.ENSEMBLE_KINDS == {"avg": 0, "consensus": 1}


# ---- the wrapper and the command line ------------------------------------------------------------------------------------------
SEQ_SPEC = {"hidden_state_size": 32, "num_layers": 1, "num_heads": 4, "intermediate_dimension_size": 48, "dropout_rate": 0.1}


def _members(data):
    from buglab.models.modelregistry import load_model

    specs = ({"modelName": "gnn-mlp", "hidden_state_size": 32, "dropout_rate": 0.1}, dict(SEQ_SPEC, modelName="seq-great"))
    members = [load_model(spec, Path("/nonexistent/m.pkl.gz"))[0] for spec in specs]
    for m in members:
        m.compute_metadata(copy.deepcopy(data))
    return members


def test_wrapper_accepts_weighted_and_still_refuses_unknown_kinds(tmp_path):
    from buglab.data.synthetic import make_buglab_seq_dataset
    from buglab.models.ensemble import _weights as W
    from buglab.models.ensemble.__main__ import main
    from buglab.models.ensemble.wrapper import EnsembleWrapper

    members = _members(make_buglab_seq_dataset(6, seed=5))
    ens = EnsembleWrapper(members, "weighted")
    assert ens.kind == "weighted" and ens.ensemble_weights == W.EnsembleWeights.identity(2) and ens.ensemble_weights.is_identity
    fitted = W.EnsembleWeights((0.0, -0.5), (1.5, 0.75), (0.0, 2.0), (10, 5), (1.0, 1.0), (0.9, 0.8))
    assert EnsembleWrapper(members, "weighted", weights=fitted).ensemble_weights is fitted
    with pytest.raises(ValueError, match="members"):
        EnsembleWrapper(members, "weighted", weights=W.EnsembleWeights.identity(3))
    with pytest.raises(ValueError, match="weighted"):
        EnsembleWrapper(members, "avg", weights=fitted)
    with pytest.raises(ValueError, match="kind"):
        EnsembleWrapper(members, "majority")
    assert EnsembleWrapper(members, "avg").ensemble_weights is None
    for argv in (["median", "m.pkl.gz"],                                   # an unknown kind, as before
                 ["weighted", "m.pkl.gz"],                                 # fitted kinds say what they are fitted on
                 ["avg", "m.pkl.gz", "--fit-on", str(tmp_path)],           # the others gain no option
                 ["consensus", "m.pkl.gz", "--host-fit"]):
        with pytest.raises(SystemExit):
            main([str(tmp_path / "o.pkl.gz")] + argv)
    assert not (tmp_path / "o.pkl.gz").exists()


def test_cli_says_that_weighted_needs_fit_on(tmp_path, capsys):
    from buglab.models.ensemble.__main__ import main

    with pytest.raises(SystemExit):
        main([str(tmp_path / "o.pkl.gz"), "weighted", "m.pkl.gz"])
    assert "--fit-on" in capsys.readouterr().err


@pytest.mark.parametrize("kind", ["avg", "consensus", "weighted"])
def test_an_ensemble_pickled_without_the_new_attribute_combines_as_before(kind, monkeypatch):
    """A file written before there were weights has no `_weights` in its state: `avg` / `consensus` go to
    hip_ops.ensemble_combine with their kind as they did; `weighted` goes to the weighted kernel with its own parameters."""
    from buglab.data.synthetic import make_buglab_seq_dataset
    from buglab.models import hip_ops
    from buglab.models.ensemble import _weights as W
    from buglab.models.ensemble.wrapper import EnsembleWrapper

    data = make_buglab_seq_dataset(6, seed=5)
    ens = EnsembleWrapper(_members(data), kind)
    if kind != "weighted":
        del ens.__dict__["_weights"]  # the state of a wrapper pickled before this attribute existed
    ens = pickle.loads(pickle.dumps(ens))
    assert ens.kind == kind and (ens.ensemble_weights is None) == (kind != "weighted")
    points = copy.deepcopy(data)
    for m in ens.models:
        m._tensorize_only_at_target_location_rewrites = False
    batches = list(ens._gather(map(ens._tensorize_all, points)))
    emb = ens._finalize(batches[0], "cpu")
    calls = []

    def fake(name):
        def combine(src, loc_idx, loc_off, rw_idx, rw_off, *rest):
            calls.append((name,) + rest)
            return torch.zeros(loc_idx.shape[1] + rw_idx.shape[1], dtype=torch.float64)
        return combine

    monkeypatch.setattr(hip_ops, "ensemble_combine", fake("ensemble_combine"))
    monkeypatch.setattr(hip_ops, "ensemble_combine_weighted", fake("ensemble_combine_weighted"))
    sizes = iter(emb.flat_sizes)
    monkeypatch.setattr(EnsembleWrapper, "_member_flat_output",
                        staticmethod(lambda nn_, mb: torch.zeros(next(sizes), dtype=torch.float32)))
    out = list(ens._predict_minibatch(emb, [None, None]))
    assert len(out) == len(emb.originals) > 0
    ident = W.EnsembleWeights.identity(2)
    assert calls == ([("ensemble_combine", kind)] if kind != "weighted" else
                     [("ensemble_combine_weighted", ident.theta, ident.beta, ident.phi)])
