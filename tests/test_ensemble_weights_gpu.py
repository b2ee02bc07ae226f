"""GPU: fitted ensembles (the `weighted` kind) on the MI355X -- bl_ens_loc_stats / bl_ens_rw_stats against the NumPy twin
(buglab/models/ensemble/_weights.py) and from launch to launch, bl_ensemble_combine_weighted against the twin and, at the
identity parameters, against the `avg` kernel, and end to end: two tiny trained members, a `weighted` ensemble fitted through
the command line on the device and with the host's statistics, its `predict` against the twin's combination of the members'
own predictions, and evaluate.py on the file."""
import copy
import json
import math
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import ensemble_weights_fixtures as X

pytestmark = pytest.mark.gpu

DEV = "cuda"
STATS_BOUND = 1e-11  # times the sum of the absolute values of the terms of a sum: tests/test_calibrate_gpu.py's bound
PARAMETERS = (((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)),                  # the identity: every member as it is
              ((0.3, 0.7, -1.1), (0.8, 1.3, 2.0), (-0.2, 0.5, 1.5)),
              ((0.0, -20.0, 20.0), (2.0 ** -6, 1.0, 2.0 ** 6), (20.0, 0.0, -20.0)))  # the corners of the boxes, one beta of 1


def _dev(a, dtype):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


@pytest.fixture(scope="module")
def pools():
    from buglab.models.ensemble import _weights as W

    loc, rw = X.edge_pools(extra_lengths=(300,))  # longer than a workgroup
    assert 300 in np.diff(loc.off)
    twin = {p: (W.loc_stats(loc, p[0], p[1]), W.rw_stats(rw, p[2])) for p in PARAMETERS}
    dev_loc = (_dev(np.nan_to_num(loc.vals, nan=0.0, neginf=-np.inf), torch.float32), _dev(loc.present, torch.int32),
               _dev(loc.off, torch.int32), _dev(loc.tgt, torch.int32))
    dev_rw = (_dev(np.nan_to_num(rw.vals, nan=0.0, neginf=-np.inf), torch.float32), _dev(rw.present, torch.int32))
    return {"twin": twin, "loc": dev_loc, "rw": dev_rw}


@pytest.mark.parametrize("params", PARAMETERS, ids=["identity", "inner", "corners"])
def test_stats_match_the_twin_and_repeat_bit_for_bit(pools, params):
    from buglab.models import hip_ops

    theta, beta, phi = params
    (want, scale), (rwant, rscale) = pools["twin"][params]
    assert np.isfinite(want).all() and np.isfinite(rwant).all()
    got = hip_ops.ens_loc_stats(*pools["loc"], theta, beta).cpu().numpy()
    rgot = hip_ops.ens_rw_stats(*pools["rw"], phi).cpu().numpy()
    assert got.shape == (7,) and rgot.shape == (4,)
    names = ["F"] + [f"dtheta{m}" for m in range(3)] + [f"dbeta{m}" for m in range(3)]
    for c, column in enumerate(names):
        print(f"[ensemble weights] {column}: device {got[c]:.17g} twin {want[c]:.17g} |d| {abs(got[c] - want[c]):.3e} "
              f"bound {STATS_BOUND * scale[c]:.3e}")
        assert abs(got[c] - want[c]) <= STATS_BOUND * scale[c], column
    for c, column in enumerate(["F_rw"] + [f"dphi{m}" for m in range(3)]):
        print(f"[ensemble weights] {column}: device {rgot[c]:.17g} twin {rwant[c]:.17g} |d| {abs(rgot[c] - rwant[c]):.3e} "
              f"bound {STATS_BOUND * rscale[c]:.3e}")
        assert abs(rgot[c] - rwant[c]) <= STATS_BOUND * rscale[c], column
    assert hip_ops.ens_loc_stats(*pools["loc"], theta, beta).cpu().numpy().tobytes() == got.tobytes()
    assert hip_ops.ens_rw_stats(*pools["rw"], phi).cpu().numpy().tobytes() == rgot.tobytes()


def test_stats_of_an_empty_pool_are_zero_and_parameters_are_counted(pools):
    from buglab.models import hip_ops

    empty = hip_ops.ens_rw_stats(torch.zeros((3, 0), dtype=torch.float32, device=DEV), torch.zeros((3, 0), dtype=torch.int32, device=DEV),
                                 (0.0, 0.5, 1.0))
    assert empty.cpu().tolist() == [0.0] * 4
    with pytest.raises(ValueError, match="members"):
        hip_ops.ens_rw_stats(*pools["rw"], (0.0, 0.0))
    with pytest.raises(RuntimeError, match="box"):
        hip_ops.ens_loc_stats(*pools["loc"], (0.0, 0.0, 21.0), (1.0, 1.0, 1.0))


def _assert_same(got, want, what):
    assert (np.isnan(got) == np.isnan(want)).all() and (np.isneginf(got) == np.isneginf(want)).all(), what
    fin = np.isfinite(want)
    assert fin.any() and (np.abs(got[fin] - want[fin]) <= 1e-12 * np.maximum(1.0, np.abs(want[fin]))).all(), what


@pytest.mark.parametrize("params", PARAMETERS, ids=["identity", "inner", "corners"])
def test_combine_kernel_matches_the_twin(params):
    """The `m3_65_entries` shape: sample 2 has an absent member and a member with a NaN and a -inf; sample 3 is predicted by no
    member and comes out NaN."""
    from buglab.models import hip_ops
    from buglab.models.ensemble import _weights as W

    theta, beta, phi = params
    src, loc_idx, loc_off, rw_idx, rw_off = X.gather_arrays(X.wide_samples(with_unpredicted=True))
    want_loc, want_rw = W.combine_weighted(src, loc_idx, loc_off, rw_idx, rw_off, theta, beta, phi)
    gather = (_dev(src, torch.float32), _dev(loc_idx, torch.int32), _dev(loc_off, torch.int32), _dev(rw_idx, torch.int32),
              _dev(rw_off, torch.int32))
    out = hip_ops.ensemble_combine_weighted(*gather, theta, beta, phi)
    assert out.dtype == torch.float64
    got = out.cpu().numpy()
    total_loc = loc_idx.shape[1]
    assert np.isnan(got[loc_off[3]:loc_off[4]]).all() and np.isnan(got[total_loc + rw_off[3]:]).all()
    assert np.isnan(want_loc[loc_off[3]:]).all() and not np.isnan(want_loc[:loc_off[2]]).any()
    _assert_same(got[:total_loc], want_loc, "locations")
    _assert_same(got[total_loc:], want_rw, "rewrites")
    assert hip_ops.ensemble_combine_weighted(*gather, theta, beta, phi).cpu().numpy().tobytes() == got.tobytes()
    if params == PARAMETERS[0]:  # the identity parameters are `avg`
        avg = hip_ops.ensemble_combine(*gather, "avg").cpu().numpy()
        _assert_same(got, avg, "avg")


# ---- end to end ----------------------------------------------------------------------------------------------------------------
SPECS = {"gnn-mlp": {"hidden_state_size": 32, "num_layers": 4},
         # max_seq_size: the sequence member drops out of the two longest of the 24 held-out samples
         "seq-great": {"hidden_state_size": 32, "num_layers": 1, "num_heads": 4, "intermediate_dimension_size": 48, "max_seq_size": 45}}
EPOCHS = {"gnn-mlp": 3, "seq-great": 30}  # of 3 minibatches each


def _restore(path):
    from buglab.runtime.neuralmodel import AbstractNeuralModel

    return AbstractNeuralModel.restore_model(Path(path), torch.device(DEV))


@pytest.fixture(scope="module")
def fitted(tmp_path_factory):
    """One graph member (9 training steps) and one sequence member (90) trained on 24 synthetic samples; a `weighted` ensemble of
    them fitted on 24 OTHER synthetic samples through the command line, once with the device's statistics and once with the host
    twin's.

    Why these members and held-out data.  Training here runs through floating-point atomics, so every run of the suite fits
    slightly different members: the comparison of the two fits has to be well conditioned for all of them, not for one.  Fitted on
    its own training samples, or with both members trained equally briefly, one member is better on EVERY sample; its weight
    then runs towards the box along a direction in which the loss flattens exponentially, the other member's temperature
    stops mattering, and the location Hessian has eigenvalues of 1e-9: where such a fit stops is decided by the last digits.
    On held-out samples, with the sequence member trained longer, each member is the better one on some samples and the location
    optimum is interior (theta_1 about -1.4, beta about 1.2 and 0.5, smallest Hessian eigenvalue 0.07 .. 0.19 over retrainings)."""
    from buglab.data.synthetic import make_buglab_seq_dataset
    from buglab.models.ensemble.__main__ import main
    from buglab.models.modelregistry import load_model
    from buglab.runtime.optim import FlatAdam
    from buglab.runtime.trainer import ModelTrainer
    from buglab.utils.msgpackutils import save_msgpack_l_gz

    root = tmp_path_factory.mktemp("weighted")
    train, data = make_buglab_seq_dataset(24, seed=41), make_buglab_seq_dataset(24, seed=43)
    paths = []
    for family in ("gnn-mlp", "seq-great"):
        path = root / f"{family}.pkl.gz"
        model = load_model(dict(SPECS[family], modelName=family), path)[0]
        trainer = ModelTrainer(model, path, max_num_epochs=EPOCHS[family], minibatch_size=8,
                               optimizer_creator=lambda params: FlatAdam(params, lr=1e-3, num_warmup_steps=0))
        torch.manual_seed(0)
        np.random.seed(0)
        trainer.train(copy.deepcopy(train), copy.deepcopy(train[:8]), show_progress_bar=False, parallelize=False, patience=100)
        paths.append(path)
    (root / "valid").mkdir()
    save_msgpack_l_gz(data, root / "valid" / "x.msgpack.l.gz")
    out = {"root": root, "data": data, "members": paths}
    with pytest.MonkeyPatch.context() as mp:
        # the msgpack reader in Python: the sequence models' token projection rejects the synthetic sequence samples as the
        # native reader presents them (tests/test_calibrate_gpu.py)
        mp.setenv("BUGLAB_NATIVE_READER", "0")
        for name, extra in (("device", []), ("host", ["--host-fit"])):
            main([str(root / f"{name}.pkl.gz"), "weighted"] + [str(p) for p in paths] +
                 ["--fit-on", str(root / "valid"), "--sequential", "--report-json", str(root / f"{name}.json")] + extra)
            out[name] = json.loads((root / f"{name}.json").read_text())
    return out


def _twin_hessian(loc, x, free):
    """Central differences of the twin's location gradient over the free parameters, symmetrised."""
    from buglab.models.ensemble import _weights as W

    M, h = x.shape[0] // 2, 1e-5
    grad = lambda v: W.loc_stats(loc, v[:M], v[M:])[0][1:]
    H = np.zeros((len(free), len(free)))
    for a, k in enumerate(free):
        e = np.zeros(x.shape[0])
        e[k] = h
        H[a] = (grad(x + e) - grad(x - e))[free] / (2 * h)
    return 0.5 * (H + H.T)


def test_cli_fits_on_the_device_what_the_host_fit_finds(fitted, capsys):
    """`--host-fit` gives the same parameters within rel=1e-6.  What that rests on, checked or printed here:
    both fits meet their gradient criterion, and the location optimum is interior with a positive definite Hessian.  The two runs
    execute the same optimiser on statistics that agree to STATS_BOUND (1e-11 of the summed absolute terms, asserted above;
    observed: a few 1e-16), so they take the same steps, and to first order their end points differ by H^-1 (g_device - g_host):
    with |H^-1| <= 1 / 0.07 and the gradients of one point at most 1e-11 x 50 apart, below 1e-8 -- a hundredth of the bound.  If
    one run takes a step more than the other (seen in two of ten fits), both still end inside the gradient criterion and the
    printed first-order bound with their actual gradients applies; observed distances: 1e-15 .. 2.5e-9 relative.
    The rewrite head is the exception and is stated as one: on every pair of tiny members tried the sequence member gives the
    true rewrite the higher probability on every buggy sample, so phi_1 has no interior optimum; it runs towards the box and stops
    near 18 where c exp(-phi) meets the gradient criterion, with a second derivative of 1e-8.  Its agreement (observed 1e-11 ..
    6e-9 relative over twenty fits) rests on the two runs taking identical steps, not on conditioning."""
    from buglab.models.ensemble import _weights as W
    from buglab.models.ensemble import fit as Fit
    from buglab.models.ensemble.wrapper import EnsembleWrapper

    model, nn_ = _restore(fitted["root"] / "device.pkl.gz")
    assert isinstance(model, EnsembleWrapper) and model.kind == "weighted"
    w = model.ensemble_weights
    report, host = fitted["device"], fitted["host"]
    print(f"[ensemble weights] device fit {report['weights']}\n[ensemble weights] host fit {host['weights']}")
    assert isinstance(w, W.EnsembleWeights) and list(w.theta) == report["weights"]["theta"] and w.fitted_on == (24, report["num_buggy"])
    assert report["num_samples"] == 24 and 0 < report["num_buggy"] < 24 and not report["host_fit"] and host["host_fit"]
    assert w.theta[0] == 0.0 and w.phi[0] == 0.0 and not w.is_identity
    # both fits met their gradient criterion, and no location parameter sits on its box
    for side in (report, host):
        for head in ("localization", "rewrite"):
            assert side["fit"][head]["converged"], (side["host_fit"], head, side["fit"][head])
        assert side["fit"]["localization"]["on_box"] == [], side["fit"]["localization"]
    # the location optimum is interior and well conditioned: the twin's Hessian there, on the pool copied to the host
    collected = Fit.collect_ensemble_pool(model, nn_, copy.deepcopy(fitted["data"]), torch.device(DEV), parallelize=False)
    loc, _ = collected.host_pools()
    x, free = np.array(w.theta + w.beta), [1, 2, 3]
    H = _twin_hessian(loc, x, free)
    eig = np.linalg.eigvalsh(H)
    g = [np.abs(np.array(side["fit"]["localization"]["gradient"])[free]) for side in (report, host)]
    first_order = np.abs(np.linalg.inv(H)) @ (g[0] + g[1])
    apart = np.abs(np.array(report["weights"]["theta"] + report["weights"]["beta"]) - np.array(host["weights"]["theta"] + host["weights"]["beta"]))[free]
    print(f"[ensemble weights] location Hessian eigenvalues {eig}; end gradients {g[0]} / {g[1]}; first-order bound on the distance "
          f"{first_order} (relative {first_order / np.abs(x[free])}); observed {apart}; phi {report['weights']['phi']} / {host['weights']['phi']}")
    assert eig[0] > 0.0
    for name in ("theta", "beta", "phi"):
        assert report["weights"][name] == pytest.approx(host["weights"][name], rel=1e-6), name
    for k in range(2):
        assert w.nll_after[k] <= w.nll_before[k]
        assert host["weights"]["nll_after"][k] <= host["weights"]["nll_before"][k]
        assert report["weights"]["nll_before"][k] == pytest.approx(host["weights"]["nll_before"][k], rel=1e-12)
    assert sum(report["location_weight"]) == pytest.approx(1.0, abs=1e-12)


def test_predict_is_the_twins_combination_of_the_members_own_predictions(fitted):
    from buglab.models.ensemble import _weights as W

    device = torch.device(DEV)
    model, nn_ = _restore(fitted["root"] / "device.pkl.gz")
    w = model.ensemble_weights
    points = copy.deepcopy(fitted["data"])
    got = list(model.predict(iter(points), nn_, device, False))
    assert len(got) == 24
    own = []
    for path in fitted["members"]:
        member, member_nn = _restore(path)
        mine = copy.deepcopy(fitted["data"])
        pos = {id(p): i for i, p in enumerate(mine)}
        own.append({pos[id(p)]: (l, r) for p, l, r in member.predict(iter(mine), member_nn, device, False)})
    # one minibatch per member, of the same samples as inside the ensemble; the sequence member rejects the longest samples
    assert len(own[0]) == 24 and 0 < len(own[1]) < 24
    for i, (point, loc, rw) in enumerate(got):
        assert point is points[i]
        nodes = [k for k in loc if k != -1]
        assert nodes == sorted(nodes) and list(loc)[-1] == -1
        locs = [np.array([o[i][0][k] for k in nodes + [-1]], np.float32) if i in o else None for o in own]
        rws = [np.array(o[i][1], np.float32) if i in o else None for o in own]
        want_loc, want_rw = W.combine_sample(locs, rws, w.theta, w.beta, w.phi)
        _assert_same(np.array(list(loc.values())), want_loc, f"sample {i} locations")
        _assert_same(np.array(rw, np.float64), want_rw, f"sample {i} rewrites")
        assert math.isclose(float(np.exp(want_loc).sum()), 1.0, abs_tol=1e-5)


def test_evaluate_loads_the_weighted_ensemble_file(fitted, capsys, monkeypatch):
    from buglab.models import evaluate

    monkeypatch.setenv("BUGLAB_NATIVE_READER", "0")
    summary = evaluate.run({"MODEL_FILENAME": str(fitted["root"] / "device.pkl.gz"), "TEST_DATA_PATH": str(fitted["root"] / "valid"),
                            "--assume-buggy": False, "--eval-only-no-bug": False, "--limit-num-elements": None, "--sequential": True})
    assert summary["num_samples"] == 24
    assert capsys.readouterr().out.strip()
