"""GPU: confidence calibration on the MI355X -- the stats kernels and the in-place apply of csrc/bl_confidence.hip against their
NumPy twin (buglab/models/_calibrate.py, which tests/test_calibrate_host.py pins to finite differences), and `calibrate_model`
end to end on a tiny gnn-mlp and a tiny seq-great.

Pools.  Segment lengths 1 (NO_BUG alone: every derivative with respect to beta is exactly 0), 2, 63, 64, 65 (one wave and its
two neighbours), 257 and 1025 (past a workgroup's 256 threads, past 16 strides of a wave); one segment (B = 1) and 300 of them
(75 workgroups of four waves, the last one partly filled is covered by the 7-segment pool); the target first and the target
NO_BUG; one -inf entry; (beta, bias) = (1, 0), (2^-4, -8), (16, 8), where exp(z) itself would overflow without the shift.

Tolerances.  Stats: each returned sum within 1e-11 * sum|terms| of the twin's, sum|terms| from the twin.  The two sides run the
same operations (the kernels are compiled without fused multiply-adds) except exp / log1p, a few fp64 ulp each over at most
about 2 000 terms, and the order of the sums, n * 2^-53: about 2e-12.  Apply: 1 ulp of fp32 against the twin's rounded fp64
value (the two fp64 values differ in their last digits, which can fall on either side of an fp32 rounding boundary)."""
import json

import numpy as np
import pytest
import torch

from tests.guard_bands import guarded
from tests.test_calibrate_host import _log_softmax

pytestmark = pytest.mark.gpu

DEV = "cuda"
LENGTHS = (1, 2, 63, 64, 65, 257, 1025)
PARAMETERS = ((1.0, 0.0), (2.0 ** -4, -8.0), (16.0, 8.0))
STATS_BOUND = 1e-11


def _pool(lengths, seed, minus_inf=True):
    """Segment s: a log-softmax of 2 * normal draws in fp32; the target first on even s, NO_BUG on odd s; one -inf entry (in the
    first segment of 65 or more entries, neither its target nor NO_BUG)."""
    from buglab.models._calibrate import Pool

    rng = np.random.default_rng(seed)
    vals, tgt = [], []
    for s, n in enumerate(lengths):
        x = 2.0 * rng.standard_normal(n)
        if minus_inf and n >= 65:
            x[n // 2] = -np.inf
            minus_inf = False
        vals.append(_log_softmax(x).astype(np.float32))
        tgt.append(0 if s % 2 == 0 else n - 1)
    off = np.zeros(len(lengths) + 1, np.int32)
    np.cumsum(lengths, out=off[1:])
    return Pool(np.concatenate(vals), off, np.asarray(tgt, np.int32))


_POOLS = {}


def pool_of(name):
    """The pools and the twin's stats on them, computed once."""
    if name not in _POOLS:
        from buglab.models import _calibrate as K

        if name == "seven":
            pool = _pool(LENGTHS, seed=1)
        elif name == "B300":
            pool = _pool([LENGTHS[s % 7] for s in range(300)], seed=2)
        else:  # "one-<length>-<first|nobug>"
            _, n, where = name.split("-")
            pool = _pool([int(n)], seed=3 + int(n), minus_inf=False)
            pool = pool._replace(tgt=np.asarray([0 if where == "first" else int(n) - 1], np.int32))
        twin = {p: (K.loc_stats(pool, *p), K.group_stats(pool, p[0])) for p in PARAMETERS}
        _POOLS[name] = (pool, twin)
    return _POOLS[name]


def _dev(pool):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in pool)


POOL_NAMES = ["seven", "B300"] + [f"one-{n}-{w}" for n in LENGTHS for w in ("first", "nobug")]


@pytest.mark.parametrize("name", POOL_NAMES)
def test_stats_kernels_against_the_twin(name):
    from buglab.models import hip_ops

    pool, twin = pool_of(name)
    dev = _dev(pool)
    for params in PARAMETERS:
        (want, scale), (gwant, gscale) = twin[params]
        assert np.isfinite(want).all() and np.isfinite(gwant).all()
        got = hip_ops.conf_loc_stats(*dev, *params).cpu().numpy()
        ggot = hip_ops.conf_group_stats(*dev, params[0]).cpu().numpy()
        for c, column in enumerate(("F", "dbeta", "dbias", "dbeta2", "dbeta dbias", "dbias2")):
            print(f"[calibrate] {name} {params} {column}: device {got[c]:.17g} twin {want[c]:.17g} |d| {abs(got[c] - want[c]):.3e} "
                  f"bound {STATS_BOUND * scale[c]:.3e}")
            assert abs(got[c] - want[c]) <= STATS_BOUND * scale[c], (name, params, column)
        for c, column in enumerate(("F_r", "F_r'", "F_r''")):
            print(f"[calibrate] {name} {params[0]} {column}: device {ggot[c]:.17g} twin {gwant[c]:.17g} |d| {abs(ggot[c] - gwant[c]):.3e} "
                  f"bound {STATS_BOUND * gscale[c]:.3e}")
            assert abs(ggot[c] - gwant[c]) <= STATS_BOUND * gscale[c], (name, params, column)
        if name.startswith("one-1-"):  # NO_BUG alone: nothing depends on beta, and the loss is log 1
            assert got.tolist() == [0.0] * 6 and ggot.tolist() == [0.0] * 3
        # two launches: bit-identical
        assert hip_ops.conf_loc_stats(*dev, *params).cpu().numpy().tobytes() == got.tobytes()
        assert hip_ops.conf_group_stats(*dev, params[0]).cpu().numpy().tobytes() == ggot.tobytes()


def test_stats_of_no_segments_and_of_what_cannot_be():
    from buglab.models import hip_ops

    none = (torch.zeros(0, dtype=torch.float32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV),
            torch.zeros(0, dtype=torch.int32, device=DEV))
    assert hip_ops.conf_group_stats(*none, 2.0).cpu().tolist() == [0.0] * 3  # a pool with zero repair groups
    assert hip_ops.conf_loc_stats(*none, 2.0, 1.0).cpu().tolist() == [0.0] * 6
    pool, _ = pool_of("seven")
    vals, off, tgt = _dev(pool)
    bad = tgt.clone()
    bad[3] = 64  # outside its segment of 64
    assert torch.isnan(hip_ops.conf_loc_stats(vals, off, bad, 1.0, 0.0)).all()
    with pytest.raises(ValueError, match="nseg"):
        hip_ops.conf_loc_stats(vals, off[:-1], tgt, 1.0, 0.0)
    with pytest.raises(RuntimeError, match="beta"):
        hip_ops.conf_loc_stats(vals, off, tgt, 0.0, 0.0)


# ---- apply ----------------------------------------------------------------------------------------------------------------
def _ordered(x):
    """fp32 values as integers in which neighbours differ by 1 (and -0.0 == 0.0)"""
    i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def _flat_case(name, seed):
    """A flat output [candidates by sample | NO_BUG by sample | repair items] from the named location pool, its repair part the
    same pool's segments as groups whose items lie scattered: -> (flat, candidate_ptr, B, group_ptr, group_items)."""
    pool, _ = pool_of(name)
    rng = np.random.default_rng(seed)
    B = pool.tgt.shape[0]
    lens = np.diff(pool.off)
    cand = np.concatenate([pool.vals[pool.off[b]:pool.off[b + 1] - 1] for b in range(B)] + [np.zeros(0, np.float32)])
    nobug = pool.vals[pool.off[1:] - 1]
    cptr = np.zeros(B + 1, np.int32)
    np.cumsum(lens - 1, out=cptr[1:])
    n_items = pool.vals.shape[0]
    items = rng.permutation(n_items).astype(np.int32)  # group g owns items[off[g] : off[g + 1]]
    repair = np.empty(n_items, np.float32)
    repair[items] = pool.vals
    return np.concatenate([cand, nobug, repair]).astype(np.float32), cptr, B, pool.off.copy(), items


@pytest.mark.parametrize("name", POOL_NAMES)
def test_apply_against_the_twin(name):
    from buglab.models import _calibrate as K
    from buglab.models import hip_ops

    flat, cptr, B, gptr, gitems = _flat_case(name, seed=5)
    n = flat.shape[0]
    to = lambda a: torch.from_numpy(a).to(DEV)
    d_cptr, d_gptr, d_gitems = to(cptr), to(gptr), to(gitems)
    for beta, bias in PARAMETERS[1:] + ((0.75, -0.5),):
        cal = K.ConfidenceCalibration(beta, bias, 1.0 / beta)
        want = flat.copy()
        K.apply_host(want, cptr, B, gptr, gitems, cal)
        g = guarded(1, n, ld=(n + 3) // 4 * 4, dtype=torch.float32, device=DEV, guard_rows=4)
        g.fill(to(flat)[None, :])
        buf = g.view[0]
        hip_ops.conf_apply(buf, d_cptr, B, d_gptr, d_gitems, beta=beta, no_bug_bias=bias, repair_beta=1.0 / beta)
        got = buf.cpu().numpy()
        g.assert_untouched(f"conf_apply {name}")
        assert (np.isneginf(got) == np.isneginf(flat)).all() and not np.isnan(got).any()
        fin = ~np.isneginf(flat)
        worst = np.abs(_ordered(got[fin]) - _ordered(want[fin])).max()
        print(f"[calibrate] apply {name} ({beta}, {bias}): worst distance to the twin {worst} ulp")
        assert worst <= 1
        C = int(cptr[-1])
        p = np.exp(got.astype(np.float64))
        for b in range(B):  # every segment is a distribution again
            at = np.concatenate([np.arange(cptr[b], cptr[b + 1]), [C + b]])
            assert abs(p[at].sum() - 1.0) <= at.shape[0] * 2.0 ** -23
        for k in range(gptr.shape[0] - 1):
            at = C + B + gitems[gptr[k]:gptr[k + 1]].astype(np.int64)
            assert abs(p[at].sum() - 1.0) <= at.shape[0] * 2.0 ** -23
    # the parts whose parameters are the identity stay as they are, bit for bit
    buf = to(flat)
    hip_ops.conf_apply(buf, d_cptr, B, d_gptr, d_gitems, beta=1.0, no_bug_bias=0.0, repair_beta=2.0)
    assert buf[:C + B].cpu().numpy().tobytes() == flat[:C + B].tobytes()
    buf = to(flat)
    hip_ops.conf_apply(buf, d_cptr, B, d_gptr, d_gitems, beta=2.0, no_bug_bias=0.0, repair_beta=1.0)
    assert buf[C + B:].cpu().numpy().tobytes() == flat[C + B:].tobytes()


# ---- end to end -----------------------------------------------------------------------------------------------------------
SPECS = {"gnn-mlp": {"hidden_state_size": 32, "num_layers": 4},
         "seq-great": {"hidden_state_size": 32, "num_layers": 1, "num_heads": 4, "intermediate_dimension_size": 48}}


@pytest.fixture(scope="module", params=["gnn-mlp", "seq-great"])
def calibrated(request, tmp_path_factory):
    """family -> a tiny detector trained for 30 steps (10 epochs of 3 minibatches, Adam at 1e-3 without warm-up: the trainer's
    default schedule would still be warming up) on 24 synthetic samples, then calibrated on them."""
    import copy

    from buglab.data.synthetic import make_buglab_dataset, make_buglab_seq_dataset
    from buglab.models import calibrate
    from buglab.models.modelregistry import load_model
    from buglab.runtime.neuralmodel import AbstractNeuralModel
    from buglab.runtime.optim import FlatAdam
    from buglab.runtime.trainer import ModelTrainer

    family = request.param
    data = (make_buglab_seq_dataset if family.startswith("seq") else make_buglab_dataset)(24, seed=41)
    root = tmp_path_factory.mktemp(family.replace("-", "_"))
    path = root / "detector.pkl.gz"
    model = load_model(dict(SPECS[family], modelName=family), path)[0]
    trainer = ModelTrainer(model, path, max_num_epochs=10, minibatch_size=8,
                           optimizer_creator=lambda params: FlatAdam(params, lr=1e-3, num_warmup_steps=0))
    torch.manual_seed(0)
    np.random.seed(0)
    trainer.train(copy.deepcopy(data), copy.deepcopy(data[:8]), show_progress_bar=False, parallelize=False, patience=100)
    device = torch.device(DEV)
    model, nn_ = AbstractNeuralModel.restore_model(path, device)
    assert model.confidence_calibration is None
    report = {}
    cal = calibrate.calibrate_model(model, nn_, data, device, report=report)
    assert model.confidence_calibration == cal
    out = root / "calibrated.pkl.gz"
    model.save(out, nn_)
    return {"family": family, "plain": path, "calibrated": out, "data": data, "cal": cal, "report": report}


def _restore(path):
    from buglab.runtime.neuralmodel import AbstractNeuralModel

    return AbstractNeuralModel.restore_model(path, torch.device(DEV))


def test_device_fit_is_the_twins_optimum(calibrated):
    """The device-fitted parameters in the twin's gradient on the pool copied to the host: max|g| <= 2e-9 n (the factor 2: the two
    sides' evaluations differ).  A parameter the fit had to clamp to its box cannot have a zero gradient: there the loss must
    still fall towards the outside (and the calibration says it did not converge)."""
    from buglab.models import _calibrate as K
    from buglab.models import calibrate

    model, nn_ = _restore(calibrated["plain"])
    collected = calibrate.collect_calibration_pool(model, nn_, calibrated["data"], torch.device(DEV))
    cal, details = calibrate.fit_on_device(collected)
    assert cal == calibrated["cal"]  # the fit is reproducible bit for bit
    loc, rw = collected.host_pools()
    n, nb = collected.num_samples, collected.num_buggy
    assert n == 24 and 0 < collected.num_bug_free < n and nb == n - collected.num_bug_free == rw.tgt.shape[0]
    g = K.loc_stats(loc, cal.beta, cal.no_bug_bias)[0][1:3]
    gr = K.group_stats(rw, cal.repair_beta)[0][1]
    print(f"[calibrate] {calibrated['family']}: {cal}; twin gradient {g} / {gr}; iterations "
          f"{details['localization']['iterations']} / {details['repair']['iterations']}")
    interior = True
    for value, grad, box, count in ((cal.beta, g[0], K.BETA_BOX, n), (cal.no_bug_bias, g[1], K.BIAS_BOX, n), (cal.repair_beta, gr, K.BETA_BOX, nb)):
        if box[0] < value < box[1]:
            assert abs(grad) <= 2e-9 * count
        else:
            interior = False
            assert (grad > 0) == (value == box[0])
    assert cal.converged == interior
    # NLL after calibration is no larger than before: (1, 0) is feasible
    report = calibrated["report"]
    assert report["localization_nll"]["after"] <= report["localization_nll"]["before"]
    assert report["repair_nll"]["after"] <= report["repair_nll"]["before"]
    assert report["localization_nll"]["before"] == pytest.approx(K.loc_stats(loc, 1.0, 0.0)[0][0] / n, rel=1e-12)
    assert 0.0 <= report["ece"]["after"] <= 1.0 and 0.0 <= report["ece"]["before"] <= 1.0
    json.dumps(report)


def _flat_outputs(model, nn_, data):
    from buglab.controllers import _batching as Bt

    out = []
    nn_.eval()
    with torch.no_grad(), model._tensorize_all_location_rewrites():
        for mb, _ in Bt.prediction_minibatches(model, ((d, None) for d in data), torch.device(DEV), False, lambda *a: None, lambda tag: None):
            out.append((Bt.flat_prediction_output(nn_, mb), mb))
    return out


def test_calibrated_outputs_are_the_twins_and_uncalibrated_ones_are_untouched(calibrated, monkeypatch):
    from buglab.models import _calibrate as K
    from buglab.models import hip_ops

    calls = []
    real = hip_ops.conf_apply
    monkeypatch.setattr(hip_ops, "conf_apply", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    data, device = calibrated["data"], torch.device(DEV)
    plain_model, plain_nn = _restore(calibrated["plain"])
    cal_model, cal_nn = _restore(calibrated["calibrated"])
    cal = cal_model.confidence_calibration
    assert cal == calibrated["cal"] and plain_model.confidence_calibration is None and not cal.is_identity

    # without a calibration: the forward's own values, bit for bit, and nothing launched
    (raw, mb), = _flat_outputs(plain_model, plain_nn, data)
    assert "confidence_calibration" not in mb
    with torch.no_grad():
        _, loc_lp, enc, _ = plain_nn.compute_localization_logprobs(mb["graph_data"])
        swap_lp, text_lp, var_lp, _ = plain_nn._compute_repair_logprobs(
            enc, mb["target_rewrites"], mb["rewrite_to_location_group"], mb["candidate_symbol_to_location_group"],
            mb["swapped_pair_to_call_location_group"], mb["repair_group_ptr"], mb["repair_group_items"])
    by_hand = torch.cat([t.reshape(-1).float() for t in (loc_lp, text_lp, var_lp, swap_lp)])
    assert raw.cpu().numpy().tobytes() == by_hand.cpu().numpy().tobytes()
    plain = list(plain_model.predict(iter(data), plain_nn, device, False))
    assert len(plain) == 24 and calls == []

    # with it: the twin's apply of the raw output, to 1 ulp
    (got, mb_cal), = _flat_outputs(cal_model, cal_nn, data)
    assert len(calls) == 1 and mb_cal["confidence_calibration"] == cal
    want = raw.cpu().numpy().copy()
    K.apply_host(want, mb["graph_data"]["candidate_ptr"].cpu().numpy(), 24, mb["repair_group_ptr"].cpu().numpy(),
                 mb["repair_group_items"].cpu().numpy(), cal)
    got = got.cpu().numpy()
    assert (np.isneginf(got) == np.isneginf(want)).all()
    fin = ~np.isneginf(want)
    assert np.abs(_ordered(got[fin]) - _ordered(want[fin])).max() <= 1

    # calibrated `predict` never reverses an order among a sample's candidates
    predictions = list(cal_model.predict(iter(data), cal_nn, device, False))
    assert len(predictions) == 24 and len(calls) == 2
    moved = False
    for (_, loc0, rw0), (_, loc1, rw1) in zip(plain, predictions):
        assert list(loc0) == list(loc1) and len(rw0) == len(rw1)
        keys = [k for k in loc0 if k != -1]
        a, b = np.array([loc0[k] for k in keys]), np.array([loc1[k] for k in keys])
        assert not ((a[:, None] > a[None, :]) & (b[:, None] < b[None, :])).any()
        moved = moved or loc0[-1] != loc1[-1]
    assert moved


def test_on_device_report_of_a_calibrated_checkpoint_is_the_host_report(calibrated):
    from buglab.models.evaluate import evaluate_on_device, evaluate_predictions

    model, nn_ = _restore(calibrated["calibrated"])
    data, device = calibrated["data"], torch.device(DEV)
    host = evaluate_predictions(model.predict(iter(data), nn_, device, False)).format()
    assert evaluate_on_device(model, nn_, data, device, parallelize=False).format() == host
    plain_model, plain_nn = _restore(calibrated["plain"])
    plain = evaluate_predictions(plain_model.predict(iter(data), plain_nn, device, False)).format()
    assert plain != host  # the confidences moved


def test_cli_writes_a_calibrated_checkpoint(calibrated, tmp_path, capsys, monkeypatch):
    from buglab.models import calibrate
    from buglab.utils.msgpackutils import save_msgpack_l_gz

    # the msgpack reader in Python: the sequence models' token projection rejects the synthetic sequence samples as the native
    # reader presents them (every one of them: "node N has no parent to fall back to"), whatever the entry point
    monkeypatch.setenv("BUGLAB_NATIVE_READER", "0")
    (tmp_path / "valid").mkdir()
    save_msgpack_l_gz(calibrated["data"], tmp_path / "valid" / "x.msgpack.l.gz")
    out, rep = tmp_path / "out.pkl.gz", tmp_path / "report.json"
    # from the CALIBRATED checkpoint: its calibration is ignored while collecting and replaced by the same fit
    cal = calibrate.run(calibrate.parse_args([str(calibrated["calibrated"]), str(tmp_path / "valid"), str(out), "--sequential",
                                              "--report-json", str(rep)]))
    text = capsys.readouterr().out
    assert "Calibrated on 24 samples" in text and "expected calibration error (15 bins)" in text and "NO_BUG bias" in text
    assert _restore(out)[0].confidence_calibration == cal
    assert cal.beta == pytest.approx(calibrated["cal"].beta, rel=1e-6)  # the same samples in the same order, through a file
    assert json.loads(rep.read_text())["calibration"]["beta"] == cal.beta
    no_bias = calibrate.run(calibrate.parse_args([str(calibrated["plain"]), str(tmp_path / "valid"), str(out), "--sequential", "--no-bias",
                                                  "--no-repair"]))
    assert no_bias.no_bug_bias == 0.0 and no_bias.repair_beta == 1.0 and no_bias.notes == ()
