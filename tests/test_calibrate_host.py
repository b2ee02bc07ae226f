"""CPU: confidence calibration's host side (buglab/models/_calibrate.py, calibrate.py) -- the NumPy twin against finite
differences of its own loss, the fit's optimality and its fixed point, the degenerate and the clamped pools, the pool indices
against the model's own collated groups, the calibrated un-batching on a CPU device, checkpoints with and without the field,
the CLI's arguments, the refusal of ensembles and the C entry points' argument errors."""
import copy
import ctypes
import pickle
from pathlib import Path

import numpy as np
import pytest
import torch

SEQ_SPEC = {"hidden_state_size": 32, "num_layers": 1, "num_heads": 4, "intermediate_dimension_size": 48, "dropout_rate": 0.1}


def _log_softmax(x):
    x = np.asarray(x, dtype=np.float64)
    return x - (x.max() + np.log(np.exp(x - x.max()).sum()))


def make_pool(lengths, targets, seed, scale=2.0):
    """A location pool: segment s has lengths[s] fp32 log-probabilities (a log-softmax of scaled normal draws), NO_BUG last,
    the target at place targets[s] (-1: NO_BUG)."""
    from buglab.models._calibrate import Pool

    rng = np.random.default_rng(seed)
    vals = [_log_softmax(scale * rng.standard_normal(n)).astype(np.float32) for n in lengths]
    off = np.zeros(len(lengths) + 1, np.int32)
    np.cumsum(lengths, out=off[1:])
    tgt = np.array([n - 1 if t < 0 else t for n, t in zip(lengths, targets)], np.int32)
    return Pool(np.concatenate(vals), off, tgt)


def noisy_pool(n, seed, sharpen=3.0, shift=1.5):
    """A miscalibrated detector's pool: the truth is drawn from p, the model reports log_softmax(sharpen * log p + shift on
    NO_BUG) -- over-confident and biased towards NO_BUG -- so that the optimum is near (1 / sharpen, -shift / sharpen)."""
    from buglab.models._calibrate import Pool

    rng = np.random.default_rng(seed)
    vals, lens, tgt = [], [], []
    for _ in range(n):
        k = int(rng.integers(2, 12))
        logp = _log_softmax(rng.standard_normal(k))
        tgt.append(int(rng.choice(k, p=np.exp(logp))))
        z = sharpen * logp
        z[-1] += shift
        vals.append(_log_softmax(z).astype(np.float32))
        lens.append(k)
    off = np.zeros(n + 1, np.int32)
    np.cumsum(lens, out=off[1:])
    return Pool(np.concatenate(vals), off, np.asarray(tgt, np.int32))


# ---- the stats ------------------------------------------------------------------------------------------------------------
def test_gradient_and_hessian_match_central_differences_of_the_loss():
    """Central differences at h = 1e-5 err by h^2 F''' / 6 ~ 1e-10 and by rounding eps F / h ~ 1e-10: relative 1e-6 is their bound."""
    from buglab.models import _calibrate as K

    pool = make_pool([4, 7, 2, 9, 5], [1, -1, 0, 3, -1], seed=3)
    h = 1e-5
    for beta, bias in ((0.7, 0.4), (1.0, 0.0), (2.5, -1.25)):
        s, _ = K.loc_stats(pool, beta, bias)
        at = lambda db, dc: K.loc_stats(pool, beta + db, bias + dc)[0]
        g_fd = np.array([(at(h, 0)[0] - at(-h, 0)[0]) / (2 * h), (at(0, h)[0] - at(0, -h)[0]) / (2 * h)])
        np.testing.assert_allclose(s[1:3], g_fd, rtol=1e-6, atol=0)
        h_fd = np.array([(at(h, 0)[1] - at(-h, 0)[1]) / (2 * h), (at(0, h)[1] - at(0, -h)[1]) / (2 * h),
                         (at(0, h)[2] - at(0, -h)[2]) / (2 * h)])
        np.testing.assert_allclose(s[3:6], h_fd, rtol=1e-6, atol=0)
        np.testing.assert_allclose((at(h, 0)[2] - at(-h, 0)[2]) / (2 * h), s[4], rtol=1e-6, atol=0)  # the mixed term, the other way
        r, _ = K.group_stats(pool, beta)
        rat = lambda db: K.group_stats(pool, beta + db)[0]
        np.testing.assert_allclose(r[1], (rat(h)[0] - rat(-h)[0]) / (2 * h), rtol=1e-6, atol=0)
        np.testing.assert_allclose(r[2], (rat(h)[1] - rat(-h)[1]) / (2 * h), rtol=1e-6, atol=0)


def test_stats_skip_zero_probability_entries_and_flag_what_cannot_be():
    from buglab.models import _calibrate as K

    pool = make_pool([5, 3], [1, -1], seed=4)
    with_inf = K.Pool(np.insert(pool.vals, 2, -np.inf).astype(np.float32), pool.off + np.array([0, 1, 1], np.int32),
                      pool.tgt + np.array([0, 0], np.int32))
    a, a_abs = K.loc_stats(pool, 1.7, -0.3)
    b, b_abs = K.loc_stats(with_inf, 1.7, -0.3)
    assert a.tobytes() == b.tobytes() and a_abs.tobytes() == b_abs.tobytes() and np.isfinite(a).all()
    one = K.Pool(np.zeros(1, np.float32), np.array([0, 1], np.int32), np.zeros(1, np.int32))  # NO_BUG alone
    assert K.loc_stats(one, 16.0, 8.0)[0].tolist() == [0.0] * 6
    assert np.isnan(K.loc_stats(K.Pool(pool.vals, pool.off, np.array([1, 7], np.int32)), 1.0, 0.0)[0]).all()  # a target outside
    empty = K.Pool(np.zeros(0, np.float32), np.zeros(1, np.int32), np.zeros(0, np.int32))
    assert K.loc_stats(empty, 1.0, 0.0)[0].tolist() == [0.0] * 6


# ---- the fit --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,seed", [(7, 3), (200, 2), (2000, 3)])
def test_fit_reaches_the_optimum(n, seed):
    from buglab.models import _calibrate as K

    pool = noisy_pool(n, seed)
    bug_free = int(np.sum(pool.tgt == np.diff(pool.off) - 1))
    assert 0 < bug_free < n  # both kinds, or the bias would be fixed
    cal, details = K.fit_host(pool, None, fit_repair=False)
    assert cal.converged and cal.notes == () and cal.repair_beta == 1.0
    assert 1 <= details["localization"]["iterations"] <= 25
    s, _ = K.loc_stats(pool, cal.beta, cal.no_bug_bias)
    assert np.abs(s[1:3]).max() <= 1e-9 * n
    for db in (-1e-3, 0.0, 1e-3):
        for dc in (-1e-3, 0.0, 1e-3):
            assert s[0] <= K.loc_stats(pool, cal.beta + db, cal.no_bug_bias + dc)[0][0]
    if n >= 200:  # the detector was sharpened by 3 and shifted by 1.5
        assert abs(cal.beta - 1 / 3) < 0.1 and abs(cal.no_bug_bias + 0.5) < 0.25
        assert s[0] < K.loc_stats(pool, 1.0, 0.0)[0][0]


def test_fitting_a_calibrated_pool_returns_the_identity():
    """After apply, (1, 0) is the optimum up to the one rounding to fp32: every value moves by at most 2^-24 |l'| ~ 6e-8 * 20, the
    gradient by at most n times that, and the Hessian is of the order n * Var(l) ~ n: the parameters move by ~1e-6.  1e-4 is
    that with a hundredfold margin."""
    from buglab.models import _calibrate as K

    pool = noisy_pool(300, 11)
    cal, _ = K.fit_host(pool, pool, fit_repair=False)
    again = K.Pool(K.apply_pool_host(pool, cal.beta, cal.no_bug_bias, True), pool.off, pool.tgt)
    cal2, _ = K.fit_host(again, None, fit_repair=False)
    assert cal2.converged and abs(cal2.beta - 1.0) <= 1e-4 and abs(cal2.no_bug_bias) <= 1e-4
    s, _ = K.loc_stats(again, cal2.beta, cal2.no_bug_bias)
    assert np.abs(s[1:3]).max() <= 1e-9 * 300
    # and the repair scale, on groups
    rcal, _ = K.fit_host(pool, pool, fit_bias=False)
    groups = K.Pool(K.apply_pool_host(pool, rcal.repair_beta, 0.0, False), pool.off, pool.tgt)
    rcal2, _ = K.fit_host(pool, groups, fit_bias=False)
    assert rcal.converged and abs(rcal.repair_beta - 1 / 3) < 0.1 and abs(rcal2.repair_beta - 1.0) <= 1e-4


def test_degenerate_pools_fix_the_bias_and_the_repair_scale():
    from buglab.models import _calibrate as K

    pool = noisy_pool(40, 5)
    last = (np.diff(pool.off) - 1).astype(np.int32)
    only_buggy = K.Pool(pool.vals, pool.off, np.minimum(pool.tgt, last - 1).astype(np.int32))
    cal, _ = K.fit_host(only_buggy, only_buggy)
    assert cal.no_bug_bias == 0.0 and K.NOTE_BIAS_FIXED in cal.notes and cal.converged and cal.beta != 1.0 and cal.repair_beta != 1.0
    s, _ = K.loc_stats(only_buggy, cal.beta, 0.0)
    assert abs(s[1]) <= 1e-9 * 40
    only_clean = K.Pool(pool.vals, pool.off, last)
    none = K.Pool(np.zeros(0, np.float32), np.zeros(1, np.int32), np.zeros(0, np.int32))
    cal, _ = K.fit_host(only_clean, none)
    assert cal.no_bug_bias == 0.0 and cal.repair_beta == 1.0 and K.NOTE_BIAS_FIXED in cal.notes and K.NOTE_REPAIR_FIXED in cal.notes
    # not asked for: no note
    cal, _ = K.fit_host(only_clean, none, fit_bias=False, fit_repair=False)
    assert cal.notes == () and cal.no_bug_bias == 0.0 and cal.repair_beta == 1.0


def test_an_optimum_outside_the_box_is_clamped_and_not_converged():
    """Every target is its segment's most probable entry by a small margin: the loss falls for ever as beta grows."""
    from buglab.models import _calibrate as K

    rng = np.random.default_rng(8)
    vals, tgt, lens = [], [], []
    for s in range(30):
        k = int(rng.integers(3, 8))
        x = rng.uniform(-0.02, 0.0, k)
        y = k - 1 if s % 2 else int(rng.integers(0, k - 1))
        x[y] = 0.01
        vals.append(_log_softmax(x).astype(np.float32)), tgt.append(y), lens.append(k)
    off = np.zeros(31, np.int32)
    np.cumsum(lens, out=off[1:])
    pool = K.Pool(np.concatenate(vals), off, np.asarray(tgt, np.int32))
    cal, details = K.fit_host(pool, pool)
    assert cal.beta == 64.0 and cal.repair_beta == 64.0 and not cal.converged
    assert K.BIAS_BOX[0] <= cal.no_bug_bias <= K.BIAS_BOX[1]
    assert any("beta clamped" in n for n in cal.notes) and details["localization"]["iterations"] < 50
    # held at the box, the loss still falls towards the outside; the bias, which is free, is at ITS optimum
    s, _ = K.loc_stats(pool, cal.beta, cal.no_bug_bias)
    assert s[1] < 0 and abs(s[2]) <= 1e-9 * 30


def test_expected_calibration_error():
    from buglab.models._calibrate import expected_calibration_error

    conf = np.array([0.95, 0.95, 0.95, 0.95, 0.55, 0.55, 1.0, 0.0])
    ok = np.array([1, 1, 1, 0, 1, 0, 1, 0], bool)
    ece, bins = expected_calibration_error(conf, ok, 10)
    # bins [0.9, 1.0]: 5 samples, accuracy 0.8, confidence 0.96; [0.5, 0.6): 2, 0.5 vs 0.55; [0, 0.1): 1, 0 vs 0
    assert ece == pytest.approx((5 * 0.16 + 2 * 0.05 + 0) / 8, abs=1e-15) and [b["count"] for b in bins] == [1, 2, 5]
    assert expected_calibration_error(np.zeros(0), np.zeros(0, bool))[0] == 0.0


# ---- the model side -------------------------------------------------------------------------------------------------------
def _model(family, data):
    from buglab.models.modelregistry import load_model

    spec = dict(SEQ_SPEC, modelName=family) if family.startswith("seq") else {"modelName": family, "hidden_state_size": 32, "dropout_rate": 0.1}
    model = load_model(spec, Path("/tmp/_bl_calibrate_host.pkl.gz"))[0]
    model.compute_metadata(copy.deepcopy(data))
    return model


def _data(family, n, seed):
    from buglab.data.synthetic import make_buglab_dataset, make_buglab_seq_dataset

    return make_buglab_seq_dataset(n, seed=seed) if family.startswith("seq") else make_buglab_dataset(n, seed=seed)


def _predict_minibatch(model, graphs):
    with model._tensorize_all_location_rewrites():
        samples = [model.tensorize(g) for g in graphs]
        assert all(s is not None for s in samples)
        return model._finalize_prediction_minibatch({"samples": samples}, "cpu")


def _random_parts(mb, seed):
    """Log-probabilities of the right sizes, normalised as the model normalises: per sample, per repair group."""
    rng = np.random.default_rng(seed)
    layout = mb["prediction_layout"]
    B = layout.num_samples
    flat = rng.standard_normal(layout.flat_size)
    cptr = mb["graph_data"]["candidate_ptr"].numpy().astype(np.int64)
    C = int(cptr[-1])
    for b in range(B):
        at = np.concatenate([np.arange(cptr[b], cptr[b + 1]), [C + b]])
        flat[at] = _log_softmax(flat[at])
    gptr, gitems = mb["repair_group_ptr"].numpy(), mb["repair_group_items"].numpy()
    for g in range(gptr.shape[0] - 1):
        at = C + B + gitems[gptr[g]:gptr[g + 1]].astype(np.int64)
        flat[at] = _log_softmax(flat[at])
    flat = flat.astype(np.float32)
    sizes = [C + B] + [int(mb[k].shape[0]) for k in ("rewrite_to_location_group", "candidate_symbol_to_location_group",
                                                      "swapped_pair_to_call_location_group")]
    assert sum(sizes) == layout.flat_size
    loc, text, var, swap = (torch.from_numpy(p.copy()) for p in np.split(flat, np.cumsum(sizes)[:-1]))
    return flat, (loc, text, var, swap)


@pytest.mark.parametrize("family", ["gnn-mlp", "seq-great"])
def test_pool_indices_and_calibrated_unbatching_on_the_cpu(family):
    """The pool's location segments list every flat entry once; its repair groups are the groups of the collated CSR the model's
    log-softmax runs over; and `_iter_per_sample_results` of a model that carries a calibration yields the twin's values."""
    from buglab.controllers._batching import selfsup_indices
    from buglab.models import _calibrate as K

    graphs = _data(family, 9, seed=12)
    model = _model(family, graphs)
    mb = _predict_minibatch(model, graphs)
    assert "confidence_calibration" not in mb
    layout, B = mb["prediction_layout"], len(graphs)
    ix = K.calibration_indices(layout, graphs, selfsup_indices(layout, graphs).tgt_loc)
    cptr = mb["graph_data"]["candidate_ptr"].numpy().astype(np.int64)
    C = int(cptr[-1])
    assert sorted(ix.loc_gather.tolist()) == list(range(C + B)) and ix.loc_len.tolist() == (np.diff(cptr) + 1).tolist()
    gptr, gitems = mb["repair_group_ptr"].numpy(), mb["repair_group_items"].numpy()
    group_of = {}
    for g in range(gptr.shape[0] - 1):
        members = frozenset((C + B + gitems[gptr[g]:gptr[g + 1]].astype(np.int64)).tolist())
        group_of.update({j: members for j in members})
    pos, buggy = 0, 0
    for b, point in enumerate(graphs):
        seg = ix.loc_gather[layout.loc_off[b]:layout.loc_off[b + 1]]
        assert seg[-1] == C + b and seg[:-1].tolist() == list(range(cptr[b], cptr[b + 1]))
        target = point["target_fix_action_idx"]
        if target is None:
            assert ix.loc_tgt[b] == ix.loc_len[b] - 1
            continue
        n = int(ix.rw_len[buggy])
        members = ix.rw_gather[pos:pos + n].tolist()
        want = int(layout.rw_idx[layout.rw_off[b] + target])
        assert members[ix.rw_tgt[buggy]] == want and frozenset(members) == group_of[want]
        pos, buggy = pos + n, buggy + 1
    assert buggy == ix.rw_len.shape[0] > 0 and pos == ix.rw_gather.shape[0]

    flat, parts = _random_parts(mb, seed=2)
    ids = torch.cat([mb["graph_data"]["reference_node_graph_idx"]["candidate_nodes"].long(), torch.arange(B)])
    kwargs = {"node_mappings": mb["node_mappings"]} if family.startswith("seq") else {}
    unbatch = lambda m: [(loc, rw) for _, loc, rw in model._iter_per_sample_results(m, ids, parts[0], parts[3], B, graphs, parts[1], parts[2],
                                                                                       **kwargs)]
    plain = unbatch(mb)
    cal = K.ConfidenceCalibration(beta=0.4, no_bug_bias=-1.5, repair_beta=2.25)
    model.confidence_calibration = cal
    mb_cal = _predict_minibatch(model, graphs)
    assert mb_cal["confidence_calibration"] == cal
    got = unbatch(mb_cal)
    want_flat = flat.copy()
    K.apply_host(want_flat, cptr, B, gptr, gitems, cal)
    assert not np.array_equal(want_flat, flat)
    model.confidence_calibration = None
    for b, ((loc, rw), (loc0, rw0)) in enumerate(zip(got, plain)):
        assert list(loc) == list(loc0) and len(rw) == len(rw0)
        assert list(loc.values()) == want_flat[layout.loc_idx[layout.loc_off[b]:layout.loc_off[b + 1]]].tolist()
        assert rw == want_flat[layout.rw_idx[layout.rw_off[b]:layout.rw_off[b + 1]]].tolist()
        assert sum(np.exp(v) for v in want_flat[ix.loc_gather[layout.loc_off[b]:layout.loc_off[b + 1]]].astype(np.float64)) == pytest.approx(1.0, abs=1e-5)
    # the identity launches nothing and changes nothing
    model.confidence_calibration = K.ConfidenceCalibration()
    assert unbatch(_predict_minibatch(model, graphs)) == plain


def test_checkpoint_round_trip_with_and_without_the_field(tmp_path):
    from buglab.models._calibrate import ConfidenceCalibration
    from buglab.runtime.neuralmodel import AbstractNeuralModel

    graphs = _data("gnn-mlp", 6, seed=3)
    model = _model("gnn-mlp", graphs)
    nn_ = torch.nn.Linear(2, 2)  # the checkpoint format is (model, module); the module is not what this is about
    assert "_confidence_calibration" not in vars(model) and model.confidence_calibration is None
    model.save(tmp_path / "plain.pkl.gz", nn_)
    plain, _ = AbstractNeuralModel.restore_model(tmp_path / "plain.pkl.gz", "cpu")
    assert "_confidence_calibration" not in vars(plain) and plain.confidence_calibration is None  # as a checkpoint from before
    cal = ConfidenceCalibration(0.75, -0.5, 1.5, False, ("a note",))
    model.confidence_calibration = cal
    model.save(tmp_path / "cal.pkl.gz", nn_)
    restored, _ = AbstractNeuralModel.restore_model(tmp_path / "cal.pkl.gz", "cpu")
    assert restored.confidence_calibration == cal and isinstance(restored.confidence_calibration, ConfidenceCalibration)
    assert pickle.loads(pickle.dumps(cal)) == cal and not cal.is_identity and ConfidenceCalibration().is_identity


def test_cli_help_and_arguments(capsys):
    from buglab.models import calibrate

    with pytest.raises(SystemExit) as e:
        calibrate.parse_args(["--help"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    for word in ("MODEL_FILENAME", "VALID_DATA_PATH", "OUT_MODEL_FILENAME", "--limit-num-elements", "--sequential", "--no-bias", "--no-repair",
                 "--num-bins", "--report-json", "BEYOND THE REFERENCE"):
        assert word in text, word
    ns = calibrate.parse_args(["m.pkl.gz", "valid", "out.pkl.gz", "--no-bias", "--num-bins", "10", "--limit-num-elements", "500"])
    assert (ns.no_bias, ns.no_repair, ns.num_bins, ns.limit_num_elements, ns.sequential, ns.report_json) == (True, False, 10, 500, False, None)
    assert calibrate.parse_args(["a", "b", "c"]).num_bins == 15


def test_ensembles_are_refused():
    from buglab.models.calibrate import calibrate_model
    from buglab.models.ensemble.wrapper import EnsembleWrapper

    graphs = _data("gnn-mlp", 4, seed=3)
    ensemble = EnsembleWrapper([_model("gnn-mlp", graphs)], "avg")
    with pytest.raises(TypeError, match=r"calibrate_model runs on a single detector / selector model; ensembles \(EnsembleWrapper\) are not "
                                        r"supported here\."):
        calibrate_model(ensemble, None, graphs, "cpu")


def test_entry_points_check_their_arguments_before_the_first_hip_call():
    from buglab.models import hip_ops

    lib = hip_ops.load_library()
    assert {"bl_conf_loc_stats", "bl_conf_group_stats", "bl_conf_apply"} <= set(hip_ops.EXPORTED_SYMBOLS)
    f = (ctypes.c_float * 8)()
    i = (ctypes.c_int32 * 8)()
    d = (ctypes.c_double * 64)()
    P = lambda a: ctypes.cast(a, ctypes.c_void_p)
    err = lambda: lib.bl_last_error().decode()
    assert lib.bl_conf_loc_stats(P(f), 8, P(i), P(i), 2, 0.0, 0.0, P(d), P(d), None) == -1 and "beta" in err()
    assert lib.bl_conf_loc_stats(P(f), 8, P(i), P(i), 2, 1.0, float("nan"), P(d), P(d), None) == -1 and "bias" in err()
    assert lib.bl_conf_loc_stats(P(f), 8, P(i), P(i), 2, float("inf"), 0.0, P(d), P(d), None) == -1
    assert lib.bl_conf_loc_stats(P(f), 8, P(i), P(i), 2, 1.0, 0.0, P(d), None, None) == -1 and "null out" in err()
    assert lib.bl_conf_loc_stats(P(f), 8, None, P(i), 2, 1.0, 0.0, P(d), P(d), None) == -1 and "null" in err()
    assert lib.bl_conf_loc_stats(P(f), 8, P(i), P(i), -1, 1.0, 0.0, P(d), P(d), None) == -1 and "negative" in err()
    assert lib.bl_conf_loc_stats(P(f), 1 << 31, P(i), P(i), 2, 1.0, 0.0, P(d), P(d), None) == -2 and "int32" in err()
    assert lib.bl_conf_group_stats(P(f), 8, P(i), P(i), 2, -1.0, P(d), P(d), None) == -1 and "bl_conf_group_stats" in err()
    assert lib.bl_conf_group_stats(None, 8, P(i), P(i), 2, 1.0, P(d), P(d), None) == -1 and "null vals" in err()
    ok = (P(f), 8, P(i), 2, 3, P(i), P(i), 1, 3, 5, 1.0, 0.0, 1.0, None)
    bad = lambda **kw: lib.bl_conf_apply(*[kw.get(k, v) for k, v in zip(
        ("flat", "n_flat", "cptr", "B", "C", "gptr", "gitems", "G", "n_items", "item_base", "beta", "bias", "rbeta", "stream"), ok)])
    assert bad(beta=0.0) == -1 and "beta" in err()
    assert bad(rbeta=float("nan")) == -1 and bad(bias=float("inf")) == -1
    assert bad(C=7) == -1 and "do not fit" in err()          # 7 candidates + 2 NO_BUG entries in 8 values
    assert bad(item_base=6) == -1 and "do not fit" in err()  # items 6 .. 9 in 8 values
    assert bad(flat=None) == -1 and bad(cptr=None) == -1 and bad(gptr=None) == -1 and bad(gitems=None) == -1 and "null" in err()
    assert bad(B=-1) == -1 and bad(n_flat=1 << 31) == -2
    assert bad(B=0, G=0, flat=None, cptr=None, gptr=None, gitems=None) == 0  # nothing to do
