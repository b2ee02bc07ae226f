"""CPU: FDR-controlled warnings without a GPU -- the NumPy twin of csrc/bl_fdr.hip (buglab/models/_fdr.py) against the plain
loops of tests/fdr_cases.py bit for bit, the flagged set against a sort-based textbook Benjamini-Hochberg, q-values against
flags, the guarantee itself on simulated scans, and how the reference travels with a checkpoint (buglab/models/fdr.py).

No tolerance anywhere but in the guarantee, whose bound is the theorem's: E[FDP] <= q * (share of clean samples)."""
import json
import math
import zlib
from fractions import Fraction

import numpy as np
import pytest

from tests import fdr_cases as C
from tests.test_visualize_host import _minibatch, _model, _unbatched_by_the_model


# ------------------------------------------------------------------------------------------------ the twin
@pytest.mark.parametrize("n_ref", [1, 2, 1023])
@pytest.mark.parametrize("B", [1, 50])
def test_counts_twin_equals_the_loops(B, n_ref):
    from buglab.models._fdr import counts_host

    src, idx, ref = C.counts_case(B, n_ref, seed=0)
    got = counts_host(src, idx, ref)
    C.assert_equal_bits(got, C.restate_counts(src, idx, ref), (B, n_ref))
    assert got[0].dtype == np.float32 and got[1].dtype == np.int32 and 0 <= got[1].min() and got[1].max() <= n_ref


def test_counts_rules_stated_once():
    """the `<=` boundary, NaN, the infinities and the two zeros as literal numbers"""
    from buglab.models._fdr import counts_host

    ref = np.array([-np.inf, -1.0, -0.0, 0.0, 0.0, 2.0, np.inf], np.float32)
    src = np.array([-np.inf, -2.0, -1.0, -0.5, -0.0, 0.0, 1.0, 2.0, 3.0, np.inf, np.nan], np.float32)
    score, count = counts_host(src, np.arange(src.shape[0]), ref)
    assert count.tolist() == [1, 1, 2, 2, 5, 5, 5, 6, 6, 7, 7]  # a tie counts every equal entry; -0.0 == 0.0; NaN: n
    assert score.tobytes() == src.tobytes()
    score, count = counts_host(src, np.array([-1, src.shape[0], 2], np.int32), ref)  # outside src: NaN
    assert count.tolist() == [7, 7, 2] and score[:2].view(np.uint32).tolist() == [0x7FC00000] * 2
    payload = np.array([0x7FC0BEEF], np.uint32).view(np.float32)  # a NaN of src keeps its bits
    assert counts_host(payload, [0], ref)[0].view(np.uint32).tolist() == [0x7FC0BEEF]
    with pytest.raises(ValueError):
        counts_host(src, [0], np.zeros(0, np.float32))


BH_CASES = [(N, n_ref, kind, q) for N in (1, 255, 1000) for n_ref in (1, 2, 1023) for kind, q in
            (("mixed", 0.1), ("mixed", 0.01), ("mixed", 1.0), ("equal", 0.1), ("top", 0.1), ("top", 1.0), ("bottom", 0.1), ("bottom", 1.0))]


@pytest.mark.parametrize("N,n_ref,kind,q", BH_CASES)
def test_bh_twin_equals_the_loops_and_the_textbook(N, n_ref, kind, q):
    from buglab.models._fdr import bh_host

    count = C.bh_counts(N, n_ref, kind)
    got = bh_host(count, n_ref, q)
    C.assert_equal_bits(got, C.restate_bh(count, n_ref, q), (N, n_ref, kind, q))
    cutoff, flag, qv, R = got
    assert (flag != 0).tolist() == C.textbook_bh(count, n_ref, q).tolist()
    assert R[-1] == N and cutoff[1] == (flag != 0).sum() and ((qv > 0) & (qv <= 1)).all()
    if kind == "top":  # every p-value is 1: everything is flagged at q = 1 and nothing below it
        assert cutoff.tolist() == ([n_ref, N] if q == 1.0 else [-1, 0])
    if q == 1.0:
        assert (flag == 1).all() and cutoff[0] == n_ref
    if kind == "bottom":  # every p-value is 1 / (n + 1)
        assert (flag == 1).all() == (1.0 <= q * (n_ref + 1))


def test_bh_rules_stated_once():
    """several samples exactly at the cutoff, as literal numbers: n + 1 = 20, N = 10, q = 1/2 (exact), so c qualifies iff
    c + 1 <= R[c]"""
    from buglab.models._fdr import bh_host, p_values

    count = np.array([0, 1, 2, 2, 2, 19, 19, 19, 19, 19], np.int32)
    cutoff, flag, qv, R = bh_host(count, 19, 0.5)
    assert R.tolist() == [1, 2, 5, 5, 5] + [5] * 14 + [10]
    assert cutoff.tolist() == [4, 5]  # c = 4: 5 <= 5 holds with equality, at an empty bin; c = 5: 6 <= 5 does not
    assert flag.tolist() == [1] * 5 + [0] * 5
    assert qv.tolist() == [3 * 10 / (20 * 5)] * 5 + [1.0] * 5  # the three samples at c = 2 pull the two before them down
    assert p_values(count, 19).tolist() == [0.05, 0.1, 0.15, 0.15, 0.15, 1.0, 1.0, 1.0, 1.0, 1.0]
    assert bh_host(count, 19, 0.29)[0].tolist() == [-1, 0]  # 30 <= 0.29 * 100 fails at c = 2, 10 <= 5.8 at c = 0
    assert bh_host(count, 19, 0.3)[0].tolist() == [2, 5]  # 30 <= fl(0.3 * 100) = 30
    assert bh_host(np.array([-5, 99], np.int32), 3, 1.0)[3].tolist() == [1, 1, 1, 2]  # out of range: clamped
    for bad in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            bh_host(count, 19, bad)
    with pytest.raises(ValueError):
        bh_host(count[:0], 19, 0.5)


def test_benjamini_yekutieli_divisor():
    from buglab.models._fdr import bh_host, effective_level, harmonic

    assert harmonic(1) == 1.0 and harmonic(4) == math.fsum([1.0, 0.5, 1 / 3, 0.25])
    N, n_ref = 1000, 1023
    # against the exact rational sum: every term 1.0 / i is off by at most 2^-53 / i, so their exact sum (what fsum rounds) by at
    # most 2^-53 * 7.5 = 8.3e-16, and the two roundings add one spacing (8.9e-16) at most: two spacings
    exact = float(sum(Fraction(1, i) for i in range(1, N + 1)))
    assert abs(harmonic(N) - exact) <= 2 * np.spacing(exact)
    assert effective_level(0.1, N) == 0.1 and effective_level(0.1, N, "arbitrary") == 0.1 / harmonic(N)
    with pytest.raises(ValueError):
        effective_level(0.1, N, "positive")
    count = C.bh_counts(N, n_ref, "mixed")
    # at q / 7.5 a discovery needs (c + 1) * 1000 <= 13.7 R: of the ~200 low samples only a crowd at c = 0 passes, while at q
    # itself (102 R) the ones at 1 .. 5 pass too
    low = np.flatnonzero(count <= n_ref // 50)
    count[low[::2]], count[low[1::2]] = 0, 1 + np.arange(low[1::2].shape[0]) % 5
    level = effective_level(0.1, N, "arbitrary")
    got = bh_host(count, n_ref, level)
    C.assert_equal_bits(got, C.restate_bh(count, n_ref, level))
    plain = bh_host(count, n_ref, 0.1)
    assert 0 < got[0][1] < plain[0][1]  # the stricter level flags fewer, and still some
    assert ((got[1] != 0) <= (plain[1] != 0)).all() and got[2].tobytes() == plain[2].tobytes()  # q-values do not depend on q


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_flagged_iff_q_value_at_most_q(seed):
    """for levels strictly between two attained q-values (and below the least, and at 1)"""
    from buglab.models._fdr import bh_host

    count = C.bh_counts(500, 200, "mixed", seed)
    qv = bh_host(count, 200, 0.5)[2]
    attained = np.unique(qv)
    assert attained.shape[0] >= 3
    levels = [attained[0] / 2] + [(a + b) / 2 for a, b in zip(attained[:-1], attained[1:])] + [1.0]
    for q in levels:
        flag = bh_host(count, 200, float(q))[1] != 0
        assert flag.tolist() == (qv <= q).tolist(), q
    assert not (bh_host(count, 200, float(levels[0]))[1] != 0).any()


# ------------------------------------------------------------------------------------------------ the guarantee
SCANS = 2000


@pytest.mark.parametrize("n_ref,N,share,shift,q", [(199, 400, 0.2, 3.0, 0.1), (63, 256, 0.25, 4.0, 0.2)])
def test_the_guarantee(n_ref, N, share, shift, q):
    """E[FDP] <= q * (share of clean samples): the mean over 2000 simulated scans stays below the theorem's bound plus three
    standard errors.  Measured: 0.0709 +- 0.0011 against 0.080, and 0.1322 +- 0.0018 against 0.150."""
    fdp, power = C.simulate_fdp(np.random.default_rng(0), n_ref, N, share, shift, q, SCANS)
    mean, se = fdp.mean(), fdp.std(ddof=1) / math.sqrt(SCANS)
    print(f"FDP {mean:.4f} +- {se:.4f}, bound {q * (1 - share):.4f}, power {power.mean():.3f}")
    assert mean <= q * (1 - share) + 3 * se
    assert power.mean() > 0.5  # the procedure is not passing by flagging nothing


@pytest.mark.parametrize("share", [0.02, 0.5])
def test_prevalence_free(share):
    """the same reference size and q at 2 % and at 50 % buggy: the bound holds at both (where a threshold fitted for a
    precision on one mix would not carry over to the other)"""
    n_ref, N, shift, q = 199, 400, 3.0, 0.1
    fdp, _ = C.simulate_fdp(np.random.default_rng(0), n_ref, N, share, shift, q, SCANS)
    mean, se = fdp.mean(), fdp.std(ddof=1) / math.sqrt(SCANS)
    print(f"share {share}: FDP {mean:.4f} +- {se:.4f}, bound {q * (1 - share):.4f}")
    assert mean <= q * (1 - share) + 3 * se


# ------------------------------------------------------------------------------------------------ the reference and the checkpoint
def test_make_null_reference():
    from buglab.models._calibrate import ConfidenceCalibration
    from buglab.models._fdr import MAX_REFERENCE, calibration_fingerprint, make_null_reference

    scores = np.array([0.5, np.nan, -1.0, 2.0, np.nan, -3.0, 7.0], np.float32)
    ref = make_null_reference(scores, 5, 4, None)  # the first five in input order, then the NaNs go
    assert ref.scores.tolist() == [-1.0, 0.5, 2.0] and ref.scores.dtype == np.float32
    assert (ref.num_kept, ref.num_dropped_nan, ref.num_skipped_buggy, ref.calibration) == (3, 2, 4, None)
    assert make_null_reference(scores, MAX_REFERENCE, 0, None).scores.tolist() == [-3.0, -1.0, 0.5, 2.0, 7.0]
    cal = ConfidenceCalibration(beta=1.25, no_bug_bias=-0.5, repair_beta=2.0)
    assert make_null_reference(scores, 7, 0, cal).calibration == (1.25, -0.5, 2.0) == calibration_fingerprint(cal)
    assert json.dumps(ref.to_dict())  # plain data
    for bad in (0, MAX_REFERENCE + 1):
        with pytest.raises(ValueError):
            make_null_reference(scores, bad, 0, None)
    with pytest.raises(ValueError, match="no score"):
        make_null_reference(np.array([np.nan], np.float32), 5, 0, None)


class _DrawnForward:
    """A real untrained gnn-mlp (its tensorise, collate and un-batching) whose forward is replaced by drawn values: this file
    runs without a GPU and the models have no CPU forward.  tests/test_fdr_gpu.py runs the real forward.  NO_BUG's
    log-probability is drawn lower for buggy samples, so a scan has something to find."""

    def __init__(self, model):
        self._model = model
        self.null_reference = None
        self.confidence_calibration = None

    def __getattr__(self, name):
        return getattr(self._model, name)

    def predict(self, data, trained_nn, device, parallelize):
        from buglab.models.basemodel import prediction_layout

        points = list(data)
        for lo in range(0, len(points), 5):
            chunk = points[lo:lo + 5]
            mb = _minibatch(self._model, chunk)
            layout = prediction_layout(mb)
            drawn = lambda rng, size: (np.round(np.log(rng.uniform(0.02, 1.0, size=size)) * 8) / 8).astype(np.float32)
            flat = drawn(np.random.default_rng(lo), layout.flat_size)
            for b, point in enumerate(chunk):  # NO_BUG's value belongs to the sample, whatever minibatch it lands in
                own = drawn(np.random.default_rng(zlib.crc32(point["graph"]["path"].encode())), 1)[0]
                flat[layout.loc_idx[layout.loc_off[b + 1] - 1]] = own - np.float32(6.0 if point["target_fix_action_idx"] is not None else 0.0)
            yield from _unbatched_by_the_model(self._model, mb, chunk, flat)


@pytest.fixture(scope="module")
def drawn():
    from buglab.data.synthetic import make_report_dataset

    clean_pool = make_report_dataset(60, seed=33)
    scanned = make_report_dataset(40, seed=34)
    model = _DrawnForward(_model("gnn-mlp", clean_pool + scanned))
    return model, clean_pool, scanned


def test_fit_skips_buggy_samples_and_truncates(drawn):
    from buglab.models import fdr as T

    model, clean_pool, _ = drawn
    num_clean = sum(p["target_fix_action_idx"] is None for p in clean_pool)
    assert 10 < num_clean < 60
    ref = T.fit_null_reference(model, None, clean_pool, "cpu", host=True, parallelize=False)
    assert model.null_reference is ref and ref.calibration is None
    assert (ref.num_kept, ref.num_dropped_nan, ref.num_skipped_buggy) == (num_clean, 0, 60 - num_clean)
    assert (np.diff(ref.scores) >= 0).all() and ref.scores.dtype == np.float32
    # the scores are the clean samples' NO_BUG log-probabilities, each once
    want = sorted(np.float32(loc[-1]) for p, loc, _ in model.predict(iter(clean_pool), None, "cpu", False) if p["target_fix_action_idx"] is None)
    assert ref.scores.tolist() == want
    # --max-reference keeps the FIRST accepted samples in input order, not the lowest scores
    short = T.fit_null_reference(model, None, clean_pool, "cpu", host=True, parallelize=False, max_reference=7)
    first = [np.float32(loc[-1]) for p, loc, _ in model.predict(iter(clean_pool), None, "cpu", False) if p["target_fix_action_idx"] is None][:7]
    assert short.num_kept == 7 and short.scores.tolist() == sorted(first) and short.num_skipped_buggy == 60 - num_clean
    with pytest.raises(ValueError):
        T.fit_null_reference(model, None, clean_pool, "cpu", host=True, max_reference=0)
    with pytest.raises(ValueError, match="no score"):
        T.fit_null_reference(model, None, [p for p in clean_pool if p["target_fix_action_idx"] is not None], "cpu", host=True)
    model.null_reference = None


def test_scan_host_path_records_and_refusals(drawn):
    from buglab.models import _fdr as F
    from buglab.models import fdr as T
    from buglab.models._calibrate import ConfidenceCalibration

    model, clean_pool, scanned = drawn
    model.null_reference = None
    with pytest.raises(LookupError, match="no null reference"):
        T.scan_with_fdr(model, None, scanned, "cpu", 0.2, host=True)
    ref = T.fit_null_reference(model, None, clean_pool, "cpu", host=True, parallelize=False)
    found = T.scan_with_fdr(model, None, scanned, "cpu", 0.2, host=True, parallelize=False, top_k=2, html=True)
    assert found.positions == list(range(40)) and found.labels == [p["target_fix_action_idx"] is not None for p in scanned]
    # the columns are the twin's on the predict values
    values = np.array([loc[-1] for _, loc, _ in model.predict(iter(scanned), None, "cpu", False)], np.float32)
    score, count = F.counts_host(values, np.arange(40), ref.scores)
    cutoff, flag, qv, _ = F.bh_host(count, ref.num_kept, 0.2)
    C.assert_equal_bits((found.score, found.count, found.q_value), (score, count, qv))
    assert found.flagged.tolist() == (flag != 0).tolist() and found.cutoff == cutoff[0] and found.num_flagged == cutoff[1]
    assert found.p_value.tolist() == [(c + 1) / (ref.num_kept + 1) for c in count.tolist()]
    assert 0 < found.num_flagged < 40 and found.q_effective == 0.2
    # records: one per sample; the flagged ones, and only they, carry suggestions (NO_BUG never among them) and are on the page
    records = found.records()
    assert [r["position"] for r in records] == list(range(40)) and len(json.loads(json.dumps(records))) == 40
    for r, c, f in zip(records, count.tolist(), found.flagged.tolist()):
        assert r["count"] == c and r["flagged"] is f and r["p_value"] == (c + 1) / (ref.num_kept + 1) and ("suggestions" in r) == f
        if f:
            assert 1 <= len(r["suggestions"]) <= 2 and all(s["kind"] == "rewrite" for s in r["suggestions"])
    assert found.html.count('<section class="snippet') == found.num_flagged
    # labelled data: the realised proportion and the power
    lab = found.summary["labelled"]
    buggy = np.array(found.labels)
    assert lab["num_labelled"] == 40 and lab["num_buggy"] == int(buggy.sum()) and lab["num_flagged"] == found.num_flagged
    assert lab["false_alarms"] == int((found.flagged & ~buggy).sum()) and lab["buggy_flagged"] == int((found.flagged & buggy).sum())
    assert lab["false_discovery_proportion"] == lab["false_alarms"] / found.num_flagged and lab["power"] == lab["buggy_flagged"] / lab["num_buggy"]
    text = F.format_summary(found.summary)
    assert "smallest attainable p-value" in text and "realised false discovery proportion" in text and f"Flagged {found.num_flagged} samples" in text
    # unlabelled data: no such block
    bare = [{k: v for k, v in p.items() if k != "target_fix_action_idx"} for p in scanned[:3]]
    assert F.realised(np.array([True, False, False]), [T._label(p) for p in bare]) is None
    # Benjamini-Yekutieli runs the same step-up at q / sum 1/i
    strict = T.scan_with_fdr(model, None, scanned, "cpu", 0.2, dependence="arbitrary", host=True, parallelize=False)
    assert strict.q_effective == 0.2 / F.harmonic(40) and strict.num_flagged <= found.num_flagged
    assert strict.flagged.tolist() == (F.bh_host(count, ref.num_kept, strict.q_effective)[1] != 0).tolist()
    # a calibration other than the one the reference was fitted under: the scores are not comparable
    model.confidence_calibration = ConfidenceCalibration(beta=2.0)
    with pytest.raises(ValueError, match="fitted under calibration"):
        T.scan_with_fdr(model, None, scanned, "cpu", 0.2, host=True)
    model.confidence_calibration = None
    for bad in (0.0, 1.5):
        with pytest.raises(ValueError):
            T.scan_with_fdr(model, None, scanned, "cpu", bad, host=True)
    with pytest.raises(ValueError, match="dependence"):
        T.scan_with_fdr(model, None, scanned, "cpu", 0.2, dependence="positive", host=True)
    model.null_reference = None


def test_ensembles_are_refused(drawn):
    from buglab.models import fdr as T
    from buglab.models.ensemble.wrapper import EnsembleWrapper

    _, clean_pool, scanned = drawn
    ensemble = EnsembleWrapper.__new__(EnsembleWrapper)  # `require_single_model` looks at the type
    with pytest.raises(TypeError, match="ensembles"):
        T.fit_null_reference(ensemble, None, clean_pool, "cpu", host=True)
    with pytest.raises(TypeError, match="ensembles"):
        T.scan_with_fdr(ensemble, None, scanned, "cpu", 0.1, host=True)


def test_checkpoint_round_trip_and_exit_status(tmp_path, capsys):
    import torch

    from buglab.data.synthetic import make_report_dataset
    from buglab.models import fdr as T
    from buglab.models._fdr import make_null_reference
    from buglab.runtime.neuralmodel import AbstractNeuralModel

    data = make_report_dataset(8, seed=35)
    model = _model("gnn-mlp", data)
    assert model.null_reference is None  # an object from before the field existed has no such attribute
    torch.manual_seed(1)
    module = model.build_neural_module()
    without = tmp_path / "plain.pkl.gz"
    model.save(without, module)
    restored, _ = AbstractNeuralModel.restore_model(without, torch.device("cpu"))
    assert restored.null_reference is None and restored.confidence_calibration is None and restored.warning_operating_point is None
    # status 2, before any data is read (the path does not exist) and before a GPU is asked for
    status = T.run(T.parse_args(["scan", str(without), str(tmp_path / "nowhere"), str(tmp_path / "out.jsonl"), "--fdr", "0.1"]))
    assert status == T.EXIT_NO_REFERENCE == 2 and "no null reference" in capsys.readouterr().err
    assert not (tmp_path / "out.jsonl").exists()
    # the reference travels with the checkpoint
    model.null_reference = make_null_reference(np.array([0.25, np.nan, -4.0, -0.5], np.float32), 4, 3, None)
    carrying = tmp_path / "reference.pkl.gz"
    model.save(carrying, module)
    restored, _ = AbstractNeuralModel.restore_model(carrying, torch.device("cpu"))
    got, want = restored.null_reference, model.null_reference
    assert got.scores.tobytes() == want.scores.tobytes() and got.scores.dtype == np.float32 and got[1:] == want[1:] == (3, 1, 3, None)
    with pytest.raises(SystemExit):
        T.parse_args(["scan", str(carrying), "data", "out"])  # --fdr is required


def test_launchers_check_before_any_hip_call():
    """host-side argument checks of hip_ops.fdr_counts / fdr_bh and of the C entry points: a bad call never reaches a kernel"""
    import ctypes

    import torch

    from buglab.models import hip_ops

    lib = hip_ops.load_library()
    assert lib.bl_fdr_bh_workspace_bytes(0) == 0 and lib.bl_fdr_bh_workspace_bytes((1 << 20) + 1) == 0
    # [R | chunk sums, chunk cutoffs | terms | chunk minima] for 1024 bins: one chunk
    assert hip_ops.fdr_bh_workspace_bytes(1023) == 4 * 1024 + 8 + 8 * 1024 + 8
    assert hip_ops.fdr_bh_workspace_bytes(1 << 20) < 13 << 20
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.bl_fdr_counts(p, 8, p, 4, p, 0, p, p, 0, 8, None) == -1 and b"at least 1" in lib.bl_last_error()
    assert lib.bl_fdr_counts(p, 8, p, 4, p, (1 << 20) + 1, p, p, 0, 8, None) == -2 and b"BL_FDR_MAX_REFERENCE" in lib.bl_last_error()
    assert lib.bl_fdr_counts(p, 8, p, 4, p, 4, p, p, 5, 8, None) == -1 and b"do not fit" in lib.bl_last_error()
    assert lib.bl_fdr_counts(p, 8, None, 4, p, 4, p, p, 0, 8, None) == -1 and b"null" in lib.bl_last_error()
    assert lib.bl_fdr_bh(p, 0, 4, 0.1, p, p, p, p, None) == -1 and b"at least 1" in lib.bl_last_error()
    for q in (0.0, 1.5, float("nan")):
        assert lib.bl_fdr_bh(p, 4, 4, q, p, p, p, p, None) == -1 and b"(0, 1]" in lib.bl_last_error()
    assert lib.bl_fdr_bh(p, 1 << 31, 4, 0.1, p, p, p, p, None) == -2 and b"int32" in lib.bl_last_error()
    assert lib.bl_fdr_bh(p, 4, 4, 0.1, None, p, p, p, None) == -1 and b"null" in lib.bl_last_error()
    assert lib.bl_fdr_bh(p, 4, 4, 0.1, ctypes.c_void_p(p.value + 4), p, p, p, None) == -1 and b"aligned" in lib.bl_last_error()
    with pytest.raises(hip_ops.HipOpsUnavailable):
        hip_ops.fdr_bh(torch.zeros(4, dtype=torch.int32), 4, 0.1)
    with pytest.raises(hip_ops.HipOpsUnavailable):
        z = torch.zeros(4)
        hip_ops.fdr_counts(z, torch.zeros(4, dtype=torch.int32), z, z, torch.zeros(4, dtype=torch.int32), 0)
