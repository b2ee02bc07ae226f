"""CPU: the paired bootstrap comparison's host side (buglab/models/_compare.py, buglab/models/compare.py) -- the draw contract,
the uniformity of the draws, the counts and metrics against `ColumnarEvaluationReport`, the bootstrap's standard errors against
theory, the paired logic, McNemar's exact test, the refusals, the C entry point's argument checks and the CLI's arguments.

Bounds.  Uniformity: the chi-square statistic of the index counts over n cells has mean n - 1 and standard deviation
sqrt(2 (n - 1)); five of those.  Standard errors: the relative standard deviation of a standard deviation estimated from R
replicates is about 1 / sqrt(2 R) (1.6 % at R = 2000, 1.1 % at R = 4000); five of those: 8 % and 6 %."""
import ctypes
import itertools
import math

import numpy as np
import pytest

from buglab.models import _compare as C

MASK = (1 << 64) - 1


def _mix_int(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def _draw_int(seed, r, n):
    """the contract in Python integers"""
    base = _mix_int((seed * 0x9E3779B97F4A7C15 + 0x9E3779B97F4A7C15) & MASK)
    return [((_mix_int((r * n + j + base) & MASK) >> 32) * n) >> 32 for j in range(n)]


# ------------------------------------------------------------------------------------------------------------------------------
def test_draw_contract_pins_and_cutting():
    assert C.draw_indices(0, 2, 10).tolist() == [[2, 9, 6, 4, 2, 1, 5, 5, 5, 3], [3, 6, 3, 2, 2, 0, 3, 0, 2, 2]]
    whole = C.draw_indices(3, 64, 257)
    assert whole.shape == (64, 257) and whole.dtype == np.int64
    assert np.array_equal(whole, np.concatenate([C.draw_indices(3, np.arange(0, 32), 257), C.draw_indices(3, np.arange(32, 64), 257)]))
    other = C.draw_indices(4, 64, 257)
    assert (whole != other).mean() > 0.9
    for seed, r, n in ((0, 0, 10), (7, 5, 33), (2 ** 64 - 1, 2 ** 40, 1000), (123, 2 ** 62 + 17, 999)):  # the last: r * n wraps
        assert C.draw_indices(seed, [r], n)[0].tolist() == _draw_int(seed, r, n)


def test_draws_near_a_32_bit_boundary_of_the_counter_stay_in_range():
    n = 1000
    at = 2 ** 33 // n
    reps = np.arange(at - 3, at + 4)
    d = C.draw_indices(0, reps, n)
    assert d.min() >= 0 and d.max() < n
    assert d[3].tolist() == _draw_int(0, at, n)
    assert len({tuple(row) for row in d.tolist()}) == len(reps)


@pytest.mark.parametrize("n,R", [(1000, 2000), (5000, 2000), (257, 4000)])
def test_draws_are_uniform(n, R):
    counts = np.zeros(n, np.int64)
    for lo in range(0, R, 500):
        counts += np.bincount(C.draw_indices(0, np.arange(lo, min(R, lo + 500)), n).ravel(), minlength=n)
    assert counts.sum() == n * R
    chi2 = float(((counts - R) ** 2).sum()) / R
    z = (chi2 - (n - 1)) / math.sqrt(2 * (n - 1))
    print(f"\n[compare] chi-square of the index counts, n {n} R {R}: {z:+.2f} standard deviations")
    assert abs(z) <= 5


# ------------------------------------------------------------------------------------------------------------------------------
# (has_bug, warned, location_correct, repair_given_location, repaired): every combination `judge_sample` can emit
JUDGE_COMBINATIONS = [(0, 0, 1, -1, 1), (0, 1, 0, -1, 0), (1, 0, 0, 0, 0), (1, 0, 0, 1, 0), (1, 1, 0, 0, 0), (1, 1, 0, 1, 0), (1, 1, 1, 0, 0),
                      (1, 1, 1, 1, 1)]


def _columnar(rows, scout, names):
    from buglab.models.evaluate import ColumnarEvaluationReport

    rows = np.asarray(rows)
    return ColumnarEvaluationReport(np.zeros(rows.shape[0]), rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3], rows[:, 4], scout, names)


def _synthetic(seed, n=400, names=("NoBug", "swap", "absent", "literal", "varmisuse")):
    rng = np.random.default_rng(seed)
    pick = np.r_[np.arange(len(JUDGE_COMBINATIONS)), rng.integers(0, len(JUDGE_COMBINATIONS), size=n - len(JUDGE_COMBINATIONS))]
    rows = np.array(JUDGE_COMBINATIONS)[pick]
    kinds = np.array([i for i, s in enumerate(names) if s not in ("NoBug", "absent")])
    scout = np.where(rows[:, 0] == 1, kinds[rng.integers(0, len(kinds), size=n)], 0)
    return _columnar(rows, scout, list(names))


def _same(a, b):
    return a == b or (a != a and b != b)


def test_identity_replicate_is_the_evaluation_report():
    reports = [_synthetic(1), None]
    rows = np.array(JUDGE_COMBINATIONS)
    # the second model: other verdicts on the same samples (has_bug and scout are the samples')
    flip = np.random.default_rng(2).integers(0, 2, size=reports[0].has_bug.shape[0]).astype(bool)
    alt = np.where(reports[0].has_bug[:, None], rows[np.where(flip, 7, 2)], rows[np.where(flip, 0, 1)])
    reports[1] = _columnar(alt, reports[0].scout, reports[0].scout_names)
    packed, K, names = C.pack_outcomes(reports)
    assert K == 5 and names == reports[0].scout_names and packed.dtype == np.uint32
    n = packed.shape[0]
    counts = C.count_words(packed[None, :], 2, K)
    assert counts.shape == (1, C.num_columns(2, K)) == (1, 5 + 2 * 14) and counts.dtype == np.int32
    metrics = C.metrics_from_counts(counts, n, 2, K)
    assert list(metrics) == C.metric_names(K) and all(v.shape == (1, 2) and v.dtype == np.float64 for v in metrics.values())
    for m, report in enumerate(reports):
        s, per = report.summary(), report.per_scout()
        assert 0 < s["num_buggy_samples"] < s["num_samples"] == n
        for name in C.RATIO_METRICS:
            assert metrics[name][0, m] == s[name], (name, m)  # bit for bit
        for k, scout in enumerate(names):
            got = metrics[f"localization_accuracy[{k}]"][0, m]
            if scout in per["localization"]:
                ok, total = per["localization"][scout]
                assert got == ok / total
            else:
                assert scout == "absent" and got != got
            if k:
                got = metrics[f"repair_accuracy_given_location[{k}]"][0, m]
                if scout in per["repair"]:
                    ok, total = per["repair"][scout]
                    assert got == ok / total
                else:
                    assert scout == "absent" and got != got
    assert (counts[0, [5 + 4 + 5, 5 + 14 + 4 + 5]] == 0).all()  # rep_ok[0] of both models
    # a report without buggy (or without correct) samples: the ratios over them are NaN, as in summary()
    clean = _columnar(np.array(JUDGE_COMBINATIONS[:2] * 3), np.zeros(6, np.int64), ["NoBug"])
    p, K1, _ = C.pack_outcomes([clean])
    got, want = C.metrics_from_counts(C.count_words(p[None, :], 1, K1), 6, 1, K1), clean.summary()
    assert all(_same(got[name][0, 0], want[name]) for name in C.RATIO_METRICS) and got["repair_accuracy"][0, 0] != got["repair_accuracy"][0, 0]


def test_twin_counts_are_the_counts_of_the_drawn_words_and_cut_anywhere():
    rng = np.random.default_rng(5)
    packed = rng.integers(0, 2 ** 32, size=300, dtype=np.uint64).astype(np.uint32)  # scout ids up to 255: beyond K too
    whole = C.bootstrap_counts_host(packed, 3, 7, 11, 0, 40)
    assert np.array_equal(whole, np.concatenate([C.bootstrap_counts_host(packed, 3, 7, 11, 0, 15), C.bootstrap_counts_host(packed, 3, 7, 11, 15, 25)]))
    draws = C.draw_indices(11, 40, 300)
    for r in (0, 39):
        w = packed[draws[r]]
        scout = w & 0xFF
        assert whole[r, :7].tolist() == [int((scout == k).sum()) for k in range(7)]
        at = 7 + 2 * 18
        flag = lambda b: (w >> np.uint32(8 + 4 * 2 + b)) & 1 != 0
        assert whole[r, at:at + 4].tolist() == [int(flag(3).sum()), int((flag(3) & (scout != 0)).sum()), int((flag(0) & (scout != 0)).sum()),
                                                int((~flag(0) & (scout == 0)).sum())]
        assert whole[r, at + 4:at + 11].tolist() == [int((flag(1) & (scout == k)).sum()) for k in range(7)]
        assert whole[r, at + 11:at + 18].tolist() == [0] + [int((flag(2) & (scout == k)).sum()) for k in range(1, 7)]


# ------------------------------------------------------------------------------------------------------------------------------
def _from_repaired(*columns):
    """one report per 0/1 column: every sample buggy, `repaired` (and with it accuracy) = the column"""
    n = len(columns[0])
    return [_columnar(np.stack([np.ones(n, int), np.ones(n, int), np.asarray(c), np.asarray(c), np.asarray(c)], axis=1), np.ones(n, np.int64),
                      ["NoBug", "swap"]) for c in columns]


def _compare(reports, **kw):
    from buglab.models.compare import compare_reports

    return compare_reports(reports, host_bootstrap=True, **kw)


def test_bootstrap_standard_error_matches_theory():
    rng = np.random.default_rng(0)
    col = (rng.uniform(size=1000) < 0.3).astype(int)
    p = col.mean()
    report = _compare(_from_repaired(col), num_replicates=2000, seed=0)
    iv = report.metrics["accuracy"][0]
    ratio = iv.se / math.sqrt(p * (1 - p) / 1000)
    print(f"\n[compare] bootstrap se / sqrt(p (1 - p) / n): {ratio:.4f}")
    assert iv.point == p and iv.num_undefined == 0 and iv.low < p < iv.high
    assert abs(ratio - 1) <= 0.08
    assert abs((iv.high - iv.low) / (2 * 1.959964 * iv.se) - 1) <= 0.1  # a 95 % percentile interval of a near-normal statistic

    a = (rng.uniform(size=4000) < 0.6).astype(int)
    b = np.where(rng.uniform(size=4000) < 0.8, a, (rng.uniform(size=4000) < 0.65).astype(int))  # agrees with a on 80 % and more
    report = _compare(_from_repaired(a, b), num_replicates=4000, seed=1)
    d = report.deltas["accuracy"][1]
    ratio = d.se / (np.std(b - a) / math.sqrt(4000))
    print(f"[compare] paired: bootstrap se of the difference / (std(b - a) / sqrt(n)): {ratio:.4f}")
    assert d.point == b.mean() - a.mean()
    assert abs(ratio - 1) <= 0.06
    # pairing is what makes the difference sharp: far below the two models' own spreads combined
    assert d.se < 0.75 * math.hypot(report.metrics["accuracy"][0].se, report.metrics["accuracy"][1].se)


def test_paired_logic():
    rng = np.random.default_rng(3)
    base = (rng.uniform(size=2000) < 0.5).astype(int)
    same = _compare(_from_repaired(base, base.copy()), num_replicates=300)
    for name, d in same.deltas.items():
        p = same.p_values[name][1]
        if d[1].num_undefined == 300:  # a ratio over correct code, of which there is none
            assert p != p, name
        else:
            assert (d[1].point, d[1].low, d[1].high, d[1].num_undefined) == (0.0, 0.0, 0.0, 0) and p == 1.0, name
    assert same.deltas["accuracy"][1] == C.Interval(0.0, 0.0, 0.0, 0.0, 0) and same.p_values["accuracy"][1] == 1.0
    assert same.mcnemar[1] == {"baseline_only": 0, "model_only": 0, "p": 1.0}

    better = base.copy()
    better[np.flatnonzero(base == 0)[:40]] = 1  # right on a strict superset: 40 discordant samples
    R = 500
    up = _compare(_from_repaired(base, better), num_replicates=R, seed=9)
    assert up.p_values["accuracy"][1] == 2 / (R + 1)
    assert up.deltas["accuracy"][1].point == better.mean() - base.mean() and up.deltas["accuracy"][1].low > 0
    assert up.mcnemar[1] == {"baseline_only": 0, "model_only": 40, "p": C.mcnemar_exact(0, 40)}
    down = _compare(_from_repaired(better, base), num_replicates=R, seed=9)
    u, d = up.deltas["accuracy"][1], down.deltas["accuracy"][1]
    assert d.point == -u.point and down.p_values["accuracy"][1] == up.p_values["accuracy"][1]
    assert d.se == pytest.approx(u.se, rel=1e-12) and d.low == pytest.approx(-u.high, abs=1e-12) and d.high == pytest.approx(-u.low, abs=1e-12)
    assert down.metrics["accuracy"][0] == up.metrics["accuracy"][1]  # the same draws, whoever is named first
    # one model: intervals only
    alone = _compare(_from_repaired(base), num_replicates=50)
    assert alone.deltas["accuracy"] == {} and alone.mcnemar == {} and len(alone.metrics["accuracy"]) == 1
    assert "NaN" in alone.to_json() and alone.metrics["no_bug_precision"][0].num_undefined == 50  # no correct code at all
    assert alone.format().startswith("Paired bootstrap over 2000 samples, 50 replicates")


def test_mcnemar_exact():
    assert C.mcnemar_exact(0, 0) == 1.0 and C.mcnemar_exact(5, 5) == 1.0 and C.mcnemar_exact(0, 10) == 2 / 1024
    for b, c in itertools.product(range(13), repeat=2):
        if b + c > 12:
            continue
        t = b + c
        brute = sum(1 for bits in itertools.product((0, 1), repeat=t) if sum(bits) <= min(b, c)) if t else 0
        want = min(1.0, 2 * brute / 2 ** t) if t else 1.0
        assert C.mcnemar_exact(b, c) == C.mcnemar_exact(c, b) == want, (b, c)
    assert 0 < C.mcnemar_exact(400, 600) < 1e-9  # integers: no overflow, no underflow to 0


def test_refusals():
    one = _from_repaired(np.ones(10, int))[0]
    with pytest.raises(ValueError, match="1 to 6"):
        _compare([one] * 7, num_replicates=10)
    many = _columnar(np.array([JUDGE_COMBINATIONS[7]] * 70), np.arange(1, 71), ["NoBug"] + [f"s{i}" for i in range(70)])
    with pytest.raises(ValueError, match="at most 64"):
        _compare([many], num_replicates=10)
    with pytest.raises(ValueError, match="not over the same samples"):
        _compare([one, _from_repaired(np.ones(11, int))[0]], num_replicates=10)
    other = _columnar(np.array([JUDGE_COMBINATIONS[0]] * 10), np.zeros(10, np.int64), ["NoBug", "swap"])  # ten correct samples instead
    with pytest.raises(ValueError, match="not over the same samples"):
        _compare([one, other], num_replicates=10)
    with pytest.raises(ValueError, match="paired set is empty"):
        _compare(_from_repaired(np.zeros(0, int)), num_replicates=10)
    # pairing: the intersection of what every model kept, and an empty one is refused
    from buglab.models.compare import paired_reports

    a, b = _synthetic(4, n=20), _synthetic(4, n=20)
    keep_a, keep_b = [0, 1, 2, 5, 7, 9, 19], [19, 9, 5, 3, 1]
    rows = lambda r, pos: _columnar(np.stack([r.has_bug, r.warned, r.location_correct, r.repair_given_location, r.repaired], axis=1)[pos],
                                    r.scout[pos], r.scout_names)
    paired, kept, dropped = paired_reports([(rows(a, keep_a), keep_a), (rows(b, keep_b), keep_b)], 20)
    assert kept.tolist() == [1, 5, 9, 19] and dropped == [13, 15]
    assert all(np.array_equal(p.scout, a.scout[kept]) and np.array_equal(p.repaired, a.repaired[kept]) for p in paired)
    with pytest.raises(ValueError, match="paired set is empty"):
        paired_reports([(rows(a, [0, 1]), [0, 1]), (rows(b, [2]), [2])], 20)


# ------------------------------------------------------------------------------------------------------------------------------
def test_entry_point_reports_argument_errors_without_a_gpu():
    from buglab.models import hip_ops

    lib = hip_ops.load_library()
    words = (ctypes.c_uint32 * 16)()
    out = (ctypes.c_int32 * 256)()
    p, o = ctypes.cast(words, ctypes.c_void_p), ctypes.cast(out, ctypes.c_void_p)
    call = lambda packed=p, n=16, M=2, K=3, seed=0, r0=0, R=4, out=o: lib.bl_bootstrap_counts(packed, n, M, K, seed, r0, R, out, None)
    BL_EINVAL, BL_ERANGE = -1, -2
    for kw, word in (({"packed": None}, b"null"), ({"out": None}, b"null"), ({"n": 0}, b"n must be"), ({"R": -1}, b"negative"),
                     ({"r0": -1}, b"negative"), ({"M": 0}, b"models"), ({"M": 7}, b"models"), ({"K": 0}, b"scouts"), ({"K": 65}, b"scouts")):
        assert call(**kw) == BL_EINVAL and word in lib.bl_last_error(), kw
    assert call(n=2 ** 31) == BL_ERANGE and b"int32" in lib.bl_last_error()
    assert call(R=0) == 0  # a no-op: nothing is launched
    assert hip_ops.BOOTSTRAP_MAX_MODELS == C.MAX_MODELS == 6 and hip_ops.BOOTSTRAP_MAX_SCOUTS == C.MAX_SCOUTS == 64


def test_cli_arguments():
    from buglab.models import compare

    a = compare.parse_args(["data", "m0.pkl.gz"])
    assert (a.DATA, a.MODEL, a.num_replicates, a.seed, a.confidence) == ("data", ["m0.pkl.gz"], 10000, 0, 0.95)
    assert (a.limit_num_elements, a.sequential, a.assume_buggy, a.eval_only_no_bug, a.host_bootstrap, a.report_json) == (None, False, False, False, False, None)
    a = compare.parse_args(["data", "a", "b", "c", "--num-replicates", "200", "--seed", "5", "--confidence", "0.9", "--limit-num-elements", "7",
                            "--sequential", "--assume-buggy", "--eval-only-no-bug", "--host-bootstrap", "--report-json", "r.json"])
    assert (a.MODEL, a.num_replicates, a.seed, a.confidence, a.limit_num_elements) == (["a", "b", "c"], 200, 5, 0.9, 7)
    assert a.sequential and a.assume_buggy and a.eval_only_no_bug and a.host_bootstrap and a.report_json == "r.json"
    assert compare.REPLICATES_PER_CALL == 4096
