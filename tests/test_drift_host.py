"""CPU: the NumPy twin of the drift-detection kernels (buglab/models/_drift.py) against the definitions it restates, the seeds
of tests/drift_cases.py against the non-vacuity condition of the GPU p-value test, and the command line with a stub for the
embedding step.  The device side is tests/test_drift_gpu.py."""
import json

import numpy as np
import pytest

from tests import drift_cases as C


# ------------------------------------------------------------------------------------------------ subsets
def test_subsets_have_n_ones_an_identity_column_and_depend_on_the_seed_alone():
    from buglab.models._drift import subset_keys, subsets_host

    for N, n in ((257, 150), (128, 64), (4, 2), (50, 2), (50, 48)):
        a = subsets_host(N, n, 40, seed=3)
        assert a.dtype == np.uint8 and a.shape == (41, N) and set(np.unique(a)) <= {0, 1}
        assert (a.sum(axis=1) == n).all()
        assert a[0, :n].all() and not a[0, n:].any()
        assert np.array_equal(a, subsets_host(N, n, 40, seed=3))
        assert np.array_equal(a[:11], subsets_host(N, n, 10, seed=3))  # not on how many are drawn
        assert not np.array_equal(a[1:], subsets_host(N, n, 40, seed=4)[1:]) or N == 4
    # a key depends on (seed, r, i): a longer sample continues the shorter one's keys
    assert np.array_equal(subset_keys(9, 5, 100)[:60], subset_keys(9, 5, 60))
    assert len({int(k) for r in (1, 2) for k in subset_keys(9, r, 1000)}) == 2000
    with pytest.raises(ValueError):
        subsets_host(5, 4, 3, 0)
    with pytest.raises(ValueError):
        subsets_host(5, 2, 0, 0)


def test_subset_membership_frequencies_pass_a_chi_square_test():
    """every row is in a drawn subset with probability n / N: the counts over R draws against Binomial(R, n / N).  With the sum
    of the counts fixed the statistic is chi-square with N - 1 degrees of freedom; 39 of them exceed 79 once in 10^4 runs (and
    the seed is fixed)"""
    from buglab.models._drift import subsets_host

    N, n, R = 40, 15, 2000
    a = subsets_host(N, n, R, seed=123)[1:]
    p = n / N
    counts = a.sum(axis=0).astype(np.float64)
    chi2 = float(((counts - R * p) ** 2).sum() / (R * p * (1 - p)) * (N - 1) / N)
    assert 12.0 < chi2 < 79.0, chi2  # (and not suspiciously even: below 12 once in 10^4 too)
    # pairs of rows: P(both in) = n (n - 1) / (N (N - 1))
    both = float((a[:, 0] & a[:, 1]).sum())
    p2 = n * (n - 1) / (N * (N - 1))
    assert abs(both - R * p2) < 4.5 * np.sqrt(R * p2 * (1 - p2))


def test_a_forced_key_tie_goes_to_the_lower_row():
    from buglab.models._drift import subsets_host

    all_equal = lambda seed, r, N: np.full(N, 42, np.uint64)
    a = subsets_host(10, 4, 3, 0, key_fn=all_equal)
    assert (a[1:, :4] == 1).all() and not a[1:, 4:].any()
    # rows 2, 5 and 7 tie at the n-th smallest key: one smaller key, then the two lower rows of the three
    def keyed(seed, r, N):
        keys = np.arange(100, 100 + N, dtype=np.uint64)
        keys[[2, 5, 7]] = 50
        keys[9] = 1
        return keys
    assert np.flatnonzero(subsets_host(10, 3, 1, 0, key_fn=keyed)[1]).tolist() == [2, 5, 9]
    top = lambda seed, r, N: np.where(np.arange(N) % 2 == 0, np.uint64(2 ** 64 - 1), np.uint64(2 ** 63)).astype(np.uint64)
    assert np.flatnonzero(subsets_host(8, 5, 1, 0, key_fn=top)[1]).tolist() == [0, 1, 3, 5, 7]


# ------------------------------------------------------------------------------------------------ the statistic
def _dense(name):
    ref = C.reference(name)
    z = ref.z.astype(np.float64)
    sq = (z * z).sum(axis=1)
    K = np.exp(-np.maximum(sq[:, None] + sq[None, :] - 2.0 * z @ z.T, 0.0) / ref.s)
    return ref, K


@pytest.mark.parametrize("name", ["edge", "exact", "least", "exact-dup", "edge-far"])
def test_mmd2_from_the_sums_equals_the_quadratic_form(name):
    from buglab.models._drift import mmd2, witness

    case = C.CASES[name]
    ref, K = _dense(name)
    n, m = case.n, case.m
    a = ref.masks.astype(np.float64)
    w = a / n - (1.0 - a) / m                      # [R + 1, N]: the weights of the two empirical means
    direct = np.einsum("ri,ij,rj->r", w, K, w)
    assert np.abs(ref.mmd2 - direct).max() <= 1e-12
    assert (direct > -1e-12).all()                  # the biased V-statistic is not negative
    # the weights sum to zero: a constant subtracted from K changes the sums and not the statistic
    for c in (0.25, float(K.mean())):
        shifted = mmd2(ref.A - c * n * n, ref.B - c * n * (n + m), ref.S - c * (n + m) ** 2, n, m)
        assert np.abs(shifted - ref.mmd2).max() <= 1e-12
    # the witness is the difference of the two mean embeddings at a scanned row
    f = witness(ref.u0, ref.rho, n, m)
    assert np.abs(f - (K[n:, :n].mean(axis=1) - K[n:, n:].mean(axis=1))).max() <= 1e-12
    assert np.abs(ref.rho - K.sum(axis=1)).max() <= 1e-9 and abs(ref.S - K.sum()) <= 1e-9 * K.sum()


def test_identical_samples_give_zero_and_a_p_value_of_one():
    from buglab.models._drift import drift_host

    x = C.rows(C.CASES["exact"])[0]
    report = drift_host(x, x[::-1].copy(), 63, seed=1)
    assert abs(report.statistic) <= 1e-12 and report.p_value == 1.0 and not report.drift
    assert np.abs(report.witness).max() <= 1e-12


def test_p_value_counts_ties_in():
    from buglab.models._drift import p_value

    assert p_value([0.5, 0.1, 0.5, 0.7, 0.2]) == 3 / 5      # 0.5 >= 0.5 counts
    assert p_value([0.5, 0.1, 0.2]) == 1 / 3
    assert p_value([0.0, 0.0, 0.0, 0.0]) == 1.0
    assert p_value([0.5, np.nextafter(0.5, 0.0)]) == 1 / 2


def test_no_spread_is_statistic_zero_and_p_value_one():
    from buglab.models._drift import bandwidth_host, drift_host

    row = np.random.default_rng(0).standard_normal(24).astype(np.float32) * 1e3
    x, y = np.tile(row, (5, 1)), np.tile(row, (7, 1))
    assert bandwidth_host(np.concatenate([x, y])) == 0.0     # whatever the fp64 sums round to
    report = drift_host(x, y, 9)
    rec = report.record()
    assert (report.bandwidth, report.statistic, report.p_value, report.drift) == (0.0, 0.0, 1.0, False) and rec["no_spread"]
    json.dumps(rec)
    z = np.random.default_rng(1).standard_normal((9, 6)).astype(np.float32)
    want = 2.0 * ((z.astype(np.float64)[:, None] - z.astype(np.float64)[None]) ** 2).sum(axis=2).mean() / 2.0
    assert abs(bandwidth_host(z) - want) <= 1e-12 * want and abs(bandwidth_host(z, 0.5) - 0.5 * want) <= 1e-12 * want
    with pytest.raises(ValueError, match="at least 2 rows"):
        drift_host(x[:1], y, 9)
    with pytest.raises(ValueError, match="permutations"):
        drift_host(x, y, 0)


# ------------------------------------------------------------------------------------------------ the cases of the GPU tests
# `far`: one row carries the whole bandwidth, every other kernel value is 1 - O(1e-3) and MMD2 is 1e-4 of S / N^2, so tau is
# a good part of the null's spread whatever the seed; the GPU test asserts the band there, and cannot assert it is narrow.
WIDE_BAND = {"edge-far", "exact-far"}


@pytest.mark.parametrize("name", list(C.CASES))
def test_the_seeds_keep_the_p_value_band_narrow(name):
    case = C.CASES[name]
    ref = C.reference(name)
    A, B, S, u0, rho = C.sums_fp32_numpy(ref.z, case.n, ref.masks, ref.s)
    err = C.err_mmd2(ref, A, B, S, case.n, case.m)
    assert err < 1e-4, err  # the stand-in is an fp32 computation
    lo, hi = C.p_band(ref, C.bound(err) * ref.unit)
    inside = round((hi - lo) * (case.R + 1))
    print(f"{name}: fp32 NumPy err {err:.3g}, band [{lo:.4g}, {hi:.4g}], {inside} permutations inside")
    if name not in WIDE_BAND:
        assert inside <= 2
    if case.shift:
        assert lo == hi == 1.0 / (case.R + 1)
    assert (ref.masks.sum(axis=1) == case.n).all() and ref.s > 0.0


# ------------------------------------------------------------------------------------------------ command line and surface
def test_command_line_parses():
    from buglab.models import drift as T

    a = T.parse_args(["m", "i", "d", "o"])
    assert (a.num_permutations, a.seed, a.alpha, a.bandwidth_scale, a.top_k, a.site) == (1000, 0, 0.05, 1.0, 20, "predicted")
    assert (a.assume_buggy, a.max_reference, a.limit_num_elements, a.sequential, a.host, a.report_json) == (False, None, None, False, False, None)
    b = T.parse_args(["m", "i", "d", "o", "--num-permutations", "99", "--seed", "4", "--alpha", "0.1", "--bandwidth-scale", "0.5", "--top-k",
                      "3", "--site", "truth", "--assume-buggy", "--max-reference", "500", "--limit-num-elements", "7", "--sequential",
                      "--host", "--report-json", "r.json"])
    assert (b.num_permutations, b.seed, b.alpha, b.bandwidth_scale, b.top_k, b.site, b.max_reference) == (99, 4, 0.1, 0.5, 3, "truth", 500)
    assert b.assume_buggy and b.sequential and b.host and b.report_json == "r.json" and b.limit_num_elements == 7
    for bad in (["--num-permutations", "0"], ["--alpha", "1.5"], ["--bandwidth-scale", "0"]):
        with pytest.raises(SystemExit):
            T.parse_args(["m", "i", "d", "o"] + bad)
    assert "BEYOND THE REFERENCE" in T.__doc__ and (T.EXIT_NO_DRIFT, T.EXIT_DRIFT, T.EXIT_DIMENSION_MISMATCH) == (0, 1, 2)
    assert T.kernel_shift(1.0) == np.exp(-1.0)


def _index(x, model_class="Stub"):
    from buglab.models import _similar as S

    n = x.shape[0]
    sites = S.SiteEmbeddings(x, np.arange(n), np.zeros(n, np.int32), np.zeros(n, np.float32), ["l"] * n, ["p"] * n, ["k"] * n, ["s"] * n, n, 0, 0)
    return S.make_index(sites, None, True, model_class, "00")


def test_exit_statuses_with_a_stub_for_the_embedding_step(tmp_path, monkeypatch, capsys):
    from buglab.models import _drift as Dr
    from buglab.models import _similar as S
    from buglab.models import drift as T

    class Stub:
        pass

    rng = np.random.default_rng(5)
    x = rng.standard_normal((80, 8)).astype(np.float32)
    index = _index(x, "Stub")
    index.save(tmp_path / "ref.npz")
    scanned = {"same": rng.standard_normal((70, 8)).astype(np.float32), "moved": (rng.standard_normal((70, 8)) + 0.8).astype(np.float32)}
    seen = {}

    def detect(model, nn, index, data, device, num_permutations, seed, **options):
        seen.update(options, num_permutations=num_permutations, seed=seed)
        report = Dr.drift_host(index.embeddings, S.centre(scanned[data], index.mean), num_permutations, seed, options["alpha"],
                               options["bandwidth_scale"], options["top_k"])
        return report._replace(num_samples=70, num_rejected=1, num_without_site=2)

    monkeypatch.setattr(T, "_open_model", lambda path: (Stub(), None, "cuda", True))
    monkeypatch.setattr(T, "_embedding_dim", lambda nn: 8)
    monkeypatch.setattr(T, "_read_data", lambda path, limit: path)
    monkeypatch.setattr(T, "detect_drift", detect)
    out, rep = tmp_path / "out.jsonl", tmp_path / "report.json"
    common = ["m", str(tmp_path / "ref.npz")]
    status = T.run(T.parse_args(common + ["same", str(out), "--num-permutations", "99", "--top-k", "4", "--report-json", str(rep), "--seed", "2"]))
    text = capsys.readouterr().out
    blob = json.loads(rep.read_text())
    assert status == T.EXIT_NO_DRIFT == 0 and "no drift at alpha 0.05" in text and blob["p_value"] > 0.05 and not blob["drift"]
    assert (blob["n"], blob["m"], blob["dim"], blob["num_permutations"], blob["seed"]) == (80, 70, 8, 99, 2)
    assert (blob["num_samples"], blob["num_rejected"], blob["num_without_site"]) == (70, 1, 2)
    assert {"bandwidth", "mmd2", "null_mean", "null_q95", "alpha", "outliers", "no_spread"} <= set(blob)
    lines = [json.loads(line) for line in out.read_text().splitlines()]
    assert len(lines) == 4 and [r["witness"] for r in lines] == sorted(r["witness"] for r in lines) and lines == blob["outliers"]
    assert (seen["top_k"], seen["site"], seen["host"], seen["max_reference"], seen["parallelize"]) == (4, "predicted", False, None, True)
    status = T.run(T.parse_args(common + ["moved", str(out), "--num-permutations", "99"]))
    assert status == T.EXIT_DRIFT == 1 and "DRIFT at alpha 0.05: p-value 0.01" in capsys.readouterr().out
    assert len(out.read_text().splitlines()) == 20
    # an index of another size: status 2 before any data is read, nothing written
    monkeypatch.setattr(T, "_embedding_dim", lambda nn: 16)
    monkeypatch.setattr(T, "_read_data", lambda path, limit: pytest.fail("the data was read"))
    other = tmp_path / "other.jsonl"
    assert T.run(T.parse_args(common + ["same", str(other)])) == T.EXIT_DIMENSION_MISMATCH == 2
    assert "size 8" in capsys.readouterr().err and not other.exists()
    # no GPU: the hot path has no CPU fallback
    monkeypatch.setattr(T, "_embedding_dim", lambda nn: 8)
    monkeypatch.setattr(T, "_open_model", lambda path: (Stub(), None, "cpu", False))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.run(T.parse_args(common + ["same", str(other)]))


def test_reference_subset_and_refusals():
    from buglab.models import drift as T
    from buglab.models.ensemble.wrapper import EnsembleWrapper

    index = _index(np.random.default_rng(0).standard_normal((30, 4)).astype(np.float32))
    assert T.reference_rows(index, None, 0).tolist() == list(range(30)) and T.reference_rows(index, 99, 0).tolist() == list(range(30))
    some = T.reference_rows(index, 10, 3)
    assert some.shape == (10,) and (np.diff(some) > 0).all() and some.tolist() == T.reference_rows(index, 10, 3).tolist()
    assert some.tolist() != T.reference_rows(index, 10, 4).tolist()
    with pytest.raises(ValueError, match="at least 2"):
        T.reference_rows(index, 1, 0)
    with pytest.raises(TypeError, match="ensembles"):
        T.detect_drift(EnsembleWrapper.__new__(EnsembleWrapper), None, index, [], "cpu")
    # the host path of drift_between needs no device
    x = np.random.default_rng(1).standard_normal((12, 4)).astype(np.float32)
    report = T.drift_between(index.embeddings, x, num_permutations=19, host=True, top_k=3)
    assert report.n == 30 and report.m == 12 and len(report.outliers) == 3 and 0.0 < report.p_value <= 1.0


def test_launchers_check_before_any_hip_call():
    import ctypes
    import os

    import torch

    from buglab.models import _drift as Dr
    from buglab.models import hip_ops
    from tests.conftest import ROOT

    header = open(os.path.join(ROOT, "include", "buglab_hip.h")).read()
    assert "#define BL_DRIFT_MAX_D 512" in header and hip_ops.DRIFT_MAX_D == Dr.MAX_D == 512
    assert "#define BL_DRIFT_MAX_PERMUTATIONS 65533" in header and hip_ops.DRIFT_MAX_PERMUTATIONS == Dr.MAX_PERMUTATIONS == 65533
    for name in ("bl_drift_ok", "bl_drift_mask_ld", "bl_drift_bandwidth", "bl_drift_subsets", "bl_drift_permutation_sums"):
        assert name in hip_ops.EXPORTED_SYMBOLS
    for name in ("drift_bandwidth", "drift_subsets", "drift_permutation_sums", "drift_ok"):
        assert name in hip_ops.services.__all__
    f32, f64, u8 = (lambda *s: torch.zeros(*s)), (lambda *s: torch.zeros(*s, dtype=torch.float64)), (lambda *s: torch.zeros(*s, dtype=torch.uint8))
    assert hip_ops.drift_ok(512, 65533) and not hip_ops.drift_ok(513, 10) and not hip_ops.drift_ok(8, 0) and not hip_ops.drift_ok(8, 65534)
    assert [hip_ops.drift_mask_ld(N) for N in (4, 32, 33, 257)] == [32, 32, 64, 288]
    with pytest.raises(ValueError, match="N >= 4"):
        hip_ops.drift_bandwidth(f32(3, 8))
    with pytest.raises(ValueError, match="scale"):
        hip_ops.drift_bandwidth(f32(8, 8), 0.0)
    with pytest.raises(ValueError, match="at least 2 rows"):
        hip_ops.drift_subsets(10, 9, 5, 0, "cuda")
    with pytest.raises(ValueError, match="GPU"):
        hip_ops.drift_subsets(10, 5, 5, 0, "cpu")
    with pytest.raises(ValueError, match="mask"):
        hip_ops.drift_permutation_sums(f32(10, 8), f32(10), u8(7, 10), 5, f64(1))
    with pytest.raises(ValueError, match="col_tiles"):
        hip_ops.drift_permutation_sums(f32(10, 8), f32(10), u8(7, 32), 5, f64(1), col_tiles=3)
    with pytest.raises(ValueError, match="shift"):
        hip_ops.drift_permutation_sums(f32(10, 8), f32(10), u8(7, 32), 5, f64(1), 1.5)
    with pytest.raises(ValueError, match="1 <= D <= 512"):
        hip_ops.drift_permutation_sums(f32(10, 513), f32(10), u8(7, 32), 5, f64(1))
    with pytest.raises(ValueError, match="GPU"):
        hip_ops.drift_permutation_sums(f32(10, 8), f32(10), u8(7, 32), 5, f64(1))

    lib = hip_ops.load_library()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.bl_drift_ok(512, 65533) == 1 and lib.bl_drift_ok(513, 1) == 0 and lib.bl_drift_ok(1, 0) == 0
    assert [lib.bl_drift_mask_ld(N) for N in (4, 33, 257)] == [32, 64, 288]
    assert lib.bl_drift_bandwidth_workspace_bytes(257, 64) == 2 * 65 * 8 and lib.bl_drift_sums_workspace_bytes(257, 199) == 2 * 17 * 201 * 8
    assert lib.bl_drift_bandwidth(None, 8, 10, 8, 1.0, p, 1 << 20, p, p, None) == -1 and b"null" in lib.bl_last_error()
    assert lib.bl_drift_bandwidth(p, 4, 10, 8, 1.0, p, 1 << 20, p, p, None) == -1 and b"row stride" in lib.bl_last_error()
    assert lib.bl_drift_bandwidth(p, 600, 10, 513, 1.0, p, 1 << 20, p, p, None) == -2 and b"BL_DRIFT_MAX_D" in lib.bl_last_error()
    assert lib.bl_drift_bandwidth(p, 8, 10, 8, 1.0, p, 8, p, p, None) == -1 and b"workspace" in lib.bl_last_error()
    assert lib.bl_drift_subsets(10, 1, 5, 0, p, 32, None) == -1 and b"at least 2 rows" in lib.bl_last_error()
    assert lib.bl_drift_subsets(10, 5, 0, 0, p, 32, None) == -1 and b"R must be" in lib.bl_last_error()
    assert lib.bl_drift_subsets(10, 5, 5, 0, p, 10, None) == -1 and b"row stride" in lib.bl_last_error()
    assert lib.bl_drift_subsets(10, 5, 70000, 0, p, 32, None) == -2
    args = lambda **kw: [kw.get(k, v) for k, v in (("z", p), ("ldz", 8), ("N", 10), ("n", 5), ("D", 8), ("rn", p), ("mask", p), ("ldm", 32),
                                                   ("R", 5), ("bw", p), ("shift", 0.3), ("ct", 0), ("ws", p), ("wsb", 1 << 20), ("o1", p),
                                                   ("o2", p), ("o3", p), ("st", None))]
    assert lib.bl_drift_permutation_sums(*args(mask=None)) == -1 and b"null" in lib.bl_last_error()
    assert lib.bl_drift_permutation_sums(*args(n=9)) == -1 and b"at least 2 rows" in lib.bl_last_error()
    assert lib.bl_drift_permutation_sums(*args(ct=5)) == -1 and b"col_tiles" in lib.bl_last_error()
    assert lib.bl_drift_permutation_sums(*args(shift=2.0)) == -1 and b"shift" in lib.bl_last_error()
    assert lib.bl_drift_permutation_sums(*args(wsb=64)) == -1 and b"workspace" in lib.bl_last_error()
    assert lib.bl_drift_permutation_sums(*args(ldm=10)) == -1 and b"row stride" in lib.bl_last_error()
    assert lib.bl_drift_permutation_sums(*args(D=600, ldz=600)) == -2 and b"512" in lib.bl_last_error()
