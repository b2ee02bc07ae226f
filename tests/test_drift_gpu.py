"""GPU: the drift-detection kernels (csrc/bl_drift.hip) against their NumPy twin -- the subsets bit for bit, the fused permutation
sums against fp64 with a plain torch fp32 computation on the same GPU as the yardstick -- and buglab/models/drift.py end to end
on two untrained models.  The shapes and their fp64 reference: tests/drift_cases.py.

The bound everywhere: err_device <= 4 max(err_torch, 2^-23), each error relative to the size of what it is an error of (for
MMD2: S / N^2, the terms that cancel).  Every test prints both errors before it asserts.
"""
import copy
import gzip
import json
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import drift_cases as C
from tests.guard_bands import guarded

pytestmark = pytest.mark.gpu

DEV = "cuda"
SPECS = {"gnn-mlp": {"modelName": "gnn-mlp", "hidden_state_size": 32, "num_layers": 4, "dropout_rate": 0.1},
         "seq-great": {"modelName": "seq-great", "hidden_state_size": 32, "num_layers": 2, "num_heads": 4, "intermediate_dimension_size": 96,
                       "dropout_rate": 0.1}}


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)  # a copy: the shared references are read-only


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _device_sums(z, n, R, seed, col_tiles=None, scale=1.0):
    """the three launches on pooled rows z (an array, or a device tensor taken as it is) -> NumPy (s, A, B, S, u0, rho, mask)"""
    from buglab.models import hip_ops
    from buglab.models.drift import kernel_shift

    d_z = _dev(z) if isinstance(z, np.ndarray) else z
    bandwidth, rownorm = hip_ops.drift_bandwidth(d_z, scale)
    mask = hip_ops.drift_subsets(d_z.shape[0], n, R, seed, DEV)
    sums, u0, rho = hip_ops.drift_permutation_sums(d_z, rownorm, mask, n, bandwidth, kernel_shift(scale), col_tiles=col_tiles)
    sums = sums.cpu().numpy()
    return float(bandwidth.cpu()[0]), sums[:R + 1], sums[R + 1:2 * R + 2], float(sums[2 * R + 2]), u0.cpu().numpy(), rho.cpu().numpy(), mask.cpu().numpy()


def _torch_sums(z, masks, s):
    """the yardstick: the same computation in plain torch fp32 on this GPU with K materialised (mm, exp, mm; no TF32-like mode)"""
    was = torch.backends.cuda.matmul.allow_tf32, torch.get_float32_matmul_precision()
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.set_float32_matmul_precision("highest")
    try:
        d_z, a = _dev(np.asarray(z, np.float32)), _dev(np.asarray(masks)).float()
        sq = (d_z * d_z).sum(dim=1)
        K = torch.exp(-(sq[:, None] + sq[None, :] - 2.0 * (d_z @ d_z.T)).clamp_min(0.0) / float(np.float32(s)))
        U = K @ a.T
        rho = K.sum(dim=1)
        out = ((a.T * U).sum(dim=0), U.sum(dim=0), rho.sum(), U[:, 0], rho)
        return tuple(t.double().cpu().numpy() for t in out)
    finally:
        torch.backends.cuda.matmul.allow_tf32 = was[0]
        torch.set_float32_matmul_precision(was[1])


@lru_cache(maxsize=None)
def _measured(name):
    """one device run and one yardstick run per case, shared by the tests"""
    case, ref = C.CASES[name], C.reference(name)
    got = _device_sums(ref.z, case.n, case.R, case.seed)
    yard = _torch_sums(ref.z, ref.masks, ref.s)
    return got, yard


# ------------------------------------------------------------------------------------------------ 1. subsets
@pytest.mark.parametrize("name", ["edge", "exact", "least"])
def test_subsets_equal_the_twin_bit_for_bit(name):
    from buglab.models import hip_ops
    from buglab.models._drift import subsets_host

    case = C.CASES[name]
    N, R = case.n + case.m, case.R
    ld = hip_ops.drift_mask_ld(N)
    for seed in (0, 0x9E3779B97F4A7C15):
        for n in sorted({2, N // 2, N - 2}):
            g = guarded(R + 2, ld, ld=ld, dtype=torch.uint8, device=DEV)
            mask = g.view.view(R + 2, ld)
            assert mask.is_contiguous() and hip_ops.drift_subsets(N, n, R, seed, out=mask) is mask
            g.assert_untouched(f"{name} mask")
            got = mask.cpu().numpy()
            assert np.array_equal(got[:R + 1, :N], subsets_host(N, n, R, seed)), (name, seed, n)
            assert (got[R + 1, :N] == 1).all() and not got[:, N:].any()


def test_subsets_at_a_size_with_many_chunks():
    from buglab.models import hip_ops
    from buglab.models._drift import subsets_host

    N, n, R = 5000, 1777, 6
    got = hip_ops.drift_subsets(N, n, R, 11, DEV).cpu().numpy()
    assert np.array_equal(got[:R + 1, :N], subsets_host(N, n, R, 11)) and not got[:, N:].any()


# ------------------------------------------------------------------------------------------------ 2. the sums against fp64
@pytest.mark.parametrize("name", list(C.CASES))
def test_statistic_and_sums_against_fp64(name):
    case, ref = C.CASES[name], C.reference(name)
    (s, A, B, S, u0, rho, mask), (tA, tB, tS, tu0, trho) = _measured(name)
    assert np.array_equal(mask[:case.R + 1, :case.n + case.m], ref.masks)
    assert abs(s - ref.s) <= 1e-12 * ref.s
    err_dev, err_torch = C.err_mmd2(ref, A, B, S, case.n, case.m), C.err_mmd2(ref, tA, tB, tS, case.n, case.m)
    print(f"\n{name}: MMD2 err_device {err_dev:.3g} err_torch {err_torch:.3g} ratio {err_dev / max(err_torch, C.EPS):.3g}")
    parts = {"A": (A, tA, ref.A), "B": (B, tB, ref.B), "S": ([S], [tS], [ref.S])}
    errs = {k: (C.err_of(d, w), C.err_of(t, w)) for k, (d, t, w) in parts.items()}
    for k, (ed, et) in errs.items():
        print(f"{name}: {k} err_device {ed:.3g} err_torch {et:.3g} ratio {ed / max(et, C.EPS):.3g}")
    assert np.isfinite(A).all() and np.isfinite(B).all() and np.isfinite(S)
    assert err_dev <= C.bound(err_torch)
    for k, (ed, et) in errs.items():
        assert ed <= C.bound(et), k


# ------------------------------------------------------------------------------------------------ 3. the p-value
@pytest.mark.parametrize("name", list(C.CASES))
def test_p_value_lies_in_the_band_of_the_fp64_twin(name):
    """`far`: one row carries the whole bandwidth, MMD2 is 1e-4 of S / N^2 and tau a good part of the null's spread for every
    seed (tests/test_drift_host.py): the band is asserted there too, only not that it is narrow."""
    from buglab.models._drift import mmd2, p_value

    case, ref = C.CASES[name], C.reference(name)
    (s, A, B, S, u0, rho, _), (tA, tB, tS, _, _) = _measured(name)
    tau = C.bound(C.err_mmd2(ref, tA, tB, tS, case.n, case.m)) * ref.unit
    lo, hi = C.p_band(ref, tau)
    p = p_value(mmd2(A, B, S, case.n, case.m))
    inside = round((hi - lo) * (case.R + 1))
    print(f"\n{name}: p {p:.6g} in [{lo:.6g}, {hi:.6g}], tau {tau:.3g}, {inside} permutations inside the band")
    if not (name.endswith("-far") and case.R > 1):
        assert inside <= 2  # not vacuous
    assert lo <= p <= hi
    if case.shift:
        assert lo == hi == p == 1.0 / (case.R + 1)


# ------------------------------------------------------------------------------------------------ 4. identical samples
def test_identical_samples():
    from buglab.models._drift import mmd2, p_value, permutation_sums_host, bandwidth_host, witness

    x = C.rows(C.CASES["exact"])[0]
    order = np.random.default_rng(2).permutation(x.shape[0])
    z = np.concatenate([x, x[order]])
    n = m = x.shape[0]
    R, seed = 63, 21
    s, A, B, S, u0, rho, mask = _device_sums(z, n, R, seed)
    fA, fB, fS, _, _ = permutation_sums_host(z, n, mask[:R + 1, :n + m], bandwidth_host(z))
    tA, tB, tS, _, _ = _torch_sums(z, mask[:R + 1, :n + m], s)
    want = mmd2(fA, fB, fS, n, m)
    unit = fS / (n + m) ** 2
    err_torch = float(np.abs(mmd2(tA, tB, tS, n, m) - want).max() / unit)
    tau = C.bound(err_torch) * unit
    stats, f = mmd2(A, B, S, n, m), witness(u0, rho, n, m)
    print(f"\nidentical: MMD2_0 {stats[0]:.3g}, tau {tau:.3g}, max |witness| {np.abs(f).max():.3g}, err_torch {err_torch:.3g}")
    assert abs(want[0]) <= 1e-12 and abs(stats[0]) <= tau
    assert p_value(stats) == 1.0
    assert np.abs(f).max() <= 2.0 * tau  # the difference of two kernel means, each within tau of the other's


# ------------------------------------------------------------------------------------------------ 5. the same bits, whatever the grid
@pytest.mark.parametrize("name", ["edge", "exact-dup", "least", "shifted", "wide", "widest"])
def test_equal_bits_on_every_run_and_for_every_tile_split(name):
    from buglab.models._drift import mmd2

    case, ref = C.CASES[name], C.reference(name)
    first = _measured(name)[0]
    for col_tiles in (None, 4, 8, 16):
        again = _device_sums(ref.z, case.n, case.R, case.seed, col_tiles)
        assert again[0] == first[0] and again[3] == first[3], col_tiles
        for a, b in zip(again[1:], first[1:]):
            assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), col_tiles
    # another order of the rows within each sample: the observed statistic moves by rounding only
    (_, A, B, S, _, _, _), (tA, tB, tS, _, _) = first, _measured(name)[1]
    tau = C.bound(C.err_mmd2(ref, tA, tB, tS, case.n, case.m)) * ref.unit
    rng = np.random.default_rng(4)
    order = np.concatenate([rng.permutation(case.n), case.n + rng.permutation(case.m)])
    _, pA, pB, pS, _, _, _ = _device_sums(ref.z[order], case.n, case.R, case.seed)
    moved = abs(mmd2(pA, pB, pS, case.n, case.m)[0] - mmd2(A, B, S, case.n, case.m)[0])
    print(f"\n{name}: MMD2_0 moves by {moved:.3g} under a row permutation, tau {tau:.3g}")
    assert moved <= tau


# ------------------------------------------------------------------------------------------------ 6. the witness
def _witness_slack(u0_err, rho_err, ref_u0, ref_rho, n, m):
    """what the errors of the two columns of U allow the witness to move by"""
    du, dr = u0_err * np.abs(ref_u0).max(), rho_err * np.abs(ref_rho).max()
    return du / n + (dr + du) / m


@pytest.mark.parametrize("name", list(C.CASES))
def test_witness_columns_and_outliers(name):
    from buglab.models._drift import outliers, witness

    case, ref = C.CASES[name], C.reference(name)
    (_, _, _, _, u0, rho, _), (_, _, _, tu0, trho) = _measured(name)
    e_u, t_u, e_r, t_r = C.err_of(u0, ref.u0), C.err_of(tu0, ref.u0), C.err_of(rho, ref.rho), C.err_of(trho, ref.rho)
    print(f"\n{name}: U[:, 0] err_device {e_u:.3g} err_torch {t_u:.3g}; rho err_device {e_r:.3g} err_torch {t_r:.3g}")
    assert e_u <= C.bound(t_u) and e_r <= C.bound(t_r)
    f, want = witness(u0, rho, case.n, case.m), witness(ref.u0, ref.rho, case.n, case.m)
    slack = _witness_slack(C.bound(t_u), C.bound(t_r), ref.u0, ref.rho, case.n, case.m)
    assert np.abs(f - want).max() <= slack
    k = min(5, case.m - 1)
    ordered = np.sort(want)
    if ordered[k] - ordered[k - 1] > 2.0 * slack:
        assert set(outliers(f, k).tolist()) == set(outliers(want, k).tolist())
    else:
        print(f"{name}: the twin's values {k} and {k + 1} are {ordered[k] - ordered[k - 1]:.3g} apart, within the bound: no claim")


# ------------------------------------------------------------------------------------------------ strides and guard bands
@pytest.mark.parametrize("name", ["edge", "exact", "least", "edge-dup", "exact-far", "wide", "widest"])
def test_strided_inputs_and_guarded_outputs_give_the_same_bits(name):
    """through the C ABI: rows with a stride of D + 3 at an unaligned base, every output and workspace inside poisoned guard
    bands (tests/guard_bands.py, as tests/test_abi_strides_gpu.py does)"""
    from buglab.models import hip_ops
    from buglab.models.drift import kernel_shift

    case, ref = C.CASES[name], C.reference(name)
    N, n, D, R = case.n + case.m, case.n, case.D, case.R
    want = _measured(name)[0]
    lib = hip_ops.load_library()
    flat = torch.full((1 + N * (D + 3) + 8,), float("nan"), dtype=torch.float32, device=DEV)
    d_z = flat[1:1 + N * (D + 3)].view(N, D + 3)[:, :D]
    d_z.copy_(_dev(ref.z))
    ld = hip_ops.drift_mask_ld(N)
    tiles = (N + 15) // 16
    f64 = lambda rows: guarded(rows, 2, ld=2, dtype=torch.int32, device=DEV, lead=6, any_width=True)
    g_rn = guarded(N, 1, ld=1, dtype=torch.float32, device=DEV, lead=5, any_width=True)
    g_bw, g_ws1 = f64(1), f64(int(lib.bl_drift_bandwidth_workspace_bytes(N, D)) // 8)
    g_mask = guarded(R + 2, ld, ld=ld, dtype=torch.uint8, device=DEV)
    g_ws2, g_sums, g_u0, g_rho = f64(2 * tiles * (R + 2)), f64(2 * R + 3), f64(N), f64(N)
    assert int(lib.bl_drift_sums_workspace_bytes(N, R)) == 2 * tiles * (R + 2) * 8
    rc = lib.bl_drift_bandwidth(d_z.data_ptr(), D + 3, N, D, 1.0, g_ws1.data_ptr(), g_ws1.rows * 8, g_rn.data_ptr(), g_bw.data_ptr(), _stream())
    assert rc == 0, lib.bl_last_error()
    rc = lib.bl_drift_subsets(N, n, R, case.seed, g_mask.data_ptr(), ld, _stream())
    assert rc == 0, lib.bl_last_error()
    rc = lib.bl_drift_permutation_sums(d_z.data_ptr(), D + 3, N, n, D, g_rn.data_ptr(), g_mask.data_ptr(), ld, R, g_bw.data_ptr(),
                                       kernel_shift(1.0), 0, g_ws2.data_ptr(), g_ws2.rows * 8, g_sums.data_ptr(), g_u0.data_ptr(),
                                       g_rho.data_ptr(), _stream())
    assert rc == 0, lib.bl_last_error()
    for g, what in ((g_rn, "rownorm"), (g_bw, "bandwidth"), (g_ws1, "bandwidth workspace"), (g_mask, "mask"), (g_ws2, "sums workspace"),
                    (g_sums, "sums"), (g_u0, "u0"), (g_rho, "rho")):
        g.assert_untouched(f"{name} {what}")
    as_f64 = lambda g: g.view.contiguous().cpu().numpy().view(np.float64)[:, 0]
    sums = as_f64(g_sums)
    got = (float(as_f64(g_bw)[0]), sums[:R + 1], sums[R + 1:2 * R + 2], float(sums[2 * R + 2]), as_f64(g_u0), as_f64(g_rho),
           g_mask.view.contiguous().cpu().numpy())
    assert got[0] == want[0] and got[3] == want[3]
    for a, b in zip(got[1:], want[1:]):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
    assert np.isfinite(sums).all()  # no poisoned padding reached a result


# ------------------------------------------------------------------------------------------------ 7. memory, and many tiles
def test_no_kernel_matrix_is_allocated():
    from buglab.models import hip_ops
    from buglab.models.drift import kernel_shift

    N, n, D, R = 8192, 4096, 64, 255
    rng = np.random.default_rng(8)
    z = rng.standard_normal((N, D)).astype(np.float32)
    z[n:] += 0.05
    d_z = _dev(z)
    bandwidth, rownorm = hip_ops.drift_bandwidth(d_z)
    mask = hip_ops.drift_subsets(N, n, R, 1, DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    sums, u0, rho = hip_ops.drift_permutation_sums(d_z, rownorm, mask, n, bandwidth, kernel_shift(1.0))
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print(f"\npeak allocation of drift_permutation_sums at N = {N}, R = {R}: {peak / 2 ** 20:.1f} MiB (one fp32 N x N: {4 * N * N / 2 ** 20:.0f} MiB)")
    assert peak < 4 * N * N
    # a sample of rows against fp64: row tiles far from the first, 256 chunks of j
    picked = np.concatenate([np.arange(0, N, 257), [n - 1, n, N - 1]])
    z64, s = z.astype(np.float64), float(bandwidth.cpu()[0])
    sq = (z64 * z64).sum(axis=1)
    K = np.exp(-np.maximum(sq[picked, None] + sq[None, :] - 2.0 * z64[picked] @ z64.T, 0.0) / s)
    tol = N * 2.0 ** -24 * K.sum(axis=1).max()  # the worst case of an fp32 sum of N terms of one sign
    assert np.abs(rho.cpu().numpy()[picked] - K.sum(axis=1)).max() <= tol
    assert np.abs(u0.cpu().numpy()[picked] - K[:, :n].sum(axis=1)).max() <= tol
    got = sums.cpu().numpy()
    assert abs(got[2 * R + 2] - rho.cpu().numpy().sum()) <= 1e-9 * got[2 * R + 2]  # S is the sum of rho


# ------------------------------------------------------------------------------------------------ 8. end to end
@pytest.fixture(scope="module")
def untrained(tmp_path_factory):
    """family -> (model, module, reference pool, scanned data, checkpoint path): seeded weights, no training"""
    from buglab.data.synthetic import make_report_dataset
    from buglab.models.modelregistry import load_model
    from buglab.runtime.neuralmodel import AbstractNeuralModel

    out = {}
    for family, spec in SPECS.items():
        kind = "seq" if family.startswith("seq") else "graph"
        pool, data = make_report_dataset(60, seed=18, kind=kind), make_report_dataset(60, seed=17, kind=kind)
        path = tmp_path_factory.mktemp("drift_" + family.replace("-", "_")) / "detector.pkl.gz"
        model = load_model(dict(spec), path)[0]
        model.compute_metadata(copy.deepcopy(pool + data))
        torch.manual_seed(5)
        model.save(path, model.build_neural_module())
        out[family] = AbstractNeuralModel.restore_model(Path(path), torch.device(DEV)) + (pool, data, path)
    return out


@pytest.mark.parametrize("family", list(SPECS))
def test_detect_drift_on_the_device_agrees_with_the_host_path(family, untrained):
    from buglab.models import _drift as Dr
    from buglab.models import _similar as S
    from buglab.models import drift as T
    from buglab.models import hip_ops, similar

    model, nn_, pool, data, _ = untrained[family]
    device = torch.device(DEV)
    was = bool(hip_ops.load_library().bl_get_deterministic())
    hip_ops.set_deterministic(True)
    try:
        index = similar.build_site_index(model, nn_, pool, device, "truth", parallelize=False)
        assert index.size >= 10 and np.unique(index.embeddings, axis=0).shape[0] > 5
        # the reference set itself: the two samples are the same points
        own = T.detect_drift(model, nn_, index, pool, device, 99, 3, site="truth", parallelize=False)
        assert own.p_value == 1.0 and not own.drift and own.n == own.m == index.size
        assert (own.num_samples, own.num_rejected, own.num_without_site) == (60, 0, 60 - index.size)
        # other data: the device against the twin on the same embeddings
        options = dict(site="predicted", assume_buggy=True, top_k=5, parallelize=False)
        dev = T.detect_drift(model, nn_, index, data, device, 199, 7, **options)
        host = T.detect_drift(model, nn_, index, data, device, 199, 7, host=True, **options)
        assert (dev.n, dev.m, dev.dim, dev.num_permutations) == (host.n, host.m, host.dim, 199) == (index.size, 60, 32, 199)
        sites = similar.embed_sites(model, nn_, data, device, "predicted", assume_buggy=True, parallelize=False)
        z = np.concatenate([index.embeddings, S.centre(sites.rows, index.mean)])
        masks = Dr.subsets_host(z.shape[0], index.size, 199, 7)
        A, B, Ssum, u0, rho = Dr.permutation_sums_host(z, index.size, masks, host.bandwidth)
        want = Dr.mmd2(A, B, Ssum, dev.n, dev.m)
        assert want[0] == host.statistic and abs(dev.bandwidth - host.bandwidth) <= 1e-12 * host.bandwidth
        tA, tB, tS, tu0, trho = _torch_sums(z, masks, host.bandwidth)
        unit = Ssum / z.shape[0] ** 2
        err_torch = float(np.abs(Dr.mmd2(tA, tB, tS, dev.n, dev.m) - want).max() / unit)
        tau = C.bound(err_torch) * unit
        err_dev = float(np.abs(np.concatenate([[dev.statistic], dev.null]) - want).max() / unit)
        print(f"\n{family}: MMD2 err_device {err_dev:.3g} err_torch {err_torch:.3g}; p device {dev.p_value:.4g} host {host.p_value:.4g}")
        assert err_dev <= C.bound(err_torch)
        null, R1 = want[1:], 200.0
        lo, hi = (1 + int((null >= want[0] + tau).sum())) / R1, (1 + int((null >= want[0] - tau).sum())) / R1
        assert lo <= dev.p_value <= hi and lo <= host.p_value <= hi
        slack = _witness_slack(C.bound(C.err_of(tu0, u0)), C.bound(C.err_of(trho, rho)), u0, rho, dev.n, dev.m)
        assert np.abs(dev.witness - host.witness).max() <= slack
        ordered = np.sort(host.witness)
        if ordered[5] - ordered[4] > 2.0 * slack:
            assert {o["position"] for o in dev.outliers} == {o["position"] for o in host.outliers}
        assert all({"position", "witness", "node", "label", "filename", "package", "scout"} <= set(o) for o in dev.outliers)
        assert [o["witness"] for o in dev.outliers] == sorted(o["witness"] for o in dev.outliers) and len(dev.outliers) == 5
        # --max-reference: a seeded subset of the index
        few = T.detect_drift(model, nn_, index, data, device, 19, 7, max_reference=12, **options)
        assert few.n == 12 and few.m == 60
    finally:
        hip_ops.set_deterministic(was)


def test_command_line(untrained, tmp_path, capsys):
    from buglab.models import drift as T
    from buglab.models import similar
    from buglab.utils.msgpackutils import save_msgpack_l_gz

    _, _, pool, data, path = untrained["gnn-mlp"]
    pool_dir, data_dir = tmp_path / "pool", tmp_path / "data"
    pool_dir.mkdir(), data_dir.mkdir()
    save_msgpack_l_gz(pool, pool_dir / "x.msgpack.l.gz"), save_msgpack_l_gz(data, data_dir / "x.msgpack.l.gz")
    out_index, out, report = tmp_path / "ref.npz", tmp_path / "drift.jsonl.gz", tmp_path / "report.json"
    assert similar.run(similar.parse_args(["index", str(path), str(pool_dir), str(out_index), "--sequential"])) == 0
    capsys.readouterr()
    status = T.run(T.parse_args([str(path), str(out_index), str(pool_dir), str(out), "--site", "truth", "--num-permutations", "99", "--top-k", "3",
                                 "--report-json", str(report), "--sequential"]))
    text = capsys.readouterr().out
    blob = json.loads(report.read_text(encoding="utf-8"))
    assert status == T.EXIT_NO_DRIFT == 0 and "no drift at alpha 0.05: p-value 1," in text
    assert blob["p_value"] == 1.0 and not blob["drift"] and blob["n"] == blob["m"] and blob["dim"] == 32 and blob["num_samples"] == 60
    with gzip.open(out, "rt", encoding="utf-8") as f:
        records = [json.loads(line) for line in f]
    assert records == blob["outliers"] and len(records) == 3
    # an index of embeddings of another size: status 2, nothing written
    index = similar.SiteIndex.load(out_index)
    index._replace(embeddings=np.zeros((index.size, 48), np.float32), mean=np.zeros(48, np.float32), dim=48).save(tmp_path / "wrong.npz")
    other = tmp_path / "other.jsonl"
    status = T.run(T.parse_args([str(path), str(tmp_path / "wrong.npz"), str(data_dir), str(other), "--sequential"]))
    assert status == T.EXIT_DIMENSION_MISMATCH == 2 and not other.exists() and "size 48" in capsys.readouterr().err


def test_no_spread_on_the_device():
    from buglab.models import drift as T

    row = np.random.default_rng(0).standard_normal(24).astype(np.float32) * 1e3
    report = T.drift_between(np.tile(row, (5, 1)), np.tile(row, (7, 1)), DEV, 9)
    assert (report.bandwidth, report.statistic, report.p_value, report.drift) == (0.0, 0.0, 1.0, False)
