"""GPU: warning triage on the MI355X -- the kernels of csrc/bl_triage.hip against their NumPy twin (buglab/models/_triage.py, which
tests/test_triage_host.py holds against autograd): counts equal, margins bit for bit, probabilities within 8 ulp, every entry of
H, g and L under the any-order summation bound, H == H^T and two runs bit for bit; strided operands and outputs inside poisoned
guard bands; the device fit against the twin's through the same driver; and `rank_warnings` on two tiny untrained models, the
device path against `host=True`.

The bounds are derived, not measured (tests/triage_cases.py::summation_bound; the 8 ulp: ocml's and libm's fp64 exp are each
specified to 1 ulp, the sum and the quotient add under 2 more, 8 leaves a factor of two)."""
import numpy as np
import pytest
import torch

from tests import triage_cases as C
from tests.guard_bands import guarded
from tests.test_similar_gpu import DEV, _deterministic, _dev, _stream, untrained  # noqa: F401  (untrained: a fixture)

pytestmark = pytest.mark.gpu


def _operands(p, c):
    d = {k: _dev(v) for k, v in p.items()}
    d["c"] = None if c is None else _dev(np.asarray(c, np.float64))
    return d


def _device(p, c, x=None):
    """(H, g, scalars, margin, probability) of the device for a problem of tests/triage_cases.py, as arrays"""
    from buglab.models import hip_ops

    d = _operands(p, c)
    x = d["x"] if x is None else x
    P = p["x"].shape[1] + 2
    blob = hip_ops.triage_newton_stats(x, d["logprob"], d["shift"], d["scale"], d["w"], d["y"], d["c"], C.L2).cpu().numpy()
    both = hip_ops.triage_score(x, d["logprob"], d["shift"], d["scale"], d["w"]).cpu().numpy()
    return blob[:P * P].reshape(P, P), blob[P * P:P * P + P], blob[P * P + P:], both[0], both[1]


def _check(got, twin, where):
    p, c, st, (abs_h, abs_g, abs_l), (z, prob) = twin
    H, g, scalars, margin, probability = got
    N = p["x"].shape[0]
    assert (int(scalars[2]), int(scalars[3])) == (st.used, st.skipped) and scalars[2] + scalars[3] == N, where
    assert margin.tobytes() == z.tobytes(), (where, "margins")  # NaN rows included
    ok = ~np.isnan(z)
    assert (np.isnan(probability) == ~ok).all() and (C.ulps_apart(probability[ok], prob[ok]) <= 8).all(), (where, "probabilities")
    assert (H == H.T).all() and np.isfinite(H).all() and np.isfinite(g).all(), where
    assert (np.abs(H - st.H) <= C.summation_bound(N, abs_h)).all(), (where, "H", float(np.abs(H - st.H).max()))
    assert (np.abs(g - st.g) <= C.summation_bound(N, abs_g)).all(), (where, "g", float(np.abs(g - st.g).max()))
    assert abs(scalars[0] - st.L) <= C.summation_bound(N, abs_l), (where, "L")
    assert abs(scalars[1] - st.csum) <= C.summation_bound(N, st.csum), (where, "sum of c")


@pytest.mark.parametrize("weighting", C.WEIGHTINGS)
@pytest.mark.parametrize("N,D", C.STAT_SHAPES)
def test_statistics_and_scores_equal_the_twin(N, D, weighting):
    twin = C.twin_stats(N, D, weighting)
    first = _device(twin[0], twin[1])
    _check(first, twin, (N, D, weighting))
    again = _device(twin[0], twin[1])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again)), "two runs differ"


@pytest.mark.parametrize("kind", C.HARD_CASES)
def test_hard_cases_equal_the_twin(kind):
    twin = C.twin_hard(kind)
    p, c, st, _, (z, prob) = twin
    got = _device(p, c)
    _check(got, twin, kind)
    if kind == "non_finite":
        assert (st.used, st.skipped) == (997, 3) and np.isnan(got[3][[5, 129, 700]]).all() and np.isnan(got[3]).sum() == 3
    if kind == "far_margins":
        far = np.abs(z) > 750.0
        assert far.any() and np.isfinite(got[2][0]) and set(got[4][far].tolist()) <= {0.0, 1.0}
    if kind == "zero_slice":  # the slice contributes exactly nothing: the same bits as with its rows' labels flipped
        flipped = dict(p, y=np.where((np.arange(1000) >= 256) & (np.arange(1000) < 384), 1 - p["y"], p["y"]).astype(np.uint8))
        other = _device(flipped, c)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got[:3], other[:3]))


def _f64_payload(g):
    return g.view.contiguous().cpu().numpy().view(np.float64).reshape(-1)


@pytest.mark.parametrize("shift", [0, 1])
def test_strided_operands_and_outputs_inside_guard_bands(shift):
    """ldx > D with NaN in the padding, every output and the workspace inside guard bands: nothing outside is written and the
    results are those of the contiguous call bit for bit.  shift 1: a base that is 4-byte aligned and no more (the scalar loads)."""
    from buglab.models import hip_ops

    N, D = 130, 62  # P = 64, two slices
    P = D + 2
    twin = C.twin_stats(N, D, "balance")
    p, c = twin[0], twin[1]
    want = _device(p, c)
    d = _operands(p, c)
    ld = D + (6 if shift == 0 else 5)  # 68 floats: rows stay 16-byte aligned; 67: nothing is
    g_x = guarded(N, D, ld=ld, dtype=torch.float32, device=DEV, lead=4 + shift, any_width=True)
    g_x.view.copy_(d["x"])
    assert g_x.data_ptr() % 16 == (0 if shift == 0 else 4)
    lib = hip_ops.load_library()
    need = hip_ops.triage_workspace_bytes(N, D)
    g_ws = guarded(1, need // 4, ld=need // 4, dtype=torch.int32, device=DEV, any_width=True)
    g_h = guarded(P, 2 * P, ld=2 * P, dtype=torch.int32, device=DEV, any_width=True)
    g_g = guarded(1, 2 * P, ld=2 * P, dtype=torch.int32, device=DEV, any_width=True)
    g_s = guarded(1, 8, ld=8, dtype=torch.int32, device=DEV, any_width=True)
    g_m = guarded(1, 2 * N, ld=2 * N, dtype=torch.int32, device=DEV, any_width=True)
    g_p = guarded(1, 2 * N, ld=2 * N, dtype=torch.int32, device=DEV, any_width=True)
    assert all(g.data_ptr() % 8 == 0 for g in (g_ws, g_h, g_g, g_s, g_m, g_p))
    rc = lib.bl_triage_newton_stats(g_x.data_ptr(), ld, d["logprob"].data_ptr(), d["shift"].data_ptr(), d["scale"].data_ptr(),
                                    d["w"].data_ptr(), d["y"].data_ptr(), d["c"].data_ptr(), N, D, C.L2, g_ws.data_ptr(), need,
                                    g_h.data_ptr(), g_g.data_ptr(), g_s.data_ptr(), _stream())
    assert rc == 0, lib.bl_last_error()
    rc = lib.bl_triage_score(g_x.data_ptr(), ld, d["logprob"].data_ptr(), d["shift"].data_ptr(), d["scale"].data_ptr(), d["w"].data_ptr(),
                             N, D, g_m.data_ptr(), g_p.data_ptr(), _stream())
    assert rc == 0, lib.bl_last_error()
    for g, name in ((g_x, "x"), (g_ws, "workspace"), (g_h, "H"), (g_g, "g"), (g_s, "scalars"), (g_m, "margin"), (g_p, "prob")):
        g.assert_untouched(name)
    got = (_f64_payload(g_h).reshape(P, P), _f64_payload(g_g), _f64_payload(g_s), _f64_payload(g_m), _f64_payload(g_p))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want)), [a.tobytes() == b.tobytes() for a, b in zip(got, want)]
    # the wrapper takes the strided view as it is
    via = _device(p, c, x=g_x.view)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(via, want))


def test_no_rows_and_argument_errors():
    from buglab.models import hip_ops

    lib = hip_ops.load_library()
    g_out = guarded(1, 2 * (36 + 6 + 4), ld=2 * 46, dtype=torch.int32, device=DEV, any_width=True)
    base = g_out.data_ptr()
    z = torch.zeros(8, dtype=torch.float64, device=DEV)
    rc = lib.bl_triage_newton_stats(None, 4, None, z.data_ptr(), z.data_ptr(), z.data_ptr(), None, None, 0, 4, 1.0, None, 0, base, base + 8 * 36,
                                    base + 8 * 42, _stream())
    assert rc == 0 and not _f64_payload(g_out).any()  # N == 0: zeros written
    g_out.assert_untouched("outputs of an empty call")
    empty = hip_ops.triage_newton_stats(torch.zeros((0, 4), device=DEV), torch.zeros(0, device=DEV), z[:5], z[:5], z[:6],
                                        torch.zeros(0, dtype=torch.uint8, device=DEV), None, 1.0)
    assert empty.shape == (46,) and not empty.any()
    assert hip_ops.triage_score(torch.zeros((0, 4), device=DEV), torch.zeros(0, device=DEV), z[:5], z[:5], z[:6]).shape == (2, 0)
    x = torch.zeros((4, 4), device=DEV)
    with pytest.raises(RuntimeError, match="workspace"):
        hip_ops.triage_newton_stats(x, x[:, 0].contiguous(), z[:5], z[:5], z[:6], torch.zeros(4, dtype=torch.uint8, device=DEV), None, 1.0,
                                    workspace=torch.zeros(3, dtype=torch.float64, device=DEV))


# ------------------------------------------------------------------------------------------------ the fit
@pytest.mark.parametrize("N,D,seed", [(2000, 64, 31), (600, 30, 32)])
def test_the_device_fit_equals_the_twins(N, D, seed):
    from buglab.models import _triage as R
    from buglab.models import triage as T

    x, lp, y = C.learnable(N, D, seed, noise=0.7)
    on_host = T.fit_triage_embeddings(x, lp, y, host=True)
    on_device = T.fit_triage_embeddings(x, lp, y, device=DEV)
    losses = sorted(entry["log_loss"] for entry in on_host.report["cv"])
    assert (losses[1] - losses[0]) > 1e-6 * losses[0]  # the choice of l2 is not a coin toss
    assert on_device.model.l2 == on_host.model.l2 and on_device.model.converged and on_host.model.converged
    assert on_device.report["all_folds_converged"] and on_host.report["all_folds_converged"] and on_device.report["path"] == "device"
    # L is l2-strongly convex over the regularised coordinates: |w_a - w_b| <= |g(w_a) - g(w_b)| / l2 <= (|g(w_a)| + |g(w_b)|) / l2,
    # with g recomputed by the twin at both points.  The intercept is not regularised: for it the smallest eigenvalue of the
    # twin's H at the twin's solution stands in place of l2 (the two points are some 1e-10 apart, H does not move between them).
    l2 = on_host.model.l2
    problem = R.HostProblem(x, lp, y, on_host.model.shift, on_host.model.scale)
    g_dev, st_host = problem.stats(on_device.model.w, None, l2).g, problem.stats(on_host.model.w, None, l2)
    gsum = float(np.linalg.norm(g_dev) + np.linalg.norm(st_host.g))
    diff = on_device.model.w - on_host.model.w
    print(f"|dw| regularised {np.linalg.norm(diff[:-1]):.3e}, intercept {abs(diff[-1]):.3e}, |g| sum {gsum:.3e}, l2 {l2:g}, "
          f"smallest eigenvalue {np.linalg.eigvalsh(st_host.H)[0]:.3e}")
    assert np.linalg.norm(diff[:-1]) <= gsum / l2
    assert abs(diff[-1]) <= gsum / float(np.linalg.eigvalsh(st_host.H)[0])
    assert (on_device.model.shift.tobytes(), on_device.model.scale.tobytes()) == (on_host.model.shift.tobytes(), on_host.model.scale.tobytes())


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("family", ["gnn-mlp", "seq-great"])
def test_rank_warnings_on_the_device_equals_the_host_path(family, untrained):  # noqa: F811
    from buglab.models import triage as T

    model, nn_, pool, data, _ = untrained[family]
    device = torch.device(DEV)
    with _deterministic():
        half = len(pool) // 2
        report = {}
        common = dict(site="predicted", assume_buggy=True, min_per_class=10, parallelize=False)
        fitted = T.fit_triage(model, nn_, pool[:half], pool[half:], device, report=report, **common)
        on_host = T.fit_triage(model, nn_, pool[:half], pool[half:], device, host=True, **common)
        assert fitted.dim == 32 and (fitted.num_accepted, fitted.num_dismissed) == (half, len(pool) - half) and report["path"] == "device"
        assert fitted.l2 == on_host.l2 and fitted.converged and on_host.converged
        assert fitted.shift.tobytes() == on_host.shift.tobytes() and fitted.fingerprint == on_host.fingerprint

        # no two probabilities closer than 1e-9: samples that are (near) copies of an earlier one are left out of the scan
        every = T.rank_scan(model, nn_, fitted, data, device, assume_buggy=True, host=True, parallelize=False)
        assert every.summary["num_warnings"] == len(data) == len(every.warnings)
        probs = np.asarray([w.triage_probability for w in every.warnings])
        keep_positions = sorted(w.position for i, w in enumerate(every.warnings) if i == 0 or probs[i - 1] - probs[i] > 1e-9)
        scan = [data[i] for i in keep_positions]
        assert len(scan) > 30
        a = T.rank_scan(model, nn_, fitted, scan, device, assume_buggy=True, parallelize=False)
        b = T.rank_scan(model, nn_, fitted, scan, device, assume_buggy=True, host=True, parallelize=False)
        pb = np.asarray([w.triage_probability for w in b.warnings])
        assert (-np.diff(pb)).min() > 1e-9
        assert [w.position for w in a.warnings] == [w.position for w in b.warnings] and sorted(w.position for w in a.warnings) == list(range(len(scan)))
        assert [w[:6] for w in a.warnings] == [w[:6] for w in b.warnings]  # position, node, label, filename, package, logprob
        assert [w.margin for w in a.warnings] == [w.margin for w in b.warnings]  # bit for bit
        assert (C.ulps_apart([w.triage_probability for w in a.warnings], pb) <= 8).all()
        assert a.summary["probability_histogram"] == b.summary["probability_histogram"] and a.summary["num_listed"] == len(scan)
        assert T.rank_warnings(model, nn_, fitted, scan, device, assume_buggy=True, top_k=5, parallelize=False) == a.warnings[:5]
        # without --assume-buggy a winning NO_BUG is no warning; filters drop, the order stays
        plain = T.rank_scan(model, nn_, fitted, scan, device, min_triage_probability=0.5, parallelize=False)
        assert plain.summary["num_warnings"] + plain.summary["num_without_site"] == len(scan)
        assert all(w.triage_probability >= 0.5 for w in plain.warnings)


def test_an_ensemble_is_refused(untrained):  # noqa: F811
    from buglab.models import triage as T
    from buglab.models.ensemble.wrapper import EnsembleWrapper

    model, nn_, pool, data, _ = untrained["gnn-mlp"]
    ensemble = EnsembleWrapper.__new__(EnsembleWrapper)  # `require_single_model` looks at the type
    with pytest.raises(TypeError, match="ensembles"):
        T.rank_warnings(ensemble, nn_, None, data, DEV)
    with pytest.raises(TypeError, match="ensembles"):
        T.fit_triage(ensemble, nn_, pool, pool, DEV)
