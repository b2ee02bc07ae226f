"""GPU: similar-bug search on the MI355X -- the kernels of csrc/bl_similar.hip against their NumPy twin (buglab/models/_similar.py,
which tests/test_similar_host.py pins to plain loops) bit for bit, the integer MFMA's operand map on exact data, strided and
shifted operands, outputs inside poisoned guard bands, and `index` / `query` end to end on two tiny untrained models: the device
path against `--host` byte for byte.

No tolerance anywhere: every kernel output is a copied fp32 value, an int8, an index, or an fp64 number formed by a fixed
sequence of rounded operations."""
import copy
import gzip
import json
from contextlib import contextmanager
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import similar_cases as C
from tests.guard_bands import guarded

pytestmark = pytest.mark.gpu

DEV = "cuda"
SPECS = {"gnn-mlp": {"modelName": "gnn-mlp", "hidden_state_size": 32, "num_layers": 4, "dropout_rate": 0.1},
         "seq-great": {"modelName": "seq-great", "hidden_state_size": 32, "num_layers": 2, "num_heads": 4, "intermediate_dimension_size": 96,
                       "dropout_rate": 0.1}}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _host(*tensors):
    return tuple(t.cpu().numpy() for t in tensors)


def _strided(a, pad, shift):
    """the same values as a view with row stride D + pad whose base is `shift` floats into an allocation"""
    N, D = a.shape
    flat = torch.full((shift + N * (D + pad) + 8,), 7.0, dtype=torch.float32, device=DEV)
    view = flat[shift:shift + N * (D + pad)].view(N, D + pad)[:, :D]
    view.copy_(_dev(a))
    return view


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _f64_of(g):
    """the payload of a guarded [n, 2 * w] int32 buffer as float64 [n, w]"""
    return g.view.contiguous().cpu().numpy().view(np.float64)


# ------------------------------------------------------------------------------------------------ bl_sim_quantize
def _quantize_case(D):
    x = C.with_invalid_rows(C.drawn_rows(11, D, seed=D, scale=3.0), seed=D)
    x[9] = x[8]
    return x, C.drawn_rows(1, D, seed=100 + D)[0]


def _assert_quantized(got, want, what):
    valid = want[3] > 0
    C.assert_equal_bits(got[1:], want[1:], what)                                  # q, sumsq, r: every row
    C.assert_equal_bits([got[0][valid]], [want[0][valid]], what)                  # c: the valid rows bit for bit,
    assert np.array_equal(got[0], want[0], equal_nan=True), what                  # the others NaN for NaN


@pytest.mark.parametrize("D", [1, 32, 100, 128, 320, 512])
def test_quantize_equals_the_twin_bit_for_bit(D):
    from buglab.models import hip_ops
    from buglab.models._similar import quantize_host

    x, mean = _quantize_case(D)
    want = quantize_host(x, mean)
    assert (want[3] > 0).sum() == 9 and not (want[3][[4, 7]] > 0).any() and want[1].shape[1] == (D + 63) // 64 * 64  # (row 1 is -mean)
    zeroed = quantize_host(x, np.zeros(D, np.float32))
    assert (zeroed[3] > 0).sum() == 8 and not (zeroed[3][[1, 4, 7]] > 0).any()
    _assert_quantized(_host(*hip_ops.similar_quantize(_dev(x), torch.zeros(D, device=DEV))), zeroed, (D, "zero mean: a zero row"))
    _assert_quantized(_host(*hip_ops.similar_quantize(_dev(x), _dev(mean))), want, (D, "contiguous"))
    for pad, shift in ((0, 1), (3, 0), (4, 4), (5, 3)):  # no quad is aligned; rows drift; everything aligned; neither
        _assert_quantized(_host(*hip_ops.similar_quantize(_strided(x, pad, shift), _dev(mean))), want, (D, pad, shift))
    # centring in place, also in a strided view
    for view in (_dev(x), _strided(x, 5, 3)):
        c, q, sumsq, r = hip_ops.similar_quantize(view, _dev(mean), out_c=view)
        assert c.data_ptr() == view.data_ptr()
        _assert_quantized(_host(view, q, sumsq, r), want, (D, "in place"))
    # a zero mean leaves what is centred as it is
    again = hip_ops.similar_quantize(_dev(want[0]), torch.zeros(D, device=DEV))
    _assert_quantized(_host(*again), quantize_host(want[0], np.zeros(D, np.float32)), (D, "zero mean"))
    assert again[1].cpu().numpy().tobytes() == want[1].tobytes()


@pytest.mark.parametrize("D", [1, 100, 320])
def test_quantize_outputs_sit_inside_guard_bands(D):
    from buglab.models import hip_ops
    from buglab.models._similar import quantize_host

    x, mean = _quantize_case(D)
    N, Dp = x.shape[0], (D + 63) // 64 * 64
    g_c = guarded(N, D, ld=D + 3, dtype=torch.float32, device=DEV, any_width=True)
    g_q = guarded(N, Dp, ld=Dp, dtype=torch.int8, device=DEV)
    g_s = guarded(N, 2, ld=2, dtype=torch.int32, device=DEV, lead=6, any_width=True)
    g_r = guarded(N, 2, ld=2, dtype=torch.int32, device=DEV, lead=6, any_width=True)
    assert g_q.data_ptr() % 16 == 0 and g_s.data_ptr() % 8 == 0 and g_r.data_ptr() % 8 == 0
    d_x, d_mean = _strided(x, 2, 1), _dev(mean)
    lib = hip_ops.load_library()
    rc = lib.bl_sim_quantize(d_x.data_ptr(), D + 2, d_mean.data_ptr(), N, D, g_c.data_ptr(), D + 3, g_q.data_ptr(), g_s.data_ptr(),
                             g_r.data_ptr(), _stream())
    assert rc == 0, lib.bl_last_error()
    for g, name in ((g_c, "c"), (g_q, "q"), (g_s, "sumsq"), (g_r, "r")):
        g.assert_untouched(name)
    got = (g_c.view.contiguous().cpu().numpy(), g_q.view.contiguous().cpu().numpy(), _f64_of(g_s)[:, 0], _f64_of(g_r)[:, 0])
    _assert_quantized(got, quantize_host(x, mean), D)
    rc = lib.bl_sim_quantize(d_x.data_ptr(), D + 2, d_mean.data_ptr(), N, D, g_c.data_ptr(), D + 3, g_q.data_ptr() + 4, g_s.data_ptr(),
                             g_r.data_ptr(), _stream())
    assert rc == -1 and b"16-byte aligned" in lib.bl_last_error()


# ------------------------------------------------------------------------------------------------ bl_sim_search_i8
NS = [1, 15, 16, 17, 63, 64, 65, 1000]
QS = [1, 16, 17, 50, 130]


def _search_data(kind, N, Q, D, seed):
    """int8 images and r of an index and of queries: the twin's own quantisation (the kernel's is tested above)"""
    from buglab.models._similar import quantize_host

    make = C.tie_rows if kind == "ties" else C.drawn_rows
    x = C.with_invalid_rows(make(N, D, seed), seed)
    y = C.with_invalid_rows(make(Q, D, seed + 1), seed + 1)
    if kind == "drawn" and Q > 2 and N > 2:
        y[2] = -x[0]  # and a query opposite to a row
    zero = np.zeros(D, np.float32)
    return quantize_host(y, zero), quantize_host(x, zero)


@pytest.mark.parametrize("kind", ["ties", "drawn"])
@pytest.mark.parametrize("D", [64, 100, 320])  # Dp = 64, 128, 320
def test_search_equals_the_twin_for_every_geometry(D, kind):
    """every N x Q of the grid; C in {1, 5, 16} and slices in {1, 2, 7} give identical bits: the top C is a prefix of the top 16
    under a total order, and a slice is a launch detail"""
    from buglab.models import hip_ops
    from buglab.models._similar import search_host

    for N in NS:
        for Q in QS:
            (cq, qq, sq, rq), (ci, qi, si, ri) = _search_data(kind, N, Q, D, seed=N + Q)
            want = search_host(qq, rq, qi, ri, 16)
            if N < 16:
                assert (want[0][:, N:] == -1).all()  # N < C: padded
            if Q > 7:
                assert (want[0][[1, 4, 7]] == -1).all()  # invalid queries have no neighbours
            if N > 7:
                assert not np.isin(want[0], [1, 4, 7]).any()  # invalid index rows are never candidates
            d = [_dev(a) for a in (qq, rq, qi, ri)]
            for cand_count in (1, 5, 16):
                for slices in (1, 2, 7):
                    got = _host(*hip_ops.similar_search(*d, cand_count, slices=slices))
                    C.assert_equal_bits(got, (want[0][:, :cand_count], want[1][:, :cand_count]), (kind, D, N, Q, cand_count, slices))
            C.assert_equal_bits(_host(*hip_ops.similar_search(*d, 16)), want, (kind, D, N, Q, "default slices"))
    if kind == "ties":
        assert (np.diff(want[1][0]) == 0).any()  # exact key ties are in the case


def test_search_operand_map_on_identity_queries():
    """query i is the unit vector e_i, index row j holds distinct integers per column, asymmetric in (j, d): every idot is one
    known entry, idot(i, j) = 127 * q[j, i], so a wrong A / B lane map or a transposed C / D map shows"""
    from buglab.models import hip_ops
    from buglab.models._similar import quantize_host, search_host

    for D in (64, 128, 192):
        N = 48
        j, d = np.meshgrid(np.arange(N), np.arange(D), indexing="ij")
        x = ((7 * j + 3 * d * d + d) % 127 + 1).astype(np.float32)  # 1 .. 127, not symmetric
        x[:, 5] = 127.0                                              # amax = 127 in every row: q == x
        y = np.eye(D, dtype=np.float32)
        zero = np.zeros(D, np.float32)
        (cq, qq, sq, rq), (ci, qi, si, ri) = quantize_host(y, zero), quantize_host(x, zero)
        assert qi.tobytes() == x.astype(np.int8).tobytes() and (qq == 127 * np.eye(D, dtype=np.int8)).all()
        idx, key = _host(*hip_ops.similar_search(_dev(qq), _dev(rq), _dev(qi), _dev(ri), 16, slices=2))
        for i in range(D):
            idot = 127 * x[:, i].astype(np.int64)
            expect = (idot * idot).astype(np.float64) * ri
            order = np.argsort(-expect, kind="stable")[:16]
            assert idx[i].tolist() == order.tolist() and key[i].tobytes() == expect[order].tobytes(), (D, i)
        C.assert_equal_bits((idx, key), search_host(qq, rq, qi, ri, 16), D)


def test_search_outputs_and_workspace_sit_inside_guard_bands():
    from buglab.models import hip_ops
    from buglab.models._similar import search_host

    N, Q, D, cand_count, slices = 65, 17, 100, 5, 7
    (cq, qq, sq, rq), (ci, qi, si, ri) = _search_data("drawn", N, Q, D, seed=9)
    lib = hip_ops.load_library()
    need = lib.bl_sim_search_workspace_bytes(Q, slices)
    assert need == Q * slices * 16 * 12
    g_idx = guarded(Q, cand_count, ld=cand_count, dtype=torch.int32, device=DEV, any_width=True)
    g_key = guarded(Q, 2 * cand_count, ld=2 * cand_count, dtype=torch.int32, device=DEV, lead=6, any_width=True)
    g_ws = guarded(need // 4, 1, ld=1, dtype=torch.int32, device=DEV, lead=6, any_width=True)
    d = [_dev(a) for a in (qq, rq, qi, ri)]
    rc = lib.bl_sim_search_i8(d[0].data_ptr(), d[1].data_ptr(), Q, d[2].data_ptr(), d[3].data_ptr(), N, 128, cand_count, slices,
                              g_ws.data_ptr(), need, g_idx.data_ptr(), g_key.data_ptr(), _stream())
    assert rc == 0, lib.bl_last_error()
    for g, name in ((g_idx, "out_idx"), (g_key, "out_key"), (g_ws, "workspace")):
        g.assert_untouched(name)
    C.assert_equal_bits((g_idx.view.contiguous().cpu().numpy(), _f64_of(g_key)), search_host(qq, rq, qi, ri, cand_count))
    # an empty index: every list is empty
    idx, key = hip_ops.similar_search(d[0], d[1], d[2][:0], d[3][:0], 4)
    assert (idx == -1).all() and not key.any()


# ------------------------------------------------------------------------------------------------ bl_sim_rescore
@pytest.mark.parametrize("D", [64, 100, 320])
def test_rescore_equals_the_twin_bit_for_bit(D):
    from buglab.models import hip_ops
    from buglab.models._similar import rescore_host, search_host

    for N in NS:
        for Q in QS:
            (cq, qq, sq, rq), (ci, qi, si, ri) = _search_data("drawn" if (N + Q) % 2 else "ties", N, Q, D, seed=N + Q)
            cand = search_host(qq, rq, qi, ri, 16)[0]  # rows with -1: N < 16, invalid queries
            if Q > 3:
                cand[3] = cand[3][::-1]      # another order of the same candidates
                cand[0, 1] = N               # out of range
                cand[Q - 1, 0] = min(4, N - 1)  # an invalid index row where N > 7, a repeated row elsewhere
            assert (cand == -1).any() or N >= 16
            d_cx, d_cy, d_sy, d_cand = _dev(cq), _dev(ci), _dev(si), _dev(cand)
            for k in (1, 5, 16):
                C.assert_equal_bits(_host(*hip_ops.similar_rescore(d_cx, d_cy, d_sy, d_cand, k)), rescore_host(cq, ci, si, cand, k), (D, N, Q, k))
            if (N, Q) in ((65, 17), (1000, 130)):  # strided and shifted operands: other loads, the same additions
                got = hip_ops.similar_rescore(_strided(cq, 3, 1), _strided(ci, 4, 4), d_sy, d_cand, 5)
                C.assert_equal_bits(_host(*got), rescore_host(cq, ci, si, cand, 5), (D, N, Q, "strided"))


def test_rescore_outputs_sit_inside_guard_bands():
    from buglab.models import hip_ops
    from buglab.models._similar import rescore_host, search_host

    N, Q, D, k = 65, 17, 100, 5
    (cq, qq, sq, rq), (ci, qi, si, ri) = _search_data("drawn", N, Q, D, seed=11)
    cand = search_host(qq, rq, qi, ri, 16)[0]
    g_idx = guarded(Q, k, ld=k, dtype=torch.int32, device=DEV, any_width=True)
    g_dot = guarded(Q, 2 * k, ld=2 * k, dtype=torch.int32, device=DEV, lead=6, any_width=True)
    d_cx, d_cy, d_sy, d_cand = _dev(cq), _dev(ci), _dev(si), _dev(cand)
    lib = hip_ops.load_library()
    rc = lib.bl_sim_rescore(d_cx.data_ptr(), D, Q, d_cy.data_ptr(), D, d_sy.data_ptr(), N, D, d_cand.data_ptr(), 16, k, g_idx.data_ptr(),
                            g_dot.data_ptr(), _stream())
    assert rc == 0, lib.bl_last_error()
    g_idx.assert_untouched("out_idx"), g_dot.assert_untouched("out_dot")
    C.assert_equal_bits((g_idx.view.contiguous().cpu().numpy(), _f64_of(g_dot)), rescore_host(cq, ci, si, cand, k))


# ------------------------------------------------------------------------------------------------ bl_sim_embed_sites
def test_embed_sites_equals_the_twin_inside_guard_bands():
    from buglab.models import hip_ops
    from buglab.models._similar import embed_sites_host

    flat, loc_idx, loc_off, cand_rows, h, truth = C.embed_case()
    B, D, capacity, first = 5, h.shape[1], 16, 3
    d = [_dev(a) for a in (flat, loc_idx, loc_off, cand_rows)]
    for d_h in (_dev(h), _strided(h, 3, 1)):
        for mode, skip, d_truth in (("predicted", False, None), ("predicted", True, None), ("truth", False, _dev(truth))):
            g_rows = guarded(capacity, D, ld=D, dtype=torch.float32, device=DEV, any_width=True)
            g_place = guarded(capacity, 1, ld=1, dtype=torch.int32, device=DEV, any_width=True)
            g_lp = guarded(capacity, 1, ld=1, dtype=torch.float32, device=DEV, any_width=True)
            rows, place, lp = g_rows.view, g_place.view[:, 0], g_lp.view[:, 0]
            hip_ops.similar_embed_sites(*d, d_h, rows, place, lp, first, mode=mode, truth=d_truth, skip_nobug=skip)
            hip_ops.similar_embed_sites(*d, d_h, rows, place, lp, first + B, mode=mode, truth=d_truth, skip_nobug=skip)  # the next minibatch
            g_rows.assert_untouched("out_rows"), g_place.assert_untouched("out_place"), g_lp.assert_untouched("out_logprob")
            got = _host(rows, place, lp)
            want = embed_sites_host(flat, loc_idx, loc_off, cand_rows, h, mode, truth, skip)
            for at in (first, first + B):
                C.assert_equal_bits([g[at:at + B] for g in got], want, (mode, skip, at))
            outside = np.r_[0:first, first + 2 * B:capacity]  # samples no launch owns: still the pattern
            assert (got[1][outside].view(np.uint32) == g_place.pattern).all() and (got[0][outside].view(np.uint32) == g_rows.pattern).all()
    assert want[1].tolist() == [2, -1, 0, -1, -1]  # the twin's own values are pinned in tests/test_similar_host.py
    with pytest.raises(ValueError, match="do not fit"):
        hip_ops.similar_embed_sites(*d, d_h, rows, place, lp, capacity - B + 1)


# ------------------------------------------------------------------------------------------------ end to end
@contextmanager
def _deterministic():
    from buglab.models import hip_ops

    was = bool(hip_ops.load_library().bl_get_deterministic())
    hip_ops.set_deterministic(True)
    try:
        yield
    finally:
        hip_ops.set_deterministic(was)


@pytest.fixture(scope="module")
def untrained(tmp_path_factory):
    """family -> (model, module, indexed pool, queried data, checkpoint path): seeded weights, no training; 60 + 60 synthetic
    samples, about half of each with a bug"""
    from buglab.data.synthetic import make_report_dataset
    from buglab.models.modelregistry import load_model
    from buglab.runtime.neuralmodel import AbstractNeuralModel

    out = {}
    for family, spec in SPECS.items():
        kind = "seq" if family.startswith("seq") else "graph"
        pool, data = make_report_dataset(60, seed=18, kind=kind), make_report_dataset(60, seed=17, kind=kind)
        path = tmp_path_factory.mktemp("similar_" + family.replace("-", "_")) / "detector.pkl.gz"
        model = load_model(dict(spec), path)[0]
        model.compute_metadata(copy.deepcopy(pool + data))
        torch.manual_seed(5)
        model.save(path, model.build_neural_module())
        out[family] = AbstractNeuralModel.restore_model(Path(path), torch.device(DEV)) + (pool, data, path)
    return out


def _same_index(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a[:9], b[:9])) and a[9:] == b[9:]


def _records(found):
    return json.dumps([f.record() for f in found], sort_keys=True)


@pytest.mark.parametrize("family", list(SPECS))
def test_index_then_query_on_the_device_equals_the_host_path(family, untrained):
    from buglab.models import similar as T

    model, nn_, pool, data, _ = untrained[family]
    device = torch.device(DEV)
    with _deterministic():
        num_buggy = sum(p["target_fix_action_idx"] is not None for p in pool)
        index = T.build_site_index(model, nn_, pool, device, "truth", "known-bug", parallelize=False)
        on_host = T.build_site_index(model, nn_, pool, device, "truth", "known-bug", host=True, parallelize=False)
        assert _same_index(index, on_host) and index.size == num_buggy and 10 < num_buggy < 60 and index.dim == 32
        assert set(index.tags.tolist()) == {"known-bug"} and all(index.scouts.tolist()) and np.isfinite(index.embeddings).all()
        assert np.unique(index.embeddings, axis=0).shape[0] > 5  # the model tells sites apart
        plain = T.build_site_index(model, nn_, pool, device, "predicted", None, False, assume_buggy=True, parallelize=False)
        assert _same_index(plain, T.build_site_index(model, nn_, pool, device, "predicted", None, False, assume_buggy=True, host=True,
                                                     parallelize=False))
        assert plain.size == 60 and not plain.mean.any() and not any(plain.scouts.tolist())

        for options in (dict(site="predicted", assume_buggy=True), dict(site="predicted"), dict(site="truth", min_similarity=0.2)):
            a = T.search_similar(model, nn_, index, data, device, 5, 16, parallelize=False, **options)
            b = T.search_similar(model, nn_, index, data, device, 5, 16, host=True, parallelize=False, **options)
            assert _records(a.found) == _records(b.found) and a.summary == b.summary, options
            positions = [f.position for f in a.found]
            assert positions == sorted(positions) and a.summary["num_samples"] == 60 and a.summary["num_rejected"] == 0
            assert a.summary["num_with_site"] == len(a.found) == 60 - a.summary["num_without_site"]
            for f in a.found:
                sims = [n["similarity"] for n in f.neighbours]
                assert sims == sorted(sims, reverse=True) and len(sims) <= 5 and all(-1.0 <= s <= 1.0 for s in sims)
        assert len(a.found) == sum(p["target_fix_action_idx"] is not None for p in data) and "labelled" in a.summary
        everyone = T.search_similar(model, nn_, index, data, device, 5, 16, site="predicted", assume_buggy=True, parallelize=False)
        assert len(everyone.found) == 60 and all(len(f.neighbours) == 5 for f in everyone.found)
        assert _records(T.find_similar(model, nn_, index, data, device, 5, 16, site="predicted", assume_buggy=True, parallelize=False)) \
            == _records(everyone.found)
        # a stream of unknown length, collated in worker threads: the buffers grow on the device
        grown = T.search_similar(model, nn_, index, (p for p in data), device, 5, 16, site="predicted", assume_buggy=True, capacity=1)
        assert _records(grown.found) == _records(everyone.found)
        # fewer candidates: still the device equals the host, and k == C is allowed
        few = T.search_similar(model, nn_, index, data, device, 3, 3, site="truth", parallelize=False)
        assert _records(few.found) == _records(T.search_similar(model, nn_, index, data, device, 3, 3, site="truth", host=True,
                                                                parallelize=False).found)

        # the indexed data itself, in the same order: every sample finds its own entry first, or an entry with the identical
        # embedding at a lower index, at a similarity of exactly 1.0 (dot == sumsq bitwise, and sqrt(s * s) == s)
        own = T.search_similar(model, nn_, index, pool, device, 1, 16, site="truth", parallelize=False)
        assert len(own.found) == index.size
        for entry, f in enumerate(own.found):
            first = f.neighbours[0]
            assert first["similarity"] == 1.0 and first["position"] <= f.position, (entry, first)
            assert first["entry"] == entry or (first["entry"] < entry
                                               and index.embeddings[first["entry"]].tobytes() == index.embeddings[entry].tobytes())
        assert own.summary["labelled"]["top1_same_scout"] > 0.5 and own.summary["top1_similarity"]["min"] == 1.0


def test_command_line_index_then_query(untrained, tmp_path, capsys):
    from buglab.models import similar as T
    from buglab.models._similar import SiteIndex
    from buglab.runtime.neuralmodel import AbstractNeuralModel
    from buglab.utils.msgpackutils import load_all_msgpack_l_gz, save_msgpack_l_gz

    _, _, pool, data, path = untrained["gnn-mlp"]
    pool_dir, data_dir = tmp_path / "pool", tmp_path / "data"
    pool_dir.mkdir(), data_dir.mkdir()
    save_msgpack_l_gz(pool, pool_dir / "x.msgpack.l.gz"), save_msgpack_l_gz(data, data_dir / "x.msgpack.l.gz")
    out_index, out, report = tmp_path / "bugs.npz", tmp_path / "similar.jsonl.gz", tmp_path / "report.json"
    with _deterministic():
        assert T.run(T.parse_args(["index", str(path), str(pool_dir), str(out_index), "--tag", "known-bug", "--sequential"])) == 0
        assert "similar index:" in capsys.readouterr().out
        index = SiteIndex.load(out_index)
        model, nn_ = AbstractNeuralModel.restore_model(path, torch.device(DEV))
        read_back = list(load_all_msgpack_l_gz(pool_dir))
        assert _same_index(index, T.build_site_index(model, nn_, read_back, DEV, "truth", "known-bug", parallelize=False))
        args = ["query", str(path), str(out_index), str(data_dir), str(out), "--top-k", "3", "--assume-buggy", "--report-json", str(report),
                "--sequential"]
        assert T.run(T.parse_args(args)) == 0
        text = capsys.readouterr().out
        with gzip.open(out, "rt", encoding="utf-8") as f:
            records = [json.loads(line) for line in f]
        want = T.search_similar(model, nn_, index, list(load_all_msgpack_l_gz(data_dir)), DEV, 3, 16, assume_buggy=True, parallelize=False)
        assert records == json.loads(_records(want.found)) and [r["position"] for r in records] == list(range(60))
        assert all(len(r["neighbours"]) == 3 and r["neighbours"][0]["tag"] == "known-bug" for r in records)
        blob = json.loads(report.read_text(encoding="utf-8"))
        assert blob == json.loads(json.dumps(want.summary))
        assert (blob["num_samples"], blob["num_with_site"], blob["num_rejected"], blob["num_invalid_embeddings"]) == (60, 60, 0, 0)
        assert "60 of 60 samples have a site" in text
        # an index of embeddings of another size: status 2, nothing written
        wrong = index._replace(embeddings=np.zeros((index.size, 48), np.float32), mean=np.zeros(48, np.float32), dim=48)
        wrong.save(tmp_path / "wrong.npz")
        other = tmp_path / "other.jsonl"
        status = T.run(T.parse_args(["query", str(path), str(tmp_path / "wrong.npz"), str(data_dir), str(other), "--sequential"]))
        assert status == T.EXIT_DIMENSION_MISMATCH == 2 and not other.exists() and "size 48" in capsys.readouterr().err


def test_other_weights_are_a_warning(untrained, caplog):
    import logging

    from buglab.models import similar as T

    model, nn_, pool, data, _ = untrained["gnn-mlp"]
    index = T.build_site_index(model, nn_, pool[:20], DEV, "truth", parallelize=False)
    with caplog.at_level(logging.WARNING, logger="buglab.models.similar"):
        T.search_similar(model, nn_, index, data[:5], DEV, 1, 4, assume_buggy=True, parallelize=False)
        assert not caplog.records
        T.search_similar(model, nn_, index._replace(fingerprint="0" * 40), data[:5], DEV, 1, 4, assume_buggy=True, parallelize=False)
    assert any("other weights" in r.getMessage() for r in caplog.records)
