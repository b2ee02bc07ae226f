"""CPU: similar-bug search without a GPU -- the NumPy twin of csrc/bl_similar.hip (buglab/models/_similar.py) against the plain
loops of tests/similar_cases.py bit for bit, the two-stage search against exact fp64 brute force on data for which the int8
stage must not lose a neighbour, the index file, and the refusals of the drivers and the launchers.

No tolerance on the twin.  The brute-force comparison is a condition on the inputs (clustered rows, queries near a row), not
a measurement: the first 16 coarse candidates hold the exact top 5 of every query."""
import logging

import numpy as np
import pytest

from tests import similar_cases as C


# ------------------------------------------------------------------------------------------------ the twin
@pytest.mark.parametrize("D", [1, 3, 32, 100, 130])
def test_quantize_twin_equals_the_loops(D):
    from buglab.models._similar import quantize_host

    x = C.with_invalid_rows(C.drawn_rows(11, D, seed=D, scale=3.0), seed=D)
    assert not np.isfinite(x[4]).all() and not np.isfinite(x[7]).all() and not x[1].any()
    x[9] = x[8]  # a duplicate row
    x[10, 0] = 0.5  # a tie of the rounding: 0.5 * 127 / amax lands on a half where amax is a power of two
    mean = C.drawn_rows(1, D, seed=100 + D)[0]
    for m in (mean, np.zeros(D, np.float32)):
        got, want = quantize_host(x, m), C.quantize_ref(x, m)
        valid = want[3] > 0
        C.assert_equal_bits([g[valid] for g in got], [w[valid] for w in want], (D, "valid rows"))
        C.assert_equal_bits(got[1:], want[1:], (D, "q, sumsq, r"))
        assert np.array_equal(got[0], want[0], equal_nan=True)
        assert got[1].shape == (11, (D + 63) // 64 * 64) and not got[1][:, D:].any()
        if m is not mean:
            assert valid.tolist() == [True, False, True, True, False, True, True, False, True, True, True]
            assert not got[1][~valid].any() and not got[2][~valid].any() and np.abs(got[1][valid]).max(axis=1).tolist() == [127] * 8


def test_quantize_rounds_half_to_even_and_rules_stated_once():
    from buglab.models._similar import quantize_host

    # amax = 127: the scale is exactly 1, so the values are rounded as they are
    x = np.array([[127.0, 0.5, 1.5, 2.5, -0.5, -1.5, 126.5, -126.5]], np.float32)
    c, q, sumsq, r = quantize_host(x, np.zeros(8, np.float32))
    assert q[0, :8].tolist() == [127, 0, 2, 2, 0, -2, 126, -126] and q.shape == (1, 64) and q.dtype == np.int8
    assert sumsq[0] == float((x.astype(np.float64) ** 2).sum()) and r[0] == 127.0 * 127.0 / sumsq[0]
    # centring is one rounded fp64 difference, rounded to fp32
    c, _, _, _ = quantize_host(np.array([[1.0, 1e-8]], np.float32), np.array([1e-8, 1.0], np.float32))
    assert c.tolist() == [[np.float32(1.0 - np.float64(np.float32(1e-8))), np.float32(np.float64(np.float32(1e-8)) - 1.0)]]


def _images(x, y, mean=None):
    from buglab.models._similar import quantize_host

    mean = np.zeros(x.shape[1], np.float32) if mean is None else mean
    return quantize_host(y, mean), quantize_host(x, mean)


@pytest.mark.parametrize("D", [1, 3, 32, 100, 130])
@pytest.mark.parametrize("kind", ["ties", "drawn"])
def test_search_and_rescore_twins_equal_the_loops(kind, D):
    from buglab.models._similar import rescore_host, search_host

    make = C.tie_rows if kind == "ties" else C.drawn_rows
    x = C.with_invalid_rows(make(23, D, seed=3 * D), seed=D)             # the index: rows 1, 4, 7 invalid
    y = C.with_invalid_rows(make(9, D, seed=3 * D + 1), seed=D + 1)      # the queries: likewise
    y[8] = -x[0] if kind == "drawn" else y[8]
    (cq, qq, sq, rq), (ci, qi, si, ri) = _images(x, y)
    for cand_count in (1, 5, 16):
        got, want = search_host(qq, rq, qi, ri, cand_count), C.search_ref(qq, rq, qi, ri, cand_count)
        C.assert_equal_bits(got, want, (kind, D, cand_count))
        assert (got[0][[1, 4, 7]] == -1).all() and not np.isin(got[0], [1, 4, 7]).any()  # invalid queries, invalid index rows
    cand = got[0].copy()
    if kind == "ties" and D >= 3:
        keys = got[1][0]
        assert (np.diff(keys) <= 0).all() and (np.diff(got[0][0])[np.diff(keys) == 0] > 0).all()  # among equal keys the index ascends
    cand[0, 3], cand[2, 0], cand[3] = -1, 23, cand[3][::-1]  # a hole, an index out of range, another order of the same candidates
    cand[5, 1] = 4                                            # an invalid index row
    for k in (1, 5, 16):
        C.assert_equal_bits(rescore_host(cq, ci, si, cand, k), C.rescore_ref(cq, ci, si, cand, k), (kind, D, k))
    a, b = rescore_host(cq, ci, si, cand, 16), rescore_host(cq, ci, si, got[0], 16)
    assert a[0][3].tolist() == b[0][3].tolist()  # the order of the candidates does not matter where no two are the same row


def test_search_special_cases():
    from buglab.models._similar import quantize_host, rescore_host, search_host, similarity

    # a query opposite to every row: all keys negative, the least negative first; N < C pads with -1; k < C
    x = np.array([[1, 0, 0], [1, 1, 0], [1, 1, 1], [2, 2, 2]], np.float32)
    y = np.array([[-1, -1, -1]], np.float32)
    (cq, qq, sq, rq), (ci, qi, si, ri) = _images(x, y)
    idx, key = search_host(qq, rq, qi, ri, 16)
    assert idx[0].tolist() == [0, 1, 2, 3] + [-1] * 12 and (key[0, :4] < 0).all() and key[0, 2] == key[0, 3] and not key[0, 4:].any()
    C.assert_equal_bits((idx, key), C.search_ref(qq, rq, qi, ri, 16))
    top, dot = rescore_host(cq, ci, si, idx, 2)
    assert top[0].tolist() == [0, 1] and dot[0].tolist() == [-1.0, -2.0]
    assert similarity(dot, sq[:, None], si[top]).tolist() == [[-1.0 / np.sqrt(3.0), -2.0 / np.sqrt(6.0)]]
    # the product idot |idot| does not fit int32: 127 * 127 * 512 squared is about 7e13
    big = np.ones((1, 512), np.float32)
    _, q, _, r = quantize_host(big, np.zeros(512, np.float32))
    idx, key = search_host(q, r, q, r, 1)
    assert idx.tolist() == [[0]] and key[0, 0] == float((127 * 127 * 512) ** 2) * r[0] and key[0, 0] > 2.0 ** 31
    # nothing to search, and no valid row to find
    idx, key = search_host(q, r, np.zeros((0, 512), np.int8), np.zeros(0), 3)
    assert idx.tolist() == [[-1, -1, -1]] and rescore_host(big, np.zeros((0, 512), np.float32), np.zeros(0), idx, 2)[0].tolist() == [[-1, -1]]
    with pytest.raises(ValueError):
        search_host(q, r, q, r, 17)
    with pytest.raises(ValueError):
        rescore_host(big, big, np.ones(1), np.zeros((1, 4), np.int32), 5)


def test_embed_sites_twin_on_the_handmade_case():
    from buglab.models._similar import embed_sites_host

    flat, loc_idx, loc_off, cand_rows, h, truth = C.embed_case()
    rows, place, logprob = embed_sites_host(flat, loc_idx, loc_off, cand_rows, h, "predicted")
    assert place.tolist() == [1, -1, 2, -1, -1] and logprob.tolist() == [-0.5, 0.0, -2.0, 0.0, 0.0]
    assert rows[0].tobytes() == h[0].tobytes() and rows[2].tobytes() == h[4].tobytes() and not rows[[1, 3, 4]].any()
    rows, place, logprob = embed_sites_host(flat, loc_idx, loc_off, cand_rows, h, "predicted", skip_nobug=True)
    assert place.tolist() == [1, 0, 2, -1, -1] and rows[1].tobytes() == h[2].tobytes() and logprob[1] == -1.5
    rows, place, logprob = embed_sites_host(flat, loc_idx, loc_off, cand_rows, h, "truth", truth)
    assert place.tolist() == [2, -1, 0, -1, -1] and rows[0].tobytes() == h[5].tobytes() and rows[2].tobytes() == h[1].tobytes()
    assert np.isnan(logprob[2]) and logprob[0] == -0.5
    with pytest.raises(ValueError):
        embed_sites_host(flat, loc_idx, loc_off, cand_rows, h, "likely")


# ------------------------------------------------------------------------------------------------ two stages against brute force
@pytest.mark.parametrize("center", [False, True])
@pytest.mark.parametrize("D,offset", [(32, 0.0), (128, 0.0), (128, 3.0), (256, 3.0)])
def test_two_stage_search_equals_exact_brute_force(D, offset, center):
    """rows = standard normal plus a shared offset per column, queries = a drawn row plus 0.7 x standard normal; N = 20000,
    Q = 200: the first 16 coarse candidates contain the exact top 5 of every query, so the re-scored neighbours ARE the exact
    top 5, with the exact cosines"""
    from buglab.models import _similar as S

    N, Q, k, cand_count = 20000, 200, 5, 16
    rng = np.random.default_rng(D + int(offset))
    base = rng.standard_normal(D) * offset
    x = (rng.standard_normal((N, D)) + base).astype(np.float32)
    y = (x[rng.integers(0, N, Q)] + 0.7 * rng.standard_normal((Q, D))).astype(np.float32)
    mean = S.column_mean(x) if center else np.zeros(D, np.float32)
    index_c = S.centre(x, mean)
    cx, qx, sx, rx = S.quantize_host(y, mean)
    cy, qy, sy, ry = S.quantize_host(index_c, np.zeros(D, np.float32))
    assert cy.tobytes() == index_c.tobytes()  # centring what is centred with a zero mean changes nothing
    cand, _ = S.search_host(qx, rx, qy, ry, cand_count)
    exact, cos = C.brute_force_top(cy, cx, k)
    assert all(set(exact[i]) <= set(cand[i]) for i in range(Q))
    idx, dot, sx2, sy2 = S.find_neighbours_host(y, mean, index_c, k, cand_count)
    assert sx2.tobytes() == sx.tobytes() and sy2.tobytes() == sy.tobytes()
    assert idx.tolist() == exact.tolist()
    sim = S.similarity(dot, sx[:, None], sy[idx])
    assert np.abs(sim - cos).max() < 1e-13 and (np.diff(sim, axis=1) <= 0).all()  # fp64 sums of <= 256 terms against BLAS


# ------------------------------------------------------------------------------------------------ file and metadata
def _sites(n=7, D=5, seed=0):
    from buglab.models._similar import SiteEmbeddings

    rows = C.drawn_rows(n, D, seed) + 2.0
    return SiteEmbeddings(rows, np.arange(n, dtype=np.int64) * 3, np.arange(n, dtype=np.int32) + 10, -np.arange(n, dtype=np.float32),
                          [f"label{i}" for i in range(n)], [f"pkg/f{i}.py" for i in range(n)], ["pkg"] * n,
                          ["" if i % 2 else "VariableMisuse" for i in range(n)], 9, 1, 1)


def test_index_round_trip_and_model_checks(tmp_path, caplog):
    from buglab.models import _similar as S

    sites = _sites()
    index = S.make_index(sites, "known-bug", True, "GnnBugLabModel", "ab" * 20)
    assert index.mean.dtype == np.float32 and index.mean.tobytes() == sites.rows.astype(np.float64).mean(0).astype(np.float32).tobytes()
    assert index.embeddings.tobytes() == (sites.rows.astype(np.float64) - index.mean.astype(np.float64)).astype(np.float32).tobytes()
    plain = S.make_index(sites, None, False, "GnnBugLabModel", "ab" * 20)
    assert not plain.mean.any() and plain.embeddings.tobytes() == sites.rows.tobytes() and plain.tags.tolist() == [""] * 7
    path = tmp_path / "sites.npz"
    index.save(path)
    assert path.exists() and not (tmp_path / "sites.npz.npz").exists()
    back = S.SiteIndex.load(path)
    for a, b in zip(index[:9], back[:9]):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    assert back[9:] == index[9:] == ("GnnBugLabModel", 5, "ab" * 20) and back.size == 7
    assert back.entry(2) == {"entry": 2, "position": 6, "node": 12, "label": "label2", "filename": "pkg/f2.py", "package": "pkg",
                             "scout": "VariableMisuse", "tag": "known-bug"}
    with np.load(path, allow_pickle=False) as z:  # nothing in the file needs pickle
        assert set(z.files) >= {"embeddings", "mean", "positions", "nodes", "labels", "paths", "packages", "scouts", "tags"}
    # an empty index travels too
    empty = S.make_index(_sites(0), "t", True, "GnnBugLabModel", "00")
    empty.save(tmp_path / "empty.npz")
    assert S.SiteIndex.load(tmp_path / "empty.npz").size == 0
    # the model checks: another size is an error, other weights a warning, the same model neither
    assert back.check_model("GnnBugLabModel", 5, "ab" * 20) is None
    assert "other weights" in back.check_model("GnnBugLabModel", 5, "cd" * 20)
    with pytest.raises(S.DimensionMismatch, match="size 5"):
        back.check_model("GnnBugLabModel", 6, "ab" * 20)
    assert issubclass(S.DimensionMismatch, ValueError)


def test_fingerprint_follows_the_weights():
    import torch

    from buglab.models._similar import model_fingerprint

    torch.manual_seed(0)
    a = torch.nn.Linear(3, 2)
    first = model_fingerprint(a)
    assert first == model_fingerprint(a) and len(first) == 40
    with torch.no_grad():
        a.weight[0, 0] += 1.0
    assert model_fingerprint(a) != first


def test_report_counts_and_scout_agreement():
    from buglab.models import _similar as S

    index = S.make_index(_sites(), "known-bug", False, "M", "00")
    found = [S.Neighbours(0, 10, "a", -0.1, "VariableMisuse", True, S.neighbour_list(index, [0, 1, -1], [0.9, 0.5, 0.0], None)),
             S.Neighbours(1, 11, "b", -0.2, "VariableMisuse", True, S.neighbour_list(index, [1, 0, -1], [0.7, 0.2, 0.0], 0.3)),
             S.Neighbours(2, 12, "c", -0.3, "", False, [])]
    assert [n["entry"] for n in found[0].neighbours] == [0, 1] and [n["entry"] for n in found[1].neighbours] == [1]
    assert found[0].record()["neighbours"][0]["similarity"] == 0.9 and found[0].record()["neighbours"][0]["tag"] == "known-bug"
    blob = S.report(found, 6, 1, 2)
    assert (blob["num_samples"], blob["num_with_site"], blob["num_rejected"], blob["num_without_site"], blob["num_invalid_embeddings"],
            blob["num_with_neighbours"]) == (6, 3, 1, 2, 1, 2)
    assert blob["top1_similarity"]["max"] == 0.9 and blob["top1_similarity"]["min"] == 0.7
    assert blob["labelled"] == {"num_queries": 2, "top1_same_scout": 0.5}  # entry 0 carries the scout, entry 1 none


# ------------------------------------------------------------------------------------------------ refusals
def test_ensembles_and_the_great_model_are_refused():
    from buglab.models import similar as T
    from buglab.models._similar import make_index
    from buglab.models.ensemble.wrapper import EnsembleWrapper
    from buglab.models.greatreimplementation import GreatVarMisuse

    index = make_index(_sites(), None, True, "M", "00")
    ensemble = EnsembleWrapper.__new__(EnsembleWrapper)  # `require_single_model` looks at the type
    great = GreatVarMisuse({"num_layers": 2, "num_heads": 4, "intermediate_dimension": 96, "dropout_rate": 0.0}, vocab_size=64, embedding_dim=64)
    for model, word in ((ensemble, "ensembles"), (great, "GreatVarMisuse")):
        with pytest.raises(TypeError, match=word):
            T.build_site_index(model, None, [], "cpu")
        with pytest.raises(TypeError, match=word):
            T.find_similar(model, None, index, [], "cpu")
        with pytest.raises(TypeError, match=word):
            T.embed_sites(model, None, [], "cpu")


def test_an_index_of_another_size_is_exit_status_2_before_any_data_is_read(tmp_path, capsys):
    import torch

    from buglab.data.synthetic import make_report_dataset
    from buglab.models import _similar as S
    from buglab.models import similar as T
    from tests.test_visualize_host import _model

    model = _model("gnn-mlp", make_report_dataset(8, seed=35))  # hidden size 32
    torch.manual_seed(1)
    module = model.build_neural_module()
    assert T.embedding_dim(module) == 32
    checkpoint = tmp_path / "detector.pkl.gz"
    model.save(checkpoint, module)
    S.make_index(_sites(D=5), None, True, type(model).__name__, "00").save(tmp_path / "other.npz")
    # the data path does not exist and no GPU is asked for: the check comes first, also for a query over no data at all
    status = T.run(T.parse_args(["query", str(checkpoint), str(tmp_path / "other.npz"), str(tmp_path / "nowhere"), str(tmp_path / "out.jsonl")]))
    assert status == T.EXIT_DIMENSION_MISMATCH == 2 and "size 5" in capsys.readouterr().err and not (tmp_path / "out.jsonl").exists()
    index = S.make_index(_sites(D=5), None, True, type(model).__name__, "00")
    with pytest.raises(S.DimensionMismatch):
        T.search_similar(model, module, index, [], "cpu", host=True)


def test_command_line_parses():
    from buglab.models import similar as T

    a = T.parse_args(["index", "m", "d", "o", "--tag", "false-alarm", "--no-center"])
    assert (a.site, a.tag, a.no_center, a.assume_buggy, a.host) == ("truth", "false-alarm", True, False, False)
    q = T.parse_args(["query", "m", "i", "d", "o", "--assume-buggy", "--min-similarity", "0.5"])
    assert (q.site, q.top_k, q.candidates, q.min_similarity, q.assume_buggy) == ("predicted", 5, 16, 0.5, True)
    assert "BEYOND THE REFERENCE" in T.__doc__ and T.EXIT_DIMENSION_MISMATCH == 2


def test_launchers_check_before_any_hip_call():
    """host-side argument checks of the hip_ops wrappers (plain ValueErrors, no GPU needed) and of the C entry points: a bad call
    never reaches a kernel"""
    import ctypes
    import os
    import re

    import torch

    from buglab.models import _similar as S
    from buglab.models import hip_ops
    from tests.conftest import ROOT

    header = open(os.path.join(ROOT, "include", "buglab_hip.h")).read()
    assert "#define BL_SIM_MAX_D 512" in header and hip_ops.SIM_MAX_D == S.MAX_D == 512
    assert "#define BL_SIM_MAX_CANDIDATES 16" in header and hip_ops.SIM_MAX_CANDIDATES == S.MAX_CANDIDATES == C.MAX_CANDIDATES == 16
    assert re.search(r"Similar-bug search.*BEYOND THE REFERENCE", header)
    for name in ("bl_sim_embed_sites", "bl_sim_quantize", "bl_sim_search_i8", "bl_sim_rescore"):
        assert name in hip_ops.EXPORTED_SYMBOLS
    f32, f64 = (lambda *s: torch.zeros(*s)), (lambda *s: torch.zeros(*s, dtype=torch.float64))
    i8, i32 = (lambda *s: torch.zeros(*s, dtype=torch.int8)), (lambda *s: torch.zeros(*s, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"\[1, 512\]"):
        hip_ops.similar_quantize(f32(2, 513), f32(513))
    with pytest.raises(ValueError, match="mean"):
        hip_ops.similar_quantize(f32(2, 8), f32(7))
    with pytest.raises(ValueError, match="candidates must be"):
        hip_ops.similar_search(i8(2, 64), f64(2), i8(3, 64), f64(3), 17)
    with pytest.raises(ValueError, match="candidates must be"):
        hip_ops.similar_search(i8(2, 64), f64(2), i8(3, 64), f64(3), 0)
    with pytest.raises(ValueError, match="multiple of 64"):
        hip_ops.similar_search(i8(2, 96), f64(2), i8(3, 96), f64(3), 4)
    with pytest.raises(ValueError, match="slices must be"):
        hip_ops.similar_search(i8(2, 64), f64(2), i8(3, 64), f64(3), 4, slices=65)
    with pytest.raises(ValueError, match="k must be"):
        hip_ops.similar_rescore(f32(2, 8), f32(3, 8), f64(3), i32(2, 4), 5)
    with pytest.raises(ValueError, match=r"\[1, 16\]"):
        hip_ops.similar_rescore(f32(2, 8), f32(3, 8), f64(3), i32(2, 17), 5)
    with pytest.raises(ValueError, match=r"\[1, 512\]"):
        hip_ops.similar_rescore(f32(2, 600), f32(3, 600), f64(3), i32(2, 4), 2)
    with pytest.raises(ValueError, match="mode must be"):
        hip_ops.similar_embed_sites(f32(4), i32(3), i32(2), i32(2), f32(2, 8), f32(4, 8), i32(4), f32(4), 0, mode="likely")
    with pytest.raises(ValueError, match="do not fit"):
        hip_ops.similar_embed_sites(f32(4), i32(3), i32(3), i32(2), f32(2, 8), f32(4, 8), i32(4), f32(4), 3)
    with pytest.raises(ValueError, match="truth"):
        hip_ops.similar_embed_sites(f32(4), i32(3), i32(3), i32(2), f32(2, 8), f32(4, 8), i32(4), f32(4), 0, mode="truth")
    # well-formed calls on CPU tensors get as far as the device check, and no further
    with pytest.raises((hip_ops.HipOpsUnavailable, ValueError), match="GPU"):
        hip_ops.similar_quantize(f32(2, 8), f32(8))
    with pytest.raises(hip_ops.HipOpsUnavailable):
        hip_ops.similar_search(i8(2, 64), f64(2), i8(3, 64), f64(3), 4)
    assert hip_ops.similar_search_slices(1, 10) == 1 and hip_ops.similar_search_slices(16, 1 << 20) == 64
    assert hip_ops.similar_search_slices(50, 20000) == 19 and hip_ops.similar_search_slices(100000, 20000) == 1  # 1024 rows; one round
    assert hip_ops.similar_search_slices(1000, 1 << 20) == 8  # 63 query tiles x 8 = 504 workgroups <= 512

    lib = hip_ops.load_library()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.bl_sim_search_workspace_bytes(3, 2) == 3 * 2 * 16 * 12 and lib.bl_sim_search_workspace_bytes(3, 65) == 0
    assert lib.bl_sim_quantize(p, 8, p, 2, 513, p, 513, p, p, p, None) == -2 and b"BL_SIM_MAX_D" in lib.bl_last_error()
    assert lib.bl_sim_quantize(p, 4, p, 2, 8, p, 8, p, p, p, None) == -1 and b"row strides" in lib.bl_last_error()
    assert lib.bl_sim_quantize(p, 8, None, 2, 8, p, 8, p, p, p, None) == -1 and b"null" in lib.bl_last_error()
    assert lib.bl_sim_search_i8(p, p, 2, p, p, 3, 96, 4, 1, p, 1 << 20, p, p, None) == -1 and b"multiple of 64" in lib.bl_last_error()
    assert lib.bl_sim_search_i8(p, p, 2, p, p, 3, 64, 17, 1, p, 1 << 20, p, p, None) == -1 and b"C = 17" in lib.bl_last_error()
    assert lib.bl_sim_search_i8(p, p, 2, p, p, 3, 64, 4, 0, p, 1 << 20, p, p, None) == -1 and b"slices" in lib.bl_last_error()
    assert lib.bl_sim_search_i8(p, p, 2, p, p, 3, 64, 4, 2, p, 100, p, p, None) == -1 and b"workspace" in lib.bl_last_error()
    assert lib.bl_sim_search_i8(p, p, 2, p, p, 3, 576, 4, 1, p, 1 << 20, p, p, None) == -2 and b"BL_SIM_MAX_D" in lib.bl_last_error()
    assert lib.bl_sim_rescore(p, 8, 2, p, 8, p, 3, 8, p, 4, 5, p, p, None) == -1 and b"k = 5" in lib.bl_last_error()
    assert lib.bl_sim_rescore(p, 8, 2, p, 8, p, 3, 8, None, 4, 2, p, p, None) == -1 and b"null" in lib.bl_last_error()
    assert lib.bl_sim_embed_sites(p, 4, p, p, 3, 2, p, 2, p, 8, 2, 8, None, 0, 7, p, p, p, 0, 4, None) == -1 and b"mode" in lib.bl_last_error()
    assert lib.bl_sim_embed_sites(p, 4, p, p, 3, 2, p, 2, p, 8, 2, 8, None, 0, 1, p, p, p, 0, 4, None) == -1 and b"truth" in lib.bl_last_error()
    assert lib.bl_sim_embed_sites(p, 4, p, p, 3, 2, p, 2, p, 8, 2, 8, None, 0, 0, p, p, p, 3, 4, None) == -1 and b"do not fit" in lib.bl_last_error()
    assert lib.bl_sim_embed_sites(p, 4, p, p, 3, 2, p, 2, p, 4, 2, 8, None, 0, 0, p, p, p, 0, 4, None) == -1 and b"row stride" in lib.bl_last_error()
