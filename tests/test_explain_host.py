"""CPU: the NumPy twin of the attribution kernels (buglab/models/_explain.py) pinned to a literal restatement of the contract
of include/buglab_hip.h (plain loops, the butterfly written out: tests/explain_cases.py), the ordering against Python's stable
`sorted`, padding and NaN rules, the index arrays, the refusals and argument checks of `explain` (no GPU is present here, so
they happen before any GPU work), and the two entry points' bookkeeping."""
import ctypes
import math
import os
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from buglab.models import _explain as E
from tests import explain_cases as C
from tests.conftest import PKG, ROOT

HEADER = os.path.join(ROOT, "include", "buglab_hip.h")
LIB = os.path.join(PKG, "buglab", "models", "hip_ops", "libbuglab_hip.so")


@pytest.mark.parametrize("D", C.WIDTHS)
def test_node_scores_twin_is_the_contract(D):
    x, g = C.operands(D)
    first = E.node_scores_host(x, g)
    assert first.dtype == np.float64 and first.tobytes() == C.restate_node_scores(x, g).tobytes()
    # the rows on the grid of halves: every order gives the same, exact, sum
    exact = (x[:5].astype(np.float64) * g[:5].astype(np.float64)).sum(axis=1)
    assert first[:5].tobytes() == exact.tobytes()
    # accumulation with a weight: one rounded product, one rounded addition
    x2, g2 = C.operands(D, seed=1)
    third = 1.0 / 3
    acc = E.node_scores_host(x2, g2, E.node_scores_host(x, g, None, third), third)
    assert acc.tobytes() == C.restate_node_scores(x2, g2, C.restate_node_scores(x, g, None, third), third).tobytes()
    assert acc.tobytes() == (third * C.restate_node_scores(x, g) + third * C.restate_node_scores(x2, g2)).tobytes()


def test_node_scores_twin_edges():
    assert E.node_scores_host(np.zeros((0, 7), np.float32), np.zeros((0, 7), np.float32)).shape == (0,)
    x = np.array([[np.inf, 1.0], [np.nan, 1.0], [3.0e38, 3.0e38]], np.float32)
    g = np.array([[1.0, -2.0], [1.0, 1.0], [3.0e38, 3.0e38]], np.float32)
    got = E.node_scores_host(x, g)
    assert got[0] == np.inf and math.isnan(got[1]) and got[2] == 2 * float(np.float32(3.0e38)) ** 2  # no overflow: the products are formed in fp64
    with pytest.raises(ValueError, match="must both be"):
        E.node_scores_host(np.zeros((2, 3), np.float32), np.zeros((2, 4), np.float32))
    with pytest.raises(ValueError, match="must both be"):
        E.node_scores_host(np.zeros((2, 0), np.float32), np.zeros((2, 0), np.float32))
    with pytest.raises(ValueError, match="score"):
        E.node_scores_host(np.zeros((2, 3), np.float32), np.zeros((2, 3), np.float32), np.zeros(3))


@pytest.mark.parametrize("by_abs", [True, False])
@pytest.mark.parametrize("k", [1, 5, 32])
def test_topk_twin_is_the_contract(k, by_abs):
    score, off, at = C.handmade()
    got = E.topk_host(score, off, k, by_abs)
    C.assert_equal_bits(got, C.restate_topk(score, off, k, by_abs), (k, by_abs))
    node, picked, sums = got
    listed = (node >= 0).sum(axis=1)
    sizes = np.diff(off)
    # padding: -1 and 0.0 behind min(k, #non-NaN) entries
    nans = np.array([int(np.isnan(score[off[b]:off[b + 1]]).sum()) for b in range(len(sizes))])
    assert (listed == np.minimum(k, sizes - nans)).all()
    assert all((node[b, listed[b]:] == -1).all() and (picked[b, listed[b]:] == 0.0).all() and str(picked[b, k - 1]) != "-0.0" for b in range(len(sizes)))
    assert listed[at["n0"]] == 0 and listed[at["few"]] == 1 and listed[at["all_nan"]] == 0
    # NaN: never listed, both sums NaN; an empty graph sums to 0
    assert 10 not in node[at["one_nan"]].tolist() and np.isnan(sums[:, at["one_nan"]]).all() and np.isnan(sums[:, at["all_nan"]]).all()
    assert (sums[:, at["n0"]] == 0.0).all()
    # the tie across waves comes out in index order; +v and -v of one magnitude
    tie = node[at["tie_waves"]].tolist()
    pm = node[at["plus_minus"]].tolist()
    if by_abs:
        assert tie[:min(k, 3)] == [63, 64, 256][:k] and pm[:min(k, 2)] == [2, 5][:k]
    else:
        assert tie[:min(k, 2)] == [64, 256][:k] and 63 not in tie[:3] and pm[0] == 5
    # the graphs on the grid of halves: exact sums
    for name in ("n1", "n63", "n65", "n256", "n1000"):
        a = score[off[at[name]]:off[at[name] + 1]]
        assert sums[0, at[name]] == math.fsum(a) and sums[1, at[name]] == math.fsum(np.abs(a)), name


@pytest.mark.parametrize("by_abs", [True, False])
def test_topk_twin_against_sorted(by_abs):
    for seed in (0, 1):
        score, off = C.drawn(seed, B=30)
        assert not np.isnan(score).any()
        node, picked, sums = E.topk_host(score, off, 32, by_abs)
        for b in range(30):
            a = score[off[b]:off[b + 1]].tolist()
            want = sorted(range(len(a)), key=lambda i: -(abs(a[i]) if by_abs else a[i]))[:32]  # stable: ties keep index order
            assert node[b, :len(want)].tolist() == want and (node[b, len(want):] == -1).all()
            assert picked[b, :len(want)].tolist() == [a[i] for i in want]
            assert sums[0, b] == pytest.approx(math.fsum(a), rel=1e-12, abs=1e-12)
    C.assert_equal_bits(E.topk_host(score, off, 7, by_abs), C.restate_topk(score, off, 7, by_abs))


def test_topk_twin_clamps_offsets_and_checks_k():
    score = np.arange(10, dtype=np.float64)
    node, _, sums = E.topk_host(score, np.array([-3, 4, 99], np.int32), 2)
    assert node.tolist() == [[3, 2], [5, 4]] and sums[0].tolist() == [6.0, 39.0]
    for k in (0, 33):
        with pytest.raises(ValueError, match="k must be"):
            E.topk_host(score, np.array([0, 10], np.int32), k)


def test_explain_indices_on_a_handmade_layout():
    from buglab.models._suggest import SuggestIndices

    i32 = lambda *v: np.asarray(v, dtype=np.int32)
    # three samples: two rewrites, none, three; flat = [loc (4 + 3 NO_BUG) | rewrites]
    six = SuggestIndices(rw_idx=i32(7, 8, 9, 10, 11), rw_loc_idx=i32(0, 1, 2, 2, -1), rw_off=i32(0, 2, 2, 5), nobug_idx=i32(4, 5, 6),
                         tgt_rw=i32(0, -1, 2), loc_idx=i32(0, 1, 4, 5, 2, 3, 6), loc_off=i32(0, 3, 4, 7), key_node=i32(0, 1, -1, -1, 0, 1, -1),
                         rw_node=i32(0, 1, 0, 0, 1))
    points = [{"graph": {"nodes": ["a"] * n}} for n in (3, 0, 5)]
    ix = E.explain_indices([3, 0, 5], 8, six, points, node_to_graph=[0, 0, 0, 2, 2, 2, 2, 2])
    assert ix.node_off.dtype == np.int32 and ix.node_off.tolist() == [0, 3, 3, 8]
    assert ix.rw_idx is not None and ix.rw_off.tolist() == [0, 2, 2, 5] and ix.nobug_idx.tolist() == [4, 5, 6]
    chosen = E.chosen_flat_indices([1, 0, -1], ix)  # a rewrite; NO_BUG of a sample without rewrites; nothing
    assert chosen.dtype == np.int32 and chosen.tolist() == [[1, 8], [5, -1], [-1, -1]]
    assert E.chosen_flat_indices([2, -1, 3], ix).tolist() == [[4, -1], [-1, -1], [6, -1]]
    assert E.chosen_flat_indices([0, -1, 1], ix).tolist() == [[0, 7], [-1, -1], [2, 10]]
    with pytest.raises(AssertionError, match="contiguous"):
        E.explain_indices([3, 0, 5], 8, six, points, node_to_graph=[0, 0, 2, 0, 2, 2, 2, 2])
    with pytest.raises(AssertionError, match="add up"):
        E.explain_indices([3, 0, 5], 9, six, points)
    with pytest.raises(AssertionError):
        E.explain_indices([3, 0, 4], 7, six, points)  # a graph with another node count than its datapoint lists


def test_node_kinds():
    from buglab.models.explain import node_kinds

    graph = {"edges": {"NextToken": [(0, 1), (1, 4)], "HasSubtoken": [(0, 5), (4, 6), (1, 4)], "Child": [(2, 0)]}}
    assert node_kinds(graph, [0, 1, 2, 4, 5, 6, 3]) == ["token", "token", "other", "token", "subtoken", "subtoken", "other"]
    assert node_kinds({"edges": {}}, [0]) == ["other"] and node_kinds(graph, []) == []


def _untouched():
    raise AssertionError("the data was read: the refusal came too late")
    yield  # pragma: no cover


def test_refusals_and_argument_checks_come_before_any_gpu_work(tmp_path):
    from buglab.models.ensemble.wrapper import EnsembleWrapper
    from buglab.models.explain import explain
    from buglab.models.greatreimplementation import GreatVarMisuse
    from buglab.models.modelregistry import load_model

    seq = load_model({"modelName": "seq-great", "hidden_state_size": 32, "num_layers": 1, "num_heads": 4, "intermediate_dimension_size": 48},
                     Path(tmp_path / "s.pkl.gz"))[0]
    great = GreatVarMisuse({"num_layers": 2, "num_heads": 4, "intermediate_dimension": 96, "dropout_rate": 0.0}, vocab_size=64, embedding_dim=64)
    graph = load_model({"modelName": "gnn-mlp", "hidden_state_size": 32, "num_layers": 4}, Path(tmp_path / "g.pkl.gz"))[0]
    for model in (seq, great):
        with pytest.raises(NotImplementedError, match="gnn-mlp and ggnn"):
            explain(model, None, _untouched(), "cuda")
    with pytest.raises(TypeError, match="ensembles"):
        explain(EnsembleWrapper([graph], "avg"), None, _untouched(), "cuda")
    for kw, word in (({"k": 0}, "k must be"), ({"k": 33}, "k must be"), ({"steps": 0}, "steps must be"), ({"steps": 1.5}, "steps must be"),
                     ({"rank": -1}, "rank must be"), ({"rank": 32}, "rank must be")):
        with pytest.raises(ValueError, match=word):
            explain(graph, None, _untouched(), "cuda", **kw)


def test_entry_points_are_exported_and_report_argument_errors_without_a_gpu():
    from buglab.models import hip_ops

    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint bl_attr_node_scores\s*\(", header) and re.search(r"\bint bl_attr_topk\s*\(", header)
    assert "#define BL_EXPLAIN_MAX_K 32" in header and hip_ops.EXPLAIN_MAX_K == E.MAX_K == 32
    lib = hip_ops.load_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    for name in ("bl_attr_node_scores", "bl_attr_topk"):
        assert f" T {name}" in nm and name in hip_ops.EXPORTED_SYMBOLS
    f32, f64, i32 = (ctypes.c_float * 64)(), (ctypes.c_double * 64)(), (ctypes.c_int32 * 64)()
    x, s, o = (ctypes.cast(a, ctypes.c_void_p) for a in (f32, f64, i32))
    scores = lambda x=x, ldx=8, g=x, ldg=8, N=4, D=8, score=s: lib.bl_attr_node_scores(x, ldx, g, ldg, N, D, 1.0, 0, score, None)
    topk = lambda score=s, off=o, B=2, N=8, k=3, node=o, out=s, sums=s, offset=0, capacity=2: lib.bl_attr_topk(score, off, B, N, k, 1, node, out, sums,
                                                                                                              offset, capacity, None)
    BL_EINVAL, BL_ERANGE = -1, -2
    for call, kw, rc, word in ((scores, {"D": 0}, BL_EINVAL, b"D >= 1"), (scores, {"N": -1}, BL_EINVAL, b"N >= 0"),
                               (scores, {"ldx": 7}, BL_EINVAL, b"strides"), (scores, {"x": None}, BL_EINVAL, b"null"),
                               (scores, {"score": None}, BL_EINVAL, b"null"), (scores, {"N": 1 << 31}, BL_ERANGE, b"beyond int32"),
                               (topk, {"k": 0}, BL_EINVAL, b"at least 1"), (topk, {"k": 33}, BL_ERANGE, b"BL_EXPLAIN_MAX_K"),
                               (topk, {"offset": 1}, BL_EINVAL, b"do not fit"), (topk, {"B": 3}, BL_EINVAL, b"do not fit"),
                               (topk, {"off": None}, BL_EINVAL, b"null"), (topk, {"score": None}, BL_EINVAL, b"null"),
                               (topk, {"B": -1}, BL_EINVAL, b"negative"), (topk, {"N": 1 << 31}, BL_ERANGE, b"beyond int32")):
        assert call(**kw) == rc and word in lib.bl_last_error(), (kw, lib.bl_last_error())
    assert scores(N=0, x=None, score=None) == 0 and topk(B=0, off=None, node=None, out=None, sums=None, capacity=0) == 0  # no-ops
