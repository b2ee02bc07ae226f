"""CPU: the run arrays of a minibatch (buglab.data.collate.message_run_arrays and its native twin bl_message_runs).

A run is a maximal stretch of consecutive messages of one type with one target.  The backward pass of the message-passing
layers computes the target half of a run's gradients once, so these arrays decide which rows exist at all: both collators must
make the same ones, and they must partition the messages exactly."""
import numpy as np
import pytest

from buglab.data import collate as C
from buglab.data import native
from buglab.data.collate import TensorizedGraphData
from buglab.data.synthetic import make_samples

I32 = np.int32


def _graph(n, lists):
    return TensorizedGraphData(np.zeros((n, 2), I32), np.ones(n, I32), [np.asarray(a, I32).reshape(-1, 2) for a in lists])


def _both(graphs, T, monkeypatch):
    monkeypatch.setenv("BUGLAB_NATIVE_COLLATE", "1")
    a = C.collate_graphs(graphs, T)
    monkeypatch.setenv("BUGLAB_NATIVE_COLLATE", "0")
    b = C.collate_graphs(graphs, T)
    assert native.available()
    for k in C.RUN_KEYS:
        assert a[k].dtype == np.int32 and b[k].dtype == np.int32 and np.array_equal(a[k], b[k]), k
    return b


def _check(gd, T):
    """every property the kernels rely on, from msg_tgt / type_ptr alone"""
    tgt, src, type_ptr = gd["msg_tgt"], gd["msg_src"], gd["type_ptr"].astype(np.int64)
    N, E = gd["token_ids"].shape[0], tgt.shape[0]
    run_ptr = gd["run_ptr"].astype(np.int64)
    R = run_ptr.shape[0] - 1
    assert R <= E and run_ptr[0] == 0 and run_ptr[-1] == E and (np.diff(run_ptr) > 0).all()  # a partition of 0..E into non-empty ranges
    typ = np.repeat(np.arange(T), np.diff(type_ptr))
    run_typ, run_tgt = typ[run_ptr[:-1]], tgt[run_ptr[:-1]]
    for r in range(R):  # one type and one target per run
        assert (typ[run_ptr[r]:run_ptr[r + 1]] == run_typ[r]).all() and (tgt[run_ptr[r]:run_ptr[r + 1]] == run_tgt[r]).all()
    same_type = run_typ[1:] == run_typ[:-1]
    assert (run_tgt[1:][same_type] != run_tgt[:-1][same_type]).all()  # maximal: neighbouring runs of one type differ in target
    gp = gd["bwd_group_ptr"].astype(np.int64)
    assert gp.shape == (2 * T + 1,) and (np.diff(gp) >= 0).all() and gp[-1] == E + R
    assert np.array_equal(gp[:T], type_ptr[:-1]) and gp[T] == E
    for t in range(T):  # group T + t = the runs of type t, as rows E + run id
        assert np.array_equal(np.flatnonzero(run_typ == t) + E, np.arange(gp[T + t], gp[T + t + 1]))
    assert gd["bwd_group_w"].tolist() == [2 * t for t in range(T)] + [2 * t + 1 for t in range(T)]
    assert np.array_equal(gd["bwd_rows_tgt"], np.concatenate([tgt, run_tgt])) and np.array_equal(gd["bwd_rows_src"], np.concatenate([src, run_tgt]))
    trp, trr = gd["tgt_run_ptr"].astype(np.int64), gd["tgt_run_rows"].astype(np.int64)
    assert trp.shape == (N + 1,) and trp[0] == 0 and trp[-1] == R and trr.shape == (R,)
    for v in range(N):  # exactly the runs of each node, ascending
        assert np.array_equal(trr[trp[v]:trp[v + 1]], np.flatnonzero(run_tgt == v) + E)
    return R, E


def test_no_messages(monkeypatch):
    gd = _both([_graph(5, [[], [], []])], 3, monkeypatch)
    assert _check(gd, 3) == (0, 0)
    gd = _both([], 4, monkeypatch)
    assert gd["run_ptr"].tolist() == [0] and gd["bwd_group_ptr"].tolist() == [0] * 9 and gd["tgt_run_ptr"].tolist() == [0]


def test_a_type_without_messages_and_a_long_run(monkeypatch):
    rng = np.random.default_rng(0)
    n = 40
    hub = np.stack([rng.integers(0, n, 200), np.full(200, 7)], axis=1)                     # every message of type 1 into node 7
    other = np.stack([rng.integers(0, n, 300), rng.integers(0, n, 300)], axis=1)
    gd = _both([_graph(n, [other, hub, [], other[:50]])], 4, monkeypatch)                    # type 2 is empty
    R, E = _check(gd, 4)
    lens = np.diff(gd["run_ptr"])
    assert lens.max() == 200 and E == 550 and R < E
    assert gd["bwd_group_ptr"][4 + 2] == gd["bwd_group_ptr"][4 + 3]                          # the empty type has no run rows either


def test_no_repeated_type_and_target(monkeypatch):
    n = 30
    a = np.stack([np.arange(n)[::-1], np.arange(n)], axis=1)                                 # every node once per type
    gd = _both([_graph(n, [a, a[:10], a[5:]]), _graph(n, [a[:3], [], a])], 3, monkeypatch)
    R, E = _check(gd, 3)
    assert R == E == gd["msg_tgt"].shape[0]
    assert np.array_equal(gd["run_ptr"], np.arange(E + 1))


def test_duplicate_edges_share_a_run(monkeypatch):
    a = [[0, 3], [0, 3], [1, 3], [0, 3], [2, 4]]                                             # (0 -> 3) three times in one type
    gd = _both([_graph(6, [a, a])], 2, monkeypatch)
    R, E = _check(gd, 2)
    assert (R, E) == (4, 10) and np.diff(gd["run_ptr"]).tolist() == [4, 1, 4, 1]


@pytest.mark.parametrize("degree", ["uniform", "powerlaw"])
def test_generators(degree, monkeypatch):
    samples = make_samples(6, seed=3, num_nodes=300, num_messages=1500, num_edge_types=5, degree=degree, max_degree=300)
    samples[2].graph_data.adjacency_lists[1] = np.zeros((0, 2), I32)
    monkeypatch.setenv("BUGLAB_NATIVE_COLLATE", "1")
    a = C.collate_samples(samples, 6)["graph_data"]
    monkeypatch.setenv("BUGLAB_NATIVE_COLLATE", "0")
    b = C.collate_samples(samples, 6)["graph_data"]
    for k in C.RUN_KEYS:
        assert np.array_equal(a[k], b[k]), k
    R, E = _check(b, 6)
    if degree == "powerlaw":
        assert np.diff(b["run_ptr"]).max() > 128 or R < E


def test_the_headline_generator_keeps_runs_below_four_fifths_of_the_messages(monkeypatch):
    """bench.py's headline minibatch (uniform in-degree, 2 000 nodes, 10 000 messages, 16 types): R / E was 0.751 when the run
    rows were introduced.  The change pays in proportion to 1 - R / E; a generator that lost the property would make the
    benchmark measure nothing of it."""
    samples = make_samples(16, seed=1000, num_nodes=2000, num_messages=10000, num_edge_types=16, degree="uniform", max_degree=512)
    monkeypatch.setenv("BUGLAB_NATIVE_COLLATE", "1")
    gd = C.collate_samples(samples, 16)["graph_data"]
    R, E = gd["run_ptr"].shape[0] - 1, gd["msg_tgt"].shape[0]
    assert E == 160000 and R / E < 0.8, R / E


def test_the_arrays_travel_in_the_minibatch_blob():
    samples = make_samples(3, seed=1, num_nodes=50, num_messages=200, num_edge_types=4)
    mb = C.collate_samples(samples, 4)
    blob, meta = C.pack_minibatch(mb)
    where = {k: (shape, o) for w, k, shape, o in meta["layout"] if w == "gd"}
    for k in C.RUN_KEYS:
        shape, o = where[k]
        assert np.array_equal(blob[o:o + shape[0]], mb["graph_data"][k]), k
    assert C.packed_size(mb) >= meta["total"]
