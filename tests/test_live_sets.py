"""CPU: the live sets of a minibatch (buglab.data.collate.live_set_arrays and its native twin bl_live_sets).

The scoring heads read the encoder's output through one gather of the rows head_gather_idx, so the gradient of the last layer's
output is zero outside those rows, the gradient of the layer below outside those rows and the sources of the messages into them,
and so on.  The backward pass of the last layers runs over these rows only (csrc/bl_mp_layer.hip), so the arrays decide which
rows are computed at all: both collators must make the same ones, they must equal a brute-force reachability, and on the fp64
oracle's full backward every row they leave out must carry a gradient that is exactly zero."""
import numpy as np
import pytest
import torch

from buglab.data import collate as C
from buglab.data import native
from buglab.data.synthetic import make_samples
from oracle import buglab_oracle as O

I32 = np.int32
T = 4
COL = {name: i for i, name in enumerate(C.LIVE_LAYOUT_COLUMNS)}


def _samples(seed=0, n=150, E=700, C_=5, B=2):
    """B graphs whose head rows are exactly their C_ candidate nodes (the repair heads of a buggy sample score the same node)"""
    return make_samples(B, seed=seed, num_nodes=n, num_messages=E, num_edge_types=T, vocab_size=300, num_candidates=C_, n_var=0, n_swap=0)


def _both(samples, monkeypatch, layers=None, fraction=None):
    if layers is not None:
        monkeypatch.setenv("BL_LIVE_LAYERS", str(layers))
    if fraction is not None:
        monkeypatch.setenv("BL_LIVE_FRACTION", repr(fraction))
    assert native.available()
    monkeypatch.setenv("BUGLAB_NATIVE_COLLATE", "1")
    a = C.collate_samples(samples, T)
    monkeypatch.setenv("BUGLAB_NATIVE_COLLATE", "0")
    b = C.collate_samples(samples, T)
    for k in ("live_arrays", "live_layout"):
        x, y = a["graph_data"][k], b["graph_data"][k]
        assert x.dtype == np.int32 and y.dtype == np.int32 and x.shape == y.shape and np.array_equal(x, y), k
    return b


def _pieces(gd, d):
    row = gd["live_layout"][d].astype(np.int64)
    nn, nr, ex, rx = row[:4]
    sizes = C._live_piece_sizes(int(nn), int(nr), int(ex), int(rx), T)
    names = C.LIVE_LAYOUT_COLUMNS[4:]
    for o in row[4:]:
        assert o % 4 == 0                                                   # 16-byte pieces inside the 16-byte-aligned blob entry
    return {k: gd["live_arrays"][row[COL[k]]:row[COL[k]] + s].astype(np.int64) for k, s in zip(names, sizes)}


def _check(gd, max_layers, fraction):
    """every property the kernels rely on, from msg_src / msg_tgt / type_ptr / head_gather_idx alone -> the live node sets"""
    src, tgt, type_ptr = gd["msg_src"].astype(np.int64), gd["msg_tgt"].astype(np.int64), gd["type_ptr"].astype(np.int64)
    N, E = gd["token_ids"].shape[0], tgt.shape[0]
    typ = np.repeat(np.arange(T), np.diff(type_ptr))
    want_nodes = np.unique(gd["head_gather_idx"].astype(np.int64))        # brute force: one reachability step per layer
    layout = gd["live_layout"]
    assert layout.shape[1] == len(C.LIVE_LAYOUT_COLUMNS) and layout.shape[0] <= max_layers
    sets = []
    for d in range(layout.shape[0]):
        p = _pieces(gd, d)
        assert np.array_equal(p["nodes"], want_nodes)
        msgs = np.array([e for e in range(E) if tgt[e] in set(want_nodes.tolist())], dtype=np.int64)
        assert np.array_equal(p["msgs"], msgs) and len(msgs) <= fraction * E
        ex = len(msgs)
        recv = np.unique(np.concatenate([want_nodes, src[msgs]]))
        assert np.array_equal(p["recv"], recv)
        # runs: a partition of 0..E' into maximal ranges of one type and one target
        rp = p["run_ptr"]
        rx = len(rp) - 1
        assert rp[0] == 0 and rp[-1] == ex and (np.diff(rp) > 0).all()
        ctyp, ctgt = typ[msgs], tgt[msgs]
        for r in range(rx):
            assert (ctyp[rp[r]:rp[r + 1]] == ctyp[rp[r]]).all() and (ctgt[rp[r]:rp[r + 1]] == ctgt[rp[r]]).all()
        rtyp, rtgt = ctyp[rp[:-1]], ctgt[rp[:-1]]
        same = rtyp[1:] == rtyp[:-1]
        assert (rtgt[1:][same] != rtgt[:-1][same]).all()
        gp = p["group_ptr"]
        assert gp.shape == (2 * T + 1,) and (np.diff(gp) >= 0).all() and gp[T] == ex and gp[-1] == ex + rx
        for t in range(T):
            assert np.array_equal(np.flatnonzero(ctyp == t), np.arange(gp[t], gp[t + 1]))
            assert np.array_equal(np.flatnonzero(rtyp == t) + ex, np.arange(gp[T + t], gp[T + t + 1]))
        assert np.array_equal(want_nodes[p["rows_tgt"]], np.concatenate([ctgt, rtgt]))          # positions in the live list
        assert np.array_equal(p["rows_src"], np.concatenate([src[msgs], rtgt]))                  # node ids
        sp, sm, cp, cr = p["src_ptr"], p["src_msgs"], p["run_csr_ptr"], p["run_csr_rows"]
        assert sp[0] == 0 and sp[-1] == ex and cp[0] == 0 and cp[-1] == rx
        for i, v in enumerate(recv):                                        # exactly the rows of each receiving node, ascending
            assert np.array_equal(sm[sp[i]:sp[i + 1]], np.flatnonzero(src[msgs] == v))
            assert np.array_equal(cr[cp[i]:cp[i + 1]], np.flatnonzero(rtgt == v) + ex)
        sets.append(want_nodes)
        want_nodes = recv
    if layout.shape[0] < max_layers and len(gd["head_gather_idx"]):      # the descent stopped because the next layer is too large
        assert np.isin(tgt, want_nodes).sum() > fraction * E
    return sets


def _oracle_output_gradients(samples, mb, layers=4, H=8):
    """d loss / d (output of every message-passing layer) on the fp64 oracle's full backward, last layer first"""
    cfg = O.OracleConfig(hidden=H, num_layers=layers, num_edge_types=T, vocab_size=300)
    params = {k: v.double().requires_grad_(True) for k, v in O.init_params(cfg, seed=0).items()}
    trace = []
    out = O.forward_loss(params, mb, cfg, trace=trace)
    outs = [t["out"] for t in trace if "out" in t]
    assert len(outs) == layers
    for o in outs:
        o.retain_grad()
    out["loss"].backward()
    return [o.grad for o in outs[::-1]]


def _assert_dead_rows_are_exactly_zero(samples, mb, sets):
    grads = _oracle_output_gradients(samples, mb)
    N = mb["graph_data"]["token_ids"].shape[0]
    for d, nodes in enumerate(sets):
        dead = np.setdiff1d(np.arange(N), nodes)
        g = grads[d].numpy()
        assert (g[dead] == 0.0).all(), d
        if len(nodes):
            assert np.abs(g[nodes]).max() > 0


def test_two_graphs_five_head_rows_each(monkeypatch):
    samples = _samples()
    mb = _both(samples, monkeypatch, layers=4, fraction=1.0)
    gd = mb["graph_data"]
    assert gd["token_ids"].shape[0] == 300 and gd["msg_tgt"].shape[0] == 1400 and np.unique(gd["head_gather_idx"]).shape[0] == 10
    sets = _check(gd, 4, 1.0)
    assert len(sets) == 4 and [len(s) for s in sets] == sorted(len(s) for s in sets) and len(sets[0]) == 10
    _assert_dead_rows_are_exactly_zero(samples, mb, sets)
    # the defaults stop where the live messages pass the fraction
    mb = _both(samples, monkeypatch, layers=C.LIVE_MAX_LAYERS, fraction=C.LIVE_FRACTION)
    assert 1 <= len(_check(mb["graph_data"], C.LIVE_MAX_LAYERS, C.LIVE_FRACTION)) <= C.LIVE_MAX_LAYERS


def test_no_head_rows_at_all(monkeypatch):
    samples = _samples(seed=1, C_=0)
    mb = _both(samples, monkeypatch, layers=3, fraction=1.0)
    gd = mb["graph_data"]
    assert gd["head_gather_idx"].shape[0] == 0 and gd["live_layout"].shape == (0, len(C.LIVE_LAYOUT_COLUMNS)) and gd["live_arrays"].shape == (0,)


def test_every_node_a_head_row(monkeypatch):
    samples = _samples(seed=2, n=40, E=150, C_=40)
    mb = _both(samples, monkeypatch, layers=3, fraction=1.0)
    sets = _check(mb["graph_data"], 3, 1.0)
    assert len(sets) == 3 and all(len(s) == 80 for s in sets)             # everything is live: nothing to leave out
    assert mb["graph_data"]["live_layout"][0, COL["num_msgs"]] == 300
    _assert_dead_rows_are_exactly_zero(samples, mb, sets)
    mb = _both(samples, monkeypatch, layers=3, fraction=0.5)                # ... and the fraction says so: no live layer
    assert mb["graph_data"]["live_layout"].shape[0] == 0


def test_a_head_row_with_no_incoming_message(monkeypatch):
    samples = _samples(seed=3)
    g = samples[1].graph_data
    lonely = int(g.reference_nodes["candidate_nodes"][2])
    g.adjacency_lists[:] = [a[a[:, 1] != lonely] for a in g.adjacency_lists]
    mb = _both(samples, monkeypatch, layers=3, fraction=1.0)
    gd = mb["graph_data"]
    sets = _check(gd, 3, 1.0)
    assert 150 + lonely in sets[0] and not (gd["msg_tgt"] == 150 + lonely).any()
    _assert_dead_rows_are_exactly_zero(samples, mb, sets)
    # head rows none of which has an incoming message: a live layer without messages, its input gradient is zero everywhere
    for s in samples:
        cand = s.graph_data.reference_nodes["candidate_nodes"]
        s.graph_data.adjacency_lists[:] = [a[~np.isin(a[:, 1], cand)] for a in s.graph_data.adjacency_lists]
    mb = _both(samples, monkeypatch, layers=3, fraction=1.0)
    sets = _check(mb["graph_data"], 3, 1.0)
    row = mb["graph_data"]["live_layout"][0]
    assert row[COL["num_msgs"]] == 0 and row[COL["num_runs"]] == 0 and row[COL["num_recv"]] == row[COL["num_nodes"]] == 10
    _assert_dead_rows_are_exactly_zero(samples, mb, sets[:1])
    assert (_oracle_output_gradients(samples, mb)[1].numpy() == 0.0).all()


def test_an_edge_type_with_no_live_message(monkeypatch):
    samples = _samples(seed=4)
    for s in samples:                                                       # type 1 exists, but never into a head row; type 2 is empty
        cand = s.graph_data.reference_nodes["candidate_nodes"]
        a = s.graph_data.adjacency_lists
        a[1] = a[1][~np.isin(a[1][:, 1], cand)]
        a[2] = np.zeros((0, 2), I32)
        assert a[1].shape[0] > 0
    mb = _both(samples, monkeypatch, layers=3, fraction=1.0)
    gd = mb["graph_data"]
    sets = _check(gd, 3, 1.0)
    gp = _pieces(gd, 0)["group_ptr"]
    assert gp[1] == gp[2] == gp[3] and gp[T + 1] == gp[T + 2] == gp[T + 3] and gp[1] > 0
    _assert_dead_rows_are_exactly_zero(samples, mb, sets)


@pytest.mark.parametrize("degree", ["uniform", "powerlaw"])
def test_generators(degree, monkeypatch):
    samples = make_samples(4, seed=3, num_nodes=200, num_messages=1000, num_edge_types=T, num_candidates=6, degree=degree, max_degree=150)
    mb = _both(samples, monkeypatch, layers=3, fraction=0.6)
    _check(mb["graph_data"], 3, 0.6)


def test_the_arrays_travel_in_the_minibatch_blob():
    mb = C.collate_samples(_samples(seed=5), T)
    gd = mb["graph_data"]
    blob, meta = C.pack_minibatch(mb)
    where = {k: (shape, o) for w, k, shape, o in meta["layout"] if w == "gd"}
    shape, o = where["live_arrays"]
    assert o % 4 == 0 and np.array_equal(blob[o:o + shape[0]], gd["live_arrays"]) and gd["live_arrays"].shape[0] > 0
    shape, o = where["live_layout"]
    assert shape == gd["live_layout"].shape and np.array_equal(blob[o:o + shape[0] * shape[1]].reshape(shape), gd["live_layout"])
    assert C.packed_size(mb) >= meta["total"]
    out = C.upload_packed(blob, meta, "cpu")["graph_data"]
    assert isinstance(out["live_layout"], np.ndarray) and np.array_equal(out["live_layout"], gd["live_layout"]) and np.array_equal(out["live_arrays"].numpy(), gd["live_arrays"])
