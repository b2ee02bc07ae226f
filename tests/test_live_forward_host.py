"""Host (no GPU): the ONE decision whether a layer call runs over its live rows -- bl_mp_layer_live_ok, asked by
GraphNeuralNetwork.forward before the layer loop and evaluated again by bl_mp_layer_bwd -- and the top-down run that
GraphNeuralNetwork._live_forward_plan makes of its answers.

The predicate does no GPU work and dereferences none of the descriptor's arrays, so the descriptors here carry made-up non-null
addresses.  A layer whose forward ran over its live rows has valid saved state on those rows only: every configuration the live
backward excludes must therefore be excluded here already, and a layer may run live only if every layer above it does."""
import ctypes
import os

import pytest
import torch

from tests.conftest import PKG

LIB = os.path.join(PKG, "buglab", "models", "hip_ops", "libbuglab_hip.so")
PTR = 0x10000  # any non-null address: never read

N, E, T, R = 300, 1400, 4, 900
LIVE = dict(live_num_nodes=10, live_num_recv=55, live_num_msgs=47, live_num_runs=40)


@pytest.fixture(scope="module")
def ops():
    if not os.path.exists(LIB):
        import __graft_entry__ as g

        g.build()
    from buglab.models import hip_ops

    hip_ops.load_library()
    return hip_ops


def _desc(ops, Din=128, Dm=128, Dout=128, **over):
    L = ops.bl_mp_layer_t()
    L.N, L.E, L.T, L.Din, L.Dm, L.Dout = N, E, T, Din, Dm, Dout
    L.msg_act, L.ln_eps, L.aggregation = ops.ACT_GELU_AGG, 1e-5, 0
    for name in ("msg_src", "msg_tgt", "type_ptr", "tgt_ptr", "tgt_msgs", "src_ptr", "src_msgs", "W", "ln_g", "ln_b", "Wd", "bd", "Wd_packed",
                 "run_ptr", "bwd_group_ptr", "bwd_group_w", "bwd_rows_tgt", "bwd_rows_src", "tgt_run_ptr", "tgt_run_rows",
                 "live_nodes", "live_recv", "live_msgs", "live_run_ptr", "live_group_ptr", "live_rows_tgt", "live_rows_src", "live_src_ptr",
                 "live_src_msgs", "live_run_csr_ptr", "live_run_csr_rows"):
        setattr(L, name, PTR)
    L.num_runs = R
    for k, v in LIVE.items():
        setattr(L, k, v)
    for k, v in over.items():
        setattr(L, k, v)
    return L


def _ok(ops, L, have_w_bwd=1, forward=1, want_winners=0):
    lib = ops.load_library()
    got = bool(lib.bl_mp_layer_live_ok(ctypes.byref(L), have_w_bwd, forward, want_winners))
    return got, lib.bl_last_error().decode()


def test_the_headline_configuration_passes_in_both_directions(ops):
    assert ops.msg_gemm_mode() == "f16x3" and ops.live_backward() and ops.live_forward() and not ops.deterministic()
    for kw in ({}, {"Din": 256, "Dm": 256}):  # a plain layer and a concat layer
        assert _ok(ops, _desc(ops, **kw), forward=1)[0] and _ok(ops, _desc(ops, **kw), forward=0)[0]


@pytest.mark.parametrize("what,over,call", [
    ("no live arrays", {"live_nodes": None}, {}),
    ("an incomplete set of live arrays", {"live_src_msgs": None}, {}),
    ("no run arrays", {"num_runs": 0}, {}),
    ("sum aggregation", {"aggregation": 1, "msg_act": 0}, {}),
    ("Din not a multiple of 128", {"Din": 64}, {}),
    ("dense update not on bf16x6", {"Wd_packed": None}, {}),
    ("message width without a one-kernel node update", {"Dm": 64}, {}),
    ("vector-unit input gradient", {}, {"have_w_bwd": 0}),
    ("a winner table is wanted", {}, {"want_winners": 1}),
    # forward scratch: compact pre [E', Dm] + map [E] + target ids [E'] inside the [E, Dm] pre-activations of the full forward;
    # with every message live it cannot fit (the backward workspace still would: E' + R' rows of Din against E rows of 2 Din)
    ("the forward scratch does not fit", {"live_num_msgs": E, "live_num_runs": 10}, {}),
    ("the compact gradient does not fit the backward workspace", {"live_num_msgs": E, "live_num_runs": E}, {"forward": 0}),
])
def test_every_excluded_configuration_is_false_with_a_reason(ops, what, over, call):
    got, why = _ok(ops, _desc(ops, **over), **call)
    assert not got and why.startswith("bl_mp_layer_live_ok: "), (what, why)


def test_forward_only_conditions_do_not_bind_backward(ops):
    """a winner table and the forward scratch concern forward alone: backward of a layer whose forward ran in full may still go live"""
    assert _ok(ops, _desc(ops), forward=0, want_winners=1)[0]
    assert _ok(ops, _desc(ops, live_num_msgs=E, live_num_runs=10), forward=0)[0]


def test_every_switch_that_excludes_the_live_backward_excludes_the_live_forward(ops):
    flips = [
        ("live backward off", lambda: ops.set_live_backward(False), lambda p: ops.set_live_backward(p)),
        ("live forward off", lambda: ops.set_live_forward(False), lambda p: ops.set_live_forward(p)),
        ("run rows off", lambda: ops.set_run_rows(False), lambda p: ops.set_run_rows(p)),
        ("bf16x6 message GEMMs", lambda: ops.set_msg_gemm_mode("bf16x6"), lambda p: ops.set_msg_gemm_mode(p)),
        ("f16x1 message GEMMs", lambda: ops.set_msg_gemm_mode("f16x1"), lambda p: ops.set_msg_gemm_mode(p)),
        ("three-kernel node update backward", lambda: ops.set_fused_node_bwd(False), lambda p: ops.set_fused_node_bwd(p)),
        ("deterministic mode", lambda: (ops.deterministic(), ops.load_library().bl_set_deterministic(1))[0],
         lambda p: ops.load_library().bl_set_deterministic(1 if p else 0)),
    ]
    for what, flip, restore in flips:
        assert _ok(ops, _desc(ops))[0], what
        prev = flip()
        try:
            got, why = _ok(ops, _desc(ops))
            back_too = _ok(ops, _desc(ops), forward=0)[0]
        finally:
            restore(prev)
        assert not got, (what, why)
        assert back_too == (what == "live forward off"), what  # its own switch is the only one that leaves the live backward on
    assert _ok(ops, _desc(ops))[0]


def test_dropout_counter_of_a_nodes_own_row_must_fit_32_bits(ops):
    big = _desc(ops)
    big.N = 1 << 26  # x Dout 128 = 2^33 counters
    big.drop = ops.Dropout(0.2, 1, 1).c()
    assert not _ok(ops, big)[0]
    big.drop = ops.Dropout(0.0, 1, 1).c()
    assert _ok(ops, big)[0]


# ---- the run from the top ---------------------------------------------------------------------------------------------------
def _plan(ops, monkeypatch, recipe, refuse=(), live_layers=4, embed=128):
    from buglab.models.hip_ops import GraphIndex
    from buglab.models.layers import messagepassing as M

    gnn = M.GraphNeuralNetwork(M.SubtokenEmbedder(10, embed), recipe)
    asked = []

    def fake_ok(din, lo_width, W, *rest):
        idx = next(i for i, l in enumerate(gnn._mp_sequence_for_test) if getattr(l, "W", None) is W)
        asked.append((idx, din, lo_width))
        return idx not in refuse

    gnn._mp_sequence_for_test = [l for l in recipe if isinstance(l, torch.nn.Module)]
    monkeypatch.setattr(ops, "live_forward_ok", fake_ok)
    z = torch.zeros(1, dtype=torch.int32)
    graph = GraphIndex(z, z, z, z, z, z, z, 1, 1, 1)
    live = [object()] * live_layers
    monkeypatch.setattr(GraphIndex, "_replace", lambda self, **kw: self)
    plan = gnn._live_forward_plan(graph, live, lambda rate, stream: ops.Dropout(rate, 0, stream))
    return plan, asked


def test_the_run_covers_the_layers_from_the_top_that_all_pass(ops, monkeypatch):
    from buglab.models.gnnlayerdefs import create_mlp_mp_layers

    recipe = create_mlp_mp_layers(128, 0.2, T, num_layers=8)
    plan, asked = _plan(ops, monkeypatch, recipe, live_layers=6)
    assert plan == {7: ops.LIVE_FWD_LAST, 6: ops.LIVE_FWD_INNER, 5: ops.LIVE_FWD_INNER, 4: ops.LIVE_FWD_INNER, 3: ops.LIVE_FWD_INNER,
                    2: ops.LIVE_FWD_INNER}
    # asked from the last layer downwards, the concat layers with both widths (the stash's first)
    assert asked == [(7, 256, 128), (6, 128, None), (5, 128, None), (4, 128, None), (3, 256, 128), (2, 128, None)]


def test_the_run_stops_at_the_first_layer_that_fails(ops, monkeypatch):
    from buglab.models.gnnlayerdefs import create_mlp_mp_layers

    recipe = create_mlp_mp_layers(128, 0.2, T, num_layers=4)
    plan, asked = _plan(ops, monkeypatch, recipe, refuse={2})
    assert plan == {3: ops.LIVE_FWD_LAST} and [a[0] for a in asked] == [3, 2]  # layers 1 and 0 are not even asked
    plan, _ = _plan(ops, monkeypatch, recipe, refuse={3})
    assert plan == {}


def test_a_gated_layer_or_edge_features_end_the_run_unasked(ops, monkeypatch):
    from buglab.models.layers import messagepassing as M

    mlp = lambda **kw: M.MlpMessagePassingLayer(128, 128, 128, T, dropout_rate=0.0, **kw)
    recipe = [mlp(), M.GatedMessagePassingLayer(128, 128, T), mlp(), mlp()]
    plan, asked = _plan(ops, monkeypatch, recipe)
    assert plan == {3: ops.LIVE_FWD_LAST, 2: ops.LIVE_FWD_INNER} and [a[0] for a in asked] == [3, 2]
    recipe = [mlp(), mlp(), mlp(features_dimension=16), mlp()]
    plan, asked = _plan(ops, monkeypatch, recipe)
    assert plan == {3: ops.LIVE_FWD_LAST} and [a[0] for a in asked] == [3]


def test_a_trailing_concat_keeps_the_full_forward(ops, monkeypatch):
    """[stash ; last] handed out as the output would expose the stash's rows nobody computed"""
    from buglab.models.layers import messagepassing as M

    r = M.ConcatResidualLayer(128)
    recipe = [r.pass_through_dummy_layer(), M.MlpMessagePassingLayer(128, 128, 128, T), r]
    plan, asked = _plan(ops, monkeypatch, recipe)
    assert plan == {} and asked == []
