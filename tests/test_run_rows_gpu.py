"""GPU: the run rows of bl_mp_layer_bwd -- the target halves of the routed f16x3 input and weight gradients computed once per
run of messages (consecutive messages of one type into one node) with the OR of the members' routing masks.

Shapes: the smallest at which these kernels can go wrong -- 300 nodes, ~1 500 messages, five types of which one is empty, one
type with more than 256 messages (runs cross the 128-row tiles), one node whose run is longer than 128, duplicate edges (exact
ties in the max), widths 128 and 256 (two column tiles per group)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_NODES, T_TYPES = 300, 5


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from buglab.models import hip_ops

    hip_ops.load_library()
    return hip_ops


def _dev(a):
    return torch.as_tensor(a).cuda().contiguous()


@pytest.fixture(scope="module")
def graph_np():
    """one graph; type 3 is empty, type 0 has 700 messages with duplicates, 200 messages of type 1 go into node 7, which is also the
    source of 120 messages of type 4 (with its one long run it still has more than 64 rows to sum: the hub split of the sums)"""
    from buglab.data import collate as C

    rng = np.random.default_rng(5)
    n = N_NODES
    pair = lambda m: np.stack([rng.integers(0, n, m), rng.integers(0, n, m)], axis=1).astype(np.int32)
    t0 = pair(600)
    t0 = np.concatenate([t0, t0[:100]])                                     # duplicate edges: same source, target and type
    t1 = np.concatenate([np.stack([rng.integers(0, n, 200), np.full(200, 7)], axis=1).astype(np.int32), pair(150)])
    t4 = np.concatenate([np.stack([np.full(120, 7), rng.integers(0, n, 120)], axis=1).astype(np.int32), pair(80)])  # node 7 also sends 120
    lists = [t0, t1, pair(250), np.zeros((0, 2), np.int32), t4]
    g = C.TensorizedGraphData(np.zeros((n, 2), np.int32), np.ones(n, np.int32), lists)
    gd = C.collate_graphs([g], T_TYPES)
    E, R = gd["msg_tgt"].shape[0], gd["run_ptr"].shape[0] - 1
    assert E == 1500 and np.diff(gd["run_ptr"]).max() >= 200 and R < E and np.diff(gd["type_ptr"]).tolist()[3] == 0
    assert gd["num_hub_nodes"] >= 1 and gd["node_order"][0] == 7           # node 7 sits in a hub slot
    return gd


def _graph_index(ops, gd, with_runs):
    d = {k: _dev(gd[k]) for k in ("msg_src", "msg_tgt", "type_ptr", "tgt_ptr", "tgt_msgs", "src_ptr", "src_msgs", "node_order")}
    runs = ops.MessageRuns(*[_dev(gd[k]) for k in ops.MessageRuns._fields]) if with_runs else None
    return ops.GraphIndex(d["msg_src"], d["msg_tgt"], d["type_ptr"], d["tgt_ptr"], d["tgt_msgs"], d["src_ptr"], d["src_msgs"], N_NODES,
                          int(gd["msg_tgt"].shape[0]), T_TYPES, d["node_order"], int(gd["num_hub_nodes"]), runs)


def _or_runs(ops, bits, run_ptr, E, R):
    ops._check(ops.load_library().bl_winbits_or_runs(bits.data_ptr(), bits.stride(0), run_ptr.data_ptr(), E, R, bits.shape[1],
                                                     torch.cuda.current_stream().cuda_stream), "bl_winbits_or_runs")
    torch.cuda.synchronize()


def _np_or(bits_np, run_ptr, R):
    return np.stack([np.bitwise_or.reduce(bits_np[run_ptr[r]:run_ptr[r + 1]], axis=0) for r in range(R)])


@pytest.mark.parametrize("words", [4, 8, 3])  # Dm = 128, 256 (16-byte pieces) and a width that takes the word-by-word form
def test_or_of_the_routing_bits_equals_numpy(ops, graph_np, words):
    run_ptr = graph_np["run_ptr"]
    E, R = int(run_ptr[-1]), run_ptr.shape[0] - 1
    rng = np.random.default_rng(words)
    bits_np = rng.integers(0, 2 ** 32, (E + R, words), dtype=np.uint64).astype(np.uint32)
    bits = _dev(bits_np.view(np.int32))
    _or_runs(ops, bits, _dev(run_ptr), E, R)
    got = bits.cpu().numpy().view(np.uint32)
    assert np.array_equal(got[:E], bits_np[:E])                             # the message rows are read only
    assert np.array_equal(got[E:], _np_or(bits_np[:E], run_ptr, R))


@pytest.mark.parametrize("Dm", [128, 256])
def test_masks_of_a_run_are_disjoint_on_bits_from_the_segmented_max(ops, graph_np, Dm):
    """What the whole change rests on: the max gives every (node, channel) to ONE message, so popcount(OR over a run) is the sum
    of the members' popcounts -- also where messages tie exactly (duplicate edges: identical rows) and where one is NaN."""
    gd = graph_np
    run_ptr = gd["run_ptr"]
    E, R = int(run_ptr[-1]), run_ptr.shape[0] - 1
    torch.manual_seed(Dm)
    pre = torch.randn(E, Dm)
    src, tgt = gd["msg_src"], gd["msg_tgt"]
    key = src.astype(np.int64) * N_NODES + tgt                              # duplicate edges inside a type carry identical messages
    for t in range(T_TYPES):
        lo, hi = gd["type_ptr"][t], gd["type_ptr"][t + 1]
        _, first = np.unique(key[lo:hi], return_index=True)
        rep = {int(k): lo + int(f) for k, f in zip(key[lo:hi][first], first)}
        idx = np.array([rep[int(k)] for k in key[lo:hi]], dtype=np.int64)
        pre[lo:hi] = pre[torch.from_numpy(idx)]
    pre[int(run_ptr[3]), 5] = float("nan")
    pre[int(gd["tgt_msgs"][gd["tgt_ptr"][7] + 3]), :] = float("nan")        # a whole NaN message inside the long run's node
    res = ops.segment_max(_dev(pre), _dev(gd["tgt_ptr"]), _dev(gd["tgt_msgs"]), N_NODES, want_bits=True, seg_order=_dev(gd["node_order"]))
    bits_e = res[-1]
    assert bits_e.shape == (E, Dm // 32)
    bits = torch.zeros((E + R, Dm // 32), dtype=torch.int32, device="cuda")
    bits[:E] = bits_e
    _or_runs(ops, bits, _dev(run_ptr), E, R)
    got = bits.cpu().numpy().view(np.uint32)
    pop = lambda a: np.unpackbits(a.view(np.uint8), axis=-1).sum(-1).astype(np.int64)
    member_sum = np.add.reduceat(pop(got[:E]), run_ptr[:-1].astype(np.int64))
    assert np.array_equal(pop(got[E:]), member_sum)
    assert np.array_equal(got[E:], _np_or(got[:E], run_ptr, R))
    assert (pop(got[:E]).reshape(-1) > 0).any() and member_sum.max() > 1


@pytest.mark.parametrize("split", [None, 96])
def test_segmented_sums_over_the_run_row_layout_match_index_add(ops, graph_np, split):
    """bl_mp_scatter_grad_runs: source halves at rows 0..E-1 through the source CSR, target halves at rows E..E+R-1 through the run
    CSR, both at column 0; node 7 (120 source rows + its run rows) takes the four-wave hub path.  Bound: fp32 summation of d terms in any order
    errs by at most d x 2^-24 x sum |terms|, per node."""
    gd = graph_np
    Din = 128
    E, R = gd["msg_tgt"].shape[0], gd["run_ptr"].shape[0] - 1
    torch.manual_seed(0)
    g_a = torch.randn(E + R, Din)
    rows_to_node = torch.from_numpy(np.concatenate([gd["msg_src"], gd["bwd_rows_tgt"][E:]]).astype(np.int64))
    ref = torch.zeros(N_NODES, Din, dtype=torch.float64).index_add_(0, rows_to_node, g_a.double())
    mag = torch.zeros(N_NODES, Din, dtype=torch.float64).index_add_(0, rows_to_node, g_a.double().abs())
    deg = torch.zeros(N_NODES, dtype=torch.float64).index_add_(0, rows_to_node, torch.ones(E + R, dtype=torch.float64))
    assert deg[7] >= 64                                                    # the hub split's threshold
    lo = torch.full((N_NODES, Din if split is None else split), float("nan"), device="cuda")
    hi = None if split is None else torch.full((N_NODES, Din - split), float("nan"), device="cuda")
    d = {k: _dev(gd[k]) for k in ("src_ptr", "src_msgs", "tgt_run_ptr", "tgt_run_rows", "node_order")}
    d_ga = _dev(g_a)
    ops._check(ops.load_library().bl_mp_scatter_grad_runs(d_ga.data_ptr(), Din, d["src_ptr"].data_ptr(), d["src_msgs"].data_ptr(),
                                                          d["tgt_run_ptr"].data_ptr(), d["tgt_run_rows"].data_ptr(), N_NODES, Din,
                                                          Din if split is None else split, lo.data_ptr(), lo.stride(0),
                                                          hi.data_ptr() if hi is not None else None, hi.stride(0) if hi is not None else 0,
                                                          d["node_order"].data_ptr(), int(gd["num_hub_nodes"]),
                                                          torch.cuda.current_stream().cuda_stream), "bl_mp_scatter_grad_runs")
    got = (lo if hi is None else torch.cat([lo, hi], 1)).cpu().double()
    err = (got - ref).abs()
    bound = deg[:, None] * 2.0 ** -24 * mag
    print(f"segmented sums: worst error {float(err.max()):.3e}, worst error / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all())


def _layer_case(Din, Dm, pair, seed):
    torch.manual_seed(seed)
    Dout = 128
    h = torch.tanh(torch.randn(N_NODES, Din)) * 1.25
    p = {"W": torch.randn(T_TYPES, 2 * Din, Dm) / math.sqrt(2 * Din), "ln_g": 1.0 + 0.1 * torch.randn(Dm), "ln_b": 0.1 * torch.randn(Dm),
         "Wd": torch.randn(Dm, Dout) / math.sqrt(Dm), "bd": 0.1 * torch.randn(Dout)}
    g_out = torch.randn(N_NODES, Dout)
    return h, p, g_out, (Din // 2 if pair else None)


def _run_layer(ops, graph, h, p, g_out, split):
    """forward + backward of the one-call layer -> (gradients on the host, winner table)"""
    leaf = lambda t: t.cuda().requires_grad_(True)
    P = {k: leaf(v) for k, v in p.items()}
    if split is None:
        h_in = [leaf(h)]
        arg = h_in[0]
    else:
        h_in = [leaf(h[:, :split].contiguous()), leaf(h[:, split:].contiguous())]
        arg = tuple(h_in)
    ops.WINNER_SINK = []
    try:
        out = ops.mp_layer(arg, P["W"], P["ln_g"], P["ln_b"], P["Wd"], P["bd"], graph, "gelu_aggregated")
        winner = ops.WINNER_SINK[0].cpu()
    finally:
        ops.WINNER_SINK = None
    out.backward(g_out.cuda())
    ops.join_side_stream()
    torch.cuda.synchronize()
    grads = {k: v.grad.cpu() for k, v in P.items()}
    grads["h"] = torch.cat([t.grad for t in h_in], 1).cpu()
    return grads, winner


def _fp64_layer_grads(gd, h, p, g_out, winner):
    """the layer in fp64 with the routing (winner per node and channel) taken from the device's forward pass"""
    src, tgt = torch.from_numpy(gd["msg_src"].astype(np.int64)), torch.from_numpy(gd["msg_tgt"].astype(np.int64))
    typ = torch.from_numpy(np.repeat(np.arange(T_TYPES), np.diff(gd["type_ptr"])).astype(np.int64))
    h64 = h.double().requires_grad_(True)
    P = {k: v.double().requires_grad_(True) for k, v in p.items()}
    a = torch.cat([h64[src], h64[tgt]], 1)
    pre = torch.zeros(src.shape[0], P["W"].shape[2], dtype=torch.float64)
    for t in range(T_TYPES):
        m = typ == t
        pre = pre.index_put((torch.nonzero(m)[:, 0],), a[m] @ P["W"][t])
    w = winner.long()
    agg = torch.where(w >= 0, pre.gather(0, w.clamp_min(0)), torch.zeros((), dtype=torch.float64))
    act = torch.nn.functional.gelu(agg)
    ln = torch.nn.functional.layer_norm(act, (act.shape[1],), P["ln_g"], P["ln_b"], 1e-5)
    out = torch.tanh(ln @ P["Wd"] + P["bd"])
    out.backward(g_out.double())
    ref = {k: v.grad for k, v in P.items()}
    ref["h"] = h64.grad
    return ref


@pytest.fixture
def deterministic_mode(ops):
    def set_(on):
        ops.set_deterministic(on)
    yield set_
    ops.set_deterministic(False)


@pytest.mark.parametrize("Din,Dm,pair", [(128, 128, False), (256, 256, False), (256, 128, True)])
@pytest.mark.parametrize("deterministic", [False, True])
def test_layer_backward_with_and_without_run_arrays(ops, graph_np, deterministic_mode, Din, Dm, pair, deterministic):
    """bl_mp_layer_bwd on the same inputs, per message (no run arrays; and run arrays with the switch off) and per run: g_h and g_W
    of every path against the fp64 layer with the device's routing, bound 2e-6 x max(1, largest reference entry) -- the bound of
    test_routed_input_gradient_from_the_nonzeros_matches_fp64.  The other gradients (ln_g, ln_b, Wd, bd) come from code the run rows
    do not touch: bit-equal between the paths in the deterministic mode, the one mode in which two calls of ONE path are
    bit-equal at all (otherwise their column sums and chunk flushes are unordered fp32 atomics).  Deterministic mode also pins
    that two runs of the run-row path are bit-equal in every gradient."""
    assert ops.msg_gemm_mode() == "f16x3" and not ops._use_vector_dgrad(ops.load_library(), 1500, Dm, 2 * Din)
    deterministic_mode(deterministic)
    h, p, g_out, split = _layer_case(Din, Dm, pair, seed=Din + Dm)
    plain, with_runs = _graph_index(ops, graph_np, False), _graph_index(ops, graph_np, True)
    old, winner = _run_layer(ops, plain, h, p, g_out, split)
    new, winner_new = _run_layer(ops, with_runs, h, p, g_out, split)
    assert torch.equal(winner, winner_new)                                  # forward is the same code: same routing
    prev = ops.set_run_rows(False)
    try:
        off, _ = _run_layer(ops, with_runs, h, p, g_out, split)             # the switch: the per-message launches on the same arrays
    finally:
        ops.set_run_rows(prev)
    ref = _fp64_layer_grads(graph_np, h, p, g_out, winner)
    for name, got in (("per message", old), ("switch off", off), ("per run", new)):
        for k in ("h", "W"):
            scale = max(1.0, float(ref[k].abs().max()))
            err = float((got[k].double() - ref[k]).abs().max())
            print(f"Din {Din} Dm {Dm} pair {pair} det {deterministic} {name}: g_{k} error {err:.3e}, largest entry {float(ref[k].abs().max()):.3e}")
            assert err < 2e-6 * scale, (name, k, err, scale)
    assert float((new["W"] - old["W"]).abs().max()) > 0 or float((new["h"] - old["h"]).abs().max()) > 0  # (another summation: it did run)
    if deterministic:
        for k in ("ln_g", "ln_b", "Wd", "bd"):
            assert torch.equal(new[k], old[k]) and torch.equal(off[k], old[k]), k
        for k in ("h", "W"):
            assert torch.equal(off[k], old[k]), k                           # switch off = today's launches, bit for bit
        again, _ = _run_layer(ops, with_runs, h, p, g_out, split)
        for k in new:
            assert torch.equal(again[k], new[k]), k
