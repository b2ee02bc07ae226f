"""GPU: the live rows of bl_mp_layer_fwd -- the FORWARD of the last message-passing layers over the rows the heads' one gather can
reach (bl_mp_layer_t.live_fwd), against the full forward of the same build (hip_ops.set_live_forward(False)) and the fp64 oracle.

A row the live forward computes is computed by the same arithmetic on the same inputs as in the full forward (the row GEMMs and
the per-node kernels are row-local, the dropout counter is the node's own row), so on the live rows every layer output and every
piece of the saved state is BIT-equal between the two, and so is the loss.  Gradients then differ only by the order of the fp32
atomics, as between any two runs: they are held to what tests/test_live_backward_gpu.py holds its two paths to -- each inside the
1e-4 parity bound of the fp64 oracle, the live one's largest error at most twice the full one's.

Shapes: hidden 128, 4 layers of the concat recipe (the last layer has Din = Dm = 256), 4 edge types, 2 graphs of 150 nodes / 700
messages with 5 candidates each, dropout 0.2; BL_LIVE_LAYERS=4 BL_LIVE_FRACTION=1.0 for the deep cases, the collators' defaults
for one."""
import ctypes
import math

import numpy as np
import pytest
import torch

from oracle import buglab_oracle as O
from tests import helpers as Hh
from tests.test_live_backward_gpu import TOL, _base, _cands, _case_hub, _case_lonely, _oracle_with_routing, _worst

pytestmark = pytest.mark.gpu

T, H = 4, 128
I32 = np.int32
DROP, SEED = 0.2, 777


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from buglab.models import hip_ops

    hip_ops.load_library()
    return hip_ops


# ---- the minibatches ------------------------------------------------------------------------------------------------------
def _case_isolated():
    """no message into any head row: the last layer's E' is 0, and so is every layer's below it (recv = nodes)"""
    samples = _base(seed=5, n_var=0, n_swap=0)
    for s in samples:
        g = s.graph_data
        g.adjacency_lists[:] = [a[~np.isin(a[:, 1], _cands(s))] for a in g.adjacency_lists]
    return samples


def _case_powerlaw():
    """power-law in-degree (node 0 of every graph receives 64 messages) with node 0 a head row: a live segment above the 40 items
    from which the full forward hands a segment to a whole workgroup -- the live forward scans it with one wave"""
    samples = _base(seed=9, n_var=0, n_swap=0, degree="powerlaw", max_degree=64)
    for s in samples:
        _cands(s)[0] = 0
    return samples


#         name: (samples, message-passing layers, BL_LIVE_LAYERS / BL_LIVE_FRACTION or None for the defaults)
CASES = {
    "defaults": (lambda: _base(seed=0, n_var=0, n_swap=0), 4, None),
    "every_layer_live": (lambda: _base(seed=0, n_var=0, n_swap=0), 4, (4, 1.0)),
    "live_node_without_incoming_message": (_case_lonely, 4, (4, 1.0)),
    "no_live_message": (_case_isolated, 4, (4, 1.0)),
    "powerlaw_hub_is_live": (_case_powerlaw, 4, (4, 1.0)),
    "hub_with_runs_is_live": (_case_hub, 4, (4, 1.0)),
    # (larger, sparser graphs with two head rows each: the live sets grow slowly enough for six layers, the lower concat layer among them)
    "concat_layer_inside_the_run": (lambda: _base(seed=11, n=900, E=1800, C_=2, n_var=0, n_swap=0), 8, (6, 1.0)),
}


def _collate(samples, monkeypatch, limits):
    from buglab.data.collate import collate_samples

    if limits is not None:
        monkeypatch.setenv("BL_LIVE_LAYERS", str(limits[0]))
        monkeypatch.setenv("BL_LIVE_FRACTION", repr(limits[1]))
    return collate_samples(samples, T)


def _module(layers, params=None, dropout=DROP):
    cfg = O.OracleConfig(hidden=H, num_layers=layers, num_edge_types=T, vocab_size=300, dropout=dropout)
    params = O.init_params(cfg, seed=0) if params is None else params
    return cfg, params, Hh.build_module_like(cfg, params)


# ---- what a layer call left behind ------------------------------------------------------------------------------------------
def _al(b):
    return (b + 255) & ~255


def _carve_saved(blob, N, bit_rows, Din, Dm, has_dact):
    """the pieces of the fused layer's saved blob (csrc/bl_mp_layer.hip, carve_saved) as typed views"""
    out, o = {}, 0

    def take(name, nbytes, dtype, shape):
        nonlocal o
        out[name] = blob[o:o + nbytes].view(dtype).view(*shape)
        o += _al(nbytes)

    take("hp", N * 3 * Din * 2, torch.int16, (N, 3 * Din))      # (sized for bf16x3; the f16x2 image is the [N, 2 Din] at its front)
    if has_dact:
        take("dact", N * Dm * 4, torch.int32, (N, Dm))
    take("bits", bit_rows * (Dm // 32) * 4, torch.int32, (bit_rows, Dm // 32))
    take("agg", N * Dm * 4, torch.int32, (N, Dm))
    take("mean", N * 4, torch.int32, (N,))
    take("rstd", N * 4, torch.int32, (N,))
    take("ln_out", N * Dm * 6, torch.int16, (N, 3 * Dm))
    out["hp"] = blob[:N * 2 * Din * 2].view(torch.int16).view(N, 2 * Din)
    assert o == blob.numel(), (o, blob.numel())
    return out


class _Capture:
    """forward hooks on the message-passing layers: each call's output, graph index and saved blob (copied before backward)"""

    def __init__(self, module):
        self.calls = []
        self._handles = [l.register_forward_hook(self._hook) for l in module._gnn.mp]

    def _hook(self, layer, inputs, out):
        saved = out.grad_fn.saved
        g, blob = saved[7], saved[10]
        self.calls.append({"out": out.detach().clone(), "g": g, "blob": blob.clone(), "Din": saved[0] + saved[1], "Dm": layer.W.shape[2],
                           "act": saved[8]})

    def close(self):
        for h in self._handles:
            h.remove()


def _step(ops, module, mb_np, fwd_on, bwd_on=True, sink=False, seed=SEED, capture=True, mutate=None, grad=True):
    """one training step -> loss, gradients, per-layer captures, profiler kinds, winners"""
    from buglab.data.collate import to_device

    prev_f, prev_b = ops.set_live_forward(fwd_on), ops.set_live_backward(bwd_on)
    cap = _Capture(module) if capture else None
    if sink:
        ops.WINNER_SINK = []
    try:
        mb = to_device(mb_np, "cuda")
        if mutate:
            mutate(mb)
        module.zero_grad(set_to_none=True)
        module.train(True)
        module.reset_metrics()
        with ops.KernelTimer() as timer:
            if grad:
                loss = module(**mb, dropout_seed=seed)
                loss.backward()
            else:
                with torch.no_grad():
                    loss = module(**mb, dropout_seed=seed)
            ops.join_side_stream()
            torch.cuda.synchronize()
            kinds = timer.summary()
        winners = [w.cpu().numpy().astype(np.int64) for w in ops.WINNER_SINK] if sink else None
    finally:
        ops.set_live_forward(prev_f)
        ops.set_live_backward(prev_b)
        ops.WINNER_SINK = None
        if cap:
            cap.close()
    grads = {k: v.clone() for k, v in Hh.module_grads(module).items()} if grad else None
    return float(loss.detach()), grads, (cap.calls if cap else None), kinds, winners


def _launches(kinds, name):
    return kinds.get(name, {"launches": 0})["launches"]


def _flop(kinds, name):
    return kinds.get(name, {"flop": 0.0})["flop"]


# ---- 1 + 2: switch on against switch off, same seed -------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_live_forward_equals_the_full_forward_on_the_live_rows(ops, monkeypatch, case):
    assert ops.msg_gemm_mode() == "f16x3"
    make, layers, limits = CASES[case]
    mb_np = _collate(make(), monkeypatch, limits)
    gd = mb_np["graph_data"]
    layout = [tuple(int(x) for x in row[:4]) for row in gd["live_layout"]]
    N, E = int(gd["token_ids"].shape[0]), int(gd["msg_src"].shape[0])
    cfg, params, module = _module(layers)
    loss_off, g_off, c_off, k_off, _ = _step(ops, module, mb_np, False)
    loss_on, g_on, c_on, k_on, _ = _step(ops, module, mb_np, True)
    _, _, _, k_sink, winners = _step(ops, module, mb_np, True, sink=True, capture=False)
    # the run of live-forward layers: from the top, as long as the compact pre-activations [E', Dm] with the message-position map
    # [E] and the target ids [E'] behind them fit the full forward's [E, Dm] workspace (a layer with every message live cannot)
    widths = ([(H, H)] * 3 + [(2 * H, 2 * H)]) * (layers // 4)
    fits = lambda ex, dm: _al(ex * dm * 4) + _al(E * 4) + _al(ex * 4) <= _al(E * dm * 4)
    depth = 0
    while depth < len(layout) and fits(layout[depth][2], widths[layers - 1 - depth][1]):
        depth += 1
    layout = layout[:depth]
    print(f"{case}: live layers (N', N'', E', R') from the last layer down {layout}; loss off {loss_off!r} on {loss_on!r}")

    # which layers ran live: the top `depth` ones with the switch on, none with it off or with a winner table wanted
    assert [c["g"].live_fwd for c in c_off] == [0] * layers
    want = [0] * (layers - depth) + [ops.LIVE_FWD_INNER] * (depth - 1) + [ops.LIVE_FWD_LAST]
    assert [c["g"].live_fwd for c in c_on] == want, ([c["g"].live_fwd for c in c_on], want)
    with_msgs = sum(1 for (_, _, ex, _) in layout if ex > 0)
    assert _launches(k_on, "live_index_fwd") == with_msgs and "live_index_fwd" not in k_off and "live_index_fwd" not in k_sink
    assert _launches(k_on, "dense_fwd") == _launches(k_off, "dense_fwd") == layers
    assert _launches(k_on, "msg_gemm_h3") == layers - depth + with_msgs and _launches(k_off, "msg_gemm_h3") == layers
    # the profiler accounts the live launches with their own sizes: 2 N' Dm Dout per dense update, 2 E' 2 Din Dm per message GEMM
    dims = [(c["Din"], c["Dm"]) for c in c_on]
    full = lambda i: (2.0 * N * dims[i][1] * H, 2.0 * E * 2 * dims[i][0] * dims[i][1])
    live_ = lambda i, d: (2.0 * layout[d][0] * dims[i][1] * H, 2.0 * layout[d][2] * 2 * dims[i][0] * dims[i][1])
    want_flop = [full(i) if i < layers - depth else live_(i, layers - 1 - i) for i in range(layers)]
    assert _flop(k_on, "dense_fwd") == pytest.approx(sum(w[0] for w in want_flop), rel=1e-9)
    assert _flop(k_on, "msg_gemm_h3") == pytest.approx(sum(w[1] for w in want_flop), rel=1e-9, abs=1e-9)

    # the properties the case is there for
    if limits is not None:
        assert depth >= min(layers, limits[0]) - 2 and depth >= 3, layout
        assert any(nn % 64 != 0 and nn % 128 != 0 and ex % 128 != 0 for (nn, _, ex, _) in layout if ex > 0) or with_msgs == 0
    else:
        assert 1 <= depth < layers, layout
    indeg = np.diff(gd["tgt_ptr"])
    live_nodes = [c["g"].live.nodes.cpu().numpy() for c in c_on[layers - depth:]][::-1]   # the last layer first, like `layout`
    if case == "live_node_without_incoming_message":
        assert any((indeg[n] == 0).any() and ex > 0 for n, (_, _, ex, _) in zip(live_nodes, layout))
    if case == "no_live_message":
        assert with_msgs == 0 and all(ex == 0 for (_, _, ex, _) in layout) and depth == layers == 4
    if case in ("powerlaw_hub_is_live", "hub_with_runs_is_live"):
        assert gd["num_hub_nodes"] >= 1 and indeg[live_nodes[0]].max() > 40, (gd["num_hub_nodes"], indeg[live_nodes[0]].max())
    if case == "concat_layer_inside_the_run":
        assert dims[7] == (256, 256) and dims[3] == (256, 256) and want[3] == ops.LIVE_FWD_INNER and want[2] == ops.LIVE_FWD_INNER and want[1] == 0

    # bit-equal on the live rows: every live layer's output and saved state; the loss
    R = int(gd["run_ptr"].shape[0]) - 1
    for i in range(layers - depth, layers):
        a, b = c_on[i], c_off[i]
        lv = a["g"].live
        nodes, recv, msgs = lv.nodes.long(), lv.recv.long(), lv.msgs.long()
        assert torch.equal(a["out"][nodes], b["out"][nodes]), f"layer {i}: output"
        sa, sb = (_carve_saved(c["blob"], N, E + R, c["Din"], c["Dm"], c["act"] != ops.ACT_NONE) for c in (a, b))
        for name, rows in (("agg", nodes), ("dact", nodes), ("mean", nodes), ("rstd", nodes), ("ln_out", nodes), ("bits", msgs), ("hp", recv)):
            assert torch.equal(sa[name][rows], sb[name][rows]), f"layer {i}: saved {name}"
    assert loss_on == loss_off and math.isfinite(loss_on)

    # the output handed out: exactly zero off the last layer's live rows (the full forward's is not)
    dead = torch.ones(N, dtype=torch.bool, device="cuda")
    dead[c_on[-1]["g"].live.nodes.long()] = False
    assert bool((c_on[-1]["out"][dead] == 0).all()) and bool((c_off[-1]["out"][dead] != 0).any())

    # gradients: both inside the parity bound of the fp64 oracle (its routing = the device's), the live forward's largest error at
    # most twice the full forward's -- the relation tests/test_live_backward_gpu.py holds its two paths to
    out, ref = _oracle_with_routing(cfg, params, mb_np, SEED, winners)
    w_off, per_off = _worst(g_off, ref)
    w_on, per_on = _worst(g_on, ref)
    print(f"  oracle loss {float(out['loss'].detach()):.7f}; worst relative gradient error off {w_off:.3e} on {w_on:.3e}")
    assert abs(loss_on - float(out["loss"].detach())) < TOL
    for name, per in (("off", per_off), ("on", per_on)):
        for k, (d, scale) in per.items():
            assert d <= TOL * scale + 1e-6, (name, k, d, scale)
    assert w_on <= 2.0 * w_off, (w_on, w_off)


# ---- 3: fallbacks -----------------------------------------------------------------------------------------------------------
def _modes(ops):
    return {
        "bf16x6": (lambda: ops.set_msg_gemm_mode("bf16x6"), lambda p: ops.set_msg_gemm_mode(p)),
        "f16x1": (lambda: ops.set_msg_gemm_mode("f16x1"), lambda p: ops.set_msg_gemm_mode(p)),
    }


@pytest.mark.parametrize("how", ["no_grad", "winner_sink", "input_transform", "bf16x6", "f16x1", "deterministic"])
def test_everything_the_live_forward_excludes_runs_the_full_forward(ops, monkeypatch, how):
    kw, restore = {}, None
    if how == "deterministic":  # (switched before collating: the collator lays the minibatch out for the ordered kernels)
        monkeypatch.setenv("BL_DETERMINISTIC", "1")
        prev, restore = ops.deterministic(), ops.set_deterministic
        ops.set_deterministic(True)
    mb_np = _collate(_base(seed=0, n_var=0, n_swap=0), monkeypatch, (4, 1.0))
    _, _, module = _module(4)
    if how == "no_grad":
        kw = {"grad": False, "capture": False}
    elif how == "winner_sink":
        kw = {"sink": True}
    elif how == "input_transform":
        kw = {"mutate": lambda mb: mb["graph_data"].__setitem__("input_transform", lambda h: h)}
    elif how != "deterministic":
        flip, restore = _modes(ops)[how]
        prev = flip()
    try:
        loss, _, calls, kinds, _ = _step(ops, module, mb_np, True, **kw)
    finally:
        if restore:
            restore(prev)
    assert "live_index_fwd" not in kinds and math.isfinite(loss)
    assert _launches(kinds, "dense_fwd") == 4 and kinds["dense_fwd"]["flop"] == pytest.approx(2.0 * 300 * (3 * H + 2 * H) * H, rel=1e-9)  # (the last layer is 2 H wide)
    if calls is not None:
        assert [c["g"].live_fwd for c in calls] == [0, 0, 0, 0]


def test_layers_below_a_layer_that_cannot_run_live_run_in_full(ops, monkeypatch):
    """[Mlp, Gated, Mlp, Mlp]: the two layers above the GGNN layer run live, the GGNN layer and the layer below it in full (launch
    shapes from the profiler), and the result equals the switch-off run's on the head rows."""
    from buglab.data.collate import to_device
    from buglab.models.layers import messagepassing as M

    mb_np = _collate(_base(seed=0, n_var=0, n_swap=0), monkeypatch, (4, 1.0))
    layout = [tuple(int(x) for x in row[:4]) for row in mb_np["graph_data"]["live_layout"]]
    torch.manual_seed(0)
    mlp = lambda: M.MlpMessagePassingLayer(H, H, H, T, dropout_rate=DROP)
    gnn = M.GraphNeuralNetwork(M.SubtokenEmbedder(300, H), [mlp(), M.GatedMessagePassingLayer(H, H, T, dropout_rate=DROP), mlp(), mlp()]).cuda().train()
    gd = to_device(mb_np, "cuda")["graph_data"]
    heads = gd["head_gather_idx"].long()
    N, E = 300, int(gd["msg_src"].shape[0])

    def run(fwd_on):
        prev = ops.set_live_forward(fwd_on)
        try:
            gnn.zero_grad(set_to_none=True)
            with ops.KernelTimer() as timer:
                out = gnn(**gd, dropout_seed=SEED, live_backward=True).output_node_representations
                out[heads].square().sum().backward()
                ops.join_side_stream()
                torch.cuda.synchronize()
                return out.detach()[heads].clone(), {k: p.grad.clone() for k, p in gnn.named_parameters()}, timer.summary()
        finally:
            ops.set_live_forward(prev)

    h_off, g_off, k_off = run(False)
    h_on, g_on, k_on = run(True)
    assert torch.equal(h_on, h_off)
    assert _launches(k_on, "live_index_fwd") == 2 and "live_index_fwd" not in k_off
    # what the two live layers leave out, by the profiler's own accounting of the launch shapes (whatever the GGNN layer adds is in both)
    assert _flop(k_off, "dense_fwd") - _flop(k_on, "dense_fwd") == pytest.approx(2.0 * (2 * N - layout[1][0] - layout[0][0]) * H * H, rel=1e-6)
    assert _flop(k_off, "msg_gemm_h3") - _flop(k_on, "msg_gemm_h3") == pytest.approx(2.0 * (2 * E - layout[1][2] - layout[0][2]) * 2 * H * H, rel=1e-6)
    for k in g_off:  # the parity bound relative to the gradient's largest entry, between the two runs
        scale = float(g_off[k].abs().max())
        assert float((g_on[k] - g_off[k]).abs().max()) <= TOL * scale + 1e-6, k


def test_backward_switch_flipped_after_a_live_forward_is_an_error_not_a_wrong_result(ops, monkeypatch):
    """forward ran over the live rows, then someone switches the live backward off: the full backward would read saved state nobody
    computed.  bl_mp_layer_bwd refuses with a text that says so; no NaN ever reaches a gradient."""
    from buglab.data.collate import to_device

    mb_np = _collate(_base(seed=0, n_var=0, n_swap=0), monkeypatch, (4, 1.0))
    _, _, module = _module(4)
    module.train(True)
    module.zero_grad(set_to_none=True)
    prev_f, prev_b = ops.set_live_forward(True), ops.set_live_backward(True)
    try:
        loss = module(**to_device(mb_np, "cuda"), dropout_seed=SEED)
        ops.set_live_backward(False)
        with pytest.raises(Exception) as err:
            loss.backward()
        ops.join_side_stream()
        torch.cuda.synchronize()
    finally:
        ops.set_live_forward(prev_f)
        ops.set_live_backward(prev_b)
    text = str(err.value)
    assert "forward ran over its live rows" in text and "live backward is switched off" in text, text
    for p in module.parameters():
        assert p.grad is None or bool(torch.isfinite(p.grad).all())


# ---- 5: guard bands and poisoned dead rows, on the C call itself ------------------------------------------------------------
GUARD = 4096  # bytes of poison in front of and behind every buffer the call writes


def _graph_index(ops, gd, T_):
    from buglab.models.hip_ops import GraphIndex, MessageRuns, live_rows_of

    runs = MessageRuns.of(*(gd[k] for k in ("run_ptr", "bwd_group_ptr", "bwd_group_w", "bwd_rows_tgt", "bwd_rows_src", "tgt_run_ptr", "tgt_run_rows")))
    g = GraphIndex(gd["msg_src"], gd["msg_tgt"], gd["type_ptr"], gd["tgt_ptr"], gd["tgt_msgs"], gd["src_ptr"], gd["src_msgs"],
                   int(gd["num_nodes"]), int(gd["num_messages"]), T_, gd.get("node_order"), int(gd.get("num_hub_nodes", -1)), runs)
    return g, live_rows_of(gd["live_arrays"], gd["live_layout"], T_)


def _banded(nbytes, fill):
    buf = torch.full((nbytes + 2 * GUARD,), fill, dtype=torch.uint8, device="cuda")
    return buf, buf[GUARD:GUARD + nbytes]


@pytest.mark.parametrize("concat", [False, True])
@pytest.mark.parametrize("depth", [0, 1])
def test_nothing_outside_the_live_set_is_read_or_written(ops, monkeypatch, concat, depth):
    """bl_mp_layer_fwd with live_fwd on buffers of the caller: the input NaN outside the rows live_recv, poison bands around the
    workspace (compact pre | message positions | target ids), the saved blob and h_out.  The live rows of the output and of the
    saved state equal the full call's on the clean input bit for bit, the bands and (inner form) every other row of h_out keep
    their poison, the LAST form's other rows are zero."""
    from buglab.data.collate import to_device
    from buglab.models.hip_ops.weights import _packed_layer_weights, _packed_message_weights

    mb_np = _collate(_case_hub(), monkeypatch, (4, 1.0))
    gd = to_device(mb_np, "cuda")["graph_data"]
    g, live = _graph_index(ops, gd, T)
    lv = live[depth]
    N, E, R = g.num_nodes, g.num_messages, g.runs.num_runs
    Din, Dm, Dout = (2 * H, 2 * H, H) if concat else (H, H, H)
    torch.manual_seed(depth + 2 * concat)
    W = (torch.randn(T, 2 * Din, Dm) / math.sqrt(2 * Din)).cuda().requires_grad_()
    ln_g, ln_b = (1.0 + 0.1 * torch.randn(Dm)).cuda(), (0.1 * torch.randn(Dm)).cuda()
    Wd, bd = (torch.randn(Dm, Dout) / math.sqrt(Dm)).cuda().requires_grad_(), (0.1 * torch.randn(Dout)).cuda()
    h = torch.tanh(torch.randn(N, Din)).cuda()
    lo, hi = (h[:, :H].contiguous(), h[:, H:].contiguous()) if concat else (h, None)
    drop = ops.Dropout(DROP, SEED, 3)
    lib = ops.load_library()
    wkn = _packed_message_weights(W, Din, True)[0]
    wd_kn = _packed_layer_weights(Wd, True)[0]
    nodes, recv, msgs = lv.nodes.long(), lv.recv.long(), lv.msgs.long()
    Ex = int(msgs.shape[0])
    assert Ex > 0 and Ex % 128 != 0 and int(nodes.shape[0]) % 64 != 0

    def call(live_fwd, lo_, hi_):
        L = ops._layer_desc(g._replace(live=lv), W, ln_g, ln_b, Wd, bd, Din, ops.ACT_GELU_AGG, drop, 0, live_fwd=live_fwd)
        L.Wd_packed = wd_kn.data_ptr()
        if live_fwd:
            assert lib.bl_mp_layer_live_ok(ctypes.byref(L), 1, 1, 0) == 1, lib.bl_last_error()
        saved = _banded(lib.bl_mp_layer_saved_bytes(N, E + R, Din, Dm, ops.ACT_GELU_AGG), 0xEE)
        ws = _banded(lib.bl_mp_layer_workspace_bytes(N, E, Din, Dm, Dout, 0), 0xEE)
        out = _banded(N * Dout * 4, 0xEE)
        ops._check(lib.bl_mp_layer_fwd(ctypes.byref(L), lo_.data_ptr(), lo_.stride(0), lo_.shape[1], hi_.data_ptr() if hi_ is not None else None,
                                       hi_.stride(0) if hi_ is not None else 0, wkn.data_ptr(), out[1].data_ptr(), None, saved[1].data_ptr(),
                                       ws[1].data_ptr(), torch.cuda.current_stream().cuda_stream), "bl_mp_layer_fwd")
        torch.cuda.synchronize()
        return saved, ws, out

    def poisoned(x):
        y = torch.full_like(x, float("nan"))
        y[recv] = x[recv]
        return y

    s_full, _, o_full = call(0, lo, hi)
    code = ops.LIVE_FWD_LAST if depth == 0 else ops.LIVE_FWD_INNER
    s_live, w_live, o_live = call(code, poisoned(lo), poisoned(hi) if hi is not None else None)
    for buf, _ in (s_live, w_live, o_live):
        assert bool((buf[:GUARD] == 0xEE).all()) and bool((buf[-GUARD:] == 0xEE).all())
    # the workspace: [compact pre | msg_pos [E] | tgt_id [E']], each piece 256-byte aligned; nothing behind it, and of the position
    # map only the live messages' entries
    pre_b, pos_b, tgt_b = _al(Ex * Dm * 4), _al(E * 4), _al(Ex * 4)
    ws = w_live[1]
    assert pre_b + pos_b + tgt_b <= ws.numel() and bool((ws[pre_b + pos_b + tgt_b:] == 0xEE).all())
    pos = ws[pre_b:pre_b + E * 4].view(torch.int32)
    dead_msgs = torch.ones(E, dtype=torch.bool, device="cuda")
    dead_msgs[msgs] = False
    assert torch.equal(pos[msgs], torch.arange(Ex, dtype=torch.int32, device="cuda")) and bool((pos[dead_msgs] == -286331154).all())  # 0xEEEEEEEE
    assert torch.equal(ws[pre_b + pos_b:pre_b + pos_b + Ex * 4].view(torch.int32), gd["msg_tgt"][msgs])
    assert bool(torch.isfinite(ws[:Ex * Dm * 4].view(torch.float32)).all())
    # the output and the saved state
    of, ol = o_full[1].view(torch.float32).view(N, Dout), o_live[1].view(torch.float32).view(N, Dout)
    assert torch.equal(ol[nodes], of[nodes]) and bool(torch.isfinite(ol[nodes]).all())
    dead = torch.ones(N, dtype=torch.bool, device="cuda")
    dead[nodes] = False
    if depth == 0:
        assert bool((ol[dead] == 0).all())
    else:
        assert bool((ol[dead].view(torch.int32) == -286331154).all())
    sf, sl = (_carve_saved(s[1], N, E + R, Din, Dm, True) for s in (s_full, s_live))
    for name, rows in (("agg", nodes), ("dact", nodes), ("mean", nodes), ("rstd", nodes), ("ln_out", nodes), ("bits", msgs), ("hp", recv)):
        assert torch.equal(sl[name][rows], sf[name][rows]), name
    dead_recv = torch.ones(N, dtype=torch.bool, device="cuda")
    dead_recv[recv] = False
    assert bool((sl["hp"][dead_recv] == -4370).all()) and bool((sl["agg"][dead] == -286331154).all())  # 0xEEEE: never written
