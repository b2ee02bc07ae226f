"""GPU: the live rows of bl_mp_layer_bwd -- the backward of the last message-passing layers over the rows the heads' one gather
can reach (the minibatch's live arrays, buglab.data.collate.live_set_arrays), against the full backward and the fp64 oracle.

Leaving out a row whose gradient is exactly zero removes only additions of zero: with the switch on and off, loss and every
parameter gradient agree up to the order of the unordered fp32 atomics.  Shapes: the smallest at which this can go wrong -- 4
layers (the last one a concat layer), hidden 128, 2 graphs of 150 nodes / 700 messages and 4 edge types with 5 head rows each,
and variations of it (see CASES)."""
import math

import numpy as np
import pytest
import torch

from oracle import buglab_oracle as O
from tests import helpers as Hh

pytestmark = pytest.mark.gpu

T, H, LAYERS = 4, 128, 4
TOL = 1e-4  # the project's parity bound (tests/test_hip_parity.py)
I32 = np.int32


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from buglab.models import hip_ops

    hip_ops.load_library()
    return hip_ops


def _dev(a):
    return torch.as_tensor(a).cuda().contiguous()


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- the minibatches ------------------------------------------------------------------------------------------------------
def _base(seed=0, n=150, E=700, C_=5, B=2, **kw):
    from buglab.data.synthetic import make_samples

    return make_samples(B, seed=seed, num_nodes=n, num_messages=E, num_edge_types=T, vocab_size=300, num_candidates=C_, **kw)


def _cands(s):
    return s.graph_data.reference_nodes["candidate_nodes"]


def _case_lonely():
    samples = _base(seed=3, n_var=0, n_swap=0)
    g = samples[1].graph_data
    lonely = int(_cands(samples[1])[2])
    g.adjacency_lists[:] = [a[a[:, 1] != lonely] for a in g.adjacency_lists]
    return samples


def _case_dead_type():
    samples = _base(seed=4, n_var=0, n_swap=0)
    for s in samples:
        a = s.graph_data.adjacency_lists
        a[1] = a[1][~np.isin(a[1][:, 1], _cands(s))]
        a[2] = np.zeros((0, 2), I32)
    return samples


def _case_hub():
    """a head row with 60 incoming messages of type 0 (12 of them duplicates: runs of length >= 2) that also sends 70 messages"""
    samples = _base(seed=6)
    rng = np.random.default_rng(6)
    g = samples[0].graph_data
    hub = int(_cands(samples[0])[1])
    into = np.stack([rng.integers(0, 150, 48), np.full(48, hub)], axis=1).astype(I32)
    out = np.stack([np.full(70, hub), rng.integers(0, 150, 70)], axis=1).astype(I32)
    g.adjacency_lists[0] = np.concatenate([g.adjacency_lists[0], into, into[:12]])
    g.adjacency_lists[3] = np.concatenate([g.adjacency_lists[3], out])
    return samples


CASES = {
    "five_head_rows_each": (lambda: _base(seed=0, n_var=0, n_swap=0), {}),
    "no_head_rows": (lambda: _base(seed=1, C_=0), {}),
    "every_node_a_head_row": (lambda: _base(seed=2, n=40, E=150, C_=40), {}),
    "head_row_without_incoming_message": (_case_lonely, {}),
    "edge_type_without_live_message": (_case_dead_type, {}),
    "live_hub_and_runs": (_case_hub, {}),
    # more head rows in larger graphs: the second live layer has more than 64 nodes, the first fewer
    "second_layer_above_64_nodes": (lambda: _base(seed=7, n=400, E=1600, C_=12), {}),
    "dropout": (lambda: _base(seed=8), {"dropout": 0.2, "seed": 777}),
}


def _collate(samples):
    from buglab.data.collate import collate_samples

    return collate_samples(samples, T)


def _live_rows(mb_np):
    """per live layer (N', N'', E', R') of the minibatch as collated"""
    return [tuple(int(x) for x in row[:4]) for row in mb_np["graph_data"]["live_layout"]]


def _run(ops, module, mb_np, seed, live_on, sink=False):
    """one training step's forward + backward -> (loss, gradients, winners, launches of the live path's own kernel)"""
    from buglab.data.collate import to_device

    prev = ops.set_live_backward(live_on)
    if sink:
        ops.WINNER_SINK = []
    try:
        mb = to_device(mb_np, "cuda")
        module.zero_grad(set_to_none=True)
        module.train(True)
        module.reset_metrics()
        with ops.KernelTimer() as timer:
            loss = module(**mb, dropout_seed=seed)
            if loss.requires_grad:  # (a minibatch without a single head row: no parameter reaches the loss)
                loss.backward()
            ops.join_side_stream()
            torch.cuda.synchronize()
            kinds = timer.summary()
        winners = [w.cpu().numpy().astype(np.int64) for w in ops.WINNER_SINK] if sink else None
    finally:
        ops.set_live_backward(prev)
        ops.WINNER_SINK = None
    grads = {k: v.clone() for k, v in Hh.module_grads(module).items()} if loss.requires_grad else None
    return float(loss.detach()), grads, winners, kinds


def _oracle_with_routing(cfg, params, mb_np, seed, winners):
    """the fp64 oracle differentiating the function the device differentiated: its routing injected (tests/test_hip_parity.py)"""
    E = int(mb_np["graph_data"]["msg_src"].shape[0])
    forced = [np.where(w < 0, E, w) for w in winners]
    return O.forward_backward({k: v.double() for k, v in params.items()}, mb_np, cfg, seed=seed, force_arg=forced)


def _worst(grads, ref):
    """largest error of any parameter gradient relative to that gradient's largest entry, and the per-parameter figures"""
    per = {}
    for k, g_ref in ref.items():
        per[k] = (Hh.maxdiff(grads[k], g_ref), float(g_ref.abs().max()))
    return max(d / max(s, 1e-30) for d, s in per.values() if s > 0), per


@pytest.mark.parametrize("case", list(CASES))
def test_live_and_full_backward_against_the_fp64_oracle(ops, case):
    """Loss and every parameter gradient, switch on and switch off, against the fp64 oracle: both inside the 1e-4 parity bound,
    and the live path's largest error no larger than twice the full path's at the same input (twice: the order of the fp32
    atomics moves the last bits between any two runs).  The launch counts say which path ran: one compact copy of the routing
    masks per live layer with live messages, none with the switch off."""
    assert ops.msg_gemm_mode() == "f16x3"
    make, kw = CASES[case]
    kw = dict(kw)
    seed = kw.pop("seed", None)
    mb_np = _collate(make())
    live = _live_rows(mb_np)
    cfg = O.OracleConfig(hidden=H, num_layers=LAYERS, num_edge_types=T, vocab_size=300, **kw)
    params = O.init_params(cfg, seed=0)
    module = Hh.build_module_like(cfg, params)
    loss_off, g_off, winners, k_off = _run(ops, module, mb_np, seed, False, sink=True)
    loss_on, g_on, _, k_on = _run(ops, module, mb_np, seed, True)
    want_launches = sum(1 for (_, _, ex, _) in live[:LAYERS] if ex > 0)
    got_on = k_on.get("winbits_gather_live", {"launches": 0})["launches"]
    assert "winbits_gather_live" not in k_off and got_on == want_launches, (k_off.keys(), got_on, live)
    if case == "no_head_rows":
        # the heads read nothing and the loss is a constant no parameter reaches (the oracle has no form for a minibatch without
        # candidates either): what is left to pin is that the forward pass does not mind the missing live arrays
        assert want_launches == 0 and g_off is None and g_on is None and "node_update_bwd" not in k_on
        print(f"{case}: loss off {loss_off:.7f} on {loss_on:.7f}")
        assert loss_on == loss_off and math.isfinite(loss_on)
        return
    out, ref = _oracle_with_routing(cfg, params, mb_np, seed, winners)
    if case == "every_node_a_head_row":
        assert want_launches == 0                                          # nothing to leave out: the full backward runs
        assert k_on["node_update_bwd"]["launches"] == k_off["node_update_bwd"]["launches"] == LAYERS
    else:
        assert want_launches >= 1
    if case == "second_layer_above_64_nodes":
        assert live[0][0] < 64 and live[1][0] > 64 and live[1][0] % 64 != 0, live
    if case == "live_hub_and_runs":
        gd = mb_np["graph_data"]
        assert np.diff(gd["tgt_ptr"]).max() >= 60 and gd["num_hub_nodes"] >= 1 and live[0][3] < live[0][2], live
    if want_launches:
        assert any((ex + rx) % 128 != 0 for (_, _, ex, rx) in live)
    w_off, per_off = _worst(g_off, ref)
    w_on, per_on = _worst(g_on, ref)
    report = "\n".join(f"  {k}: off {per_off[k][0]:.3e} on {per_on[k][0]:.3e} largest entry {per_off[k][1]:.3e}" for k in ref)
    print(f"{case}: live layers {live}; loss off {loss_off:.7f} on {loss_on:.7f} oracle {float(out['loss'].detach()):.7f}; "
          f"worst relative gradient error off {w_off:.3e} on {w_on:.3e}\n{report}")
    ref_loss = float(out["loss"].detach())
    assert abs(loss_off - ref_loss) < TOL and abs(loss_on - ref_loss) < TOL
    assert loss_on == loss_off                                              # forward is the same code
    for name, per in (("off", per_off), ("on", per_on)):
        for k, (d, scale) in per.items():
            assert d <= TOL * scale + 1e-6, (name, k, d, scale)
    assert w_on <= 2.0 * w_off, (w_on, w_off, report)


def test_a_second_consumer_of_the_full_output_gets_no_gradient(ops):
    """The contract of the live mode: the gradient enters the encoder through head_node_representations only, and the full output
    is handed out detached -- a second consumer gets no gradient rather than a silently truncated one.  Without head_gather_idx
    or with the switch off the full output stays attached and the full backward runs (launch counts)."""
    from buglab.data.collate import to_device

    mb_np = _collate(_base(seed=0, n_var=0, n_swap=0))
    cfg = O.OracleConfig(hidden=H, num_layers=LAYERS, num_edge_types=T, vocab_size=300)
    module = Hh.build_module_like(cfg, O.init_params(cfg, seed=0))
    module.train(True)
    mb = to_device(mb_np, "cuda")
    gd = mb["graph_data"]

    def step(graph_data):
        module.zero_grad(set_to_none=True)
        with ops.KernelTimer() as timer:
            out = module._compute_gnn_output(graph_data, None)
            full, head = out.output_node_representations, out.head_node_representations
            if head is not None:
                (head.sum() + (full.sum() if full.requires_grad else 0.0)).backward()
            else:
                full.sum().backward()
            ops.join_side_stream()
            torch.cuda.synchronize()
            return full.requires_grad, timer.summary().get("winbits_gather_live", {"launches": 0})["launches"]

    prev = ops.set_live_backward(True)
    try:
        attached, launches = step(gd)
        assert not attached and launches >= 1
        attached, launches = step({k: v for k, v in gd.items() if k not in ("head_gather_idx", "head_local_idx")})
        assert attached and launches == 0
        ops.set_live_backward(False)
        attached, launches = step(gd)
        assert attached and launches == 0
    finally:
        ops.set_live_backward(prev)


def test_all_layer_outputs_keep_the_full_backward(ops):
    mb_np = _collate(_base(seed=0, n_var=0, n_swap=0))
    cfg = O.OracleConfig(hidden=H, num_layers=LAYERS, num_edge_types=T, vocab_size=300, use_all_gnn_layer_outputs=True)
    from buglab.models.gnn import GnnBugLabModule

    base = Hh.build_module_like(cfg, None)
    module = GnnBugLabModule(base._gnn, cfg.rewrite_vocab_size, use_all_gnn_layer_outputs=True).cuda()
    _, _, _, kinds = _run(ops, module, mb_np, None, True)
    assert "winbits_gather_live" not in kinds and kinds["node_update_bwd"]["launches"] == LAYERS


# ---- the new entry points: strided operands, guard bands -------------------------------------------------------------------
GUARD = 3  # rows of NaN / poison in front of and behind every output


def _guarded(rows, cols, ld=None, dtype=torch.float32, fill=float("nan")):
    ld = cols if ld is None else ld
    buf = torch.full((rows + 2 * GUARD, ld), fill, dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + rows]


def _guards_untouched(buf, rows, cols, fill_is_nan=True):
    body = buf[GUARD:GUARD + rows]
    edge = torch.cat([buf[:GUARD].reshape(-1), buf[GUARD + rows:].reshape(-1), body[:, cols:].reshape(-1)])
    return bool(torch.isnan(edge).all()) if fill_is_nan else bool((edge == -1).all())


@pytest.mark.parametrize("words,ld_in,ld_out", [(4, 4, 4), (8, 12, 8), (3, 5, 7)])
def test_gather_of_the_routing_masks(ops, words, ld_in, ld_out):
    rng = np.random.default_rng(words)
    E, n = 333, 77
    bits_np = rng.integers(0, 2 ** 32, (E, ld_in), dtype=np.uint64).astype(np.uint32)
    rows = np.sort(rng.choice(E, n, replace=False)).astype(I32)
    bits = _dev(bits_np.view(np.int32))
    buf, out = _guarded(n, words, ld_out, dtype=torch.int32, fill=-1)
    ops._check(ops.load_library().bl_winbits_gather(bits.data_ptr(), ld_in, E, _dev(rows).data_ptr(), n, words, out.data_ptr(), ld_out, _stream()),
               "bl_winbits_gather")
    torch.cuda.synchronize()
    assert np.array_equal(out[:, :words].cpu().numpy().view(np.uint32), bits_np[rows, :words])
    assert _guards_untouched(buf, n, words, fill_is_nan=False)
    assert ops.load_library().bl_winbits_gather(bits.data_ptr(), ld_in, E, None, n, words, out.data_ptr(), ld_out, _stream()) != 0


@pytest.mark.parametrize("Dm,Dout,nrows", [(128, 128, 10), (256, 128, 64), (256, 128, 139), (128, 128, 1)])
@pytest.mark.parametrize("p_drop", [0.0, 0.25])
def test_node_update_backward_over_a_row_list(ops, Dm, Dout, nrows, p_drop):
    """bl_node_update_bwd_rows against bl_node_update_bwd on the same tensors with g_out zero outside the rows: packed g_z and gq of
    the listed rows equal the full call's rows bit for bit (the same arithmetic on the same inputs, the row's own dropout
    counter); the column sums (bias, gamma, beta) agree up to the order of their fp32 atomics.  Partial last tile (139 = 2 x 64 +
    11), fewer than 64 rows, one row; guard rows around every per-row output."""
    N = 300
    torch.manual_seed(Dm + nrows)
    rows_np = np.sort(np.random.default_rng(nrows).choice(N, nrows, replace=False)).astype(I32)
    rows = _dev(rows_np)
    h_out = torch.tanh(torch.randn(N, Dout)).cuda()
    g_full = torch.zeros(N, Dout)
    g_full[torch.from_numpy(rows_np.astype(np.int64))] = torch.randn(nrows, Dout)
    g_full = g_full.cuda()
    agg, dact = torch.randn(N, Dm).cuda(), torch.rand(N, Dm).cuda()
    mean, rstd = agg.mean(1).contiguous(), (1.0 / (agg.var(1, unbiased=False) + 1e-5).sqrt()).contiguous()
    ln_g = (1.0 + 0.1 * torch.randn(Dm)).cuda()
    Wd = (torch.randn(Dm, Dout) / math.sqrt(Dm)).cuda()
    wd_nk = ops.pack_weights_x6(Wd.unsqueeze(0), False)
    drop = ops.Dropout(p_drop, 1234, 5)
    lib = ops.load_library()

    def outputs(n):
        gz = _guarded(n, 3 * Dout, dtype=torch.int16, fill=-1)
        gq = _guarded(n, Dm)
        gqp = _guarded(n, 3 * Dm, dtype=torch.int16, fill=-1)
        small = [torch.zeros(Dout, device="cuda"), torch.zeros(Dm, device="cuda"), torch.zeros(Dm, device="cuda")]
        return gz, gq, gqp, small

    gz_f, gq_f, gqp_f, s_f = outputs(N)
    ops._check(lib.bl_node_update_bwd(g_full.data_ptr(), h_out.data_ptr(), N, Dout, drop.c(), wd_nk.data_ptr(), agg.data_ptr(), mean.data_ptr(),
                                      rstd.data_ptr(), ln_g.data_ptr(), dact.data_ptr(), Dm, gz_f[1].data_ptr(), s_f[0].data_ptr(),
                                      gq_f[1].data_ptr(), gqp_f[1].data_ptr(), s_f[1].data_ptr(), s_f[2].data_ptr(), _stream()), "bl_node_update_bwd")
    gz_r, gq_r, gqp_r, s_r = outputs(nrows)
    ops._check(lib.bl_node_update_bwd_rows(g_full.data_ptr(), h_out.data_ptr(), rows.data_ptr(), nrows, Dout, drop.c(), wd_nk.data_ptr(),
                                           agg.data_ptr(), mean.data_ptr(), rstd.data_ptr(), ln_g.data_ptr(), dact.data_ptr(), Dm,
                                           gz_r[1].data_ptr(), s_r[0].data_ptr(), gq_r[1].data_ptr(), gqp_r[1].data_ptr(), s_r[1].data_ptr(),
                                           s_r[2].data_ptr(), _stream()), "bl_node_update_bwd_rows")
    torch.cuda.synchronize()
    idx = rows.long()
    assert torch.equal(gz_r[1], gz_f[1][idx]) and torch.equal(gq_r[1], gq_f[1][idx]) and torch.equal(gqp_r[1], gqp_f[1][idx])
    dead = torch.ones(N, dtype=torch.bool, device="cuda")
    dead[idx] = False
    assert bool((gq_f[1][dead] == 0).all())                                 # what the live path rests on: zero rows in, zero rows out
    assert _guards_untouched(gz_r[0], nrows, 3 * Dout, False) and _guards_untouched(gq_r[0], nrows, Dm) and _guards_untouched(gqp_r[0], nrows, 3 * Dm, False)
    for a, b, terms in zip(s_r, s_f, (nrows, nrows, nrows)):
        # column sums of at most `terms` non-zero entries each, in any order: |difference| <= 2 x terms x 2^-24 x sum of |entries|,
        # and the sum of |entries| of a column is at most terms x the largest entry
        scale = float(b.abs().max()) + 1.0
        assert float((a - b).abs().max()) <= 2.0 * terms * 2.0 ** -24 * terms * scale
    assert lib.bl_node_update_bwd_rows(g_full.data_ptr(), h_out.data_ptr(), None, nrows, Dout, drop.c(), wd_nk.data_ptr(), agg.data_ptr(),
                                       mean.data_ptr(), rstd.data_ptr(), ln_g.data_ptr(), dact.data_ptr(), Dm, gz_r[1].data_ptr(), s_r[0].data_ptr(),
                                       gq_r[1].data_ptr(), gqp_r[1].data_ptr(), s_r[1].data_ptr(), s_r[2].data_ptr(), _stream()) != 0


@pytest.mark.parametrize("split,ld_extra", [(None, 0), (96, 0), (128, 32)])
def test_segmented_sums_into_listed_rows(ops, split, ld_extra):
    """bl_mp_scatter_grad_rows over the reduced CSRs of a live layer as the collator makes them: the rows of the receiving nodes
    equal an fp64 index_add within the summation bound of tests/test_run_rows_gpu.py, every other row and the guard rows stay as
    they were; strided outputs."""
    from buglab.data import collate as C

    mb_np = _collate(_case_hub())
    gd = mb_np["graph_data"]
    N, Din = gd["token_ids"].shape[0], 256
    row = gd["live_layout"][1].astype(np.int64)                           # the second live layer: sources of its own
    col = {k: i for i, k in enumerate(C.LIVE_LAYOUT_COLUMNS)}
    nn, nr, ex, rx = (int(x) for x in row[:4])
    piece = lambda k, n: gd["live_arrays"][row[col[k]]:row[col[k]] + n]
    recv, src_ptr, src_msgs = piece("recv", nr), piece("src_ptr", nr + 1), piece("src_msgs", ex)
    rc_ptr, rc_rows, rows_src = piece("run_csr_ptr", nr + 1), piece("run_csr_rows", rx), piece("rows_src", ex + rx)
    assert ex > 0 and rx > 0 and nr > nn
    torch.manual_seed(1)
    g_a = torch.randn(ex + rx, Din)
    to_node = torch.from_numpy(rows_src.astype(np.int64))                   # a message's row goes to its source, a run's to its target
    ref = torch.zeros(N, Din, dtype=torch.float64).index_add_(0, to_node, g_a.double())
    mag = torch.zeros(N, Din, dtype=torch.float64).index_add_(0, to_node, g_a.double().abs())
    deg = torch.zeros(N, dtype=torch.float64).index_add_(0, to_node, torch.ones(ex + rx, dtype=torch.float64))
    w_lo = Din if split is None else split
    lo_buf, lo = _guarded(N, w_lo, w_lo + ld_extra)
    hi_buf, hi = (None, None) if split is None else _guarded(N, Din - split, Din - split + ld_extra)
    lo[:, :w_lo] = 0.0
    if hi is not None:
        hi[:, :Din - split] = 0.0
    d_ga = _dev(g_a)
    d = [_dev(a) for a in (src_ptr, src_msgs, rc_ptr, rc_rows, recv)]
    ops._check(ops.load_library().bl_mp_scatter_grad_rows(d_ga.data_ptr(), Din, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                                                          d[4].data_ptr(), nr, Din, w_lo, lo.data_ptr(), lo.stride(0),
                                                          hi.data_ptr() if hi is not None else None, hi.stride(0) if hi is not None else 0,
                                                          _stream()), "bl_mp_scatter_grad_rows")
    torch.cuda.synchronize()
    got = (lo[:, :w_lo] if hi is None else torch.cat([lo[:, :w_lo], hi[:, :Din - split]], 1)).cpu().double()
    err = (got - ref).abs()
    assert bool((err <= deg[:, None] * 2.0 ** -24 * mag).all())
    outside = np.setdiff1d(np.arange(N), recv)
    assert bool((got[outside] == 0).all()) and float(ref[outside].abs().max()) == 0.0
    assert _guards_untouched(lo_buf, N, w_lo) and (hi_buf is None or _guards_untouched(hi_buf, N, Din - split))
