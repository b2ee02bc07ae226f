"""GPU: the loss assembly (csrc/bl_loss.hip) and the small head kernels it replaces (csrc/bl_head_ops.hip, csrc/bl_heads_fused.hip)
called on their own, against fp64, at the shapes where they change path: tests/loss_cases.py holds the cases and the restatement.
Every bound is 4 x the error of the same expression evaluated in float32 on the CPU + 1e-6 (tests/loss_cases.py: abs_bound /
rel_bound): the kernels sum in wave-butterfly order where torch sums sequentially, and the device's expf / logf are good to about
2 ulp where the host's round correctly.  Each test prints the kernel's error next to err32."""
import ctypes
import math
from ctypes import c_int32, c_void_p

import numpy as np
import pytest
import torch

from tests import loss_cases as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from buglab.models import hip_ops

    hip_ops.load_library()
    return hip_ops


def _dev(a, dtype=None):
    t = torch.tensor(np.asarray(a)) if not isinstance(a, torch.Tensor) else a
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda().contiguous()


def _nan(n):
    return torch.full((int(n),), math.nan, dtype=torch.float32, device="cuda")


def _check_abs(table, what, got, r32, r64):
    err32, bound = L.abs_bound(r32, r64)
    err = L.max_error(got.cpu(), r64)
    table.append((what, err, err32, bound))
    assert err <= bound, f"{what}: kernel error {err:.3e} > bound {bound:.3e} (err32 {err32:.3e})"


def _check_rel(table, what, got, r32, r64):
    err32, bound, scale = L.rel_bound(r32, r64)
    err = L.max_error(got.cpu(), r64)
    table.append((what, err / scale if scale else err, err32, bound / scale if scale else bound))
    assert err <= bound, f"{what}: kernel error {err:.3e} > bound {bound:.3e} (err32 {err32:.3e} of scale {scale:.3e})"


def _print_table(title, table):
    worst = {}
    for what, err, err32, bound in table:
        w = worst.get(what)
        if w is None or err / max(bound, 1e-300) > w[0] / max(w[2], 1e-300):
            worst[what] = (err, err32, bound)
    print(f"\n{title}: " + "  ".join(f"{k} err {e:.2e} err32 {e32:.2e} bound {b:.2e}" for k, (e, e32, b) in worst.items()))


# ------------------------------------------------------------------------------------------------ (a), (b): the loss assembly
class _DeviceCase:
    def __init__(self, ops, case):
        self.case = case
        self.scores, self.logits = _dev(case.loc_scores), _dev(case.repair_logits)
        self.ix = ops.BugLossIndex(_dev(case.loc_group_ptr), _dev(case.loc_group_items), _dev(case.candidate_ptr), _dev(case.has_bug),
                                   _dev(case.correct_candidate_idxs), _dev(case.repair_group_ptr), _dev(case.repair_group_items),
                                   tuple(_dev(g) for g in case.logit_group), tuple(_dev(t) for t in case.target), case.G)


def _run_abi(ops, dc, w_buggy, abstain, g_loss):
    """bl_bug_loss_fwd + _bwd through the C ABI, every output pre-filled with NaN -> the outputs, on the device"""
    case, lib = dc.case, ops.load_library()
    d = ops._bug_loss_desc(dc.scores, dc.logits, case.sizes, dc.ix, w_buggy, abstain)
    for k in case.null_fixers:
        d.logit_group[k], d.target[k] = None, None
    C, B, R, G = case.C, case.B, case.R, case.G
    loc_lp, rep_lp, gmax, loss, stats = _nan(C + B), _nan(max(1, R)), _nan(max(1, G)), _nan(1), _nan(16)
    ops._check(lib.bl_bug_loss_fwd(ctypes.byref(d), loc_lp.data_ptr(), rep_lp.data_ptr(), gmax.data_ptr(), loss.data_ptr(), stats.data_ptr(),
                                   ops._stream()), "bl_bug_loss_fwd")
    scratch, g_scores, g_logits = _nan(C + B + R + 1), _nan(C), _nan(max(1, R))
    g = torch.tensor([g_loss], dtype=torch.float32, device="cuda")
    ops._check(lib.bl_bug_loss_bwd(ctypes.byref(d), loc_lp.data_ptr(), rep_lp.data_ptr(), g.data_ptr(), scratch.data_ptr(),
                                   g_scores.data_ptr(), g_logits.data_ptr(), ops._stream()), "bl_bug_loss_bwd")
    torch.cuda.synchronize()
    return loc_lp, rep_lp[:R], gmax[:G], loss, stats, g_scores, g_logits[:R]


@pytest.mark.parametrize("name", L.CASE_NAMES)
def test_bug_loss_kernels_match_fp64(ops, name):
    """(a) bl_bug_loss_fwd / _bwd on their own against the fp64 restatement, over w_buggy x abstain x g_loss; every entry the
    header promises is written (the outputs start as NaN); a second run is bit-identical.  err32 of a quantity is taken over all
    runs of the case (loss_cases.case_err32).
    (b) hip_ops.bug_loss through autograd gives the same loss, stats and gradients bit for bit."""
    case = L.get_case(name)
    dc = _DeviceCase(ops, case)
    empty = torch.tensor(np.diff(case.repair_group_ptr) == 0)
    table = []
    for w_buggy, abstain, g_loss in L.GRID:
        what = f"{name} w={w_buggy} a={abstain} g={g_loss}"
        r64 = L.get_ref(name, w_buggy, abstain, g_loss)
        out = _run_abi(ops, dc, w_buggy, abstain, g_loss)
        loc_lp, rep_lp, gmax, loss, stats, g_scores, g_logits = out
        for t, field in zip(out, L.LossRef._fields):
            assert not bool(torch.isnan(t).any()), f"{what}: {field} has entries nobody wrote"
        def check(what_q, field, got_q, ref_q):
            err32, bound = L.bound_of(name, field, ref_q)
            err = L.max_error(got_q.cpu(), ref_q)
            scale = float(ref_q.abs().max()) if field in L.REL_FIELDS and ref_q.numel() else 0.0
            table.append((what_q, err / scale if scale else err, err32, bound / scale if scale else bound))
            assert err <= bound, f"{what}: {what_q}: kernel error {err:.3e} > bound {bound:.3e} (err32 {err32:.3e})"

        check("loc_logprobs", "loc_logprobs", loc_lp, r64.loc_logprobs)
        check("repair_logprobs", "repair_logprobs", rep_lp, r64.repair_logprobs)
        check("group_max", "group_max", gmax, r64.group_max)
        assert bool((gmax.cpu()[empty] == -math.inf).all()) and bool(torch.isfinite(gmax.cpu()[~empty]).all()), what
        check("loss", "loss", loss, r64.loss.reshape(1))
        got = dict(zip(L.STATS, stats.cpu().tolist()))
        want = dict(zip(L.STATS, r64.stats.tolist()))
        for k in L.COUNT_STATS:
            assert got[k] == want[k], (what, k, got[k], want[k])
        for k in L.SUM_STATS:
            i = L.STATS.index(k)
            check(k, "stats", stats[i:i + 1], r64.stats[i:i + 1])
        assert got["loss"] == float(loss), what
        check("g_loc_scores", "g_loc_scores", g_scores, r64.g_loc_scores)
        check("g_repair_logits", "g_repair_logits", g_logits, r64.g_repair_logits)
        again = _run_abi(ops, dc, w_buggy, abstain, g_loss)
        for t, u, field in zip(out, again, L.LossRef._fields):
            assert torch.equal(t, u), f"{what}: {field} differs between two runs"
        # (b) the autograd wrapper: the same numbers
        xs, xl = dc.scores.clone().requires_grad_(True), dc.logits.clone().requires_grad_(True)
        loss_b, stats_b = ops.bug_loss(xs, xl, case.sizes, dc.ix, w_buggy, abstain)
        loss_b.backward(torch.tensor(g_loss, dtype=torch.float32, device="cuda"))
        torch.cuda.synchronize()
        assert torch.equal(loss_b.detach().reshape(1), loss) and torch.equal(stats_b, stats), what
        assert torch.equal(xs.grad, g_scores) and torch.equal(xl.grad if xl.grad is not None else torch.zeros_like(xl), g_logits), what
    _print_table(name, table)


# ------------------------------------------------------------------------------------------------ (c) the op-by-op kernels
def _segment_inputs(case, which):
    if which == "loc":
        x = np.concatenate([case.loc_scores, np.ones(case.B, np.float32)])
        return x, case.loc_index, case.loc_group_ptr, case.loc_group_items, case.B
    return case.repair_logits, case.repair_index, case.repair_group_ptr, case.repair_group_items, case.G


@pytest.mark.parametrize("layout", ["csr", "permuted", "contiguous"])
@pytest.mark.parametrize("which", ["loc", "repair"])
@pytest.mark.parametrize("name", ["boundary", "many_graphs", "wide_range"])
def test_segment_log_softmax_kernels_match_fp64(ops, name, which, layout):
    """bl_segment_log_softmax_fwd / _bwd over the cases' segments (1 .. 201 items, empty ones among the repair groups) as the
    collator lays them out, with the values moved by a permutation that seg_items undoes, and with seg_items = NULL over
    contiguous segments.  Five entries behind the last item belong to no segment: nobody may write them."""
    x, index, ptr, items, nseg = _segment_inputs(L.get_case(name), which)
    n, tail = x.shape[0], 5
    rng = np.random.default_rng(11)
    if layout == "permuted":  # entry i moves to place perm[i]
        perm = rng.permutation(n)
    elif layout == "contiguous":  # entry items[j] moves to place j: every segment is a run
        perm = np.empty(n, np.int64)
        perm[items] = np.arange(n)
    else:
        perm = np.arange(n)
    xp, idxp = np.empty(n, np.float32), np.empty(n, np.int64)
    xp[perm], idxp[perm] = x, index
    seg_items = None if layout == "contiguous" else _dev(perm[items].astype(np.int32))
    if layout == "contiguous":
        assert np.array_equal(perm[items], np.arange(n))
    gy = rng.standard_normal(n).astype(np.float32)

    def ref(dtype):
        xr = torch.tensor(xp, dtype=dtype).requires_grad_(True)
        y = L.segment_log_softmax_ref(xr, torch.tensor(idxp), nseg)
        (g,) = torch.autograd.grad(y, xr, torch.tensor(gy, dtype=dtype))
        return y.detach(), g

    (y64, g64), (y32, g32) = ref(torch.float64), ref(torch.float32)
    lib, ptr_d = ops.load_library(), _dev(ptr)
    xd = _dev(np.concatenate([xp, np.full(tail, 3.0, np.float32)]))
    y = torch.full((n + tail,), 7.0, dtype=torch.float32, device="cuda")
    ops._check(lib.bl_segment_log_softmax_fwd(xd.data_ptr(), ptr_d.data_ptr(), ops._p(seg_items), nseg, 1e-12, y.data_ptr(), ops._stream()),
               "bl_segment_log_softmax_fwd")
    gyd = _dev(np.concatenate([gy, np.ones(tail, np.float32)]))
    gx = torch.full((n + tail,), 7.0, dtype=torch.float32, device="cuda")
    ops._check(lib.bl_segment_log_softmax_bwd(gyd.data_ptr(), y.data_ptr(), ptr_d.data_ptr(), ops._p(seg_items), nseg, gx.data_ptr(),
                                              ops._stream()), "bl_segment_log_softmax_bwd")
    torch.cuda.synchronize()
    table = []
    _check_abs(table, "y", y[:n], y32, y64)
    _check_rel(table, "g_x", gx[:n], g32, g64)
    assert bool((y[n:] == 7.0).all()) and bool((gx[n:] == 7.0).all())
    _print_table(f"segment_log_softmax {name} {which} {layout}", table)


@pytest.mark.parametrize("with_b", [True, False])
@pytest.mark.parametrize("H", [4, 60, 64, 100, 512, 1000])
@pytest.mark.parametrize("R", [1, 77, 1025])
def test_rowdot_kernels_match_fp64(ops, R, H, with_b):
    """bl_rowdot_fwd / _bwd: y = x . w (+ b) with a row stride above H; g_x = g_y w^T into a matrix with guard columns; g_w and
    g_b are added to what the buffers hold (0.5).  In deterministic mode a second run gives the same bits."""
    gen = torch.Generator().manual_seed(1000 * R + H)
    xs = torch.randn(R, H + 3, generator=gen)
    x, w, b, gy = xs[:, :H], torch.randn(H, generator=gen), torch.randn(1, generator=gen), torch.randn(R, generator=gen)

    def ref(dtype):
        xr, wr, br = (t.to(dtype).clone().requires_grad_(True) for t in (x, w, b))
        y = xr @ wr + (br if with_b else 0.0)
        y.backward(gy.to(dtype))
        return y.detach(), xr.grad, wr.grad + 0.5, (br.grad if with_b else torch.zeros(1, dtype=dtype)) + 0.5

    r64, r32 = ref(torch.float64), ref(torch.float32)
    lib = ops.load_library()
    xd, wd, bd, gyd = _dev(xs), _dev(w), _dev(b), _dev(gy)
    table, first = [], None
    was = ops.deterministic()
    try:
        for mode in (False, True, True):
            ops.set_deterministic(mode)
            y = _nan(R)
            ops._check(lib.bl_rowdot_fwd(xd.data_ptr(), H + 3, wd.data_ptr(), bd.data_ptr() if with_b else None, R, H, y.data_ptr(), ops._stream()),
                       "bl_rowdot_fwd")
            gx = torch.full((R, H + 2), math.nan, dtype=torch.float32, device="cuda")
            gw, gb = torch.full((H,), 0.5, device="cuda"), torch.full((1,), 0.5, device="cuda")
            ops._check(lib.bl_rowdot_bwd(gyd.data_ptr(), xd.data_ptr(), H + 3, wd.data_ptr(), R, H, gx.data_ptr(), H + 2, gw.data_ptr(),
                                         gb.data_ptr() if with_b else None, ops._stream()), "bl_rowdot_bwd")
            torch.cuda.synchronize()
            _check_abs(table, "y", y, r32[0], r64[0])
            _check_rel(table, "g_x", gx[:, :H], r32[1], r64[1])
            _check_rel(table, "g_w", gw, r32[2], r64[2])
            _check_rel(table, "g_b", gb, r32[3], r64[3])
            assert bool(torch.isnan(gx[:, H:]).all()), "guard columns of g_x were written"
            if mode and first is not None:
                assert all(torch.equal(a, c) for a, c in zip(first, (y, gx[:, :H], gw, gb))), "deterministic mode: two runs differ"
            elif mode:
                first = (y, gx[:, :H].clone(), gw, gb)
    finally:
        ops.set_deterministic(was)
    _print_table(f"rowdot R={R} H={H} b={with_b}", table)


@pytest.mark.parametrize("index", ["one_row", "random"])
@pytest.mark.parametrize("width,col_off", [(5, 3), (64, 0)])
def test_scatter_add_rows_matches_fp64_and_the_ordered_walk(ops, width, col_off, index):
    """bl_scatter_add_rows: out[idx[r], :] += src[r, col_off : col_off + width] into a pre-filled output whose rows are longer than
    `width`; 1000 rows aimed at one output row, and a random index that leaves a row alone.  Deterministic mode equals, bit for
    bit, float32 additions of the rows in ascending order (the walk of scatter_add_rows_serial_kernel)."""
    R, nout, ld_src, ld_out = 1000, 9, col_off + width + 2, width + 3
    rng = np.random.default_rng(width + (7 if index == "random" else 0))
    src = rng.standard_normal((R, ld_src)).astype(np.float32)
    idx = np.full(R, 4, np.int32) if index == "one_row" else rng.choice([0, 1, 2, 3, 5, 6, 7, 8], R).astype(np.int32)  # row 4: untouched
    out0 = rng.standard_normal((nout, ld_out)).astype(np.float32)
    part = src[:, col_off:col_off + width]

    def ref(dtype):
        o = torch.tensor(out0[:, :width], dtype=dtype).clone()
        return o.index_add_(0, torch.tensor(idx).long(), torch.tensor(part, dtype=dtype))

    r64, r32 = ref(torch.float64), ref(torch.float32)
    walk = out0.copy()
    for r in range(R):
        walk[idx[r], :width] = walk[idx[r], :width] + part[r]
    lib, src_d, idx_d = ops.load_library(), _dev(src), _dev(idx)
    table = []
    was = ops.deterministic()
    try:
        for mode in (False, True):
            ops.set_deterministic(mode)
            out = _dev(out0)
            ops._check(lib.bl_scatter_add_rows(src_d.data_ptr(), ld_src, col_off, width, idx_d.data_ptr(), R, out.data_ptr(), ld_out,
                                               ops._stream()), "bl_scatter_add_rows")
            torch.cuda.synchronize()
            got = out.cpu()
            _check_rel(table, "deterministic" if mode else "atomic", got[:, :width], r32, r64)
            assert torch.equal(got[:, width:], torch.tensor(out0[:, width:])), "columns beyond `width` were written"
            untouched = 4 if index == "random" else 0
            assert torch.equal(got[untouched], torch.tensor(out0[untouched]))
            if mode:
                assert np.array_equal(got.numpy().view(np.uint32), walk.view(np.uint32)), "deterministic mode is not the ascending walk"
    finally:
        ops.set_deterministic(was)
    _print_table(f"scatter_add_rows width={width} {index}", table)


@pytest.mark.parametrize("width", [4, 516])
@pytest.mark.parametrize("R", [1, 300])
def test_gather_rows_copies_exactly_and_leaves_the_guard_columns(ops, R, width):
    rng = np.random.default_rng(R + width)
    N, ld_x, ld_out = 40, width + 4, width + 8
    x = rng.standard_normal((N, ld_x)).astype(np.float32)
    idx = rng.integers(0, N, R).astype(np.int32)
    if R > 1:
        idx[1::3] = idx[0]  # duplicates
    out = torch.full((R, ld_out), -5.0, dtype=torch.float32, device="cuda")
    x_d, idx_d = _dev(x), _dev(idx)
    ops._check(ops.load_library().bl_gather_rows(x_d.data_ptr(), ld_x, idx_d.data_ptr(), R, width, out.data_ptr(), ld_out, ops._stream()),
               "bl_gather_rows")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got[:, :width].view(np.uint32), x[idx.astype(np.int64), :width].view(np.uint32))
    assert (got[:, width:] == -5.0).all()


@pytest.mark.parametrize("H,R,layout,with_b2", [(32, 1, "shared", True), (32, 1000, "shared3", False), (64, 129, "shared3", True),
                                                (64, 1000, "plain_first", True), (128, 129, "shared", False), (128, 1, "shared3", True),
                                                (256, 129, "plain_first", False), (256, 1, "shared", True)])
def test_mlp_score_calls_match_fp64_autograd(ops, H, R, layout, with_b2):
    """bl_gather_concat_mlp_score_fwd / _bwd against fp64 autograd of w2 . relu(cat(x_j[idx_j]) @ W1 + b1) + b2.
    shared: two sources gather from ONE matrix, whose gradient matrix both add to; shared3: the same plus a third source without
    an index and without a gradient; plain_first: the index-free source comes first.  Every gradient buffer arrives holding 0.25:
    the call accumulates.  idx has duplicate rows."""
    gen = torch.Generator().manual_seed(H + 3 * R)
    rng = np.random.default_rng(H * R)
    N = 37
    X, E = torch.randn(N, H, generator=gen), torch.randn(R, H, generator=gen)
    ia, ib = (torch.tensor(rng.integers(0, N, R)) for _ in range(2))
    if R > 2:
        ia[2], ib[1] = ia[0], ia[0]
    srcs = {"shared": [("X", ia), ("X", ib)], "shared3": [("X", ia), ("X", ib), ("E", None)], "plain_first": [("E", None), ("X", ia)]}[layout]
    K = len(srcs) * H
    W1 = torch.randn(K, H, generator=gen) / math.sqrt(K)
    b1, w2, b2, gs = torch.randn(H, generator=gen), torch.randn(H, generator=gen) / math.sqrt(H), torch.randn(1, generator=gen), torch.randn(R, generator=gen)

    def ref(dtype):
        Xr = X.to(dtype).clone().requires_grad_(True)
        P = [t.to(dtype).clone().requires_grad_(True) for t in (W1, b1, w2, b2)]
        a = torch.cat([Xr[i] if m == "X" else E.to(dtype) for m, i in srcs], dim=-1)
        z = a @ P[0] + P[1]
        # (no hidden unit so close to 0 that float32 could switch its relu the other way: a case that drifts fails here)
        assert dtype != torch.float64 or float(z.detach().abs().min()) > 1e-5, float(z.detach().abs().min())
        score = torch.relu(z) @ P[2] + (P[3] if with_b2 else 0.0)
        score.backward(gs.to(dtype))
        gb2 = P[3].grad if with_b2 else torch.zeros(1, dtype=dtype)
        return score.detach(), Xr.grad + 0.25, P[0].grad + 0.25, P[1].grad + 0.25, P[2].grad + 0.25, gb2 + 0.25

    r64, r32 = ref(torch.float64), ref(torch.float32)
    lib = ops.load_library()
    Xd, Ed, iad, ibd = _dev(X), _dev(E), _dev(ia, torch.int32), _dev(ib, torch.int32)
    dsrc = [(Xd if m == "X" else Ed, None if i is None else (iad if i is ia else ibd)) for m, i in srcs]
    rows, K2 = ops._rows(dsrc)
    assert K2 == K
    W1d, b1d, w2d, b2d, gsd = (_dev(t) for t in (W1, b1, w2, b2, gs))
    hidden, score = torch.full((R, H), math.nan, device="cuda"), _nan(R)
    ops._check(lib.bl_gather_concat_mlp_score_fwd(ctypes.byref(rows), W1d.data_ptr(), b1d.data_ptr(), w2d.data_ptr(),
                                                  b2d.data_ptr() if with_b2 else None, R, H, hidden.data_ptr(), score.data_ptr(), ops._stream()),
               "bl_gather_concat_mlp_score_fwd")
    gX = torch.full((N, H), 0.25, device="cuda")
    gW1, gb1, gw2, gb2 = (torch.full(s, 0.25, device="cuda") for s in ((K, H), (H,), (H,), (1,)))
    gx, ld = (c_void_p * 3)(), (c_int32 * 3)()
    for j, (m, _) in enumerate(srcs):
        if m == "X":
            gx[j], ld[j] = gX.data_ptr(), H
    ws = torch.empty((lib.bl_gather_concat_mlp_score_workspace_bytes(R, H, K),), dtype=torch.uint8, device="cuda")
    ops._check(lib.bl_gather_concat_mlp_score_bwd(ctypes.byref(rows), W1d.data_ptr(), w2d.data_ptr(), hidden.data_ptr(), gsd.data_ptr(), R, H,
                                                  ws.data_ptr(), gW1.data_ptr(), gb1.data_ptr(), gw2.data_ptr(),
                                                  gb2.data_ptr() if with_b2 else None, gx, ld, ops._stream()), "bl_gather_concat_mlp_score_bwd")
    torch.cuda.synchronize()
    table = []
    _check_abs(table, "score", score, r32[0], r64[0])
    for what, got, i in (("g_x", gX, 1), ("g_W1", gW1, 2), ("g_b1", gb1, 3), ("g_w2", gw2, 4), ("g_b2", gb2, 5)):
        _check_rel(table, what, got, r32[i], r64[i])
    _print_table(f"mlp_score H={H} R={R} {layout} b2={with_b2}", table)
