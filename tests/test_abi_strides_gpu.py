"""GPU: the C ABI's strided operands.  include/buglab_hip.h gives almost every entry point explicit leading dimensions and
promises only 16-byte aligned pointers and ld / widths in multiples of 4 floats; the Python wrappers pass contiguous tensors
from the allocator (ld == width, 256-byte aligned), so this file calls the entry points directly (ops.load_library().bl_*) with

  * every matrix inside a guard-banded allocation (tests/guard_bands.py): base pointer 16- but not 32-byte aligned, ld drawn
    from {width + 4, width + 36}, NaN patterns in the padding columns and in 256 rows before and after;
  * the payload compared with an fp64 reference built from the payloads alone, at the bound the contiguous test of the same
    entry point in tests/test_hip_kernels.py asserts (cited at each check: a leading dimension changes addresses, not
    arithmetic);
  * where the kernel has no atomics, bit equality with the same call on ld == width copies;
  * every output finite (a padding NaN that reaches a result shows here) and every buffer's guard untouched.

Accumulating outputs (weight gradients, bias gradients, the scatter-add target) start from 0.5, so "adds into" is checked.
Index arrays are one-dimensional, have no leading dimension and are passed as allocated.

Covered: bl_gemm_rows, bl_gemm_rows_routed, bl_gemm_wgrad, bl_gemm_wgrad_routed, bl_pack_bf16x3, bl_pack_bf16x3_cols,
bl_pack_f16x2, bl_gemm_rows_x6, bl_gemm_rows_x6_epi, bl_gemm_rows_x6w, bl_gemm_rows_h3, bl_gemm_wgrad_x6,
bl_gemm_wgrad_routed_x6, bl_gemm_wgrad_h3, bl_segment_max_fwd / _bwd, bl_act_bwd / _packed, bl_mp_scatter_grad / _split,
bl_embed_subtoken_pool_fwd / _bwd / _bwd_sorted, bl_gru_cell_fwd / _bwd, bl_routed_dgrad_vec / _nodes / _nodes_rows,
bl_gather_rows, bl_scatter_add_rows, bl_rowdot_fwd / _bwd, bl_localization_scores_fwd / _bwd, bl_gru_scan_fwd / _bwd, the
bl_mp_layer_fwd / _bwd call (`saved` and the workspaces of the last three sized by the library's own size functions and
guarded); group_w on the eleven grouped GEMMs; the "any width" entry points at an odd width.

A bound marked DERIVED is not taken from an existing test: the comment next to it gives the reasoning.

TODO: the `_v` head-view kernels and bl_great_layer_* (their strides are exercised by the one-call-layer parity tests; guarding
them needs the layer's internal layout)."""
import ctypes
import itertools
import math

import numpy as np
import pytest
import torch

from tests.guard_bands import PATTERN_16, guarded

pytestmark = pytest.mark.gpu

SIZES = [130, 0, 1, 257, 64]  # the grouped GEMM tests' list: an empty group, a one-row group, partial tiles


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from buglab.models import hip_ops

    hip_ops.load_library()
    return hip_ops


def _dev(a, dtype=None):
    t = torch.as_tensor(a)
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda().contiguous()


def _ptr(sizes):
    p = np.zeros(len(sizes) + 1, dtype=np.int32)
    p[1:] = np.cumsum(sizes)
    return p


class Bufs:
    """The guarded buffers of one call.  first_pad 4 or 36: the buffers' leading dimensions are width + first_pad, width + the other
    one, and so on in turn (each drawn from {width + 4, width + 36}), bases 16- but not 32-byte aligned (lead = 4).
    first_pad 1 (the "any width" entry points only): ld = width + 2 with nothing rounded to 4 and lead = 1, so that rows and base are
    4-byte aligned and no more.
    first_pad 0: the contiguous twin of a case -- ld == width everywhere and lead = 0, so that every base pointer is aligned as the
    allocator hands it out (the guard rows are whole multiples of 4 KiB); still guarded."""

    def __init__(self, first_pad):
        self.first_pad, self.all, self.outs, self.keep = first_pad, [], [], []
        self.lead = {0: 0, 1: 1}.get(first_pad, 4)
        self._pads = itertools.cycle((4, 36) if first_pad == 4 else (36, 4))

    def _ld(self, width, ld, fixed):
        """ld of the next buffer: the caller's own (two operands that share one in the ABI), the width (`fixed`: the ABI gives this
        operand no leading dimension), or the width rounded up to 4 plus the next pad"""
        if ld is not None:
            return ld
        if fixed:
            return width
        if self.first_pad == 1:
            return width + 2
        return (width + 3) // 4 * 4 + (next(self._pads) if self.first_pad else 0)

    def _add(self, name, g, out=False, check_finite=True):
        self.all.append((name, g))
        if out:
            self.outs.append((name, g, check_finite))
        return g

    def inp(self, name, t, fixed=False, guard_rows=256, ld=None):
        """guarded copy of a 2-D host tensor; guard_rows: 2 for the tiled weight images, whose "rows" are whole groups of 10^5
        elements"""
        t = torch.as_tensor(t)
        g = guarded(t.shape[0], t.shape[1], ld=self._ld(t.shape[1], ld, fixed), dtype=t.dtype, device="cuda", lead=self.lead,
                    guard_rows=guard_rows, any_width=fixed or ld is not None or self.first_pad == 1)
        g.fill(t.cuda())
        return self._add(name, g)

    def vec(self, name, t):
        """a vector operand (bias, weights of a row dot): one guarded row"""
        t = torch.as_tensor(t).reshape(1, -1)
        g = guarded(1, t.shape[1], ld=(t.shape[1] + 3) // 4 * 4, dtype=t.dtype, device="cuda", lead=self.lead)
        g.fill(t.cuda())
        return self._add(name, g)

    def out(self, name, rows, width, dtype=torch.float32, fill=None, fixed=False, live_rows=None, check_finite=True, ld=None):
        g = guarded(rows, width, ld=self._ld(width, ld, fixed), dtype=dtype, device="cuda", lead=self.lead, live_rows=live_rows,
                    any_width=fixed or ld is not None or self.first_pad == 1)
        if fill is not None:
            g.fill(fill)
        return self._add(name, g, out=True, check_finite=check_finite)

    def blob(self, name, nbytes):
        """an opaque byte buffer of exactly the size a *_bytes / *_elems function reports (saved state, workspace): one guarded
        row with at least 256 KiB of pattern on each side (two 256 x 128 fp32 tiles).  What the library keeps in it is its own
        business: only the bytes around it are checked."""
        ld = (max(int(nbytes), 1) + 15) // 16 * 16
        g = guarded(1, max(int(nbytes), 1), ld=ld, dtype=torch.uint8, device="cuda", lead=self.lead, guard_rows=(-(-262144 // ld) + 15) // 16 * 16)  # (x 16: the twin's base stays 256-byte aligned)
        return self._add(name, g)

    def dev(self, a, dtype=None):
        t = _dev(a, dtype)
        self.keep.append(t)  # referenced until the sync
        return t

    def finish(self):
        """sync, every float output finite, every guard untouched -> {name: contiguous payload on the host}"""
        torch.cuda.synchronize()
        res = {}
        for name, g, check_finite in self.outs:
            p = g.payload()
            if check_finite and p.dtype == torch.float32:
                assert bool(torch.isfinite(p).all()), f"{name}: non-finite values in the output (pad {self.first_pad})"
            res[name] = p.cpu()
        for name, g in self.all:
            g.assert_untouched(f"{name} (pad {self.first_pad})")
        return res


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _rows_t(ops, srcs):
    """bl_rows_t from [(Guarded, device index or None)]"""
    r = ops.bl_rows_t()
    for j, (g, idx) in enumerate(srcs):
        r.x[j], r.idx[j], r.ld[j], r.width[j] = g.data_ptr(), (idx.data_ptr() if idx is not None else None), g.ld, g.width
    r.nsrc = len(srcs)
    return r


def _rows_packed_t(ops, srcs):
    """bl_rows_packed_t from [(Guarded packed int16, device index or None, width)]"""
    r = ops.bl_rows_packed_t()
    for j, (g, idx, w) in enumerate(srcs):
        r.xp[j], r.idx[j], r.width[j] = g.data_ptr(), (idx.data_ptr() if idx is not None else None), w
    r.nsrc = len(srcs)
    return r


def _both(run, pad):
    """the strided call and its ld == width twin"""
    return run(pad), run(0)


def _assert_bit_equal(got, twin, names=None):
    for k in names or got:
        assert torch.equal(got[k], twin[k]), f"{k}: the strided call and the contiguous call differ in bits"


def _gw_rows(T, K, gap=3):
    """rows of a grouped weight gradient with gw_group_stride = (K + gap) * ld_gw: live rows = the K rows of each group"""
    return (torch.arange(T * (K + gap)) % (K + gap)) < K


# ------------------------------------------------------------------------------------------------ the harness itself
def test_guard_check_trips_on_a_device_side_write(ops):
    """Positive control on the device, no kernel involved: one torch index write into a padding column, one into the row after
    the payload and one into the element in front of it are each found and named; payload writes are not."""
    g = guarded(129, 96, ld=100, dtype=torch.float32, device="cuda")
    assert g.view.is_cuda and g.view.data_ptr() % 32 == 16 and g.view.stride() == (100, 1)
    g.fill(torch.randn(129, 96))
    g.view[128, 95] = 3.0
    g.assert_untouched("payload writes only")
    flat = g.bits.view(torch.float32)
    for at, text in ((g.offset + 7 * 100 + 96, "row 7, col 96"), (g.offset + 129 * 100 + 3, "row M+0, col 3"), (g.offset - 1, "row -1, col 99")):
        saved = g.bits[at].clone()
        flat[at] = 0.0
        with pytest.raises(AssertionError) as e:
            g.assert_untouched("planted")
        assert text in str(e.value), str(e.value)
        g.bits[at] = saved
        g.assert_untouched("restored")


# ------------------------------------------------------------------------------------------------ (a) exact-fp32 GEMMs
def _gemm_rows_case(ops, pad, form, M, N, widths, sizes=None, group_w=None, T=None, seed=0):
    """form "kn": C = A . B_g; "nk": C = A . B_g^T; "epi": kn + bias + tanh + dropout.  Sources of more than one width list entry
    are gathered, each with its own ld."""
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    K, G = int(sum(widths)), (len(sizes) if sizes else 1)
    T = T or G
    gw_map = list(group_w) if group_w is not None else list(range(G))
    ptr = _ptr(sizes) if sizes else np.array([0, M], dtype=np.int32)
    R = 70
    gathered = len(widths) > 1 or sizes is not None
    xs = [torch.randn(R if gathered else M, w) for w in widths]
    idxs = [rng.integers(0, R, M).astype(np.int32) if gathered else None for _ in widths]
    W = torch.randn(T, K, N) / math.sqrt(K)  # logical [T][K][N]
    Wst = W if form != "nk" else W.transpose(1, 2).contiguous()  # stored [T][N][K] for the transposed form
    bias = torch.randn(N) if form == "epi" else None
    A = torch.cat([x[i.astype(np.int64)] if i is not None else x for x, i in zip(xs, idxs)], -1).double()
    ref = torch.zeros(M, N, dtype=torch.float64)
    for g in range(G):
        lo, hi = int(ptr[g]), int(ptr[g + 1])
        ref[lo:hi] = A[lo:hi] @ W[gw_map[g]].double()
    drop = ops.NO_DROPOUT
    if form == "epi":
        from oracle import buglab_oracle as O

        drop = ops.Dropout(0.3, 1234, 7)
        keep = torch.from_numpy(O.dropout_keep_mask(1234, 7, M * N, 0.3)).view(M, N)
        ref = torch.tanh(ref + bias.double()) * keep / (1 - np.float32(0.3)).astype(np.float64)

    def run(p):
        b = Bufs(p)
        srcs = [(b.inp(f"a.x[{j}]", x), b.dev(i) if i is not None else None) for j, (x, i) in enumerate(zip(xs, idxs))]
        gb = b.inp("b", Wst.reshape(-1, Wst.shape[-1]))  # [T * rows, cols] with ldb > cols
        gbias = b.vec("bias", bias) if bias is not None else None
        c = b.out("c", M, N)
        rows = _rows_t(ops, srcs)
        d_ptr = b.dev(ptr) if sizes else None
        d_gw = b.dev(np.array(gw_map, dtype=np.int32)) if group_w is not None else None
        ops._check(ops.load_library().bl_gemm_rows(ctypes.byref(rows), gb.data_ptr(), Wst.shape[1] * gb.ld, gb.ld, int(form == "nk"),
                                                   gbias.data_ptr() if gbias else None, d_ptr.data_ptr() if sizes else None,
                                                   d_gw.data_ptr() if d_gw is not None else None, G, M, N, K,
                                                   ops.ACT_TANH if form == "epi" else ops.ACT_NONE, drop.c(), c.data_ptr(), c.ld, _stream()),
                   "bl_gemm_rows")
        return b.finish()

    return run, ref


@pytest.mark.parametrize("pad", [4, 36])
@pytest.mark.parametrize("form,M,N,widths,sizes", [
    ("kn", 1, 96, (64,), None), ("kn", 129, 160, (64,), None), ("kn", 257, 256, (256,), None), ("nk", 257, 96, (256,), None),
    ("kn", 452, 160, (32, 32), SIZES), ("nk", 452, 96, (128, 128), SIZES), ("kn", 129, 96, (64,) * 1 + (64,), None),
    ("epi", 257, 160, (64, 64, 128), None), ("epi", 129, 96, (64,), None),
    ("kn", 65 * 128 + 1, 160, (64,), None),  # (enough row tiles for the 128-row-tile kernel; the shapes above take the few-tiles form)
])
def test_gemm_rows_strided(ops, pad, form, M, N, widths, sizes):
    """Would catch: a B / A / bias load that assumes ld == width, a float4 store past column N into c's padding, a tail row tile
    stored past row M, padding NaNs of a partial k stage or column tile reaching the accumulators."""
    run, ref = _gemm_rows_case(ops, pad, form, M, N, widths, sizes)
    got, twin = _both(run, pad)
    err = float((got["c"].double() - ref).abs().max())
    # test_gemm_rows_grouped_gathered: < 2e-5 abs at K <= 256; test_gemm_rows_bias_act_dropout_three_sources: < 3e-5 with the epilogue
    assert err < (3e-5 if form == "epi" else 2e-5), err
    _assert_bit_equal(got, twin)


def _routed_case(ops, pad, Nout, K, sizes, group_w=None, T=None):
    """bl_gemm_rows_routed: C[r] = (gq[tgt[r]] masked to r's wins) . B_g^T, winner table with ld_winner > K"""
    rng = np.random.default_rng(3)
    torch.manual_seed(3)
    G, M, Nn = len(sizes), int(sum(sizes)), 61
    T = T or G
    gw_map = list(group_w) if group_w is not None else list(range(G))
    ptr = _ptr(sizes)
    tgt = rng.integers(0, Nn, M).astype(np.int32)
    arg = np.full((Nn, K), -1, dtype=np.int32)
    for n in range(Nn):
        inc = np.nonzero(tgt == n)[0]
        if len(inc):
            arg[n] = rng.choice(inc, K)
    gq, W = torch.randn(Nn, K), torch.randn(T, Nout, K) / math.sqrt(K)
    won = torch.from_numpy(arg[tgt] == np.arange(M)[:, None])
    Gm = torch.where(won, gq[tgt.astype(np.int64)].double(), torch.zeros(M, K, dtype=torch.float64))
    ref = torch.zeros(M, Nout, dtype=torch.float64)
    for g in range(G):
        lo, hi = int(ptr[g]), int(ptr[g + 1])
        ref[lo:hi] = Gm[lo:hi] @ W[gw_map[g]].double().T

    def run(p):
        b = Bufs(p)
        ggq, gwin, gb = b.inp("gq", gq), b.inp("winner", torch.from_numpy(arg)), b.inp("b", W.reshape(-1, K))
        c = b.out("c", M, Nout)
        d_tgt, d_ptr = b.dev(tgt), b.dev(ptr)
        d_gw = b.dev(np.array(gw_map, dtype=np.int32)) if group_w is not None else None
        rows = _rows_t(ops, [(ggq, d_tgt)])
        ops._check(ops.load_library().bl_gemm_rows_routed(ctypes.byref(rows), gwin.data_ptr(), gwin.ld, gb.data_ptr(), Nout * gb.ld, gb.ld,
                                                          d_ptr.data_ptr(), d_gw.data_ptr() if d_gw is not None else None, G, M, Nout, K,
                                                          c.data_ptr(), c.ld, _stream()), "bl_gemm_rows_routed")
        return b.finish()

    return run, ref


@pytest.mark.parametrize("pad", [4, 36])
@pytest.mark.parametrize("Nout,K", [(96, 64), (160, 256)])
def test_gemm_rows_routed_strided(ops, pad, Nout, K):
    """Would catch: the winner table read at ld == K, gq rows read at ld == K, stores into c's padding."""
    run, ref = _routed_case(ops, pad, Nout, K, SIZES)
    got, twin = _both(run, pad)
    # test_segment_max_layernorm_fwd_bwd asserts the routed exact-fp32 GEMMs inside its layer chain at < 3e-5 x max(1, largest
    # entry); there is no contiguous test of this entry point alone, so that bound is REUSED here for the same kernel at K <= 256
    assert float((got["c"].double() - ref).abs().max()) < 3e-5 * max(1.0, float(ref.abs().max()))
    _assert_bit_equal(got, twin)


def _wgrad_case(ops, pad, N, widths, sizes, routed, group_w=None, T=None):
    """bl_gemm_wgrad / bl_gemm_wgrad_routed: gw[group_w[g]] += rows(a)^T . g rows, gw strided in both directions"""
    rng = np.random.default_rng(4)
    torch.manual_seed(4)
    K, G, M, R, Nn = int(sum(widths)), len(sizes), int(sum(sizes)), 70, 61
    T = T or G
    gw_map = list(group_w) if group_w is not None else list(range(G))
    ptr = _ptr(sizes)
    xs = [torch.randn(R, w) for w in widths]
    idxs = [rng.integers(0, R, M).astype(np.int32) for _ in widths]
    A = torch.cat([x[i.astype(np.int64)] for x, i in zip(xs, idxs)], -1).double()
    if routed:
        tgt = rng.integers(0, Nn, M).astype(np.int32)
        arg = np.full((Nn, N), -1, dtype=np.int32)
        for n in range(Nn):
            inc = np.nonzero(tgt == n)[0]
            if len(inc):
                arg[n] = rng.choice(inc, N)
        gnode = torch.randn(Nn, N)
        Gm = torch.where(torch.from_numpy(arg[tgt] == np.arange(M)[:, None]), gnode[tgt.astype(np.int64)].double(), torch.zeros(M, N, dtype=torch.float64))
    else:
        gnode = torch.randn(M, N)
        Gm = gnode.double()
    ref = torch.full((T, K, N), 0.5, dtype=torch.float64)
    for g in range(G):
        lo, hi = int(ptr[g]), int(ptr[g + 1])
        ref[gw_map[g]] += A[lo:hi].T @ Gm[lo:hi]

    def run(p):
        b = Bufs(p)
        srcs = [(b.inp(f"a.x[{j}]", x), b.dev(i)) for j, (x, i) in enumerate(zip(xs, idxs))]
        gg = b.inp("g", gnode)
        gw = b.out("gw", T * (K + 3), N, fill=0.5, live_rows=_gw_rows(T, K))
        d_ptr = b.dev(ptr)
        d_gw = b.dev(np.array(gw_map, dtype=np.int32)) if group_w is not None else None
        gwp = d_gw.data_ptr() if d_gw is not None else None
        rows = _rows_t(ops, srcs)
        lib = ops.load_library()
        if routed:
            gwin, d_tgt = b.inp("winner", torch.from_numpy(arg)), b.dev(tgt)
            ops._check(lib.bl_gemm_wgrad_routed(ctypes.byref(rows), gg.data_ptr(), gg.ld, d_tgt.data_ptr(), gwin.data_ptr(), gwin.ld, d_ptr.data_ptr(),
                                                gwp, G, M, N, K, gw.data_ptr(), (K + 3) * gw.ld, gw.ld, _stream()), "bl_gemm_wgrad_routed")
        else:
            ops._check(lib.bl_gemm_wgrad(ctypes.byref(rows), gg.data_ptr(), gg.ld, d_ptr.data_ptr(), gwp, G, M, N, K, gw.data_ptr(),
                                         (K + 3) * gw.ld, gw.ld, _stream()), "bl_gemm_wgrad")
        return b.finish()

    return run, ref.reshape(T * K, N)


@pytest.mark.parametrize("pad", [4, 36])
@pytest.mark.parametrize("routed", [False, True])
@pytest.mark.parametrize("N,widths", [(96, (32, 32)), (160, (128, 128))])
def test_gemm_wgrad_strided(ops, pad, routed, N, widths):
    """Would catch: atomics addressed with ld_gw == N or a group stride of K * ld_gw (the gap rows between the groups and gw's
    padding columns are guard), g / winner rows read at ld == N, a partial feature or column tile added past K or N."""
    run, ref = _wgrad_case(ops, pad, N, widths, SIZES, routed)
    got = run(pad)
    # test_gemm_rows_grouped_gathered (plain) / test_segment_max_layernorm_fwd_bwd (routed, inside its layer chain) assert these
    # weight gradients at < 3e-5 x max(1, largest entry): REUSED for the same kernels; the 0.5 the payload starts from is exact
    assert float((got["gw"].double() - ref).abs().max()) < 3e-5 * max(1.0, float(ref.abs().max()))


# ------------------------------------------------------------------------------------------------ (b) packers and packed GEMMs
def _unpack_bf16x3(p, D):
    u = p.numpy().view(np.uint16).astype(np.uint32) << 16
    return torch.from_numpy(u.view(np.float32).astype(np.float64)).view(p.shape[0], 3, D).sum(1)


def _unpack_f16x2(p, D):
    return torch.from_numpy(p.numpy().view(np.float16).astype(np.float64)).view(p.shape[0], 2, D).sum(1)


@pytest.mark.parametrize("pad", [4, 36])
@pytest.mark.parametrize("R,D", [(1, 8), (129, 96), (257, 320)])
def test_pack_bf16x3_strided(ops, pad, R, D):
    """Would catch: source rows read at ld == D, a vectorised tail that packs padding columns into the next plane."""
    torch.manual_seed(R)
    x = torch.randn(R, D)

    def run(p):
        b = Bufs(p)
        gx, out = b.inp("x", x), b.out("out", R, 3 * D, dtype=torch.int16, fixed=True)
        ops._check(ops.load_library().bl_pack_bf16x3(gx.data_ptr(), gx.ld, R, D, out.data_ptr(), _stream()), "bl_pack_bf16x3")
        return b.finish()

    got, twin = _both(run, pad)
    # test_gemm_rows_bf16x6_is_fp32_accurate: hi + mid + lo reproduces the fp32 value to 2^-24 of the largest entry
    assert float((_unpack_bf16x3(got["out"], D) - x.double()).abs().max()) <= 2.0 ** -24 * float(x.abs().max())
    _assert_bit_equal(got, twin)


@pytest.mark.parametrize("pad", [4, 36])
@pytest.mark.parametrize("kind", ["bf16x3_cols", "f16x2"])
@pytest.mark.parametrize("R,D,D_total,col_off", [(129, 96, 160, 32), (257, 32, 96, 8), (1, 8, 24, 8)])
def test_pack_into_a_column_window_strided(ops, pad, kind, R, D, D_total, col_off):
    """bl_pack_bf16x3_cols / bl_pack_f16x2 with col_off > 0 and D_total > col_off + D.  Would catch: writes outside the window
    of a plane (the other columns of the packed rows must keep what they held), source rows read at ld == D."""
    torch.manual_seed(R + D)
    planes = 3 if kind == "bf16x3_cols" else 2
    x = torch.tanh(torch.randn(R, D)) * 1.25
    scale = 256.0

    def run(p):
        b = Bufs(p)
        gx = b.inp("x", x)
        out = b.out("out", R, planes * D_total, dtype=torch.int16, fixed=True)  # starts as the 0x7FC1 pattern everywhere
        lib = ops.load_library()
        if kind == "bf16x3_cols":
            ops._check(lib.bl_pack_bf16x3_cols(gx.data_ptr(), gx.ld, R, D, D_total, col_off, out.data_ptr(), _stream()), "bl_pack_bf16x3_cols")
        else:
            ops._check(lib.bl_pack_f16x2(gx.data_ptr(), gx.ld, R, D, D_total, col_off, scale, None, out.data_ptr(), _stream()), "bl_pack_f16x2")
        return b.finish()

    got, twin = _both(run, pad)
    o = got["out"].view(R, planes, D_total)
    window = torch.zeros(D_total, dtype=torch.bool)
    window[col_off:col_off + D] = True
    assert bool((o[:, :, ~window] == PATTERN_16).all()), "columns outside the window were written"
    w = o[:, :, window].contiguous().view(R, planes * D)
    if kind == "bf16x3_cols":
        assert float((_unpack_bf16x3(w, D) - x.double()).abs().max()) <= 2.0 ** -24 * float(x.abs().max())
    else:  # test_gemm_rows_f16x3_is_fp32_accurate: 2^-23 relative or 2^-25 / scale absolute
        tol = torch.maximum(x.double().abs() * 2.0 ** -23, torch.full((R, D), 2.0 ** -25 / scale, dtype=torch.float64))
        assert bool(((_unpack_f16x2(w, D) / scale - x.double()).abs() <= tol).all())
    _assert_bit_equal(got, twin)


def _packed_rows_case(ops, pad, kind, N, widths, sizes, M=None, routed=False, group_w=None, T=None):
    """bl_gemm_rows_x6 / _x6_epi / _x6w / _h3 with ldc > N (and ld_bits > K / 32 in the routed form).  The packed operands have
    no leading dimension in the ABI: they are made by the wrappers and copied into guarded, 16-byte-only aligned buffers."""
    rng = np.random.default_rng(5)
    torch.manual_seed(5)
    K, G = int(sum(widths)), (len(sizes) if sizes else 1)
    M = int(sum(sizes)) if sizes else M
    T = T or G
    gw_map = list(group_w) if group_w is not None else list(range(G))
    ptr = _ptr(sizes) if sizes else np.array([0, M], dtype=np.int32)
    R = 70
    h3 = kind == "h3"
    xs = [torch.tanh(torch.randn(R, w)) * 1.25 for w in widths]
    idxs = [rng.integers(0, R, M).astype(np.int32) for _ in widths]
    W = torch.randn(T, K, N) / math.sqrt(K)
    bias = torch.randn(N) * 0.1 if kind == "x6_epi" else None
    A = torch.cat([x[i.astype(np.int64)] for x, i in zip(xs, idxs)], -1)
    bits = None
    if routed:  # any bit pattern is a valid routing mask here (test_wide_row_gemm_is_bit_identical_to_the_128_tile)
        bits = rng.integers(-2 ** 31, 2 ** 31, (M, K // 32)).astype(np.int32)
        bits[::7] = 0
        keepm = np.unpackbits(bits.view(np.uint8).reshape(M, -1), axis=1, bitorder="little").astype(bool)
        A = torch.where(torch.from_numpy(keepm), A, torch.zeros_like(A))
    ref = torch.zeros(M, N, dtype=torch.float64)
    for g in range(G):
        lo, hi = int(ptr[g]), int(ptr[g + 1])
        ref[lo:hi] = A[lo:hi].double() @ W[gw_map[g]].double()
    # the exact-fp32 kernel's own error on the same operands (the yardstick of the existing bound)
    Ad, Wd = _dev(A), _dev(W)
    d_ptr0 = _dev(ptr)
    exact = ops.gemm_rows([(Ad, None)], Wd, M, N, b_group_stride=K * N, ldb=N, group_ptr=d_ptr0 if sizes else None,
                          group_w=_dev(np.array(gw_map, dtype=np.int32)) if group_w is not None else None, G=G)
    err32 = float((exact.cpu().double() - ref).abs().max())
    drop = ops.NO_DROPOUT
    if kind == "x6_epi":
        from oracle import buglab_oracle as O

        drop = ops.Dropout(0.25, 7, 3)
        keep = torch.from_numpy(O.dropout_keep_mask(7, 3, M * N, 0.25)).view(M, N)
        ref = torch.tanh(ref + bias.double()) * keep / (1 - np.float32(0.25)).astype(np.float64)
    if h3:
        packed = [ops.pack_f16x2(_dev(x), ops.H3_ROW_SCALE).cpu() for x in xs]
        image = ops.pack_weights_h3(Wd, True).cpu()
    else:
        packed = [ops.pack_bf16x3(_dev(x)).cpu() for x in xs]
        image = (ops.pack_weights_x6w if kind == "x6w" else ops.pack_weights_x6)(Wd, True).cpu()

    def run(p):
        b = Bufs(p)
        srcs = [(b.inp(f"a.xp[{j}]", xp, fixed=True), b.dev(i), w) for j, (xp, i, w) in enumerate(zip(packed, idxs, widths))]
        gb = b.inp("bp", image, fixed=True, guard_rows=2)
        gbits = b.inp("win_bits", torch.from_numpy(bits)) if routed else None
        gbias = b.vec("bias", bias) if bias is not None else None
        c = b.out("c", M, N)
        d_ptr = b.dev(ptr) if sizes else None
        d_gw = b.dev(np.array(gw_map, dtype=np.int32)) if group_w is not None else None
        pp, gp = (d_ptr.data_ptr() if sizes else None), (d_gw.data_ptr() if d_gw is not None else None)
        bp_, ldb_ = (gbits.data_ptr(), gbits.ld) if routed else (None, 0)
        r = _rows_packed_t(ops, srcs)
        lib = ops.load_library()
        if kind == "x6_epi":
            ops._check(lib.bl_gemm_rows_x6_epi(ctypes.byref(r), gb.data_ptr(), gb.ld, pp, gp, G, M, N, K, gbias.data_ptr(), ops.ACT_TANH, drop.c(),
                                               c.data_ptr(), c.ld, _stream()), "bl_gemm_rows_x6_epi")
        elif h3:
            ops._check(lib.bl_gemm_rows_h3(ctypes.byref(r), bp_, ldb_, gb.data_ptr(), gb.ld, pp, gp, G, M, N, K,
                                           1.0 / (ops.H3_ROW_SCALE * ops.H3_W_SCALE), None, c.data_ptr(), c.ld, _stream()), "bl_gemm_rows_h3")
        else:
            fn = lib.bl_gemm_rows_x6w if kind == "x6w" else lib.bl_gemm_rows_x6
            ops._check(fn(ctypes.byref(r), bp_, ldb_, gb.data_ptr(), gb.ld, pp, gp, G, M, N, K, c.data_ptr(), c.ld, _stream()), "bl_gemm_rows_" + kind)
        return b.finish()

    return run, ref, err32


@pytest.mark.parametrize("pad", [4, 36])
@pytest.mark.parametrize("kind,N,widths,sizes,M,routed", [
    ("x6", 96, (32, 32), SIZES, None, False), ("x6", 160, (128, 128), SIZES, None, False), ("x6", 256, (64,), None, 257, False),
    ("x6", 96, (256,), SIZES, None, True), ("x6", 160, (64,), None, 1, False),
    ("x6_epi", 160, (64,), None, 129, False), ("x6_epi", 96, (128, 128), None, 257, False),
    ("x6w", 256, (128, 128), SIZES, None, False), ("x6w", 256, (64,), None, 129, False), ("x6w", 256, (256,), SIZES, None, True),
    ("h3", 96, (32, 32), SIZES, None, False), ("h3", 160, (128, 128), None, 257, False), ("h3", 256, (256,), SIZES, None, True),
])
def test_packed_row_gemms_strided(ops, pad, kind, N, widths, sizes, M, routed):
    """Would catch: the epilogue's stores at ldc == N or past column N of the last column tile (the 128- and 256-wide tiles),
    tail row tiles stored past M, routing words read at ld_bits == K / 32, operands assumed better than 16-byte aligned."""
    run, ref, err32 = _packed_rows_case(ops, pad, kind, N, widths, sizes, M=M, routed=routed)
    got, twin = _both(run, pad)
    err = float((got["c"].double() - ref).abs().max())
    if kind == "x6_epi":
        # DERIVED from test_dense_bf16x6_gemms_match_fp64's < 5e-6 against fp64 through tanh, which is asserted there without
        # dropout: the epilogue here multiplies the surviving entries by 1 / (1 - p) = 1 / 0.75 once, so the same absolute error
        # is scaled by that factor and by nothing else
        assert err < 5e-6 / 0.75, err
    else:  # test_gemm_rows_bf16x6_is_fp32_accurate / test_gemm_rows_f16x3_is_fp32_accurate
        assert err < 2e-5 and err < 4 * err32 + 1e-6, (err, err32)
    _assert_bit_equal(got, twin)


def _packed_wgrad_case(ops, pad, kind, N, widths, sizes, group_w=None, T=None):
    """bl_gemm_wgrad_x6 / _routed_x6 / _h3 with ld_gw > N and gw_group_stride > K * ld_gw"""
    rng = np.random.default_rng(6)
    torch.manual_seed(6)
    K, G, M, R, Nn = int(sum(widths)), len(sizes), int(sum(sizes)), 70, 61
    T = T or G
    gw_map = list(group_w) if group_w is not None else list(range(G))
    ptr = _ptr(sizes)
    routed, h3 = kind == "routed_x6", kind == "h3"
    xs = [torch.tanh(torch.randn(R, w)) * 1.25 for w in widths]
    idxs = [rng.integers(0, R, M).astype(np.int32) for _ in widths]
    A = torch.cat([x[i.astype(np.int64)] for x, i in zip(xs, idxs)], -1).double()
    tgt = rng.integers(0, Nn, M).astype(np.int32)
    gnode = torch.randn(Nn, N)
    Gm = gnode[tgt.astype(np.int64)].double()
    bits = None
    if routed:
        bits = rng.integers(-2 ** 31, 2 ** 31, (M, N // 32)).astype(np.int32)
        bits[::7] = 0
        keepm = np.unpackbits(bits.view(np.uint8).reshape(M, -1), axis=1, bitorder="little").astype(bool)
        Gm = torch.where(torch.from_numpy(keepm), Gm, torch.zeros_like(Gm))
    ref = torch.full((T, K, N), 0.5, dtype=torch.float64)
    for g in range(G):
        lo, hi = int(ptr[g]), int(ptr[g + 1])
        ref[gw_map[g]] += A[lo:hi].T @ Gm[lo:hi]
    if h3:
        am = ops.amax(_dev(gnode))
        packed = [ops.pack_f16x2(_dev(x), ops.H3_ROW_SCALE).cpu() for x in xs]
        gpk = ops.pack_f16x2(_dev(gnode), 1.0, amax=am).cpu()
    else:
        packed = [ops.pack_bf16x3(_dev(x)).cpu() for x in xs]
        gpk = ops.pack_bf16x3(_dev(gnode)).cpu()

    def run(p):
        b = Bufs(p)
        srcs = [(b.inp(f"a.xp[{j}]", xp, fixed=True), b.dev(i), w) for j, (xp, i, w) in enumerate(zip(packed, idxs, widths))]
        gg = b.inp("g_packed", gpk, fixed=True)
        gbits = b.inp("win_bits", torch.from_numpy(bits)) if routed else None
        gw = b.out("gw", T * (K + 3), N, fill=0.5, live_rows=_gw_rows(T, K))
        d_ptr, d_tgt = b.dev(ptr), b.dev(tgt)
        d_gw = b.dev(np.array(gw_map, dtype=np.int32)) if group_w is not None else None
        gp = d_gw.data_ptr() if d_gw is not None else None
        r = _rows_packed_t(ops, srcs)
        lib = ops.load_library()
        stride = (K + 3) * gw.ld
        if h3:
            d_am = b.dev(am)
            ops._check(lib.bl_gemm_wgrad_h3(ctypes.byref(r), gg.data_ptr(), d_tgt.data_ptr(), None, 0, d_ptr.data_ptr(), gp, G, M, N, K,
                                            1.0 / ops.H3_ROW_SCALE, d_am.data_ptr(), gw.data_ptr(), stride, gw.ld, _stream()), "bl_gemm_wgrad_h3")
        elif routed:
            ops._check(lib.bl_gemm_wgrad_routed_x6(ctypes.byref(r), gg.data_ptr(), d_tgt.data_ptr(), gbits.data_ptr(), gbits.ld, d_ptr.data_ptr(), gp,
                                                   G, M, N, K, gw.data_ptr(), stride, gw.ld, _stream()), "bl_gemm_wgrad_routed_x6")
        else:
            ops._check(lib.bl_gemm_wgrad_x6(ctypes.byref(r), gg.data_ptr(), d_tgt.data_ptr(), d_ptr.data_ptr(), gp, G, M, N, K, gw.data_ptr(),
                                            stride, gw.ld, _stream()), "bl_gemm_wgrad_x6")
        return b.finish()

    return run, ref.reshape(T * K, N)


def _packed_wgrad_bound(kind, got, ref):
    err, scale = float((got.double() - ref).abs().max()), float(ref.abs().max())
    if kind == "h3":  # test_routed_gemms_f16x3_match_fp64: < 4e-6 x the largest entry
        assert err < 4e-6 * scale, (err, scale)
    elif kind == "routed_x6":  # test_routed_gemms_bf16x6_match_fp64: < 2e-6 x max(scale, 1) x 4
        assert err < 2e-6 * max(scale, 1.0) * 4, (err, scale)
    else:  # test_dense_bf16x6_gemms_match_fp64: < 1e-4 x max(1, largest entry)
        assert err < 1e-4 * max(1.0, scale), (err, scale)


@pytest.mark.parametrize("pad", [4, 36])
@pytest.mark.parametrize("tile", [256, 128])
@pytest.mark.parametrize("kind", ["x6", "routed_x6", "h3"])
@pytest.mark.parametrize("N,widths", [(96, (32, 32)), (160, (128, 128))])
def test_packed_wgrad_strided(ops, pad, tile, kind, N, widths):
    """Both bl_set_wgrad_tile settings ((128, 128) sources with K = 256 take the 256 x 128 tile at the default).  Would catch: a
    tile flushed with ld_gw == N or a group stride of K * ld_gw, a 256-row tile's second half added past row K, a partial column
    tile added past N into gw's padding."""
    prev = ops.set_wgrad_tile(tile)
    try:
        run, ref = _packed_wgrad_case(ops, pad, kind, N, widths, SIZES)
        got = run(pad)
    finally:
        ops.set_wgrad_tile(prev)
    _packed_wgrad_bound(kind, got["gw"], ref)


# ------------------------------------------------------------------------------------------------ group_w
GROUP_W = [1, 0, 1, 1]   # G = 4 groups over T = 2 weight matrices: three groups share matrix 1
GW_SIZES = [130, 1, 257, 64]


@pytest.mark.parametrize("group_w", [GROUP_W, [0, 1, 2, 3]], ids=["shared", "identity"])
@pytest.mark.parametrize("entry", ["rows", "rows_routed", "wgrad", "wgrad_routed", "rows_x6", "rows_x6_epi", "rows_x6w", "rows_h3", "wgrad_x6",
                                   "wgrad_routed_x6", "wgrad_h3"])
def test_group_w_maps_groups_to_weight_matrices(ops, entry, group_w):
    """The group-to-weight map every grouped GEMM takes and no caller passes: rows forms read B of matrix group_w[g]; weight
    gradient forms add into matrix group_w[g] -- the three groups that share matrix 1 must SUM into it (on top of the 0.5 that is
    there), matrix 0 gets its one row.  The identity map is the control.  Would catch: group_w ignored, applied to the wrong
    operand, or groups overwriting instead of accumulating."""
    T = max(group_w) + 1
    if entry == "rows":
        run, ref = _gemm_rows_case(ops, 4, "kn", int(sum(GW_SIZES)), 96, (32, 32), GW_SIZES, group_w=group_w, T=T)
        assert float((run(4)["c"].double() - ref).abs().max()) < 2e-5  # test_gemm_rows_grouped_gathered
    elif entry == "rows_routed":
        run, ref = _routed_case(ops, 4, 96, 64, GW_SIZES, group_w=group_w, T=T)
        assert float((run(4)["c"].double() - ref).abs().max()) < 3e-5 * max(1.0, float(ref.abs().max()))
    elif entry in ("wgrad", "wgrad_routed"):
        run, ref = _wgrad_case(ops, 4, 96, (32, 32), GW_SIZES, entry == "wgrad_routed", group_w=group_w, T=T)
        assert float((run(4)["gw"].double() - ref).abs().max()) < 3e-5 * max(1.0, float(ref.abs().max()))
    elif entry.startswith("rows_"):
        kind = entry[5:]
        run, ref, err32 = _packed_rows_case(ops, 4, kind, 256 if kind == "x6w" else 96, (32, 32), GW_SIZES, group_w=group_w, T=T)
        err = float((run(4)["c"].double() - ref).abs().max())
        assert (err < 5e-6 / 0.75) if kind == "x6_epi" else (err < 2e-5 and err < 4 * err32 + 1e-6), (err, err32)
    else:
        kind = entry[6:]
        run, ref = _packed_wgrad_case(ops, 4, kind, 96, (32, 32), GW_SIZES, group_w=group_w, T=T)
        _packed_wgrad_bound(kind, run(4)["gw"], ref)


# ------------------------------------------------------------------------------------------------ (c) row-wise graph kernels
def _segment_max_case(ops, pad, D, act, bwd=True):
    from oracle import buglab_oracle as O

    rng = np.random.default_rng(2)
    torch.manual_seed(2)
    nseg, E = 57, 1300
    seg = rng.integers(0, nseg, E)
    seg[seg == 5] = 6
    seg[seg == 40] = 41      # empty segments
    seg[:513] = 11           # one segment of (at least) 513 items
    items = np.argsort(seg, kind="stable").astype(np.int32)
    ptr = _ptr(np.bincount(seg, minlength=nseg))
    order = np.concatenate([[11], np.delete(np.arange(nseg), 11)]).astype(np.int32)  # the hub first, as the collator lists it
    x, go = torch.randn(E, D), torch.randn(nseg, D)
    xr = x.double().requires_grad_(True)
    xa = O._gelu(xr) if act == "gelu" else xr
    ref, arg = O.scatter_max_with_arg(xa, torch.from_numpy(seg), nseg)
    ref = O._gelu(ref) if act == "gelu_aggregated" else ref
    ref.backward(go.double())
    a_ref = torch.where(arg == E, torch.full_like(arg, -1), arg)
    W32 = (D + 31) // 32
    wonp = np.zeros((E, W32 * 32), dtype=bool)
    wonp[:, :D] = (a_ref[torch.from_numpy(seg).long()] == torch.arange(E)[:, None]).numpy()
    ref_bits = torch.from_numpy(np.packbits(wonp.reshape(E, W32, 32), axis=-1, bitorder="little").view(np.int32).reshape(E, W32))

    def run(p):
        b = Bufs(p)
        gx = b.inp("x", x)
        out, garg = b.out("out", nseg, D, fixed=True), b.out("arg", nseg, D, dtype=torch.int32, fixed=True)
        dact, wb = b.out("dact", nseg, D, fixed=True), b.out("winbits", E, W32, dtype=torch.int32, fixed=True)
        d_ptr, d_items, d_order = b.dev(ptr), b.dev(items), b.dev(order)
        lib = ops.load_library()
        ops._check(lib.bl_segment_max_fwd(gx.data_ptr(), gx.ld, d_ptr.data_ptr(), d_items.data_ptr(), nseg, D, ops._ACTS[act], out.data_ptr(),
                                          garg.data_ptr(), None, None, 1e-5, None, None, None, dact.data_ptr(), wb.data_ptr(), d_order.data_ptr(),
                                          _stream()), "bl_segment_max_fwd")
        if not bwd:
            return b.finish()
        # backward: g_x shares x's leading dimension in the ABI
        ggo, d_seg = b.inp("g_out", go, fixed=True), b.dev(seg.astype(np.int32))
        g_x = b.out("g_x", E, D, ld=gx.ld)
        ops._check(lib.bl_segment_max_bwd(ggo.data_ptr(), garg.data_ptr(), gx.data_ptr(), gx.ld, d_seg.data_ptr(), E, D, ops._ACTS[act],
                                          g_x.data_ptr(), _stream()), "bl_segment_max_bwd")
        return b.finish()

    got, twin = _both(run, pad)
    # test_segment_max_layernorm_fwd_bwd: out < 1e-6, arg and the routing bits exact, g_x < 1e-5
    assert float((got["out"].double() - ref.detach()).abs().max()) < 1e-6
    assert torch.equal(got["arg"].long(), a_ref) and torch.equal(got["winbits"], ref_bits)
    if bwd:
        assert float((got["g_x"].double() - xr.grad).abs().max()) < 1e-5
    _assert_bit_equal(got, twin)


@pytest.mark.parametrize("pad", [4, 36])
@pytest.mark.parametrize("D,act", [(8, "none"), (96, "gelu"), (320, "gelu_aggregated")])
def test_segment_max_fwd_bwd_strided(ops, pad, D, act):
    """bl_segment_max_fwd with ldx > D, seg_items and seg_order given, a 513-item segment (the four-wave hub path) and empty
    segments; bl_segment_max_bwd on the same rows.  Would catch: item rows read at ldx == D, padding lanes (d >= D) of the last
    64-lane group compared or stored, routing words written past ceil(D / 32), g_x rows written at the wrong stride."""
    _segment_max_case(ops, pad, D, act)


@pytest.mark.parametrize("pad", [4, 36])
@pytest.mark.parametrize("R,N", [(1, 8), (129, 96), (257, 320)])
def test_act_bwd_strided(ops, pad, R, N):
    """bl_act_bwd and bl_act_bwd_packed with ld > N (g_y, y and g_z share it).  Would catch: rows addressed at ld == N, the packed
    copy written at 3 ld instead of 3 N, column sums that include padding columns or rows past nrows."""
    from oracle import buglab_oracle as O

    torch.manual_seed(N)
    drop = ops.Dropout(0.2, 99, 3)
    keep = torch.from_numpy(O.dropout_keep_mask(99, 3, R * N, 0.2)).view(R, N)
    t = torch.tanh(torch.randn(R, N).double())
    y, g = (t * keep / (1 - 0.2)).float(), torch.randn(R, N)
    ref = g.double() * keep / (1 - 0.2) * (1 - t * t)

    def run(p):
        b = Bufs(p)
        ld = N + p  # g_y, y and g_z share one leading dimension in the ABI
        bufs = {"g_y": b.inp("g_y", g, ld=ld), "y": b.inp("y", y, ld=ld), "g_z": b.out("g_z", R, N, ld=ld), "g_z2": b.out("g_z2", R, N, ld=ld)}
        gb, gb2 = b.out("g_bias", 1, N, fill=0.5, fixed=True), b.out("g_bias2", 1, N, fill=0.5, fixed=True)
        gzp = b.out("g_z_packed", R, 3 * N, dtype=torch.int16, fixed=True)
        lib = ops.load_library()
        ops._check(lib.bl_act_bwd(bufs["g_y"].data_ptr(), bufs["y"].data_ptr(), R, N, ld, ops.ACT_TANH, drop.c(), bufs["g_z"].data_ptr(), gb.data_ptr(),
                                  _stream()), "bl_act_bwd")
        ops._check(lib.bl_act_bwd_packed(bufs["g_y"].data_ptr(), bufs["y"].data_ptr(), R, N, ld, ops.ACT_TANH, drop.c(), bufs["g_z2"].data_ptr(),
                                         gb2.data_ptr(), gzp.data_ptr(), _stream()), "bl_act_bwd_packed")
        return b.finish()

    got, twin = _both(run, pad)
    # test_act_bwd_and_bias: g_z < 1e-5, the column sums < 1e-4
    assert float((got["g_z"].double() - ref).abs().max()) < 1e-5
    for k in ("g_bias", "g_bias2"):
        assert float((got[k][0].double() - (0.5 + ref.sum(0))).abs().max()) < 1e-4
    # test_node_update_bwd_matches_fp64's bound on a packed g_z: 1e-6 x max(1, largest entry)
    assert float((_unpack_bf16x3(got["g_z_packed"], N) - ref).abs().max()) < 1e-6 * max(1.0, float(ref.abs().max()))
    _assert_bit_equal(got, twin, ("g_z", "g_z2", "g_z_packed"))
    assert torch.equal(got["g_z"], got["g_z2"])


def _mp_scatter_case(ops, pad, form, Din, split=32):
    from buglab.data.collate import _csr

    rng = np.random.default_rng(3)
    torch.manual_seed(3)
    N, E = 129, 700
    src, tgt = rng.integers(0, N, E), rng.integers(0, N, E)
    tgt[:150] = 7
    ga = torch.randn(E, 2 * Din)
    ref = torch.full((N, Din), 0.5 if form == "accumulate" else 0.0, dtype=torch.float64)
    ref.index_add_(0, torch.from_numpy(src), ga[:, :Din].double())
    ref.index_add_(0, torch.from_numpy(tgt), ga[:, Din:].double())
    (sp, sm), (tp, tm) = _csr(src, N), _csr(tgt, N)

    def run(p):
        b = Bufs(p)
        gga = b.inp("g_a", ga)
        d = [b.dev(a) for a in (sp, sm, tp, tm)]
        lib = ops.load_library()
        if form == "split":
            lo, hi = b.out("g_h_lo", N, split), b.out("g_h_hi", N, Din - split)
            ops._check(lib.bl_mp_scatter_grad_split(gga.data_ptr(), gga.ld, *(t.data_ptr() for t in d), N, Din, split, lo.data_ptr(), lo.ld,
                                                    hi.data_ptr(), hi.ld, None, _stream()), "bl_mp_scatter_grad_split")
        else:
            gh = b.out("g_h", N, Din, fill=0.5 if form == "accumulate" else None)
            ops._check(lib.bl_mp_scatter_grad(gga.data_ptr(), gga.ld, *(t.data_ptr() for t in d), N, Din, int(form == "accumulate"), gh.data_ptr(),
                                              gh.ld, None, _stream()), "bl_mp_scatter_grad")
        return b.finish()

    got, twin = _both(run, pad)
    joined = torch.cat([got["g_h_lo"], got["g_h_hi"]], 1) if form == "split" else got["g_h"]
    assert float((joined.double() - ref).abs().max()) < 1e-4  # test_mp_scatter_grad
    _assert_bit_equal(got, twin)


@pytest.mark.parametrize("pad", [4, 36])
@pytest.mark.parametrize("form,Din", [("one", 8), ("one", 96), ("one", 320), ("accumulate", 96), ("split", 96)])
def test_mp_scatter_grad_strided(ops, pad, form, Din):
    """bl_mp_scatter_grad with ld_ga > 2 Din and ld_gh > Din (accumulate 0 and 1) and bl_mp_scatter_grad_split with split = 32.
    Would catch: the target half read at column Din of a row addressed with ld == 2 Din, padding lanes d >= Din of the last
    64-lane group stored, the second output written at the first one's stride."""
    _mp_scatter_case(ops, pad, form, Din)


def _gru_cell_case(ops, pad, N, D):
    torch.manual_seed(D)
    gi, gh, h, go = torch.randn(N, 3 * D), torch.randn(N, 3 * D), torch.randn(N, D), torch.randn(N, D)
    gi64, gh64, h64 = (t.double().requires_grad_(True) for t in (gi, gh, h))
    r = torch.sigmoid(gi64[:, :D] + gh64[:, :D])
    z = torch.sigmoid(gi64[:, D:2 * D] + gh64[:, D:2 * D])
    n = torch.tanh(gi64[:, 2 * D:] + r * gh64[:, 2 * D:])
    ref = (1 - z) * n + z * h64
    ref.backward(go.double())

    def run(p):
        b = Bufs(p)
        ggi, ggh, ggo = b.inp("gi", gi, fixed=True), b.inp("gh", gh, fixed=True), b.inp("g_out", go, fixed=True)
        gh_ = b.inp("h", h)
        out = b.out("out", N, D, fixed=True)
        o_gi, o_gh, o_h = b.out("g_gi", N, 3 * D, fixed=True), b.out("g_gh", N, 3 * D, fixed=True), b.out("g_h", N, D, fixed=True)
        lib = ops.load_library()
        ops._check(lib.bl_gru_cell_fwd(ggi.data_ptr(), ggh.data_ptr(), gh_.data_ptr(), gh_.ld, N, D, ops.NO_DROPOUT.c(), out.data_ptr(), _stream()),
                   "bl_gru_cell_fwd")
        ops._check(lib.bl_gru_cell_bwd(ggo.data_ptr(), ggi.data_ptr(), ggh.data_ptr(), gh_.data_ptr(), gh_.ld, N, D, ops.NO_DROPOUT.c(),
                                       o_gi.data_ptr(), o_gh.data_ptr(), o_h.data_ptr(), _stream()), "bl_gru_cell_bwd")
        return b.finish()

    got, twin = _both(run, pad)
    # DERIVED, not inherited (no contiguous test of the cell alone exists): fp32 elementwise arithmetic on O(1) values -- expf /
    # tanhf to a few ulp, a handful of products and sums, every intermediate below 4 in size -- stays below 20 ulp(4) = 1e-5 abs;
    # it is also the bound test_act_bwd_and_bias asserts for its elementwise g_z
    assert float((got["out"].double() - ref.detach()).abs().max()) < 1e-5
    assert float((got["g_gi"].double() - gi64.grad).abs().max()) < 1e-5
    assert float((got["g_gh"].double() - gh64.grad).abs().max()) < 1e-5
    assert float((got["g_h"].double() - h64.grad).abs().max()) < 1e-5  # (the direct part z x g_out IS the whole gradient w.r.t. h here)
    _assert_bit_equal(got, twin)


@pytest.mark.parametrize("pad", [4, 36])
@pytest.mark.parametrize("N,D", [(1, 8), (129, 96), (257, 320)])
def test_gru_cell_strided(ops, pad, N, D):
    """bl_gru_cell_fwd / _bwd with ld_h > D (gi, gh, out and the gradients are contiguous in the ABI).  Would catch: h read at
    ld == D, the last thread block running past N x D."""
    _gru_cell_case(ops, pad, N, D)


@pytest.mark.parametrize("entry", ["segment_max_fwd", "mp_scatter_grad", "mp_scatter_grad_accumulate", "mp_scatter_grad_split", "gru_cell"])
def test_any_width_entry_points_at_an_odd_width(ops, entry):
    """The entry points whose header text says "any width", at D = 7 with ld = 9 and a base that is 4-byte aligned and no more
    (bl_segment_max_bwd is not one of them: it moves float4s).  Would catch: a vectorised access that needs a multiple of 4, lanes
    d >= D of a 64-lane group stored into the next row.  Same references, bounds and bit equality with the contiguous call as the
    multiple-of-4 cases."""
    if entry == "segment_max_fwd":
        _segment_max_case(ops, 1, 7, "gelu", bwd=False)
    elif entry == "gru_cell":
        _gru_cell_case(ops, 1, 129, 7)
    else:
        _mp_scatter_case(ops, 1, {"mp_scatter_grad": "one", "mp_scatter_grad_accumulate": "accumulate", "mp_scatter_grad_split": "split"}[entry], 7, split=3)


# ------------------------------------------------------------------------------------------------ (e) heads
@pytest.mark.parametrize("pad", [4, 36])
@pytest.mark.parametrize("R,D", [(1, 8), (129, 96), (257, 320)])
def test_gather_scatter_rows_strided(ops, pad, R, D):
    """bl_gather_rows with ld_x and ld_out; bl_scatter_add_rows with col_off = 16, ld_src and ld_out into a target that holds
    0.5.  Would catch: float4 copies at ld == width, the column window of the source taken at the wrong offset, adds that land
    in the target's padding."""
    rng = np.random.default_rng(R)
    torch.manual_seed(R)
    nx, nt, width = 300, 20, max(4, D - 16 - 4)
    x, src = torch.randn(nx, D), torch.randn(R, 16 + width + 4)
    idx, tidx = rng.integers(0, nx, R).astype(np.int32), rng.integers(0, nt, R).astype(np.int32)
    ref_add = torch.full((nt, width), 0.5, dtype=torch.float64).index_add_(0, torch.from_numpy(tidx).long(), src[:, 16:16 + width].double())

    def run(p):
        b = Bufs(p)
        gx, gsrc = b.inp("x", x), b.inp("src", src)
        out, tgt = b.out("out", R, D), b.out("target", nt, width, fill=0.5)
        d_idx, d_tidx = b.dev(idx), b.dev(tidx)
        lib = ops.load_library()
        ops._check(lib.bl_gather_rows(gx.data_ptr(), gx.ld, d_idx.data_ptr(), R, D, out.data_ptr(), out.ld, _stream()), "bl_gather_rows")
        ops._check(lib.bl_scatter_add_rows(gsrc.data_ptr(), gsrc.ld, 16, width, d_tidx.data_ptr(), R, tgt.data_ptr(), tgt.ld, _stream()),
                   "bl_scatter_add_rows")
        return b.finish()

    got, twin = _both(run, pad)
    assert torch.equal(got["out"], x[idx.astype(np.int64)])  # test_gather_rows_fwd_bwd: exact
    assert float((got["target"].double() - ref_add).abs().max()) < 1e-5  # test_rowdot_and_scatter_add
    _assert_bit_equal(got, twin, ("out",))


@pytest.mark.parametrize("pad", [4, 36])
@pytest.mark.parametrize("R,H", [(1, 8), (129, 96), (257, 320)])
def test_rowdot_strided(ops, pad, R, H):
    """bl_rowdot_fwd / _bwd with ldx > H and ld_gx > H; g_w and g_b accumulate on top of 0.5.  Would catch: rows read at
    ldx == H, padding columns entering the dot product or the weight gradient, g_x rows written at ldx."""
    torch.manual_seed(H)
    x, w, bia, gy = torch.randn(R, H), torch.randn(H), torch.randn(1), torch.randn(R)

    def run(p):
        b = Bufs(p)
        gx, gw_, gb_ = b.inp("x", x), b.vec("w", w), b.vec("b", torch.cat([bia, torch.zeros(3)]))
        ggy = b.vec("g_y", torch.cat([gy, torch.zeros((-R) % 4)]))
        y = b.out("y", 1, R, fixed=True) if R % 4 == 0 else b.out("y", 1, (R + 3) // 4 * 4, fixed=True, check_finite=False)
        g_x, g_w, g_b = b.out("g_x", R, H), b.out("g_w", 1, H, fill=0.5, fixed=True), b.out("g_b", 1, 4, fill=0.5, fixed=True)
        lib = ops.load_library()
        ops._check(lib.bl_rowdot_fwd(gx.data_ptr(), gx.ld, gw_.data_ptr(), gb_.data_ptr(), R, H, y.data_ptr(), _stream()), "bl_rowdot_fwd")
        ops._check(lib.bl_rowdot_bwd(ggy.data_ptr(), gx.data_ptr(), gx.ld, gw_.data_ptr(), R, H, g_x.data_ptr(), g_x.ld, g_w.data_ptr(),
                                     g_b.data_ptr(), _stream()), "bl_rowdot_bwd")
        return b.finish()

    got, twin = _both(run, pad)
    # test_rowdot_and_scatter_add: y < 1e-5, g_x < 1e-6, g_w and g_b < 1e-4
    yv = got["y"][0, :R]
    assert bool(torch.isfinite(yv).all()) and float((yv.double() - (x.double() @ w.double() + bia.double())).abs().max()) < 1e-5
    assert bool(torch.isnan(got["y"][0, R:]).all())  # the vector's tail past R kept the pattern
    assert float((got["g_x"] - gy[:, None] * w[None]).abs().max()) < 1e-6
    assert float((got["g_w"][0].double() - (0.5 + (gy.double()[:, None] * x.double()).sum(0))).abs().max()) < 1e-4
    assert abs(float(got["g_b"][0, 0]) - (0.5 + float(gy.double().sum()))) < 1e-4 and bool((got["g_b"][0, 1:] == 0.5).all())
    assert torch.equal(got["y"][0, :R], twin["y"][0, :R]) and torch.equal(got["g_x"], twin["g_x"])


# ------------------------------------------------------------------------------------------------ (c) the subtoken embedder
@pytest.mark.parametrize("pad", [4, 36])
@pytest.mark.parametrize("combination,before", [("max", False), ("max", True), ("sum", True), ("mean", False)])
def test_embed_subtoken_pool_strided(ops, pad, combination, before):
    """bl_embed_subtoken_pool_fwd with ld_out > H, bl_embed_subtoken_pool_bwd and _bwd_sorted with ld_g > H, the table gradient
    starting from 0.5.  Would catch: the pooled rows stored at ld_out == H (the float4 store of the last column group running into
    the padding), g_out rows read at ld_g == H, a dropout counter taken from the strided address instead of n * H + h."""
    from buglab.data.collate import token_occurrence_chunks
    from oracle import buglab_oracle as O

    rng = np.random.default_rng(6)
    torch.manual_seed(6)
    V, H, N, S = 97, 96, 129, 6
    comb = {"max": 0, "sum": 1, "mean": 2}[combination]
    table, go = torch.randn(V, H), torch.randn(N, H)
    ids = rng.integers(0, V, (N, S)).astype(np.int32)
    ids[: N // 2, 0] = 7  # a hot token: several chunks of the sorted form
    lens = rng.integers(1, S + 1, N).astype(np.int32)
    tr = table.clone().requires_grad_(True)
    ref = O.embed_nodes(tr, ids, lens, 0.25, 42, "before_pooling" if before else "after_pooling", combination)
    ref.backward(go)
    occ, cptr, ctok = token_occurrence_chunks(ids, lens, chunk=16)
    drop = ops.Dropout(0.25, 42, 0)

    def run(p):
        b = Bufs(p)
        gt, ggo = b.inp("table", table, fixed=True), b.inp("g_out", go)
        out = b.out("out", N, H)
        argsub = b.out("argsub", N, H, dtype=torch.int8, fixed=True) if comb == 0 else None
        g_table, g_table_s = b.out("g_table", V, H, fill=0.5, fixed=True), b.out("g_table_sorted", V, H, fill=0.5, fixed=True)
        d_ids, d_lens, d_occ, d_cptr, d_ctok = (b.dev(a) for a in (ids, lens, occ, cptr, ctok))
        ap = argsub.data_ptr() if argsub is not None else None
        lib = ops.load_library()
        ops._check(lib.bl_embed_subtoken_pool_fwd(gt.data_ptr(), V, H, d_ids.data_ptr(), d_lens.data_ptr(), N, S, comb, drop.c(), int(before),
                                                  out.data_ptr(), out.ld, ap, _stream()), "bl_embed_subtoken_pool_fwd")
        ops._check(lib.bl_embed_subtoken_pool_bwd(ggo.data_ptr(), ggo.ld, d_ids.data_ptr(), d_lens.data_ptr(), ap, N, S, H, V, comb, drop.c(),
                                                  int(before), g_table.data_ptr(), _stream()), "bl_embed_subtoken_pool_bwd")
        ops._check(lib.bl_embed_subtoken_pool_bwd_sorted(ggo.data_ptr(), ggo.ld, d_occ.data_ptr(), d_cptr.data_ptr(), d_ctok.data_ptr(),
                                                         int(ctok.shape[0]), d_lens.data_ptr(), ap, S, H, comb, drop.c(), int(before),
                                                         g_table_s.data_ptr(), _stream()), "bl_embed_subtoken_pool_bwd_sorted")
        return b.finish()

    got, twin = _both(run, pad)
    # test_embed_fwd_bwd: the pooled rows < 1e-6 (max) / 1e-5 (sum, mean), the table gradient < 1e-4, in both forms
    assert float((got["out"] - ref.detach()).abs().max()) < (1e-6 if combination == "max" else 1e-5)
    for k in ("g_table", "g_table_sorted"):
        assert float((got[k] - (0.5 + tr.grad)).abs().max()) < 1e-4, k
    _assert_bit_equal(got, twin, ("out",) + (("argsub",) if comb == 0 else ()))


# ------------------------------------------------------------------------------------------------ (d) routed input gradient
@pytest.mark.parametrize("pad", [4, 36])
@pytest.mark.parametrize("Dm,Din,split", [(64, 64, None), (64, 64, 32), (128, 128, None), (128, 128, 32)])
def test_routed_dgrad_strided(ops, pad, Dm, Din, split):
    """bl_routed_dgrad_vec / _nodes / _nodes_rows with ld_gq, ld_bits, ld_ga, ld_lo, ld_hi and ld_src above their widths; one or
    two node-gradient outputs.  Would catch: gq rows or routing words read at ld == width, a per-message row stored at ld == 2 Din,
    atomics addressed with the other output's leading dimension or past column split, source rows of messages that won nothing
    left unwritten (they would read back as the NaN pattern)."""
    rng = np.random.default_rng(7)
    torch.manual_seed(7)
    sizes = SIZES
    N, T, E = 61, len(sizes), int(sum(sizes))
    assert ops.load_library().bl_routed_dgrad_vec_ok(Dm, 2 * Din) == 1
    W = torch.randn(T, 2 * Din, Dm) / math.sqrt(2 * Din)
    gq = torch.randn(N, Dm)
    ptr = _ptr(sizes)
    tgt = np.concatenate([np.sort(rng.integers(0, N, s)) for s in sizes]).astype(np.int32)  # target-sorted inside a type
    src = rng.integers(0, N, E).astype(np.int32)
    arg = np.full((N, Dm), -1, dtype=np.int32)
    for n in range(N):
        inc = np.nonzero(tgt == n)[0]
        if len(inc):
            arg[n] = rng.choice(inc[: max(1, len(inc) - 1)], Dm)  # (the last incoming message of a node wins nothing)
    won = arg[tgt] == np.arange(E)[:, None]
    Gm = torch.where(torch.from_numpy(won), gq[tgt.astype(np.int64)].double(), torch.zeros(E, Dm, dtype=torch.float64))
    ref_dA = torch.zeros(E, 2 * Din, dtype=torch.float64)
    for t in range(T):
        ref_dA[ptr[t]:ptr[t + 1]] = Gm[ptr[t]:ptr[t + 1]] @ W[t].double().T
    ref_tgt = torch.zeros(N, Din, dtype=torch.float64).index_add_(0, torch.from_numpy(tgt.astype(np.int64)), ref_dA[:, Din:])
    ref_h = ref_tgt.clone().index_add_(0, torch.from_numpy(src.astype(np.int64)), ref_dA[:, :Din])
    bits = np.packbits(won.reshape(E, Dm // 32, 32), axis=-1, bitorder="little").view(np.int32).reshape(E, Dm // 32)
    wt = W.transpose(1, 2).contiguous()  # [T, Dm, 2 Din]: no leading dimension in the ABI

    def run(p):
        b = Bufs(p)
        ggq, gbits = b.inp("gq", gq), b.inp("win_bits", torch.from_numpy(bits))
        gwt = b.inp("wt", wt.reshape(T * Dm, 2 * Din), fixed=True)
        d_src, d_tgt, d_ptr = b.dev(src), b.dev(tgt), b.dev(ptr)
        g_a = b.out("g_a", E, 2 * Din)
        sp = Din if split is None else split

        def node_outputs(tag):  # the caller zeroes what the atomics add into
            lo = b.out("g_h_lo" + tag, N, sp, fill=0.0)
            return lo, (b.out("g_h_hi" + tag, N, Din - sp, fill=0.0) if split is not None else None)

        lo, hi = node_outputs("")
        lo2, hi2 = node_outputs("_rows")
        g_src = b.out("g_src", E, Din)
        lib = ops.load_library()
        common = (gbits.data_ptr(), gbits.ld, d_ptr.data_ptr(), T, gwt.data_ptr(), E, Dm)
        ops._check(lib.bl_routed_dgrad_vec(ggq.data_ptr(), ggq.ld, d_tgt.data_ptr(), *common, 2 * Din, g_a.data_ptr(), g_a.ld, _stream()),
                   "bl_routed_dgrad_vec")
        ops._check(lib.bl_routed_dgrad_nodes(ggq.data_ptr(), ggq.ld, d_src.data_ptr(), d_tgt.data_ptr(), *common, Din, sp, lo.data_ptr(), lo.ld,
                                             hi.data_ptr() if hi else None, hi.ld if hi else 0, _stream()), "bl_routed_dgrad_nodes")
        ops._check(lib.bl_routed_dgrad_nodes_rows(ggq.data_ptr(), ggq.ld, d_src.data_ptr(), d_tgt.data_ptr(), *common, Din, sp, lo2.data_ptr(),
                                                  lo2.ld, hi2.data_ptr() if hi2 else None, hi2.ld if hi2 else 0, g_src.data_ptr(), g_src.ld,
                                                  _stream()), "bl_routed_dgrad_nodes_rows")
        return b.finish()

    got, twin = _both(run, pad)

    def joined(tag):
        return (torch.cat([got["g_h_lo" + tag], got["g_h_hi" + tag]], 1) if split is not None else got["g_h_lo" + tag]).double()

    # test_routed_input_gradient_from_the_nonzeros_matches_fp64: every output < 2e-6 x max(1, largest entry of its reference family)
    tol_a, tol_h = 2e-6 * max(1.0, float(ref_dA.abs().max())), 2e-6 * max(1.0, float(ref_h.abs().max()))
    assert float((got["g_a"].double() - ref_dA).abs().max()) < tol_a
    assert float((joined("") - ref_h).abs().max()) < tol_h
    assert float((got["g_src"].double() - ref_dA[:, :Din]).abs().max()) < tol_a
    assert float((joined("_rows") - ref_tgt).abs().max()) < tol_h  # the target halves alone
    _assert_bit_equal(got, twin, ("g_a",))  # (the node sums are atomics)


# ------------------------------------------------------------------------------------------------ (e) the localization head
@pytest.mark.parametrize("pad", [4, 36])
def test_localization_scores_strided(ops, pad):
    """bl_localization_scores_fwd / _bwd with ld_x > H and ld_gx > H at H = 96, one graph without candidates, `saved` and both
    workspaces of exactly the bytes the library's own size functions report, guarded.  Would catch: a size function that reports
    less than the call uses (the guard behind the blob), node rows read or the node gradient added at ld == H, the empty graph's
    pooled row or a workspace tail reaching a result."""
    rng = np.random.default_rng(8)
    torch.manual_seed(8)
    H, Nn, per_graph = 96, 200, [50, 0, 129, 1]
    B, C = len(per_graph), int(sum(per_graph))
    cand = rng.integers(0, Nn, C).astype(np.int32)
    cand_graph = np.repeat(np.arange(B), per_graph).astype(np.int32)
    cand_ptr = _ptr(per_graph)
    x, g_score = torch.randn(Nn, H), torch.randn(C)
    Ws, bs = torch.randn(H, H) / math.sqrt(H), torch.randn(H) * 0.1
    W1, b1, w = torch.randn(2 * H, H) / math.sqrt(2 * H), torch.randn(H) * 0.1, torch.randn(H) / math.sqrt(H)
    leaves = [t.double().requires_grad_(True) for t in (x, Ws, bs, W1, b1, w)]
    x64, Ws64, bs64, W164, b164, w64 = leaves
    xc = x64[torch.from_numpy(cand).long()]
    summary = xc @ Ws64 + bs64
    pooled = torch.stack([summary[cand_ptr[g]:cand_ptr[g + 1]].max(0).values if per_graph[g] else torch.zeros(H, dtype=torch.float64)
                          for g in range(B)])
    ref = torch.sigmoid(torch.cat([xc, pooled[torch.from_numpy(cand_graph).long()]], 1) @ W164 + b164) @ w64
    ref.backward(g_score.double())

    def run(p):
        b = Bufs(p)
        lib = ops.load_library()
        gx = b.inp("x", x)
        gWs, gW1 = b.inp("Ws", Ws, fixed=True), b.inp("W1", W1, fixed=True)
        gbs, gb1, gw_, ggs = b.vec("bs", bs), b.vec("b1", b1), b.vec("w", w), b.vec("g_score", g_score)
        saved = b.blob("saved", lib.bl_localization_scores_saved_bytes(C, B, H))
        ws_f = b.blob("ws_fwd", lib.bl_localization_scores_workspace_bytes(C, B, H, 0))
        ws_b = b.blob("ws_bwd", lib.bl_localization_scores_workspace_bytes(C, B, H, 1))
        score = b.out("score", 1, C, fixed=True)
        g_x = b.out("g_x", Nn, H, fill=0.5)
        g_Ws, g_W1 = b.out("g_Ws", H, H, fill=0.5, fixed=True), b.out("g_W1", 2 * H, H, fill=0.5, fixed=True)
        g_bs, g_b1, g_w = (b.out(n, 1, H, fill=0.5, fixed=True) for n in ("g_bs", "g_b1", "g_w"))
        d_cand, d_cg, d_cp = b.dev(cand), b.dev(cand_graph), b.dev(cand_ptr)
        ops._check(lib.bl_localization_scores_fwd(gx.data_ptr(), gx.ld, d_cand.data_ptr(), d_cg.data_ptr(), d_cp.data_ptr(), C, B, H, gWs.data_ptr(),
                                                  gbs.data_ptr(), gW1.data_ptr(), gb1.data_ptr(), gw_.data_ptr(), saved.data_ptr(), ws_f.data_ptr(),
                                                  score.data_ptr(), _stream()), "bl_localization_scores_fwd")
        ops._check(lib.bl_localization_scores_bwd(gx.data_ptr(), gx.ld, d_cand.data_ptr(), d_cg.data_ptr(), d_cp.data_ptr(), C, B, H, gWs.data_ptr(),
                                                  gW1.data_ptr(), gw_.data_ptr(), saved.data_ptr(), ws_b.data_ptr(), ggs.data_ptr(), g_x.data_ptr(),
                                                  g_x.ld, g_Ws.data_ptr(), g_bs.data_ptr(), g_W1.data_ptr(), g_b1.data_ptr(), g_w.data_ptr(),
                                                  _stream()), "bl_localization_scores_bwd")
        return b.finish()

    got, twin = _both(run, pad)
    # DERIVED, not inherited (no contiguous test calls this entry point alone): the call chains the kernels above -- row GEMMs
    # (their own bound: 3e-5 abs with an epilogue at K <= 256), the exact segmented max, row dots (1e-5), column sums and atomic
    # adds (1e-4) -- on O(1) values with 1 / sqrt(K)-scaled weights, so no stage amplifies the one before it: three chained stages
    # forward stay below 1e-4, the accumulated gradients below 1e-4 x max(1, largest entry) as everywhere else in this file.
    assert float((got["score"][0].double() - ref.detach()).abs().max()) < 1e-4
    for name, leaf in (("g_x", x64), ("g_Ws", Ws64), ("g_bs", bs64), ("g_W1", W164), ("g_b1", b164), ("g_w", w64)):
        want = 0.5 + leaf.grad.reshape(got[name].shape)
        assert float((got[name].double() - want).abs().max()) < 1e-4 * max(1.0, float(want.abs().max())), name
    _assert_bit_equal(got, twin, ("score",))  # (forward has no atomics)


# ------------------------------------------------------------------------------------------------ (f) sequence kernels
@pytest.mark.parametrize("pad", [4, 36])
@pytest.mark.parametrize("Hh", [32, 128])
def test_gru_scan_strided(ops, pad, Hh):
    """bl_gru_scan_fwd / _bwd with ld_gi > 6 Hh, ld_out > 2 Hh, ld_g > 2 Hh and ld_ggi > 6 Hh, lens = [L, 1, 7], `saved` of exactly
    bl_gru_scan_saved_elems floats, guarded.  Would catch: gi rows read at ld == 6 Hh (the two-steps-ahead prefetch included), the
    zeros of padded positions written at the wrong stride or past row B L, a saved block larger than the size function says."""
    torch.manual_seed(Hh)
    B, L = 3, 9
    lens = np.array([L, 1, 7], dtype=np.int32)
    R = B * L
    gi, go = torch.randn(R, 6 * Hh), torch.randn(R, 2 * Hh)
    w_hh, b_hh = torch.randn(2, Hh, 3 * Hh) / math.sqrt(Hh), torch.randn(2, 3 * Hh) * 0.1
    # fp64: torch.nn.GRU's recurrence over each sequence's own length, the reverse direction from its last real token
    gi64, w64 = gi.double().requires_grad_(True), w_hh.double()
    b64 = b_hh.double().requires_grad_(True)  # (a leaf, so that every gh -- the first step's h is a constant -- can keep its gradient)
    ref = torch.zeros(R, 2 * Hh, dtype=torch.float64)
    ghs = {}
    rows = []
    for b_ in range(B):
        for d in range(2):
            h = torch.zeros(Hh, dtype=torch.float64)
            steps = range(int(lens[b_])) if d == 0 else range(int(lens[b_]) - 1, -1, -1)
            for t in steps:
                row = b_ * L + t
                g = gi64[row, d * 3 * Hh:(d + 1) * 3 * Hh]
                gh = h @ w64[d] + b64[d]
                gh.retain_grad()
                ghs[(d, row)] = gh
                r, z = torch.sigmoid(g[:Hh] + gh[:Hh]), torch.sigmoid(g[Hh:2 * Hh] + gh[Hh:2 * Hh])
                h = (1 - z) * torch.tanh(g[2 * Hh:] + r * gh[2 * Hh:]) + z * h
                rows.append((row, d, h))
    out64 = torch.zeros(R, 2 * Hh, dtype=torch.float64)
    loss = sum((h * go[row, d * Hh:(d + 1) * Hh].double()).sum() for row, d, h in rows)
    loss.backward()
    for row, d, h in rows:
        out64[row, d * Hh:(d + 1) * Hh] = h.detach()
    ref_ggh = torch.zeros(2, R, 3 * Hh, dtype=torch.float64)
    for (d, row), gh in ghs.items():
        ref_ggh[d, row] = gh.grad

    def run(p):
        b = Bufs(p)
        lib = ops.load_library()
        ggi, ggo = b.inp("gi", gi), b.inp("g_out", go)
        gw, gb = b.inp("w_hh", w_hh.reshape(2 * Hh, 3 * Hh), fixed=True), b.inp("b_hh", b_hh, fixed=True)
        saved = b.blob("saved", 4 * lib.bl_gru_scan_saved_elems(B, L, Hh))
        out, g_gi = b.out("out", R, 2 * Hh), b.out("g_gi", R, 6 * Hh)
        g_gh = b.out("g_gh", 2 * R, 3 * Hh, fixed=True)
        d_lens = b.dev(lens)
        ops._check(lib.bl_gru_scan_fwd(ggi.data_ptr(), ggi.ld, gw.data_ptr(), gb.data_ptr(), d_lens.data_ptr(), B, L, Hh, out.data_ptr(), out.ld,
                                       saved.data_ptr(), _stream()), "bl_gru_scan_fwd")
        ops._check(lib.bl_gru_scan_bwd(ggo.data_ptr(), ggo.ld, gw.data_ptr(), saved.data_ptr(), d_lens.data_ptr(), B, L, Hh, g_gi.data_ptr(),
                                       g_gi.ld, g_gh.data_ptr(), _stream()), "bl_gru_scan_bwd")
        return b.finish()

    got, twin = _both(run, pad)
    # test_stack_matches_torch_gru_over_packed_sequences: outputs < 1e-4, gradients <= 1e-4 x the largest entry + 1e-6; zeros at
    # padded positions are exact
    assert float((got["out"].double() - out64).abs().max()) < 1e-4
    valid = torch.from_numpy((np.arange(L)[None, :] < lens[:, None]).reshape(-1))
    assert float(got["out"][~valid].abs().max()) == 0.0 and float(got["g_gi"][~valid].abs().max()) == 0.0
    assert float((got["g_gi"].double() - gi64.grad).abs().max()) <= 1e-4 * float(gi64.grad.abs().max()) + 1e-6
    assert float((got["g_gh"].double().view(2, R, 3 * Hh) - ref_ggh).abs().max()) <= 1e-4 * float(ref_ggh.abs().max()) + 1e-6
    _assert_bit_equal(got, twin)


# ------------------------------------------------------------------------------------------------ (g) the layer call
def test_mp_layer_call_strided(ops):
    """bl_mp_layer_fwd / _bwd once at Din = Dm = Dout = 64 with the ConcatResidual pair [h_lo ; h_hi] (width_lo = 32) and its
    gradients g_h_lo / g_h_hi all strided, `saved` and both workspaces of exactly bl_mp_layer_saved_bytes / _workspace_bytes,
    guarded.  The reference is the same call on contiguous copies: bit-equal forward (output and winner table), gradients within
    the bound of test_fused_layer_call_equals_kernel_by_kernel_path.  This is the case that tells whether the size functions and
    the kernels agree: a kernel inside the call that uses more of `saved` / `ws` than reported changes the guard behind the blob.
    Would also catch: the pair read with one leading dimension for both halves, the packed input built from padding columns."""
    from buglab.data.collate import _csr
    from buglab.models.hip_ops import graph as G
    from buglab.models.hip_ops.weights import _packed_message_weights

    rng = np.random.default_rng(9)
    torch.manual_seed(9)
    N, T, Din, Dm, Dout, w_lo = 129, 3, 64, 64, 64, 32
    sizes = [300, 0, 400]
    E = int(sum(sizes))
    type_ptr = _ptr(sizes)
    tgt = np.concatenate([np.sort(rng.integers(0, N - 4, s)) for s in sizes]).astype(np.int32)  # (the last nodes receive nothing)
    src = rng.integers(0, N, E).astype(np.int32)
    (tp, tm), (sp, sm) = _csr(tgt.astype(np.int64), N), _csr(src.astype(np.int64), N)
    h_lo, h_hi, g_out = torch.randn(N, w_lo), torch.randn(N, Din - w_lo), torch.randn(N, Dout)
    W = torch.randn(T, 2 * Din, Dm) / math.sqrt(2 * Din)
    ln_g, ln_b = torch.rand(Dm) + 0.5, torch.randn(Dm) * 0.1
    Wd, bd = torch.randn(Dm, Dout) / math.sqrt(Dm), torch.randn(Dout) * 0.1
    drop = ops.Dropout(0.1, 11, 3)
    lib = ops.load_library()

    def run(p):
        b = Bufs(p)
        d = {k: b.dev(v) for k, v in dict(src=src, tgt=tgt, type_ptr=type_ptr, tp=tp, tm=tm, sp=sp, sm=sm, W=W, ln_g=ln_g, ln_b=ln_b, Wd=Wd,
                                          bd=bd).items()}
        wkn, wnk = _packed_message_weights(d["W"], Din, True)
        b.keep += [wkn, wnk]
        L = G.bl_mp_layer_t()
        L.N, L.E, L.T, L.Din, L.Dm, L.Dout = N, E, T, Din, Dm, Dout
        L.msg_src, L.msg_tgt, L.type_ptr = d["src"].data_ptr(), d["tgt"].data_ptr(), d["type_ptr"].data_ptr()
        L.tgt_ptr, L.tgt_msgs, L.src_ptr, L.src_msgs = d["tp"].data_ptr(), d["tm"].data_ptr(), d["sp"].data_ptr(), d["sm"].data_ptr()
        L.node_order, L.num_hub_slots, L.aggregation = None, 0, 0
        L.W, L.ln_g, L.ln_b, L.Wd, L.bd = (d[k].data_ptr() for k in ("W", "ln_g", "ln_b", "Wd", "bd"))
        L.msg_act, L.ln_eps, L.drop = ops.ACT_GELU_AGG, 1e-5, drop.c()  # (Wt, Wd_packed NULL: matrix-core input gradient, exact-fp32 dense)
        glo, ghi, ggo = b.inp("h_lo", h_lo), b.inp("h_hi", h_hi), b.inp("g_out", g_out, fixed=True)
        saved = b.blob("saved", lib.bl_mp_layer_saved_bytes(N, E, Din, Dm, ops.ACT_GELU_AGG))
        ws_f = b.blob("ws_fwd", lib.bl_mp_layer_workspace_bytes(N, E, Din, Dm, Dout, 0))
        ws_b = b.blob("ws_bwd", lib.bl_mp_layer_workspace_bytes(N, E, Din, Dm, Dout, 1))
        h_out = b.out("h_out", N, Dout, fixed=True)
        winner = b.out("winner", N, Dm, dtype=torch.int32, fixed=True)
        g_lo, g_hi = b.out("g_h_lo", N, w_lo), b.out("g_h_hi", N, Din - w_lo)
        g_W = b.out("g_W", T * 2 * Din, Dm, fill=0.5, fixed=True)
        g_Wd = b.out("g_Wd", Dm, Dout, fill=0.5, fixed=True)
        g_lng, g_lnb, g_bd = (b.out(n, 1, w, fill=0.5, fixed=True) for n, w in (("g_ln_g", Dm), ("g_ln_b", Dm), ("g_bd", Dout)))
        ops._check(lib.bl_mp_layer_fwd(ctypes.byref(L), glo.data_ptr(), glo.ld, w_lo, ghi.data_ptr(), ghi.ld, wkn.data_ptr(), h_out.data_ptr(),
                                       winner.data_ptr(), saved.data_ptr(), ws_f.data_ptr(), _stream()), "bl_mp_layer_fwd")
        ops._check(lib.bl_mp_layer_bwd(ctypes.byref(L), h_out.data_ptr(), ggo.data_ptr(), wnk.data_ptr(), saved.data_ptr(), ws_b.data_ptr(),
                                       g_lo.data_ptr(), g_lo.ld, w_lo, g_hi.data_ptr(), g_hi.ld, g_W.data_ptr(), g_lng.data_ptr(),
                                       g_lnb.data_ptr(), g_Wd.data_ptr(), g_bd.data_ptr(), _stream(), None, 1), "bl_mp_layer_bwd")
        return b.finish()

    got, twin = _both(run, 4)
    _assert_bit_equal(got, twin, ("h_out", "winner"))
    assert bool((got["winner"][N - 4:] == -1).all()) and bool((got["winner"][: N - 4] < E).all())
    for k in ("g_h_lo", "g_h_hi", "g_W", "g_Wd", "g_ln_g", "g_ln_b", "g_bd"):
        ref = twin[k]
        # test_fused_layer_call_equals_kernel_by_kernel_path: <= 1e-5 x the largest entry + 1e-7 (atomics reorder sums)
        assert float((got[k] - ref).abs().max()) <= 1e-5 * float(ref.abs().max()) + 1e-7, k
