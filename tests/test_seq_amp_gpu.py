"""GPU: the bf16x1 mode of the sequence models' projection GEMMs (hip_ops.set_seq_gemm_mode("bf16x1"), `train.py --amp` on seq-*):
the packed-row entry points bl_gemm_rows_x6 / _epi / _epi2 / bl_gemm_rows_x6w / bl_gemm_wgrad_x6 reading only the high plane of
the bf16x3 images, one MFMA term, fp32 accumulation.

Entry points are checked against fp64 products of the DECODED high planes (what the kernel is supposed to read), so operand
rounding is in the reference and the bound is the fp32 accumulation alone: 2 K 2^-24 sum|a||b| per element plus one fp32 ulp of
the result.  Where an epilogue multiplies the product by a constant (the dropout scale, the mask scale) the accumulation term is
multiplied by the same constant: that is how an error passes through a linear step."""
import copy
import ctypes
import json
import logging
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPI_ACT, EPI_ACT_PACK, EPI_RES, EPI_MASK_PACK = 0, 1, 2, 3  # BL_X6_EPI_* (include/buglab_hip.h)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from buglab.models import hip_ops

    hip_ops.load_library()
    assert hip_ops.seq_gemm_mode() == "bf16x6"  # the default
    return hip_ops


@pytest.fixture()
def x1(ops):
    prev = ops.set_seq_gemm_mode("bf16x1")
    try:
        yield ops
    finally:
        ops.set_seq_gemm_mode(prev)
    assert ops.seq_gemm_mode() == prev


# ---- decoding the packed images -------------------------------------------------------------------------------------------
def _bf16(bits: torch.Tensor) -> torch.Tensor:
    """int16 bf16 bit patterns -> fp64"""
    return ((bits.cpu().to(torch.int32) & 0xFFFF) << 16).view(torch.float32).double()


def _rows_plane(packed: torch.Tensor, D: int, plane: int = 0) -> torch.Tensor:
    """bl_pack_bf16x3 rows [R, 3 D] -> plane `plane` as fp64 [R, D]"""
    return _bf16(packed[:, plane * D:(plane + 1) * D])


def _rows_value(packed: torch.Tensor, D: int) -> torch.Tensor:
    """the fp32 value a three-plane image holds (hi + mid + lo is exact in fp64)"""
    return (_rows_plane(packed, D, 0) + _rows_plane(packed, D, 1) + _rows_plane(packed, D, 2)).float()


def _weights_plane0(image: torch.Tensor, G: int, K: int, N: int, wide: bool) -> torch.Tensor:
    """high plane of bl_pack_weights_x6 / _x6w's image as fp64 [G, K, N] (layouts: csrc/bl_gemm_x6.hip, csrc/bl_x6w_image.h)"""
    nst = K // 32
    if not wide:  # per (group, 128-column tile, 32-k stage): [i 2][plane 3][row_lo 64][k-group 4] x 8, column 64 i + row_lo
        ntn = (N + 127) // 128
        t = _bf16(image).view(G, ntn, nst, 2, 3, 64, 4, 8)[:, :, :, :, 0]  # [G, tile, stage, i, row_lo, k-group, 8]
        return t.permute(0, 2, 5, 6, 1, 3, 4).reshape(G, K, ntn * 128)[:, :, :N]
    # per (group, 256-column tile, stage): [plane 3][column 256][slot 4] x 8, k-group kg of column n in slot kg ^ ((n >> 2) & 3)
    ntn = (N + 255) // 256
    t = _bf16(image).view(G, ntn, nst, 3, 256, 4, 8)[:, :, :, 0]
    n = torch.arange(256)[:, None]
    slot = (torch.arange(4)[None, :] ^ ((n >> 2) & 3)).view(1, 1, 1, 256, 4, 1).expand(G, ntn, nst, 256, 4, 8)
    t = torch.gather(t, 4, slot)  # [.., column, k-group, 8]
    return t.permute(0, 2, 4, 5, 1, 3).reshape(G, K, ntn * 256)[:, :, :N]


def _ulp32(v: torch.Tensor) -> torch.Tensor:
    return torch.from_numpy(np.spacing(np.abs(v.numpy()).astype(np.float32)).astype(np.float64))


def _dev(a, dtype=None):
    t = torch.as_tensor(a)
    return (t.to(dtype) if dtype is not None else t).cuda()


class _Operands:
    """x [R, K] rows (gathered through idx) and W [G, K, N], packed once, with the fp64 view of what a bf16x1 kernel reads"""

    def __init__(self, ops, rng, M, K, N, *, G=1, sizes=None, gather=False, wide=False, R=None):
        R = R or (max(M, 8) if not gather else 37)
        self.M, self.K, self.N, self.G = M, K, N, G
        x = torch.from_numpy(rng.standard_normal((R, K)).astype(np.float32))
        W = torch.from_numpy((rng.standard_normal((G, K, N)) / math.sqrt(K)).astype(np.float32))
        self.idx = rng.integers(0, R, M).astype(np.int32) if gather else None  # (M > R or the birthday bound: repeats)
        if gather and M > 1:
            self.idx[-1] = self.idx[0]
        self.ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32) if sizes is not None else None
        self.xp = ops.pack_bf16x3(x.cuda())
        self.image = (ops.pack_weights_x6w if wide else ops.pack_weights_x6)(W.cuda(), True)
        self.wide = wide
        A = _rows_plane(self.xp, K)
        self.A = A[torch.from_numpy(self.idx.astype(np.int64))] if gather else A[:M]
        self.B = _weights_plane0(self.image, G, K, N, wide)
        self.d_idx = _dev(self.idx) if gather else None
        self.d_ptr = _dev(self.ptr) if sizes is not None else None

    def product(self, keep=None):
        """fp64 A0 . B0 and sum |a||b| per element, group by group"""
        A = self.A if keep is None else self.A * keep
        ref, mag = torch.zeros(self.M, self.N, dtype=torch.float64), torch.zeros(self.M, self.N, dtype=torch.float64)
        bounds = self.ptr if self.ptr is not None else np.array([0, self.M])
        for g in range(len(bounds) - 1):
            lo, hi = int(bounds[g]), int(bounds[g + 1])
            ref[lo:hi] = A[lo:hi] @ self.B[g]
            mag[lo:hi] = A[lo:hi].abs() @ self.B[g].abs()
        return ref, mag

    def source(self):
        return [(self.xp, self.d_idx, self.K)]


def _assert_within(got: torch.Tensor, ref: torch.Tensor, mag: torch.Tensor, K: int, what, factor: float = 1.0):
    got = got.cpu().double()
    assert bool(torch.isfinite(got).all()), what
    bound = factor * 2.0 * K * 2.0 ** -24 * mag + _ulp32(ref)
    excess = (got - ref).abs() - bound
    worst = int(torch.argmax(excess))
    assert float(excess.max()) <= 0.0, (what, float((got - ref).abs().flatten()[worst]), float(bound.flatten()[worst]))


SHAPES = [(M, K, N) for M in (1, 63, 65, 129) for K in (32, 96) for N in (32, 96)]


# ---- 1. entry points against fp64 on the plane-0 operands -----------------------------------------------------------------
def test_rows_no_epilogue_matches_fp64_of_the_high_planes(x1):
    """bl_gemm_rows_x6 in bf16x1: every (rows, K, N) of the grid; two groups with one of them empty; a gathered row index with
    repeats; the routed form (win_bits AND-mask on a gathered source)."""
    ops, rng = x1, np.random.default_rng(0)
    for M, K, N in SHAPES:
        o = _Operands(ops, rng, M, K, N)
        ref, mag = o.product()
        _assert_within(ops.gemm_rows_x6(o.source(), o.image, M, N), ref, mag, K, ("plain", M, K, N))
    for sizes in ((0, 65), (129, 0)):
        M = sum(sizes)
        o = _Operands(ops, rng, M, 96, 96, G=2, sizes=sizes, gather=True)
        ref, mag = o.product()
        _assert_within(ops.gemm_rows_x6(o.source(), o.image, M, 96, group_ptr=o.d_ptr, G=2), ref, mag, 96, ("grouped + gathered", sizes))
    # group_w: the second group uses the first group's weights
    o = _Operands(ops, rng, 70, 32, 96, G=2, sizes=(33, 37))
    o.B = o.B[[1, 0]]
    ref, mag = o.product()
    _assert_within(ops.gemm_rows_x6(o.source(), o.image, 70, 96, group_ptr=o.d_ptr, group_w=_dev(np.array([1, 0], dtype=np.int32)), G=2),
                   ref, mag, 32, "group_w")
    for M, K, N in ((65, 96, 96), (129, 32, 32)):
        o = _Operands(ops, rng, M, K, N, gather=True)
        bits = rng.integers(-2 ** 31, 2 ** 31, (M, K // 32)).astype(np.int32)
        bits[::7] = 0
        keep = torch.from_numpy(np.unpackbits(bits.view(np.uint8).reshape(M, -1), axis=1, bitorder="little").astype(np.float64))
        ref, mag = o.product(keep)
        _assert_within(ops.gemm_rows_x6(o.source(), o.image, M, N, win_bits=_dev(bits)), ref, mag, K, ("routed", M, K, N))


def test_rows_bias_relu_dropout_matches_fp64_of_the_high_planes(x1):
    """bl_gemm_rows_x6_epi in bf16x1: drop(relu(A . B + bias)) with the counter index row * N + column of the six-term form"""
    from oracle import buglab_oracle as O

    ops, rng = x1, np.random.default_rng(1)
    cases = [(M, K, N, None, False) for M, K, N in SHAPES] + [(65, 96, 96, (0, 65), True), (129, 32, 96, (129, 0), True)]
    for M, K, N, sizes, gather in cases:
        o = _Operands(ops, rng, M, K, N, G=2 if sizes else 1, sizes=sizes, gather=gather)
        bias = torch.from_numpy(rng.standard_normal(N).astype(np.float32))
        p = 0.3
        scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))  # bl_make_drop
        keep = torch.from_numpy(O.dropout_keep_mask(21, 4, M * N, p)).view(M, N).double()
        z, mag = o.product()
        ref = torch.relu(z + bias.double()) * keep * scale
        got = ops.gemm_rows_x6(o.source(), o.image, M, N, group_ptr=o.d_ptr, G=o.G, bias=bias.cuda(), act=ops.ACT_RELU, drop=ops.Dropout(p, 21, 4))
        # + one ulp of the pre-activation for the fp32 bias add, through the same scale
        _assert_within(got, ref, mag + (_ulp32(z + bias.double()) / (2.0 * K * 2.0 ** -24)), K, ("epi", M, K, N, sizes), factor=scale)
        assert bool(((got.cpu() == 0) | (keep > 0)).all())  # a dropped element is exactly zero


def _epi2(ops, o, M, N, K, form, *, bias=None, act=0, drop=None, res=None, y_packed=None, mask_scale=1.0, colsum=None, packed=False):
    lib = ops.load_library()
    e = ops.bl_x6_epi_t()
    e.form, e.act, e.mask_scale = form, act, mask_scale
    e.bias = bias.data_ptr() if bias is not None else None
    e.drop = (drop or ops.NO_DROPOUT).c()
    if res is not None:
        e.res, e.ld_res = res.data_ptr(), res.stride(0)
    e.y_packed = y_packed.data_ptr() if y_packed is not None else None
    e.colsum = colsum.data_ptr() if colsum is not None else None
    cp = torch.full((M, 3 * N), 0x7FC0, dtype=torch.int16, device="cuda") if packed else None  # (bf16 NaN: every plane must be written)
    e.c_packed = cp.data_ptr() if packed else None
    c = torch.full((M, N), float("nan"), device="cuda") if not packed else None
    r, K_ = ops._rows_packed(o.source())
    assert K_ == K
    ops._check(lib.bl_gemm_rows_x6_epi2(ctypes.byref(r), o.image.data_ptr(), M, N, K, ctypes.byref(e), c.data_ptr() if c is not None else None,
                                        N, ops._stream()), "bl_gemm_rows_x6_epi2")
    return cp if packed else c


def test_rows_residual_and_packed_outputs_match_fp64_of_the_high_planes(x1):
    """bl_gemm_rows_x6_epi2 in bf16x1, the three forms the GREAT layer uses: + residual (fp32 result); bias + relu + dropout with
    the result ONLY as a full three-plane image; the product masked by a packed forward output, packed, with column sums."""
    from oracle import buglab_oracle as O

    ops, rng = x1, np.random.default_rng(2)
    for M, K, N in SHAPES:
        o = _Operands(ops, rng, M, K, N, gather=(M == 65))
        z, mag = o.product()
        res = torch.from_numpy(rng.standard_normal((M, N)).astype(np.float32))
        got = _epi2(ops, o, M, N, K, EPI_RES, res=res.cuda())
        _assert_within(got, z + res.double(), mag, K, ("res", M, K, N))

        bias = torch.from_numpy(rng.standard_normal(N).astype(np.float32))
        p = 0.25
        scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
        keep = torch.from_numpy(O.dropout_keep_mask(5, 9, M * N, p)).view(M, N).double()
        ref = torch.relu(z + bias.double()) * keep * scale
        cp = _epi2(ops, o, M, N, K, EPI_ACT_PACK, bias=bias.cuda(), act=ops.ACT_RELU, drop=ops.Dropout(p, 5, 9), packed=True)
        val = _rows_value(cp, N)
        _assert_within(val, ref, mag + (_ulp32(z + bias.double()) / (2.0 * K * 2.0 ** -24)), K, ("act_pack", M, K, N), factor=scale)
        # a FULL image: the three planes are bl_pack_bf16x3 of the value they add up to
        assert torch.equal(cp, ops.pack_bf16x3(val.cuda())), ("act_pack planes", M, K, N)

        y = torch.relu(torch.from_numpy(rng.standard_normal((M, N)).astype(np.float32)))  # about half of the entries masked
        colsum = torch.zeros(N, device="cuda")
        ms = 1.25
        cp = _epi2(ops, o, M, N, K, EPI_MASK_PACK, y_packed=ops.pack_bf16x3(y.cuda()), mask_scale=ms, colsum=colsum, packed=True)
        ref = torch.where(y != 0, z * ms, torch.zeros_like(z))
        val = _rows_value(cp, N)
        _assert_within(val, ref, mag, K, ("mask_pack", M, K, N), factor=ms)
        assert torch.equal(cp, ops.pack_bf16x3(val.cuda())), ("mask_pack planes", M, K, N)
        # column sums of the fp32 results: their own fp32 summation (M terms, any order) on top
        want = val.double().sum(0)
        slack = M * 2.0 ** -24 * val.double().abs().sum(0) + _ulp32(want)
        assert bool(((colsum.cpu().double() - want).abs() <= slack).all()), ("colsum", M, K, N)


def test_wide_rows_match_fp64_of_the_high_planes(x1):
    """bl_gemm_rows_x6w in bf16x1 (128 x 256 tile, LDS-DMA of the high planes only): 127 and 257 rows, two K's, grouped with an
    empty group, gathered, routed."""
    ops, rng = x1, np.random.default_rng(3)
    N = 256
    for M in (127, 257):
        for K in (64, 192):
            o = _Operands(ops, rng, M, K, N, wide=True)
            ref, mag = o.product()
            _assert_within(ops.gemm_rows_x6(o.source(), o.image, M, N, wide=True), ref, mag, K, ("wide", M, K))
    o = _Operands(ops, rng, 257, 128, N, G=2, sizes=(0, 257), gather=True, wide=True)
    ref, mag = o.product()
    _assert_within(ops.gemm_rows_x6(o.source(), o.image, 257, N, group_ptr=o.d_ptr, G=2, wide=True), ref, mag, 128, "wide grouped + gathered")
    o = _Operands(ops, rng, 127, 64, 512, gather=True, wide=True)  # two column tiles
    bits = rng.integers(-2 ** 31, 2 ** 31, (127, 2)).astype(np.int32)
    bits[::5] = 0
    keep = torch.from_numpy(np.unpackbits(bits.view(np.uint8).reshape(127, -1), axis=1, bitorder="little").astype(np.float64))
    ref, mag = o.product(keep)
    _assert_within(ops.gemm_rows_x6(o.source(), o.image, 127, 512, win_bits=_dev(bits), wide=True), ref, mag, 64, "wide routed")


def test_weight_gradient_matches_fp64_of_the_high_planes(x1):
    """bl_gemm_wgrad_x6 in bf16x1: gw[g] += rows^T . G rows over groups of 1, 33 and 70 rows (the contraction length of the bound),
    direct and gathered on both sides, into a non-zero gw.  (The entry point takes no win_bits.)"""
    ops, rng = x1, np.random.default_rng(4)
    sizes = (1, 33, 70)
    M, G = sum(sizes), len(sizes)
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    for K in (32, 96):
        for N in (32, 96):
            for gather in (False, True):
                R = 50 if gather else M
                x = torch.from_numpy(rng.standard_normal((R, K)).astype(np.float32))
                gz = torch.from_numpy(rng.standard_normal((R, N)).astype(np.float32))
                xp, gp = ops.pack_bf16x3(x.cuda()), ops.pack_bf16x3(gz.cuda())
                ia = rng.integers(0, R, M).astype(np.int32) if gather else None
                ig = rng.integers(0, R, M).astype(np.int32) if gather else None
                A, Gr = _rows_plane(xp, K), _rows_plane(gp, N)
                if gather:
                    A, Gr = A[torch.from_numpy(ia.astype(np.int64))], Gr[torch.from_numpy(ig.astype(np.int64))]
                else:
                    A, Gr = A[:M], Gr[:M]
                gw0 = torch.from_numpy(rng.standard_normal((G, K, N)).astype(np.float32))
                gw = gw0.clone().cuda()
                ops.gemm_wgrad_x6([(xp, _dev(ia) if gather else None, K)], gp, M, N, gw, g_idx=_dev(ig) if gather else None,
                                  gw_group_stride=K * N, group_ptr=_dev(ptr), G=G)
                for g, rows in enumerate(sizes):
                    lo, hi = int(ptr[g]), int(ptr[g + 1])
                    ref = A[lo:hi].T @ Gr[lo:hi]
                    mag = A[lo:hi].abs().T @ Gr[lo:hi].abs()
                    # the tile is added to gw by one fp32 atomic per element: one more rounding, of the sum
                    got = gw[g].cpu().double()
                    bound = 2.0 * rows * 2.0 ** -24 * mag + _ulp32(ref) + _ulp32(ref + gw0[g].double())
                    assert bool(((got - (ref + gw0[g].double())).abs() <= bound).all()), (K, N, gather, rows)


# ---- 2. the mode is really on ---------------------------------------------------------------------------------------------
def test_one_term_differs_from_six_terms_and_switching_back_is_bit_exact(ops):
    rng = np.random.default_rng(5)
    M, K, N = 65, 96, 96
    o = _Operands(ops, rng, M, K, N)
    assert ops.seq_gemm_mode() == "bf16x6"
    six = ops.gemm_rows_x6(o.source(), o.image, M, N)
    assert ops.set_seq_gemm_mode("bf16x1") == "bf16x6"
    try:
        one = ops.gemm_rows_x6(o.source(), o.image, M, N)
    finally:
        assert ops.set_seq_gemm_mode("bf16x6") == "bf16x1"
    rel = ((one - six).abs() / six.abs().clamp_min(1e-30))
    assert float(rel.max()) > 1e-4, float(rel.max())
    assert torch.equal(ops.gemm_rows_x6(o.source(), o.image, M, N), six)
    lib = ops.load_library()  # any other mode code is refused and changes nothing
    assert lib.bl_set_seq_gemm_mode(2) == -1 and lib.bl_set_seq_gemm_mode(-1) == -1 and lib.bl_seq_gemm_mode() == 0  # BL_EINVAL, unchanged


# ---- 3. / 4. the GREAT layer ----------------------------------------------------------------------------------------------
def _layer_case(p, seed=1):
    from buglab.data.seqcollate import edge_csr
    from buglab.models.hip_ops import RelEdges
    from buglab.models.layers.relational_transformer import RelationalTransformerEncoderLayer

    B, L, H, dk, FF, T = 2, 24, 2, 32, 64, 3
    torch.manual_seed(seed)
    D = H * dk
    stack = torch.nn.ModuleList([RelationalTransformerEncoderLayer(D, dk, dk, H, T, dim_feedforward=FF, dropout=p) for _ in range(2)]).cuda().train()
    with torch.no_grad():
        for l in stack:
            l.norm1_g.add_(0.2 * torch.randn_like(l.norm1_g))
            l.norm1_b.add_(0.2 * torch.randn_like(l.norm1_b))
    rng = np.random.default_rng(0)
    lens_np = np.array([L, 17], dtype=np.int32)
    ne = 6 * B * L
    s_ = rng.integers(0, B, size=ne)
    e = np.stack([s_, (rng.random(ne) * lens_np[s_]).astype(np.int64), (rng.random(ne) * lens_np[s_]).astype(np.int64)], 1)
    rp, key, code = edge_csr(e, rng.integers(0, T, size=ne), B, L)
    edges = RelEdges(torch.from_numpy(rp).cuda(), torch.from_numpy(key).cuda(), torch.from_numpy(code).cuda(), int(key.shape[0]))
    x0 = torch.randn(B * L, D, device="cuda")
    w = torch.randn(B * L, D, device="cuda")
    return stack, torch.from_numpy(lens_np).cuda(), edges, x0, w, (B, L), p


def _run_stack(ops, case, fused, *, before_backward=None):
    stack, lens, edges, x0, w, (B, L), p = case
    was = ops.FUSED_GREAT_LAYER, ops.LINEAR_X6_MIN_ROWS
    ops.FUSED_GREAT_LAYER, ops.LINEAR_X6_MIN_ROWS = fused, 1  # (48 rows: the op-by-op Linears must take the packed-row path too)
    try:
        for q in stack.parameters():
            q.grad = None
        x = x0.clone().requires_grad_(True)
        assert stack[0].fused_call_ok(B, L) == fused
        y, chain = x, {}
        for i, l in enumerate(stack):
            y = l(y, lens, edges, B, L, dropout_seed=11 if p > 0 else None, dropout_stream=8 * (i + 1), chain=chain)
        if before_backward is not None:
            before_backward(y)
        (y * w).sum().backward()
        torch.cuda.synchronize()
        return y.detach().clone(), x.grad.clone(), {n: (q.grad.clone() if q.grad is not None else None) for n, q in stack.named_parameters()}
    finally:
        ops.FUSED_GREAT_LAYER, ops.LINEAR_X6_MIN_ROWS = was


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_one_call_layer_equals_the_op_by_op_path_in_bf16x1(x1, p):
    """bl_great_layer_fwd / _bwd follow the switch without new arguments: in bf16x1 they equal the op-by-op path in bf16x1, with
    the tolerances of test_seq_great_gpu.py::test_one_call_layer_equals_the_op_by_op_path -- and differ from the bf16x6 layer.

    In this mode an ulp in a Linear's input decides between two bf16 neighbours 2^-8 apart, so the two paths must normalise with
    the same kernel: hip_ops.add_layernorm takes the layer call's four-channels-per-lane LayerNorm while the mode is bf16x1 (with
    the other kernel, an ulp apart in half of the elements, two of eight dropout seeds differed by 1e-3 .. 4e-3 at p = 0.1 -- this
    case's seed among them).  Measured with it, three weight seeds x twelve dropout seeds: outputs and input gradients bit-equal,
    parameter gradients within 3e-7 (the order of their fp32 atomics)."""
    ops = x1
    case = _layer_case(p)
    y_f, gx_f, gp_f = _run_stack(ops, case, True)
    y_o, gx_o, gp_o = _run_stack(ops, case, False)
    close = lambda a, b, tol: float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))
    print("fused vs op-by-op, bf16x1: y", float((y_f - y_o).abs().max()), "g_x", float((gx_f - gx_o).abs().max()))
    assert close(y_f, y_o, 2e-5), float((y_f - y_o).abs().max())
    assert close(gx_f, gx_o, 5e-5), float((gx_f - gx_o).abs().max())
    for n in gp_o:
        if gp_o[n] is None:
            assert gp_f[n] is None or float(gp_f[n].abs().max()) == 0.0, n
            continue
        assert gp_f[n] is not None, n
        assert close(gp_f[n], gp_o[n], 5e-5), (n, float((gp_f[n] - gp_o[n]).abs().max()), float(gp_o[n].abs().max()))
    ops.set_seq_gemm_mode("bf16x6")
    try:
        y_6, _, _ = _run_stack(ops, case, True)
    finally:
        ops.set_seq_gemm_mode("bf16x1")
    assert float((y_f - y_6).abs().max()) > 1e-4  # the layer call really ran the one-term GEMMs


def test_layer_backward_checks_the_mode_of_its_saved_state(ops):
    """bl_great_layer_bwd refuses a `saved` written in the other mode (BL_EINVAL): provoked by telling the autograd node a wrong
    forward mode.  Left alone, the node runs its backward in the forward's mode whatever the switch says by then -- the one-call
    layer and the op-by-op Linears alike -- so a switch between the passes changes no gradient."""
    case = _layer_case(0.1)

    def lie(y):  # the last layer's node: claim the forward ran in the other mode
        assert y.grad_fn.seq_mode == 1
        y.grad_fn.seq_mode = 0

    prev = ops.set_seq_gemm_mode("bf16x1")
    try:
        with pytest.raises(RuntimeError, match="bl_great_layer_bwd.*sequence GEMM mode"):
            _run_stack(ops, case, True, before_backward=lie)
        assert ops.seq_gemm_mode() == "bf16x1"  # the scope around the failed call restored the mode
        for fused in (True, False):
            y_a, gx_a, gp_a = _run_stack(ops, case, fused)
            y_b, gx_b, gp_b = _run_stack(ops, case, fused, before_backward=lambda y: ops.set_seq_gemm_mode("bf16x6"))
            assert ops.seq_gemm_mode() == "bf16x6"  # the backward left the switch where the caller put it
            ops.set_seq_gemm_mode("bf16x1")
            assert torch.equal(y_a, y_b) and torch.equal(gx_a, gx_b), fused
            for n in gp_a:  # (weight gradients are summed by fp32 atomics: equal up to their order)
                if gp_a[n] is not None:
                    assert float((gp_a[n] - gp_b[n]).abs().max()) <= 1e-6 * max(1.0, float(gp_a[n].abs().max())), (fused, n)
    finally:
        ops.set_seq_gemm_mode(prev)


# ---- 5. accuracy against the reference layer ------------------------------------------------------------------------------
def _golden_great(ops):
    """the `great` fixture (reference RelationalTransformerEncoderLayer x 2, D = 64, L = 23) through the HIP layers ->
    (relative output error, worst relative gradient error, max abs output error) against the fixture's fp32 vectors; the two
    relative figures are the ones tests/golden/make_golden_seq_amp.py takes of the reference under bf16 autocast"""
    from buglab.data.seqcollate import edge_csr
    from buglab.models.hip_ops import RelEdges
    from buglab.models.layers.relational_transformer import RelationalTransformerEncoderLayer
    from tests.test_seq_great_gpu import PARAMS

    z = np.load(os.path.join(GOLD, "great_great.npz"))
    D, H, layers, FF, T, value_bias, scalar = (int(v) for v in z["cfg"])
    B, L0, _ = z["x"].shape
    L = (L0 + 3) // 4 * 4
    stack = torch.nn.ModuleList([
        RelationalTransformerEncoderLayer(D, D // H, D // H, H, T, dim_feedforward=FF, dropout=0.0, use_edge_value_biases=bool(value_bias),
                                          edge_attention_bias_is_scalar=bool(scalar), normalisation_mode=str(z["norm"]))
        for _ in range(layers)]).cuda()
    with torch.no_grad():
        for i, layer in enumerate(stack):
            for ours, (ref, how) in PARAMS.items():
                q = getattr(layer, ours, None)
                if q is not None:
                    v = z[f"p.{i}.{ref}"]
                    q.copy_(torch.from_numpy(np.ascontiguousarray(v.T if how == "T" else v)))
    x = torch.zeros(B, L, D)
    x[:, :L0] = torch.from_numpy(z["x"])
    x = x.cuda().requires_grad_(True)
    masked = np.ones((B, L), dtype=bool)
    masked[:, :L0] = z["masked"]
    lens = torch.from_numpy((~masked).sum(1).astype(np.int32)).cuda()
    rp, key, code = edge_csr(z["edges"], z["edge_types"], B, L)
    edges = RelEdges(torch.from_numpy(rp).cuda(), torch.from_numpy(key).cuda(), torch.from_numpy(code).cuda(), int(key.shape[0]))
    was = ops.LINEAR_X6_MIN_ROWS
    ops.LINEAR_X6_MIN_ROWS = 1  # (72 rows: the Linears must run on the packed-row GEMMs the switch governs)
    try:
        y, chain = x.view(B * L, D), {}
        for layer in stack:
            y = layer(y, lens, edges, B, L, chain=chain)
        y = y.view(B, L, D)
        w = torch.zeros(B, L, D)
        w[:, :L0] = torch.from_numpy(z["w"])
        (y * w.cuda() * torch.from_numpy(~masked).cuda()[:, :, None]).sum().backward()
        torch.cuda.synchronize()
    finally:
        ops.LINEAR_X6_MIN_ROWS = was
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
    ref_y = torch.zeros(B, L, D)
    ref_y[:, :L0] = torch.from_numpy(z["y"])
    m = torch.from_numpy(~masked)
    got_y = y.detach().cpu()
    errs = {"g_x": rel(x.grad.cpu()[:, :L0], torch.from_numpy(z["g_x"]))}
    for i, layer in enumerate(stack):
        for ours, (ref, how) in PARAMS.items():
            q = getattr(layer, ours, None)
            if q is None:
                continue
            want = torch.from_numpy(np.ascontiguousarray(z[f"g.{i}.{ref}"].T if how == "T" else z[f"g.{i}.{ref}"]))
            if float(want.norm()) > 0:
                errs[f"g.{i}.{ours}"] = rel(q.grad.cpu() if q.grad is not None else torch.zeros_like(want), want)
    return rel(got_y[m], ref_y[m]), max(errs.values()), float((got_y - ref_y)[m].abs().max())


def test_bf16x1_layer_is_as_accurate_as_the_reference_under_bf16_autocast(ops):
    """The limit is measured on the reference itself: tests/golden/seq_amp_autocast_error.json holds the relative output error and
    the worst relative gradient error of the reference's RelationalTransformerEncoderLayer stack under
    torch.autocast("cpu", torch.bfloat16) against its fp32 run on the `great` fixture (make_golden_seq_amp.py).  The bf16x1 HIP
    layers must stay within 4x of each (autocast also rounds intermediate results, this path does not: 4x covers accumulation-order
    differences without admitting a wrong plane -- the mid plane alone would be off by 100 %); bf16x6 keeps its 1e-4."""
    limit = json.load(open(os.path.join(GOLD, "seq_amp_autocast_error.json")))
    out6, grad6, abs6 = _golden_great(ops)
    assert abs6 < 1e-4 and out6 < 1e-4 and grad6 < 1e-4, (out6, grad6, abs6)
    prev = ops.set_seq_gemm_mode("bf16x1")
    try:
        out1, grad1, _ = _golden_great(ops)
    finally:
        ops.set_seq_gemm_mode(prev)
    print(f"bf16x1 against the fp32 reference: output {out1:.3e} (autocast {limit['output']:.3e}), "
          f"gradient {grad1:.3e} (autocast {limit['gradient']:.3e}); bf16x6: output {out6:.3e}, gradient {grad6:.3e}")
    assert out1 <= 4.0 * limit["output"], (out1, limit["output"])
    assert grad1 <= 4.0 * limit["gradient"], (grad1, limit["gradient"])
    assert out1 > 10.0 * out6  # reduced precision is visible


# ---- 6. training ------------------------------------------------------------------------------------------------------------
SPEC = {"modelName": "seq-great", "hidden_state_size": 64, "num_layers": 2, "num_heads": 2, "intermediate_dimension_size": 64, "dropout_rate": 0.1}


_STEPS = {}  # key -> [(loss of a training step, seq_gemm_mode() inside it)]


class _StepHook:
    """forward hook of the trained module (a top-level class: the trainer pickles the module, hooks included, at every checkpoint)"""

    def __init__(self, key):
        self.key = key

    def __call__(self, module, args, output):
        if module.training:
            from buglab.models import hip_ops

            _STEPS[self.key].append((output.detach(), hip_ops.seq_gemm_mode()))


def _train_curve(ops, tmp_path, enable_amp, caplog):
    from buglab.data.synthetic import make_buglab_seq_dataset
    from buglab.models.modelregistry import load_model
    from buglab.runtime.optim import FlatAdam
    from buglab.runtime.trainer import ModelTrainer

    data = make_buglab_seq_dataset(40, seed=7)
    model = load_model(dict(SPEC), tmp_path / f"m{int(enable_amp)}.pkl.gz")[0]
    trainer = ModelTrainer(model, tmp_path / f"m{int(enable_amp)}.pkl.gz", max_num_epochs=6, minibatch_size=8, enable_amp=enable_amp,
                           optimizer_creator=lambda params: FlatAdam(params, lr=1e-3, num_warmup_steps=0))
    key = f"amp={enable_amp}"
    _STEPS[key] = []
    # a hook on every training step: the module's forward in train mode
    trainer.register_training_start_hook(lambda model_, nn_, optimizer: nn_.register_forward_hook(_StepHook(key)))
    torch.manual_seed(0)
    np.random.seed(0)
    with caplog.at_level(logging.INFO, logger="buglab.runtime.trainer"):
        caplog.clear()
        trainer.train(copy.deepcopy(data), copy.deepcopy(data[:8]), show_progress_bar=False, parallelize=False, patience=100)
    log = "\n".join(r.getMessage() for r in caplog.records)
    steps = _STEPS.pop(key)
    return np.array([float(v) for v, _ in steps]), [m for _, m in steps], log


def test_trainer_amp_sets_the_sequence_mode_names_the_projections_and_trains(ops, tmp_path, caplog):
    """ModelTrainer(enable_amp=True) on a tiny seq-great (hidden 64, 2 layers, 2 heads, 40 synthetic samples, 30 steps): the INFO line
    names the projections (and not the message GEMMs, of which this model has none), the mode is bf16x1 inside every training step
    and bf16x6 again afterwards, and the loss curve follows the bf16x6 curve of the same seed within the band
    test_hip_parity.py::test_amp_mode_is_fp16_accurate_and_trains uses for f16x1 against f16x3: first loss within 2e-2, every step
    within 10 % + 0.03, and the loss comes down by 0.05 between the first and the last five steps."""
    before_msg = ops.msg_gemm_mode()
    a, modes_a, log_a = _train_curve(ops, tmp_path, False, caplog)
    b, modes_b, log_b = _train_curve(ops, tmp_path, True, caplog)
    assert ops.seq_gemm_mode() == "bf16x6" and ops.msg_gemm_mode() == before_msg
    assert len(a) == len(b) == 30, (len(a), len(b))
    assert set(modes_a) == {"bf16x6"} and set(modes_b) == {"bf16x1"}
    assert "--amp" not in log_a
    assert "--amp: QKV / output / feed-forward projections with bf16 operands" in log_b and "message GEMMs" not in log_b, log_b
    print("bf16x6 curve", np.round(a, 4).tolist())
    print("bf16x1 curve", np.round(b, 4).tolist())
    assert np.isfinite(b).all()
    assert abs(a[0] - b[0]) < 2e-2, (a[0], b[0])
    assert (np.abs(a - b) <= 0.10 * np.maximum(a, b) + 0.03).all(), (a, b)
    assert b[-5:].mean() < b[:5].mean() - 0.05, (b[:5], b[-5:])


def test_train_cli_with_amp_on_seq_great(ops, tmp_path):
    """`python -m buglab.models.train seq-great ... --amp` (reference train.py:8,106): trains, saves a checkpoint that restores, and
    leaves the process in the default modes."""
    from buglab.data.synthetic import make_buglab_seq_dataset
    from buglab.models import train
    from buglab.models.gnn import GnnBugLabModel
    from buglab.utils.msgpackutils import save_msgpack_l_gz

    data = make_buglab_seq_dataset(40, seed=9)
    (tmp_path / "train").mkdir()
    (tmp_path / "valid").mkdir()
    save_msgpack_l_gz(data[:32], tmp_path / "train" / "a.msgpack.l.gz")
    save_msgpack_l_gz(data[32:], tmp_path / "valid" / "v.msgpack.l.gz")
    model_path = tmp_path / "model.pkl.gz"
    before = ops.msg_gemm_mode()
    spec = {k: v for k, v in SPEC.items() if k != "modelName"}
    args = train.parse_args(["seq-great", str(tmp_path / "train"), str(tmp_path / "valid"), str(model_path), "--max-num-epochs", "2",
                             "--minibatch-size", "8", "--quiet", "--sequential", "--amp", "--model-spec", json.dumps(spec)])
    assert args["--amp"]
    train.run(args)
    assert ops.seq_gemm_mode() == "bf16x6" and ops.msg_gemm_mode() == before
    assert model_path.exists()
    _, nn_ = GnnBugLabModel.restore_model(model_path, torch.device("cuda"))
    assert all(bool(torch.isfinite(q).all()) for q in nn_.parameters())


# ---- 6. the fp16 counterpart: the one-term forms of the f16x3 entry points ------------------------------------------------
def _f16(bits: torch.Tensor) -> torch.Tensor:
    """int16 fp16 bit patterns -> fp64"""
    return bits.cpu().contiguous().view(torch.float16).double()


def _weights_h3_plane0(image: torch.Tensor, G: int, K: int, N: int) -> torch.Tensor:
    """high plane of bl_pack_weights_h3's image as fp64 [G, K, N], scale included (layout: csrc/bl_h3_image.h) -- per (group,
    128-column tile, 32-k stage): [i 2][plane 2][row_lo 64][k-group 4] x 8, column 64 i + row_lo"""
    nst, ntn = K // 32, (N + 127) // 128
    t = _f16(image).view(G, ntn, nst, 2, 2, 64, 4, 8)[:, :, :, :, 0]  # [G, tile, stage, i, row_lo, k-group, 8]
    return t.permute(0, 2, 5, 6, 1, 3, 4).reshape(G, K, ntn * 128)[:, :, :N]


@pytest.fixture()
def h1(ops):
    prev = ops.set_msg_gemm_mode("f16x1")
    try:
        yield ops
    finally:
        ops.set_msg_gemm_mode(prev)
    assert ops.msg_gemm_mode() == prev


def _keep_of(bits: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.unpackbits(bits.view(np.uint8).reshape(bits.shape[0], -1), axis=1, bitorder="little").astype(np.float64))


H3_SHAPES = [(M, K, N) for M in (1, 65, 129) for K in (32, 96) for N in (32, 96)]


def test_h3_rows_one_term_matches_fp64_of_the_high_planes(h1):
    """bl_gemm_rows_h3 in f16x1 against out_scale x the fp64 product of the decoded fp16 high planes (their scales are powers of
    two, so they are in the planes and leave through out_scale exactly): every (rows, K, N) of the grid; two groups with one of
    them empty on a gathered source; the routed form.  Products of two 11-bit significands are exact in fp32 and the accumulation
    is fp32: the bound is _assert_within's."""
    ops, rng = h1, np.random.default_rng(6)
    out_scale = 1.0 / (ops.H3_ROW_SCALE * ops.H3_W_SCALE)

    def case(M, K, N, *, sizes=None, gather=False, routed=False):
        G = len(sizes) if sizes else 1
        R = 37 if gather else max(M, 8)
        x = torch.from_numpy(rng.standard_normal((R, K)).astype(np.float32))
        W = torch.from_numpy((rng.standard_normal((G, K, N)) / math.sqrt(K)).astype(np.float32))
        xp, image = ops.pack_f16x2(x.cuda()), ops.pack_weights_h3(W.cuda(), True)
        idx = rng.integers(0, R, M).astype(np.int32) if gather else None
        A = _f16(xp[:, :K])
        A = A[torch.from_numpy(idx.astype(np.int64))] if gather else A[:M]
        bits = None
        if routed:
            bits = rng.integers(-2 ** 31, 2 ** 31, (M, K // 32)).astype(np.int32)
            bits[::7] = 0
            A = A * _keep_of(bits)
        B = _weights_h3_plane0(image, G, K, N)
        ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32) if sizes else np.array([0, M], dtype=np.int32)
        ref, mag = torch.zeros(M, N, dtype=torch.float64), torch.zeros(M, N, dtype=torch.float64)
        for g in range(G):
            lo, hi = int(ptr[g]), int(ptr[g + 1])
            ref[lo:hi] = (A[lo:hi] @ B[g]) * out_scale
            mag[lo:hi] = (A[lo:hi].abs() @ B[g].abs()) * out_scale
        got = ops.gemm_rows_h3([(xp, _dev(idx) if gather else None, K)], image, M, N, out_scale=out_scale,
                               group_ptr=_dev(ptr) if sizes else None, G=G, win_bits=_dev(bits) if routed else None)
        _assert_within(got, ref, mag, K, ("h3 rows", M, K, N, sizes, gather, routed))

    for M, K, N in H3_SHAPES:
        case(M, K, N)
    for sizes in ((0, 65), (129, 0)):
        case(sum(sizes), 96, 96, sizes=sizes, gather=True)
    for M, K, N in H3_SHAPES:
        case(M, K, N, gather=True, routed=True)


def test_h3_weight_gradient_one_term_matches_fp64_of_the_high_planes(h1):
    """bl_gemm_wgrad_h3 in f16x1: gw[g] = out_scale x rows^T . G rows over groups of 1, 65 and 129 rows (the contraction length of
    the bound), plain (direct rows) and routed (both sides gathered, the gradient rows masked by the winner bits), K and N in
    {32, 96} -- the smallest the argument checks admit.  gw starts at zero and every group is one chunk, so the flush adds no
    rounding of its own."""
    ops, rng = h1, np.random.default_rng(7)
    sizes = (1, 65, 129)
    M, G = sum(sizes), len(sizes)
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    g_scale = 1024.0
    out_scale = 1.0 / (ops.H3_ROW_SCALE * g_scale)
    for K in (32, 96):
        for N in (32, 96):
            for routed in (False, True):
                R = 50 if routed else M
                x = torch.from_numpy(rng.standard_normal((R, K)).astype(np.float32))
                gz = torch.from_numpy(rng.standard_normal((R, N)).astype(np.float32))
                xp, gp = ops.pack_f16x2(x.cuda()), ops.pack_f16x2(gz.cuda(), g_scale)
                A, Gr = _f16(xp[:, :K]), _f16(gp[:, :N])
                ia = ig = bits = None
                if routed:
                    ia, ig = rng.integers(0, R, M).astype(np.int32), rng.integers(0, R, M).astype(np.int32)
                    bits = rng.integers(-2 ** 31, 2 ** 31, (M, N // 32)).astype(np.int32)
                    bits[::7] = 0
                    A, Gr = A[torch.from_numpy(ia.astype(np.int64))], Gr[torch.from_numpy(ig.astype(np.int64))] * _keep_of(bits)
                gw = torch.zeros((G, K, N), device="cuda")
                ops.gemm_wgrad_h3([(xp, _dev(ia) if routed else None, K)], gp, M, N, gw, out_scale=out_scale, g_idx=_dev(ig) if routed else None,
                                  win_bits=_dev(bits) if routed else None, gw_group_stride=K * N, group_ptr=_dev(ptr), G=G)
                for g, rows in enumerate(sizes):
                    lo, hi = int(ptr[g]), int(ptr[g + 1])
                    ref = (A[lo:hi].T @ Gr[lo:hi]) * out_scale
                    mag = (A[lo:hi].abs().T @ Gr[lo:hi].abs()) * out_scale
                    _assert_within(gw[g], ref, mag, rows, ("h3 wgrad", K, N, routed, rows))
