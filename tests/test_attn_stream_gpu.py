"""GPU: the streaming (online-softmax) relational attention, csrc/bl_attn_stream.hip, against float64 and against the
stored-probability paths it stands next to.

Yardstick: a direct float64 restatement of the attention on the CPU (`_ref64` below; oracle/great_oracle.relational_attention
projects x -> qkv and the context -> output inside, so it cannot take a qkv matrix or return its gradient), with the oracle's own
counter-hash dropout masks (oracle.buglab_oracle.apply_dropout) and autograd for the gradients.  For each quantity (context, g_qkv,
g_bias_f, g_bias_r; valid rows only)   err(x) = max|x - x64| / max(1, max|x64|).

Bounds:
  * at L <= 1024 both paths are measured against the same float64 values: err_stream <= 4 * max(err_stored, 2^-23) -- the running
    rescale adds at most L / tile roundings per accumulator, a random walk over 16 tiles gives 4 -- and the two paths agree within
    the project's 2e-5 * scale (tests/test_seq_great_gpu.py);
  * beyond 1024 only the streaming path exists: err <= 4 * yard * (L / 1024), yard = the stored path's error at the (1, 1024, 2, 32,
    8, 0.1) case of this module clamped below by 2^-23 (the error of a length-L sum grows at most linearly).
Measured on MI355X (err_stream / max(err_stored, 2^-23), worst quantity): see DESIGN.md "Streaming relational attention"."""
import copy
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
QUANTITIES = ("context", "g_qkv", "g_bias_f", "g_bias_r")
TILE = 64  # keys per tile of the kernels (ST_BN)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from buglab.models import hip_ops

    hip_ops.load_library()
    was = hip_ops.STREAMING_ATTENTION
    yield
    hip_ops.STREAMING_ATTENTION = was


# ---- inputs: those of test_fused_attention_kernels_equal_the_gemm_and_rowwise_path ------------------------------------------------
def make_case(B, L, H, dk, T, p, no_csr=False, seed=None):
    from buglab.data.seqcollate import edge_csr

    rng = np.random.default_rng(L + dk if seed is None else seed)
    D = H * dk
    lens = rng.integers(max(1, L // 3), L + 1, B).astype(np.int32)
    lens[0] = L
    if B > 1:
        lens[1] = min(L, 37)  # ends inside the first key tile: every later tile of this sample is padding only
    ne = 6 * L
    e = np.stack([rng.integers(0, B, ne), rng.integers(0, L, ne), rng.integers(0, L, ne)], 1)
    e = e[(e[:, 1] < lens[e[:, 0]]) & (e[:, 2] < lens[e[:, 0]]) & (e[:, 1] != 3)]  # (position 3 has no outgoing entries)
    e = np.concatenate([e, e[:5]])  # repeated edges accumulate
    # a hub: position 7 of sample 0 takes part in 90 + 40 more edges (more than the 64 entries a wave holds per row)
    hub = np.stack([np.zeros(90, np.int64), np.full(90, 7), rng.integers(0, int(lens[0]), 90)], 1)
    e = np.concatenate([e, hub, hub[:, [0, 2, 1]][:40]])
    if no_csr:
        e = e[:0]
    kinds = rng.integers(0, T, e.shape[0])
    rp, key, code = edge_csr(e, kinds, B, L)
    g = torch.Generator().manual_seed(1000 + L + 7 * B)
    qkv = torch.randn(B * L, 3 * D, generator=g)
    bf, br = torch.randn(T, D, generator=g) * 0.3, torch.randn(T, D, generator=g) * 0.3
    w = torch.randn(B * L, D, generator=g)
    valid = (torch.arange(L)[None, :] < torch.from_numpy(lens).long()[:, None]).reshape(-1)
    return dict(B=B, L=L, H=H, dk=dk, T=T, p=p, lens=lens, rp=rp, key=key, code=code, qkv=qkv, bf=bf, br=br, w=w, valid=valid, seed=5, stream=2)


def _ref64(c):
    """float64 on the CPU: (context, g_qkv, g_bias_f, g_bias_r) at the valid rows, loss = sum(context[valid] * w[valid])"""
    from oracle.buglab_oracle import apply_dropout

    B, L, H, dk, T = (c[k] for k in ("B", "L", "H", "dk", "T"))
    qkv = c["qkv"].double().requires_grad_(True)
    bf, br = c["bf"].double().requires_grad_(True), c["br"].double().requires_grad_(True)
    t = qkv.view(B, L, H, 3, dk)
    q, k, v = t[:, :, :, 0] * dk ** -0.5, t[:, :, :, 1], t[:, :, :, 2]  # [B, L, H, dk]; multihead_attention.py:54
    scores = torch.einsum("bihd,bjhd->bijh", q, k)  # [B, query, key, H]
    if c["key"].shape[0]:
        rows = torch.from_numpy(np.repeat(np.arange(B * L), np.diff(c["rp"])))
        key, code = torch.from_numpy(c["key"]).long(), torch.from_numpy(c["code"]).long()
        b, i = rows // L, rows % L
        table = torch.stack([bf, br], 1).reshape(2 * T, H, dk)  # code = 2 t + direction
        term = (table[code] * q[b, i]).sum(-1)  # [n, H]   relational_multihead_attention.py:135-152
        scores = scores.contiguous().index_put((b, i, key), term, accumulate=True)
    lens = torch.from_numpy(c["lens"]).long()
    masked = torch.arange(L)[None, :] >= lens[:, None]  # [B, key]
    scores = scores.permute(0, 3, 1, 2).masked_fill(masked[:, None, None, :], -np.inf)  # [B, H, query, key]
    probs = torch.softmax(scores, dim=-1)
    probs = apply_dropout(probs.contiguous(), c["p"], c["seed"], c["stream"])  # mask element ((b H + h) L + i) L + j
    ctx = torch.einsum("bhij,bjhd->bihd", probs, v).reshape(B * L, H * dk)
    (ctx[c["valid"]] * c["w"].double()[c["valid"]]).sum().backward()
    zero = torch.zeros(T, H * dk, dtype=torch.float64)
    return (ctx.detach()[c["valid"]], qkv.grad[c["valid"]], bf.grad if bf.grad is not None else zero, br.grad if br.grad is not None else zero)


def run_gpu(c, switch, full=False):
    """the library on the case under STREAMING_ATTENTION = switch: the four quantities (float64, CPU), or with full=True the raw
    device tensors (context, lse or None, g_qkv) over all rows"""
    from buglab.models import hip_ops as ops

    B, L, H, dk, T = (c[k] for k in ("B", "L", "H", "dk", "T"))
    n = int(c["key"].shape[0])
    dev = "cuda"
    edges = ops.RelEdges(torch.from_numpy(c["rp"]).to(dev), torch.from_numpy(c["key"]).to(dev), torch.from_numpy(c["code"]).to(dev), n)
    lens = torch.from_numpy(c["lens"]).to(dev)
    qkv, bf, br = (c[k].to(dev).requires_grad_(True) for k in ("qkv", "bf", "br"))
    w, valid = c["w"].to(dev), c["valid"].to(dev)
    was = ops.STREAMING_ATTENTION
    ops.STREAMING_ATTENTION = switch
    try:
        want = ops.attention_path(L, dk, T)
        out = ops.rel_attention(qkv, lens, edges, bf, br, None, None, B, L, H, dk, T, drop=ops.Dropout(c["p"], c["seed"], c["stream"]))
        lse = out.grad_fn.saved[1].clone() if want == "stream" else None
        (out[valid] * w[valid]).sum().backward()
        torch.cuda.synchronize()
    finally:
        ops.STREAMING_ATTENTION = was
    if full:
        return want, out.detach(), lse, qkv.grad
    zero = torch.zeros(T, H * dk, dtype=torch.float64)
    g = lambda t: t.grad.detach().double().cpu() if t.grad is not None else zero
    return want, (out.detach()[valid].double().cpu(), qkv.grad[valid].double().cpu(), g(bf), g(br))


def errs(got, ref):
    return [float((a - b).abs().max()) / max(1.0, float(b.abs().max())) for a, b in zip(got, ref)]


@functools.lru_cache(maxsize=None)
def measured(shape):
    """(errors of the stored path, errors of the streaming path, path agreement / scale) per quantity for a shape of SHAPES"""
    B, L, H, dk, T, p = shape
    c = make_case(B, L, H, dk, T, max(p, 0.1) if p < 0 else p, no_csr=p < 0)
    ref = _ref64(c)
    path_s, stored = run_gpu(c, "0")
    path_t, stream = run_gpu(c, "1")
    assert path_s in ("fused", "rowwise") and path_t == "stream"
    agree = [float((a - b).abs().max()) / max(1.0, float(b.abs().max())) for a, b in zip(stream, stored)]
    return errs(stored, ref), errs(stream, ref), agree


def check_against_stored(name, e_stored, e_stream, agree):
    fails = []
    for qn, a, b, d in zip(QUANTITIES, e_stored, e_stream, agree):
        ratio = b / max(a, ULP)
        print(f"{name} {qn}: err_stored {a:.3e} err_stream {b:.3e} ratio {ratio:.2f} paths differ by {d:.3e} x scale")
        if not b <= 4.0 * max(a, ULP):
            fails.append(f"{qn}: err_stream {b:.3e} > 4 * max(err_stored {a:.3e}, 2^-23)")
        if not d < 2e-5:
            fails.append(f"{qn}: the two paths differ by {d:.3e} x scale (>= 2e-5)")
    assert not fails, (name, fails)


# ---- 1. both paths against float64 -------------------------------------------------------------------------------------------------
YARD_SHAPE = (1, 1024, 2, 32, 8, 0.1)
SHAPES = [(2, 64, 4, 32, 3, 0.0), (3, 200, 2, 32, 8, 0.2), (2, 68, 2, 32, 4, 0.3), (1, 512, 4, 32, 8, 0.1), (2, 72, 2, 32, 4, -0.1), YARD_SHAPE]


@pytest.mark.parametrize("shape", SHAPES)
def test_streaming_and_stored_paths_against_fp64(shape):
    """(p < 0: no CSR at all, dropout 0.1.)  L = 68 and 72 are no multiple of the key tile; (2, 64, ..) and (2, 68, ..) hold a sample of 37
    tokens, whose later key tiles are padding only."""
    e_stored, e_stream, agree = measured(shape)
    check_against_stored(str(shape), e_stored, e_stream, agree)


# ---- 2. beyond the old limit ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1028, 2, 32, 4, 0.1), (1, 1540, 2, 32, 8, 0.2)])
def test_beyond_1024_keys_against_fp64(shape):
    """`auto` (the default) picks the streaming kernels here; before them this call failed in the softmax launcher (L outside 1..1024)."""
    B, L, H, dk, T, p = shape
    yard = measured(YARD_SHAPE)[0]
    c = make_case(B, L, H, dk, T, p)
    path, got = run_gpu(c, "auto")
    assert path == "stream"
    fails = []
    for qn, e, y in zip(QUANTITIES, errs(got, _ref64(c)), yard):
        bound = 4.0 * max(y, ULP) * (L / 1024.0)
        print(f"{shape} {qn}: err {e:.3e} bound {bound:.3e} (yard {y:.3e})")
        if not e <= bound:
            fails.append(f"{qn}: {e:.3e} > {bound:.3e}")
    assert not fails, fails


# ---- 3. forced rescale -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["key-second-tile", "key-last-tile", "edge-second-tile", "edge-last-tile"])
def test_a_late_tile_carries_the_row_maximum(where):
    """One query row whose largest score, by more than 60, sits in the second or in the last key tile: every accumulator of the row is
    rescaled by e^-60 or less when that tile arrives.  Once through a key row, once through an edge term (a bias row that only this
    entry uses)."""
    B, L, H, dk, T, p = 2, 256, 2, 32, 4, 0.1
    c = make_case(B, L, H, dk, T, p, seed=77)
    i_star, j_star = 10, (TILE + 6 if where.endswith("second-tile") else L - 3)
    scale = dk ** -0.5
    t = c["qkv"].view(B, L, H, 3, dk)
    if where.startswith("key"):
        for h in range(H):
            q = t[0, i_star, h, 0] * scale
            t[0, j_star, h, 1] = 80.0 * q / float(q @ q)  # q_i . k_j = 80
    else:
        # type T - 1 forward is used by this entry alone: (sample 0, source i*, target j*) -> query row i*, key j*, code 2 (T - 1)
        from buglab.data.seqcollate import edge_csr

        rows = np.repeat(np.arange(B * L), np.diff(c["rp"]))
        fwd = c["code"] % 2 == 0
        e = np.stack([rows[fwd] // L, rows[fwd] % L, c["key"][fwd]], 1)
        kinds = np.minimum(c["code"][fwd] // 2, T - 2)
        e, kinds = np.concatenate([e, [[0, i_star, j_star]]]), np.concatenate([kinds, [T - 1]])
        c["rp"], c["key"], c["code"] = edge_csr(e, kinds, B, L)
        for h in range(H):
            q = t[0, i_star, h, 0] * scale
            c["bf"][T - 1, h * dk:(h + 1) * dk] = 80.0 * q / float(q @ q)  # <q_i, bias> = 80
    # the condition itself, in float64
    q64, k64 = t[0, i_star, :, 0].double() * scale, t[0, :, :, 1].double()
    s = torch.einsum("hd,jhd->hj", q64, k64)
    rows = np.repeat(np.arange(B * L), np.diff(c["rp"]))
    table = torch.stack([c["bf"], c["br"]], 1).reshape(2 * T, H, dk).double()
    for key, code in zip(c["key"][rows == i_star], c["code"][rows == i_star]):
        s[:, key] += (table[code] * q64).sum(-1)
    assert bool((s[:, j_star] - s[:, :j_star].max(dim=1).values > 60.0).all()) and j_star // TILE >= 1
    ref = _ref64(c)
    _, stored = run_gpu(c, "0")
    _, stream = run_gpu(c, "1")
    agree = [float((a - b).abs().max()) / max(1.0, float(b.abs().max())) for a, b in zip(stream, stored)]
    path, out, lse, g_qkv = run_gpu(c, "1", full=True)
    assert path == "stream"
    for name, x in (("context", out), ("lse", lse), ("g_qkv", g_qkv)):  # padded rows included
        assert bool(torch.isfinite(x).all()), name
    check_against_stored(where, errs(stored, ref), errs(stream, ref), agree)


# ---- 4. reproducibility, padding, the derivative with dropout on ---------------------------------------------------------------------
def test_reproducible_and_padding_never_reaches_valid_rows():
    B, L, H, dk, T, p = 3, 200, 2, 32, 8, 0.2
    D = H * dk
    c = make_case(B, L, H, dk, T, p)
    path, out1, lse1, g1 = run_gpu(c, "1", full=True)
    _, out2, lse2, g2 = run_gpu(c, "1", full=True)
    assert path == "stream"
    assert torch.equal(out1, out2) and torch.equal(lse1, lse2) and torch.equal(g1, g2)  # no float atomics on ctx, dQ, dK, dV
    assert bool(torch.isfinite(out1).all()) and bool(torch.isfinite(lse1).all()) and bool(torch.isfinite(g1).all())  # padded query rows too
    # +50 on the padded positions of sample 1 (37 tokens): its valid rows move by rounding at most, the other samples not at all
    n1 = int(c["lens"][1])
    c2 = dict(c, qkv=c["qkv"].clone())
    c2["qkv"].view(B, L, 3 * D)[1, n1:] += 50.0
    _, out3, _, _ = run_gpu(c2, "1", full=True)
    a, b = out1.view(B, L, D), out3.view(B, L, D)
    assert float((a[1, :n1] - b[1, :n1]).abs().max()) < 1e-4
    assert float((a[0] - b[0]).abs().max()) == 0.0 and float((a[2] - b[2]).abs().max()) == 0.0
    # the upstream gradient of padded query rows is zero and stays zero through dS: they leave no trace in dK / dV, and dQ there is 0
    gq = g1.view(B, L, H, 3, dk)
    assert float(gq[1, n1:].abs().max()) == 0.0


def test_directional_derivative_with_dropout_on():
    B, L, H, dk, T, p = 2, 136, 2, 32, 4, 0.25
    c = make_case(B, L, H, dk, T, p)
    _, _, _, g = run_gpu(c, "1", full=True)
    g = g.cpu()
    d = g / g.norm()  # along the gradient: the derivative is |grad|, well above the fp32 noise of the difference
    eps = 1e-3
    valid, w = c["valid"], c["w"]

    def f(qkv):
        _, out, _, _ = run_gpu(dict(c, qkv=qkv), "1", full=True)
        return float((out.cpu().double()[valid] * w.double()[valid]).sum())

    num = (f(c["qkv"] + eps * d) - f(c["qkv"] - eps * d)) / (2 * eps)
    ana = float((g.double() * d.double()).sum())
    assert abs(num - ana) <= 5e-2 * abs(ana), (num, ana)


# ---- 5. memory -------------------------------------------------------------------------------------------------------------------------
def test_no_score_matrix_is_allocated():
    from buglab.models import hip_ops as ops

    B, L, H, dk, T, p = 2, 1024, 4, 32, 4, 0.1
    c = make_case(B, L, H, dk, T, p)
    one_matrix = B * H * L * L * 4
    dev = "cuda"
    edges = ops.RelEdges(torch.from_numpy(c["rp"]).to(dev), torch.from_numpy(c["key"]).to(dev), torch.from_numpy(c["code"]).to(dev),
                         int(c["key"].shape[0]))
    lens, w = torch.from_numpy(c["lens"]).to(dev), c["w"].to(dev)
    peaks = {}
    was = ops.STREAMING_ATTENTION
    try:
        for switch in ("1", "0"):
            ops.STREAMING_ATTENTION = switch
            qkv, bf, br = (c[k].to(dev).requires_grad_(True) for k in ("qkv", "bf", "br"))
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            out = ops.rel_attention(qkv, lens, edges, bf, br, None, None, B, L, H, dk, T, drop=ops.Dropout(p, 5, 2))
            (out * w).sum().backward()
            torch.cuda.synchronize()
            peaks[switch] = torch.cuda.max_memory_allocated() - base
            del out, qkv, bf, br
    finally:
        ops.STREAMING_ATTENTION = was
    print(f"peak allocation over forward + backward: streaming {peaks['1']} B, stored {peaks['0']} B, one score matrix {one_matrix} B")
    assert peaks["1"] < one_matrix
    assert peaks["0"] > 2 * one_matrix


# ---- 6. end to end through the registry --------------------------------------------------------------------------------------------------
def _long_dataset():
    """two of test_seq_model_end_to_end_matches_oracle's synthetic samples and one of 1100 - 1300 tokens"""
    from buglab.data.synthetic import make_buglab_seq_datapoint, make_buglab_seq_dataset

    data = make_buglab_seq_dataset(2, seed=5)
    data.append(make_buglab_seq_datapoint(np.random.default_rng(9), num_statements=225, buggy=True))
    return data


def _model_case(model_name):
    from pathlib import Path

    from buglab.models.modelregistry import load_model
    from oracle import great_oracle as G

    data = _long_dataset()
    model = load_model({"modelName": model_name, "hidden_state_size": 64, "num_heads": 2, "num_layers": 2, "intermediate_dimension_size": 96,
                        "max_seq_size": 1536, "dropout_rate": 0.0}, Path("/tmp/_bl_stream_e2e.pkl.gz"))[0]
    model.compute_metadata(copy.deepcopy(data))
    torch.manual_seed(0)
    module = model.build_neural_module().train()
    samples = [model.tensorize(copy.deepcopy(d)) for d in data]
    assert all(s is not None for s in samples)
    assert 1100 <= samples[2].base.graph_data.num_nodes <= 1300
    mb_np = model.collate_minibatch({"samples": samples})
    cfg = G.GreatConfig(d_model=64, num_heads=2, num_layers=2, dim_feedforward=96, num_edge_types=max(1, len(model.edge_types)),
                        use_edge_value_biases=model_name == "seq-rat")
    return dict(model=model, module=module, mb=mb_np, cfg=cfg, data=data, layer_type="transformer" if model_name == "seq-transformer" else "great")


@pytest.mark.parametrize("model_name", ["seq-great", "seq-transformer"])
def test_a_model_with_a_long_sample_matches_the_oracle(model_name):
    """One training step's loss and gradients against oracle/seq_oracle.py at test_seq_model_end_to_end_matches_oracle's tolerances, and
    predict() on the long sample.  The layers take the op-by-op path (bl_great_layer_ok says no beyond 1024) with the streaming attention."""
    from buglab.data.collate import to_device
    from buglab.models import hip_ops as ops
    from tests import seq_parity_cases as S

    case = _model_case(model_name)
    L = int(case["mb"]["graph_data"]["seq_len"])
    assert 1100 <= L <= 1300 and ops.attention_path(L, 32, case["cfg"].num_edge_types if case["layer_type"] == "great" else 1) == "stream"
    want = S.oracle_model(case, 0.0)
    nn_ = case["module"].cuda().train()
    nn_.reset_metrics()
    loss = nn_(**to_device(case["mb"], "cuda"))
    loss.backward()
    torch.cuda.synchronize()
    assert abs(float(loss.detach()) - float(want["loss"])) < 1e-4, (float(loss.detach()), float(want["loss"]))
    got = S.model_tensors(nn_, S.grad)
    assert set("g." + k for k in got) == set(want) - {"loss"}
    for k, g in got.items():
        w = want["g." + k]
        assert float((g - w).abs().max()) <= 1e-4 * float(w.abs().max()) + 1e-6, k
    res = list(case["model"].predict(iter(copy.deepcopy(case["data"])), nn_, "cuda", parallelize=False))
    assert len(res) == len(case["data"])
    point, loc, rewrites = max(res, key=lambda r: len(r[0]["graph"]["nodes"]))  # the long sample
    assert len(point["graph"]["nodes"]) > 1100 and len(rewrites) == len(point["candidate_rewrites"]) and -1 in loc
    assert abs(sum(np.exp(v) for v in loc.values()) - 1.0) < 1e-4


def test_seq_rat_beyond_1024_is_refused_before_any_launch():
    """(raised by attention_path in the first layer's attention, from Python: no attention kernel has been launched)"""
    from buglab.data.collate import to_device

    case = _model_case("seq-rat")
    nn_ = case["module"].cuda().train()
    mb = to_device(case["mb"], "cuda")
    with pytest.raises(ValueError) as ei:
        nn_(**mb)
    msg = str(ei.value)
    assert f"L={int(case['mb']['graph_data']['seq_len'])}" in msg and "1024" in msg and "value biases" in msg
