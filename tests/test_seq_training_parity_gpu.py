"""GPU: the sequence models' TRAINING arithmetic -- dropout on, rezero, normalisation "off" -- on the HIP path against the float64
oracles that restate the library's counter-hash dropout (oracle/great_oracle.py, oracle/transformer_oracle.py, oracle/seq_oracle.py).
Outputs at the valid positions and EVERY gradient (input, all parameters including the edge-bias tables and the alphas); ragged
lengths with lens[0] = L, repeated edges, a hub row (tests/seq_parity_cases.py builds the cases, tests/test_seq_dropout_oracle_host.py
proves on the CPU that each of them would expose a wrong dropout site by >= 100 x the tolerance).

Tolerance: |got - want|_max <= 1e-4 * max(1, |want|_max) per tensor, the project's rule for these kernels against float64 at p = 0
(tests/test_seq_great_gpu.py).  Every p > 0 case runs next to its p = 0 twin on the same inputs and prints both maxima
(`pytest -s` shows them: "parity <case>: p=0 <err> (<tensor>) | p=<p> <err> (<tensor>)").

Observed maxima on an MI355X (worst tensor of each case in the tolerance's measure; p = 0 twin | p > 0), bound 1e-4:

  one-call layer      (2,64,2,96,3)      p=0 4.7e-07 | p=0.1 4.3e-07, p=0.3 4.2e-07, p=0.5 3.8e-07
                      (3,200,4,256,8)    p=0 6.0e-07 | p=0.1 5.7e-07, p=0.3 5.0e-07, p=0.5 4.5e-07
                      (2,512,8,1024,8)   p=0 9.4e-07 | p=0.1 7.0e-07, p=0.3 7.4e-07, p=0.5 5.8e-07
                      no edges           p=0 3.8e-07 | p=0.3 4.0e-07
  one-call layer off  (2,64,2,96,3)      p=0 6.7e-07 | p=0.1 6.1e-07, p=0.3 5.0e-07, p=0.5 4.9e-07
                      (3,200,4,256,8)    p=0 5.3e-07 | p=0.1 4.8e-07, p=0.3 4.7e-07, p=0.5 5.4e-07
  + row-wise attention (2,64,2,96,3)     p=0 6.0e-07 | p=0.1 4.8e-07, p=0.3 4.2e-07, p=0.5 4.3e-07
                      (3,200,4,256,8)    p=0 5.6e-07 | p=0.1 5.5e-07, p=0.3 6.0e-07, p=0.5 5.0e-07
  dk16 4.8e-07 | 5.7e-07     rat 3.9e-07 | 4.3e-07     scalar key bias 1.2e-06 | 1.9e-06     normoff 4.0e-07 | 4.7e-07      (p=0 | p=0.2)
  rezero scalar postnorm 1.7e-06 | 3.9e-07, prenorm 3.4e-06 | 6.2e-07; vector postnorm 4.0e-07 | 5.0e-07, prenorm 6.5e-07 | 4.6e-07
  transformer         (3,40,64,4,96,2) 3.9e-07 | 4.4e-07   (2,132,128,4,256,3) 5.6e-07 | 8.3e-07   (2,64,64,2,128,1) 2.6e-07 | 3.5e-07   (p=0 | p=0.1)
  models              seq-great 64/4 1.2e-07 | 7.0e-08, 64/2 7.1e-08 | 7.8e-08; seq-rat 1.1e-07 | 7.1e-08; seq-transformer 5.4e-08 | 1.0e-07;
                      var-misuse 3.0e-07 | 2.6e-07                                                                             (p=0 | p=0.1)
  negative control    stream shifted by one: 1.4e+00 (one-call shape), 2.3e+00 (dk16) -- unshifted 3.8e-07, 5.7e-07
No case exceeded the rule and no p > 0 error stands out from its p = 0 twin: the tests found no fault in the dropout sites.
"""
import numpy as np
import pytest
import torch

from tests import seq_parity_cases as C

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from buglab.models import hip_ops

    hip_ops.load_library()


def _edges(case):
    from buglab.data.seqcollate import edge_csr
    from buglab.models.hip_ops import RelEdges

    if case["kind"] != "relational":
        return None
    rp, key, code = edge_csr(case["edges"], case["types"], case["B"], case["L"])
    return RelEdges(torch.from_numpy(rp).cuda(), torch.from_numpy(key).cuda(), torch.from_numpy(code).cuda(), int(key.shape[0]))


def _hip_stack(case, p, seed=C.SEED, stream_shift=0):
    """the case's layers on the device, training mode -> the oracle's result dict"""
    B, L, D = case["B"], case["L"], case["D"]
    stack = case["stack"].cuda().train()
    for l in stack:
        l.dropout_rate = p
    for q in stack.parameters():
        q.grad = None
    lens = torch.from_numpy(case["lens"]).cuda()
    edges = _edges(case)
    x = case["x"].cuda().reshape(B * L, D).requires_grad_(True)
    y, chain = x, {}
    for i, l in enumerate(stack):
        y = l(y, lens, edges, B, L, dropout_seed=seed if p > 0 else None, dropout_stream=8 * (i + 1) + stream_shift, chain=chain)
    (y * case["w"].cuda().reshape(B * L, D)).sum().backward()
    torch.cuda.synchronize()
    valid = case["valid"]
    out = {"y": y.detach().cpu().view(B, L, D)[valid], "g.x": x.grad.cpu().view(B, L, D)[valid]}
    out.update({"g." + k: v for k, v in C.layer_tensors(stack, C.grad).items()})
    return out


def _check_pair(tag, hip, oracle, p):
    """p = 0 twin first, then p > 0, both printed before either is asserted"""
    e0, n0 = C.worst(hip(0.0), oracle(0.0))
    if p > 0:
        e1, n1 = C.worst(hip(p), oracle(p))
        print(f"\nparity {tag}: p=0 {e0:.3e} ({n0}) | p={p} {e1:.3e} ({n1})")
    else:
        print(f"\nparity {tag}: p=0 {e0:.3e} ({n0})")
    assert e0 <= C.TOLERANCE, (tag, "p=0", e0, n0)
    if p > 0:
        assert e1 <= C.TOLERANCE, (tag, p, e1, n1, "p=0 twin", e0)


def _stack_pair(tag, case, p):
    _check_pair(tag, lambda pd: _hip_stack(case, pd), lambda pd: C.oracle_stack(case, pd), p)


# ---- a. the one-call layer -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", C.FUSED_PS)
@pytest.mark.parametrize("shape", C.FUSED_SHAPES)
def test_one_call_layer_stack_with_dropout_matches_fp64(shape, p):
    case = C.relational_case(*shape, p=p)
    assert case["stack"][0].cuda().fused_call_ok(case["B"], case["L"])
    _stack_pair(f"one-call {shape}", case, p)


def test_one_call_layer_stack_without_edges_matches_fp64():
    case = C.relational_case(**C.NO_EDGES, p=0.3)
    assert case["stack"][0].cuda().fused_call_ok(case["B"], case["L"])
    _stack_pair("one-call no-edges", case, 0.3)


# ---- b. the same shapes on the op-by-op layer: with the one-kernel attention, and with the GEMM + row-wise attention kernels ----------
@pytest.mark.parametrize("p", C.FUSED_PS)
@pytest.mark.parametrize("shape", C.FUSED_SHAPES[:2])
@pytest.mark.parametrize("switches", [("FUSED_GREAT_LAYER",), ("FUSED_GREAT_LAYER", "FUSED_ATTENTION")], ids=lambda s: "+".join(s) + "=off")
def test_op_by_op_paths_of_the_one_call_shapes_match_fp64(switches, shape, p):
    """(the one-call layer does not look at FUSED_ATTENTION: the row-wise attention kernels are reached with both switches off)"""
    from buglab.models import hip_ops

    case = C.relational_case(*shape, p=p)
    before = {k: getattr(hip_ops, k) for k in switches}
    for k in switches:
        setattr(hip_ops, k, False)
    try:
        assert not case["stack"][0].cuda().fused_call_ok(case["B"], case["L"])
        _stack_pair(f"{'+'.join(switches)}=off {shape}", case, p)
    finally:
        for k, v in before.items():
            setattr(hip_ops, k, v)


# ---- c. configurations that always take the op-by-op path ------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.OP_BY_OP_CONFIGS))
def test_op_by_op_configurations_match_fp64(name):
    case = C.relational_case(**C.OP_BY_OP_CONFIGS[name], p=C.OP_BY_OP_P)
    assert not case["stack"][0].cuda().fused_call_ok(case["B"], case["L"])
    _stack_pair(name, case, C.OP_BY_OP_P)


# ---- d. layers/transformer.py -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L,D,H,FF,layers", C.TRANSFORMER_SHAPES)
def test_transformer_stack_with_dropout_matches_fp64(B, L, D, H, FF, layers):
    case = C.transformer_case(B, L, D, H, FF, layers)
    _stack_pair(f"transformer {(B, L, D, H, FF, layers)}", case, C.TRANSFORMER_P)


# ---- e. whole models -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model_name,hidden,heads", C.MODELS)
def test_seq_models_with_dropout_match_oracle(model_name, hidden, heads):
    """loss and all parameter gradients; the only place the encoder's streams 0 (embedder) and 1 (input dropout, dropout_rows) meet an
    independent reference."""
    from buglab.data.collate import to_device

    case = C.model_case(model_name, hidden, heads)
    nn_ = case["module"].cuda().train()
    mb = to_device(case["mb"], "cuda")

    def hip(p):
        for q in nn_.parameters():
            q.grad = None
        nn_.reset_metrics()
        nn_._gnn.dropout_rate = p  # (without a seed a training-mode module draws one of its own: the p = 0 twin sets the rates instead)
        for l in nn_._gnn.layers:
            l.dropout_rate = p
        loss = nn_(**mb, dropout_seed=C.MODEL_SEED)
        loss.backward()
        torch.cuda.synchronize()
        out = {"loss": loss.detach().cpu().double().reshape(1)}
        out.update({"g." + k: v for k, v in C.model_tensors(nn_, C.grad).items()})
        return out

    _check_pair(f"{model_name} {hidden}/{heads}", hip, lambda pd: C.oracle_model(case, pd), C.MODEL_P)


def test_varmisuse_model_with_dropout_matches_oracle():
    from tests.test_great_varmisuse_gpu import _edges_device

    case = C.varmisuse_case()
    m, B, L = case["module"].cuda().train(), case["B"], case["L"]
    n_ids = C.VARMISUSE["n_ids"]
    half = case["e_all"].shape[0] // 2
    edges, e_all, t_all = _edges_device(case["e_all"][:half], case["t_all"][:half], n_ids, B, L)
    assert np.array_equal(e_all, case["e_all"]) and np.array_equal(t_all, case["t_all"])

    def hip(p):
        for q in m.parameters():
            q.grad = None
        for l in m.seq_layers:
            l.dropout_rate = p
        m.reset_metrics()
        x = case["emb"].cuda().requires_grad_(True)
        loss = m.loss_from_embedded(x, B, L, case["lens_att"].cuda(), edges, case["err"].cuda(), case["cand"].cuda(), case["tgt"].cuda(),
                                    dropout_seed=C.VARMISUSE["seed"] if p > 0 else None)
        loss.backward()
        torch.cuda.synchronize()
        out = {"loss": loss.detach().cpu().double().reshape(1), "g.emb": x.grad.cpu()}
        out.update({"g." + k: v for k, v in C.varmisuse_tensors(m, C.grad).items()})
        return out

    _check_pair("var-misuse", hip, lambda pd: C.oracle_varmisuse(case, pd), C.VARMISUSE["p"])


# ---- f. hip_ops.dropout_rows -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("width", [8, 320])
def test_dropout_rows_equals_the_counter_hash_exactly(width, p):
    """forward and backward are x * keep * float32(1 / (1 - p)) bit for bit (the kernel's 1.0f / (1.0f - p) rounds to the same float
    for these p: asserted), 1001 rows -- not a multiple of any block size."""
    from buglab.models import hip_ops
    from oracle import buglab_oracle as O

    R, seed, stream = 1001, 21, 1
    torch.manual_seed(width)
    x = torch.randn(R, width)
    g = torch.randn(R, width)
    scale = np.float32(1.0 / (1.0 - p))
    assert scale == np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    keep = torch.from_numpy(O.dropout_keep_mask(seed, stream, R * width, p)).view(R, width) if p > 0 else torch.ones(R, width, dtype=torch.bool)
    xs = x.cuda().requires_grad_(True)
    y = hip_ops.dropout_rows(xs, hip_ops.Dropout(p, seed, stream))
    y.backward(g.cuda())
    torch.cuda.synchronize()
    zero = torch.zeros(())
    assert torch.equal(y.detach().cpu(), torch.where(keep, x * float(scale), zero))
    assert torch.equal(xs.grad.cpu(), torch.where(keep, g * float(scale), zero))
    if p > 0:
        assert abs(float(keep.float().mean()) - (1 - p)) < 0.01
        want = O.apply_dropout(x.double(), p, seed, stream)  # the oracle's own form, float64
        assert float((y.detach().cpu().double() - want).abs().max()) <= 1e-6 * float(want.abs().max())


# ---- g. negative control -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [C.FUSED_SHAPES[0], C.OP_BY_OP_CONFIGS["dk16"]])
def test_shifted_dropout_stream_fails_the_parity_bound_by_100x(shape):
    """The HIP layers drawing from `dropout_stream + 1` against the unshifted oracle: the discrepancy is at least 100 x the tolerance
    (the GPU-side twin of the host test's teeth: the comparison above is able to fail)."""
    case = C.relational_case(**shape, p=0.2) if isinstance(shape, dict) else C.relational_case(*shape, p=0.2)
    want = C.oracle_stack(case, 0.2)
    ok, _ = C.worst(_hip_stack(case, 0.2), want)
    shifted, name = C.worst(_hip_stack(case, 0.2, stream_shift=1), want)
    print(f"\nnegative control {shape}: unshifted {ok:.3e} | shifted stream {shifted:.3e} ({name})")
    assert ok <= C.TOLERANCE
    assert shifted >= C.TEETH * C.TOLERANCE, (shifted, name)
