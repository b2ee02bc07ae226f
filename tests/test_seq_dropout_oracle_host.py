"""CPU: the float64 oracles of the sequence models with the library's dropout, rezero and normalisation "off"
(oracle/great_oracle.py, oracle/transformer_oracle.py, oracle/seq_oracle.py) -- their own properties, before any kernel is compared
with them (tests/test_seq_training_parity_gpu.py):

  * p = 0 / seed = None is bit-identical to the call form that knew no dropout;
  * the transformer restatement against torch.nn.TransformerEncoderLayer(...).double() itself at p = 0: outputs and all gradients
    within 1e-10 (float64 on both sides: the two differ in summation order only, ~1e-16 relative per operation);
  * TEETH: for every case of the GPU tests and every dropout site, the oracle with that one site altered -- drawing from the next
    stream, or without the 1 / (1 - p) factor -- differs from the oracle by at least 100 x the GPU tests' tolerance, in the output or
    a gradient, in the tolerance's own measure.  This is a condition on the chosen inputs: a kernel that is wrong at one site cannot
    hide inside the tolerance.  The same for the value-bias convention of "rat" (dropped vs. undropped probabilities).
"""
import numpy as np
import pytest
import torch

from oracle import buglab_oracle as O
from oracle import great_oracle as G
from oracle import transformer_oracle as TO
from tests import seq_parity_cases as C

NEED = C.TEETH * C.TOLERANCE


def _assert_teeth(evaluate, p, alterations):
    base = evaluate(p, None)
    for alter in alterations:
        d = C.discrepancy(evaluate(p, alter), base)
        assert d >= NEED, (alter, d, NEED)


def test_dropout_off_is_bit_identical_to_the_old_call_form():
    case = C.relational_case(2, 24, 2, 48, 3, dk=16, value_bias=True, norm="prenorm", seed=3)
    p = C.layer_tensors(case["stack"], C.value)
    x, masked = case["x"].double(), ~case["valid"]
    e, t = torch.from_numpy(case["edges"]), torch.from_numpy(case["types"])
    old = G.encoder_stack(p, x, masked, e, t, case["cfg"])
    assert torch.equal(old, G.encoder_stack(p, x, masked, e, t, case["cfg"], p_drop=0.0, seed=5))
    assert torch.equal(old, G.encoder_stack(p, x, masked, e, t, case["cfg"], p_drop=0.3, seed=None))
    assert not torch.equal(old, G.encoder_stack(p, x, masked, e, t, case["cfg"], p_drop=0.3, seed=5))
    a = G.relational_attention(p, "layers.0.", x, masked, e, t, case["cfg"])
    assert torch.equal(a, G.relational_attention(p, "layers.0.", x, masked, e, t, case["cfg"], p_drop=0.0, seed=1, stream=8))
    l = G.encoder_layer(p, "layers.0.", x, masked, e, t, case["cfg"])
    assert torch.equal(l, G.encoder_layer(p, "layers.0.", x, masked, e, t, case["cfg"], p_drop=0.5, seed=None, stream=8))
    mc = C.model_case("seq-great", 64, 4)
    pm = C.model_tensors(mc["module"], C.value)
    from oracle import seq_oracle as SO

    old = SO.forward_loss(pm, mc["mb"], mc["cfg"])["loss"]
    assert torch.equal(old, SO.forward_loss(pm, mc["mb"], mc["cfg"], p_drop=0.0, seed=3)["loss"])
    assert torch.equal(old, SO.forward_loss(pm, mc["mb"], mc["cfg"], p_drop=0.1, seed=None)["loss"])
    assert not torch.equal(old, SO.forward_loss(pm, mc["mb"], mc["cfg"], p_drop=0.1, seed=3)["loss"])


def test_dropout_sites_use_the_documented_layouts():
    """One layer, by hand: the probabilities' mask is indexed [B * H * L, L] with row (b * H + h) * L + q, the row sites [B * L, N]."""
    case = C.relational_case(2, 12, 2, 24, 2, dk=8, layers=1, seed=4)
    p = C.layer_tensors(case["stack"], C.value)
    cfg, x, masked = case["cfg"], case["x"].double(), ~case["valid"]
    e, t = torch.from_numpy(case["edges"]), torch.from_numpy(case["types"])
    B, L, H, dk = 2, 12, 2, 8
    pd, seed, stream = 0.3, 9, 16
    # rebuild the attention output from the undropped probabilities and the documented mask
    qkv = (x @ p["layers.0.self_attn._selfatt_head_transforms.weight"].T).reshape(B, L, H, 3 * dk)
    v = qkv[..., 2 * dk:]
    keep = torch.from_numpy(O.dropout_keep_mask(seed, stream, B * H * L * L, pd)).view(B, H, L, L)  # [b, h, q, k]
    got = G.relational_attention(p, "layers.0.", x, masked, e, t, cfg, p_drop=pd, seed=seed, stream=stream)
    q, kk = qkv[..., :dk] * dk ** -0.5, qkv[..., dk:2 * dk]
    scores = torch.einsum("bkhd,bqhd->bqkh", kk, q)
    s, src, tgt = e[:, 0], e[:, 1], e[:, 2]
    bf = p["layers.0.self_attn._edge_attention_biases.weight"][t].reshape(-1, H, dk)
    br = p["layers.0.self_attn._reverse_edge_attention_biases.weight"][t].reshape(-1, H, dk)
    scores = scores.contiguous().index_put((torch.cat([s, s]), torch.cat([src, tgt]), torch.cat([tgt, src])),
                                           torch.cat([(bf * q[s, src]).sum(-1), (br * q[s, tgt]).sum(-1)]), accumulate=True)
    scores = scores.permute(0, 3, 1, 2).masked_fill(masked[:, None, None, :], -np.inf)  # [b, h, q, k]
    probs = torch.softmax(scores, -1) * keep / (1.0 - pd)
    ctx = torch.einsum("bhqk,bkhd->bqhd", probs, v).reshape(B, L, H * dk)
    want = ctx @ p["layers.0.self_attn._out_proj.weight"].T
    assert float((got - want).abs().max()) < 1e-12
    # a row site: feed-forward output, [B * L, D]
    y3 = G.encoder_layer(p, "layers.0.", x, masked, e, t, cfg, p_drop=pd, seed=seed, stream=stream, _alter=None)
    assert y3.shape == x.shape and torch.isfinite(y3).all()
    flat = torch.arange(B * L * cfg.d_model, dtype=torch.float64).view(B, L, cfg.d_model)
    k1 = torch.from_numpy(O.dropout_keep_mask(seed, stream + 1, flat.numel(), pd)).view(B * L, cfg.d_model)
    assert torch.equal(G._site(flat, 1, pd, seed, stream, None).view(B * L, -1) != 0, k1 & (flat.view(B * L, -1) != 0))


@pytest.mark.parametrize("B,L,D,H,FF,layers", C.TRANSFORMER_SHAPES)
def test_transformer_restatement_matches_torch_in_float64(B, L, D, H, FF, layers):
    case = C.transformer_case(B, L, D, H, FF, layers)
    valid, w = case["valid"], case["w"].double()
    xr = case["x"].double().requires_grad_(True)
    h = xr
    for l in case["torch"]:  # reference seqmodel.py:380-384 -- [L, B, D] in, src_key_padding_mask = padding positions
        h = l(h.transpose(0, 1), src_key_padding_mask=~valid).transpose(0, 1)
    (h * w).sum().backward()
    # the oracle's parameters arrive through the HIP layer's own layout maps (fp32 copies of exactly representable values)
    p = C.leaves(C.layer_tensors(case["stack"], C.value))
    x = case["x"].double().requires_grad_(True)
    y = TO.encoder_stack(p, x, ~valid, layers, H)
    (y * w).sum().backward()
    assert float((y - h).detach()[valid].abs().max()) <= 1e-10
    assert float((x.grad - xr.grad)[valid].abs().max()) <= 1e-10 * max(1.0, float(xr.grad.abs().max()))
    for i, l in enumerate(case["torch"]):
        for name, q in l.named_parameters():
            got = p[f"layers.{i}.{name}"]
            assert torch.equal(got.detach(), q.detach()), name
            assert float((got.grad - q.grad).abs().max()) <= 1e-10 * max(1.0, float(q.grad.abs().max())), (i, name)
    assert torch.equal(y, TO.encoder_stack(p, x, ~valid, layers, H, p_drop=0.0, seed=4))


# ---- teeth -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", C.FUSED_PS)
@pytest.mark.parametrize("shape", C.FUSED_SHAPES)
def test_teeth_relational_stack_one_call_shapes(shape, p):
    case = C.relational_case(*shape, p=p)
    _assert_teeth(lambda pd, alter: C.oracle_stack(case, pd, alter=alter), p, C.LAYER_ALTERATIONS)


def test_teeth_relational_stack_without_edges():
    case = C.relational_case(**C.NO_EDGES, p=0.3)
    _assert_teeth(lambda pd, alter: C.oracle_stack(case, pd, alter=alter), 0.3, C.LAYER_ALTERATIONS)


@pytest.mark.parametrize("name", list(C.OP_BY_OP_CONFIGS))
def test_teeth_relational_stack_op_by_op_configurations(name):
    case = C.relational_case(**C.OP_BY_OP_CONFIGS[name], p=C.OP_BY_OP_P)
    alterations = C.LAYER_ALTERATIONS + ([(0, "vb_undropped")] if name == "rat" else [])  # (rat: which probabilities the value biases read)
    _assert_teeth(lambda pd, alter: C.oracle_stack(case, pd, alter=alter), C.OP_BY_OP_P, alterations)


@pytest.mark.parametrize("B,L,D,H,FF,layers", C.TRANSFORMER_SHAPES)
def test_teeth_transformer_stack(B, L, D, H, FF, layers):
    case = C.transformer_case(B, L, D, H, FF, layers)
    _assert_teeth(lambda pd, alter: C.oracle_stack(case, pd, alter=alter), C.TRANSFORMER_P, C.LAYER_ALTERATIONS)


@pytest.mark.parametrize("model_name,hidden,heads", C.MODELS)
def test_teeth_whole_models(model_name, hidden, heads):
    case = C.model_case(model_name, hidden, heads)
    alterations = C.ENCODER_ALTERATIONS + C.LAYER_ALTERATIONS + ([(0, "vb_undropped")] if model_name == "seq-rat" else [])
    _assert_teeth(lambda pd, alter: C.oracle_model(case, pd, alter=alter), C.MODEL_P, alterations)


def test_teeth_varmisuse_model():
    case = C.varmisuse_case()
    _assert_teeth(lambda pd, alter: C.oracle_varmisuse(case, pd, alter=alter), C.VARMISUSE["p"], C.LAYER_ALTERATIONS)
