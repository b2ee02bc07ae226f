"""Cases shared by tests/test_seq_dropout_oracle_host.py (CPU: the oracles' own properties and the "teeth" conditions) and
tests/test_seq_training_parity_gpu.py (GPU: the HIP sequence layers and models against the float64 oracles, dropout ON).

A case is built on the CPU from seeds: the library's own modules (plain nn.Module parameter holders until `forward`), inputs, ragged
lengths with lens[0] = L, repeated edges and a hub row.  The host test evaluates only the oracle on it; the GPU test moves the very
same modules to the device.  Nothing here looks at a kernel's output.

TOLERANCE = 1e-4: |got - want|_max <= 1e-4 * max(1, |want|_max) for outputs and each gradient -- the project's rule for these kernels
against float64 at p = 0 (tests/test_seq_great_gpu.py).  A dropout site adds one multiplication by an exact 0/1 mask and one
fp32-rounded constant (relative 6e-8) and no other rounding, so the rule carries over to p > 0 unchanged.
TEETH = 100: a wrong site must move the oracle by at least TEETH * TOLERANCE in the same measure (a condition on the inputs)."""
import copy
import math
from pathlib import Path

import numpy as np
import torch

from oracle import great_oracle as G
from oracle import seq_oracle as SO
from oracle import transformer_oracle as TO

TOLERANCE = 1e-4
TEETH = 100.0
SEED = 11  # dropout seed of the stack cases

# ours -> (reference state_dict name, transposed?)
ENC = {"qkv_W": ("self_attn._selfatt_head_transforms.weight", True), "out_W": ("self_attn._out_proj.weight", True),
       "edge_bias_f": ("self_attn._edge_attention_biases.weight", False), "edge_bias_r": ("self_attn._reverse_edge_attention_biases.weight", False),
       "edge_vbias_f": ("self_attn._edge_value_biases.weight", False), "edge_vbias_r": ("self_attn._reverse_edge_value_biases.weight", False),
       "lin1_W": ("linear1.weight", True), "lin1_b": ("linear1.bias", False), "lin2_W": ("linear2.weight", True), "lin2_b": ("linear2.bias", False),
       "norm1_g": ("norm1.weight", False), "norm1_b": ("norm1.bias", False), "norm2_g": ("norm2.weight", False), "norm2_b": ("norm2.bias", False),
       "alpha1": ("_alpha1", False), "alpha2": ("_alpha2", False)}
HEADS = {"_localization_module.": "loc.", "_text_repair_module.": "text.", "_varmisuse_module.": "var.", "_argswap_module.": "swap."}

# (B, L, H, FF, T), head dimension 32: the one-call layer's shapes; the last is the shipped size
FUSED_SHAPES = [(2, 64, 2, 96, 3), (3, 200, 4, 256, 8), (2, 512, 8, 1024, 8)]
FUSED_PS = [0.1, 0.3, 0.5]  # 0.3: float32(p) * 2^24 is not an integer; 0.5: the scale is exactly 2
NO_EDGES = dict(B=2, L=96, H=2, FF=64, T=4, edges_on=False)
# configurations that always take the op-by-op path, each at p = 0 and p = 0.2
OP_BY_OP_P = 0.2
OP_BY_OP_CONFIGS = {
    "dk16": dict(B=2, L=96, H=4, FF=96, T=5, dk=16),
    "rat": dict(B=2, L=64, H=2, FF=96, T=3, value_bias=True, norm="prenorm"),
    "scalar_key_bias": dict(B=2, L=64, H=2, FF=96, T=3, scalar=True),
    "rezero_scalar_postnorm": dict(B=2, L=64, H=2, FF=96, T=3, rezero="scalar"),
    "rezero_scalar_prenorm": dict(B=2, L=64, H=2, FF=96, T=3, rezero="scalar", norm="prenorm"),
    "rezero_vector_postnorm": dict(B=2, L=64, H=2, FF=96, T=3, rezero="vector"),
    "rezero_vector_prenorm": dict(B=2, L=64, H=2, FF=96, T=3, rezero="vector", norm="prenorm"),
    "normoff": dict(B=2, L=64, H=2, FF=96, T=3, norm="off"),
}
TRANSFORMER_SHAPES = [(3, 40, 64, 4, 96, 2), (2, 132, 128, 4, 256, 3), (2, 64, 64, 2, 128, 1)]  # test_stack_matches_torch_transformer_encoder_layer
TRANSFORMER_P = 0.1
MODELS = [("seq-great", 64, 4), ("seq-great", 64, 2), ("seq-rat", 64, 4), ("seq-transformer", 64, 4)]
MODEL_P, MODEL_SEED = 0.1, 7


def rel_err(got, want) -> float:
    """the tolerance's measure: |got - want|_max / max(1, |want|_max)"""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).abs().max()) / max(1.0, float(want.abs().max()))


def worst(got: dict, want: dict):
    """(largest rel_err, its name) over the union of names; a gradient that is missing on one side counts as zeros"""
    errs = {}
    for k in set(got) | set(want):
        a, b = got.get(k), want.get(k)
        a = torch.zeros_like(b) if a is None else a
        b = torch.zeros_like(a) if b is None else b
        errs[k] = rel_err(a, b)
    k = max(errs, key=errs.get)
    return errs[k], k


def _f64(t):
    return t.detach().cpu().double().contiguous()


def layer_tensors(layers, pick) -> dict:
    """{oracle name: pick(parameter) as float64 CPU} of a stack of the library's encoder layers."""
    from buglab.models.layers.transformer import TransformerEncoderLayer

    out = {}
    for i, layer in enumerate(layers):
        t = {k: pick(v) for k, v in layer.named_parameters()}
        if isinstance(layer, TransformerEncoderLayer):
            for k, v in layer.torch_layout(t).items():
                out[f"layers.{i}.{k}"] = _f64(v)
        else:
            for ours, (ref, tr) in ENC.items():
                if ours in t:
                    out[f"layers.{i}.{ref}"] = _f64(t[ours].T if tr else t[ours])
    return out


def value(p):
    return p.detach()


def grad(p):
    return p.grad if p.grad is not None else torch.zeros_like(p)


def leaves(t: dict) -> dict:
    return {k: v.clone().requires_grad_(True) for k, v in t.items()}


def grads_of(p: dict) -> dict:
    return {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in p.items()}


# ---- a stack of relational layers ------------------------------------------------------------------------------------------
def relational_case(B, L, H, FF, T, dk=32, *, layers=2, edges_on=True, value_bias=False, scalar=False, norm="postnorm", rezero="off",
                    p=0.1, seed=0):
    from buglab.models.layers.relational_transformer import RelationalTransformerEncoderLayer

    D = H * dk
    torch.manual_seed(1000 + seed)
    stack = torch.nn.ModuleList([
        RelationalTransformerEncoderLayer(D, dk, dk, H, T, dim_feedforward=FF, dropout=p, use_edge_value_biases=value_bias,
                                          edge_attention_bias_is_scalar=scalar, rezero_mode=rezero, normalisation_mode=norm)
        for _ in range(layers)])
    with torch.no_grad():
        for l in stack:
            if norm != "off":  # LayerNorm affine away from (1, 0) so that the norm1 / norm2 mix-up is visible
                for q in (l.norm1_g, l.norm2_g):
                    q.add_(0.2 * torch.randn_like(q))
                for q in (l.norm1_b, l.norm2_b):
                    q.add_(0.2 * torch.randn_like(q))
            if rezero != "off":  # at their zero initialisation the layer is the identity
                for q in (l.alpha1, l.alpha2):
                    q.copy_(0.7 + 0.4 * torch.randn_like(q))
            for q in (l.edge_bias_f, l.edge_bias_r):
                q.mul_(0.3)
    rng = np.random.default_rng(seed)
    lens = rng.integers(max(1, L // 2), L + 1, size=B).astype(np.int32)
    lens[0] = L
    ne = 6 * L
    e = np.stack([rng.integers(0, B, ne), rng.integers(0, L, ne), rng.integers(0, L, ne)], 1)
    e = e[(e[:, 1] < lens[e[:, 0]]) & (e[:, 2] < lens[e[:, 0]]) & (e[:, 1] != 3)]  # (position 3 has no outgoing entries)
    e = np.concatenate([e, e[:5]])  # repeated edges accumulate
    # a hub: position 7 of sample 0 takes part in 90 more edges (more than the 64 entries a wave fetches ahead per row)
    hub = np.stack([np.zeros(90, np.int64), np.full(90, 7), rng.integers(0, int(lens[0]), 90)], 1)
    e = np.concatenate([e, hub, hub[:, [0, 2, 1]][:40]])
    if not edges_on:
        e = e[:0]
    types = rng.integers(0, T, e.shape[0])
    x = torch.randn(B, L, D)
    valid = torch.arange(L)[None, :] < torch.from_numpy(lens).long()[:, None]
    w = torch.randn(B, L, D) * valid[:, :, None]  # loss weights, masked to the valid positions
    cfg = G.GreatConfig(d_model=D, num_heads=H, num_layers=layers, dim_feedforward=FF, num_edge_types=T, use_edge_value_biases=value_bias,
                        edge_attention_bias_is_scalar=scalar, normalisation_mode=norm, rezero_mode=rezero)
    return dict(kind="relational", stack=stack, cfg=cfg, B=B, L=L, D=D, lens=lens, edges=e.astype(np.int64), types=types.astype(np.int64),
                x=x, w=w, valid=valid)


def oracle_stack(case, p_drop, seed=SEED, alter=None) -> dict:
    """float64: {"y": output at the valid positions, "g.x": input gradient there, "g.<name>": every parameter gradient}"""
    p = leaves(layer_tensors(case["stack"], value))
    x = case["x"].double().requires_grad_(True)
    masked = ~case["valid"]
    if case["kind"] == "relational":
        y = G.encoder_stack(p, x, masked, torch.from_numpy(case["edges"]), torch.from_numpy(case["types"]), case["cfg"],
                            p_drop=p_drop, seed=seed if p_drop > 0 else None, _alter=alter)
    else:
        y = TO.encoder_stack(p, x, masked, len(case["stack"]), case["H"], p_drop=p_drop, seed=seed if p_drop > 0 else None, _alter=alter)
    (y * case["w"].double()).sum().backward()
    out = {"y": y.detach()[case["valid"]], "g.x": x.grad[case["valid"]]}
    out.update({"g." + k: v for k, v in grads_of(p).items()})
    return out


# ---- a stack of plain transformer layers -----------------------------------------------------------------------------------
def transformer_case(B, L, D, H, FF, layers, p=TRANSFORMER_P):
    """The inputs of test_stack_matches_torch_transformer_encoder_layer; case["torch"] is the float64 torch module stack itself."""
    from buglab.models.layers.transformer import TransformerEncoderLayer

    torch.manual_seed(B * 1000 + L)
    ref = torch.nn.ModuleList([torch.nn.TransformerEncoderLayer(d_model=D, nhead=H, dim_feedforward=FF, dropout=0.0) for _ in range(layers)]).double()
    with torch.no_grad():  # (torch zero-initialises the projection biases: give them values so that their handling is tested)
        for l in ref:
            for b in (l.self_attn.in_proj_bias, l.self_attn.out_proj.bias):
                b.uniform_(-0.3, 0.3)
            for n in (l.norm1, l.norm2):
                n.weight.uniform_(0.5, 1.5)
                n.bias.uniform_(-0.2, 0.2)
            for q in l.parameters():  # the HIP layer holds fp32 copies: make the float64 values exactly representable
                q.copy_(q.float().double())
    stack = torch.nn.ModuleList([TransformerEncoderLayer(D, H, FF, dropout=p).load_torch_layer(l) for l in ref])
    lens = np.array([L, max(1, L // 2), max(1, L - 7)][:B], dtype=np.int32)
    x = torch.randn(B, L, D)
    valid = torch.arange(L)[None, :] < torch.from_numpy(lens).long()[:, None]
    w = torch.randn(B, L, D) * valid[:, :, None]
    return dict(kind="transformer", stack=stack, torch=ref, B=B, L=L, D=D, H=H, lens=lens, x=x, w=w, valid=valid)


# ---- whole models through the registry -------------------------------------------------------------------------------------
def model_case(model_name, hidden, heads, p=MODEL_P):
    """(model, module on the CPU, minibatch as NumPy, oracle config): the host pipeline of test_seq_model_end_to_end_matches_oracle."""
    from buglab.data.synthetic import make_buglab_seq_dataset
    from buglab.models.modelregistry import load_model

    data = make_buglab_seq_dataset(6, seed=5)
    model = load_model({"modelName": model_name, "hidden_state_size": hidden, "num_layers": 2, "num_heads": heads, "intermediate_dimension_size": 96,
                        "dropout_rate": p}, Path("/tmp/_bl_seq_dropout_parity.pkl.gz"))[0]
    model.compute_metadata(copy.deepcopy(data))
    torch.manual_seed(0)
    module = model.build_neural_module().train()
    with torch.no_grad():
        for l in module._gnn.layers:
            for n in ("norm1_g", "norm2_g", "norm1_b", "norm2_b"):
                q = getattr(l, n)
                q.add_(0.2 * torch.randn_like(q))
            # peaked attention, as in a trained model: at the initialisation's near-uniform probabilities a missing 1 / (1 - p) on
            # the encoder's input is a common factor that the first LayerNorm removes, and the teeth condition would not hold
            (l.in_proj_W if hasattr(l, "in_proj_W") else l.qkv_W).mul_(2.0)
    samples = [model.tensorize(copy.deepcopy(d)) for d in data]
    assert all(s is not None for s in samples)
    mb_np = model.collate_minibatch({"samples": samples})
    cfg = G.GreatConfig(d_model=hidden, num_heads=heads, num_layers=2, dim_feedforward=96, num_edge_types=max(1, len(model.edge_types)),
                        use_edge_value_biases=model_name == "seq-rat")
    return dict(model=model, module=module, mb=mb_np, cfg=cfg, layer_type="transformer" if model_name == "seq-transformer" else "great")


def model_tensors(module, pick) -> dict:
    """{oracle name: pick(parameter) as float64 CPU} of a SeqBugLabModule"""
    out = layer_tensors(module._gnn.layers, pick)
    for k, v in module.named_parameters():
        if k == "_gnn.embed.table":
            out["embed.table"] = _f64(pick(v))
        elif k == "_gnn.positional_encoding":
            out["positional_encoding"] = _f64(pick(v))
        elif k in ("_gnn.input_norm_g", "_gnn.input_norm_b"):
            out["input_norm." + ("weight" if k.endswith("_g") else "bias")] = _f64(pick(v))
        else:
            for a, b in HEADS.items():
                if k.startswith(a):
                    out[b + k[len(a):]] = _f64(pick(v))
    return out


def oracle_model(case, p_drop, seed=MODEL_SEED, alter=None) -> dict:
    """float64: {"loss", "g.<name>" for every parameter}"""
    p = leaves(model_tensors(case["module"], value))
    out = SO.forward_loss(p, case["mb"], case["cfg"], p_drop=p_drop, seed=seed if p_drop > 0 else None, layer_type=case["layer_type"], _alter=alter)
    out["loss"].backward()
    res = {"loss": out["loss"].detach().reshape(1)}
    res.update({"g." + k: v for k, v in grads_of(p).items()})
    return res


# ---- the var-misuse model (greatreimplementation.py, prenorm) ----------------------------------------------------------------
VARMISUSE = dict(D=64, H=2, FF=96, layers=2, n_ids=3, B=3, L=48, p=0.1, seed=5)


def varmisuse_case():
    from buglab.models.greatreimplementation import GreatVarMisuseModule
    from buglab.models.layers.messagepassing import SubtokenEmbedder

    c = VARMISUSE
    D, H, FF, layers, n_ids, B, L = (c[k] for k in ("D", "H", "FF", "layers", "n_ids", "B", "L"))
    torch.manual_seed(3)
    m = GreatVarMisuseModule(SubtokenEmbedder(32, D, 6, 0.0, subtoken_combination="mean"), num_edge_types=2 * n_ids, num_layers=layers,
                             num_heads=H, intermediate_dimension=FF, dropout_rate=c["p"]).train()
    with torch.no_grad():
        for layer in m.seq_layers:
            for q in (layer.norm1_g, layer.norm2_g, layer.norm1_b, layer.norm2_b):
                q.add_(0.2 * torch.randn_like(q))
            layer.edge_bias_f.mul_(0.3)
            layer.edge_bias_r.mul_(0.3)
        m.ln_out_g.add_(0.2 * torch.randn_like(m.ln_out_g))
    g = torch.Generator().manual_seed(1)
    lengths = torch.tensor([L, 30, 41])
    lens_att = torch.minimum(lengths + 1, torch.tensor(L)).to(torch.int32)
    E = 400
    s = torch.randint(0, B, (E,), generator=g)
    edges = torch.stack([s, (torch.rand(E, generator=g) * lengths[s]).long(), (torch.rand(E, generator=g) * lengths[s]).long()], 1).numpy()
    edges[5] = edges[4]
    ids = torch.randint(0, n_ids, (E,), generator=g).numpy()
    err = torch.tensor([0, 17, 9], dtype=torch.int32)
    cand = torch.zeros(B, L, dtype=torch.bool)
    tgt = torch.zeros(B, L, dtype=torch.bool)
    cand[:, [3, 9, 17, 25]] = True
    tgt[1, [3, 20]] = True
    tgt[2, [25]] = True
    emb = 0.5 * torch.randn(B * L, D, generator=g)
    e_all = np.concatenate([edges, edges[:, [0, 2, 1]]])  # reverse edges get ids of their own (greatreimplementation.py)
    t_all = np.concatenate([ids, ids + n_ids])
    cfg = G.GreatConfig(d_model=D, num_heads=H, num_layers=layers, dim_feedforward=FF, num_edge_types=2 * n_ids, normalisation_mode="prenorm")
    return dict(module=m, emb=emb, lens_att=lens_att, e_all=e_all, t_all=t_all, err=err, cand=cand, tgt=tgt, cfg=cfg, B=B, L=L, D=D)


def varmisuse_tensors(m, pick) -> dict:
    out = layer_tensors(m.seq_layers, pick)
    for k in ("ln_out_g", "ln_out_b", "predictions_W", "predictions_b"):
        out[k] = _f64(pick(getattr(m, k)))
    return out


def oracle_varmisuse(case, p_drop, seed=VARMISUSE["seed"], alter=None) -> dict:
    from tests.test_great_varmisuse_gpu import ref_head  # the float64 restatement of the reference's head

    m, B, L, D = case["module"], case["B"], case["L"], case["D"]
    p = leaves(varmisuse_tensors(m, value))
    x = case["emb"].double().requires_grad_(True)
    h = x.reshape(B, L, D) + m.positional_encodings[:L].double().cpu()[None]
    masked = torch.arange(L)[None, :] >= case["lens_att"].long()[:, None]
    h = G.encoder_stack(p, h, masked, torch.from_numpy(case["e_all"]), torch.from_numpy(case["t_all"]), case["cfg"], p_drop=p_drop,
                        seed=seed if p_drop > 0 else None, _alter=alter)
    _, loss, _ = ref_head(h.reshape(B * L, D), p["ln_out_g"], p["ln_out_b"], p["predictions_W"], p["predictions_b"], case["lens_att"],
                          case["err"], case["cand"], case["tgt"], B, L)
    loss.backward()
    res = {"loss": loss.detach().reshape(1), "g.emb": x.grad}
    res.update({"g." + k: v for k, v in grads_of(p).items()})
    return res


# ---- the alterations of the teeth conditions ---------------------------------------------------------------------------------
LAYER_ALTERATIONS = [(site, how) for site in range(4) for how in ("stream", "noscale")]
ENCODER_ALTERATIONS = [(site, how) for site in ("embed", "input") for how in ("stream", "noscale")]


def discrepancy(altered: dict, base: dict) -> float:
    """how far a wrong variant is from the oracle, in the tolerance's measure, at its most visible tensor"""
    return worst(altered, base)[0]
