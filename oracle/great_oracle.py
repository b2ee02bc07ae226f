"""CPU oracle for the `seq-great` relational-transformer block (SURVEY.md section 8f rank 1,
BASELINE.json configs[4]).  TEST INFRASTRUCTURE ONLY -- groundwork for the device path of a later round:
no product code imports this file and the registry still raises NotImplementedError for "seq-great".

PARITY STATUS: **pinned**.  Unlike the ptgnn layers of `gnn-mlp`, this block lives in the reference tree
(`buglab/models/layers/multihead_attention.py`, `relational_multihead_attention.py`,
`relational_transformer.py`), is pure PyTorch and importable offline: `tests/golden/make_golden_great.py`
runs the reference's own `RelationalTransformerEncoderLayer` stack on seeded inputs and commits inputs,
weights, outputs and gradients; `tests/test_great_oracle_golden.py` checks this restatement against them.

Weights are passed as a dict with the reference's own state_dict names (per layer prefix `layers.{i}.`).

DROPOUT.  The reference's stateful Philox masks cannot be reproduced, so the pinned parity runs use p = 0 (the default here:
`p_drop = 0` or `seed = None` is the reference's arithmetic, bit for bit what this file computed before it knew dropout).
With `p_drop > 0` and a seed the oracle speaks the LIBRARY's dropout instead: the stateless counter hash of
`buglab_oracle.dropout_keep_mask` (keep element i of a site iff lowbias32(i + key(seed, stream)) >> 8 >= float32(p) * 2^24,
kept values times 1 / (1 - p)).  The sites are the reference's four nn.Dropout modules; streams and element indices are the
specification of the HIP path as `hip_ops` / `csrc/bl_common.h` document it (written down from there, not fitted to output):

  stream + 0   attention probabilities, after the softmax (multihead_attention.py:72).  Element index = row-major index into
               [B * H * L, L]: row (b * H + h) * L + q, column = key position.  The value-bias term of "rat" reads the DROPPED
               probabilities, as the reference does (relational_multihead_attention.py:155-178 receives what :72 returned).
  stream + 1   attention sublayer output, after the rezero scale and before the residual sum (relational_transformer.py:112-113).
               Element index = row-major index into [B * L, D].
  stream + 2   feed-forward hidden activations, after the ReLU (:120).  Row-major [B * L, FF].
  stream + 3   feed-forward sublayer output, after the rezero scale and before the residual sum (:121-122).  Row-major [B * L, D].

Layer i of a stack gets `stream = 8 * (i + 1)` (the encoder keeps streams 0 and 1 for the embedder and its input dropout).

REZERO / NORMALISATION.  `rezero_mode` "scalar" / "vector" multiplies each sublayer output by `_alpha1` / `_alpha2` (a scalar or a
[D] vector) before its dropout (:112, :121); `normalisation_mode` "off" drops both LayerNorms (:82-84).  Both are pinned to the
reference by the golden cases `rezero_scalar`, `rezero_vector`, `normoff`.

`_alter = (site, how)` is for the tests' "teeth" conditions only: it evaluates a deliberately WRONG variant -- how = "stream":
that site draws from stream + 1 of its own; "noscale": the 1 / (1 - p) factor is left out at that site; (0, "vb_undropped"):
the value-bias term reads the undropped probabilities."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import torch
import torch.nn.functional as F

from oracle.buglab_oracle import apply_dropout


@dataclass
class GreatConfig:
    """`seq-great` as the registry builds it: reference modelregistry.py:97-127 (hidden 256, 5 layers, 8 heads,
    FF 1024, postnorm, rezero off) and seqmodel.py:91-106 (key = value dim = D / heads, edge value biases only
    for layer_type "rat", `edge_attention_bias_is_scalar` left at its default False -> the query-bias branch)."""

    d_model: int = 256
    num_heads: int = 8
    num_layers: int = 5
    dim_feedforward: int = 1024
    num_edge_types: int = 8
    use_edge_value_biases: bool = False
    edge_attention_bias_is_scalar: bool = False
    normalisation_mode: str = "postnorm"  # "postnorm" | "prenorm" | "off"
    rezero_mode: str = "off"  # "off" | "scalar" | "vector": `_alpha1` / `_alpha2` of relational_transformer.py:93-104
    activation: str = "relu"  # relational_transformer.py:29 default, not overridden by seqmodel.py

    @property
    def head_dim(self) -> int:
        return self.d_model // self.num_heads


def _site(t, site: int, p_drop: float, seed: Optional[int], stream: int, _alter):
    """Dropout site `site` of a layer on `t`, whose row-major order is the site's element index (module docstring)."""
    if seed is None or p_drop <= 0.0:
        return t
    how = _alter[1] if (_alter is not None and _alter[0] == site) else None
    y = apply_dropout(t.contiguous(), p_drop, seed, stream + site + (1 if how == "stream" else 0))
    return y * (1.0 - p_drop) if how == "noscale" else y


def relational_attention(p: Dict[str, torch.Tensor], pre: str, x, masked, edges, edge_types, cfg: GreatConfig,
                         p_drop: float = 0.0, seed: Optional[int] = None, stream: int = 0, _alter: Optional[Tuple[int, str]] = None):
    """RelationalMultiheadAttention.forward (relational_multihead_attention.py:72-88).

    x [B, L, D]; masked bool [B, L] (True = padding key) or None; edges int64 [E, 3] = (sample, source, target);
    edge_types int64 [E].  p_drop, seed, stream: dropout on the probabilities (site `stream + 0`, module docstring)."""
    B, L, _ = x.shape
    H, dk = cfg.num_heads, cfg.head_dim
    # multihead_attention.py:46-57: one bias-free projection, per head [q | k | v], queries pre-scaled by dk^-0.5
    qkv = (x @ p[pre + "self_attn._selfatt_head_transforms.weight"].T).reshape(B, L, H, 3 * dk)
    q, k, v = torch.split(qkv, [dk, dk, dk], dim=-1)
    q = q * dk ** -0.5
    scores = torch.einsum("bkhd,bqhd->bqkh", k, q)  # :59-65   [B, query, key, head]
    if edges.shape[0] > 0:  # relational_multihead_attention.py:90-112
        s, src, tgt = edges[:, 0], edges[:, 1], edges[:, 2]
        bias = p[pre + "self_attn._edge_attention_biases.weight"][edge_types]
        bias_r = p[pre + "self_attn._reverse_edge_attention_biases.weight"][edge_types]
        if cfg.edge_attention_bias_is_scalar:  # :119-134 (GREAT as published: scalar x key, target side)
            e_f = torch.einsum("eh,ehd->eh", bias, k[s, tgt])
            e_r = torch.einsum("eh,ehd->eh", bias_r, k[s, src])
        else:  # :135-152 (what `seq-great` actually runs: vector bias x query, source side)
            e_f = torch.einsum("ehd,ehd->eh", bias.reshape(-1, H, dk), q[s, src])
            e_r = torch.einsum("ehd,ehd->eh", bias_r.reshape(-1, H, dk), q[s, tgt])
        scores = scores.contiguous().index_put((torch.cat([s, s]), torch.cat([src, tgt]), torch.cat([tgt, src])),
                                               torch.cat([e_f, e_r]), accumulate=True)
    scores = scores.transpose(2, 3)  # multihead_attention.py:67-77   [B, query, head, key]
    if masked is not None:
        scores = scores.masked_fill(masked[:, None, None, :], -math.inf)
    probs = F.softmax(scores, dim=-1)
    undropped = probs
    if seed is not None and p_drop > 0.0:  # multihead_attention.py:72; the library's mask is indexed [B, head, query, key]
        probs = _site(probs.permute(0, 2, 1, 3), 0, p_drop, seed, stream, _alter).permute(0, 2, 1, 3)
    ctxv = torch.einsum("blhq,bqhd->blhd", probs, v)  # :79-80
    if cfg.use_edge_value_biases and edges.shape[0] > 0:  # relational_multihead_attention.py:155-178 ("rat")
        s, src, tgt = edges[:, 0], edges[:, 1], edges[:, 2]
        if _alter == (0, "vb_undropped"):
            probs = undropped
        vb = probs[s, src, :, tgt].unsqueeze(-1) * p[pre + "self_attn._edge_value_biases.weight"][edge_types].reshape(-1, H, dk)
        vb_r = probs[s, tgt, :, src].unsqueeze(-1) * p[pre + "self_attn._reverse_edge_value_biases.weight"][edge_types].reshape(-1, H, dk)
        ctxv = ctxv.contiguous().index_put((torch.cat([s, s]), torch.cat([src, tgt])), torch.cat([vb, vb_r]), accumulate=True)
    return ctxv.reshape(B, L, H * dk) @ p[pre + "self_attn._out_proj.weight"].T  # multihead_attention.py:82-88


def encoder_layer(p: Dict[str, torch.Tensor], pre: str, x, masked, edges, edge_types, cfg: GreatConfig,
                  p_drop: float = 0.0, seed: Optional[int] = None, stream: int = 0, _alter: Optional[Tuple[int, str]] = None):
    """RelationalTransformerEncoderLayer.forward (relational_transformer.py:106-125)."""
    def ln(t, which):
        return F.layer_norm(t, (cfg.d_model,), p[pre + which + ".weight"], p[pre + which + ".bias"], 1e-5)

    assert cfg.normalisation_mode in ("postnorm", "prenorm", "off") and cfg.rezero_mode in ("off", "scalar", "vector")
    rezero = cfg.rezero_mode != "off"
    act = F.relu if cfg.activation == "relu" else F.gelu
    a_in = ln(x, "norm1") if cfg.normalisation_mode == "prenorm" else x
    att = relational_attention(p, pre, a_in, masked, edges, edge_types, cfg, p_drop, seed, stream, _alter)
    if rezero:
        att = p[pre + "_alpha1"] * att  # :112
    x = x + _site(att, 1, p_drop, seed, stream, _alter)
    if cfg.normalisation_mode == "postnorm":
        x = ln(x, "norm1")
    f_in = ln(x, "norm2") if cfg.normalisation_mode == "prenorm" else x
    hidden = _site(act(f_in @ p[pre + "linear1.weight"].T + p[pre + "linear1.bias"]), 2, p_drop, seed, stream, _alter)
    ff = hidden @ p[pre + "linear2.weight"].T + p[pre + "linear2.bias"]
    if rezero:
        ff = p[pre + "_alpha2"] * ff  # :121
    x = x + _site(ff, 3, p_drop, seed, stream, _alter)
    if cfg.normalisation_mode == "postnorm":
        x = ln(x, "norm1")  # sic: the reference re-uses norm1 for the second sublayer (:123-124); norm2 stays unused
    return x


def encoder_stack(p: Dict[str, torch.Tensor], x, masked, edges, edge_types, cfg: GreatConfig, prefix: str = "layers.",
                  p_drop: float = 0.0, seed: Optional[int] = None, _alter: Optional[Tuple[int, str]] = None):
    """The `__seq_layers` loop of SeqBugLabModule (reference seqmodel.py, layer_type in {"great", "rat"}); layer i draws its
    dropout masks from streams 8 * (i + 1) + {0, 1, 2, 3}."""
    for i in range(cfg.num_layers):
        x = encoder_layer(p, f"{prefix}{i}.", x, masked, edges, edge_types, cfg, p_drop, seed, 8 * (i + 1), _alter)
    return x
