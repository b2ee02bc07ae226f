"""CPU oracle of `buglab/models/layers/transformer.py`: a float64 restatement of torch.nn.TransformerEncoderLayer as the
reference stacks it for `seq-transformer` (seqmodel.py:108-118: post-norm, relu, nn.MultiheadAttention with biased input /
output projections, queries scaled by dk^-0.5 AFTER the bias, a LayerNorm of its own per sublayer).  TEST INFRASTRUCTURE ONLY.

PARITY STATUS: **pinned** at p = 0 against torch.nn.TransformerEncoderLayer(...).double() itself, outputs and all gradients
(tests/test_seq_dropout_oracle_host.py).  Parameters are passed under torch's own state_dict names (`{prefix}{i}.self_attn.in_proj_weight`, ...).

Dropout: torch's Philox masks cannot be reproduced; with `p_drop > 0` and a seed the oracle applies the library's counter-hash
dropout (`buglab_oracle.apply_dropout`) at torch's four sites, with the streams and element indices of the relational layer
(oracle/great_oracle.py's module docstring): stream + 0 attention probabilities [B * H * L, L] (row (b * H + h) * L + q), + 1
attention sublayer output [B * L, D], + 2 feed-forward hidden after the ReLU [B * L, FF], + 3 feed-forward sublayer output [B * L, D]."""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import torch
import torch.nn.functional as F

from oracle.great_oracle import _site


def encoder_layer(p: Dict[str, torch.Tensor], pre: str, x, masked, num_heads: int, p_drop: float = 0.0, seed: Optional[int] = None,
                  stream: int = 0, _alter: Optional[Tuple[int, str]] = None):
    """x [B, L, D]; masked bool [B, L] (True = padding key: `src_key_padding_mask`)."""
    B, L, D = x.shape
    H, dk = num_heads, D // num_heads
    qkv = x @ p[pre + "self_attn.in_proj_weight"].T + p[pre + "self_attn.in_proj_bias"]  # rows of the weight: [q | k | v], each [H, dk]
    q, k, v = (t.reshape(B, L, H, dk).transpose(1, 2) for t in torch.split(qkv, [D, D, D], dim=-1))  # [B, H, L, dk]
    scores = (q * dk ** -0.5) @ k.transpose(-1, -2)  # [B, H, query, key]
    if masked is not None:
        scores = scores.masked_fill(masked[:, None, None, :], -math.inf)
    probs = _site(F.softmax(scores, dim=-1), 0, p_drop, seed, stream, _alter)
    ctx = (probs @ v).transpose(1, 2).reshape(B, L, D)
    att = ctx @ p[pre + "self_attn.out_proj.weight"].T + p[pre + "self_attn.out_proj.bias"]
    x = F.layer_norm(x + _site(att, 1, p_drop, seed, stream, _alter), (D,), p[pre + "norm1.weight"], p[pre + "norm1.bias"], 1e-5)
    hidden = _site(F.relu(x @ p[pre + "linear1.weight"].T + p[pre + "linear1.bias"]), 2, p_drop, seed, stream, _alter)
    ff = hidden @ p[pre + "linear2.weight"].T + p[pre + "linear2.bias"]
    return F.layer_norm(x + _site(ff, 3, p_drop, seed, stream, _alter), (D,), p[pre + "norm2.weight"], p[pre + "norm2.bias"], 1e-5)


def encoder_stack(p: Dict[str, torch.Tensor], x, masked, num_layers: int, num_heads: int, prefix: str = "layers.", p_drop: float = 0.0,
                  seed: Optional[int] = None, _alter: Optional[Tuple[int, str]] = None):
    """Layer i draws its dropout masks from streams 8 * (i + 1) + {0, 1, 2, 3} (SequenceEncoder.forward)."""
    for i in range(num_layers):
        x = encoder_layer(p, f"{prefix}{i}.", x, masked, num_heads, p_drop, seed, 8 * (i + 1), _alter)
    return x
