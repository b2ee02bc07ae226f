#!/usr/bin/env python
"""Golden vectors for the GREAT var-misuse model (buglab/models/greatreimplementation.py): the encoder is the REFERENCE's own
`RelationalTransformerEncoderLayer` stack (pure PyTorch, importable offline -- as in make_golden_great.py), the position table and
the output head are restated here from their formulas (reference greatreimplementation.py:60-67, :118-214).  The token embedder
is bypassed: the fixture starts from the embedded sequence.  Run in the build container only:
    python tests/golden/make_golden_varmisuse.py
Writes tests/golden/varmisuse_prenorm.npz (embedded input, weights, masks, logits, loss, stats, every gradient)."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, "/root/reference")
from buglab.models.layers.relational_transformer import RelationalTransformerEncoderLayer  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def positions(L, D):
    pos = np.arange(L, dtype=np.float64)[:, None]
    i = np.arange(D, dtype=np.float64)[None, :]
    a = pos / 10000.0 ** (2.0 * i / D)
    return torch.tensor(np.where(np.arange(D)[None, :] % 2 == 0, np.sin(a), np.cos(a)), dtype=torch.float32)


def make(seed=0, D=64, H=4, FF=96, n_ids=3, layers=2, lengths=(23, 17, 9, 23), E=60):
    torch.manual_seed(seed)
    T = 2 * n_ids
    stack = torch.nn.ModuleList([
        RelationalTransformerEncoderLayer(d_model=D, key_query_dimension=D // H, value_dimension=D // H, nhead=H, num_edge_types=T,
                                          dim_feedforward=FF, dropout=0.0, use_edge_value_biases=False, normalisation_mode="prenorm")
        for _ in range(layers)])
    with torch.no_grad():
        for l in stack:
            for nrm in (l.norm1, l.norm2):
                nrm.weight.add_(0.3 * torch.randn_like(nrm.weight))
                nrm.bias.add_(0.3 * torch.randn_like(nrm.bias))
    ln_g = (1.0 + 0.3 * torch.randn(D)).requires_grad_(True)
    ln_b = (0.3 * torch.randn(D)).requires_grad_(True)
    W = (torch.randn(D, 2) / D ** 0.5).requires_grad_(True)  # [in, out]
    bias = (0.1 * torch.randn(2)).requires_grad_(True)
    g = torch.Generator().manual_seed(seed + 1)
    B, L = len(lengths), max(lengths)
    lens = torch.tensor(lengths)
    emb = torch.randn(B, L, D, generator=g, requires_grad=True)
    s = torch.randint(0, B, (E,), generator=g)
    src = (torch.rand(E, generator=g) * lens[s]).long()
    tgt = (torch.rand(E, generator=g) * lens[s]).long()
    ids = torch.randint(0, n_ids, (E,), generator=g)
    edges = torch.stack([s, src, tgt], 1)
    # edges plus their reversal with the type shifted by n (greatreimplementation.py:332-334)
    all_edges = torch.cat([edges, edges[:, [0, 2, 1]]])
    all_types = torch.cat([ids, ids + n_ids])
    err = torch.tensor([0, 5, 3, 11])  # sample 0: NO_BUG
    cand = torch.zeros(B, L, dtype=torch.bool)
    targ = torch.zeros(B, L, dtype=torch.bool)
    cand[1, [2, 5, 8, 12, 16]] = True
    targ[1, [8, 14]] = True            # two targets, 14 is not a candidate
    cand[2, [1, 3, 6]] = True
    targ[2, [6]] = True
    cand[3, [4, 11, 19, 22]] = True
    targ[3, [4, 22]] = True

    x = emb + positions(L, D)[None]
    token_mask = torch.arange(L)[None, :] > lens[:, None]  # sic: position `length` is not masked (:198)
    state = x
    for l in stack:
        state = l(state, token_mask, all_edges, all_types)
    logits = F.layer_norm(state, (D,), ln_g, ln_b, 1e-5) @ W + bias
    logits = logits.masked_fill(token_mask[:, :, None], -float("inf"))
    loc = logits[:, :, 0]
    ptr_lp = torch.log_softmax(logits[:, :, 1].masked_fill(~cand, -float("inf")), dim=-1)
    loc_loss = F.cross_entropy(loc, err)
    buggy = err != 0
    rep_lp = torch.logsumexp(ptr_lp[buggy].masked_fill(~targ[buggy], -float("inf")), dim=-1)
    rep_loss = -rep_lp.mean()
    loss = loc_loss + rep_loss
    loss.backward()
    loc_ok = loc.argmax(-1) == err
    rep_ok = targ[buggy][torch.arange(int(buggy.sum())), ptr_lp[buggy].argmax(-1)]
    per_loc = F.cross_entropy(loc, err, reduction="none")
    stats = np.array([B, int(loc_ok.sum()), int((loc_ok & buggy).sum()), int(buggy.sum()), int(rep_ok.sum()),
                      float(per_loc.sum()), float(-rep_lp.sum()), 1.0])
    out = {"emb": emb.detach().numpy(), "lengths": lens.numpy().astype(np.int32), "edges": edges.numpy(), "edge_ids": ids.numpy(),
           "error_location": err.numpy().astype(np.int32), "candidate_mask": cand.numpy(), "target_mask": targ.numpy(),
           "logits": logits.detach().numpy(), "loss": np.array(float(loss)), "stats": stats,
           "cfg": np.array([D, H, layers, FF, n_ids]), "g_emb": emb.grad.numpy()}
    for name, t in (("ln_g", ln_g), ("ln_b", ln_b), ("W", W), ("bias", bias)):
        out["p." + name], out["g." + name] = t.detach().numpy(), t.grad.numpy()
    for k, v in stack.state_dict().items():
        out["p.layers." + k] = v.numpy()
    for k, v in stack.named_parameters():
        out["g.layers." + k] = v.grad.numpy()
    np.savez_compressed(os.path.join(HERE, "varmisuse_prenorm.npz"), **out)
    print("loss", float(loss), "stats", stats)


if __name__ == "__main__":
    make()
