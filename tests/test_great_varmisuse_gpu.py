"""GPU: the GREAT var-misuse model on the HIP path.
  * the head (hip_ops.varmisuse_head, csrc/bl_varmisuse_head.hip) against a float64 torch restatement of the reference's head
    (greatreimplementation.py:143-174, :202-214): logits, loss, stats, every gradient; bit-identical reruns; no NaN;
  * the module (embedded input -> positions -> reference-built encoder -> head) against tests/golden/varmisuse_prenorm.npz,
    produced by the reference's own RelationalTransformerEncoderLayer (tests/golden/make_golden_varmisuse.py);
  * the default configuration's shape (D 512, 8 heads, FF 2048, 10 prenorm layers, L 512) against the float64 CPU oracle;
  * traingreat end to end on synthetic GREAT data, a falling loss on a fixed minibatch, and a checkpoint round trip."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# ours -> (reference state_dict name, transposed?)
LAYER_PARAMS = {
    "qkv_W": ("self_attn._selfatt_head_transforms.weight", True), "out_W": ("self_attn._out_proj.weight", True),
    "edge_bias_f": ("self_attn._edge_attention_biases.weight", False),
    "edge_bias_r": ("self_attn._reverse_edge_attention_biases.weight", False),
    "lin1_W": ("linear1.weight", True), "lin1_b": ("linear1.bias", False), "lin2_W": ("linear2.weight", True), "lin2_b": ("linear2.bias", False),
    "norm1_g": ("norm1.weight", False), "norm1_b": ("norm1.bias", False), "norm2_g": ("norm2.weight", False), "norm2_b": ("norm2.bias", False),
}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from buglab.models import hip_ops

    hip_ops.load_library()


def ref_head(x, g, b, W, bias, lens_att, err, cand, tgt, B, L):
    """The reference's head from its formulas (float64 in the tests).  x [B * L, D]; positions >= lens_att are masked."""
    D = x.shape[1]
    logits = F.layer_norm(x.reshape(B, L, D), (D,), g, b, 1e-5) @ W + bias
    masked = torch.arange(L)[None, :] >= lens_att.long()[:, None]
    logits = logits.masked_fill(masked[:, :, None], -math.inf)
    # the reference masks the pointer column in place (:210-211): the stored logits carry -inf at non-candidates too
    logits = torch.stack([logits[:, :, 0], logits[:, :, 1].masked_fill(~cand, -math.inf)], dim=-1)
    loc = logits[:, :, 0]
    ptr = torch.log_softmax(logits[:, :, 1], dim=-1)
    err = err.long()
    loc_loss = F.cross_entropy(loc, err)
    buggy = err != 0
    nb = int(buggy.sum())
    per_loc = F.cross_entropy(loc, err, reduction="none")
    loc_ok = loc.argmax(-1) == err
    if nb > 0:
        rep_lp = torch.logsumexp(ptr[buggy].masked_fill(~tgt[buggy], -math.inf), dim=-1)
        rep_loss = -rep_lp.mean()
        rep_ok = int(tgt[buggy][torch.arange(nb), ptr[buggy].argmax(-1)].sum())
        rep_sum = float(-rep_lp.detach().sum())
    else:
        rep_loss, rep_ok, rep_sum = 0.0, 0, 0.0
    stats = [B, int(loc_ok.sum()), int((loc_ok & buggy).sum()), nb, rep_ok, float(per_loc.sum()), rep_sum, 1.0]
    return logits.reshape(B * L, 2), loc_loss + rep_loss, stats


def _rel(a, b, scale=0.0):
    """max |a - b| relative to max |b|, or to `scale` where that is larger: g_ln_b and g_bias of the head are sums of
    softmax-minus-one-hot terms, zero up to rounding, so they are measured against the size of g_W instead."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), scale, 1e-30))


def _head_case(D, B, L, seed, no_bug=False, full_lengths=False, ties=False):
    g = torch.Generator().manual_seed(seed)
    ln_g = 1 + 0.3 * torch.randn(D, generator=g, dtype=torch.float64)
    ln_b = 0.3 * torch.randn(D, generator=g, dtype=torch.float64)
    W = torch.randn(D, 2, generator=g, dtype=torch.float64) / D ** 0.5
    bias = 0.1 * torch.randn(2, generator=g, dtype=torch.float64)
    x = torch.randn(B * L, D, generator=g, dtype=torch.float64)
    lens = torch.randint(L // 2, L + 1, (B,), generator=g)
    if full_lengths:
        lens[0] = L  # length == L: lens_att = min(L + 1, L) = L
    lens_att = torch.minimum(lens + 1, torch.full_like(lens, L)).to(torch.int32)
    cand = torch.zeros(B, L, dtype=torch.bool)
    tgt = torch.zeros(B, L, dtype=torch.bool)
    err = torch.zeros(B, dtype=torch.int32)
    for s in range(B):
        n = int(lens[s])
        c = torch.randperm(n - 1, generator=g)[: max(2, n // 4)] + 1
        cand[s, c] = True
        if not no_bug and s % 3 != 2:
            err[s] = int(c[0])
            tgt[s, c[1]] = True
            tgt[s, int(torch.randint(1, n, (1,), generator=g))] = True  # maybe not a candidate
    if ties:
        # rows 3 and 7 of sample 0 identical and aligned with W[:, 0] * ln_g: the two largest localization logits, equal; the
        # error sits at the later one, so the first-index argmax misses it
        x[3] = W[:, 0] * ln_g
        x[7] = x[3]
        err[0] = 7
        cand[0, 3] = cand[0, 7] = True
        tgt[0, 7] = True
    return x, ln_g, ln_b, W, bias, lens_att, err, cand, tgt


def _run_hip(x, ln_g, ln_b, W, bias, lens_att, err, cand, tgt):
    from buglab.models import hip_ops

    dev = "cuda"
    leaf = lambda t: t.float().to(dev).requires_grad_(True)
    xs, gs, bs, Ws, bis = leaf(x), leaf(ln_g), leaf(ln_b), leaf(W), leaf(bias)
    stats = torch.zeros(hip_ops.VARMISUSE_STATS, dtype=torch.float64, device=dev)
    loss, logits, nb = hip_ops.varmisuse_head(xs, gs, bs, Ws, bis, lens_att.to(dev), err.to(dev), cand.to(dev), tgt.to(dev), stats)
    loss.backward()
    torch.cuda.synchronize()
    return {"loss": loss.detach().cpu(), "logits": logits.cpu(), "nb": float(nb), "stats": stats.cpu(), "x": xs.grad.cpu(),
            "ln_g": gs.grad.cpu(), "ln_b": bs.grad.cpu(), "W": Ws.grad.cpu(), "bias": bis.grad.cpu()}


@pytest.mark.parametrize("case", [
    dict(D=64, B=3, L=23, seed=0, full_lengths=True),     # L not a multiple of 4, a sample with length == L
    dict(D=128, B=4, L=37, seed=1, no_bug=True),          # no buggy sample: repair loss 0, no NaN
    dict(D=512, B=5, L=64, seed=2, ties=True),            # logit ties: first index
    dict(D=512, B=30, L=130, seed=3),
])
def test_head_matches_float64_restatement(case):
    B, L = case["B"], case["L"]
    x, ln_g, ln_b, W, bias, lens_att, err, cand, tgt = _head_case(**case)
    ref_in = [t.clone().requires_grad_(True) for t in (x, ln_g, ln_b, W, bias)]
    logits_ref, loss_ref, stats_ref = ref_head(*ref_in, lens_att, err, cand, tgt, B, L)
    loss_ref.backward() if isinstance(loss_ref, torch.Tensor) else None
    out = _run_hip(x, ln_g, ln_b, W, bias, lens_att, err, cand, tgt)
    again = _run_hip(x, ln_g, ln_b, W, bias, lens_att, err, cand, tgt)
    # -inf exactly where the reference has it, the finite logits within 1e-5
    lr = logits_ref.detach()
    assert torch.equal(torch.isinf(out["logits"]), torch.isinf(lr))
    fin = ~torch.isinf(lr)
    assert _rel(out["logits"][fin], lr[fin]) < 1e-5
    assert abs(float(out["loss"]) - float(loss_ref)) <= 1e-5 * abs(float(loss_ref))
    s = out["stats"].tolist()
    assert s[:5] == stats_ref[:5] and s[7] == 1.0 and out["nb"] == stats_ref[3]
    for k in (5, 6):
        assert abs(s[k] - stats_ref[k]) <= 1e-5 * max(1.0, abs(stats_ref[k]))
    if case.get("ties"):
        r = out["logits"].reshape(B, L, 2)[0]
        assert r[3, 0] == r[7, 0] and int(r[:, 0].argmax()) == 3
    scale = float(ref_in[3].grad.abs().max())
    for name, t in zip(("x", "ln_g", "ln_b", "W", "bias"), ref_in):
        ref_g = t.grad if t.grad is not None else torch.zeros_like(t)
        assert torch.isfinite(out[name]).all(), name
        sc = scale if name in ("ln_b", "bias") else 0.0
        assert _rel(out[name], ref_g, sc) < 1e-5, (name, _rel(out[name], ref_g, sc))
    masked = torch.arange(L)[None, :] >= lens_att.long()[:, None]
    assert (out["x"].reshape(B, L, -1)[masked] == 0).all()
    for k in ("loss", "logits", "x", "ln_g", "ln_b", "W", "bias"):  # bit-identical reruns
        assert torch.equal(out[k], again[k]), k


def _small_module(D, H, FF, layers, n_ids, vocab=32):
    from buglab.models.greatreimplementation import GreatVarMisuseModule
    from buglab.models.layers.messagepassing import SubtokenEmbedder

    return GreatVarMisuseModule(SubtokenEmbedder(vocab, D, 6, 0.0, subtoken_combination="mean"), num_edge_types=2 * n_ids,
                                num_layers=layers, num_heads=H, intermediate_dimension=FF, dropout_rate=0.0)


def _load_layers(module, params, prefix):
    with torch.no_grad():
        for i, layer in enumerate(module.seq_layers):
            for ours, (ref, tr) in LAYER_PARAMS.items():
                v = torch.as_tensor(np.asarray(params[f"{prefix}{i}.{ref}"]))
                getattr(layer, ours).copy_(v.T if tr else v)


def _edges_device(edges, ids, n_ids, B, L):
    from buglab.data.seqcollate import edge_csr
    from buglab.models.hip_ops import RelEdges

    e = np.concatenate([edges, edges[:, [0, 2, 1]]])
    t = np.concatenate([ids, ids + n_ids])
    rp, key, code = edge_csr(e, t, B, L)
    c = lambda a: torch.from_numpy(a).cuda()
    return RelEdges(c(rp), c(key), c(code), int(key.shape[0])), e, t


def test_module_matches_reference_golden():
    z = np.load(os.path.join(GOLD, "varmisuse_prenorm.npz"))
    D, H, layers, FF, n_ids = (int(v) for v in z["cfg"])
    B, L0, _ = z["emb"].shape
    L = (L0 + 3) // 4 * 4  # padded like a collated minibatch: the extra position is masked
    m = _small_module(D, H, FF, layers, n_ids).cuda()
    _load_layers(m, {k[2:]: z[k] for k in z.files if k.startswith("p.layers.")}, "layers.")
    with torch.no_grad():
        m.ln_out_g.copy_(torch.from_numpy(z["p.ln_g"]))
        m.ln_out_b.copy_(torch.from_numpy(z["p.ln_b"]))
        m.predictions_W.copy_(torch.from_numpy(z["p.W"]))
        m.predictions_b.copy_(torch.from_numpy(z["p.bias"]))
    emb = torch.zeros(B, L, D)
    emb[:, :L0] = torch.from_numpy(z["emb"])
    emb = emb.reshape(B * L, D).cuda().requires_grad_(True)
    lengths = torch.from_numpy(z["lengths"])
    lens_att = torch.minimum(lengths + 1, torch.tensor(L0)).to(torch.int32).cuda()
    edges, _, _ = _edges_device(z["edges"], z["edge_ids"], n_ids, B, L)
    pad = lambda a: torch.from_numpy(np.pad(a, ((0, 0), (0, L - L0)))).cuda()
    m.reset_metrics()
    loss = m.loss_from_embedded(emb, B, L, lens_att, edges, torch.from_numpy(z["error_location"]).cuda(), pad(z["candidate_mask"]),
                                pad(z["target_mask"]))
    loss.backward()
    assert abs(float(loss) - float(z["loss"])) < 1e-4 * abs(float(z["loss"]))
    s = m.metric_stats.cpu().numpy()
    assert (s[:5] == z["stats"][:5]).all() and np.allclose(s[5:7], z["stats"][5:7], rtol=1e-4)
    g_emb = emb.grad.reshape(B, L, D)[:, :L0].cpu()
    assert _rel(g_emb, torch.from_numpy(z["g_emb"])) < 1e-4
    assert (emb.grad.reshape(B, L, D)[:, L0:] == 0).all()
    scale = float(np.abs(z["g.W"]).max())
    for ours, key in (("ln_out_g", "g.ln_g"), ("ln_out_b", "g.ln_b"), ("predictions_W", "g.W"), ("predictions_b", "g.bias")):
        sc = scale if ours in ("ln_out_b", "predictions_b") else 0.0
        assert _rel(getattr(m, ours).grad, torch.from_numpy(z[key]), sc) < 1e-4, ours
    for i, layer in enumerate(m.seq_layers):
        for ours, (ref, tr) in LAYER_PARAMS.items():
            want = torch.from_numpy(z[f"g.layers.{i}.{ref}"])
            assert _rel(getattr(layer, ours).grad, want.T if tr else want) < 1e-4, (i, ours)
    metrics = m.report_metrics()
    assert metrics["Num samples"] == B and metrics["Localization Accuracy"] == z["stats"][1] / B


def test_full_size_matches_float64_oracle():
    """The default configuration's shape: D 512, 8 heads, FF 2048, 10 prenorm layers, L 512, B 2 (oracle/great_oracle.py)."""
    from oracle import great_oracle as O

    D, H, FF, layers, n_ids, B, L = 512, 8, 2048, 10, 4, 2, 512
    torch.manual_seed(0)
    m = _small_module(D, H, FF, layers, n_ids).cuda()
    with torch.no_grad():
        for layer in m.seq_layers:
            for p in (layer.norm1_g, layer.norm2_g):
                p.add_(0.2 * torch.randn_like(p))
            layer.edge_bias_f.mul_(0.1)
            layer.edge_bias_r.mul_(0.1)
        m.ln_out_g.add_(0.2 * torch.randn_like(m.ln_out_g))
    g = torch.Generator().manual_seed(1)
    lengths = torch.tensor([L, 300])
    lens_att = torch.minimum(lengths + 1, torch.tensor(L)).to(torch.int32)
    E = 1500
    s = torch.randint(0, B, (E,), generator=g)
    edges = torch.stack([s, (torch.rand(E, generator=g) * lengths[s]).long(), (torch.rand(E, generator=g) * lengths[s]).long()], 1).numpy()
    ids = torch.randint(0, n_ids, (E,), generator=g).numpy()
    err = torch.tensor([0, 17], dtype=torch.int32)
    cand = torch.zeros(B, L, dtype=torch.bool)
    tgt = torch.zeros(B, L, dtype=torch.bool)
    cand[:, [3, 17, 40, 99, 250]] = True
    tgt[1, [40, 120]] = True
    emb = 0.5 * torch.randn(B * L, D, generator=g)
    rel_edges, e_all, t_all = _edges_device(edges, ids, n_ids, B, L)
    x = emb.cuda().requires_grad_(True)
    m.reset_metrics()
    loss = m.loss_from_embedded(x, B, L, lens_att.cuda(), rel_edges, err.cuda(), cand.cuda(), tgt.cuda())
    loss.backward()
    # float64 CPU restatement with the same weights
    cfg = O.GreatConfig(d_model=D, num_heads=H, num_layers=layers, dim_feedforward=FF, num_edge_types=2 * n_ids, normalisation_mode="prenorm")
    p = {}
    for i, layer in enumerate(m.seq_layers):
        for ours, (ref, tr) in LAYER_PARAMS.items():
            v = getattr(layer, ours).detach().double().cpu()
            p[f"layers.{i}.{ref}"] = (v.T if tr else v).clone().requires_grad_(True)
    head = [t.detach().double().cpu().requires_grad_(True) for t in (m.ln_out_g, m.ln_out_b, m.predictions_W, m.predictions_b)]
    x64 = emb.double().requires_grad_(True)
    h = x64.reshape(B, L, D) + m.positional_encodings[:L].double().cpu()[None]
    masked = torch.arange(L)[None, :] >= lens_att.long()[:, None]
    h = O.encoder_stack(p, h, masked, torch.from_numpy(e_all), torch.from_numpy(t_all), cfg)
    _, loss64, _ = ref_head(h.reshape(B * L, D), *head, lens_att, err, cand, tgt, B, L)
    loss64.backward()
    assert abs(float(loss) - float(loss64)) < 1e-4 * abs(float(loss64))
    assert _rel(x.grad, x64.grad) < 1e-4
    scale = float(head[2].grad.abs().max())
    for t, ours in zip(head, ("ln_out_g", "ln_out_b", "predictions_W", "predictions_b")):
        sc = scale if ours in ("ln_out_b", "predictions_b") else 0.0
        assert _rel(getattr(m, ours).grad, t.grad, sc) < 1e-4, ours
    # the encoder layers' own weight gradients: 1e-3 (measured up to 3.7e-4, the last layer's lin1_W -- the existing layers'
    # split-product GEMMs summed over 1024 rows, ten layers deep); loss, input and head gradients above hold 1e-4
    for i, layer in enumerate(m.seq_layers):
        for ours, (ref, tr) in LAYER_PARAMS.items():
            want = p[f"layers.{i}.{ref}"].grad
            assert _rel(getattr(layer, ours).grad, want.T if tr else want) < 1e-3, (i, ours)


def _small_factory():
    from buglab.models.greatreimplementation import GreatVarMisuse

    cfg = {"num_layers": 2, "num_heads": 4, "intermediate_dimension": 128, "dropout_rate": 0.1, "rezero_mode": "off",
           "normalization_mode": "prenorm"}
    return GreatVarMisuse(cfg, vocab_size=256, embedding_dim=64, max_length=256)


def test_loss_falls_on_a_fixed_minibatch():
    from buglab.data.synthetic_great import make_great_records
    from buglab.runtime.optim import FlatAdam

    model = _small_factory()
    recs = make_great_records(24, seed=5)
    model.compute_metadata(recs)
    nn = model.build_neural_module().cuda().train()
    mb = model.finalize_minibatch({"samples": [model.tensorize(r) for r in recs]}, "cuda")
    opt = FlatAdam(nn.parameters(), lr=1e-3, clip_gradient_norm=0.25, num_warmup_steps=0)
    losses = []
    for _ in range(40):
        opt.zero_grad()
        loss = nn(**mb)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert all(math.isfinite(v) for v in losses)
    assert np.mean(losses[-5:]) < 0.6 * np.mean(losses[:3]), losses
    metrics = nn.report_metrics()
    assert metrics["Num samples"] == 40 * 24 and 0.0 <= metrics["Localization Accuracy"] <= 1.0


def test_traingreat_trains_and_checkpoint_restores(tmp_path):
    from buglab.data.synthetic_great import make_great_records, write_great_dir
    from buglab.models import traingreat
    from buglab.runtime.neuralmodel import AbstractNeuralModel

    write_great_dir(str(tmp_path / "train"), make_great_records(96, seed=11), per_file=32)
    write_great_dir(str(tmp_path / "valid"), make_great_records(40, seed=12), per_file=20)
    model_path = tmp_path / "great.pkl.gz"
    args = traingreat.parse_args([str(tmp_path / "train"), str(tmp_path / "valid"), str(model_path), "--max-num-epochs", "2",
                                  "--minibatch-size", "16", "--quiet"])
    best = traingreat.run(args, model_factory=_small_factory)
    assert model_path.exists() and math.isfinite(best)
    model, nn = AbstractNeuralModel.restore_model(model_path, torch.device("cuda:0"))
    nn.eval()
    nn.reset_metrics()
    total, n = 0.0, 0
    valid = list(traingreat.load_all_json_l_gz(str(tmp_path / "valid")))
    with torch.no_grad():
        for mb, _ in model.minibatch_iterator(model.tensorize_dataset(valid), "cuda", 16):
            total += float(nn(**mb))
            n += 1
    assert abs(total / n - best) < 1e-5 * max(1.0, abs(best))
    assert nn.report_metrics()["Num samples"] == 40
    # continue training from the checkpoint
    args2 = traingreat.parse_args([str(tmp_path / "train"), str(tmp_path / "valid"), str(tmp_path / "again.pkl.gz"), "--max-num-epochs",
                                   "1", "--minibatch-size", "16", "--quiet", "--restore-path", str(model_path)])
    assert math.isfinite(traingreat.run(args2))
