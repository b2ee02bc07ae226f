"""GPU: knowledge distillation on the MI355X -- the kernels of csrc/bl_distill.hip against the torch fp64 restatement of
tests/test_distill_host.py (evaluated here on the fp32 inputs), the soft-target term inside GnnBugLabModule, and teacher
annotation -> student training end to end.

Pool: see tests/test_distill_host.py (segment lengths across the 64-lane wave, permuted repair groups, one-hot / consensus /
all -inf teachers, B = 1, C = 0, G = 0, scores 40 N(0, 1) at tau = 0.5).

Tolerances, derived.  The kernels work in fp64 and round once to fp32 (relative 2^-24); the fp64 work on either side differs by
a few 1e-16 relative plus the order of a sum of a few hundred terms, orders of magnitude below that.  KL sums and delta:
|out - ref| <= 2^-23 |ref| + 1e-12.  Backward outputs: 2^-22 |ref| + 1e-12 (bound of three fp32 roundings: delta, / tau, * g; the
kernel makes two).  The integer counters are exact against the twin."""
import copy
import json
import math

import numpy as np
import pytest
import torch

from tests.guard_bands import guarded
from tests.test_distill_host import CASES, _log_softmax, case_of, taus_of, torch_reference

pytestmark = pytest.mark.gpu

DEV = "cuda"
G_LOC, G_REP = 0.7, -1.3  # upstream gradients of the two sums in the backward test


def _guarded_vec(a, dtype=torch.float32):
    """A 1-D operand inside a guard band whose padding is poisoned; a zero-length one is an ordinary empty tensor."""
    n = int(a.shape[0])
    if n == 0:
        return None, torch.zeros(0, dtype=dtype, device=DEV)
    g = guarded(1, n, ld=(n + 3) // 4 * 4, dtype=dtype, device=DEV, guard_rows=4)
    g.fill(torch.from_numpy(np.ascontiguousarray(a)).to(DEV)[None, :])
    return g, g.view[0]


def _out_vec(n):
    if n == 0:
        return None, torch.zeros(0, dtype=torch.float32, device=DEV)
    g = guarded(1, n, ld=(n + 3) // 4 * 4, dtype=torch.float32, device=DEV, guard_rows=4)
    return g, g.view[0]


_REFS = {}


def reference_of(key, tau):
    """The torch fp64 restatement and the twin, once per (case, tau)."""
    if (key, tau) not in _REFS:
        from buglab.models import _distill as K

        case = case_of(key)
        g = (float(np.float32(G_LOC)), float(np.float32(G_REP)))
        kl_loc, kl_rep, gs1, gl1, _ = torch_reference(case, tau)
        _, _, gs, gl, _ = torch_reference(case, tau, *g)
        twin = K.distill_terms(case["loc_scores"], case["logits"], case["teacher_loc"], case["teacher_rep"], case["cptr"], case["gptr"],
                               case["gitems"], tau)
        _REFS[(key, tau)] = {"kl": (kl_loc, kl_rep), "delta": np.concatenate([gs1, gl1]) * tau, "grads": (gs, gl), "twin": twin}
    return _REFS[(key, tau)]


@pytest.mark.parametrize("key", list(CASES))
def test_kernels_against_the_torch_restatement(key):
    from buglab.models import hip_ops

    case = case_of(key)
    Cn, R = case["loc_scores"].shape[0], case["logits"].shape[0]
    operands = [_guarded_vec(case[k]) for k in ("loc_scores", "logits", "teacher_loc", "teacher_rep")]
    scores, logits, tl, tr = (t for _, t in operands)
    cptr, gptr, gitems = (torch.from_numpy(case[k]).to(DEV) for k in ("cptr", "gptr", "gitems"))
    for tau in taus_of(key):
        ref = reference_of(key, tau)
        g_delta, delta = _out_vec(Cn + R)
        g_out, out = _out_vec(hip_ops.DISTILL_OUT)
        hip_ops.distill_fwd(scores, logits, tl, tr, cptr, gptr, gitems, tau, delta=delta, out=out)
        got, got_delta = out.cpu().numpy(), delta.cpu().numpy()
        for g in (g_delta, g_out):
            if g is not None:
                g.assert_untouched(f"distill_fwd {key} tau {tau}")
        for name, value, want in (("location KL", got[0], ref["kl"][0]), ("repair KL", got[1], ref["kl"][1])):
            bound = 2.0 ** -23 * abs(want) + 1e-12
            print(f"[distill] {key} tau {tau} {name}: device {value:.9g} reference {want:.17g} |d| {abs(float(value) - want):.3e} bound {bound:.3e}")
            assert abs(float(value) - want) <= bound, (key, tau, name)
        err = np.abs(got_delta.astype(np.float64) - ref["delta"])
        bound = 2.0 ** -23 * np.abs(ref["delta"]) + 1e-12
        print(f"[distill] {key} tau {tau} delta: worst |d| / bound {float((err / bound).max()) if err.size else 0.0:.3f}")
        assert not np.isnan(got_delta).any() and (err <= bound).all(), (key, tau)
        twin = ref["twin"]
        assert got[2:].tolist() == [twin.distilled_loc, twin.distilled_rep, twin.agreement, twin.skipped, 0.0, 0.0], (key, tau)
        if key == "no-candidates":
            assert got[0] == 0.0  # location segments without candidates: NO_BUG alone, q = p = 1
        # backward, into guarded gradient targets
        g_gs, gs = _out_vec(Cn)
        g_gl, gl = _out_vec(R)
        g_kl = torch.tensor([G_LOC, G_REP], dtype=torch.float32, device=DEV)
        hip_ops.distill_bwd(delta, Cn, g_kl, tau, g_loc_scores=gs, g_logits=gl)
        for g in (g_gs, g_gl, g_delta):
            if g is not None:
                g.assert_untouched(f"distill_bwd {key} tau {tau}")
        for name, value, want in (("g_loc_scores", gs.cpu().numpy(), ref["grads"][0]), ("g_repair_logits", gl.cpu().numpy(), ref["grads"][1])):
            err = np.abs(value.astype(np.float64) - want)
            bound = 2.0 ** -22 * np.abs(want) + 1e-12
            print(f"[distill] {key} tau {tau} {name}: worst |d| / bound {float((err / bound).max()) if err.size else 0.0:.3f}")
            assert not np.isnan(value).any() and (err <= bound).all(), (key, tau, name)
        # two runs: bit-equal
        delta2, out2 = hip_ops.distill_fwd(scores, logits, tl, tr, cptr, gptr, gitems, tau)
        assert out2.cpu().numpy().tobytes() == got.tobytes() and delta2.cpu().numpy().tobytes() == got_delta.tobytes()
    for g, _ in operands:
        if g is not None:
            g.assert_untouched(f"distill operands {key}")


def _index(cptr, gptr, gitems):
    from buglab.models import hip_ops

    none = torch.zeros(0, dtype=torch.int32, device=DEV)
    return hip_ops.BugLossIndex(none, none, cptr, torch.zeros(cptr.shape[0] - 1, dtype=torch.bool, device=DEV), none, gptr, gitems,
                                (none, none, none), (none, none, none), int(gptr.shape[0]) - 1)


def test_operator_is_differentiable_once():
    from buglab.models import hip_ops

    case = case_of("mixed")
    tau = 2.0
    ref = reference_of("mixed", tau)
    to = lambda k: torch.from_numpy(case[k]).to(DEV)
    scores, logits = to("loc_scores").requires_grad_(), to("logits").requires_grad_()
    ix = _index(to("cptr"), to("gptr"), to("gitems"))
    kl, stats = hip_ops.distill_loss(scores, logits, to("teacher_loc"), to("teacher_rep"), ix, tau)
    assert kl.shape == (2,) and stats.shape == (6,) and kl.requires_grad and not stats.requires_grad
    loss = float(np.float32(G_LOC)) * kl[0] + float(np.float32(G_REP)) * kl[1]
    loss.backward(retain_graph=True)
    for got, want in ((scores.grad, ref["grads"][0]), (logits.grad, ref["grads"][1])):
        assert (np.abs(got.cpu().numpy().astype(np.float64) - want) <= 2.0 ** -22 * np.abs(want) + 1e-12).all()
    with pytest.raises(RuntimeError, match="second backward"):
        loss.backward()
    with pytest.raises(ValueError, match="teacher_loc"):
        hip_ops.distill_loss(scores, logits, to("teacher_loc")[:-1], to("teacher_rep"), ix, tau)
    with pytest.raises(RuntimeError, match="temperature"):
        hip_ops.distill_loss(scores, logits, to("teacher_loc"), to("teacher_rep"), ix, 0.0)


# ---- the term inside the module -------------------------------------------------------------------------------------------
def _minibatch(ncand):
    from buglab.data.collate import collate_samples, to_device
    from buglab.data.synthetic import make_samples

    return to_device(collate_samples(make_samples(7, seed=21, num_nodes=max(90, 2 * ncand), num_messages=400, num_edge_types=5, vocab_size=300,
                                                  num_candidates=ncand), 5), DEV)


def _teacher_arrays(mb, seed=8):
    """Random normalised teacher distributions over the minibatch's own location segments and repair groups; the first location
    segment has one entry at -inf."""
    rng = np.random.default_rng(seed)
    cptr = mb["graph_data"]["candidate_ptr"].cpu().numpy()
    gptr, gitems = mb["repair_group_ptr"].cpu().numpy(), mb["repair_group_items"].cpu().numpy()
    B, Cn, R = cptr.shape[0] - 1, int(cptr[-1]), gitems.shape[0]
    tl, tr = np.zeros(Cn + B, np.float32), np.zeros(R, np.float32)
    for b in range(B):
        x = 2.0 * rng.standard_normal(cptr[b + 1] - cptr[b] + 1)
        if b == 0:
            x[1] = -np.inf
        t = _log_softmax(x).astype(np.float32)
        tl[cptr[b]:cptr[b + 1]], tl[Cn + b] = t[:-1], t[-1]
    for g in range(gptr.shape[0] - 1):
        n = gptr[g + 1] - gptr[g]
        if n:
            tr[gitems[gptr[g]:gptr[g + 1]]] = _log_softmax(2.0 * rng.standard_normal(n)).astype(np.float32)
    assert R > 0
    return {"teacher_loc_logprobs": torch.from_numpy(tl).to(DEV), "teacher_repair_logprobs": torch.from_numpy(tr).to(DEV)}


def _module(w_buggy=1.0):
    from buglab.models.gnn import build_gnn_mlp_module

    torch.manual_seed(4)
    return build_gnn_mlp_module(64, 4, 5, vocabulary_size=300, dropout_rate=0.0, buggy_samples_weight=w_buggy).to(DEV).train()


def _step(module, mb, **extra):
    from buglab.models import hip_ops

    module.zero_grad(set_to_none=True)
    loss = module(**mb, dropout_seed=3, **extra)
    loss.backward()
    hip_ops.join_side_stream()
    torch.cuda.synchronize()
    return loss.detach().clone(), {k: p.grad.clone() for k, p in module.named_parameters()}


def _scores_and_logits(module, mb, with_sizes=False):
    """The module's own localization scores and cat(text, var, swap) logits, as _forward_fused_loss computes them."""
    gd = mb["graph_data"]
    out = module._compute_gnn_output(gd, 3)
    h, refs = module._head_inputs(out)
    scores = module._localization_module.compute_localization_scores(
        h, refs["candidate_nodes"], out.node_graph_idx_reference["candidate_nodes"], mb["has_bug"].shape[0], gd["candidate_ptr"])
    parts = module._repair_logits(out, mb["target_rewrites"])
    logits = torch.cat(parts)
    return (scores, logits, tuple(int(p.shape[0]) for p in parts)) if with_sizes else (scores, logits)


def test_weight_zero_and_eval_mode_change_nothing():
    """lambda = 0 with the arrays present: the same launches as without them, so loss and gradients are torch.equal -- compared in
    the library's deterministic mode, the only one in which two runs of ONE configuration are bit-identical (free-running atomics
    in the weight gradients otherwise).  lambda > 0 in eval(): the term is skipped."""
    from buglab.models import hip_ops

    hip_ops.set_deterministic(True)
    try:
        mb = _minibatch(9)
        teacher = _teacher_arrays(mb)
        plain_loss, plain_grads = _step(_module(), mb)
        module = _module()
        module.set_distillation(0.0, 2.0)
        loss, grads = _step(module, mb, **teacher)
        counts = []
        for extra in (teacher, {}):  # (after the first step, which also packs the weights)
            calls = hip_ops.CALL_COUNT
            _step(module, mb, **extra)
            counts.append(hip_ops.CALL_COUNT - calls)
        assert counts[0] == counts[1]  # nothing more is launched
        assert torch.equal(loss, plain_loss)
        for k, g in grads.items():
            assert torch.equal(g, plain_grads[k]), k
        assert "Teacher agreement" not in module.report_metrics()
        module.set_distillation(0.3, 2.0)
        module.eval()
        with torch.no_grad():
            assert torch.equal(module(**mb, **teacher), _module().eval()(**mb))
            module(**mb)  # validation data need no annotation
        assert "Teacher agreement" not in module.report_metrics()
    finally:
        hip_ops.set_deterministic(False)


@pytest.mark.parametrize("w_buggy,ncand", [(1.0, 9), (2.5, 9), (2.5, 90)])
def test_training_loss_and_gradients_with_the_soft_targets(w_buggy, ncand):
    from buglab.models import _distill as K
    from buglab.models import hip_ops

    lam, tau = 0.3, 2.0
    mb = _minibatch(ncand)
    teacher = _teacher_arrays(mb)
    B = int(mb["has_bug"].shape[0])
    l_hard, _ = _step(_module(w_buggy), mb)
    module = _module(w_buggy)
    module.set_distillation(lam, tau)
    loss, grads = _step(module, mb, **teacher)
    metrics = module.report_metrics()

    # the loss: L_hard of the plain run, KL from the twin on the module's own scores
    with torch.no_grad():
        scores, logits = _scores_and_logits(module, mb)
    cptr, gptr, gitems = (t.cpu().numpy() for t in (mb["graph_data"]["candidate_ptr"], mb["repair_group_ptr"], mb["repair_group_items"]))
    twin = K.distill_terms(scores.cpu().numpy(), logits.cpu().numpy(), teacher["teacher_loc_logprobs"].cpu().numpy(),
                           teacher["teacher_repair_logprobs"].cpu().numpy(), cptr, gptr, gitems, tau)
    want = (1.0 - lam) * float(l_hard) + lam * tau * tau * (twin.kl_loc / B + w_buggy * twin.kl_rep / B)
    print(f"[distill] module w_buggy {w_buggy} ncand {ncand}: loss {float(loss):.9g} expected {want:.9g} (hard {float(l_hard):.9g}, "
          f"KL {twin.kl_loc:.6g} / {twin.kl_rep:.6g})")
    assert twin.kl_loc > 0 and twin.kl_rep > 0
    assert abs(float(loss) - want) <= 1e-6 * max(1.0, abs(want))
    assert metrics["Distillation KL (localization)"] == pytest.approx(twin.kl_loc / B, rel=1e-5)
    assert metrics["Distillation KL (repair)"] == pytest.approx(twin.kl_rep / twin.distilled_rep, rel=1e-5)
    assert metrics["Teacher agreement"] == twin.agreement / B
    module.reset_metrics()
    assert module.report_metrics() == {}

    # the gradients: the same loss from torch ops on the device, through the same module
    ref_module = _module(w_buggy)
    ref_module.zero_grad(set_to_none=True)
    scores, logits, sizes = _scores_and_logits(ref_module, mb, with_sizes=True)
    gd = mb["graph_data"]
    ix = hip_ops.BugLossIndex(gd["loc_group_ptr"], gd["loc_group_items"], gd["candidate_ptr"], mb["has_bug"], mb["correct_candidate_node_idxs"],
                              mb["repair_group_ptr"], mb["repair_group_items"],
                              (mb["rewrite_to_location_group"], mb["candidate_symbol_to_location_group"], mb["swapped_pair_to_call_location_group"]),
                              (mb["correct_rewrite_idxs"], mb["correct_candidate_symbols"], mb["correct_swapped_pair"]),
                              int(mb["repair_group_ptr"].shape[0]) - 1)
    hard, _ = hip_ops.bug_loss(scores, logits, sizes, ix, w_buggy, ref_module._localization_module._abstain_weight)  # L_hard, as the module assembles it
    assert abs(float(hard) - float(l_hard)) <= 1e-6 * max(1.0, abs(float(l_hard)))
    tl, tr = teacher["teacher_loc_logprobs"].double(), teacher["teacher_repair_logprobs"].double()
    Cn = scores.shape[0]

    def seg_kl(z, t):
        keep = t > -float("inf")
        lq = torch.log_softmax(z.double() / tau, dim=0)
        lp = torch.log_softmax(t[keep] / tau, dim=0)
        return (lp.exp() * (lp - lq[keep])).sum()

    one = torch.ones(1, dtype=torch.float32, device=DEV)
    kl_loc = sum(seg_kl(torch.cat([scores[cptr[b]:cptr[b + 1]], one]), torch.cat([tl[cptr[b]:cptr[b + 1]], tl[Cn + b:Cn + b + 1]])) for b in range(B))
    items = torch.from_numpy(gitems.astype(np.int64)).to(DEV)
    kl_rep = sum(seg_kl(logits[items[gptr[g]:gptr[g + 1]]], tr[items[gptr[g]:gptr[g + 1]]]) for g in range(len(gptr) - 1) if gptr[g + 1] > gptr[g])
    ref_loss = (1.0 - lam) * hard + (lam * tau * tau * (kl_loc / B + w_buggy * kl_rep / B)).float()
    ref_loss.backward()
    hip_ops.join_side_stream()
    torch.cuda.synchronize()
    assert abs(float(ref_loss) - float(loss)) <= 1e-6 * max(1.0, abs(float(ref_loss)))
    for k, p in ref_module.named_parameters():
        ref = p.grad
        worst = float((grads[k] - ref).abs().max())
        assert worst <= 2e-5 * float(ref.abs().max()) + 1e-8, (k, worst, float(ref.abs().max()))


def test_training_with_the_term_on_needs_the_arrays_and_the_fused_path():
    from buglab.models import hip_ops

    mb = _minibatch(9)
    module = _module()
    module.set_distillation(0.3, 2.0)
    with pytest.raises(ValueError, match="annotated by buglab.models.distill and a graph student"):
        module(**mb, dropout_seed=3)
    hip_ops.FUSED_LOSS = False
    try:
        with pytest.raises(NotImplementedError, match="fused-loss path"):
            module(**mb, dropout_seed=3, **_teacher_arrays(mb))
    finally:
        hip_ops.FUSED_LOSS = True


# ---- end to end -----------------------------------------------------------------------------------------------------------
def _location_groups(record):
    """{reference node: the original indices of the rewrites whose `predict` values are that location group's}.  The rule is
    `PredictionLayout`'s (reference basemodel.py:240-346): within a scout family (text / var-misuse / arg-swap) the k-th rewrite
    in first-seen-location order takes the k-th value of the family's entries ordered by location.  Where a family's rewrites
    come in ascending node order -- the graph data here -- that is simply "the rewrites at the node"."""
    refs = record["graph"]["reference_nodes"]
    family = lambda scout: {"VariableMisuseRewriteScout": "var", "ArgSwapRewriteScout": "swap"}.get(scout, "text")
    groups = {}
    for fam in ("text", "var", "swap"):
        by_node = {}
        for i, (scout, _) in enumerate(record["candidate_rewrite_metadata"]):
            if family(scout) == fam:
                by_node.setdefault(refs[i], []).append(i)
        original = [i for idxs in by_node.values() for i in idxs]                     # first-seen-location order
        owner = [node for node in sorted(by_node) for _ in by_node[node]]             # the entries, ordered by location
        for i, node in zip(original, owner):
            groups.setdefault(node, []).append(i)
    return groups


def _check_annotation(records, expect):
    assert len(records) == expect
    for r in records:
        nodes = np.unique(r["graph"]["reference_nodes"]).tolist()
        assert list(r["teacher_location_nodes"]) == nodes + [-1]
        loc, rw = np.asarray(r["teacher_location_logprobs"], np.float64), np.asarray(r["teacher_rewrite_logprobs"], np.float64)
        assert loc.shape == (len(nodes) + 1,) and rw.shape == (len(r["candidate_rewrites"]),)
        assert (loc.astype(np.float32) == loc).all() and (rw.astype(np.float32) == rw).all() and not np.isnan(loc).any()
        lse = lambda v: float(np.log(np.exp(v[v > -np.inf]).sum()))
        assert abs(lse(loc)) <= 1e-5
        for node, at in _location_groups(r).items():  # each location group's rewrites are a distribution
            assert abs(lse(rw[at])) <= 1e-5, node


def _train(model, path, data, valid, *, epochs=10, distillation=None, seed=0):
    from buglab.runtime.optim import FlatAdam
    from buglab.runtime.trainer import ModelTrainer

    trainer = ModelTrainer(model, path, max_num_epochs=epochs, minibatch_size=8, distillation=distillation,
                           optimizer_creator=lambda params: FlatAdam(params, lr=1e-3, num_warmup_steps=0))
    torch.manual_seed(seed)
    np.random.seed(seed)
    return trainer


@pytest.fixture(scope="module")
def taught(tmp_path_factory):
    """A tiny gnn-mlp teacher (the SPECS of tests/test_calibrate_gpu.py, 24 synthetic samples, 30 Adam steps at 1e-3 without
    warm-up) and the 24 records annotated by it."""
    from buglab.data.synthetic import make_buglab_dataset
    from buglab.models import distill
    from buglab.models.modelregistry import load_model
    from buglab.runtime.neuralmodel import AbstractNeuralModel
    from tests.test_calibrate_gpu import SPECS

    root = tmp_path_factory.mktemp("distill")
    data = make_buglab_dataset(24, seed=41)
    path = root / "teacher.pkl.gz"
    model = load_model(dict(SPECS["gnn-mlp"], modelName="gnn-mlp"), path)[0]
    _train(model, path, data, data).train(copy.deepcopy(data), copy.deepcopy(data[:8]), show_progress_bar=False, parallelize=False, patience=100)
    model, nn_ = AbstractNeuralModel.restore_model(path, torch.device(DEV))
    report = {}
    records = list(distill.annotate_with_teacher(model, nn_, copy.deepcopy(data), torch.device(DEV), False, report))
    return {"root": root, "data": data, "teacher": path, "records": records, "report": report, "specs": SPECS}


def test_teacher_annotates_every_record(taught):
    _check_annotation(taught["records"], 24)
    assert taught["report"]["records_in"] == taught["report"]["records_out"] == 24 and taught["report"]["records_dropped"] == 0
    assert taught["report"]["records_with_unnormalised_rewrite_groups"] == 0  # every family's rewrites come in ascending node order
    # the records are the input records plus the three keys: the teacher's own additions to the graph are not written
    for r, d in zip(taught["records"], taught["data"]):
        assert {k: v for k, v in r.items() if not k.startswith("teacher_")} == d


def test_annotation_cli_and_a_sequence_teacher(taught, tmp_path, capsys):
    from buglab.data.synthetic import make_buglab_seq_dataset
    from buglab.models import distill
    from buglab.models.modelregistry import load_model
    from buglab.utils.msgpackutils import load_msgpack_l_gz, save_msgpack_l_gz

    (tmp_path / "in").mkdir()
    save_msgpack_l_gz(taught["data"][:16], tmp_path / "in" / "a.msgpack.l.gz")
    save_msgpack_l_gz(taught["data"][16:], tmp_path / "in" / "b.msgpack.l.gz")
    rep = tmp_path / "report.json"
    report = distill.main([str(taught["teacher"]), str(tmp_path / "in"), str(tmp_path / "out"), "--sequential", "--report-json", str(rep)])
    text = capsys.readouterr().out
    assert "Annotated 24 of 24 records in 2 shard(s)" in text and "mean teacher entropy" in text
    assert json.loads(rep.read_text())["records_out"] == 24 and report["records_dropped"] == 0 and report["mean_location_entropy"] > 0
    back = [r for name in ("a", "b") for r in load_msgpack_l_gz(tmp_path / "out" / f"{name}.msgpack.l.gz", native=False)]
    _check_annotation(back, 24)
    for r, mine in zip(back, taught["records"]):  # the same teacher, through files
        assert np.allclose(r["teacher_location_logprobs"], mine["teacher_location_logprobs"], rtol=0, atol=1e-5)
    with pytest.raises(ValueError, match="overwrite"):
        distill.main([str(taught["teacher"]), str(tmp_path / "in"), str(tmp_path / "in"), "--sequential"])

    # a sequence teacher (untrained: its distributions are distributions all the same)
    seq_data = make_buglab_seq_dataset(24, seed=41)
    model = load_model(dict(taught["specs"]["seq-great"], modelName="seq-great"), tmp_path / "seq.pkl.gz")[0]
    model.compute_metadata(copy.deepcopy(seq_data))
    torch.manual_seed(0)
    nn_ = model.build_neural_module().to(DEV)
    report = {}
    records = list(distill.annotate_with_teacher(model, nn_, copy.deepcopy(seq_data), torch.device(DEV), False, report))
    _check_annotation(records, report["records_out"])
    assert report["records_out"] + report["records_dropped"] == 24 and report["records_out"] > 0
    # the synthetic sequence records list a family's rewrites out of node order: `predict`'s family rule shows, and is reported
    by_node = lambda r: all(sorted(at) == [i for i, n in enumerate(r["graph"]["reference_nodes"]) if n == node]
                            for node, at in _location_groups(r).items())
    assert report["records_with_unnormalised_rewrite_groups"] >= 1
    assert report["records_with_unnormalised_rewrite_groups"] <= sum(not by_node(r) for r in records)


def test_consensus_teacher_and_one_training_step(taught, tmp_path):
    from buglab.data.collate import collate_samples, to_device
    from buglab.models import distill
    from buglab.models.ensemble.wrapper import EnsembleModuleWrapper, EnsembleWrapper
    from buglab.models.modelregistry import load_model
    from buglab.runtime.neuralmodel import AbstractNeuralModel

    data = taught["data"]
    # two copies of the trained teacher that disagree by construction: the localization score is w . sigmoid(...), 32 terms in
    # (0, 1), against NO_BUG's constant logit 1.0 -- with w = -5 every candidate scores below it, with w = +5 one scores above it
    members = [AbstractNeuralModel.restore_model(taught["teacher"], torch.device(DEV)) for _ in range(2)]
    for (_, nn_), value in zip(members, (-5.0, 5.0)):
        with torch.no_grad():
            nn_._localization_module.w.fill_(value)
    ensemble = EnsembleWrapper([m for m, _ in members], "consensus")
    nns = EnsembleModuleWrapper([nn_ for _, nn_ in members]).to(DEV)
    records = list(distill.annotate_with_teacher(ensemble, nns, copy.deepcopy(data), torch.device(DEV), False))
    _check_annotation(records, 24)
    disagreeing = [r for r in records if all(v == -math.inf for v in r["teacher_location_logprobs"][:-1])]
    agreeing = [r for r in records if r not in disagreeing]
    print(f"[distill] consensus teacher: {len(disagreeing)} of 24 samples without consensus")
    assert disagreeing and all(r["teacher_location_logprobs"][-1] == 0.0 for r in disagreeing)
    # one training step of a student on them
    student = load_model(dict(taught["specs"]["gnn-mlp"], modelName="gnn-mlp"), tmp_path / "student.pkl.gz")[0]
    student.compute_metadata(copy.deepcopy(data))
    torch.manual_seed(1)
    nn_ = student.build_neural_module().to(DEV).train()
    nn_.set_distillation(0.5, 2.0)
    samples = [student.tensorize(r) for r in records]
    mb = to_device(collate_samples(samples, student.gnn_model.num_presented_edge_types), DEV)
    loss = nn_(**mb)
    loss.backward()
    torch.cuda.synchronize()
    assert math.isfinite(float(loss))
    assert all(torch.isfinite(p.grad).all() for p in nn_.parameters() if p.grad is not None)
    assert len(agreeing) + len(disagreeing) == 24


def _mean_location_kl(model, nn_, records):
    from buglab.models import _distill as K

    total, n = 0.0, 0
    plain = [{k: v for k, v in r.items() if not k.startswith("teacher_")} for r in copy.deepcopy(records)]
    for (point, loc, _), r in zip(model.predict(iter(plain), nn_, torch.device(DEV), False), records):
        assert point["graph"]["reference_nodes"] == r["graph"]["reference_nodes"]
        student = [loc[n_] for n_ in r["teacher_location_nodes"]]
        total += K.location_kl(r["teacher_location_logprobs"], student, 1.0)
        n += 1
    assert n == len(records)
    return total / n


def test_student_moves_towards_its_teacher(taught, tmp_path):
    """A gnn-mlp student with another seed, trained on the annotated records through ModelTrainer(distillation=(1.0, 2.0)) and
    validated on un-annotated ones: its mean per-sample location KL to the teacher (twin, tau = 1, from `predict`) is strictly
    smaller after training than at its initialisation.  Measured on an MI355X: see BASELINE.md."""
    from buglab.models.modelregistry import load_model
    from buglab.runtime.neuralmodel import AbstractNeuralModel

    records, data = taught["records"], taught["data"]
    path = tmp_path / "student.pkl.gz"
    student = load_model(dict(taught["specs"]["gnn-mlp"], modelName="gnn-mlp"), path)[0]
    trainer = _train(student, path, records, data, distillation=(1.0, 2.0), seed=1)
    trainer.load_metadata_and_create_network(copy.deepcopy(records), False, False)
    trainer.neural_module = trainer.neural_module.to(DEV)
    before = _mean_location_kl(student, trainer.neural_module, records)
    seen = []
    trainer.register_train_epoch_end_hook(lambda model, nn_, epoch, metrics: seen.append(metrics))
    trainer.train(copy.deepcopy(records), copy.deepcopy(data[:8]), show_progress_bar=False, initialize_metadata=False, parallelize=False,
                  patience=100)
    nn_ = trainer.neural_module
    assert nn_.distillation == (0.0, 1.0)  # the trainer's setting ends with the training
    after = _mean_location_kl(student, nn_, records)
    print(f"[distill] student's mean location KL to the teacher: {before:.6f} at initialisation -> {after:.6f} after 30 steps")
    assert after < before
    assert len(seen) == 10 and all({"Distillation KL (localization)", "Distillation KL (repair)", "Teacher agreement"} <= set(m) for m in seen)
    assert seen[-1]["Distillation KL (localization)"] < seen[0]["Distillation KL (localization)"]
    # the saved student is an ordinary checkpoint
    model, restored = AbstractNeuralModel.restore_model(path, torch.device(DEV))
    assert restored.distillation == (0.0, 1.0)
    assert len(list(model.predict(iter(copy.deepcopy(data[:4])), restored, torch.device(DEV), False))) == 4


def test_train_cli_with_distillation(taught, tmp_path):
    from buglab.models import evaluate, train
    from buglab.utils.msgpackutils import save_msgpack_l_gz

    (tmp_path / "train").mkdir()
    (tmp_path / "valid").mkdir()
    save_msgpack_l_gz(taught["records"][:12], tmp_path / "train" / "a.msgpack.l.gz")
    save_msgpack_l_gz(taught["records"][12:], tmp_path / "train" / "b.msgpack.l.gz")
    save_msgpack_l_gz(taught["data"][:8], tmp_path / "valid" / "v.msgpack.l.gz")  # un-annotated
    model_path = tmp_path / "student.pkl.gz"
    train.run(train.parse_args(["gnn-mlp", str(tmp_path / "train"), str(tmp_path / "valid"), str(model_path), "--distill-weight", "0.5",
                                "--distill-temperature", "2", "--sequential", "--max-num-epochs", "1", "--minibatch-size", "8", "--quiet",
                                "--model-spec", json.dumps(taught["specs"]["gnn-mlp"])]))
    assert model_path.exists()
    metrics = evaluate.run({"MODEL_FILENAME": str(model_path), "TEST_DATA_PATH": str(tmp_path / "valid"), "--assume-buggy": False,
                            "--eval-only-no-bug": False, "--limit-num-elements": None, "--sequential": True})
    assert metrics["num_samples"] == 8
