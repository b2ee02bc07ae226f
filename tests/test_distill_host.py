"""Host (no GPU): knowledge distillation -- the NumPy twin of csrc/bl_distill.hip against a torch fp64 autograd restatement, the
teacher targets' way through tensorize / collate / pack / upload and through both msgpack readers, and the switches.

The pool (shared with tests/test_distill_gpu.py).  Location segments with 0, 1, 62, 63, 64, 65, 127, 128 and 200 candidates in
one minibatch: with the NO_BUG item the lengths cross a wave at 63 -> 64.  Repair groups of 1, 2, 63, 64, 65, 129 and 300 items
whose places are a permutation of the logits (interleaved across the text | var | swap slices).  Teachers: random normalised
log-probabilities; one-hot (one 0, the rest -inf); `consensus`-style (every candidate -inf, NO_BUG 0); all -inf (skipped and
counted).  Scores 3 N(0, 1), and 40 N(0, 1) at tau = 0.5, where exp(z / tau) itself would overflow without the shift."""
import copy
import pickle
from pathlib import Path

import numpy as np
import pytest
import torch

from buglab.data import collate as C

CANDIDATES = (0, 1, 62, 63, 64, 65, 127, 128, 200)
GROUPS = (1, 2, 63, 64, 65, 129, 300)
TAUS = (0.5, 1.0, 2.0, 4.0)


def _log_softmax(x):
    x = np.asarray(x, np.float64)
    m = x.max()
    return x - m - np.log(np.exp(x - m).sum())


def _teacher(rng, n, kind, nobug_last):
    """n teacher log-probabilities in fp32: 'random' | 'onehot' | 'consensus' (needs nobug_last) | 'skip' (all -inf)."""
    if kind == "random":
        return _log_softmax(2.0 * rng.standard_normal(n)).astype(np.float32)
    t = np.full(n, -np.inf, np.float32)
    if kind == "onehot":
        t[int(rng.integers(0, n))] = 0.0
    elif kind == "consensus":
        assert nobug_last
        t[-1] = 0.0
    return t


def make_case(name, candidates=CANDIDATES, groups=GROUPS, seed=0, scale=3.0):
    """-> dict of NumPy arrays: loc_scores [C], logits [R], teacher_loc [C + B], teacher_rep [R], cptr [B + 1], gptr [G + 1],
    gitems [R].  name: 'random' | 'onehot' | 'mixed' (segments cycle random, one-hot, consensus, all -inf; groups cycle random,
    one-hot, all -inf)."""
    rng = np.random.default_rng(seed)
    B, G = len(candidates), len(groups)
    cptr = np.zeros(B + 1, np.int32)
    np.cumsum(candidates, out=cptr[1:])
    gptr = np.zeros(G + 1, np.int32)
    np.cumsum(groups, out=gptr[1:])
    Cn, R = int(cptr[-1]), int(gptr[-1])
    loc_kinds = {"random": ["random"], "onehot": ["onehot"], "mixed": ["random", "onehot", "consensus", "skip"]}[name]
    rep_kinds = {"random": ["random"], "onehot": ["onehot"], "mixed": ["random", "onehot", "skip"]}[name]
    teacher_loc = np.zeros(Cn + B, np.float32)
    for b, n in enumerate(candidates):
        t = _teacher(rng, n + 1, loc_kinds[b % len(loc_kinds)], True)
        teacher_loc[cptr[b]:cptr[b + 1]] = t[:-1]
        teacher_loc[Cn + b] = t[-1]
    gitems = rng.permutation(R).astype(np.int32)  # group g owns gitems[gptr[g] : gptr[g + 1]]
    teacher_rep = np.zeros(R, np.float32)
    for g, n in enumerate(groups):
        teacher_rep[gitems[gptr[g]:gptr[g + 1]]] = _teacher(rng, n, rep_kinds[g % len(rep_kinds)], False)
    return {"loc_scores": (scale * rng.standard_normal(Cn)).astype(np.float32), "logits": (scale * rng.standard_normal(R)).astype(np.float32),
            "teacher_loc": teacher_loc, "teacher_rep": teacher_rep, "cptr": cptr, "gptr": gptr, "gitems": gitems}


CASES = {
    "random": dict(name="random", seed=1),
    "onehot": dict(name="onehot", seed=2),
    "mixed": dict(name="mixed", seed=3),
    "hot": dict(name="mixed", seed=4, scale=40.0),                      # run at tau = 0.5 only
    "no-groups": dict(name="random", groups=(), seed=5),                 # G = 0, R = 0
    "one-graph": dict(name="random", candidates=(65,), groups=(3,), seed=6),   # B = 1
    "no-candidates": dict(name="mixed", candidates=(0, 0, 0), groups=(2, 5), seed=7),  # C = 0
}
_CASES = {}


def case_of(key):
    if key not in _CASES:
        _CASES[key] = make_case(**CASES[key])
    return _CASES[key]


def taus_of(key):
    return (0.5,) if key == "hot" else TAUS


def torch_reference(case, tau, g_loc=1.0, g_rep=1.0):
    """The torch fp64 restatement on the fp32 inputs: log_softmax per segment, kl_div over the teacher's support.
    -> (kl_loc, kl_rep, d(g_loc kl_loc + g_rep kl_rep) / d loc_scores, ... / d logits, per-segment KLs), float64."""
    F = torch.nn.functional
    s = torch.tensor(case["loc_scores"], dtype=torch.float64, requires_grad=True)
    l = torch.tensor(case["logits"], dtype=torch.float64, requires_grad=True)
    tl = torch.tensor(case["teacher_loc"], dtype=torch.float64)
    tr = torch.tensor(case["teacher_rep"], dtype=torch.float64)
    cptr, gptr, gitems = case["cptr"], case["gptr"], torch.tensor(case["gitems"], dtype=torch.int64)
    Cn = s.shape[0]

    def seg(z, t):
        keep = t > -float("inf")
        if not bool(keep.any()):
            return z.sum() * 0.0
        lq = F.log_softmax(z / tau, dim=0)
        lp = F.log_softmax(t[keep] / tau, dim=0)
        return F.kl_div(lq[keep], lp, reduction="sum", log_target=True)

    one = torch.ones(1, dtype=torch.float64)
    kls = [seg(torch.cat([s[cptr[b]:cptr[b + 1]], one]), torch.cat([tl[cptr[b]:cptr[b + 1]], tl[Cn + b:Cn + b + 1]]))
           for b in range(len(cptr) - 1)]
    klr = [seg(l[gitems[gptr[g]:gptr[g + 1]]], tr[gitems[gptr[g]:gptr[g + 1]]]) for g in range(len(gptr) - 1)]
    zero = s.sum() * 0.0 + l.sum() * 0.0
    kl_loc = torch.stack(kls).sum() if kls else zero
    kl_rep = torch.stack(klr).sum() if klr else zero
    (g_loc * kl_loc + g_rep * kl_rep + zero).backward()
    return (float(kl_loc.detach()), float(kl_rep.detach()), s.grad.numpy(), l.grad.numpy(), np.asarray([float(k.detach()) for k in kls + klr]))


@pytest.mark.parametrize("key", list(CASES))
def test_twin_against_torch_autograd(key):
    from buglab.models import _distill as K

    case = case_of(key)
    Cn = case["loc_scores"].shape[0]
    for tau in taus_of(key):
        out = K.distill_terms(case["loc_scores"], case["logits"], case["teacher_loc"], case["teacher_rep"], case["cptr"], case["gptr"],
                              case["gitems"], tau)
        kl_loc, kl_rep, gs, gl, seg = torch_reference(case, tau)
        close = lambda a, b: np.all(np.abs(np.asarray(a) - np.asarray(b)) <= 1e-12 * np.abs(b) + 1e-15)
        assert close(out.kl_loc, kl_loc) and close(out.kl_rep, kl_rep), (key, tau, out.kl_loc, kl_loc, out.kl_rep, kl_rep)
        assert close(out.seg_kl, seg)
        assert close(out.delta[:Cn] / tau, gs) and close(out.delta[Cn:] / tau, gl), (key, tau)
        assert (out.seg_kl >= -1e-15).all()
    # the counters, by hand
    B, G = len(case["cptr"]) - 1, len(case["gptr"]) - 1
    assert out.distilled_loc + out.distilled_rep + out.skipped == B + G
    if CASES[key]["name"] == "mixed":
        assert out.skipped == sum(b % 4 == 3 for b in range(B)) + sum(g % 3 == 2 for g in range(G))
        # consensus-style and all -inf segments leave their candidates a delta of q (p = 0) and of 0
        b = 3 if B > 3 else None
        if b is not None:
            assert (out.delta[case["cptr"][b]:case["cptr"][b + 1]] == 0).all() and out.seg_kl[b] == 0.0
    else:
        assert out.skipped == 0
    if key == "no-candidates":
        # NO_BUG alone: q = 1; KL is exactly 0 where the teacher's NO_BUG has a probability
        assert out.kl_loc == 0.0 and out.seg_kl[:B].tolist() == [0.0] * B
    g0, g1 = K.distill_grads(out.delta.astype(np.float32), Cn, 0.25, -3.0, 2.0)
    assert g0.dtype == np.float32 and np.allclose(g0, 0.25 * out.delta[:Cn] / 2.0, rtol=1e-6, atol=1e-12)
    assert np.allclose(g1, -3.0 * out.delta[Cn:] / 2.0, rtol=1e-6, atol=1e-12)


def test_twin_helpers():
    from buglab.models import _distill as K

    lp = _log_softmax([0.3, -1.0, 2.0])
    assert K.location_kl(lp, lp) == pytest.approx(0.0, abs=1e-15)
    assert K.location_kl(lp, lp + 7.0, tau=2.0) == pytest.approx(0.0, abs=1e-15)  # shift-invariant in the student
    assert K.location_kl([0.0, -np.inf], np.log([0.5, 0.5])) == pytest.approx(np.log(2.0), rel=1e-15)
    assert K.entropy(np.log([0.5, 0.5])) == pytest.approx(np.log(2.0)) and K.entropy([0.0, -np.inf]) == 0.0
    with pytest.raises(ValueError, match="teacher_loc"):
        K.distill_terms(np.zeros(2), np.zeros(0), np.zeros(2), np.zeros(0), [0, 2], [0], [], 1.0)


# ---- the data path --------------------------------------------------------------------------------------------------------
def _model(where=None):
    import tempfile

    from buglab.models.modelregistry import load_model

    where = Path(where) if where is not None else Path(tempfile.mkdtemp(prefix="bl_distill_"))  # a save location; nothing is written
    return load_model({"modelName": "gnn-mlp", "hidden_state_size": 32, "num_layers": 4}, where / "model.pkl.gz")[0]


def _marked(records):
    """location value -(node + 1), NO_BUG -0.5, rewrite i -(i + 1)"""
    out = []
    for r in copy.deepcopy(records):
        nodes = np.unique(r["graph"]["reference_nodes"]).tolist()
        r["teacher_location_nodes"] = nodes + [-1]
        r["teacher_location_logprobs"] = [-(float(n) + 1.0) for n in nodes] + [-0.5]
        r["teacher_rewrite_logprobs"] = [-(float(i) + 1.0) for i in range(len(r["candidate_rewrites"]))]
        out.append(r)
    return out


@pytest.fixture(scope="module")
def marked():
    from buglab.data.synthetic import make_buglab_dataset

    data = make_buglab_dataset(12, seed=31)
    model = _model()
    model.compute_metadata(copy.deepcopy(data))
    return model, data, _marked(data)


def _check_markers(mb, records, as_np=np.asarray):
    gd = mb["graph_data"]
    B = len(records)
    cand = as_np(gd["reference_node_ids"]["candidate_nodes"]).astype(np.int64)
    cptr = as_np(gd["candidate_ptr"]).astype(np.int64)
    node_off = np.concatenate([[0], np.cumsum(np.asarray(gd["num_nodes_per_graph"], np.int64))])
    tl, tr = as_np(mb["teacher_loc_logprobs"]), as_np(mb["teacher_repair_logprobs"])
    assert tl.dtype == np.float32 and tr.dtype == np.float32
    Cn = cand.shape[0]
    assert tl.shape == (Cn + B,)
    for b in range(B):
        own = cand[cptr[b]:cptr[b + 1]] - node_off[b]  # the candidate rows' node ids inside their own graph
        assert own.tolist() == np.unique(records[b]["graph"]["reference_nodes"]).tolist()
        assert tl[cptr[b]:cptr[b + 1]].tolist() == [-(float(n) + 1.0) for n in own]
        assert tl[Cn + b] == -0.5
    # every logit of cat(text, var, swap): its original rewrite index, and that rewrite sits at the logit's location
    fams = (("rewrite_to_location_group", "text_rewrite_original_idxs"), ("candidate_symbol_to_location_group", "candidate_rewrite_original_idxs"),
            ("swapped_pair_to_call_location_group", "pair_rewrite_original_idx"))
    at, seen = 0, 0
    for groups_key, orig_key in fams:
        groups = as_np(mb[groups_key]).astype(np.int64)
        k = 0
        for b in range(B):
            for i in mb[orig_key][b]:
                assert tr[at + k] == -(float(i) + 1.0), (groups_key, b, i)
                row = groups[k]  # location groups are numbered like the candidate rows
                assert cptr[b] <= row < cptr[b + 1] and cand[row] - node_off[b] == records[b]["graph"]["reference_nodes"][i]
                k += 1
        assert k == groups.shape[0]
        at += k
        seen += k
    assert tr.shape == (seen,) and seen > 0


def _minibatch(model, records):
    samples = [model.tensorize(copy.deepcopy(r)) for r in records]
    assert all(s is not None for s in samples)
    return samples, C.collate_samples(samples, model.gnn_model.num_presented_edge_types)


def test_teacher_values_sit_beside_their_items(marked):
    model, data, records = marked
    samples, mb = _minibatch(model, records)
    assert all(s.teacher_targets is not None and s.teacher_targets[0].dtype == np.float32 for s in samples)
    assert len(samples[0].teacher_targets[1]) == len(records[0]["candidate_rewrites"])
    _check_markers(mb, records)
    # rewrites at every location (what a selector or predict tensorises): the same rule
    with model._tensorize_all_location_rewrites():
        _, mb_all = _minibatch(model, records)
    assert mb_all["teacher_repair_logprobs"].shape[0] == sum(len(r["candidate_rewrites"]) for r in records)
    _check_markers(mb_all, records)
    # through the loader processes' path
    blob, meta = C.pack_minibatch(mb)
    pickle.loads(pickle.dumps(meta))
    up = C.upload_packed(blob, meta, "cpu")
    assert up["teacher_loc_logprobs"].dtype == torch.float32
    _check_markers(up, records, as_np=lambda t: t.numpy() if hasattr(t, "numpy") else np.asarray(t))


@pytest.mark.parametrize("native", [False, True])
def test_teacher_keys_survive_both_readers(marked, tmp_path, native):
    from buglab.data import native as N
    from buglab.utils.msgpackutils import load_msgpack_l_gz, save_msgpack_l_gz

    if native and not N.available():
        pytest.skip("the native reader is not built")
    model, data, records = marked
    save_msgpack_l_gz(records, tmp_path / "a.msgpack.l.gz")
    back = list(load_msgpack_l_gz(tmp_path / "a.msgpack.l.gz", native=native))
    assert len(back) == len(records)
    for r, b in zip(records, back):
        for k in ("teacher_location_nodes", "teacher_location_logprobs", "teacher_rewrite_logprobs"):
            assert list(b[k]) == r[k]
    if not native:  # the Python reader returns the graph as it was written (the native one appends the subtoken nodes)
        assert all(b["graph"]["nodes"] == r["graph"]["nodes"] for b, r in zip(back, records))
    samples = [model.tensorize(b) for b in back]
    mb = C.collate_samples(samples, model.gnn_model.num_presented_edge_types)
    _check_markers(mb, records)


def _same_blob(a, b, layout):
    """every array of the two blobs, bit for bit (the padding between them is whatever np.empty held)"""
    return all(a[o:o + int(np.prod(shape, dtype=np.int64))].tobytes() == b[o:o + int(np.prod(shape, dtype=np.int64))].tobytes()
               for _, _, shape, o in layout)


def test_nothing_changes_without_the_keys(marked):
    model, data, records = marked
    samples, mb = _minibatch(model, data)
    assert all(s.teacher_targets is None for s in samples)
    assert "teacher_loc_logprobs" not in mb and "teacher_repair_logprobs" not in mb
    # the parent's code path: the NamedTuple built from its fourteen fields, positionally
    parent_samples = [C.BaseTensorizedBugLabGnn(*tuple(s)[:14]) for s in samples]
    assert all(p.teacher_targets is None and len(p) == 15 for p in parent_samples)
    parent_mb = C.collate_samples(parent_samples, model.gnn_model.num_presented_edge_types)
    assert set(parent_mb) == set(mb)
    blob, meta = C.pack_minibatch(mb)
    pblob, pmeta = C.pack_minibatch(parent_mb)
    assert meta["layout"] == pmeta["layout"] and meta["total"] == pmeta["total"] and _same_blob(blob, pblob, meta["layout"])
    parent_meta_keys = {"layout", "total", "head_spans", "num_graphs", "num_nodes", "num_messages", "type_ptr_host", "num_nodes_per_graph",
                        "num_repair_groups", "num_hub_nodes", "original_idxs"}
    assert set(meta) == set(pmeta) == parent_meta_keys
    # and with them: the int32 blob and its layout are the same, only `meta` grows by the two arrays
    _, tmb = _minibatch(model, records)
    tblob, tmeta = C.pack_minibatch(tmb)
    assert tmeta["layout"] == meta["layout"] and tmeta["total"] == meta["total"] and _same_blob(tblob, blob, meta["layout"])
    assert set(tmeta) == parent_meta_keys | {"teacher_loc_logprobs", "teacher_repair_logprobs"}
    assert C.packed_size(tmb) == C.packed_size(mb)


def test_record_errors_name_the_mismatch(marked):
    model, data, records = marked
    good = [model.tensorize(copy.deepcopy(r)) for r in records[:3]]
    plain = model.tensorize(copy.deepcopy(data[3]))
    with pytest.raises(ValueError, match="3 of the minibatch's 4 samples"):
        C.collate_samples(good + [plain], model.gnn_model.num_presented_edge_types)
    r = copy.deepcopy(records[0])
    r["teacher_location_logprobs"] = r["teacher_location_logprobs"][:-1]
    with pytest.raises(ValueError, match=r"teacher_location_logprobs for \d+ teacher_location_nodes"):
        model.tensorize(r)
    r = copy.deepcopy(records[0])
    r["teacher_location_nodes"] = r["teacher_location_nodes"][:-1] + [r["teacher_location_nodes"][-2] + 1]  # NO_BUG replaced by a node
    with pytest.raises(ValueError, match=r"not the sample's candidate nodes \+ \[-1\]"):
        model.tensorize(r)
    r = copy.deepcopy(records[0])
    r["teacher_location_nodes"][0] += 1000
    with pytest.raises(ValueError, match="teacher_location_nodes"):
        model.tensorize(r)
    r = copy.deepcopy(records[0])
    r["teacher_rewrite_logprobs"] = r["teacher_rewrite_logprobs"] + [0.0]
    with pytest.raises(ValueError, match=r"teacher_rewrite_logprobs for \d+ candidate_rewrites"):
        model.tensorize(r)
    r = copy.deepcopy(records[0])
    del r["teacher_rewrite_logprobs"]
    with pytest.raises(ValueError, match="but not"):
        model.tensorize(r)


def test_sequence_students_ignore_the_keys(tmp_path):
    from buglab.data.synthetic import make_buglab_seq_dataset
    from buglab.models.modelregistry import load_model

    data = make_buglab_seq_dataset(4, seed=2)
    model = load_model({"modelName": "seq-great", "hidden_state_size": 32, "num_layers": 1, "num_heads": 4, "intermediate_dimension_size": 48},
                       tmp_path / "seq.pkl.gz")[0]
    model.compute_metadata(copy.deepcopy(data))
    plain = model.tensorize(copy.deepcopy(data[0]))
    annotated = model.tensorize(_marked(data[:1])[0])
    assert plain is not None and type(annotated) is type(plain)
    assert getattr(annotated, "teacher_targets", None) is None


# ---- switches -------------------------------------------------------------------------------------------------------------
def test_train_flags():
    from buglab.models import train

    base = ["gnn-mlp", "train", "valid", "m.pkl.gz"]
    args = train.parse_args(base)
    assert args["--distill-weight"] == "0" and args["--distill-temperature"] == "1"
    args = train.parse_args(base + ["--distill-weight", "0.5", "--distill-temperature=2"])
    assert args["--distill-weight"] == "0.5" and args["--distill-temperature"] == "2"
    assert "--distill-weight=<w>" in train.__doc__ and "--distill-temperature=<t>" in train.__doc__


def test_set_distillation_checks_and_is_not_pickled():
    from buglab.models.gnn import build_gnn_mlp_module

    m = build_gnn_mlp_module(32, 4, 3, 50)
    assert m.distillation == (0.0, 1.0)
    for w in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="weight"):
            m.set_distillation(w, 1.0)
    for t in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="temperature"):
            m.set_distillation(0.5, t)
    assert m.distillation == (0.0, 1.0)
    m.set_distillation(0.3, 2.0)
    assert m.distillation == (0.3, 2.0)
    back = pickle.loads(pickle.dumps(m))
    assert back.distillation == (0.0, 1.0) and m.distillation == (0.3, 2.0)
    m.set_distillation()
    assert m.distillation == (0.0, 1.0)
    assert "Teacher agreement" not in m.report_metrics()


def test_trainer_takes_the_setting(tmp_path):
    from buglab.runtime.trainer import ModelTrainer

    t = ModelTrainer(_model(tmp_path), tmp_path / "student.pkl.gz", distillation=(1.0, 2.0))
    assert t._distillation == (1.0, 2.0)
    assert ModelTrainer(_model(tmp_path), tmp_path / "student.pkl.gz")._distillation is None


def test_distill_cli_arguments_and_teacher_rule():
    from buglab.models import distill
    from buglab.models.greatreimplementation import GreatVarMisuse

    a = distill.parse_args(["teacher.pkl.gz", "data", "out", "--limit-num-elements", "7", "--sequential", "--report-json", "r.json"])
    assert (a.TEACHER_MODEL, a.DATA_PATH, a.OUT_DIR, a.limit_num_elements, a.sequential, a.report_json) == \
        ("teacher.pkl.gz", "data", "out", 7, True, "r.json")
    with pytest.raises(ValueError, match="GREAT var-misuse"):
        distill.require_teacher(GreatVarMisuse.__new__(GreatVarMisuse))


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    import ctypes

    from buglab.models import hip_ops

    assert {"bl_distill_fwd", "bl_distill_bwd", "bl_distill_workspace_bytes"} <= set(hip_ops.EXPORTED_SYMBOLS)
    lib = hip_ops.load_library()
    buf = (ctypes.c_double * 64)()
    P = ctypes.cast(buf, ctypes.c_void_p)
    err = lambda: lib.bl_last_error().decode()
    assert lib.bl_distill_workspace_bytes(3, 5) == 2 * 8 * 8 and lib.bl_distill_workspace_bytes(0, 0) == 16
    assert lib.bl_distill_workspace_bytes(-1, 0) == -1
    fwd = dict(loc_scores=P, logits=P, tl=P, tr=P, cptr=P, gptr=P, gitems=P, B=2, G=2, C=4, R=4, tau=1.0, ws=P, delta=P, out=P, stream=None)
    bad = lambda **kw: lib.bl_distill_fwd(*[kw.get(k, v) for k, v in fwd.items()])
    assert bad(tau=0.0) == -1 and "temperature" in err()
    assert bad(tau=float("nan")) == -1 and bad(tau=float("inf")) == -1
    assert bad(B=-1) == -1 and "negative" in err()
    assert bad(out=None) == -1 and "null out" in err()
    assert bad(cptr=None) == -1 and "candidate_ptr" in err()
    assert bad(gitems=None) == -1 and "repair_group_items" in err()
    assert bad(B=0) == -1 and "without a graph" in err()
    assert bad(G=0) == -1 and "without a group" in err()
    assert bad(C=1 << 31) == -2 and "int32" in err()
    bwd = dict(delta=P, C=4, R=4, g_loc=P, g_rep=P, tau=2.0, gs=P, gl=P, stream=None)
    badb = lambda **kw: lib.bl_distill_bwd(*[kw.get(k, v) for k, v in bwd.items()])
    assert badb(tau=-1.0) == -1 and "temperature" in err()
    assert badb(delta=None) == -1 and "null delta" in err()
    assert badb(gs=None) == -1 and "g_loc_scores" in err()
    assert badb(R=-4) == -1 and badb(C=1 << 31) == -2
    assert badb(C=0, R=0, delta=None, gs=None, gl=None) == 0  # nothing to do, nothing launched
