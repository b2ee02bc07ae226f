"""GPU: explanations on the MI355X -- the two kernels of csrc/bl_explain.hip against their NumPy twin
(buglab/models/_explain.py, which tests/test_explain_host.py pins to a literal restatement of the contract) bit for bit, their
offset writes into run-long buffers between poisoned guard regions, the gradient `input_gradients` returns against the fp64
oracle's, the independence of a minibatch's graphs, the integrated-gradients accumulation of the driver, and the public paths
end to end on two tiny untrained graph models: `explain`, its command line, `visualize --explain`.

The kernels' outputs carry no tolerance.  Gradients carry the project's own bar (tests/test_hip_parity.py): maxdiff <= 1e-4 *
max|G_ref| + 1e-6."""
import copy
import gzip
import json
from contextlib import contextmanager
from pathlib import Path

import numpy as np
import pytest
import torch

from buglab.models import _explain as E
from tests import explain_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = 1e-4  # tests/test_hip_parity.py: forward values against the oracle
SPECS = {"gnn-mlp": {"modelName": "gnn-mlp", "hidden_state_size": 32, "num_layers": 4, "dropout_rate": 0.1},
         "ggnn": {"modelName": "ggnn", "hidden_state_size": 32, "dropout_rate": 0.1}}


def _grad_bar(got, ref):
    ref = torch.as_tensor(ref).detach().cpu().double()
    d = float((torch.as_tensor(got).detach().cpu().double() - ref).abs().max())
    scale = float(ref.abs().max())
    print(f"gradient maxdiff {d:.3e} at scale {scale:.3e} (bar {1e-4 * scale + 1e-6:.3e})")
    return d <= 1e-4 * scale + 1e-6, (d, scale)


@contextmanager
def _deterministic():
    from buglab.models import hip_ops

    was = bool(hip_ops.load_library().bl_get_deterministic())
    hip_ops.set_deterministic(True)
    try:
        yield
    finally:
        hip_ops.set_deterministic(was)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _scores(x, g, score=None, weight=1.0, accumulate=False):
    from buglab.models import hip_ops

    if score is None:
        score = torch.full((x.shape[0],), 123.0, dtype=torch.float64, device=DEV)
    hip_ops.attribute_node_scores(x, g, score, weight=weight, accumulate=accumulate)
    return score


def _topk_buffers(capacity, k):
    return (torch.full((capacity, k), 77, dtype=torch.int32, device=DEV), torch.full((capacity, k), 123.0, dtype=torch.float64, device=DEV),
            torch.full((2, capacity), 123.0, dtype=torch.float64, device=DEV))


def _topk(score, off, k, by_abs=True, into=None, offset=0):
    from buglab.models import hip_ops

    out = into if into is not None else _topk_buffers(off.shape[0] - 1, k)
    hip_ops.attribute_topk(score, off, *out, offset, k=k, by_abs=by_abs)
    return out


def _host(out):
    return tuple(t.cpu().numpy() for t in out)


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the kernels against the twin, bit for bit
def _strided(a, pad, shift):
    """the same values as a view with row stride D + pad whose base is `shift` floats into an allocation"""
    N, D = a.shape
    flat = torch.full((shift + N * (D + pad) + 8,), 7.0, dtype=torch.float32, device=DEV)
    view = flat[shift:shift + N * (D + pad)].view(N, D + pad)[:, :D]
    view.copy_(_dev(a))
    return view


@pytest.mark.parametrize("D", C.WIDTHS)
def test_node_scores_equal_the_twin_bit_for_bit(D):
    pairs = [C.operands(D, seed=s) for s in range(3)]
    x, g = pairs[0]
    want = E.node_scores_host(x, g)
    first = _scores(_dev(x), _dev(g)).cpu().numpy()
    assert first.tobytes() == want.tobytes(), np.argwhere(first != want)[:5]
    assert _scores(_dev(x), _dev(g)).cpu().numpy().tobytes() == first.tobytes()  # the same launch twice: identical bytes
    # row stride above D (a multiple of 4 and not: the 16-byte loads and the scalar ones), and a base that is not 16-byte aligned
    for pad, shift in ((4 - D % 4 if D % 4 else 4, 0), (5, 0), (3, 1), (4 - D % 4 if D % 4 else 4, 3)):
        xs, gs = _strided(x, pad, shift), _strided(g, pad, shift)
        assert xs.stride(0) == D + pad and xs.data_ptr() % 16 == (4 * shift) % 16
        assert _scores(xs, gs).cpu().numpy().tobytes() == want.tobytes(), (pad, shift)
    assert _scores(_strided(x, 5, 1), _dev(g)).cpu().numpy().tobytes() == want.tobytes()  # only one operand off the fast path
    # the steps of a path: three calls with weights 1/3
    third, acc, want3 = 1.0 / 3, None, None
    for i, (a, b) in enumerate(pairs):
        acc = _scores(_dev(a), _dev(b), acc, weight=third, accumulate=i > 0)
        want3 = E.node_scores_host(a, b, want3, third)
    assert acc.cpu().numpy().tobytes() == want3.tobytes()


def test_node_scores_at_the_models_widths_and_many_nodes():
    rng = np.random.default_rng(5)
    x, g = rng.standard_normal((1003, 128)).astype(np.float32), rng.standard_normal((1003, 128)).astype(np.float32)
    assert _scores(_dev(x), _dev(g)).cpu().numpy().tobytes() == E.node_scores_host(x, g).tobytes()
    empty = torch.zeros((0, 16), dtype=torch.float32, device=DEV)
    assert _scores(empty, empty).shape == (0,)  # N = 0: a no-op


@pytest.mark.parametrize("by_abs", [True, False])
@pytest.mark.parametrize("k", [1, 5, 32])
def test_topk_equals_the_twin_bit_for_bit(k, by_abs):
    score, off, at = C.handmade()
    got = _host(_topk(_dev(score), _dev(off), k, by_abs))
    C.assert_equal_bits(got, E.topk_host(score, off, k, by_abs), ("handmade", k, by_abs))
    tie = got[0][at["tie_waves"]].tolist()
    assert tie[:min(k, 3)] == [63, 64, 256][:k] if by_abs else tie[:min(k, 2)] == [64, 256][:k]  # the tie across waves, in index order
    assert (got[0][at["all_nan"]] == -1).all() and np.isnan(got[2][:, at["one_nan"]]).all()
    score, off = C.drawn(3, B=50)
    first = _host(_topk(_dev(score), _dev(off), k, by_abs))
    C.assert_equal_bits(first, E.topk_host(score, off, k, by_abs), ("drawn", k, by_abs))
    again = _host(_topk(_dev(score), _dev(off), k, by_abs))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))  # the same launch twice: identical bytes


# ------------------------------------------------------------------------------------------------------------------------------
# 2. offsets and guard regions
def test_offsets_and_guard_regions():
    """two launches at offsets 0 and B fill one buffer; what lies before and after it keeps its poison"""
    from buglab.models import hip_ops

    score, off, _ = C.handmade()
    B = off.shape[0] - 1
    score2, off2 = C.drawn(4, B=B)
    k, guard, N = 5, 512, 2 * B
    flats = (torch.full((2 * guard + N * k,), 77, dtype=torch.int32, device=DEV), torch.full((2 * guard + N * k,), 123.0, dtype=torch.float64, device=DEV),
             torch.full((2 * guard + 2 * N,), 123.0, dtype=torch.float64, device=DEV))
    out = (flats[0][guard:guard + N * k].view(N, k), flats[1][guard:guard + N * k].view(N, k), flats[2][guard:guard + 2 * N].view(2, N))
    d_score, d_off = _dev(score), _dev(off)
    _topk(d_score, d_off, k, into=out, offset=0)
    _topk(_dev(score2), _dev(off2), k, by_abs=False, into=out, offset=B)
    node, picked, sums = _host(out)
    C.assert_equal_bits((node[:B], picked[:B], sums[:, :B]), E.topk_host(score, off, k), "offset 0")
    C.assert_equal_bits((node[B:], picked[B:], sums[:, B:]), E.topk_host(score2, off2, k, by_abs=False), "offset B")
    for flat, size, poison in zip(flats, (N * k, N * k, 2 * N), (77, 123.0, 123.0)):
        host = flat.cpu().numpy()
        assert (host[:guard] == poison).all() and (host[guard + size:] == poison).all()
    # `score` likewise: N values between poisoned regions
    x, g = C.operands(65)
    flat = torch.full((2 * guard + x.shape[0],), 123.0, dtype=torch.float64, device=DEV)
    _scores(_dev(x), _dev(g), flat[guard:guard + x.shape[0]])
    host = flat.cpu().numpy()
    assert (host[:guard] == 123.0).all() and (host[guard + x.shape[0]:] == 123.0).all()
    assert host[guard:guard + x.shape[0]].tobytes() == E.node_scores_host(x, g).tobytes()
    # what does not fit, k = 33 and inconsistent shapes are refused before anything is written
    before = [t.clone() for t in out] + [flat.clone()]
    with pytest.raises(ValueError, match="do not fit"):
        _topk(d_score, d_off, k, into=out, offset=B + 1)
    with pytest.raises(ValueError, match="k must be"):
        hip_ops.attribute_topk(d_score, d_off, *_topk_buffers(B, 33), 0, k=33)
    with pytest.raises(ValueError, match="inconsistent shapes"):
        hip_ops.attribute_topk(d_score, d_off, out[0], torch.empty((N, k - 1), dtype=torch.float64, device=DEV), out[2], 0, k=k)
    with pytest.raises(ValueError, match="inconsistent shapes"):
        hip_ops.attribute_topk(d_score.view(1, -1), d_off, *out, 0, k=k)
    dx, dg = _dev(x), _dev(g)
    with pytest.raises(ValueError, match="inconsistent shapes"):
        hip_ops.attribute_node_scores(dx, dg[:, :64], flat[guard:guard + x.shape[0]])
    with pytest.raises(ValueError, match="inconsistent shapes"):
        hip_ops.attribute_node_scores(dx, dg, flat[guard:guard + x.shape[0] + 1])
    with pytest.raises(ValueError, match="contiguous rows"):
        hip_ops.attribute_node_scores(dx.t(), dg.t(), flat[guard:guard + 65])
    with pytest.raises(ValueError, match="ROCm GPU"):
        hip_ops.attribute_node_scores(dx.cpu(), dg, flat[guard:guard + x.shape[0]])
    assert all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(before, list(out) + [flat]))  # (bytes: the sums hold NaNs)


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the gradient is the right gradient
def test_input_gradients_match_the_fp64_oracle():
    from buglab.data.collate import to_device
    from buglab.models import hip_ops
    from oracle import buglab_oracle as O
    from tests import helpers as Hh

    cfg, _, mb_np = Hh.make_case(B=3, n=60, E=300, T=4, H=64, layers=4)
    params = O.init_params(cfg, seed=0)
    module = Hh.build_module_like(cfg, params).eval()
    named = dict(module.named_parameters())
    frozen_before = named["_gnn.mp.0.ln_b"]
    frozen_before.requires_grad_(False)              # a flag that is off stays off
    bound = named["_gnn.mp.1.Wd"]                     # a .grad an optimiser bound for direct accumulation stays that tensor, untouched
    bound.grad, bound._bl_direct_grad = torch.zeros_like(bound), True
    bound_grad = bound.grad
    flags = {k: p.requires_grad for k, p in named.items()}
    mb = to_device(mb_np, DEV)
    B = 3
    with torch.no_grad():
        _, loc_lp, _, _ = module.compute_localization_logprobs(mb["graph_data"])
    loc = loc_lp.cpu().numpy()
    sample = np.concatenate([np.asarray(mb_np["graph_data"]["reference_node_graph_idx"]["candidate_nodes"], dtype=np.int64), np.arange(B)])
    assert sample.shape == loc.shape
    idx = [int(np.flatnonzero(sample == b)[np.argmax(loc[sample == b])]) for b in range(B)]  # the predicted location's flat entry
    chosen = torch.tensor([[i, -1] for i in idx], dtype=torch.int32, device=DEV)
    hip_ops.WINNER_SINK = []
    try:
        x, G, objective = E.input_gradients(module, mb, chosen)
        winners = [w.cpu().numpy().astype(np.int64) for w in hip_ops.WINNER_SINK]
    finally:
        hip_ops.WINNER_SINK = None
    assert len(winners) == cfg.num_layers and x.shape == G.shape == (180, 64) and objective.dtype == torch.float64
    n_msgs = int(mb_np["graph_data"]["msg_src"].shape[0])
    forced = [np.where(w < 0, n_msgs, w) for w in winners]  # the oracle differentiates the function the HIP path routed
    p64 = {k: v.double().requires_grad_() for k, v in params.items()}
    trace = []
    with torch.enable_grad():
        out = O.forward_loss(p64, mb_np, cfg, trace=trace, force_arg=forced)
        (G_ref,) = torch.autograd.grad(out["loc_logprobs"][idx].sum(), trace[0]["embed"])
    assert Hh.maxdiff(x, trace[0]["embed"]) < TOL
    assert Hh.maxdiff(objective, out["loc_logprobs"][idx]) < TOL
    ok, figures = _grad_bar(G, G_ref)
    assert ok, figures
    assert float(G_ref.abs().max()) > 1e-3  # (a gradient that is there to be compared)
    # the device scores from this x and G equal the twin's bit for bit
    assert _scores(x, G).cpu().numpy().tobytes() == E.node_scores_host(x.cpu().numpy(), G.cpu().numpy()).tobytes()
    # nothing of the model was touched
    assert {k: p.requires_grad for k, p in named.items()} == flags and not frozen_before.requires_grad
    assert bound.grad is bound_grad and not bound.grad.any()
    assert all(p.grad is None for k, p in named.items() if p is not bound)
    # ... also when the run raises
    with pytest.raises(AttributeError):
        E.input_gradients(module, mb, None)  # (fails after the forward, inside the frozen region)
    assert {k: p.requires_grad for k, p in named.items()} == flags and bound.grad is bound_grad


# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def untrained(tmp_path_factory):
    """family -> (model, module, data, path): seeded weights, no training; 60 synthetic samples = two predict minibatches"""
    from buglab.data.synthetic import make_report_dataset
    from buglab.models.modelregistry import load_model
    from buglab.runtime.neuralmodel import AbstractNeuralModel

    out = {}
    for family, spec in SPECS.items():
        data = make_report_dataset(60, seed=17, kind="graph")
        path = tmp_path_factory.mktemp(family.replace("-", "_")) / "detector.pkl.gz"
        model = load_model(dict(spec), path)[0]
        model.compute_metadata(copy.deepcopy(data))
        torch.manual_seed(5)
        model.save(path, model.build_neural_module())
        out[family] = AbstractNeuralModel.restore_model(Path(path), torch.device(DEV)) + (data, path)
    return out


def _minibatches(model, data):
    """the predict minibatches of `data` with their suggest / explain index arrays, as the driver builds them"""
    from buglab.controllers import _batching as Bt
    from buglab.models import _suggest as S

    def extend(layout, points, dev, mb):
        six = S.suggest_indices(layout, points, mb.get("node_mappings"))
        return {"six": six, "eix": E.explain_indices(mb["graph_data"]["num_nodes_per_graph"], int(mb["graph_data"]["num_nodes"]), six, points)}

    with torch.no_grad(), model._tensorize_all_location_rewrites():
        return [mb for mb, _ in Bt.prediction_minibatches(model, ((d, i) for i, d in enumerate(data)), torch.device(DEV), False, extend,
                                                          lambda tag: None, extend_sees_minibatch=True)]


def _predicted_location_entries(nn_, mb):
    """per graph: (its place among the graph's location entries, the flat index) of the most probable location"""
    with torch.no_grad():
        flat = E.flat_output(nn_, mb).cpu().numpy()
    six = mb["selfsup"]["six"]
    out = []
    for b in range(six.nobug_idx.shape[0]):
        entries = six.loc_idx[six.loc_off[b]:six.loc_off[b + 1]]
        place = int(np.argmax(flat[entries]))
        out.append((place, int(entries[place])))
    return out


def test_chosen_entries_on_the_device_are_the_host_rule(untrained):
    """the driver's device ops against _explain.chosen_flat_indices: a rewrite, NO_BUG, nothing, and an entry past the sample's"""
    from buglab.controllers._batching import to_device_i32
    from buglab.models.explain import _chosen_on_device

    model, _, data, _ = untrained["gnn-mlp"]
    mb = _minibatches(model, data[:20])[0]
    eix = mb["selfsup"]["eix"]
    n_rw = np.diff(eix.rw_off)
    assert (n_rw > 0).any()
    fields = ("rw_idx", "rw_loc_idx", "rw_off", "nobug_idx")
    ix = dict(zip(fields, to_device_i32([getattr(eix, f) for f in fields], DEV)))
    for entry in (np.zeros(20, np.int64), n_rw, np.maximum(n_rw - 1, 0), np.full(20, -1), np.arange(20) % 3 - 1):
        got = _chosen_on_device(torch.from_numpy(np.asarray(entry, np.int32)).to(DEV), ix).cpu().numpy()
        assert got.dtype == np.int32 and np.array_equal(got, E.chosen_flat_indices(entry, eix)), entry
    empty = dict(ix, rw_idx=ix["rw_idx"][:0], rw_loc_idx=ix["rw_loc_idx"][:0], rw_off=torch.zeros_like(ix["rw_off"]))
    got = _chosen_on_device(torch.tensor([0, -1] * 10, dtype=torch.int32, device=DEV), empty).cpu().numpy()  # a minibatch without rewrites
    assert np.array_equal(got[:, 0], np.where(np.arange(20) % 2 == 0, eix.nobug_idx, -1)) and (got[:, 1] == -1).all()


# 4. one backward serves every graph
def test_one_backward_serves_every_graph(untrained):
    model, nn_, data, _ = untrained["gnn-mlp"]
    which = 7
    both = _minibatches(model, data)
    alone = _minibatches(model, [data[which]])
    assert len(both) == 2 and both[0]["selfsup"]["six"].nobug_idx.shape[0] == 50 and len(alone) == 1
    picks = _predicted_location_entries(nn_, both[0])
    chosen = torch.tensor([[flat_index, -1] for _, flat_index in picks], dtype=torch.int32, device=DEV)
    _, G_all, f_all = E.input_gradients(nn_, both[0], chosen)
    six = alone[0]["selfsup"]["six"]
    same_place = int(six.loc_idx[six.loc_off[0]:six.loc_off[1]][picks[which][0]])  # the same location entry, in the minibatch of one
    x_one, G_one, f_one = E.input_gradients(nn_, alone[0], torch.tensor([[same_place, -1]], dtype=torch.int32, device=DEV))
    off = both[0]["selfsup"]["eix"].node_off
    rows = G_all[int(off[which]):int(off[which + 1])]
    assert rows.shape == G_one.shape and abs(float(f_all[which]) - float(f_one[0])) < TOL
    ok, figures = _grad_bar(rows, G_one)  # only rounding couples the graphs: the gradient operand's tensor scale is batch-wide
    assert ok, figures
    assert float(G_one.abs().max()) > 0
    # a graph whose entry is absent gets no gradient at all
    chosen[3] = -1
    _, G_without, f_without = E.input_gradients(nn_, both[0], chosen)
    assert not G_without[int(off[3]):int(off[4])].any() and float(f_without[3]) == 0.0


# ------------------------------------------------------------------------------------------------------------------------------
# 5. integrated gradients plumbing
def test_integrated_gradients_accumulation_is_the_twins(untrained, monkeypatch):
    from buglab.models.explain import explain

    model, nn_, data, _ = untrained["gnn-mlp"]
    few = data[:10]
    recorded, inputs = [], []
    original = E.input_gradients

    def recording(nn, mb, flat_indices, alpha=1.0):
        x, G, objective = original(nn, mb, flat_indices, alpha)
        recorded.append((alpha, x.cpu().numpy().copy(), G.cpu().numpy().copy()))
        return x, G, objective

    monkeypatch.setattr(E, "input_gradients", recording)
    first_layer = nn_._gnn.mp[0]
    hook = first_layer.register_forward_pre_hook(lambda mod, args: inputs.append((args[0][0] if isinstance(args[0], tuple) else args[0]).detach().clone()))
    try:
        with _deterministic():
            records = [x.record() for x in explain(model, nn_, few, DEV, 32, steps=4, parallelize=False)]
    finally:
        hook.remove()
    assert [a for a, _, _ in recorded] == [0.125, 0.375, 0.625, 0.875]  # alpha_m = (m - 1/2) / 4
    x = recorded[0][1]
    assert all(r[1].tobytes() == x.tobytes() for r in recorded)
    # the forwards of the run: the ranking one at x, the four steps at alpha_m x exactly, the baseline at 0 x
    assert len(inputs) == 6 and inputs[0].cpu().numpy().tobytes() == x.tobytes() and not inputs[5].any()
    for (alpha, _, _), seen in zip(recorded, inputs[1:5]):
        assert torch.equal(seen, alpha * torch.from_numpy(x).to(DEV))
    score = None
    for _, _, G in recorded:
        score = E.node_scores_host(x, G, score, 0.25)
    off = np.concatenate([[0], np.cumsum([len(p["graph"]["nodes"]) for p in few])])
    assert off[-1] == x.shape[0]
    node, picked, sums = E.topk_host(score, off, 32)
    for b, r in enumerate(records):
        assert r["position"] == b and r["steps"] == 4 and r["explained"] is not None
        listed = int((node[b] >= 0).sum())
        assert [a["node"] for a in r["attributions"]] == node[b, :listed].tolist()
        assert np.asarray([a["score"] for a in r["attributions"]]).tobytes() == picked[b, :listed].tobytes()
        assert np.float64(r["sum"]).tobytes() == sums[0, b].tobytes() and np.float64(r["abs_sum"]).tobytes() == sums[1, b].tobytes()
        assert all(np.isfinite(r[name]) for name in ("sum", "objective", "baseline"))
        print(f"sample {b}: completeness gap {r['sum'] - (r['objective'] - r['baseline']):+.4e} (objective {r['objective']:.4f}, baseline {r['baseline']:.4f})")


# ------------------------------------------------------------------------------------------------------------------------------
# 6. end to end
def _check_records(records, data, k, signed=False):
    assert [r["position"] for r in records] == list(range(len(data)))
    for r, point in zip(records, data):
        nodes = point["graph"]["nodes"]
        got = r["attributions"]
        assert r["explained"] is not None and 0 < len(got) <= k
        assert all(0 <= a["node"] < len(nodes) and a["label"] == nodes[a["node"]] and a["kind"] in ("token", "subtoken", "other") for a in got)
        keys = [(a["score"] if signed else abs(a["score"]), a["node"]) for a in got]
        assert all(p[0] > q[0] or (p[0] == q[0] and p[1] < q[1]) for p, q in zip(keys, keys[1:]))
        assert sum(a["share"] for a in got) <= 1 + 1e-12 and all(a["share"] == abs(a["score"]) / r["abs_sum"] for a in got if r["abs_sum"] > 0)
        assert np.isfinite(r["objective"]) and "baseline" not in r and r["steps"] == 1


@pytest.mark.parametrize("family", list(SPECS))
def test_explain_end_to_end(family, untrained):
    from buglab.models.explain import explain
    from buglab.models.suggest import suggest

    model, nn_, data, _ = untrained[family]
    device = torch.device(DEV)
    grads_before = [p.grad for p in nn_.parameters()]
    flags_before = [p.requires_grad for p in nn_.parameters()]
    suggested = [s.record() for s in suggest(model, nn_, data, device, 5, parallelize=False)]
    by_rank = {}
    for rank in (0, 1):
        found = list(explain(model, nn_, data, device, 10, rank=rank, parallelize=False))
        assert len(found) == 60 and [x.position for x in found] == list(range(60)) and all(x.datapoint is d for x, d in zip(found, data))
        by_rank[rank] = records = [x.record() for x in found]
        _check_records(records, data, 10)
        for r, s in zip(records, suggested):
            assert len(s["suggestions"]) > rank and r["explained"] == s["suggestions"][rank]
            assert r["objective"] == r["explained"]["logprob"]  # no calibration here: the objective is the ranked joint log-probability
    assert any(a["explained"] != b["explained"] for a, b in zip(by_rank[0], by_rank[1]))
    assert all(p.grad is g for p, g in zip(nn_.parameters(), grads_before)) and [p.requires_grad for p in nn_.parameters()] == flags_before
    # signed order, NO_BUG left out, the host path (the twin on copied arrays), a rank nobody has
    with _deterministic():
        signed = [x.record() for x in explain(model, nn_, data, device, 10, signed=True, parallelize=False)]
        _check_records(signed, data, 10, signed=True)
        plain = [x.record() for x in explain(model, nn_, data, device, 10, parallelize=False)]
        again = [x.record() for x in explain(model, nn_, data, device, 10, parallelize=False)]
        assert json.dumps(plain, sort_keys=True) == json.dumps(again, sort_keys=True)  # two runs: identical records
        # a stream of unknown length, collated in worker threads: the buffers grow on the device
        streamed = [x.record() for x in explain(model, nn_, iter(data), device, 10, parallelize=True, capacity=1)]
        assert json.dumps(streamed, sort_keys=True) == json.dumps(plain, sort_keys=True)
        on_host = [x.record() for x in explain(model, nn_, data, device, 10, host=True, parallelize=False)]
        assert json.dumps(on_host, sort_keys=True) == json.dumps(plain, sort_keys=True)
    assert [r["explained"] for r in signed] == [r["explained"] for r in by_rank[0]]
    buggy = [x.record() for x in explain(model, nn_, data[:12], device, 3, assume_buggy=True, parallelize=False)]
    assert all(r["explained"]["kind"] == "rewrite" and len(r["attributions"]) <= 3 for r in buggy)
    nobody = [x.record() for x in explain(model, nn_, data[:12], device, 3, rank=31, parallelize=False)]
    assert all(r == {"position": i, "explained": None, "steps": 1, "attributions": []} for i, r in enumerate(nobody))


def test_command_line_writes_the_records(untrained, tmp_path, capsys):
    from buglab.models import explain as T
    from buglab.utils.msgpackutils import load_all_msgpack_l_gz, save_msgpack_l_gz

    model, nn_, data, path = untrained["gnn-mlp"]
    folder = tmp_path / "shard"
    folder.mkdir()
    save_msgpack_l_gz(data, folder / "x.msgpack.l.gz")
    out = tmp_path / "explanations.jsonl.gz"
    arguments = {"MODEL_FILENAME": str(path), "DATA_PATH": str(folder), "OUT_PATH": str(out), "--top-k": 4, "--steps": 2, "--rank": 0,
                 "--signed": False, "--assume-buggy": False, "--limit-num-elements": None, "--sequential": True, "--host": False}
    with _deterministic():
        assert T.run(arguments) == 60
        assert "60 samples explained, 0 rejected" in capsys.readouterr().err
        read_back = list(load_all_msgpack_l_gz(folder))  # the samples as the tool reads them
        want = [x.record() for x in T.explain(model, nn_, read_back, DEV, 4, steps=2, parallelize=False)]
    with gzip.open(out, "rt", encoding="utf-8") as f:
        records = [json.loads(line) for line in f]
    assert records == json.loads(json.dumps(want)) and [r["position"] for r in records] == list(range(60))
    assert all(len(r["attributions"]) <= 4 and r["steps"] == 2 and "baseline" in r for r in records)


# ------------------------------------------------------------------------------------------------------------------------------
# 7. visualize --explain
def test_visualize_with_explain_adds_influences_and_nothing_else(untrained):
    from buglab.models.visualize import report_to_html, report_to_json, scan

    model, nn_, data, _ = untrained["gnn-mlp"]
    plain = scan(model, nn_, iter(data), DEV, order_by_confidence=True, show_top_k=6)
    shown = scan(model, nn_, iter(data), DEV, order_by_confidence=True, show_top_k=6, explain=3)
    assert len(plain.snippets) == len(shown.snippets) == 6 and plain.selected.tolist() == shown.selected.tolist()
    assert all("influences" not in ctx for ctx in plain.snippets)
    for ctx, o in zip(shown.snippets, shown.selected.tolist()):
        influences = ctx["influences"]
        assert 0 < len(influences) <= 3 and all(set(i) == {"label", "kind", "share"} and 0 <= i["share"] <= 1 for i in influences)
        assert all(i["label"] in data[o]["graph"]["nodes"] for i in influences)
    # without the flag: today's contexts, page and data, byte for byte
    stripped = [{name: value for name, value in ctx.items() if name != "influences"} for ctx in shown.snippets]
    assert json.dumps(stripped, sort_keys=True) == json.dumps(plain.snippets, sort_keys=True)
    page, page_explained = report_to_html(plain.snippets), report_to_html(shown.snippets)
    assert "influenced by" not in page and page_explained.count("influenced by: ") == 6
    assert "\n".join(line for line in page_explained.split("\n") if "influenced by: " not in line) == page
    assert report_to_html(stripped) == page and report_to_json(plain._replace(snippets=stripped)) == report_to_json(plain)
    assert "influences" in report_to_json(shown) and "influences" not in report_to_json(plain)
